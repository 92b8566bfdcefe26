"""Multiscale Hessian vesselness (DESIGN.md section 9 entry f7): the float64 model tests/vesselness_model.py is checked on the
CPU (explicit taps against scipy, known answers), then vmask_vesselness / vesselness.vesselnessFilter must agree with it to
1e-9 absolute outside the tie set, the measure's one discontinuity."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vesselness_model as M
from conftest import ROOT
from test_mask_stage import _volumes
from arterynetwork_amd import vesselness as VS
from arterynetwork_amd._capi import VrgError

SIGMAS = (0.6, 1.0, 2.5)                                # radii 2, 4 and 10 at unit spacing
BAR = 1e-9                                              # the project's bar for float64 quantities against their oracle; V lies in [0, 1]
TIE_CAP = 1e-3                                          # of a case's voxels


def _input(seed, shape):
    """The sinusoid tube of the stage-1 tests scaled to 100, Gaussian noise of sigma 10 on every voxel; and the brain mask."""
    brain, ves = _volumes(seed, shape)
    noise = np.random.default_rng(1000 + seed).normal(0.0, 10.0, shape)
    return 100.0 * ves.astype(np.float64) + noise, brain


# ------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize('sigma', [0.8, 1.5, 2.5])
def test_model_explicit_taps_equal_scipy(sigma):
    I, _ = _input(1, (20, 18, 16))
    for spacing in ((1.0, 1.0, 1.0), (1.0, 1.0, 2.0)):
        for order in M.ORDERS.values():
            a, b = M.derivative_explicit(I, sigma, spacing, order), M.derivative_scipy(I, sigma, spacing, order)
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    r, phi, d1, d2 = M.taps(2.5)
    assert r == 10 and len(phi) == 21 and abs(phi.sum() - 1) < 1e-15 and phi[3] == phi[-4] and d1[3] == -d1[-4] > 0


def test_model_extent_below_radius():
    """Clamped indices: a radius larger than the extent is legal (scipy's mode='nearest' and the explicit taps agree)."""
    I, _ = _input(2, (2, 5, 3))
    for order in M.ORDERS.values():
        a, b = M.derivative_explicit(I, 2.5, (1, 1, 1), order), M.derivative_scipy(I, 2.5, (1, 1, 1), order)
        assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max())


def test_model_known_answers():
    zero = M.vesselness(np.zeros((9, 8, 7)), SIGMAS)                       # automatic gamma: every gamma is 0, every scale gives 0
    assert not zero['V'].any() and not zero['scale'].any() and not zero['gammas'].any()
    # any other constant c: the truncated, sampled second-derivative taps do not sum to 0 (their sum k is negative: the window
    # cuts variance off), so H = c sigma^2 k I everywhere, three equal eigenvalues - a small blob response, known in closed form
    const = M.vesselness(np.full((9, 8, 7), 7.0), SIGMAS, gamma=5.0)
    lam = [7.0 * s * s * M.taps(s)[3].sum() for s in SIGMAS]
    assert all(-0.5 < l < 0 for l in lam)
    expect = max((1 - np.exp(-2.0)) * np.exp(-2.0) * (1 - np.exp(-3 * l * l / 50.0)) for l in lam)
    assert np.abs(const['V'] - expect).max() < 1e-12 and expect < 1e-3
    s = 2.0
    for axis in range(3):
        line = M.gaussian_line((25, 25, 25), axis, s)
        lam = M.sorted_eigenvalues(M.hessian(line, s))[12, 12, 12]
        # along the line the volume is constant: l1 is the smoothed amplitude (<= 100) times the taps' sum again - 0 for the measure
        assert abs(lam[0]) <= 100.0 * s * s * abs(M.taps(s)[3].sum()) and abs(lam[0]) < 1e-3 * abs(lam[2])
        assert lam[1] < -1.0 and abs(lam[1] - lam[2]) < 1e-9 * abs(lam[2])
        assert abs(lam[2] + 100.0 / 4) < 0.5                                 # -A s^2 sigma^2 / (s^2 + sigma^2)^2 at sigma = s, sampled
        res = M.vesselness(line, (s / 2, s, 2 * s), gamma=10.0)
        at = res['per_scale'][:, 12, 12, 12]
        assert at[1] > at[0] and at[1] > at[2] and res['scale'][12, 12, 12] == 1
        assert res['V'][12, 12, 12] > 0.8                                    # (1 - e^-2) (1 - e^-6.25)


def test_model_symmetries():
    I, brain = _input(3, (20, 18, 16))
    a = M.vesselness(I, SIGMAS, mask=brain)
    dark = M.vesselness(-I, SIGMAS, mask=brain, bright=False)
    assert np.abs(a['V'] - dark['V']).max() < 1e-12 and a['V'].max() > 0.3
    tripled = M.vesselness(3.0 * I, SIGMAS, mask=brain)                      # automatic gamma scales with the volume
    assert np.abs(a['V'] - tripled['V'])[~a['ties']].max() < 1e-12
    assert np.allclose(tripled['gammas'], 3.0 * a['gammas'], rtol=1e-13)
    assert not a['V'][brain == 0].any() and a['V'].min() >= 0 and a['V'].max() <= 1


def test_sigmas_from_diameters():
    s = VS.sigmasFromDiameters(1.0, 8.0, 4)
    assert np.allclose(s, [0.5, 1.0, 2.0, 4.0])
    assert np.allclose(VS.sigmasFromDiameters(3.0, 9.0, 1), [1.5])
    assert np.allclose(VS.sigmasFromDiameters(2.0, 2.0, 3), [1.0, 1.0, 1.0])
    for bad in ((0.0, 1.0, 3), (2.0, 1.0, 3), (1.0, 2.0, 0), (1.0, float('inf'), 2)):
        with pytest.raises(ValueError):
            VS.sigmasFromDiameters(*bad)


def test_argument_errors_raise():
    """Wrong arguments are refused before a device is looked for: no GPU needed."""
    I = np.zeros((6, 5, 4))
    with pytest.raises(ValueError):
        VS.vesselnessFilter(np.zeros((6, 5)), SIGMAS)
    with pytest.raises(ValueError):
        VS.vesselnessFilter(np.zeros((2, 6, 5, 4)), SIGMAS)
    with pytest.raises(ValueError):
        VS.vesselnessFilter(I, SIGMAS, brainVolumeMask=np.ones((6, 5, 5)))
    with pytest.raises(ValueError):
        VS.vesselnessFilter(I, SIGMAS, spacing=(1.0, 1.0))
    with pytest.raises(ValueError):
        VS.vesselnessFilter(I, [])
    bad = [dict(sigmas=[1.0] * 33), dict(sigmas=[1.0, -1.0]), dict(sigmas=[float('nan')]), dict(sigmas=[float('inf')]),
           dict(sigmas=[0.1]),                               # radius int(0.9) = 0
           dict(sigmas=[16.2]),                              # radius 65
           dict(sigmas=[1.0], spacing=(1.0, 1.0, 9.0)),      # radius int(0.94) = 0 on axis 2
           dict(sigmas=[1.0], spacing=(1.0, 0.0, 1.0)), dict(sigmas=[1.0], spacing=(1.0, float('nan'), 1.0)),
           dict(sigmas=[1.0], alpha=0.0), dict(sigmas=[1.0], alpha=float('inf')), dict(sigmas=[1.0], beta=-0.5), dict(sigmas=[1.0], beta=float('nan'))]
    for kw in bad:
        with pytest.raises(VrgError) as e:
            VS.vesselnessFilter(I, **kw)
        assert e.value.code == -1, kw                        # VRG_E_ARG
    with pytest.raises(VrgError) as e:                       # the shape envelope of the other voxel passes
        VS._G._check(VS._lib().vmask_vesselness(0, I.ctypes.data, 6, 2000, 2000, 600, None, np.ones(1).ctypes.data, 1, None, 0.5, 0.5, 0.0, 1, I.ctypes.data, None, None))
    assert e.value.code == -1 and 'shape' in str(e.value)


# ------------------------------------------------------------------ GPU: against the model
SHAPES = [(40, 36, 30), (17, 64, 9), (1, 50, 33), (3, 130, 5), (2, 6, 300), (70, 65, 67)]
# (input dtype, mask, gamma, spacing): both dtypes, with and without a mask, fixed and automatic gamma pairwise; one anisotropic spacing
VARIANTS = {'f64-auto': (np.float64, False, None, None), 'f32-mask-auto': (np.float32, True, None, None),
            'f64-mask-fixed': (np.float64, True, 15.0, None), 'f32-fixed': (np.float32, False, 15.0, None),
            'f64-auto-aniso': (np.float64, False, None, (1.0, 1.0, 2.0))}
SEEDS = {}                                                   # shape -> seed, where seed 0 put more than TIE_CAP of a case's voxels into the tie set


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    dtype, masked, gamma, spacing = VARIANTS[variant]
    I, brain = _input(SEEDS.get(shape, 0), shape)
    I = I.astype(dtype)
    ref = M.vesselness(I, SIGMAS, gamma=gamma, mask=brain if masked else None, spacing=spacing)
    for a in (I, brain) + tuple(ref.values()):
        a.setflags(write=False)
    return I, (brain if masked else None), gamma, spacing, ref


def _compare(got, info, ref, label):
    """The bar of the issue; returns the largest deviation outside the tie set."""
    free = ~ref['ties']
    assert ref['ties'].sum() <= TIE_CAP * ref['ties'].size, 'tie set too large: change the seed of this case'
    dev = float(np.abs(got - ref['V'])[free].max())
    gdev = float(np.abs(info['gammas'] / ref['gammas'] - 1).max())
    # the model's V_sigma at the returned scale index attains the maximum
    at_scale = np.take_along_axis(ref['per_scale'], info['scale'][None].astype(np.int64), axis=0)[0]
    sdev = float(np.abs(at_scale - ref['V'])[free].max())
    print('{}: ties {} of {}, max |V - model| {:.3e}, gammas rel {:.3e}, scale consistency {:.3e}, max V {:.3f}'.format(
        label, int(ref['ties'].sum()), ref['ties'].size, dev, gdev, sdev, float(ref['V'].max())))
    assert got.dtype == np.float64 and got.shape == ref['V'].shape
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert dev <= BAR
    assert gdev <= 1e-12
    assert sdev <= BAR and info['scale'].dtype == np.uint8 and not info['scale'][got == 0].any()
    return dev


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_model_tie_sets_are_small(shape, variant):
    """No GPU: the cases of the GPU comparison keep their tie sets under the cap, and are not trivial."""
    ref = _case(shape, variant)[4]
    assert ref['ties'].sum() <= TIE_CAP * ref['ties'].size
    assert ref['V'].max() > 0.2 and (ref['V'] > 0).mean() > 0.02 and (ref['gammas'] > 0).all()
    assert len(set(np.unique(ref['scale']))) == 3


@pytest.mark.gpu
@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_vesselness_matches_model(shape, variant):
    I, brain, gamma, spacing, ref = _case(shape, variant)
    info = {'scale': None}
    got = VS.vesselnessFilter(I, SIGMAS, gamma=gamma, brainVolumeMask=brain, spacing=spacing, info=info)
    _compare(got, info, ref, '{} {}'.format('x'.join(map(str, shape)), variant))
    if brain is not None:
        assert not got[brain == 0].any()


@pytest.mark.gpu
def test_vesselness_dark_and_wide_radius():
    """bright=False on the negated volume; a scale whose radius (18) exceeds every extent of the volume and takes the
    narrower column tile of the axis-0 pass."""
    I, brain, _, _, _ = _case((17, 64, 9), 'f64-auto')
    ref = M.vesselness(-I, (1.0, 4.5), bright=False)
    info = {'scale': None}
    got = VS.vesselnessFilter(-I, (1.0, 4.5), bright=False, info=info)
    _compare(got, info, ref, '17x64x9 dark, sigma 4.5')


@pytest.mark.gpu
def test_vesselness_is_deterministic():
    I, brain, gamma, spacing, ref = _case((40, 36, 30), 'f32-mask-auto')
    a_info, b_info = {'scale': None}, {'scale': None}
    a = VS.vesselnessFilter(I, SIGMAS, brainVolumeMask=brain, info=a_info)
    b = VS.vesselnessFilter(I, SIGMAS, brainVolumeMask=brain, info=b_info)
    assert a.tobytes() == b.tobytes() and a_info['scale'].tobytes() == b_info['scale'].tobytes()
    assert a_info['gammas'].tobytes() == b_info['gammas'].tobytes()


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import vesselness as VS
from test_vesselness import _input, SIGMAS
I, brain = _input(4, (40, 36, 31))
dev = torch.device('cuda', 0)
for dtype in (np.float32, np.float64):
    hi, di = {{'scale': None}}, {{'scale': None}}
    host = VS.vesselnessFilter(I.astype(dtype), SIGMAS, brainVolumeMask=brain, info=hi)
    t = VS.vesselnessFilter(torch.as_tensor(I.astype(dtype), device=dev), SIGMAS, brainVolumeMask=torch.as_tensor(brain, device=dev), info=di)
    assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == I.shape and host.max() > 0.2
    assert t.cpu().numpy().tobytes() == host.tobytes()
    assert di['scale'].is_cuda and di['scale'].cpu().numpy().tobytes() == hi['scale'].tobytes()
    assert di['gammas'].tobytes() == hi['gammas'].tobytes()
# an integer tensor goes in as float64; a host mask with a device volume
q = np.round(I).astype(np.int16)
t = VS.vesselnessFilter(torch.as_tensor(q, device=dev), SIGMAS, brainVolumeMask=brain)
assert t.cpu().numpy().tobytes() == VS.vesselnessFilter(q, SIGMAS, brainVolumeMask=brain).tobytes()
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_vesselness_device_resident():
    """A tensor on the GPU goes in by its device pointer and a float64 tensor on the same device comes out, bit-identical
    to the host call.  Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def _gaussian_tube(shape, seed=7):
    """A bright tube with a Gaussian cross-section of width 2 voxels that swings along axis 0, noise of sigma 10; the brain
    mask; the squared distance of every voxel to the tube's axis."""
    brain, _ = _volumes(seed, shape)
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    c = [(n - 1) / 2.0 for n in shape]
    d2 = (y - c[1] - 0.15 * shape[1] * np.sin(2 * np.pi * x / shape[0])) ** 2 + (z - c[2]) ** 2
    return 100.0 * np.exp(-0.5 * d2 / 4.0) + np.random.default_rng(seed).normal(0.0, 10.0, shape), brain, d2


@pytest.mark.gpu
def test_vesselness_main_feeds_stage_one(tmp_path, capsys):
    """main writes float32 vesselnessFiltered.nii.gz with the input's affine; generateVesselVolume.main runs on the same
    folder next and its mask is the tube."""
    from arterynetwork_amd import nifti, generateVesselVolume as G
    shape = (48, 40, 32)
    I, brain, d2 = _gaussian_tube(shape)
    aff = np.array([[0.5, 0, 0, -10.0], [0, 0.5, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    nifti.saveVolume(I, aff, str(tmp_path / 'brainVolume.nii.gz'), astype=np.float32)
    nifti.saveVolume(I, aff, str(tmp_path / '401 3D MRA BRAIN.nii.gz'), astype=np.float32)
    nifti.saveVolume(brain, aff, str(tmp_path / 'brainVolumeMask.nii.gz'))
    sigmas = (0.5, 1.0)                                       # millimetres: 1 and 2 voxels in plane
    ves = VS.main(str(tmp_path), sigmas=sigmas)
    path = os.path.join(str(tmp_path), 'vesselnessFiltered.nii.gz')
    assert 'vesselnessFiltered.nii.gz saved to {}.'.format(path) in capsys.readouterr().out
    stored, aff2 = nifti.loadVolume(str(tmp_path), 'vesselnessFiltered.nii.gz')
    assert stored.dtype == np.float32 and np.array_equal(stored, ves.astype(np.float32)) and np.allclose(aff2, aff)
    spacing = np.sqrt((aff2[:3, :3] ** 2).sum(axis=0))        # the column norms of the affine as the file holds it (float32: 0.6 is not exact)
    assert np.allclose(spacing, (0.5, 0.5, 0.6))
    ref = M.vesselness(I.astype(np.float32), sigmas, mask=brain, spacing=spacing)
    assert np.abs(ves - ref['V'])[~ref['ties']].max() <= BAR and ref['V'].max() > 0.5
    mask = G.main(str(tmp_path))
    assert mask.dtype == np.uint8 and mask.sum() > 150
    assert d2[mask != 0].max() <= 9.0                          # nothing further than 1.5 widths from the tube's axis ...
    assert len(np.unique(np.nonzero(mask)[0])) >= 40           # ... which it follows through the brain mask (44 of the 48 planes)


# ------------------------------------------------------------------ no GPU needed: the kernels' resource records
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_vesselness_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vves_device.hip' in build.SOURCES
    out = tmp_path / 'vves_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vves_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):
        recs[m.group(1)] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1))
    kernels = {k: v for k, v in recs.items() if 'k_ves_' in k}
    for frag in ('k_ves_axis2IfE', 'k_ves_axis2IdE', 'k_ves_axis1E', 'k_ves_axis0ILi0E', 'k_ves_axis0ILi1E'):
        assert any(frag in k for k in kernels), 'kernel not found: ' + frag
    for k, scratch in kernels.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (k, scratch)
