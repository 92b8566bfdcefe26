"""Skull stripping (DESIGN.md section 9 entry f17): the numpy / scipy model tests/brain_model.py is checked on the CPU (its two
Laplacians of Gaussian against each other, Otsu against a brute-force loop, what the edge term is for, the border rules), then
the GPU entries must return: numpy's histogram, the restated model's bits for the edge response, scipy.ndimage's morphology,
largest component and hole filling voxel for voxel, and the model's mask - stage by stage - end to end."""
import functools
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

import brain_model as M
from conftest import ROOT
from arterynetwork_amd import brain as BR
from arterynetwork_amd._capi import VrgError

BAR = 1e-9                                               # of the input's span: the project's bar for float64 quantities against their oracle
SPACINGS = (None, (1.0, 1.0, 2.0), (0.5, 0.7, 1.3))

# the tile extents of the edge kernels (csrc/vbrain_device.hip): k_brain_axis0 BZ; k_brain_axis1 BY and 4 BY; k_brain_axis2 BLX and BX2
E_LOG = ((8,), (8, 32), (64, 256))


def _tile_shapes():
    """Per axis and tile extent E: E - 1, E, E + 1 and 2 E + 1 on that axis, the other two extents small."""
    shapes = []
    for axis in range(3):
        for E in E_LOG[axis]:
            for n in (E - 1, E, E + 1, 2 * E + 1):
                s = [3, 5, 6]
                s[axis] = n
                shapes.append(tuple(s))
    return shapes


LOG_SMALL = [(1, 1, 7), (5, 1, 1), (3, 4, 5)]
LOG_TILES = [s for s in _tile_shapes() if s not in LOG_SMALL]


def _noisy(shape, seed=0):
    """A bright box on a dark ground, a ramp along axis 2, Gaussian noise of sigma 5 on every voxel."""
    v = np.random.default_rng(seed).normal(0.0, 5.0, shape)
    v[tuple(slice(n // 4, n - n // 4) for n in shape)] += 100.0
    return v + 0.5 * np.arange(shape[2])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _phantom(shape, csf, noise, seed):
    I, brain = M.head_phantom(shape, csf, noise, seed)
    I.setflags(write=False)
    brain.setflags(write=False)
    return I, brain


@functools.lru_cache(maxsize=None)
def _model(shape, csf, noise, seed, edge=0.05, restated=False):
    """The model's result on a phantom, computed once: (mask, info)."""
    return M.extract(_phantom(shape, csf, noise, seed)[0], edge=edge, diffusion=M.DIFFUSION, restated=restated)


# ------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize('spacing', SPACINGS, ids=str)
def test_model_restated_log_is_scipys(spacing):
    I = _noisy((11, 13, 17), seed=1)
    span = np.ptp(I)
    for sigma in (0.8, 1.0, 2.0):
        a, b = M.log_restated(I, sigma, spacing), M.log_scipy(I, sigma, spacing)
        dev = np.abs(a - b).max() / span
        print('sigma {} spacing {}: {:.3e}'.format(sigma, spacing, dev))
        assert dev <= BAR
    # a flat volume: the truncated taps of phi'' do not sum to 0 exactly - E is about -2.2e-4 of the intensity at sigma 1, never above 0
    flat = M.log_restated(np.full((4, 5, 6), 37.3))
    assert (flat <= 0).all() and np.abs(flat).max() <= 1e-3 * 37.3


def test_model_otsu_is_the_brute_force_loop():
    rng = np.random.default_rng(2)
    cases = [rng.integers(0, 1000, 256) for _ in range(20)]
    cases += [rng.integers(0, 2, 256) * rng.integers(0, 10 ** 7, 256) for _ in range(10)]
    two = np.zeros(256, np.int64)
    two[3], two[200] = 5, 5                                                # every t in 3..199 is a maximum: the first one wins
    flat = np.ones(256, np.int64)
    cases += [two, flat, M.histogram(_phantom(M.PHANTOM_SHAPES[0], 15.0, 3, 0)[0])[2]]
    for c in cases:
        between, _ = M.otsu_table(c)
        t = M.otsu_brute(c)
        assert int(np.argmax(between)) == t
        assert BR.otsu(c)[0] == t
    assert M.otsu_brute(two) == 3
    lo, hi, counts = M.histogram(_phantom(M.PHANTOM_SHAPES[0], 15.0, 0, 0)[0])
    fl, contrast, t = M.floor_contrast(counts, lo, hi)
    assert 15.0 < fl < 85.0 and 50.0 < contrast < 110.0                   # between the gap and the scalp; about brain minus air
    assert M.floor_contrast(counts, lo, hi, floor=fl)[:2] == (fl, contrast)
    assert M.floor_contrast(counts, lo, hi, floor=lo - 1.0)[2] == 0 and M.floor_contrast(counts, lo, hi, floor=hi + 1.0)[2] == 254


CASES = [(shape, csf, noise, seed) for shape in M.PHANTOM_SHAPES for csf in (15.0, 55.0) for noise in (0, 3, 6) for seed in (0, 1, 2)]


def test_model_finds_the_brain_with_the_edge_term():
    """Dice >= 0.99 on all 36 phantoms.  Measured when this was written: 0.9923 .. 1.0000."""
    scores = [M.dice(_model(*case)[0], _phantom(*case)[1]) for case in CASES]
    print('Dice {:.4f} .. {:.4f}'.format(min(scores), max(scores)))
    assert len(scores) == 36 and min(scores) >= 0.99


def test_model_without_the_edge_term_merges_scalp_and_brain():
    """With the gap above the floor (csf = 55) and the edge term off, scalp and brain stay one component: Dice <= 0.6.
    Measured when this was written: 0.5154 and 0.5640 for the two shapes."""
    scores = [M.dice(_model(*case, edge=1e300)[0], _phantom(*case)[1]) for case in CASES if case[1] == 55.0]
    print('Dice {:.4f} .. {:.4f}'.format(min(scores), max(scores)))
    assert len(scores) >= 12 and max(scores) <= 0.6


def test_model_needs_the_diffusion_on_noisy_data():
    """What the docstrings say: without the diffusion a noisy case of the second shape fails (Dice 0.515 when this was written)."""
    I, brain = _phantom(M.PHANTOM_SHAPES[1], 55.0, 6, 0)
    assert M.dice(M.extract(I, restated=False)[0], brain) <= 0.6
    assert M.dice(_model(M.PHANTOM_SHAPES[1], 55.0, 6, 0)[0], brain) >= 0.99


def test_model_border_rules():
    full = np.ones((4, 5, 6), bool)
    assert not M.erode(full, 1, 0)[0].any() and M.erode(full, 1, 0)[1:-1, 1:-1, 1:-1].all() and M.erode(full, 1, 0).sum() == 2 * 3 * 4
    assert M.erode(full, 3, 1).all()                                       # the outside counts as 1: nothing is eaten at a face
    half = np.zeros((7, 5, 6), bool)
    half[:3] = True                                                        # touches the face i0 = 0
    planes = np.arange(7)[:, None, None] * np.ones((1, 5, 6))
    assert np.array_equal(M.erode(half, 1, 1), planes < 2)                 # eaten only where it ends inside the volume
    assert not M.erode(half, 1, 0)[0].any() and not M.erode(half, 1, 0)[:, 0].any() and M.erode(half, 1, 0).sum() == 1 * 3 * 4
    assert np.array_equal(M.dilate(half, 1), planes < 4)
    assert np.array_equal(M.erode(half, 0), half) and np.array_equal(M.dilate(half, 0), half)
    # closing with the outside as 1 gives back a body on a face; with 0 it would eat it there
    assert np.array_equal(M.erode(M.dilate(half, 2), 2, 1), half) and not np.array_equal(M.erode(M.dilate(half, 2), 2, 0), half)


def _diagonal_leak():
    """A box with a one-voxel cavity whose only way out runs across a diagonal: 6-connectivity does not pass, the cavity is filled."""
    m = np.zeros((7, 7, 7), np.uint8)
    m[1:6, 1:6, 1:6] = 1
    m[3, 3, 3] = 0                                                         # the cavity
    m[3, 3, 4] = 0
    m[3, 4, 5] = 0                                                         # diagonal to (3, 3, 4), open to the outside through (3, 4, 6)
    return m


def test_model_fill_holes_closes_a_diagonal_leak():
    m = _diagonal_leak()
    filled = ndi.binary_fill_holes(m)
    assert filled[3, 3, 3] and filled[3, 3, 4] and not filled[3, 4, 5]


# ------------------------------------------------------------------ no GPU needed: arguments
def test_argument_errors_raise():
    """What the host can check is refused before a device is looked for: no GPU needed."""
    I = np.zeros((6, 5, 4))
    m = np.zeros((6, 5, 4), np.uint8)
    nan, inf = float('nan'), float('inf')
    for kw in [dict(volume=np.zeros((6, 5))), dict(sigma=0.0), dict(sigma=nan), dict(sigma=inf), dict(sigma=0.1), dict(sigma=17.0),
               dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, nan, 1.0)), dict(sigma=1.0, spacing=(1.0, 1.0, 9.0))]:
        args = dict(volume=I)
        args.update(kw)
        with pytest.raises(ValueError):
            BR.laplacianOfGaussian(**args)
    for kw in [dict(volume=np.zeros((6, 5))), dict(sigma=-1.0), dict(edge=nan), dict(floor=inf), dict(floor=nan), dict(erosion=-1), dict(erosion=1.5),
               dict(erosion=1001), dict(closing=-1), dict(closing=1001), dict(diffusion=dict(iterations=3)), dict(diffusion=5),
               dict(diffusion=dict(conductance=20, radius=1)), dict(diffusion=dict(conductance=-1.0)), dict(spacing=(1.0, -1.0, 1.0)),
               dict(seed=(1, 2)), dict(seed=(6, 0, 0)), dict(seed=(0, 0, -1)), dict(seed=(0.5, 0, 0)), dict(info=[])]:
        args = dict(volume=I)
        args.update(kw)
        with pytest.raises(ValueError):
            BR.brainExtraction(**args)
    for f in (BR.binaryErosion, BR.binaryDilation):
        for kw in (dict(steps=-1), dict(steps=1.5), dict(steps=100001)):
            with pytest.raises(ValueError):
                f(m, **kw)
        with pytest.raises(ValueError):
            f(np.zeros((6, 5), np.uint8))
    for border in (2, -1):
        with pytest.raises(ValueError):
            BR.binaryErosion(m, 1, border)
    for kw in (dict(connectivity=0), dict(connectivity=4), dict(seed=(0, 0, 4)), dict(seed=(0, 0)), dict(mask=np.zeros((6, 5), np.uint8))):
        args = dict(mask=m)
        args.update(kw)
        with pytest.raises(ValueError):
            BR.largestComponent(**args)
    with pytest.raises(ValueError):
        BR.fillHoles(np.zeros((6, 5), np.uint8))
    with pytest.raises(ValueError):
        BR.intensityFloor(np.zeros((6, 5)))
    with pytest.raises(ValueError):
        BR.intensityFloor(I, floor=nan)
    with pytest.raises(ValueError):
        BR.otsu(np.zeros(255))
    with pytest.raises(ValueError):
        BR.main('.', spacing=(1.0, 1.0, 1.0))


def _refusals(dll, inp, f32, msk, shape, outs):
    """Every refused input of the six C entries: (label, return code).  `inp`, `f32` and `msk` are addresses of a float64 volume,
    a float32 volume and a uint8 mask of that shape; `outs` of the outputs: E (float64), a uint8 volume, lo, hi, the 256 counts,
    a size, 5 stage volumes, 16 info numbers."""
    oE, oM, oLo, oHi, oC, oS, oSt, oI = outs
    sp = lambda *h: np.array(h, dtype=np.float64)
    keep = []                                            # (the spacing arrays must outlive the calls)
    inf, nan = float('inf'), float('nan')
    big = (2000, 2000, 600)

    def hist(label, volume=inp, dtype=6, dims=shape, lo=oLo, hi=oHi, counts=oC):
        return 'histogram ' + label, dll.vmask_brain_histogram(0, volume, dtype, *dims, lo, hi, counts)

    def log(label, volume=inp, dtype=6, dims=shape, spacing=None, sigma=1.0, to=oE):
        if spacing is not None:
            keep.append(spacing)
        return 'log ' + label, dll.vmask_brain_log(0, volume, dtype, *dims, spacing.ctypes.data if spacing is not None else None, sigma, to)

    def morph(label, mask=msk, dims=shape, op=0, steps=1, border=0, to=oM):
        return 'morph ' + label, dll.vmask_binary_morph(0, mask, *dims, op, steps, border, to)

    def largest(label, mask=msk, dims=shape, connectivity=1, seed=-1, to=oM, size=oS):
        return 'largest ' + label, dll.vmask_largest_component(0, mask, *dims, connectivity, seed, to, size)

    def fill(label, mask=msk, dims=shape, to=oM):
        return 'fill ' + label, dll.vmask_fill_holes(0, mask, *dims, to)

    def extract(label, volume=inp, dtype=6, dims=shape, spacing=None, sigma=1.0, threshold=1.0, floor=10.0, erosion=1, closing=1, seed=-1, to=oM):
        if spacing is not None:
            keep.append(spacing)
        return 'extract ' + label, dll.vmask_brain_extract(0, volume, dtype, *dims, spacing.ctypes.data if spacing is not None else None, sigma,
                                                           threshold, floor, erosion, closing, seed, to, oSt, oI)
    V = shape[0] * shape[1] * shape[2]
    return [hist('dtype 4', dtype=4), hist('dtype 7', volume=f32, dtype=7), hist('null volume', volume=None), hist('null lo', lo=None),
            hist('null hi', hi=None), hist('null counts', counts=None), hist('shape 0', dims=(0, shape[1], shape[2])), hist('shape envelope', dims=big),
            log('sigma 0', sigma=0.0), log('sigma < 0', sigma=-1.0), log('sigma nan', sigma=nan), log('sigma inf', sigma=inf),
            log('radius 0', sigma=0.1), log('radius 65', sigma=16.2), log('radius 65 by the spacing', sigma=2.0, spacing=sp(1, 1, 0.1)),
            log('spacing 0', spacing=sp(1, 0, 1)), log('spacing < 0', spacing=sp(-1, 1, 1)), log('spacing nan', spacing=sp(1, 1, nan)),
            log('spacing inf', spacing=sp(inf, 1, 1)), log('dtype 4', dtype=4), log('dtype 7', dtype=7), log('null volume', volume=None),
            log('null out', to=None), log('shape 0', dims=(shape[0], 0, shape[2])), log('shape envelope', dims=big),
            morph('op 2', op=2), morph('op -1', op=-1), morph('steps -1', steps=-1), morph('steps 100001', steps=100001), morph('border 2', border=2),
            morph('border -1', border=-1), morph('border 1 with a dilation', op=1, border=1), morph('null mask', mask=None), morph('null out', to=None),
            morph('shape 0', dims=(shape[0], shape[1], 0)), morph('shape envelope', dims=big),
            largest('connectivity 0', connectivity=0), largest('connectivity 4', connectivity=4), largest('seed -2', seed=-2), largest('seed V', seed=V),
            largest('null mask', mask=None), largest('null out', to=None), largest('shape 0', dims=(0, shape[1], shape[2])), largest('shape envelope', dims=big),
            fill('null mask', mask=None), fill('null out', to=None), fill('shape 0', dims=(0, shape[1], shape[2])), fill('shape envelope', dims=big),
            extract('sigma 0', sigma=0.0), extract('sigma nan', sigma=nan), extract('radius 65', sigma=16.2), extract('spacing 0', spacing=sp(1, 0, 1)),
            extract('spacing nan', spacing=sp(nan, 1, 1)), extract('threshold nan', threshold=nan), extract('floor nan', floor=nan),
            extract('floor inf', floor=inf), extract('erosion -1', erosion=-1), extract('erosion 1001', erosion=1001), extract('closing -1', closing=-1),
            extract('closing 1001', closing=1001), extract('seed -2', seed=-2), extract('seed V', seed=V), extract('dtype 4', dtype=4),
            extract('dtype 7', volume=f32, dtype=7), extract('null volume', volume=None), extract('null out', to=None),
            extract('shape 0', dims=(shape[0], 0, shape[2])), extract('shape envelope', dims=big)]


N_REFUSALS = 68
SENTINEL = 77


def test_c_entries_refuse_before_a_device_is_looked_for():
    """Host pointers, no GPU needed: every refusal is VRG_E_ARG and leaves the outputs alone."""
    dll = BR._lib()
    shape = (4, 5, 6)
    I = _noisy(shape)
    I32 = I.astype(np.float32)
    msk = (I > 50).astype(np.uint8)
    outs = [np.full(shape, -12345.0), np.full(shape, SENTINEL, np.uint8), np.full(1, -12345.0), np.full(1, -12345.0), np.full(256, SENTINEL, np.uint64),
            np.full(1, SENTINEL, np.int64), np.full((5,) + shape, SENTINEL, np.uint8), np.full(16, SENTINEL, np.int64)]
    res = _refusals(dll, I.ctypes.data, I32.ctypes.data, msk.ctypes.data, shape, [o.ctypes.data for o in outs])
    assert len(res) == N_REFUSALS
    for label, rc in res:
        assert rc == -1, label                           # VRG_E_ARG
    assert all((o == (-12345.0 if o.dtype == np.float64 else SENTINEL)).all() for o in outs)
    assert np.array_equal(I, _noisy(shape)) and np.array_equal(msk, (I > 50).astype(np.uint8))


# ------------------------------------------------------------------ no GPU needed: the kernels' resource records
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_brain_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vbrain_device.hip' in build.SOURCES
    out = tmp_path / 'vbrain_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vbrain_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    want = {'k_brain_minmax': 2, 'k_brain_hist': 2, 'k_brain_axis2': 2, 'k_brain_axis1': 1, 'k_brain_axis0': 4, 'k_bits_pack': 1, 'k_bits_unpack': 1,
            'k_bits_count': 1, 'k_bits_morph': 2, 'k_brain_sizes': 1, 'k_brain_winner': 1, 'k_brain_select': 1, 'k_fill_faces': 1, 'k_fill_apply': 1}
    for kernel, n in want.items():
        assert sum(kernel in k for k in recs) == n, (kernel, sorted(recs))
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        # the first build: k_brain_axis1 66, k_brain_axis0 64 (E) and 66 (bits) - 24 float64 sums per thread -, k_bits_morph 40 and 38,
        # k_brain_axis2 26, everything else 10 .. 19
        assert vgprs <= 72, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ GPU: the histogram
def _edge_volume(shape, dtype):
    """Values on the bin edges lo + k (hi - lo) / 256 with lo = 0, hi = 256 - the integers 0..256 - and halves between them."""
    n = int(np.prod(shape))
    v = np.resize(np.concatenate([np.arange(257.0), np.arange(256.0) + 0.5, [256.0, 256.0, 0.0]]), n)
    if n < 257:
        v[0], v[-1] = 0.0, 256.0
    if dtype == np.int16:
        v = np.floor(v)
    return v.reshape(shape).astype(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.int16], ids=lambda d: np.dtype(d).name)
def test_histogram_is_numpys(dtype):
    for shape in ((1, 1, 2), (3, 4, 5), (9, 17, 65), (40, 33, 70)):
        vols = [_edge_volume(shape, dtype), (_noisy(shape, seed=3) * (10 if dtype == np.int16 else 1)).astype(dtype)]
        if dtype != np.int16:
            vols.append((_noisy(shape, seed=4) * 1e-3 - 7.0).astype(dtype))
        for v in vols:
            before = v.copy()
            fl, contrast, lo, hi, counts = BR.intensityFloor(v)
            rlo, rhi, rcounts = M.histogram(v)
            assert (lo, hi) == (rlo, rhi) and counts.dtype == np.uint64 and np.array_equal(counts, rcounts), (shape, dtype)
            assert int(counts.sum()) == v.size and np.array_equal(v, before)
            rfl, rcontrast, _ = M.floor_contrast(rcounts, rlo, rhi)
            assert (fl, contrast) == (rfl, rcontrast)
            given = BR.intensityFloor(v, floor=0.5 * (lo + hi))
            assert given[:2] == M.floor_contrast(rcounts, rlo, rhi, floor=0.5 * (lo + hi))[:2]
    for bad in (np.full((3, 4, 5), 2.5), np.array([[[1.0, np.nan, 2.0]]]), np.array([[[1.0, np.inf, 2.0]]], np.float32)):
        with pytest.raises(VrgError):
            BR.intensityFloor(bad)


# ---- k_brain_minmax and k_brain_hist are capped at 1024 workgroups of 256 threads: voxels from 262 144 on are met on a second turn
SECOND_TURN = 1024 * 256
LATE_SHAPE = (5, 210, 257)                                 # 269 850 voxels: the last 7 706 on the second turn


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_histogram_is_numpys_on_the_second_turn(dtype):
    """269 850 voxels > 262 144: the minimum and the maximum are voxels that only the second turn of k_brain_minmax sees, and the
    256 counts, which k_brain_hist's second turn adds to, are numpy's and sum to V."""
    V = int(np.prod(LATE_SHAPE))
    assert SECOND_TURN < V < 2 * SECOND_TURN
    v = _noisy(LATE_SHAPE, seed=7).astype(dtype)
    v.flat[SECOND_TURN + 5], v.flat[V - 2] = v.min() - 50.0, v.max() + 50.0
    assert int(v.argmin()) == SECOND_TURN + 5 and int(v.argmax()) == V - 2
    before = v.copy()
    fl, contrast, lo, hi, counts = BR.intensityFloor(v)
    rlo, rhi, rcounts = M.histogram(v)
    assert (lo, hi) == (rlo, rhi) == (float(v.flat[SECOND_TURN + 5]), float(v.flat[V - 2]))
    assert counts.dtype == np.uint64 and np.array_equal(counts, rcounts) and int(counts.sum()) == V
    assert (fl, contrast) == M.floor_contrast(rcounts, rlo, rhi)[:2] and np.array_equal(v, before)
    # the same volume with the first turn's voxels alone gives other counts: the second turn's voxels are in these
    assert not np.array_equal(np.bincount(np.minimum(255.0, np.floor((v.ravel()[:SECOND_TURN].astype(np.float64) - lo) * (256.0 / (hi - lo)))).astype(np.int64), minlength=256), rcounts)


@pytest.mark.gpu
@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf], ids=['nan', 'inf', '-inf'])
def test_a_voxel_that_is_not_finite_on_the_second_turn_is_refused(value):
    """One NaN (Inf) at a raster index >= 262 144, which only the second turn of k_brain_minmax meets: every entry refuses."""
    for dtype, at in ((np.float32, SECOND_TURN), (np.float64, int(np.prod(LATE_SHAPE)) - 1), (np.float32, SECOND_TURN + 4321)):
        v = _noisy(LATE_SHAPE, seed=8).astype(dtype)
        assert np.isfinite(v).all()
        v.flat[at] = value
        with pytest.raises(VrgError):
            BR.intensityFloor(v)
        with pytest.raises(VrgError):
            BR.laplacianOfGaussian(v)
        with pytest.raises(VrgError):
            BR.brainExtraction(v)
        with pytest.raises(VrgError):
            BR.brainExtraction(v, floor=50.0)


# ------------------------------------------------------------------ GPU: the edge response
def _log_case(shape, sigma, spacing, dtype, seed=0):
    I = _noisy(shape, seed).astype(dtype)
    before = I.copy()
    got = BR.laplacianOfGaussian(I, sigma, spacing)
    ref = M.log_restated(I, sigma, spacing)
    label = '{} sigma {} {} {}'.format(shape, sigma, spacing, np.dtype(dtype).name)
    assert got.dtype == np.float64 and got.shape == tuple(shape), label
    assert np.array_equal(_bits(got), _bits(ref)), '{}: {} voxels differ, max {:.3e}'.format(label, int((got != ref).sum()), np.abs(got - ref).max())
    assert np.array_equal(I, before), label


@pytest.mark.gpu
@pytest.mark.parametrize('shape', LOG_SMALL, ids=lambda s: 'x'.join(map(str, s)))
def test_log_is_the_model_small_shapes(shape):
    """Tap radii 2, 4, 7, 12 and 64 against extents of 1, 3, 4, 5 and 7: smaller than, equal to and larger than the axis."""
    for sigma in (0.5, 1.0, 1.75, 3.0, 16.0):
        for dtype in (np.float32, np.float64):
            _log_case(shape, sigma, None, dtype)
    for spacing in SPACINGS[1:]:
        for sigma in (0.8, 2.0):
            _log_case(shape, sigma, spacing, np.float64)
            _log_case(shape, sigma, spacing, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', LOG_TILES, ids=lambda s: 'x'.join(map(str, s)))
def test_log_is_the_model_at_the_tile_extents(shape):
    for i, spacing in enumerate(SPACINGS):
        _log_case(shape, 1.0, spacing, (np.float64, np.float32, np.float64)[i], seed=i)
    _log_case(shape, 2.6, None, np.float32, seed=5)                        # radius 10: wider than a thread's 8 rows / planes


@pytest.mark.gpu
def test_log_is_the_model_beyond_32768_rows():
    """129 x 255 = 32 895 rows > 32 768: k_brain_axis2's workgroups fill a second row of the grid, rows 32 768 .. 32 894."""
    shape = (129, 255, 3)
    assert shape[0] * shape[1] > 32768
    _log_case(shape, 1.0, None, np.float32, seed=6)
    _log_case(shape, 1.0, (0.5, 0.7, 1.3), np.float64, seed=7)


@pytest.mark.gpu
def test_log_refuses_voxels_that_are_not_finite():
    I = _noisy((5, 6, 7))
    I[2, 3, 4] = np.nan
    with pytest.raises(VrgError):
        BR.laplacianOfGaussian(I)
    with pytest.raises(VrgError):
        BR.brainExtraction(I)


# ------------------------------------------------------------------ GPU: the morphology
def _masks(shape, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random(shape) < p).astype(np.uint8) for p in (0.5, 0.9, 0.99)] + [np.ones(shape, np.uint8), np.zeros(shape, np.uint8)]


@pytest.mark.gpu
@pytest.mark.parametrize('n2', [1, 2, 63, 64, 65, 127, 128, 129, 193])
def test_morphology_is_scipys(n2):
    for n0, n1 in itertools.product((1, 2, 5), repeat=2):
        shape = (n0, n1, n2)
        for k, m in enumerate(_masks(shape, seed=n0 * 7 + n1)):
            before = m.copy()
            for steps in (0, 1, 2, 3, min(shape) + 1):
                for border in (0, 1):
                    got = BR.binaryErosion(m, steps, border)
                    assert got.dtype == np.uint8 and np.array_equal(got, M.erode(m, steps, border)), ('erode', shape, k, steps, border)
                assert np.array_equal(BR.binaryDilation(m, steps), M.dilate(m, steps)), ('dilate', shape, k, steps)
            assert np.array_equal(m, before)


@pytest.mark.gpu
def test_morphology_takes_any_non_zero_value_and_more_rows():
    m = (np.random.default_rng(5).random((9, 17, 130)) < 0.8) * np.random.default_rng(6).integers(1, 255, (9, 17, 130))
    for steps in (1, 4):
        assert np.array_equal(BR.binaryErosion(m, steps, 1), M.erode(m != 0, steps, 1))
        assert np.array_equal(BR.binaryErosion(m, steps), M.erode(m != 0, steps))
        assert np.array_equal(BR.binaryDilation(m == 0, steps), M.dilate(m == 0, steps))


# ------------------------------------------------------------------ GPU: the largest component
STRUCTURES = {c: ndi.generate_binary_structure(3, c) for c in (1, 2, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize('connectivity', [1, 2, 3])
def test_largest_component_is_scipys(connectivity):
    for shape, p, seed in (((6, 7, 9), 0.3, 0), ((9, 17, 65), 0.25, 1), ((5, 4, 130), 0.5, 2), ((1, 1, 9), 0.6, 3), ((12, 11, 64), 0.2, 4)):
        m = (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)
        ref, size, _ = M.largest(m, STRUCTURES[connectivity])
        n = []
        got = BR.largestComponent(m, connectivity, size=n)
        assert got.dtype == np.uint8 and np.array_equal(got, ref) and n == [size], (shape, connectivity)
        # a seed inside a smaller component, and one on the background
        lab, ncomp = ndi.label(m, STRUCTURES[connectivity])
        sizes = np.bincount(lab.ravel())[1:]
        small = int(np.argmin(sizes)) + 1
        if ncomp > 1 and sizes[small - 1] < size:
            at = tuple(int(x) for x in np.argwhere(lab == small)[-1])
            n = []
            assert np.array_equal(BR.largestComponent(m, connectivity, seed=at, size=n), lab == small) and n == [int(sizes[small - 1])]
        if (m == 0).any():
            with pytest.raises(VrgError):
                BR.largestComponent(m, connectivity, seed=tuple(int(x) for x in np.argwhere(m == 0)[0]))


@pytest.mark.gpu
def test_largest_component_ties_empty_and_full():
    m = np.zeros((4, 5, 70), np.uint8)
    m[3, 1, 60:66] = 1                                                     # six voxels, met second in raster order
    m[0, 3, 2:8] = 1                                                       # six voxels, met first
    m[2, 2, 2:5] = 1
    n = []
    got = BR.largestComponent(m, size=n)
    assert n == [6] and got[0, 3, 2:8].all() and got.sum() == 6
    assert np.array_equal(got, M.largest(m)[0])
    n = []
    assert not BR.largestComponent(np.zeros((3, 4, 5), np.uint8), size=n).any() and n == [0]
    with pytest.raises(VrgError):
        BR.largestComponent(np.zeros((3, 4, 5), np.uint8), seed=(1, 1, 1))
    for connectivity in (1, 2, 3):
        n = []
        assert BR.largestComponent(np.ones((2, 3, 130), np.uint8), connectivity, size=n).all() and n == [2 * 3 * 130]
    # diagonal neighbours: one component under 18 / 26 neighbours, two under 6
    d = np.zeros((3, 3, 3), np.uint8)
    d[0, 0, 0] = d[0, 1, 1] = d[1, 1, 1] = 1
    assert BR.largestComponent(d, 1).sum() == 2 and BR.largestComponent(d, 2).sum() == 3 and BR.largestComponent(d, 3).sum() == 3


# ---- k_brain_sizes: 2048 workgroups x 4 waves = 8192 waves, each a contiguous run of ceil(trips / 8192) trips of 64 voxels.  Above
# 524 288 voxels a run holds two trips and the wave carries the counts it holds from one trip into the next.
SIZES_SHAPE = (20, 160, 170)                               # 544 000 voxels = 8500 trips: runs of 2 trips, 128 voxels


def _check_largest(m, connectivity=1, label=''):
    ref, size, _ = M.largest(m, STRUCTURES[connectivity])
    n = []
    got = BR.largestComponent(m, connectivity, size=n)
    assert got.dtype == np.uint8 and np.array_equal(got, ref) and n == [size], (label, connectivity, n, size)
    return got, size


def test_sizes_shape_gives_every_wave_two_trips():
    V = int(np.prod(SIZES_SHAPE))
    trips = -(-V // 64)
    assert V > 2048 * 4 * 64 and -(-trips // (2048 * 4)) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('connectivity', [1, 2, 3])
def test_largest_component_is_scipys_when_a_wave_takes_two_trips(connectivity):
    """544 000 voxels, p = 0.3: under 6 neighbours 33 537 components, the largest of 1292 and 1108 voxels; under 18 and 26 one that
    runs through the whole volume and so through every wave's run.  Also a seed in a small component, and one on the background."""
    m = (np.random.default_rng(3).random(SIZES_SHAPE) < 0.3).astype(np.uint8)
    before = m.copy()
    got, size = _check_largest(m, connectivity, 'random 0.3')
    lab, ncomp = ndi.label(m, STRUCTURES[connectivity])
    sizes = np.bincount(lab.ravel())[1:]
    if connectivity == 1:
        assert ncomp == 33537 and sorted(sizes)[-2:] == [1108, 1292] and size == 1292
    else:
        assert size > m.sum() // 2
    for small in (int(np.argmin(sizes)) + 1, int(np.argsort(sizes, kind='stable')[len(sizes) // 2]) + 1, ncomp):      # the last label lies at the volume's end
        at = tuple(int(x) for x in np.argwhere(lab == small)[-1])
        n = []
        assert np.array_equal(BR.largestComponent(m, connectivity, seed=at, size=n), lab == small) and n == [int(sizes[small - 1])], small
    with pytest.raises(VrgError):
        BR.largestComponent(m, connectivity, seed=tuple(int(x) for x in np.argwhere(m == 0)[-1]))
    assert np.array_equal(m, before)


@pytest.mark.gpu
def test_largest_component_tie_and_slab_across_the_waves_runs():
    V = int(np.prod(SIZES_SHAPE))
    # two equal largest components in a sprinkle of small ones; the second in raster order lies wholly in the volume's second half, so
    # other waves count it: the first one wins
    m = (np.random.default_rng(4).random(SIZES_SHAPE) < 0.05).astype(np.uint8)
    m[0:3, 0:8, 0:45] = 0
    m[14:17, 98:106, 48:89] = 0
    m[1, 2:6, 3:40] = 1                                                    # 148 voxels, from raster index 27 543 on
    m[15, 100:104, 50:87] = 1                                              # 148 voxels, from raster index 425 050 on
    assert np.ravel_multi_index((15, 100, 50), SIZES_SHAPE) > V // 2 > 524288 // 2 > np.ravel_multi_index((1, 5, 39), SIZES_SHAPE)
    sizes = np.bincount(ndi.label(m, STRUCTURES[1])[0].ravel())[1:]
    assert sorted(sizes)[-2:] == [148, 148] and sorted(sizes)[-3] < 148
    got, size = _check_largest(m, 1, 'tie')
    assert size == 148 and got[1, 2:6, 3:40].all() and got.sum() == 148 and not got[15].any()
    flipped = m[::-1, ::-1, ::-1].copy()                                   # now the other box is met first
    got, size = _check_largest(flipped, 1, 'tie, flipped')
    assert size == 148 and got[4, 56:60, 83:120].all() and got.sum() == 148
    # a slab through the whole volume: every row of it, 170 voxels, crosses the boundary between two waves' runs of 128
    s = (np.random.default_rng(5).random(SIZES_SHAPE) < 0.2).astype(np.uint8)
    s[:, 80, :] = 1
    for connectivity in (1, 3):
        got, size = _check_largest(s, connectivity, 'slab')
        assert got[:, 80, :].all() and size >= 20 * 170


# ------------------------------------------------------------------ GPU: hole filling
def _nested():
    """A hole inside an island inside a hole: everything inside the outer shell is filled."""
    m = np.zeros((11, 11, 67), np.uint8)
    m[1:10, 1:10, 1:66] = 1
    m[2:9, 2:9, 2:65] = 0                                                  # the outer hole
    m[3:8, 3:8, 3:64] = 1                                                  # the island
    m[4:7, 4:7, 4:63] = 0                                                  # its hole
    return m


@pytest.mark.gpu
def test_fill_holes_is_scipys():
    cases = [(np.random.default_rng(s).random(shape) < p).astype(np.uint8)
             for s, (shape, p) in enumerate((((6, 7, 9), 0.6), ((9, 17, 65), 0.7), ((5, 6, 130), 0.8), ((1, 1, 9), 0.5), ((1, 7, 9), 0.7), ((12, 11, 65), 0.9)))]
    opened = np.zeros((7, 7, 65), np.uint8)
    opened[1:6, 1:6, 1:60] = 1
    opened[2:5, 2:5, 2:59] = 0
    closed = opened.copy()
    opened[3, 3, 0:2] = 0                                                  # the cavity reaches the face i2 = 0
    cases += [opened, closed, _diagonal_leak(), _nested(), np.zeros((4, 5, 6), np.uint8), np.ones((4, 5, 6), np.uint8), np.array([[[0, 1, 0, 0, 1, 0, 1, 1, 0]]], np.uint8)]
    for m in cases:
        before = m.copy()
        got = BR.fillHoles(m)
        assert got.dtype == np.uint8 and np.array_equal(got, ndi.binary_fill_holes(m)), m.shape
        assert np.array_equal(m, before)
    assert np.array_equal(BR.fillHoles(opened), opened) and BR.fillHoles(closed).sum() == 5 * 5 * 59
    d = BR.fillHoles(_diagonal_leak())
    assert d[3, 3, 3] == 1 and d[3, 3, 4] == 1 and d[3, 4, 5] == 0
    assert BR.fillHoles(_nested()).sum() == 9 * 9 * 65 and not BR.fillHoles(np.zeros((4, 5, 6), np.uint8)).any()


# ------------------------------------------------------------------ GPU: end to end
E2E = [(shape, csf, noise, 0) for shape in M.PHANTOM_SHAPES for csf in (15.0, 55.0) for noise in (0, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', E2E, ids=lambda c: '{}-csf{:g}-noise{}'.format('x'.join(map(str, c[0])), c[1], c[2]))
def test_extraction_is_the_model(case):
    I, brain = _phantom(*case)
    ref, rinfo = _model(*case, restated=True)
    info = dict(stages=True)
    got = BR.brainExtraction(I, diffusion=M.DIFFUSION, info=info)
    assert info['floor'] == rinfo['floor'] and info['contrast'] == rinfo['contrast'] and info['components'] == rinfo['components']
    for k in M.STAGES:
        assert np.array_equal(info['stages'][k], rinfo['stages'][k]), k
        assert info['counts'][k] == int(rinfo['stages'][k].sum()), k
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    assert M.dice(got, brain) >= 0.99 and info['peakBytes'] > 5 * 8 * I.size and info['mainSize'] == info['counts']['main']
    assert set(info['microseconds']) == set(BR.TIMED) and all(v >= 0 for v in info['microseconds'].values())
    again = BR.brainExtraction(I, diffusion=M.DIFFUSION)
    assert again.tobytes() == got.tobytes()


@pytest.mark.gpu
def test_extraction_handles_floor_seed_and_steps():
    I, _ = _phantom(M.PHANTOM_SHAPES[0], 15.0, 0, 0)
    for kw in (dict(floor=40.0), dict(erosion=2, closing=3), dict(erosion=0, closing=0), dict(sigma=1.5, edge=0.02), dict(spacing=(1.0, 1.0, 2.0)),
               dict(seed=(24, 28, 20)), dict(edge=-0.01)):
        info = dict(stages=True)
        got = BR.brainExtraction(I.astype(np.float32), info=info, **kw)
        ref, rinfo = M.extract(I.astype(np.float32), **kw)
        assert np.array_equal(got, ref), kw
        for k in M.STAGES:
            assert np.array_equal(info['stages'][k], rinfo['stages'][k]), (kw, k)
    # the scalp holds a component of its own after the erosion: a seed there keeps it, a seed in the gap is refused
    st = M.extract(I)[1]['stages']
    lab, n = ndi.label(st['eroded'], M.CROSS)
    assert n >= 2
    other = tuple(int(x) for x in np.argwhere((lab > 0) & ~st['main'])[0])
    assert np.array_equal(BR.brainExtraction(I, seed=other), M.extract(I, seed=other)[0])
    gap = tuple(int(x) for x in np.argwhere(~st['eroded'])[0])
    with pytest.raises(VrgError):
        BR.brainExtraction(I, seed=gap)


def _shells(shape):
    """Nested ellipsoids without a distance transform: brain 90 / 110, a gap at 15, scalp at 85, air at 0; float32."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float32) - (n - 1) / 2.0 for n in shape], indexing='ij', sparse=True)
    q = sum((g / (0.38 * n)) ** 2 for g, n in zip(grids, shape))
    I = np.zeros(shape, np.float32)
    I[q <= 1.32] = 85.0
    I[q <= 1.12] = 15.0
    I[q <= 1.0] = 90.0
    I[q <= 0.5] = 110.0
    I[shape[0] // 2, shape[1] // 2, shape[2] // 2:] = np.where(q[shape[0] // 2, shape[1] // 2, shape[2] // 2:] <= 1.32, 90.0, 0.0)
    return I, q <= 1.0


@pytest.mark.gpu
def test_extraction_256x256x192():
    """n2 = 192 is three whole words and n1 n2 exceeds every tile.  E against scipy's within 1e-9 of the span; steps 4-7 exactly,
    against scipy fed the device's own E, so that a rounding difference at the threshold cannot pass for a morphology fault."""
    shape = (256, 256, 192)
    I, brain = _shells(shape)
    E = BR.laplacianOfGaussian(I)
    dev = np.abs(E - M.log_scipy(I)).max() / float(np.ptp(I))
    print('max |E - scipy| / span {:.3e}'.format(dev))
    assert dev <= BAR
    info = dict(stages=True)
    got = BR.brainExtraction(I, info=info)
    st, ncomp = M.morphology(I, E, info['floor'], info['threshold'])
    for k in M.STAGES:
        assert np.array_equal(info['stages'][k], st[k]), k
        assert info['counts'][k] == int(st[k].sum()), k
    assert np.array_equal(got, st['final']) and info['components'] == ncomp
    lo, hi, counts = M.histogram(I)
    assert (info['floor'], info['contrast']) == M.floor_contrast(counts, lo, hi)[:2]
    assert M.dice(got, brain) >= 0.99


# ------------------------------------------------------------------ GPU: device pointers, in a process of their own
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import brain as BR
import brain_model as M
from test_brain import _noisy, _refusals, _masks, N_REFUSALS, SENTINEL
dev = torch.device('cuda', 0)

I, brain = M.head_phantom(M.PHANTOM_SHAPES[1], 55.0, 6, 0)
for dtype in (np.float64, np.float32):
    host = I.astype(dtype)
    t = torch.as_tensor(host, device=dev)
    info, hinfo = dict(stages=True), dict(stages=True)
    got = BR.brainExtraction(t, diffusion=M.DIFFUSION, info=info)
    ref = BR.brainExtraction(host, diffusion=M.DIFFUSION, info=hinfo)
    assert got.is_cuda and got.device == t.device and got.dtype == torch.uint8 and tuple(got.shape) == I.shape
    assert got.cpu().numpy().tobytes() == ref.tobytes()
    for k in M.STAGES:
        assert info['stages'][k].is_cuda and info['stages'][k].cpu().numpy().tobytes() == hinfo['stages'][k].tobytes(), k
    assert info['counts'] == hinfo['counts'] and info['floor'] == hinfo['floor'] and info['contrast'] == hinfo['contrast']
    assert BR.brainExtraction(t, diffusion=M.DIFFUSION).cpu().numpy().tobytes() == ref.tobytes()
    E = BR.laplacianOfGaussian(t, 1.0, (1.0, 1.0, 2.0))
    assert E.is_cuda and E.dtype == torch.float64 and E.cpu().numpy().tobytes() == BR.laplacianOfGaussian(host, 1.0, (1.0, 1.0, 2.0)).tobytes()
    assert BR.intensityFloor(t)[:4] == BR.intensityFloor(host)[:4] and np.array_equal(BR.intensityFloor(t)[4], BR.intensityFloor(host)[4])
    assert t.cpu().numpy().tobytes() == host.tobytes()          # the input is unchanged
assert M.dice(ref, brain) >= 0.99
print('EXTRACTION OK')

# a mask whose storage is not 8-byte aligned: a view that starts one byte into a buffer
shape = (5, 2, 129)
n = shape[0] * shape[1] * shape[2]
for m in _masks(shape, seed=9):
    buf = torch.zeros(n + 8, dtype=torch.uint8, device=dev)
    view = buf[1:1 + n].view(shape)
    view.copy_(torch.as_tensor(m, device=dev))
    assert view.data_ptr() % 8 == 1 and view.is_contiguous()
    for steps in (1, 3):
        for border in (0, 1):
            got = BR.binaryErosion(view, steps, border)
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), M.erode(m, steps, border))
        assert np.array_equal(BR.binaryDilation(view, steps).cpu().numpy(), M.dilate(m, steps))
    assert np.array_equal(BR.fillHoles(view).cpu().numpy(), BR.fillHoles(m)) and np.array_equal(BR.largestComponent(view).cpu().numpy(), BR.largestComponent(m))
    assert np.array_equal(view.cpu().numpy(), m)
print('UNALIGNED OK')

shape = (4, 5, 6)
a = torch.as_tensor(_noisy(shape), device=dev)
a32 = a.to(torch.float32)
msk = (a > 50).to(torch.uint8)
outs = [torch.full(shape, -12345.0, dtype=torch.float64, device=dev), torch.full(shape, SENTINEL, dtype=torch.uint8, device=dev),
        torch.full((1,), -12345.0, dtype=torch.float64, device=dev), torch.full((1,), -12345.0, dtype=torch.float64, device=dev),
        torch.full((256,), SENTINEL, dtype=torch.int64, device=dev), torch.full((1,), SENTINEL, dtype=torch.int64, device=dev),
        torch.full((5,) + shape, SENTINEL, dtype=torch.uint8, device=dev), torch.full((16,), SENTINEL, dtype=torch.int64, device=dev)]
torch.cuda.synchronize()
res = _refusals(BR._lib(), a.data_ptr(), a32.data_ptr(), msk.data_ptr(), shape, [o.data_ptr() for o in outs])
assert len(res) == N_REFUSALS
for label, rc in res:
    assert rc == -1, label
torch.cuda.synchronize()
assert all(bool((o == (-12345.0 if o.dtype == torch.float64 else SENTINEL)).all()) for o in outs)
assert a.cpu().numpy().tobytes() == _noisy(shape).tobytes()
print('REFUSALS OK')
"""


@functools.lru_cache(maxsize=None)
def _device_run():
    script = DEVICE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    return out.returncode, out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_brain_device_resident():
    """A tensor on the GPU goes in by its device pointer and stays there through the diffusion, the histogram and the extraction;
    a tensor on the same device comes out, with the bytes of the host call and of a second run.  Own process: torch is imported
    before the HIP library there."""
    rc, stdout, tail = _device_run()
    assert 'EXTRACTION OK' in stdout, tail


@pytest.mark.gpu
def test_morphology_with_an_unaligned_device_tensor():
    rc, stdout, tail = _device_run()
    assert 'UNALIGNED OK' in stdout, tail


@pytest.mark.gpu
def test_brain_refusals_with_device_pointers():
    """Every refused input of the six C entries, with device pointers: VRG_E_ARG, the sentinels in the outputs untouched."""
    rc, stdout, tail = _device_run()
    assert rc == 0 and 'REFUSALS OK' in stdout, tail


# ------------------------------------------------------------------ GPU: the files
@pytest.mark.gpu
def test_brain_main_writes_the_mask_and_the_brain(tmp_path, capsys):
    from arterynetwork_amd import nifti
    I, _ = _phantom(M.PHANTOM_SHAPES[1], 15.0, 3, 0)
    aff = np.array([[0.5, 0, 0, -10.0], [0, 0.5, 0, 3.0], [0, 0, 0.75, 7.5], [0, 0, 0, 1.0]])
    nifti.saveVolume(I, aff, str(tmp_path / 'headVolume.nii.gz'), astype=np.float32)
    mask = BR.main(str(tmp_path), sigma=0.75, diffusion=dict(conductance=20.0, iterations=3))
    said = capsys.readouterr().out
    for name in ('brainVolumeMask.nii.gz', 'brainVolume.nii.gz'):
        assert '{} saved to {}.'.format(name, os.path.join(str(tmp_path), name)) in said
    stored, aff2 = nifti.loadVolume(str(tmp_path), 'brainVolumeMask.nii.gz')
    volume, aff3 = nifti.loadVolume(str(tmp_path), 'brainVolume.nii.gz')
    head, _ = nifti.loadVolume(str(tmp_path), 'headVolume.nii.gz')
    assert stored.dtype == np.uint8 and np.array_equal(stored, mask) and np.allclose(aff2, aff) and np.allclose(aff3, aff)
    assert volume.dtype == np.float32 and np.array_equal(volume, head * mask) and mask.any() and not mask.all()
    # the spacing came from the affine's columns
    I32 = I.astype(np.float32)
    assert np.array_equal(mask, BR.brainExtraction(I32, sigma=0.75, diffusion=dict(conductance=20.0, iterations=3), spacing=(0.5, 0.5, 0.75)))
    assert np.array_equal(mask, M.extract(I32, sigma=0.75, diffusion=dict(conductance=20.0, iterations=3), spacing=(0.5, 0.5, 0.75))[0])
    assert not np.array_equal(mask, BR.brainExtraction(I32, sigma=0.75, diffusion=dict(conductance=20.0, iterations=3)))
    # other names
    BR.main(str(tmp_path), maskName='m.nii.gz', brainName='b.nii.gz', sigma=0.75)
    assert os.path.exists(str(tmp_path / 'm.nii.gz')) and os.path.exists(str(tmp_path / 'b.nii.gz'))
