"""Multiscale Hessian vesselness (DESIGN.md section 9 entry f7): the float64 model tests/vesselness_model.py is checked on the
CPU (explicit taps against scipy, known answers), then vmask_vesselness / vesselness.vesselnessFilter must agree with it to
1e-9 absolute outside the tie set, the measure's one discontinuity.  Noise-free phantoms, on which eigenvalues of the Hessian
coincide over whole regions, hold it to PHANTOM_BAR besides; the restated eigen-solves of the model file show on the CPU that the
phantoms tell a closed-form solve from a well-conditioned one."""
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


# ------------------------------------------------------------------ CPU: noise-free phantoms and the restated eigen-solves
# On noisy input two eigenvalues practically never coincide; on these they do, and a closed-form eigen-solve loses half its
# digits there.  (phantom, shape, variant); variant = (input dtype, gamma, mask, bright, spacing).
PHANTOM_VARIANTS = {'f64-g15': (np.float64, 15.0, False, True, None), 'f64-auto': (np.float64, None, False, True, None),
                    'f32-g15': (np.float32, 15.0, False, True, None), 'f64-auto-mask': (np.float64, None, True, True, None),
                    'f64-g15-dark': (np.float64, 15.0, False, False, None), 'f64-auto-aniso': (np.float64, None, False, True, (1.0, 1.0, 2.0))}
ONLY = {'f64-auto-mask': ('cube', 'ball'), 'f64-g15-dark': ('cube',), 'f64-auto-aniso': ('cube',)}
PHANTOM_CASES = [(ph, shape, v) for ph in M.PHANTOMS for shape in [(16, 16, 16), (17, 20, 9)] + ([(24, 24, 24)] if ph == 'blob' else [])
                 for v in PHANTOM_VARIANTS if ph in ONLY.get(v, M.PHANTOMS)]
CUBE_CASES = [('cube', shape, v) for shape in ((16, 16, 16), (17, 20, 9)) for v in ('f64-g15', 'f64-auto')]
# the least max V of a phantom's cases is 0.59 (cube), 0.39 (blob), 0.0081 (half-spaces: a step is a plate, not a vessel;
# what is left comes from the taps' sum), 0.70 (ball), 0.116 (voxel): not trivial means half of that, about
MIN_MAX_V = {'cube': 0.3, 'blob': 0.2, 'half0': 0.004, 'half2': 0.004, 'ball': 0.35, 'voxel': 0.05}
# The largest |V(restated eig3_deflation) - V(eigvalsh)| over PHANTOM_CASES on the CPU (numpy 2 / LAPACK eigvalsh) is
# PHANTOM_MEASURED; the kernel gets 100 times that: its FMA contraction and the other summation order of its taps, which on
# the noisy cases took the closed form from 2e-15 (restatement) to 1.1e-14 (GPU).  Four orders of magnitude below BAR.
PHANTOM_MEASURED = 7.3e-16                                 # 7.216e-16, at cube-16x16x16-f64-g15
PHANTOM_BAR = 100 * PHANTOM_MEASURED


def _case_id(case):
    return '{}-{}-{}'.format(case[0], 'x'.join(map(str, case[1])), case[2])


@functools.lru_cache(maxsize=None)
def _phantom_case(phantom, shape, variant):
    dtype, gamma, masked, bright, spacing = PHANTOM_VARIANTS[variant]
    I = (M.PHANTOMS[phantom](shape) * (1.0 if bright else -1.0)).astype(dtype)
    mask = M.cut_mask(shape) if masked else None
    kw = dict(gamma=gamma, mask=mask, spacing=spacing, bright=bright)
    ref = M.vesselness(I, SIGMAS, **kw)
    for a in (I,) + tuple(ref.values()) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    return I, kw, ref


def _restated_deviation(case, solver):
    I, kw, ref = _phantom_case(*case)
    got = M.vesselness(I, SIGMAS, solver=solver, **kw)
    assert np.isfinite(got['V']).all()
    return float(np.abs(got['V'] - ref['V'])[~ref['ties']].max())


@pytest.mark.parametrize('case', PHANTOM_CASES, ids=_case_id)
def test_phantom_cases_discriminate(case):
    """No GPU: a phantom case has its tie set under the cap (every one is empty), is not trivial, and the restated deflation
    solve agrees with eigvalsh on it - two independent float64 solvers, a tenth of PHANTOM_BAR being the room for another LAPACK."""
    I, kw, ref = _phantom_case(*case)
    assert ref['ties'].sum() <= TIE_CAP * ref['ties'].size
    assert ref['V'].max() > MIN_MAX_V[case[0]] and (ref['gammas'] > 0).all()
    if kw['mask'] is not None:                                  # the mask cuts through the phantom: response on both sides of its face
        full = M.vesselness(I, SIGMAS, gamma=15.0)['V']
        assert full[kw['mask'] != 0].max() > 0.1 and full[kw['mask'] == 0].max() > 0.1
    dev = _restated_deviation(case, M.eig3_deflation)
    print('{}: ties {}, max V {:.4f}, restated deflation solve against eigvalsh {:.3e}'.format(_case_id(case), int(ref['ties'].sum()), float(ref['V'].max()), dev))
    assert dev <= PHANTOM_BAR / 10


def test_phantom_bar_is_the_measured_one():
    """PHANTOM_MEASURED is what the restated solver deviates by over all the phantom cases, to a factor of 3 either way."""
    worst = max(_restated_deviation(case, M.eig3_deflation) for case in PHANTOM_CASES)
    print('largest deviation of the restated deflation solve over {} phantom cases: {:.3e}'.format(len(PHANTOM_CASES), worst))
    assert PHANTOM_MEASURED / 3 <= worst <= 3 * PHANTOM_MEASURED and PHANTOM_BAR <= 1e-3 * BAR


@pytest.mark.parametrize('case', CUBE_CASES, ids=_case_id)
def test_restated_closed_form_breaks_the_bar_on_cubes(case):
    """The closed trigonometric form, as the kernel had it, misses BAR on every cube case (8.4e-9, 5.1e-9, 2.1e-9, 1.2e-9):
    the phantoms tell the solvers apart.  On the suite's noisy input both stay below 1e-14."""
    dev = _restated_deviation(case, M.eig3_closed_form)
    print('{}: restated closed form against eigvalsh {:.3e}'.format(_case_id(case), dev))
    assert dev > BAR


def test_restated_solvers_agree_on_noisy_input():
    I, brain, gamma, spacing, ref = _case((17, 64, 9), 'f64-auto')
    for solver in (M.eig3_closed_form, M.eig3_deflation):
        got = M.vesselness(I, SIGMAS, solver=solver)
        assert np.abs(got['V'] - ref['V'])[~ref['ties']].max() <= 1e-14


def test_restated_solvers_on_degenerate_matrices():
    """Zero, multiples of the unit matrix, exact double eigenvalues on either side, diagonal and rotated: no NaN, ascending
    order, eigvalsh's values to a few ulp of the largest."""
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.normal(size=(200, 3, 3)))[0]
    H = [np.zeros((3, 3)), np.eye(3), -7.0 * np.eye(3), np.diag([1.0, 1.0, 2.0]), np.diag([2.0, 1.0, 1.0]), np.diag([1.0, 2.0, 1.0]),
         np.diag([-1.0, -1.0, 1.0]), np.ones((3, 3)), np.array([[0.0, 0.0, 2.0], [0.0, -2.0, 0.0], [2.0, 0.0, 0.0]])]
    for d in ([1.0, 1.0, 2.0], [-3.0, 1.0, 1.0], [1.0, 1.0 + 1e-9, 5.0], [1.0, 1.0, 1.0 + 1e-9], [0.0, 0.0, 1.0], [-2.0, 0.5, 3.0]):
        H += list(Q @ np.diag(d) @ Q.transpose(0, 2, 1))
    H = np.array(H)
    H = 0.5 * (H + H.transpose(0, 2, 1))
    ref = np.linalg.eigvalsh(H)
    scale = np.maximum(np.abs(ref).max(axis=-1), 1e-300)
    e = M.eig3_deflation(H)
    assert np.isfinite(e).all() and (np.diff(e, axis=-1) >= 0).all()
    assert (np.abs(e - ref).max(axis=-1) / scale).max() <= 16 * np.finfo(np.float64).eps
    closed = M.eig3_closed_form(H)                              # the closed form: finite as well, but 1e-8 off where two coincide
    assert np.isfinite(closed).all() and 1e-9 < (np.abs(closed - ref).max(axis=-1) / scale).max() < 1e-7


# ------------------------------------------------------------------ GPU
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


# ------------------------------------------------------------------ GPU: noise-free phantoms, known answers
@pytest.mark.gpu
@pytest.mark.parametrize('case', PHANTOM_CASES, ids=_case_id)
def test_vesselness_phantoms_match_model(case):
    """Coinciding eigenvalues over whole regions: BAR as everywhere, and the measured allowance PHANTOM_BAR."""
    I, kw, ref = _phantom_case(*case)
    info = {'scale': None}
    got = VS.vesselnessFilter(I, SIGMAS, gamma=kw['gamma'], brainVolumeMask=kw['mask'], spacing=kw['spacing'], bright=kw['bright'], info=info)
    dev = _compare(got, info, ref, _case_id(case))
    assert np.isfinite(got).all() and dev <= PHANTOM_BAR
    if kw['mask'] is not None:
        assert not got[kw['mask'] == 0].any()


@pytest.mark.gpu
def test_vesselness_zero_volume_and_empty_mask():
    """Automatic gamma without any structure: every gamma is 0 and every scale contributes 0 - on zeros, and on a noisy
    volume under a mask that is 0 everywhere."""
    noisy, brain = _input(0, (9, 8, 7))
    for volume, mask in ((np.zeros((9, 8, 7)), None), (np.zeros((9, 8, 7), np.float32), brain), (noisy, np.zeros_like(brain))):
        info = {'scale': None}
        got = VS.vesselnessFilter(volume, SIGMAS, brainVolumeMask=mask, info=info)
        assert got.dtype == np.float64 and got.shape == (9, 8, 7)
        assert not got.any() and not info['scale'].any() and not info['gammas'].any()


@pytest.mark.gpu
def test_vesselness_constant_volume():
    """Three equal eigenvalues at every voxel, none isolated: the closed-form value of test_model_known_answers."""
    lam = [7.0 * s * s * M.taps(s)[3].sum() for s in SIGMAS]
    expect = max((1 - np.exp(-2.0)) * np.exp(-2.0) * (1 - np.exp(-3 * l * l / 50.0)) for l in lam)
    for dtype in (np.float64, np.float32):
        info = {'scale': None}
        got = VS.vesselnessFilter(np.full((9, 8, 7), 7.0, dtype), SIGMAS, gamma=5.0, info=info)
        print('constant 7, {}: max |V - closed form| {:.3e} of {:.3e}'.format(np.dtype(dtype).name, float(np.abs(got - expect).max()), expect))
        assert np.isfinite(got).all() and np.abs(got - expect).max() < 1e-12
        assert (info['gammas'] == 5.0).all()


@functools.lru_cache(maxsize=None)
def _line_case(axis):
    line = M.gaussian_line((25, 25, 25), axis, 2.0)
    ref = M.vesselness(line, (1.0, 2.0, 4.0), gamma=10.0)
    for a in (line,) + tuple(ref.values()):
        a.setflags(write=False)
    return line, ref


@pytest.mark.parametrize('axis', range(3))
def test_model_line_tie_sets_are_small(axis):
    ref = _line_case(axis)[1]
    assert ref['ties'].sum() <= TIE_CAP * ref['ties'].size and ref['scale'][12, 12, 12] == 1 and ref['V'][12, 12, 12] > 0.8


@pytest.mark.gpu
@pytest.mark.parametrize('axis', range(3))
def test_vesselness_straight_line(axis):
    """A tube of Gaussian width 2 along each axis: l2 = l3 along its whole centre line; the middle scale wins there."""
    line, ref = _line_case(axis)
    info = {'scale': None}
    got = VS.vesselnessFilter(line, (1.0, 2.0, 4.0), gamma=10.0, info=info)
    dev = _compare(got, info, ref, 'line along axis {}'.format(axis))
    assert dev <= PHANTOM_BAR
    assert info['scale'][12, 12, 12] == 1 and got[12, 12, 12] > 0.8


@pytest.mark.gpu
def test_vesselness_repeated_scale_keeps_the_first():
    """`scale` is the first scale that attains the maximum: a scale given twice never shows its second index, and changes
    no bit of V."""
    I, brain, _, _, _ = _case((17, 64, 9), 'f64-auto')
    twice, once = {'scale': None}, {'scale': None}
    a = VS.vesselnessFilter(I, (1.0, 1.0, 2.5), info=twice)
    b = VS.vesselnessFilter(I, (1.0, 2.5), info=once)
    assert a.tobytes() == b.tobytes() and a.max() > 0.2
    assert not (twice['scale'] == 1).any() and (twice['scale'] == 2).any() and (twice['scale'] == 0).any()
    assert np.array_equal(twice['scale'] == 2, once['scale'] == 1)
    assert twice['gammas'][0] == twice['gammas'][1] == once['gammas'][0] and twice['gammas'][2] == once['gammas'][1]


# ------------------------------------------------------------------ GPU: column tiles and grids
# The widest column tile whose ring fits the LDS (col_geo): the axis-0 pass (six arrays) has TX = 64 up to r = 17, 32 up to
# r = 34, 16 up to r = 64; the axis-1 pass (three arrays) 64 up to r = 42, then 32.  6x37x131: two row segments along axis 2
# with the full halo, an odd row length, a column-tile tail on both column passes, every extent but one below the radius.
# id: (shape, sigma, input dtype, spacing)
GEOMETRY = {'r17': ((6, 37, 131), 4.2, np.float64, None), 'r34': ((6, 37, 131), 8.4, np.float64, None), 'r35': ((6, 37, 131), 8.7, np.float64, None),
            'r42': ((6, 37, 131), 10.4, np.float64, None), 'r43': ((6, 37, 131), 10.7, np.float64, None), 'r64': ((6, 37, 131), 15.9, np.float64, None),
            # an even row length; the axis-0 ring of 2 * 64 + 64 rows advances (70 rows: two steps)
            'r64-ring': ((70, 20, 130), 15.9, np.float64, None),
            # radii 8, 16 and 32 in one call
            'r8-16-32': ((12, 40, 140), 4.0, np.float64, (2.0, 1.0, 0.5)),
            # more than 32768 blocks: 32 852 column tiles in the axis-0 pass (grid.y = 2, dead blocks at the tail); 33 215 row blocks in the axis-2 pass
            'fold-axis0': ((1, 1450, 1450), 1.0, np.float32, None), 'fold-axis2': ((365, 364, 4), 1.0, np.float32, None)}


@functools.lru_cache(maxsize=None)
def _geometry_case(name):
    shape, sigma, dtype, spacing = GEOMETRY[name]
    I = _input(SEEDS.get(shape, 0), shape)[0].astype(dtype)
    ref = M.vesselness(I, (sigma,), spacing=spacing)
    for a in (I,) + tuple(ref.values()):
        a.setflags(write=False)
    return I, ref


def test_geometry_cases_take_the_paths_they_name():
    """No GPU: the radii, the number of column tiles and of row blocks that the comments above promise."""
    radius = lambda name, a: int(4.0 * GEOMETRY[name][1] / (GEOMETRY[name][3] or (1.0, 1.0, 1.0))[a] + 0.5)
    assert [radius(n, 0) for n in ('r17', 'r34', 'r35', 'r42', 'r43', 'r64', 'r64-ring')] == [17, 34, 35, 42, 43, 64, 64]
    assert [radius('r8-16-32', a) for a in range(3)] == [8, 16, 32]
    lds = lambda arrays, r, tx: arrays * (2 * r + 1024 // tx) * tx * 8
    for arrays, r, tx in ((6, 17, 64), (6, 34, 32), (3, 42, 64)):       # the last radius of a tile width; 64, the largest legal one, fits the next
        assert lds(arrays, r, tx) <= 152 * 1024 < lds(arrays, r + 1, tx)
    assert lds(6, 64, 16) <= 152 * 1024 and lds(3, 64, 32) <= 152 * 1024
    assert -(-1450 * 1450 // 64) == 32852 and -(-365 * 364 // 4) == 33215


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_vesselness_tiles_and_grids(name):
    shape, sigma, dtype, spacing = GEOMETRY[name]
    I, ref = _geometry_case(name)
    info = {'scale': None}
    got = VS.vesselnessFilter(I, (sigma,), spacing=spacing, info=info)
    _compare(got, info, ref, '{} {} sigma {}'.format(name, 'x'.join(map(str, shape)), sigma))
    assert ref['V'].max() > 0.01


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
