"""Nonlinear registration (DESIGN.md section 9 entry f18).  On the CPU: what the numpy model tests/warp_model.py states - the sampler
at a zero warp is the affine one, the interpolant's gradient, Thirion's bound, the recovery of a known deformation -, the refusals,
the kernels' resource records, the 4-D NIfTI round trip.  On the GPU: the force pass, the three-numerator fit, the upsampled warp,
the resampled volumes and ``registerNonlinear``'s warp and trace must be the model's bits."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import registration_model as RM
import warp_model as M
from conftest import ROOT
from arterynetwork_amd import bias as B
from arterynetwork_amd import registration as R
from arterynetwork_amd.registration import registerNonlinear, warpResample          # (what this file is about)

# csrc/vwarp_device.hip (test_extents_are_the_kernels reads them): WT threads take WT consecutive (i1, i2) columns in k_warp_force,
# k_warp_fit and k_warp_expand, WT values of i2 in k_warp_rows; k_warp_expand0 marches over WZ planes of axis 0; k_warp_up,
# k_warp_linear and k_warp_nearest stride over at most WGRID workgroups, so their second trip begins at voxel WGRID * WT
WT, WZ, WGRID = 256, 32, 1024
SECOND_TRIP = WGRID * WT


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _noise(shape, seed, dtype=np.float64):
    return (100.0 + 30.0 * np.random.default_rng(seed).standard_normal(shape)).astype(dtype)


def _smooth(shape, seed, dtype=np.float64):
    """A volume with structure on every axis that has more than one voxel, and a little noise."""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape], indexing='ij')
    v = 100.0 + 60.0 * g[0] - 40.0 * g[1] * g[2] + 30.0 * np.sin(3.0 * g[1] + 2.0 * g[2]) + 5.0 * np.random.default_rng(seed).standard_normal(shape)
    return v.astype(dtype)


def _warp(shape, seed, size=1.5):
    return size * np.random.default_rng(seed).uniform(-1.0, 1.0, (3,) + tuple(shape))


def _scaled(n, m, shift=(0.0, 0.0, 0.0)):
    """The fixed grid stretched over the moving one, with a shift in moving voxels."""
    T = np.eye(4)
    for a in range(3):
        T[a, a] = (m[a] - 1.0) / (n[a] - 1.0) if n[a] > 1 else 0.0
        T[a, 3] = shift[a]
    return T


def _rotated(n, m, degrees=10.0):
    """Rotation and anisotropic scale onto another grid."""
    fA, mA = RM.affine_of((0.8, 1.0, 1.6), n), RM.affine_of((1.3, 0.9, 1.1), m, centre_at=(0.4, -0.3, 0.2))
    W = R.paramsToMatrix([0.7, -0.4, 0.3] + [np.deg2rad(degrees)] * 3, 6, np.zeros(3))
    return R.voxelMap(W, fA, mA)


def _turned(n, m, degrees=25.0, shrink=1.1):
    """The fixed grid scaled to `shrink` of the moving one's extent and turned about the two centres by `degrees` on every axis: no
    coefficient of the map is zero, and at 1.1 voxels all over the fixed grid, the last ones in raster order too, lie inside and outside."""
    rot = R.paramsToMatrix([0.0, 0.0, 0.0] + [np.deg2rad(degrees)] * 3, 6, np.zeros(3))[:3, :3]
    scale = np.array([shrink * (m[a] - 1.0) / (n[a] - 1.0) if n[a] > 1 else 0.0 for a in range(3)])
    T = np.eye(4)
    T[:3, :3] = rot * scale[None, :]
    T[:3, 3] = (np.array(m) - 1.0) / 2.0 - T[:3, :3] @ ((np.array(n) - 1.0) / 2.0)
    return T


def _scales(fixed, moving):
    flo, fhi = RM.extrema(fixed)
    mlo, mhi = RM.extrema(moving)
    return flo, R.binScale(flo, fhi, 1), mlo, R.binScale(mlo, mhi, 1)


# ------------------------------------------------------------------ CPU: a zero warp is the affine sampler
def test_model_with_a_zero_warp_samples_as_the_affine_model():
    n, m = (9, 11, 13), (8, 12, 10)
    for dtype in (np.float32, np.float64):
        moving = _noise(m, 1, dtype)
        moving[2, 3, 4] = np.nan
        for T in (np.eye(4), _scaled(n, m, (0.5, -0.5, 0.5)), _rotated(n, m)):
            value, ok = M.sample(moving, T, np.zeros((3,) + n))
            want, want_ok = RM.sample(moving, T, n)
            assert np.array_equal(ok, want_ok) and np.array_equal(_bits(value[ok]), _bits(want[ok]))
            delta, part, S, count = M.force(_noise(n, 2), moving, T, np.zeros((3,) + n), 0.0, 0.01, 0.0, 0.01)
            assert np.array_equal(part != 0, want_ok) and count == int(want_ok.sum())
            for order, mv, fill in ((1, moving, -3.0), (0, moving, -3.0), (0, np.nan_to_num(moving).astype(np.int16), 7)):
                assert _same(M.resample(mv, T, np.zeros((3,) + n), order, fill), RM.resample(mv, T, n, order, fill))
            assert _same(M.resample(moving, T, -np.zeros((3,) + n), 1, 0.0), RM.resample(moving, T, n, 1, 0.0))      # u = -0.0 too


# ------------------------------------------------------------------ CPU: the gradient
def test_model_gradient_is_the_central_difference_of_its_sampler():
    """Inside one cell the interpolant is linear along each axis, so a central difference whose two points stay in the cell has no
    truncation error; what is left is rounding.  The points are k / 64 inside their cell and h = 2^-10, so p, p + h and p - h and
    the fractions t are exact.  A sample is three nested steps lo + t (hi - lo) of three roundings each on values of at most
    2 V in size (V = max |moving|): its error is at most 9 x 2 V x 2^-53 x 2 = 36 V 2^-53 (the factor 2: an error made early is
    carried, with weight at most 1, through the later steps - a loose bound).  The difference of two samples over 2 h carries
    36 V 2^-53 / h; the gradient itself is built from the same steps on differences of at most 2 V: another 72 V 2^-53.
    tolerance = 36 V 2^-53 / h + 72 V 2^-53, about 4e-10 at V = 250."""
    m = (7, 6, 8)
    rng = np.random.default_rng(3)
    moving = _noise(m, 4)
    h = 2.0 ** -10
    cells = np.stack([rng.integers(0, e - 1, 500) for e in m])
    p = [cells[a] + rng.integers(8, 57, 500) / 64.0 for a in range(3)]
    value, ok, g = M.interpolant(moving, p)
    assert ok.all()
    V = float(np.abs(moving).max())
    tol = 36.0 * V * 2.0 ** -53 / h + 72.0 * V * 2.0 ** -53
    worst = 0.0
    for a in range(3):
        up, dn = [x.copy() for x in p], [x.copy() for x in p]
        up[a] = up[a] + h
        dn[a] = dn[a] - h
        fd = (M.interpolant(moving, up)[0] - M.interpolant(moving, dn)[0]) / (2.0 * h)
        worst = max(worst, float(np.abs(fd - g[a]).max()))
        assert np.abs(g[a]).max() > 1.0
    print('worst |central difference - gradient| = {:.3e}, allowed {:.3e}'.format(worst, tol))
    assert worst <= tol
    flat = M.interpolant(np.full(m, 42.0), p)
    assert all(not x.any() for x in flat[2]) and (flat[0] == 42.0).all()          # exactly 0 on a constant volume
    n = (5, 6, 7)
    delta, part, S, count = M.force(np.full(n, 42.0), np.full(n, 42.0), np.eye(4), _warp(n, 5, 0.4), 42.0, 0.0, 42.0, 0.0)
    assert not delta.any() and S == 0.0 and 0 < count == int(part.sum())           # den == 0: no force, and the voxel takes part


# ------------------------------------------------------------------ CPU: Thirion's bound
def test_model_force_never_exceeds_max_step():
    for seed, maxStep, n, m in ((0, 0.5, (9, 10, 11), (10, 9, 12)), (1, 0.1, (6, 7, 8), (6, 7, 8)), (2, 2.0, (12, 5, 9), (7, 8, 6))):
        fixed, moving = _noise(n, seed), _noise(m, seed + 10, np.float32)
        for T in (_scaled(n, m), _rotated(n, m)):
            delta, part, S, count = M.force(fixed, moving, T, _warp(n, seed + 20), *_scales(fixed, moving), maxStep=maxStep)
            size = np.sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2])
            assert count > 20 and size.max() > 0.2 * maxStep
            assert size.max() <= maxStep, (seed, size.max())
            assert not delta[:, part == 0].any()


# ------------------------------------------------------------------ CPU: recovery of a known deformation
# The three-class phantom with vessels and a smooth texture under a smooth warp of 2.5 voxels at its peak (half a sine period per
# axis: coarser than any lattice of the run), intensities 0.7 v + 20, Gaussian noise of 1 % of the range; the mask is the tissue.
# name: (deformed_pair's arguments, registerNonlinear's).  RATIOS: the mean end-point error over the mask after the run, over the one
# with u = 0 and the same W, measured with the model on the CPU when this was written; the bar is twice that, and never 1 or more.
RECOVERY = {'same grid': (dict(), dict()),
            'another grid and affine': (dict(other_grid=True, seed=1), dict()),
            'two levels': (dict(seed=2), dict(levels=2, iterations=20))}
RATIOS = {'same grid': 0.520, 'another grid and affine': 0.322, 'two levels': 0.483}


def _case(name):
    pair_kw, run_kw = RECOVERY[name]
    fixed, fA, moving, mA, W, truth = M.deformed_pair(**pair_kw)
    mask = (fixed > 50.0).astype(np.uint8)
    return fixed, moving, dict(W=W, fixedAffine=fA, movingAffine=mA, fixedMask=mask, **run_kw), truth


@functools.lru_cache(maxsize=None)
def _model_run(name):
    fixed, moving, kw, _ = _case(name)
    warp, trace = M.register_nonlinear(fixed, moving, **kw)
    warp.setflags(write=False)
    trace.setflags(write=False)
    return warp, trace


@pytest.mark.parametrize('name', sorted(RECOVERY))
def test_model_recovers_a_known_deformation(name):
    fixed, moving, kw, truth = _case(name)
    warp, trace = _model_run(name)
    T = R.voxelMap(kw['W'], kw['fixedAffine'], kw['movingAffine'])
    before = M.end_point_error(np.zeros_like(truth), truth, T, kw['fixedMask'])
    after = M.end_point_error(warp, truth, T, kw['fixedMask'])
    print('{}: mean end-point error {:.3f} -> {:.3f} moving voxels, ratio {:.3f}; cost {:.3e} -> {:.3e} in {} iterations'.format(
        name, before, after, after / before, trace[0, 1], trace[-1, 1], len(trace)))
    assert before > 1.0 and after < before
    assert after / before <= min(2.0 * RATIOS[name], 0.999)
    assert trace[-1, 1] < trace[0, 1]                                     # the cost ends below its first value
    assert warp.shape == (3,) + fixed.shape and trace.shape[1] == 4 and (np.diff(trace[:, 0]) >= 0).all()
    assert (trace[:, 2] > 0).all() and (trace[:, 2] == np.floor(trace[:, 2])).all()


# ------------------------------------------------------------------ CPU: refusals
def test_argument_errors_raise():
    """What the host can check is refused before a device is looked for: no GPU needed."""
    f, m = np.zeros((9, 8, 10)), np.zeros((8, 8, 8))
    nan = float('nan')
    bad = [dict(fixed=np.zeros((9, 8))), dict(moving=np.zeros((2, 8, 8, 8))), dict(fixedMask=np.ones((9, 8, 9))), dict(W=np.eye(3)), dict(W=np.zeros((4, 4))),
           dict(fixedAffine=np.full((4, 4), nan)), dict(movingAffine=np.eye(2)), dict(splineSpans=(2, 2)), dict(splineSpans=(0, 2, 2)), dict(splineSpans=(65, 2, 2)),
           dict(splineSpans=(1.5, 2, 2)), dict(levels=0), dict(levels=9), dict(iterations=0), dict(iterations=201), dict(maxStep=0.0), dict(maxStep=-1.0),
           dict(maxStep=nan), dict(maxStep=float('inf')), dict(convergenceThreshold=0.0), dict(convergenceThreshold=nan)]
    for kw in bad:
        args = dict(fixed=f, moving=m)
        args.update(kw)
        with pytest.raises(ValueError):
            registerNonlinear(**args)
    u = np.zeros((3, 9, 8, 10))
    for kw in (dict(warp=np.zeros((9, 8, 10))), dict(warp=np.zeros((2, 9, 8, 10))), dict(order=2), dict(W=np.eye(3)), dict(moving=np.zeros((8, 8))),
               dict(moving=np.zeros((8, 8, 8), np.int64), order=0), dict(moving=np.zeros((8, 8, 8), np.uint8), order=0, fill=256),
               dict(moving=np.zeros((8, 8, 8), np.int16), order=0, fill=0.5)):
        args = dict(moving=m, W=None, warp=u)
        args.update(kw)
        with pytest.raises(ValueError):
            warpResample(**args)
    for kw in (dict(warp=np.zeros((3, 9, 8, 9))), dict(T=np.eye(2)), dict(T=np.full((3, 4), nan)), dict(flo=nan), dict(fs=float('inf')), dict(mlo=nan), dict(ms=nan),
               dict(maxStep=0.0), dict(mask=np.ones((9, 8, 9))), dict(fixed=np.zeros((9, 8))), dict(moving=np.zeros((8, 8)))):
        args = dict(fixed=f, moving=m, T=np.eye(4), warp=u, flo=0.0, fs=1.0, mlo=0.0, ms=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            R.forcePass(**args)
        args.update(spans=(2, 2, 2))
        with pytest.raises(ValueError):
            R.warpLevel(**args)
    for kw in (dict(spans=(0, 1, 1)), dict(spans=(65, 1, 1)), dict(iterations=0), dict(iterations=201), dict(convergenceThreshold=0.0)):
        args = dict(fixed=f, moving=m, T=np.eye(4), warp=u, flo=0.0, fs=1.0, mlo=0.0, ms=1.0, spans=(2, 2, 2))
        args.update(kw)
        with pytest.raises(ValueError):
            R.warpLevel(**args)
    for args in ((np.zeros((9, 8, 10)), np.ones((9, 8, 10)), (1, 1, 1)), (u, np.ones((9, 8, 9)), (1, 1, 1)), (u, np.ones((9, 8, 10)), (0, 1, 1)), (u, np.ones((9, 8, 10)), (1, 1))):
        with pytest.raises(ValueError):
            R.fitForces(*args)
    for args in ((np.zeros((9, 8, 10)), (4, 4, 4)), (u, (4, 4)), (u, (4, 0, 4))):
        with pytest.raises(ValueError):
            R.upsampleWarp(*args)
    with pytest.raises(ValueError):
        R.mainNonlinear('.', None)
    with pytest.raises(ValueError):
        R.mainNonlinear('.', 'other.nii.gz', W=np.eye(4))


SENTINEL = 0xA5
VALUE = -12345.0


def _refusals(dll, p, shape, mshape):
    """Every refused input of the C entries: (label, return code).  `p` holds the addresses of a float64 fixed volume, a uint8 mask
    and a float64 warp [3] of `shape`, of float64 and uint8 volumes of `mshape`, of the outputs delta ([3] float64), part (uint8), phi
    ([3][4][4][4] float64), fine ([3] float64), out (float64), u (a float64 warp that the loop would update), and - host pointers
    always - S, count, trace, ntrace."""
    keep = []

    def T(*rows):
        keep.append(np.ascontiguousarray(np.array(rows if rows else np.eye(4)[:3], dtype=np.float64)))
        return keep[-1].ctypes.data

    def ints(*values):
        keep.append(np.array(values, dtype=np.intc))
        return keep[-1].ctypes.data
    nan, inf = float('nan'), float('inf')
    bad_T = np.eye(4)[:3].copy()
    bad_T[1, 2] = nan
    inf_T = np.eye(4)[:3].copy()
    inf_T[2, 3] = inf
    huge = (2000, 2000, 600)

    def force(label, fixed=p['fixed'], fdtype=6, mask=p['mask'], n=shape, u=p['warp'], mov=p['f64'], mdtype=6, m=mshape, t=None, flo=0.0, fs=1.0, mlo=0.0,
              ms=1.0, step=0.5, delta=p['delta'], part=p['part'], S=p['S'], count=p['count']):
        t = T() if t is None else t
        return 'force ' + label, dll.vmask_warp_force(0, fixed, fdtype, mask, *n, u, mov, mdtype, *m, t, flo, fs, mlo, ms, step, delta, part, S, count)

    def field(label, fixed=p['fixed'], fdtype=6, mask=p['mask'], n=shape, mov=p['f64'], mdtype=6, m=mshape, t=None, flo=0.0, fs=1.0, mlo=0.0, ms=1.0,
              spans=(1, 1, 1), iterations=3, step=0.5, threshold=0.01, u=p['u']):
        t = T() if t is None else t
        s = ints(*spans) if spans is not None else None
        return 'field ' + label, dll.vmask_warp_field(0, fixed, fdtype, mask, *n, mov, mdtype, *m, t, flo, fs, mlo, ms, s, iterations, step, threshold, u, p['trace'], p['ntrace'])

    def fit(label, delta=p['warp'], part=p['mask'], n=shape, spans=(1, 1, 1), phi=p['phi']):
        return 'fit ' + label, dll.vmask_warp_fit(0, delta, part, *n, ints(*spans) if spans is not None else None, phi)

    def up(label, coarse=p['warp'], c=shape, fine=p['fine'], n=shape):
        return 'upsample ' + label, dll.vmask_warp_upsample(0, coarse, *c, fine, *n)

    def resample(label, v=p['f64'], dtype=6, m=mshape, t=None, u=p['warp'], order=1, fill=0.0, out=p['out'], n=shape):
        t = T() if t is None else t
        return 'resample ' + label, dll.vmask_warp_resample(0, v, dtype, *m, t, u, order, fill, out, *n)
    res = [force('null fixed', fixed=None), force('null warp', u=None), force('null moving', mov=None), force('null T', t=0), force('null delta', delta=None),
           force('null part', part=None), force('null S', S=None), force('null count', count=None), force('fixed dtype 0', fdtype=0), force('moving dtype 4', mdtype=4),
           force('moving dtype 7', mdtype=7), force('T nan', t=T(*bad_T)), force('T inf', t=T(*inf_T)), force('flo nan', flo=nan), force('fs inf', fs=inf),
           force('mlo nan', mlo=nan), force('ms inf', ms=inf), force('step 0', step=0.0), force('step -1', step=-1.0), force('step nan', step=nan),
           force('step inf', step=inf), force('step 1e-200', step=1e-200), force('fixed extent 0', n=(shape[0], 0, shape[2])), force('fixed envelope', n=huge),
           force('moving extent 0', m=(0, mshape[1], mshape[2])), force('moving envelope', m=huge), force('moving extent 32001', m=(32001, 1, 1))]
    res += [field('null fixed', fixed=None), field('null moving', mov=None), field('null T', t=0), field('null spans', spans=None), field('null warp', u=None),
            field('spans 0', spans=(1, 0, 1)), field('spans 65', spans=(1, 1, 65)), field('iterations 0', iterations=0), field('iterations 201', iterations=201),
            field('threshold 0', threshold=0.0), field('threshold nan', threshold=nan), field('threshold inf', threshold=inf), field('step 0', step=0.0),
            field('step inf', step=inf), field('fixed dtype 3', fdtype=3), field('moving dtype 1', mdtype=1), field('T nan', t=T(*bad_T)), field('ms nan', ms=nan),
            field('flo inf', flo=inf), field('fixed extent 0', n=(0, 1, 1)), field('fixed envelope', n=huge), field('moving envelope', m=huge)]
    res += [fit('null delta', delta=None), fit('null part', part=None), fit('null spans', spans=None), fit('null phi', phi=None), fit('spans 0', spans=(0, 1, 1)),
            fit('spans 65', spans=(1, 65, 1)), fit('extent 0', n=(1, 0, 1)), fit('envelope', n=huge)]
    res += [up('null coarse', coarse=None), up('null fine', fine=None), up('coarse extent 0', c=(0, 1, 1)), up('coarse envelope', c=huge), up('fine extent 0', n=(1, 1, 0)),
            up('fine envelope', n=huge)]
    res += [resample('null moving', v=None), resample('null T', t=0), resample('null warp', u=None), resample('null out', out=None), resample('order 2', order=2),
            resample('order -1', order=-1), resample('order 1 of uint8', v=p['u8'], dtype=0), resample('order 0 of int64', dtype=4, order=0),
            resample('order 0 of uint16', dtype=2, order=0), resample('T nan', t=T(*bad_T)), resample('T inf', t=T(*inf_T), order=0),
            resample('fill 256 of uint8', v=p['u8'], dtype=0, order=0, fill=256.0), resample('fill 0.5 of int16', dtype=1, order=0, fill=0.5),
            resample('fill nan of int32', dtype=3, order=0, fill=nan), resample('moving extent 0', m=(1, 0, 1)), resample('moving envelope', m=huge),
            resample('fixed extent 0', n=(0, 1, 1)), resample('fixed envelope', n=huge)]
    return res


N_REFUSALS = 27 + 22 + 8 + 6 + 18


def _host_outputs():
    return dict(S=np.full(1, VALUE), count=np.full(1, -777, np.int64), trace=np.full((3, 3), VALUE), ntrace=np.full(1, -777, np.int64))


def test_c_entries_refuse_before_a_device_is_looked_for():
    """Host pointers, no GPU needed: every refusal is VRG_E_ARG and leaves the outputs alone."""
    dll = R._lib()
    shape, mshape = (4, 5, 6), (3, 4, 5)
    a = dict(fixed=np.ones(shape), mask=np.ones(shape, np.uint8), warp=np.zeros((3,) + shape), f64=np.ones(mshape), u8=np.ones(mshape, np.uint8),
             delta=np.full((3,) + shape, VALUE), part=np.full(shape, SENTINEL, np.uint8), phi=np.full((3, 4, 4, 4), VALUE), fine=np.full((3,) + shape, VALUE),
             out=np.full(shape, VALUE), u=np.full((3,) + shape, VALUE), **_host_outputs())
    res = _refusals(dll, {k: v.ctypes.data for k, v in a.items()}, shape, mshape)
    assert len(res) == N_REFUSALS
    for label, rc in res:
        assert rc == -1, label                               # VRG_E_ARG
    for k in ('delta', 'phi', 'fine', 'out', 'u', 'S', 'trace'):
        assert (a[k] == VALUE).all(), k
    assert (a['part'] == SENTINEL).all() and a['count'][0] == -777 and a['ntrace'][0] == -777
    assert (a['fixed'] == 1.0).all() and not a['warp'].any()
    import ctypes
    host = np.full(4, VALUE)
    assert dll.vmask_reg_fetch(None, host.ctypes.data, 8) == -1 and dll.vmask_reg_fetch(ctypes.c_void_p(host.ctypes.data), None, 8) == -1
    assert dll.vmask_reg_fetch(ctypes.c_void_p(host.ctypes.data), host.ctypes.data, 0) == -1 and (host == VALUE).all()


# ------------------------------------------------------------------ no GPU needed: the kernels
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vwarp_device.hip')


def test_extents_are_the_kernels():
    text = open(SOURCE).read()
    assert int(re.search(r'constexpr int WT = (\d+);', text).group(1)) == WT
    assert int(re.search(r'constexpr int WZ = (\d+);', text).group(1)) == WZ
    assert int(re.search(r'constexpr int WGRID = (\d+);', text).group(1)) == WGRID


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_warp_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vwarp_device.hip' in build.SOURCES
    out = tmp_path / 'vwarp_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vwarp_device.hip'],
                       cwd=os.path.dirname(SOURCE), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    counts = {k: sum(k in name for name in recs) for k in ('k_warp_force', 'k_warp_rows', 'k_warp_fit', 'k_warp_expand', 'k_warp_up', 'k_warp_linear', 'k_warp_nearest')}
    # ("k_warp_expand" is in the names of k_warp_expand and k_warp_expand0)
    assert counts == dict(k_warp_force=4, k_warp_rows=1, k_warp_fit=3, k_warp_expand=2, k_warp_up=1, k_warp_linear=2, k_warp_nearest=5), sorted(recs)
    assert len(recs) == 18, sorted(recs)
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        # the cross-compile gives: k_warp_force 55 (float32, float32), 62, 53 and 60 (float64, float64); k_warp_fit 54 (first pass), 56 and 56;
        # k_warp_up 48; k_warp_linear 41 and 44; k_warp_nearest 30 to 32; k_warp_expand 20, k_warp_expand0 24; k_warp_rows 14.  64 is the
        # next multiple of 8 above the largest: eight waves a SIMD stay possible
        assert vgprs <= 64, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ no GPU needed: the warp's file
def test_nifti_round_trips_a_4d_warp(tmp_path):
    from arterynetwork_amd import nifti
    warp = _warp((5, 6, 7), 9).astype(np.float32)
    stored = np.moveaxis(warp, 0, 3)
    affine = RM.affine_of((0.8, 1.0, 1.6), (5, 6, 7), centre_at=(1.0, 2.0, 3.0))
    for name in ('warp.nii.gz', 'warp.nii'):
        path = os.path.join(str(tmp_path), name)
        nifti.saveVolume(stored, affine, path, astype=np.float32)
        back, aff = nifti.loadVolume(str(tmp_path), name)
        assert back.shape == (5, 6, 7, 3) and back.dtype == np.float32 and np.array_equal(back, stored) and np.allclose(aff, affine)
        assert nifti.read(path)[2]['dim'][:5] == (4, 5, 6, 7, 3)
        assert np.array_equal(np.moveaxis(back, 3, 0), warp)
    volume = np.arange(24, dtype=np.int16).reshape(2, 3, 4)                  # a 3-D volume is stored as before
    nifti.saveVolume(volume, affine, os.path.join(str(tmp_path), 'v.nii.gz'), astype=np.int16)
    assert nifti.read(os.path.join(str(tmp_path), 'v.nii.gz'))[2]['dim'][:5] == (3, 2, 3, 4, 1)
    assert np.array_equal(nifti.loadVolume(str(tmp_path), 'v.nii.gz')[0], volume)


# ------------------------------------------------------------------ GPU: the force pass
def _check_force(fixed, moving, T, u, mask=None, maxStep=0.5, scales=None, label=''):
    scales = _scales(fixed, moving) if scales is None else scales
    before = (fixed.copy(), moving.copy(), u.copy())
    want = M.force(fixed, moving, T, u, *scales, maxStep=maxStep, mask=mask)
    got = R.forcePass(fixed, moving, T, u, *scales, maxStep=maxStep, mask=mask)
    assert got[0].dtype == np.float64 and got[0].shape == (3,) + fixed.shape and got[1].dtype == np.uint8, label
    assert np.array_equal(got[1], want[1]), '{}: part differs at {} voxels'.format(label, int((got[1] != want[1]).sum()))
    assert np.array_equal(_bits(got[0]), _bits(want[0])), '{}: delta differs at {} values'.format(label, int((_bits(got[0]) != _bits(want[0])).sum()))
    assert got[3] == want[3] and np.array_equal(_bits(got[2]), _bits(want[2])), (label, got[2:], want[2:])
    again = R.forcePass(fixed, moving, T, u, *scales, maxStep=maxStep, mask=mask)
    assert _same(again[0], got[0]) and _same(again[1], got[1]) and again[2:] == got[2:], label          # a repeat is identical
    assert _same(fixed, before[0]) and _same(moving, before[1]) and _same(u, before[2]), label
    return got


# (2, 15, 17): 255 columns; (3, 16, 16): 256; (3, 257, 1): 257, a second workgroup of one column; (2, 1, 257): k_warp_rows' second workgroup
FORCE_SHAPES = [(1, 1, 9), (9, 1, 1), (5, 7, 3), (17, 16, 15), (2, 15, 17), (3, 16, 16), (3, 257, 1), (2, 1, 257), (2, 2, 257)]
MOVING_SHAPES = [(7, 6, 5), (1, 6, 5), (7, 1, 5), (7, 6, 1), (1, 1, 1)]


def test_force_shapes_are_around_the_workgroup():
    assert [s[1] * s[2] for s in FORCE_SHAPES[4:8]] == [WT - 1, WT, WT + 1, WT + 1] and FORCE_SHAPES[7][2] == WT + 1 and FORCE_SHAPES[8][1] * FORCE_SHAPES[8][2] > 2 * WT


@pytest.mark.gpu
@pytest.mark.parametrize('n', FORCE_SHAPES, ids=['x'.join(map(str, s)) for s in FORCE_SHAPES])
def test_force_pass_is_the_model_at_every_shape(n):
    counted = 0
    for k, m in enumerate(MOVING_SHAPES):
        fixed = _smooth(n, 1 + k, np.float32 if k % 2 else np.float64)
        moving = _smooth(m, 10 + k, np.float64 if k % 3 else np.float32)
        mask = (np.random.default_rng(k).random(n) < 0.6).astype(np.uint8)
        for label, T in (('stretched', _scaled(n, m)), ('half a voxel', _scaled(n, m, (0.5, -0.5, 0.5))), ('rotated', _rotated(n, m))):
            for u in (np.zeros((3,) + n), _warp(n, 20 + k, 0.8)):
                for msk in (None, mask):
                    got = _check_force(fixed, moving, T, u, msk, label='{} {} {} mask {}'.format(n, m, label, msk is not None))
                    counted += got[3]
                    if label == 'stretched' and not u.any():
                        assert got[3] == (int(np.prod(n)) if msk is None else int(mask.sum()))          # every voxel of the mask is inside
    assert counted > 0


@pytest.mark.gpu
def test_force_pass_borders_non_finite_values_and_a_vanishing_denominator():
    n = (6, 7, 8)
    V = int(np.prod(n))
    v = _smooth(n, 3)
    zero = np.zeros((3,) + n)
    planes = [V // e for e in n]
    assert _check_force(v, v, np.eye(4), zero, label='p = 0 and p = m - 1')[3] == V
    for a in range(3):
        T = np.eye(4)
        T[a, 3] = -5e-324                                        # p = -5e-324 at index 0 (outside), p = i at i > 0
        assert _check_force(v, v, T, zero, label='one ulp below 0 on axis %d' % a)[3] == V - planes[a]
        T[a, 3] = np.spacing(float(n[a] - 1))                    # p = nextafter(m - 1) at the last index (outside)
        assert _check_force(v, v, T, zero, label='one ulp above m - 1 on axis %d' % a)[3] == V - planes[a]
        u = zero.copy()                                          # the same through the warp: the last plane one ulp beyond, the first on 0 from -1
        np.moveaxis(u[a], a, 0)[-1] = np.spacing(float(n[a] - 1))
        assert _check_force(v, v, np.eye(4), u, label='the warp one ulp above m - 1 on axis %d' % a)[3] == V - planes[a]
        u = zero.copy()
        np.moveaxis(u[a], a, 0)[0] = float(n[a] - 1)             # index 0 lands exactly on m - 1: inside
        np.moveaxis(u[a], a, 0)[-1] = -float(n[a] - 1)           # the last index exactly on 0: inside
        assert _check_force(v, v, np.eye(4), u, label='the warp exactly on the borders of axis %d' % a)[3] == V
        u[a].flat[0] = np.nan
        assert _check_force(v, v, np.eye(4), u, label='a NaN in the warp')[3] == V - 1
    for dtype in (np.float32, np.float64):
        wild_f, wild_m = _smooth(n, 4), _smooth(n, 5, dtype)
        wild_f[1, 2, 3], wild_f[5, 5, 5] = np.nan, np.inf
        wild_m[2, 2, 2], wild_m[4, 3, 4], wild_m[5, 6, 7] = np.nan, -np.inf, np.inf
        # each value of the moving volume that is not finite takes the 8 fixed voxels around it out (at the far corner the clamped
        # neighbours), the two of the fixed volume themselves
        got = _check_force(wild_f, wild_m, np.eye(4), zero, label='nan and inf, identity')
        assert got[3] == V - 2 - 3 * 8 and np.isfinite(got[0]).all() and np.isfinite(got[2])
        got = _check_force(wild_f, wild_m, _scaled(n, n, (0.5, 0.5, 0.5)), _warp(n, 6, 0.4), label='nan and inf, half a voxel')
        assert 0 < got[3] < V - 2 - 8 and np.isfinite(got[0]).all()
    flat = np.full(n, 42.0)
    got = _check_force(flat, flat.astype(np.float32), np.eye(4), _warp(n, 7, 0.4), label='constant volumes: r == 0, G == 0, den == 0')
    assert got[3] > V // 4 and not got[0].any() and got[2] == 0.0 and (got[1] == 1).sum() == got[3]
    patch = v.copy()
    patch[1:5, 1:6, 1:7] = 42.0                                   # a constant patch in both: den == 0 inside it, forces around it
    got = _check_force(patch, patch, np.eye(4), zero, label='a constant patch')
    assert got[3] == V and not got[0].any() and got[2] == 0.0
    shifted = np.eye(4)
    shifted[:3, 3] = (0.25, -0.25, 0.5)
    got = _check_force(patch, patch, shifted, zero, label='a constant patch, shifted')
    assert not got[0][:, 2:4, 2:5, 2:5].any() and got[0].any() and (got[1][2:4, 2:5, 2:5] == 1).all()
    for step in (0.05, 3.0):
        got = _check_force(v, _noise(n, 8), _rotated(n, n), _warp(n, 9), maxStep=step, label='maxStep %g' % step)
        assert np.sqrt(got[0][0] * got[0][0] + got[0][1] * got[0][1] + got[0][2] * got[0][2]).max() <= step
    far = np.eye(4)
    far[0, 3] = 100.0
    got = _check_force(v, v, far, zero, label='every voxel outside')
    assert got[3] == 0 and got[2] == 0.0 and not got[0].any() and not got[1].any()
    got = _check_force(v, v, np.eye(4), zero, mask=np.zeros(n, np.uint8), label='an empty mask')
    assert got[3] == 0 and not got[1].any()


@pytest.mark.gpu
def test_force_pass_over_many_workgroups_and_planes():
    """70 x 61 x 63: 3843 columns are 16 workgroups (the last of 3 columns), k_warp_rows runs one; the march is 70 planes long."""
    n, m = (70, 61, 63), (22, 19, 21)
    fixed, moving = _smooth(n, 11, np.float32), _smooth(m, 12)
    mask = (np.random.default_rng(13).random(n) < 0.5).astype(np.uint8)
    got = _check_force(fixed, moving, _rotated(n, m), _warp(n, 14), mask, label='70x61x63')
    assert 1000 < got[3] < int(mask.sum())
    n = (3, 2, 600)                                               # k_warp_rows: three workgroups
    got = _check_force(_smooth(n, 15), _smooth((4, 3, 90), 16), _scaled(n, (4, 3, 90)), _warp(n, 17, 0.3), label='3x2x600')
    assert got[3] > 300 and got[1][:, :, 2 * WT:].any()                 # (every voxel lies on a face: the warp takes many outside)


# ------------------------------------------------------------------ GPU: the three-numerator fit
def _tile_shapes():
    shapes = []
    for axis, E in enumerate((WZ, WT, WT)):
        for n in (E - 1, E, E + 1, 2 * E + 1):
            s = [3, 5, 6]
            s[axis] = n
            shapes.append(tuple(s))
    return shapes


FIT_SHAPES = [(1, 1, 1), (2, 3, 1), (4, 4, 4), (5, 70, 3), (33, 30, 41)] + _tile_shapes()
FIT_SPANS = [(1, 1, 1), (1, 2, 4), (8, 3, 2), (2, 8, 3), (3, 2, 8)]          # 8 spans on an extent of 3 leave control points without support


@pytest.mark.gpu
@pytest.mark.parametrize('shape', FIT_SHAPES, ids=['x'.join(map(str, s)) for s in FIT_SHAPES])
def test_fit_is_three_bias_fits(shape):
    rng = np.random.default_rng(sum(shape))
    delta = rng.standard_normal((3,) + shape)
    masks = dict(full=np.ones(shape, np.uint8), random=(rng.random(shape) < 0.5).astype(np.uint8), empty=np.zeros(shape, np.uint8))
    spans_here = FIT_SPANS if max(shape) < WT - 1 else [FIT_SPANS[1], FIT_SPANS[2], FIT_SPANS[4]]          # (the model's time at the long extents)
    for spans in spans_here + ([(64, 1, 1), (1, 64, 64)] if shape == (4, 4, 4) else []):
        for kind, part in masks.items():
            before = delta.copy()
            got = R.fitForces(delta, part, spans)
            assert got.dtype == np.float64 and got.shape == (3,) + tuple(k + 3 for k in spans)
            three = np.stack([B.bsplineFit(delta[c], part, spans) for c in range(3)])
            assert np.array_equal(_bits(got), _bits(three)), (shape, spans, kind, 'against vmask_bias_fit')
            assert np.array_equal(_bits(got), _bits(M.fit3(delta, part, spans))), (shape, spans, kind, 'against the model')
            assert _same(delta, before)
            if kind == 'empty':
                assert not got.any()
            if kind == 'full' and max(spans) == 8 and min(shape) >= 2 and shape[spans.index(8)] == 3:
                assert (got == 0.0).any() and got.any()            # control points that no voxel reaches stay +0.0
    wild = delta.copy()
    wild[:, masks['random'] == 0] = np.nan                         # what delta holds where part == 0 does not matter
    assert np.array_equal(_bits(R.fitForces(wild, masks['random'], (2, 2, 2))), _bits(R.fitForces(delta, masks['random'], (2, 2, 2))))


# ------------------------------------------------------------------ GPU: the warp between levels
UP_SHAPES = [((1, 1, 1), (1, 1, 1)), ((1, 1, 1), (2, 1, 2)), ((4, 3, 5), (8, 6, 10)), ((4, 3, 5), (7, 5, 9)), ((5, 1, 9), (9, 1, 17)), ((20, 18, 17), (40, 36, 33)),
             ((3, 4, 2), (9, 3, 5))]


@pytest.mark.gpu
def test_upsampled_warp_is_the_model():
    for c, n in UP_SHAPES:                                        # even and odd fine extents, extents of 1, and a pair that is no pyramid
        coarse = _warp(c, sum(n), 3.0)
        before = coarse.copy()
        got, want = R.upsampleWarp(coarse, n), M.upsample(coarse, n)
        assert got.dtype == np.float64 and got.shape == (3,) + n
        assert np.array_equal(_bits(got), _bits(want)), (c, n, int((_bits(got) != _bits(want)).sum()))
        assert _same(coarse, before)
    ramp = np.stack([np.broadcast_to(np.arange(4.0)[:, None, None], (4, 3, 5))] * 3)          # 2 x a linear warp, clamped at the faces
    got = R.upsampleWarp(ramp, (8, 6, 10))
    assert np.array_equal(got[0][:, 0, 0], 2.0 * np.clip((np.arange(8.0) - 0.5) * 0.5, 0.0, 3.0)) and (got[0] == got[0][:, :1, :1]).all()
    assert not R.upsampleWarp(np.zeros((3, 4, 3, 5)), (8, 6, 10)).any()


@pytest.mark.gpu
def test_upsampled_warp_on_the_second_trip():
    c, n = (2, 3, 8739), (3, 5, 17477)
    assert int(np.prod(n)) > SECOND_TRIP
    coarse = _warp(c, 21, 2.0)
    got, want = R.upsampleWarp(coarse, n), M.upsample(coarse, n)
    assert np.array_equal(_bits(got), _bits(want)) and got.reshape(3, -1)[:, SECOND_TRIP:].any()


# ------------------------------------------------------------------ GPU: the resampled volume
RESAMPLE_TYPES = (np.uint8, np.int16, np.int32, np.float32, np.float64)


def _through(moving, T, u, order, fill):
    n = u.shape[1:]
    got = warpResample(moving, T, u, order=order, fill=fill)                   # (T as W between identity affines: the voxel map is inv(W))
    want = M.resample(moving, np.linalg.inv(T), u, order, fill)
    return got, want, n


@pytest.mark.gpu
def test_warp_resample_is_the_model_and_a_zero_warp_is_resample():
    for n, m in (((5, 7, 3), (7, 6, 5)), ((17, 16, 15), (7, 6, 1)), ((9, 1, 1), (1, 6, 5)), ((12, 10, 9), (11, 9, 10))):
        W = np.linalg.inv(_rotated(n, m))                            # warpResample inverts it again
        for u in (np.zeros((3,) + n), -np.zeros((3,) + n), _warp(n, 31, 1.2)):
            for dtype in (np.float32, np.float64):
                moving = _noise(m, 32, dtype)
                for fill in (-7.5, float('nan')):
                    got, want, _ = _through(moving, W, u, 1, fill)
                    assert got.dtype == np.float64 and got.shape == n and got.tobytes() == want.tobytes(), (n, m, dtype, fill)
                    if not u.any():
                        assert got.tobytes() == R.resample(moving, np.linalg.inv(W), n, order=1, fill=fill).tobytes()
            for dtype in RESAMPLE_TYPES:
                moving = (_noise(m, 33) * 0.5).astype(dtype)
                got, want, _ = _through(moving, W, u, 0, 250)
                assert _same(got, want), (n, m, dtype)
                if not u.any():
                    assert _same(got, R.resample(moving, np.linalg.inv(W), n, order=0, fill=250))
            labels = _noise(m, 34) > 100.0                           # bool goes in as uint8
            assert _same(warpResample(labels, W, u, order=0), M.resample(labels.astype(np.uint8), np.linalg.inv(W), u, 0, 0))
    n = (6, 7, 8)
    v = _noise(n, 35)
    u = np.zeros((3,) + n)
    u[2] = 0.5
    out = warpResample(v, None, u, fill=-1.0)                        # half a voxel along axis 2: midway between two neighbours, the last plane outside
    assert np.array_equal(out[:, :, :-1], v[:, :, :-1] + 0.5 * (v[:, :, 1:] - v[:, :, :-1])) and (out[:, :, -1] == -1.0).all()
    u[2] = 0.49
    assert np.array_equal(warpResample(v.astype(np.int32), None, u, order=0), v.astype(np.int32))
    u[2] = 0.5                                                       # floor(p + 0.5): the next voxel, the fill beyond the last
    assert np.array_equal(warpResample(v.astype(np.int32), None, u, order=0, fill=-9)[:, :, :-1], v.astype(np.int32)[:, :, 1:])


@pytest.mark.gpu
def test_warp_resample_on_the_second_trip():
    n, m = (70, 61, 63), (22, 19, 21)
    assert int(np.prod(n)) > SECOND_TRIP
    W = np.linalg.inv(_turned(n, m))
    u = _warp(n, 36, 2.0)
    moving = _noise(m, 37, np.float32)
    got, want, _ = _through(moving, W, u, 1, float('nan'))
    assert got.tobytes() == want.tobytes()
    late = got.ravel()[SECOND_TRIP:]
    assert 0 < int(np.isnan(late).sum()) < len(late)                 # the fill shows out there, and so do samples
    got, want, _ = _through(moving.astype(np.int16), W, u, 0, -5)
    assert _same(got, want) and 0 < int((got.ravel()[SECOND_TRIP:] == -5).sum()) < len(late)


# ------------------------------------------------------------------ GPU: one level, and the whole run
@pytest.mark.gpu
def test_level_is_the_model_and_ends_early():
    n, m = (33, 12, 20), (30, 14, 18)                             # 33 planes: k_warp_expand0's second block of planes
    fixed, moving = _smooth(n, 41), _smooth(m, 42, np.float32)
    T = _scaled(n, m, (0.3, -0.2, 0.1))
    scales = _scales(fixed, moving)
    mask = (np.random.default_rng(43).random(n) < 0.7).astype(np.uint8)
    start = _warp(n, 44, 0.3)
    for spans, msk, u0, kw in (((2, 2, 2), None, np.zeros((3,) + n), dict(iterations=4)), ((3, 1, 5), mask, start, dict(iterations=3, maxStep=1.0)),
                               ((1, 1, 1), None, start, dict(iterations=50, convergenceThreshold=0.2))):
        before = u0.copy()
        got, rows = R.warpLevel(fixed, moving, T, u0, *scales, spans, mask=msk, **kw)
        want, want_rows = M.level(fixed, moving, T, u0, *scales, spans, mask=msk, threshold=kw.get('convergenceThreshold', 0.01),
                                  **{k: v for k, v in kw.items() if k != 'convergenceThreshold'})
        assert np.array_equal(_bits(got), _bits(want)), (spans, int((_bits(got) != _bits(want)).sum()))
        assert rows.shape == want_rows.shape and np.array_equal(_bits(rows), _bits(want_rows)), (rows, want_rows)
        assert _same(u0, before) and got is not u0
    assert 1 <= len(rows) < 50 and rows[-1, 2] < 0.2 and (rows[:-1, 2] >= 0.2).all()          # the threshold ended the last one
    far = np.eye(4)
    far[0, 3] = 1000.0
    with pytest.raises(ValueError):
        R.warpLevel(fixed, moving, far, start, *scales, (2, 2, 2))
    with pytest.raises(ValueError):
        R.warpLevel(fixed, moving, T, start, *scales, (2, 2, 2), mask=np.zeros(n, np.uint8))
    with pytest.raises(ValueError):
        M.level(fixed, moving, far, start, *scales, (2, 2, 2))


def _assert_same_run(got, want, label):
    (warp, trace), (wm, tm) = got, want
    assert isinstance(warp, np.ndarray) and warp.dtype == np.float64 and warp.shape == wm.shape, label
    assert trace.shape == tm.shape and np.array_equal(_bits(trace), _bits(tm)), (label, trace[:3], tm[:3])
    assert np.array_equal(_bits(warp), _bits(wm)), (label, int((_bits(warp) != _bits(wm)).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(RECOVERY))
def test_register_nonlinear_is_the_model_on_the_recovery_phantom(name):
    """40 x 36 x 33, three levels, a mask: the warp and the trace bit for bit, so the recovery measured on the model is the GPU's."""
    fixed, moving, kw, truth = _case(name)
    before = (fixed.copy(), moving.copy(), kw['fixedMask'].copy())
    got = registerNonlinear(fixed, moving, **kw)
    _assert_same_run(got, _model_run(name), name)
    assert _same(fixed, before[0]) and _same(moving, before[1]) and _same(kw['fixedMask'], before[2])
    if name == 'same grid':
        again = registerNonlinear(fixed, moving, **kw)
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()          # a second run is byte-identical


@pytest.mark.gpu
def test_register_nonlinear_is_the_model_without_a_mask_in_float32_and_at_one_level():
    fixed, fA, moving, mA, W, _ = M.deformed_pair(other_grid=True, seed=1)
    f32, m32 = fixed.astype(np.float32), moving.astype(np.float32)
    kw = dict(W=W, fixedAffine=fA, movingAffine=mA, iterations=8)
    _assert_same_run(registerNonlinear(f32, m32, levels=1, **kw), M.register_nonlinear(f32, m32, levels=1, **kw), 'levels=1, float32')
    got = registerNonlinear(fixed, m32, levels=3, splineSpans=(1, 2, 3), maxStep=0.25, **kw)
    _assert_same_run(got, M.register_nonlinear(fixed, m32, levels=3, splineSpans=(1, 2, 3), maxStep=0.25, **kw), 'no mask, spans (1, 2, 3)')
    assert sorted(set(got[1][:, 0])) == [0.0, 1.0, 2.0]
    small = registerNonlinear(fixed[:14, :15, :13], m32, levels=3, **kw)                  # 7 x 8 x 7 would fall below 8: one level only
    assert set(small[1][:, 0]) == {0.0}
    ints = np.round(fixed).astype(np.int16), np.round(moving).astype(np.uint8)           # other dtypes go in as float64
    _assert_same_run(registerNonlinear(*ints, levels=2, **kw), M.register_nonlinear(ints[0].astype(np.float64), ints[1].astype(np.float64), levels=2, **kw), 'integers')
    with pytest.raises(ValueError):
        registerNonlinear(fixed, moving, fixedMask=np.zeros(fixed.shape, np.uint8), **kw)          # nothing takes part
    far = W.copy()
    far[0, 3] += 1000.0
    with pytest.raises(ValueError):
        registerNonlinear(fixed, moving, **dict(kw, W=far))


# ------------------------------------------------------------------ GPU: device pointers, in a process of their own
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import registration as R
import warp_model as M
from test_warp import _refusals, _host_outputs, _smooth, _warp, _rotated, _scales, N_REFUSALS, SENTINEL, VALUE
dev = torch.device('cuda', 0)
t = lambda a: torch.as_tensor(a, device=dev)
n, m = (12, 10, 9), (11, 9, 10)
fixed, mask, u = _smooth(n, 1), (np.random.default_rng(0).random(n) < 0.6).astype(np.uint8), _warp(n, 2, 0.8)
T = _rotated(n, m)
for dtype in (np.float32, np.float64):
    moving = _smooth(m, 3, dtype)
    scales = _scales(fixed, moving)
    host = R.forcePass(fixed, moving, T, u, *scales, mask=mask)
    got = R.forcePass(t(fixed), t(moving), T, t(u), *scales, mask=t(mask))
    assert got[0].is_cuda and got[0].dtype == torch.float64 and got[1].is_cuda and got[1].dtype == torch.uint8
    assert got[0].cpu().numpy().tobytes() == host[0].tobytes() and got[1].cpu().numpy().tobytes() == host[1].tobytes() and got[2:] == host[2:] and host[3] > 100
    mixed = R.forcePass(fixed, t(moving), T, u, *scales, mask=mask)                    # host and device arrays in one call
    assert mixed[0].tobytes() == host[0].tobytes() and mixed[2:] == host[2:]
    phi = R.fitForces(got[0], got[1], (2, 3, 1))
    assert phi.is_cuda and phi.cpu().numpy().tobytes() == R.fitForces(host[0], host[1], (2, 3, 1)).tobytes()
    fine = R.upsampleWarp(t(u), (24, 19, 18))
    assert fine.is_cuda and fine.cpu().numpy().tobytes() == R.upsampleWarp(u, (24, 19, 18)).tobytes()
    tu = t(u)
    lev, rows = R.warpLevel(t(fixed), t(moving), T, tu, *scales, (2, 2, 2), iterations=3, mask=t(mask))
    hl, hrows = R.warpLevel(fixed, moving, T, u, *scales, (2, 2, 2), iterations=3, mask=mask)
    assert lev.is_cuda and lev.cpu().numpy().tobytes() == hl.tobytes() and rows.tobytes() == hrows.tobytes() and lev.data_ptr() == tu.data_ptr()
    W = np.linalg.inv(T)
    for order, mv in ((1, moving), (0, moving), (0, (moving * 0.5).astype(np.int16))):
        out = R.warpResample(t(mv), W, t(u), order=order, fill=-3)
        assert out.is_cuda and out.cpu().numpy().tobytes() == R.warpResample(mv, W, u, order=order, fill=-3).tobytes()
        assert R.warpResample(t(mv), W, u, order=order, fill=-3).cpu().numpy().tobytes() == out.cpu().numpy().tobytes()         # a host warp beside a tensor
    assert t(moving).cpu().numpy().tobytes() == moving.tobytes()
fx, fA, mv, mA, W, _ = M.deformed_pair(other_grid=True, seed=1)
fx, mv = np.array(fx), np.array(mv)
kw = dict(W=W, fixedAffine=fA, movingAffine=mA, levels=2, iterations=5)
warp, trace = R.registerNonlinear(t(fx), t(mv), fixedMask=t(fx > 50.0), **kw)
wh, th = R.registerNonlinear(fx, mv, fixedMask=(fx > 50.0), **kw)
assert warp.is_cuda and warp.dtype == torch.float64 and tuple(warp.shape) == (3,) + fx.shape
assert warp.cpu().numpy().tobytes() == wh.tobytes() and trace.tobytes() == th.tobytes() and len(trace) == 10
print('DEVICE RESIDENT OK')

shape, mshape = (4, 5, 6), (3, 4, 5)
full = lambda s, v, dt=torch.float64: torch.full(s, v, dtype=dt, device=dev)
a = dict(fixed=full(shape, 1.0), mask=full(shape, 1, torch.uint8), warp=full((3,) + shape, 0.0), f64=full(mshape, 1.0), u8=full(mshape, 1, torch.uint8),
         delta=full((3,) + shape, VALUE), part=full(shape, SENTINEL, torch.uint8), phi=full((3, 4, 4, 4), VALUE), fine=full((3,) + shape, VALUE),
         out=full(shape, VALUE), u=full((3,) + shape, VALUE))
h = _host_outputs()
torch.cuda.synchronize()
p = {{k: v.data_ptr() for k, v in a.items()}}
p.update({{k: v.ctypes.data for k, v in h.items()}})
res = _refusals(R._lib(), p, shape, mshape)
assert len(res) == N_REFUSALS
for label, rc in res:
    assert rc == -1, label
torch.cuda.synchronize()
for k in ('delta', 'phi', 'fine', 'out', 'u'):
    assert bool((a[k] == VALUE).all()), k
assert bool((a['part'] == SENTINEL).all()) and bool((a['fixed'] == 1.0).all()) and not bool(a['warp'].any())
assert (h['S'] == VALUE).all() and (h['trace'] == VALUE).all() and h['count'][0] == -777 and h['ntrace'][0] == -777
# the loop's own refusal - nothing takes part - leaves the warp alone as well
far = np.eye(4)[:3].copy(); far[0, 3] = 1000.0
spans = np.array([1, 1, 1], np.intc)
rc = R._lib().vmask_warp_field(0, p['fixed'], 6, None, *shape, p['f64'], 6, *mshape, far.ctypes.data, 0.0, 1.0, 0.0, 1.0, spans.ctypes.data, 3, 0.5, 0.01, p['u'], None, None)
torch.cuda.synchronize()
assert rc == -1 and bool((a['u'] == VALUE).all())
print('REFUSALS OK')
"""


@functools.lru_cache(maxsize=None)
def _device_run():
    script = DEVICE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    return out.returncode, out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_warp_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, bit-identical to the host
    call; the inputs are unchanged.  Own process: torch is imported before the HIP library there."""
    rc, stdout, tail = _device_run()
    assert 'DEVICE RESIDENT OK' in stdout, tail


@pytest.mark.gpu
def test_warp_refusals_with_device_pointers():
    """Every refused input of the C entries, with device pointers: VRG_E_ARG, the sentinels in the outputs untouched."""
    rc, stdout, tail = _device_run()
    assert rc == 0 and 'REFUSALS OK' in stdout, tail


# ------------------------------------------------------------------ GPU: the files
@pytest.mark.gpu
def test_main_nonlinear_writes_its_files_and_a_mask_follows(tmp_path, capsys):
    from arterynetwork_amd import nifti
    fixed, fA, moving, mA, W, truth = M.deformed_pair(other_grid=True, seed=1)
    folder = str(tmp_path)
    nifti.saveVolume(fixed, fA, os.path.join(folder, 'brainVolume.nii.gz'), astype=np.float32)
    nifti.saveVolume(moving, mA, os.path.join(folder, 'followUp.nii.gz'), astype=np.float32)
    label = (moving > 0.7 * 150.0 + 20.0).astype(np.uint8) * 7         # the two inner classes and the vessels, in the moving image's space
    nifti.saveVolume(label, mA, os.path.join(folder, 'followUpMask.nii.gz'))
    np.savetxt(os.path.join(folder, 'followUpToFixed.mat'), W, fmt='%.17g')                # what registration.main leaves
    kw = dict(levels=2, iterations=10)
    warp, result = R.mainNonlinear(folder, 'followUp.nii.gz', **kw)
    printed = capsys.readouterr().out
    for name in ('followUpWarped.nii.gz', 'followUpWarp.nii.gz'):
        assert '{} saved to {}.'.format(name, os.path.join(folder, name)) in printed
    assert 'followUpToFixed.mat saved' not in printed                                      # the matrix was there: no affine search ran
    f32, m32 = fixed.astype(np.float32), moving.astype(np.float32)
    fA32, mA32 = nifti.loadVolume(folder, 'brainVolume.nii.gz')[1], nifti.loadVolume(folder, 'followUp.nii.gz')[1]
    want_warp, _ = registerNonlinear(f32, m32, W=W, fixedAffine=fA32, movingAffine=mA32, **kw)
    assert warp.tobytes() == want_warp.tobytes()
    want = warpResample(m32, W, warp, fA32, mA32, order=1, fill=0)
    assert result.dtype == np.float64 and np.array_equal(_bits(result), _bits(want))
    vol, aff = nifti.loadVolume(folder, 'followUpWarped.nii.gz')
    assert vol.dtype == np.float32 and np.array_equal(vol, want.astype(np.float32)) and np.allclose(aff, fA)
    stored, aff = nifti.loadVolume(folder, 'followUpWarp.nii.gz')
    assert stored.dtype == np.float32 and stored.shape == fixed.shape + (3,) and np.allclose(aff, fA)
    assert np.array_equal(np.moveaxis(stored, 3, 0), warp.astype(np.float32))
    # a mask of the moving image's space, carried through the stored (float32) warp, lands on the support of the volume carried the same way
    out = R.applyWarp(folder, 'followUpMask.nii.gz', 'followUpToFixed.mat', 'followUpWarp.nii.gz')
    stored_mask, aff = nifti.loadVolume(folder, 'followUpMaskWarped.nii.gz')
    assert out.dtype == np.uint8 and stored_mask.dtype == np.uint8 and np.array_equal(stored_mask, out) and np.allclose(aff, fA) and set(np.unique(out)) == {0, 7}
    warp32 = np.moveaxis(stored, 3, 0).astype(np.float64)
    assert np.array_equal(out, warpResample(label, W, warp32, fA32, mA32, order=0, fill=0))
    smooth = R.applyWarp(folder, 'followUp.nii.gz', 'followUpToFixed.mat', 'followUpWarp.nii.gz', order=1, outputName='again.nii.gz')
    assert np.array_equal(_bits(smooth), _bits(warpResample(m32, W, warp32, fA32, mA32, order=1, fill=0)))
    # Where the up to 8 moving voxels around a sample point are all in the mask (all outside it), the nearest one is, and the trilinear
    # sample, a mean of values above (not above) the mask's threshold, is on the same side: there the carried mask IS the carried
    # volume's support.  Elsewhere - the rim, where the 8 disagree - nearest and trilinear may differ.  frac: the mask carried trilinearly.
    frac = warpResample((label != 0).astype(np.float32), W, warp32, fA32, mA32, order=1, fill=0)
    support = smooth > 0.7 * 150.0 + 20.0
    sure = (frac == 0.0) | (frac == 1.0)
    print('the 8 neighbours agree at {:.4f} of the voxels; the carried mask holds {} voxels, the support {}'.format(sure.mean(), int((out != 0).sum()), int(support.sum())))
    assert np.array_equal((out != 0)[sure], support[sure]) and sure.mean() > 0.5 and (out != 0)[sure].any()
    # without a matrix file the affine search runs first and leaves one
    os.remove(os.path.join(folder, 'followUpToFixed.mat'))
    R.mainNonlinear(folder, 'followUp.nii.gz', levels=1, iterations=2, outputName='b.nii.gz', warpName='bWarp.nii.gz')
    printed = capsys.readouterr().out
    assert 'followUpToFixed.mat saved to' in printed and np.loadtxt(os.path.join(folder, 'followUpToFixed.mat')).shape == (4, 4)
    assert os.path.exists(os.path.join(folder, 'b.nii.gz')) and os.path.exists(os.path.join(folder, 'bWarp.nii.gz'))
