"""Rigid and affine registration (DESIGN.md section 9 entry f16).  On the CPU: the host cost entry against its numpy restatement,
paramsToMatrix, what the step is for on the numpy model tests/registration_model.py alone, the refusals, the kernels' resource
records, the histogram's walk (csrc/vreg_walk.h) against the split of every voxel it visits.  On the GPU: the joint histogram must return the model's counts, the extrema, bin images, pyramids and resampled volumes
the model's bits, and ``register`` the model's matrix and trace bit for bit."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import registration_model as M
from conftest import ROOT
from arterynetwork_amd import registration as R

# k_reg_hist of csrc/vreg_device.hip: the fixed voxels a workgroup takes per grid-stride trip, and the most workgroups of a launch
# (test_trip_extent_and_grid_are_the_kernels reads them)
G, WORKGROUPS = 256, 1024

# largest |vmask_reg_cost - cost_numpy| seen for mi and nmi over COST_CASES, and what is allowed: ten times it.  The deviation is the
# host's log against numpy's log of float64 scalars; every case agreed to the last bit: 0.0 seen (numpy 1.x / 2.x scalar path on x86-64).
LOG_SEEN = 0.0
LOG_BAR = 10.0 * LOG_SEEN


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ CPU: the cost
def _cost_cases():
    rng = np.random.default_rng(0)
    cases = []
    for B in (8, 64, 128):
        cases.append(('random %d' % B, rng.integers(0, 1000, (B, B)).astype(np.uint64), 0.0, 0))
        sparse = (rng.integers(0, 50000, (B, B)) * (rng.random((B, B)) < 0.1)).astype(np.uint64)
        cases.append(('sparse %d' % B, sparse, 0.25, int(sparse.sum())))
        diag = np.zeros((B, B), np.uint64)
        diag[np.arange(B), np.arange(B)] = rng.integers(1, 9999, B).astype(np.uint64)
        cases.append(('diagonal %d' % B, diag, 0.0, 0))
        one = np.zeros((B, B), np.uint64)
        one[B // 3, B // 2] = 777
        cases.append(('single bin %d' % B, one, 0.0, 0))
        cases.append(('empty %d' % B, np.zeros((B, B), np.uint64), 0.0, 0))
        border = np.zeros((B, B), np.uint64)
        border[1, 2], border[1, 5], border[3, 3] = 100, 100, 50                    # N = 250 = 0.25 * 1000
        cases.append(('at the overlap border %d' % B, border, 0.25, 1000))
        cases.append(('below the overlap border %d' % B, border, 0.25, 1001))
    return cases


COST_CASES = _cost_cases()


def test_corratio_cost_is_the_restatement():
    for label, H, overlap, nmask in COST_CASES:
        before = H.copy()
        got, want = R.costFromHistogram(H, 'corratio', overlap, nmask), M.cost_numpy(H, 'corratio', overlap, nmask)
        assert np.array_equal(_bits(got), _bits(want)), (label, got, want)
        assert np.array_equal(H, before)
        if label.startswith('diagonal') or label.startswith('single bin'):
            assert got == 0.0, label                       # the moving bin is a function of the fixed bin
        if label.startswith('empty') or label.startswith('below'):
            assert got == float('inf'), label
        if label.startswith('at the') or label.startswith('random'):
            assert 0.0 < got <= 1.0, (label, got)


def test_mi_and_nmi_costs_are_near_the_restatement():
    worst = 0.0
    for label, H, overlap, nmask in COST_CASES:
        for name in ('mi', 'nmi'):
            got, want = R.costFromHistogram(H, name, overlap, nmask), M.cost_numpy(H, name, overlap, nmask)
            if np.isinf(want):
                assert got == want, (label, name)
                continue
            print('{} {}: {!r} against {!r}'.format(label, name, got, want))
            worst = max(worst, abs(got - want))
            if label.startswith('diagonal'):
                assert got < -1.0 if name == 'mi' else got == -2.0, (label, name, got)
            if label.startswith('single bin'):
                assert got == 0.0, (label, name, got)
    print('worst |cost - restatement| = {:.3e}'.format(worst))
    assert worst <= LOG_BAR


# ------------------------------------------------------------------ CPU: the parameters
def test_params_to_matrix():
    centre = np.array([3.0, -20.0, 7.5])
    for dof in R.DOFS:
        assert np.array_equal(R.paramsToMatrix(np.zeros(dof), dof, centre), np.eye(4)), dof
    rng = np.random.default_rng(1)
    for _ in range(20):
        W = R.paramsToMatrix(np.concatenate((rng.uniform(-30, 30, 3), rng.uniform(-np.pi, np.pi, 3))), 6, centre)
        assert np.abs(W[:3, :3] @ W[:3, :3].T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(W[:3, :3]) - 1.0) <= 1e-15
        assert np.array_equal(W[3], [0.0, 0.0, 0.0, 1.0])
    # dof 12 is its documented composition, and the parts come back out of it
    p = np.array([4.0, -3.0, 2.5, 0.2, -0.1, 0.3, 0.05, -0.04, 0.1, 0.02, -0.03, 0.01])
    W = R.paramsToMatrix(p, 12, centre)

    def hom(m3=np.eye(3), t=np.zeros(3)):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = m3, t
        return m
    c, s = np.cos(p[3:6]), np.sin(p[3:6])
    Rx = [[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]
    Ry = [[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]]
    Rz = [[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]
    shear = np.array([[1, p[9], p[10]], [0, 1, p[11]], [0, 0, 1.0]])
    want = hom(t=centre) @ hom(t=p[:3]) @ hom(Rz) @ hom(Ry) @ hom(Rx) @ hom(np.diag(1.0 + p[6:9])) @ hom(shear) @ hom(t=-centre)
    assert np.abs(W - want).max() <= 1e-13
    A = W[:3, :3]                                        # A = Rot . Scale . Shear: QR gives them back
    Q, U = np.linalg.qr(A)
    sign = np.sign(np.diag(U))
    Q, U = Q * sign, (U.T * sign).T
    assert np.abs(np.diag(U) - (1.0 + p[6:9])).max() <= 1e-14
    assert np.abs(U / np.diag(U)[:, None] - shear).max() <= 1e-14
    assert np.abs(Q - np.array(Rz) @ np.array(Ry) @ np.array(Rx)).max() <= 1e-14
    assert np.abs(W[:3, 3] - (centre + p[:3] - A @ centre)).max() <= 1e-13
    assert np.array_equal(R.paramsToMatrix(p[:7], 7, centre)[:3, :3], R.paramsToMatrix(np.concatenate((p[:6], [p[6]] * 3)), 9, centre)[:3, :3])
    for bad in ((np.zeros(6), 5), (np.zeros(7), 6), (np.full(6, np.nan), 6)):
        with pytest.raises(ValueError):
            R.paramsToMatrix(bad[0], bad[1], centre)


# ------------------------------------------------------------------ CPU: what the step is for, on the model alone
SHAPE, SPACING = (40, 48, 36), (1.0, 1.0, 1.5)
MOVING_SHAPE, MOVING_SPACING = (44, 38, 42), (1.1, 1.3, 1.2)
TRUE = (3.1, -2.3, 1.7, np.deg2rad(8.0), np.deg2rad(-6.0), np.deg2rad(10.0))


@functools.lru_cache(maxsize=None)
def _pair(dof=6, small=False):
    """(fixed, fixedAffine, moving, movingAffine, W_true): the phantom, and what another scanner makes of it - another grid and
    spacing, the known rigid (dof 7: and 5 % larger) W_true, the intensities through v^0.6, 2 % noise.  small: half the extents."""
    shape, mshape = (SHAPE, MOVING_SHAPE) if not small else ((20, 24, 18), (22, 19, 21))
    sp, msp = (SPACING, MOVING_SPACING) if not small else ((2.0, 2.0, 3.0), (2.2, 2.6, 2.4))
    fA, mA = M.affine_of(sp, shape), M.affine_of(msp, mshape, centre_at=(1.0, -0.5, 0.7))
    fixed = M.phantom(shape)
    centre = (fA @ np.append((np.array(shape) - 1.0) / 2.0, 1.0))[:3]
    W = R.paramsToMatrix(TRUE + ((0.05,) if dof == 7 else ()), dof, centre)
    moving = M.moving_of(fixed, fA, W, mshape, mA)
    for a in (fixed, moving, fA, mA, W):
        a.setflags(write=False)
    return fixed, fA, moving, mA, W


@pytest.mark.parametrize('dof,cost', [(6, 'corratio'), (6, 'nmi'), (7, 'corratio')], ids=['rigid-corratio', 'rigid-nmi', 'dof7-scaled'])
def test_model_recovers_a_known_transform(dof, cost):
    """The moving image is the phantom under a rotation of (8, -6, 10) degrees and a translation of (3.1, -2.3, 1.7) on a grid
    of another shape and spacing, its intensities through a monotone map with 2 % noise.  The largest displacement of the fixed
    grid's 8 corners between the recovered and the true W must stay below the smallest fixed voxel spacing, 1.0.
    Measured when this was written: corratio 0.053, nmi 0.399, dof 7 on the 5 % scaled copy 0.442 (from 11.5 before)."""
    fixed, fA, moving, mA, W_true = _pair(dof)
    W, trace = M.register(fixed, moving, fixedAffine=fA, movingAffine=mA, dof=dof, cost=cost)
    start = M.corner_error(np.eye(4), W_true, SHAPE, fA)
    err = M.corner_error(W, W_true, SHAPE, fA)
    print('dof {} {}: corner error {:.3f} (from {:.2f}), evaluations {}, {} accepted steps'.format(dof, cost, err, start, trace['evaluations'].tolist(), len(trace['steps'])))
    assert start > 5.0 and err < min(SPACING)
    assert len(trace['evaluations']) == 3 and trace['steps'].shape[1] == dof + 2
    assert (np.diff(trace['steps'][:, 0]) >= 0).all()
    for level in range(3):                               # within a level every accepted step lowers the cost
        c = trace['steps'][trace['steps'][:, 0] == level, -1]
        assert (np.diff(c) < 0).all()


def _integer_copies():
    """The small pair with the moving volume rounded into 0 .. 255, as float64, uint8 and int16 copies of the same numbers."""
    fixed, fA, moving, mA, _ = _pair(6, small=True)
    moving = np.clip(np.round(moving), 0.0, 255.0)
    return [(fixed.astype(t), moving.astype(t)) for t in (np.float64, np.uint8, np.int16)], fA, mA


def test_model_takes_integer_volumes_as_volumes():
    """A uint8 volume is a volume, not a mask: its pyramid is the block mean, and the search is the float copy's, level by level."""
    copies, fA, mA = _integer_copies()
    kw = dict(fixedAffine=fA, movingAffine=mA, levels=2, maxEvaluations=120)
    (f, m) = copies[0]
    W, trace = M.register(f, m, **kw)
    assert trace['evaluations'][0] > 40 and (trace['steps'][:, 0] == 0.0).sum() > 3          # the coarse level has something to search
    for fi, mi in copies[1:]:
        assert np.array_equal(_bits(M.shrink(fi)), _bits(M.shrink(f))) and M.shrink(fi).max() > 1.0
        Wi, ti = M.register(fi, mi, **kw)
        assert Wi.tobytes() == W.tobytes() and ti['steps'].tobytes() == trace['steps'].tobytes() and np.array_equal(ti['evaluations'], trace['evaluations'])
        Wm, tm = M.register(fi, mi, fixedMask=(fi > 0), **kw)                                # a bool mask beside a uint8 volume
        Wf, tf = M.register(f, m, fixedMask=(f > 0).astype(np.uint8), **kw)
        assert Wm.tobytes() == Wf.tobytes() and tm['steps'].tobytes() == tf['steps'].tobytes()


# ------------------------------------------------------------------ CPU: refusals
def test_argument_errors_raise():
    """What the host can check is refused before a device is looked for: no GPU needed."""
    f, m = np.zeros((9, 8, 10)), np.zeros((8, 8, 8))
    nan = float('nan')
    bad = [dict(fixed=np.zeros((9, 8))), dict(moving=np.zeros((2, 8, 8, 8))), dict(fixedMask=np.ones((9, 8, 9))), dict(dof=8), dict(cost='ssd'),
           dict(bins=7), dict(bins=129), dict(levels=0), dict(levels=9), dict(minOverlap=1.5), dict(minOverlap=nan), dict(maxEvaluations=0),
           dict(fixedAffine=np.eye(3)), dict(movingAffine=np.zeros((4, 4))), dict(fixedAffine=np.full((4, 4), nan)), dict(initial=np.zeros(5)),
           dict(initial=np.full(6, nan)), dict(search=(10.0,)), dict(search=(10.0, 0.0)), dict(search=(-1.0, 5.0)), dict(search=(180.0, 1.0))]
    for kw in bad:
        args = dict(fixed=f, moving=m)
        args.update(kw)
        with pytest.raises(ValueError):
            R.register(**args)
    bins = np.zeros((4, 5, 6), np.uint8)
    for kw in (dict(bins=7), dict(bins=129), dict(T=np.eye(3)), dict(T=np.full((3, 4), nan)), dict(mlo=nan), dict(ms=float('inf')),
               dict(fixedBins=np.zeros((4, 5, 6))), dict(fixedBins=np.zeros((4, 5), np.uint8)), dict(moving=np.zeros((4, 5)))):
        args = dict(fixedBins=bins, moving=np.zeros((4, 5, 6)), T=np.eye(4))
        args.update(kw)
        with pytest.raises(ValueError):
            R.jointHistogram(**args)
    for kw in (dict(bins=7), dict(lo=nan), dict(s=-1.0), dict(s=float('inf')), dict(mask=np.ones((4, 5, 5))), dict(volume=np.zeros((4, 5)))):
        args = dict(volume=np.zeros((4, 5, 6)), lo=0.0, s=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            R.quantise(**args)
    for kw in (dict(order=2), dict(shape=(4, 5)), dict(shape=(4, 0, 5)), dict(T=np.eye(2)), dict(moving=np.zeros((4, 5, 6), np.int64), order=0),
               dict(moving=np.zeros((4, 5, 6), np.uint8), order=0, fill=256), dict(moving=np.zeros((4, 5, 6), np.int16), order=0, fill=0.5),
               dict(moving=np.zeros((4, 5), np.uint8), order=0), dict(moving=np.zeros((4, 5)))):
        args = dict(moving=np.zeros((4, 5, 6)), T=np.eye(4), shape=(4, 5, 6))
        args.update(kw)
        with pytest.raises(ValueError):
            R.resample(**args)
    with pytest.raises(ValueError):
        R.extrema(np.zeros((4, 5, 6)), np.ones((4, 5, 5)))
    with pytest.raises(ValueError):
        R.shrink(np.zeros((4, 5)))
    for args in ((np.zeros((7, 7)),), (np.zeros((8, 9)),), (np.zeros((8, 8)), 'ssd'), (np.zeros((8, 8)), 'mi', -0.1), (np.zeros((8, 8)), 'mi', 0.5, -1)):
        with pytest.raises(ValueError):
            R.costFromHistogram(*args)
    with pytest.raises(ValueError):
        R.main('.', None)
    with pytest.raises(ValueError):
        R.main('.', 'other.nii.gz', fixedAffine=np.eye(4))


SENTINEL = 0xA5


def _refusals(dll, p, shape, mshape):
    """Every refused input of the C entries: (label, return code).  `p` holds the addresses of a uint8 bin image and a uint8 mask
    of `shape`, of float64, float32 and uint8 volumes of `mshape`, and of the outputs: H (128 x 128 uint64), bins (uint8, `shape`),
    out (float64 room for `shape`), lohi (2 float64)."""
    keep = []

    def T(*rows):
        keep.append(np.ascontiguousarray(np.array(rows if rows else np.eye(4)[:3], dtype=np.float64)))
        return keep[-1].ctypes.data
    nan, inf = float('nan'), float('inf')
    bad_T = np.eye(4)[:3].copy()
    bad_T[1, 2] = nan
    inf_T = np.eye(4)[:3].copy()
    inf_T[2, 3] = inf
    huge = (2000, 2000, 600)

    def hist(label, fb=p['fb'], n=shape, mov=p['f64'], dtype=6, m=mshape, t=None, B=64, mlo=0.0, ms=1.0, H=p['H']):
        t = T() if t is None else t
        return 'hist ' + label, dll.vmask_reg_joint_hist(0, fb, *n, mov, dtype, *m, t, B, mlo, ms, H)

    def quant(label, v=p['f64'], dtype=6, mask=None, n=mshape, B=64, lo=0.0, s=1.0, out=p['bins']):
        return 'quantise ' + label, dll.vmask_reg_quantise(0, v, dtype, mask, *n, B, lo, s, out, None)

    def minmax(label, v=p['f64'], dtype=6, n=mshape, out=p['lohi']):
        return 'minmax ' + label, dll.vmask_reg_minmax(0, v, dtype, None, *n, out)

    def shrink(label, v=p['f64'], dtype=6, n=mshape, out=p['out']):
        return 'shrink ' + label, dll.vmask_reg_shrink(0, v, dtype, *n, out)

    def resample(label, v=p['f64'], dtype=6, m=mshape, t=None, order=1, fill=0.0, out=p['out'], n=shape):
        t = T() if t is None else t
        return 'resample ' + label, dll.vmask_reg_resample(0, v, dtype, *m, t, order, fill, out, *n)
    res = [hist('bins 7', B=7), hist('bins 129', B=129), hist('bins 0', B=0), hist('T nan', t=T(*bad_T)), hist('T inf', t=T(*inf_T)),
           hist('fixed extent 0', n=(shape[0], 0, shape[2])), hist('fixed envelope', n=huge), hist('moving extent 0', m=(0, mshape[1], mshape[2])),
           hist('moving envelope', m=huge), hist('moving extent 32001', m=(32001, 1, 1)), hist('dtype 0', mov=p['u8'], dtype=0), hist('dtype 4', dtype=4),
           hist('dtype 7', dtype=7), hist('mlo nan', mlo=nan), hist('ms inf', ms=inf), hist('null bins', fb=None), hist('null moving', mov=None),
           hist('null T', t=0), hist('null H', H=None)]
    res += [quant('bins 7', B=7), quant('bins 129', B=129), quant('lo nan', lo=nan), quant('s < 0', s=-1.0), quant('s inf', s=inf), quant('dtype 0', v=p['u8'], dtype=0),
            quant('null volume', v=None), quant('null bins', out=None), quant('extent 0', n=(0, 1, 1)), quant('envelope', n=huge)]
    res += [minmax('dtype 3', dtype=3), minmax('null volume', v=None), minmax('null out', out=None), minmax('extent 0', n=(1, 0, 1)), minmax('envelope', n=huge)]
    res += [shrink('dtype 1', dtype=1), shrink('dtype 4', dtype=4), shrink('null volume', v=None), shrink('null out', out=None), shrink('extent 0', n=(1, 1, 0)),
            shrink('envelope', n=huge)]
    res += [resample('order 2', order=2), resample('order -1', order=-1), resample('order 1 of uint8', v=p['u8'], dtype=0), resample('order 0 of int64', dtype=4, order=0),
            resample('order 0 of uint16', dtype=2, order=0), resample('T nan', t=T(*bad_T)), resample('T inf', t=T(*inf_T), order=0),
            resample('fill 256 of uint8', v=p['u8'], dtype=0, order=0, fill=256.0), resample('fill -1 of uint8', v=p['u8'], dtype=0, order=0, fill=-1.0),
            resample('fill 0.5 of int16', dtype=1, order=0, fill=0.5), resample('fill nan of int32', dtype=3, order=0, fill=nan),
            resample('null moving', v=None), resample('null T', t=0), resample('null out', out=None), resample('moving extent 0', m=(1, 0, 1)),
            resample('moving envelope', m=huge), resample('fixed extent 0', n=(0, 1, 1)), resample('fixed envelope', n=huge)]
    return res


N_REFUSALS = 19 + 10 + 5 + 6 + 18


def test_c_entries_refuse_before_a_device_is_looked_for():
    """Host pointers, no GPU needed: every refusal is VRG_E_ARG and leaves the outputs alone."""
    dll = R._lib()
    shape, mshape = (4, 5, 6), (3, 4, 5)
    a = dict(fb=np.zeros(shape, np.uint8), f64=np.ones(mshape), f32=np.ones(mshape, np.float32), u8=np.ones(mshape, np.uint8),
             H=np.full((128, 128), SENTINEL, np.uint64), bins=np.full(shape, SENTINEL, np.uint8), out=np.full(shape, -12345.0), lohi=np.full(2, -12345.0))
    res = _refusals(dll, {k: v.ctypes.data for k, v in a.items()}, shape, mshape)
    assert len(res) == N_REFUSALS
    for label, rc in res:
        assert rc == -1, label                               # VRG_E_ARG
    assert (a['H'] == SENTINEL).all() and (a['bins'] == SENTINEL).all() and (a['out'] == -12345.0).all() and (a['lohi'] == -12345.0).all()
    assert (a['f64'] == 1.0).all() and (a['fb'] == 0).all()
    H = np.ones((8, 8), np.uint64)
    cost = np.full(1, -12345.0)
    for args in ((None, 8, 0, 0.0, 0, cost.ctypes.data), (H.ctypes.data, 8, 0, 0.0, 0, None), (H.ctypes.data, 7, 0, 0.0, 0, cost.ctypes.data),
                 (H.ctypes.data, 129, 0, 0.0, 0, cost.ctypes.data), (H.ctypes.data, 8, 3, 0.0, 0, cost.ctypes.data), (H.ctypes.data, 8, -1, 0.0, 0, cost.ctypes.data),
                 (H.ctypes.data, 8, 0, -0.1, 0, cost.ctypes.data), (H.ctypes.data, 8, 0, 1.5, 0, cost.ctypes.data), (H.ctypes.data, 8, 0, float('nan'), 0, cost.ctypes.data),
                 (H.ctypes.data, 8, 0, 0.5, -1, cost.ctypes.data)):
        assert dll.vmask_reg_cost(*args) == -1, args
    assert cost[0] == -12345.0
    import ctypes
    held = ctypes.c_void_p(12345)
    dll.vmask_reg_hold.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    assert dll.vmask_reg_hold(0, None, 0, ctypes.byref(held)) == -1 and dll.vmask_reg_hold(0, None, -8, ctypes.byref(held)) == -1
    assert dll.vmask_reg_hold(0, None, 8, None) == -1 and held.value == 12345
    dll.vmask_reg_release(None)                          # allowed


# ------------------------------------------------------------------ no GPU needed: the kernels
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
SOURCE = os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vreg_device.hip')


def test_trip_extent_and_grid_are_the_kernels():
    text = open(SOURCE).read()
    assert int(re.search(r'constexpr int RG = (\d+);', text).group(1)) == G
    assert int(re.search(r'constexpr int RT = (\d+);', text).group(1)) == 256
    assert int(re.search(r'constexpr int RGRID = (\d+);', text).group(1)) == WORKGROUPS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_registration_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vreg_device.hip' in build.SOURCES
    out = tmp_path / 'vreg_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vreg_device.hip'],
                       cwd=os.path.dirname(SOURCE), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    counts = {k: sum(k in name for name in recs) for k in ('k_reg_hist', 'k_reg_minmax', 'k_reg_quantise', 'k_reg_shrink', 'k_reg_linear', 'k_reg_nearest')}
    assert counts == dict(k_reg_hist=2, k_reg_minmax=2, k_reg_quantise=2, k_reg_shrink=3, k_reg_linear=2, k_reg_nearest=5), sorted(recs)
    assert len(recs) == 16, sorted(recs)
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        # the cross-compile gives: k_reg_hist 45 (float32) and 48 (float64); k_reg_linear 41 and 44; k_reg_shrink 32 (mask), 28 and 38; k_reg_nearest 24
        # and 26; k_reg_minmax 14 and 16; k_reg_quantise 14.  The largest, 48, is a multiple of 8 as it stands.
        assert vgprs <= 48, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ no GPU needed: the histogram's walk
# A stand-alone host program over csrc/vreg_walk.h, the code k_reg_hist runs: from every start below the stride, advance_split must
# reproduce split(v) - and both the plain quotients and remainders of v - at every trip up to V.  argv: n0 n1 n2, repeated.
# Per shape and stride it prints the steps checked and, of the advances into a live trip, how many carried on k, on j, on both.
WALK_PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "vreg_walk.h"

int main(int argc, char** argv) {
    const int64_t groups[] = {1, 2, 3, 7, 1024};
    long bad = 0;
    for (int a = 1; a + 2 < argc; a += 3) {
        const Ext n{std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2])};
        const int64_t V = (int64_t)n.n0 * n.n1 * n.n2;
        for (int64_t g : groups) {
            const int64_t stride = g * 256;
            int di, dj, dk;
            split(stride, n, di, dj, dk);
            if (dj >= n.n1 || dk >= n.n2 || ((int64_t)di * n.n1 + dj) * n.n2 + dk != stride) { std::printf("split of the stride is wrong\n"); bad++; }
            long long steps = 0, ck = 0, cj = 0, cb = 0, trips = 0;
            for (int64_t start = 0; start < stride && start < V; start++) {
                int i, j, k;
                split(start, n, i, j, k);
                long long t = 0;
                for (int64_t v = start; v < V; v += stride) {
                    const int64_t wi = v / ((int64_t)n.n1 * n.n2), wj = (v / n.n2) % n.n1, wk = v % n.n2;
                    int si, sj, sk;
                    split(v, n, si, sj, sk);
                    if (i != wi || j != wj || k != wk || si != wi || sj != wj || sk != wk) {
                        if (bad < 5) std::printf("(%d, %d, %d) stride %lld voxel %lld: walked (%d, %d, %d), split (%d, %d, %d), is (%lld, %lld, %lld)\n", n.n0, n.n1, n.n2,
                                                 (long long)stride, (long long)v, i, j, k, si, sj, sk, (long long)wi, (long long)wj, (long long)wk);
                        bad++;
                    }
                    steps++; t++;
                    if (v + stride < V) {
                        const bool kc = k + dk >= n.n2, jc = j + (kc ? 1 : 0) + dj >= n.n1;
                        ck += kc; cj += jc; cb += kc && jc;
                    }
                    advance_split(n, di, dj, dk, i, j, k);
                }
                if (t > trips) trips = t;
            }
            std::printf("walk %d %d %d %lld steps %lld trips %lld carries %lld %lld %lld\n", n.n0, n.n1, n.n2, (long long)stride, steps, trips, ck, cj, cb);
        }
    }
    std::printf(bad ? "FAILED %ld\n" : "OK\n", bad);
    return bad ? 1 : 0;
}
"""

CARRY_SHAPES = [(70, 61, 63), (130, 64, 65)]             # k_reg_hist takes carries on its second (and third) trip: test_carry_shapes_take_carries
WALK_SHAPES = [(3, 5, 17477)] + CARRY_SHAPES + [(9, 241, 121), (1, 1, 262145), (641, 409, 1), (263, 1, 997), (2, 2, 2),
                                                 (1, 211, 307), (97, 1, 701), (211, 307, 1),                      # each extent 1
                                                 (5, 7, 11), (30, 29, 30), (13, 30, 5), (23, 6, 29), (17, 17, 17)]   # trips in the hundreds at g = 1


def _walk_carries(n, stride=None):
    """A restatement of k_reg_hist's walk in numpy, every start at once: (trips, and of the advances into a live trip the number that
    carry on k, on j, on both at once).  The stride is the kernel's: min(ceil(V / G), WORKGROUPS) workgroups of G voxels.
    The walked (i, j, k) is checked against the quotients and remainders at every trip."""
    n0, n1, n2 = n
    V = n0 * n1 * n2
    S = min(-(-V // G), WORKGROUPS) * G if stride is None else stride
    di, dj, dk = S // (n1 * n2), (S // n2) % n1, S % n2
    v = np.arange(min(S, V), dtype=np.int64)
    i, j, k = v // (n1 * n2), (v // n2) % n1, v % n2
    trips, ck, cj, cb = 0, 0, 0, 0
    while len(v):
        trips += 1
        assert np.array_equal(i, v // (n1 * n2)) and np.array_equal(j, (v // n2) % n1) and np.array_equal(k, v % n2), (n, trips)
        live = v + S < V
        k = k + dk
        kc = k >= n2
        k, j = np.where(kc, k - n2, k), j + kc + dj
        jc = j >= n1
        j, i = np.where(jc, j - n1, j), i + jc + di
        ck, cj, cb = ck + int((kc & live).sum()), cj + int((jc & live).sum()), cb + int((kc & jc & live).sum())
        keep = live
        v, i, j, k = (v + S)[keep], i[keep], j[keep], k[keep]
    return trips, ck, cj, cb


def test_carry_shapes_take_carries():
    """Why (70, 61, 63) and (130, 64, 65) are in the GPU tests: on the kernel's own stride, 1024 x 256 = 262 144 = split (68, 13, 1) and
    (63, 0, 64) there, voxels advance into a live second (third) trip with a carry on k, on j, and on both at once - at (130, 64, 65)
    dj = 0, so every j carry is a j of exactly n1.  At (3, 5, 17477), the older two-trip case, the 11 voxels of the second trip
    (k < 11, stride split (2, 4, 17466)) take none: a dropped or doubled carry would pass there."""
    assert _walk_carries((3, 5, 17477)) == (2, 0, 0, 0)
    assert _walk_carries((70, 61, 63)) == (2, 108, 820, 14)
    assert _walk_carries((130, 64, 65)) == (3, 274368, 4224, 4224)
    for n in CARRY_SHAPES:
        assert int(np.prod(n)) > WORKGROUPS * G and min(_walk_carries(n)[1:]) > 0
    assert (262144 // (64 * 65), (262144 // 65) % 64, 262144 % 65) == (63, 0, 64) and (262144 // (61 * 63), (262144 // 63) % 61, 262144 % 63) == (68, 13, 1)
    assert 2 * 262144 < 130 * 64 * 65 < 3 * 262144 and 262144 < 70 * 61 * 63 < 2 * 262144


def test_walk_reproduces_split_at_every_trip(tmp_path):
    """csrc/vreg_walk.h on the host: every start below the stride, every trip up to V, strides g x 256 for g in 1, 2, 3, 7, 1024,
    over WALK_SHAPES; the carries the program counts on the kernel's own stride are the restatement's."""
    cxx = os.environ.get('CXX', 'g++')
    src, exe = tmp_path / 'walk.cpp', tmp_path / 'walk'
    src.write_text(WALK_PROGRAM)
    p = subprocess.run([cxx, '-O1', '-std=c++17', '-I', os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)] + [str(e) for n in WALK_SHAPES for e in n], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), r.stdout[-3000:]
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f and f[0] == 'walk':
            rows[(int(f[1]), int(f[2]), int(f[3])), int(f[4])] = (int(f[6]), int(f[8]), tuple(int(x) for x in f[10:13]))
    assert len(rows) == 5 * len(WALK_SHAPES)
    most = 0
    for (n, stride), (steps, trips, carries) in rows.items():
        V = int(np.prod(n))
        assert steps == V and trips == -(-V // stride), (n, stride)                        # every voxel is on exactly one start's walk
        assert (trips,) + carries == _walk_carries(n, stride), (n, stride)
        most = max(most, trips)
    assert most >= 1000 and sum(t >= 100 for _, t, _ in rows.values()) >= 10              # long walks: (1, 1, 262145) at g = 1 has 1025 trips
    for n in CARRY_SHAPES:
        assert rows[n, WORKGROUPS * G][1:] == (_walk_carries(n)[0], _walk_carries(n)[1:])


# ------------------------------------------------------------------ GPU: the joint histogram
def _volume(shape, kind, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        v = 100.0 + 30.0 * rng.standard_normal(shape)
    elif kind == 'two':
        v = np.where(rng.random(shape) < 0.5, 10.0, 250.0)
    elif kind == 'constant':
        v = np.full(shape, 42.0)
    else:                                                    # a brain-like image: half background, a smooth part and noise
        g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape], indexing='ij')
        v = 100.0 + 60.0 * g[0] - 40.0 * g[1] * g[2] + 5.0 * rng.standard_normal(shape)
        v[rng.random(shape) < 0.5] = 0.0
    return v.astype(dtype)


def _mask(kind, shape, seed=0):
    if kind == 'full':
        return None
    if kind == 'random':
        return (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
    m = np.zeros(shape, np.uint8)
    if kind == 'one':
        m[tuple(n // 2 for n in shape)] = 1
    return m                                                 # 'empty'


def _scaled(n, m, shift=(0.0, 0.0, 0.0)):
    """The fixed grid stretched over the moving one, with a shift in moving voxels."""
    T = np.eye(4)
    for a in range(3):
        T[a, a] = (m[a] - 1.0) / (n[a] - 1.0) if n[a] > 1 else 0.0
        T[a, 3] = shift[a]
    return T


def _rotated(n, m, degrees=10.0):
    fA, mA = M.affine_of((0.8, 1.0, 1.6), n), M.affine_of((1.3, 0.9, 1.1), m, centre_at=(0.4, -0.3, 0.2))
    W = R.paramsToMatrix([0.7, -0.4, 0.3] + [np.deg2rad(degrees)] * 3, 6, np.zeros(3))
    return R.voxelMap(W, fA, mA)


def _check_hist(fixed, moving, T, B=64, mask='full', label=''):
    """The GPU's counts against the model's; returns (H, the number of voxels that take part)."""
    m = _mask(mask, fixed.shape)
    flo, fhi = M.extrema(fixed, m)
    if not np.isfinite(flo):                                 # an empty mask: every voxel is 255 whatever the bins are
        flo = fhi = 0.0
    fb, inside = M.quantise(fixed, flo, R.binScale(flo, fhi, B), B, m)
    mlo, mhi = M.extrema(moving)
    ms = R.binScale(mlo, mhi, B)
    before = (fb.copy(), moving.copy())
    want = M.joint_histogram(fb, moving, T, B, mlo, ms)
    got = R.jointHistogram(fb, moving, T, B, mlo, ms)
    assert got.dtype == np.uint64 and got.shape == (B, B), label
    assert np.array_equal(got, want), '{}: {} cells differ, sums {} and {}'.format(label, int((got != want).sum()), int(got.sum()), int(want.sum()))
    assert np.array_equal(R.jointHistogram(fb, moving, T, B, mlo, ms), got), label                      # a repeat is identical
    assert np.array_equal(fb, before[0]) and _same(moving, before[1]), label
    return got, inside


TRIP_SHAPES = [(3, 5, 17), (2, 4, 32), (1, 1, 257), (3, 9, 19)]            # G - 1, G, G + 1, 2 G + 1 voxels
FIXED_SHAPES = [(1, 1, 1), (2, 3, 1), (5, 7, 3), (33, 30, 41)] + TRIP_SHAPES
MOVING_SHAPES = [(7, 6, 5), (1, 6, 5), (7, 1, 5), (7, 6, 1), (1, 1, 1)]


def test_trip_shapes_are_around_the_trip_extent():
    assert [int(np.prod(s)) for s in TRIP_SHAPES] == [G - 1, G, G + 1, 2 * G + 1]


@pytest.mark.gpu
@pytest.mark.parametrize('n', FIXED_SHAPES, ids=['x'.join(map(str, s)) for s in FIXED_SHAPES])
def test_joint_histogram_is_the_model_at_every_shape(n):
    fixed = _volume(n, 'brain', 1)
    for k, m in enumerate(MOVING_SHAPES):
        moving = _volume(m, 'noise', 2 + k, np.float32 if k % 2 else np.float64)
        for label, T in (('stretched', _scaled(n, m)), ('half a voxel', _scaled(n, m, (0.5, -0.5, 0.5))), ('rotated', _rotated(n, m))):
            for B, mask in ((64, 'full'), (8, 'random'), (128, 'one')):
                H, inside = _check_hist(fixed, moving, T, B, mask, '{} {} {} B {} mask {}'.format(n, m, label, B, mask))
                assert int(H.sum()) <= inside
                if label == 'stretched':
                    assert int(H.sum()) == inside                  # every voxel of the mask is inside


@pytest.mark.gpu
def test_joint_histogram_when_the_stride_loop_runs_twice():
    n = (3, 5, 17477)
    assert int(np.prod(n)) > WORKGROUPS * G
    fixed = _volume(n, 'brain', 3)
    moving = _volume((4, 6, 301), 'noise', 4, np.float32)
    H, inside = _check_hist(fixed, moving, _scaled(n, moving.shape), 64, 'random', 'two trips')
    assert int(H.sum()) > 0.9 * inside and int(H.sum(axis=1).max()) > inside // 3       # the background's row holds its half


def _turned(n, m, degrees=10.0, shrink=0.7):
    """The fixed grid shrunk to `shrink` of the moving one's extent and turned about the two centres by `degrees` on every axis: no
    coefficient of the map is zero, and at 0.7 every fixed voxel, the last ones in raster order too, lies inside the moving volume."""
    rot = R.paramsToMatrix([0.0, 0.0, 0.0] + [np.deg2rad(degrees)] * 3, 6, np.zeros(3))[:3, :3]
    scale = np.array([shrink * (m[a] - 1.0) / (n[a] - 1.0) if n[a] > 1 else 0.0 for a in range(3)])
    T = np.eye(4)
    T[:3, :3] = rot * scale[None, :]
    T[:3, 3] = (np.array(m) - 1.0) / 2.0 - T[:3, :3] @ ((np.array(n) - 1.0) / 2.0)
    return T


def _inside_from(T, n, m, first):
    """How many fixed voxels of raster index >= first the map puts inside the moving volume."""
    p = M._coords(T, n)
    inside = np.ones(n, bool)
    for a in range(3):
        inside &= (p[a] >= 0.0) & (p[a] <= m[a] - 1.0)
    return int(inside.ravel()[first:].sum())


@pytest.mark.gpu
@pytest.mark.parametrize('n,dtype', [((70, 61, 63), np.float32), ((130, 64, 65), np.float64)], ids=['70x61x63-float32', '130x64x65-float64'])
def test_joint_histogram_where_the_walk_carries(n, dtype):
    """269 010 and 540 800 fixed voxels against the 262 144 of one trip of the whole grid: a second, and a third, trip whose voxels
    advance with carries on k, on j and on both (test_carry_shapes_take_carries counts them: 108 / 820 / 14 and 274 368 / 4 224 /
    4 224).  Under the turned maps a wrong i or j cannot hide behind a zero coefficient.  The stretched, the late half-voxel and the
    turned map put voxels of every later trip inside the moving volume; the maps '_scaled + (0.5, -0.5, 0.5)' and '_rotated' are run
    as well, though at (70, 61, 63) they leave the last two planes, which are the second trip, outside."""
    assert n in CARRY_SHAPES
    V, m = int(np.prod(n)), (22, 19, 21)
    trips = -(-V // (WORKGROUPS * G))
    fixed, moving = _volume(n, 'brain', 20), _volume(m, 'noise', 21, dtype)
    maps = [('stretched', _scaled(n, m), True), ('half a voxel', _scaled(n, m, (0.5, -0.5, 0.5)), False), ('rotated', _rotated(n, m), False),
            ('half a voxel, late', _scaled(n, m, (-0.5, 0.5, -0.5)), True), ('turned', _turned(n, m), True), ('turned, partly outside', _turned(n, m, 25.0, 1.1), True)]
    for label, T, late in maps:
        if late:                                             # the last trip counts voxels
            assert _inside_from(T, n, m, (trips - 1) * WORKGROUPS * G) > 0, label
        for B, mask in ((64, 'full'), (64, 'random')) + (((128, 'random'),) if label == 'turned' else ()):
            H, inside = _check_hist(fixed, moving, T, B, mask, '{} {} B {} mask {}'.format(n, label, B, mask))
            assert 0 < int(H.sum()) <= inside
            if label in ('stretched', 'turned'):
                assert int(H.sum()) == inside                    # every voxel of the mask is inside
            if mask == 'full' and label != 'rotated':
                assert int(H.sum()) == _inside_from(T, n, m, 0) > V // 3


@pytest.mark.gpu
def test_joint_histogram_identity_shifts_and_outside():
    n = (9, 11, 13)
    v = _volume(n, 'noise', 5)
    for B in (8, 64, 128):
        for mask in ('full', 'random', 'one', 'empty'):
            H, inside = _check_hist(v, v, np.eye(4), B, mask, 'identity B {} {}'.format(B, mask))
            assert int(H.sum()) == inside                        # every voxel of the mask is inside
            if mask == 'full':
                assert not (H - np.diag(np.diag(H))).any()       # fixed == moving, binned between the same extrema: H is diagonal
            if mask == 'empty':
                assert inside == 0 and not H.any()               # a bin image of 255 only: H = 0, not an error
    for shift in ((1.0, 0.0, 0.0), (0.0, -2.0, 0.0), (3.0, 1.0, -4.0)):
        T = np.eye(4)
        T[:3, 3] = shift
        H, _ = _check_hist(v, v, T, 64, 'full', 'shift {}'.format(shift))
        assert int(H.sum()) == int(np.prod([e - abs(s) for e, s in zip(n, shift)]))
    for label, T in (('far away', _scaled(n, n, (100.0, 0.0, 0.0))), ('behind', _scaled(n, n, (0.0, 0.0, -13.0)))):
        assert not _check_hist(v, v, T, 64, 'full', label)[0].any()                 # every voxel outside: H = 0
    T = np.diag([1e308, 1e308, 1e308, 1.0])                    # a finite map whose p overflows: inf, and inf - inf, are outside
    T[:3, 3] = 1e308
    assert not _check_hist(v, v, T, 64, 'full', 'p = inf')[0].any()
    T[:3, 3] = -1e308
    assert int(_check_hist(v, v, T, 64, 'full', 'p = inf - 1e308')[0].sum()) == 1     # index 1 on every axis lands on p = 0


@pytest.mark.gpu
def test_joint_histogram_borders_count_as_inside_and_one_ulp_beyond_does_not():
    n = (6, 7, 8)
    v = _volume(n, 'noise', 6)
    V = int(np.prod(n))
    planes = [V // e for e in n]
    assert int(_check_hist(v, v, np.eye(4), 64, 'full', 'p = 0 and p = m - 1')[0].sum()) == V
    for a in range(3):
        T = np.eye(4)
        T[a, 3] = -5e-324                                        # p = -5e-324 at index 0 (outside), p = i at i > 0
        assert int(_check_hist(v, v, T, 64, 'full', 'one ulp below 0 on axis %d' % a)[0].sum()) == V - planes[a]
        T[a, 3] = np.spacing(float(n[a] - 1))                    # p = nextafter(m - 1) at the last index (outside)
        assert int(_check_hist(v, v, T, 64, 'full', 'one ulp above m - 1 on axis %d' % a)[0].sum()) == V - planes[a]
        # p = -0.0 for every voxel, on an axis where the moving volume has one voxel: inside
        T = np.eye(4)
        T[a, :] = -0.0
        moving = np.take(v, [2], axis=a)
        assert np.signbit(M._coords(T, n)[a]).all()
        assert int(_check_hist(v, moving, T, 64, 'full', 'p = -0.0 on axis %d' % a)[0].sum()) == V


@pytest.mark.gpu
def test_joint_histogram_contention_two_levels_and_non_finite_values():
    n = (64, 64, 64)
    c = _volume(n, 'constant', 0)
    H, inside = _check_hist(c, c.astype(np.float32), np.eye(4), 64, 'full', 'constant 64^3')
    assert inside == 262144 and int(H[0, 0]) == 262144 and int(H.sum()) == 262144       # every count in one cell
    n = (12, 10, 9)
    for dtype in (np.float32, np.float64):
        two, noise = _volume(n, 'two', 7, dtype), _volume(n, 'noise', 8, dtype)
        H, _ = _check_hist(two.astype(np.float64), two, np.eye(4), 8, 'full', 'two levels')
        assert int(np.count_nonzero(H)) == 2 and H[0, 0] and H[7, 7]
        _check_hist(two.astype(np.float64), noise, _rotated(n, n), 64, 'random', 'two levels against noise')
        wild_f, wild_m = noise.astype(np.float64), noise.copy()
        wild_f[1, 2, 3], wild_f[5, 5, 5] = np.nan, np.inf
        wild_m[2, 2, 2], wild_m[7, 3, 4], wild_m[11, 9, 8] = np.nan, -np.inf, np.inf
        H, inside = _check_hist(wild_f, wild_m, np.eye(4), 64, 'full', 'nan and inf, identity')
        # a sample that touches a value that is not finite is not finite, even where its weight is 0: each of the three takes the 8 voxels
        # with it whose 2 x 2 x 2 neighbourhood holds it (at the far corner the clamped neighbours); the two of the fixed volume lie elsewhere
        assert inside == int(np.prod(n)) - 2 and int(H.sum()) == int(np.prod(n)) - 2 - 3 * 8
        H, inside = _check_hist(wild_f, wild_m, _scaled(n, n, (0.5, 0.5, 0.5)), 64, 'full', 'nan and inf, half a voxel')
        assert 0 < int(H.sum()) < inside - 8


# ------------------------------------------------------------------ GPU: extrema, bin image, pyramid, resampled volume
SMALL_SHAPES = [(1, 1, 1), (2, 3, 1), (5, 7, 3), (33, 30, 41), (3, 5, 17), (1, 1, 257), (3, 9, 19)]


@pytest.mark.gpu
@pytest.mark.parametrize('n', SMALL_SHAPES, ids=['x'.join(map(str, s)) for s in SMALL_SHAPES])
def test_extrema_quantise_and_shrink_are_the_model(n):
    for dtype in (np.float32, np.float64):
        v = _volume(n, 'brain', 9, dtype)
        if v.size > 4:
            v.flat[1], v.flat[3] = np.nan, np.inf
        for kind in ('full', 'random', 'one', 'empty'):
            m = _mask(kind, n)
            before = v.copy()
            got, want = R.extrema(v, m), M.extrema(v, m)
            assert got == want, (n, dtype, kind, got, want)
            if not np.isfinite(want[0]):                         # no finite voxel in the mask
                continue
            for B in (8, 64, 128):
                s = R.binScale(want[0], want[1], B)
                (gb, gi), (wb, wi) = R.quantise(v, want[0], s, B, m), M.quantise(v, want[0], s, B, m)
                assert _same(gb, wb) and gi == wi, (n, dtype, kind, B, int((gb != wb).sum()))
                assert gb[gb != 255].max(initial=0) <= B - 1
            assert _same(v, before)
        finite = np.nan_to_num(v, nan=1.0, posinf=2.0)
        got, want = R.shrink(finite), M.shrink(finite)
        assert got.dtype == np.float64 and got.shape == tuple((e + 1) // 2 for e in n)
        assert np.array_equal(_bits(got), _bits(want)), (n, dtype, int((got != want).sum()))
    for kind in ('random', 'one', 'empty'):
        m = _mask(kind, n)
        got, want = R.shrink(m, mask=True), M.shrink(m, mask=True)
        assert _same(got, want) and got.dtype == np.uint8, (n, kind)
    assert _same(R.shrink(np.ones(n, bool), mask=True), np.ones([(e + 1) // 2 for e in n], np.uint8))
    small = np.round(_volume(n, 'brain', 15)).astype(np.uint8)          # a uint8 VOLUME is no mask: its block mean
    assert np.array_equal(_bits(R.shrink(small)), _bits(M.shrink(small.astype(np.float64)))) and np.array_equal(_bits(M.shrink(small)), _bits(R.shrink(small)))


@pytest.mark.gpu
def test_shrink_is_the_block_mean_and_twice_is_the_pyramid():
    v = np.arange(6 * 4 * 2, dtype=np.float64).reshape(6, 4, 2)
    assert np.array_equal(R.shrink(v), v.reshape(3, 2, 2, 2, 1, 2).mean(axis=(1, 3, 5)))
    odd = _volume((9, 7, 5), 'noise', 10)
    once = R.shrink(odd)
    corner = 0.0
    for _ in range(8):
        corner = corner + odd[8, 6, 4]
    assert once.shape == (5, 4, 3) and once[4, 3, 2] == 0.125 * corner               # the far corner is clamped onto itself, eight times
    assert np.array_equal(_bits(R.shrink(once)), _bits(M.shrink(M.shrink(odd))))


@pytest.mark.gpu
@pytest.mark.parametrize('n', SMALL_SHAPES, ids=['x'.join(map(str, s)) for s in SMALL_SHAPES])
def test_resample_is_the_model(n):
    for k, m in enumerate(MOVING_SHAPES[:4]):
        maps = (_scaled(n, m), _scaled(n, m, (0.5, -0.5, 0.5)), _rotated(n, m), _scaled(n, m, (100.0, 0.0, 0.0)))
        for dtype in (np.float32, np.float64):
            moving = _volume(m, 'noise', 11 + k, dtype)
            moving.flat[0] = np.nan
            before = moving.copy()
            for T in maps:
                for fill in (0.0, -7.5, float('nan')):
                    got, want = R.resample(moving, T, n, order=1, fill=fill), M.resample(moving, T, n, order=1, fill=fill)
                    assert got.dtype == np.float64 and got.shape == tuple(n)
                    assert got.tobytes() == want.tobytes(), (n, m, dtype, fill, int((_bits(got) != _bits(want)).sum()))
            assert _same(moving, before)
        for dtype in R.NEAREST_TYPES:
            moving = (_volume(m, 'noise', 12 + k) * (1.0 if np.dtype(dtype).kind == 'f' else 0.5)).astype(dtype)
            for T in maps:
                got, want = R.resample(moving, T, n, order=0, fill=3), M.resample(moving, T, n, order=0, fill=3)
                assert _same(got, want), (n, m, dtype)
                assert set(np.unique(got)) <= set(np.unique(moving)) | {dtype(3)}
        far = R.resample(_volume(m, 'noise', 13), maps[3], n, order=1, fill=-7.5)
        assert (far == -7.5).all()                               # fill is written outside
        assert (R.resample(np.ones(m, np.int16), maps[3], n, order=0, fill=-9) == -9).all()
    assert R.resample(np.ones((3, 3, 3), bool), np.eye(4), (3, 3, 3), order=0).dtype == np.uint8
    W = R.paramsToMatrix([1.0, 2.0, 0.0, 0.1, 0.0, 0.0], 6, np.zeros(3))
    fA, mA = M.affine_of((1, 1, 2), (5, 6, 7)), M.affine_of((2, 1, 1), (4, 6, 8))
    mv = _volume((4, 6, 8), 'noise', 14)
    assert _same(R.resample(mv, (W, fA, mA), (5, 6, 7)), R.resample(mv, R.voxelMap(W, fA, mA), (5, 6, 7)))


# ---- the second turn of the passes that are capped at WORKGROUPS workgroups of 256 threads: voxels from 262 144 on
SECOND_TURN = WORKGROUPS * 256
LATE_SHAPE = (70, 61, 63)                                  # 269 010 voxels: 6 866 of them, the planes i >= 68 and a little more, on the second turn


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_extrema_and_quantise_on_the_second_turn(dtype):
    """k_reg_minmax and k_reg_quantise at 269 010 voxels > 262 144: the minimum and the maximum lie on the second turn only, and a NaN,
    an Inf and a voxel outside the mask out there get 255 and are not counted."""
    n = LATE_SHAPE
    V = int(np.prod(n))
    assert SECOND_TURN < V < 2 * SECOND_TURN
    v = _volume(n, 'brain', 30, dtype)
    at_min, at_max, at_nan, at_inf, at_out = SECOND_TURN, V - 1, SECOND_TURN + 257, V - 300, SECOND_TURN + 3000
    v.flat[at_min], v.flat[at_max], v.flat[at_nan], v.flat[at_inf] = -1234.5, 4321.0, np.nan, np.inf
    mask = _mask('random', n, 31)
    for at in (at_min, at_max, at_nan, at_inf):
        mask.flat[at] = 1
    mask.flat[at_out] = 0
    early = mask.copy()
    early.reshape(-1)[SECOND_TURN:] = 0
    before = v.copy()
    for label, m in (('no mask', None), ('mask', mask), ('a mask without the second turn', early)):
        got, want = R.extrema(v, m), M.extrema(v, m)
        assert got == want, (label, got, want)
        assert (got == (-1234.5, 4321.0)) == (m is not early), label
        for B in (64, 128):
            s = R.binScale(want[0], want[1], B)
            (gb, gi), (wb, wi) = R.quantise(v, want[0], s, B, m), M.quantise(v, want[0], s, B, m)
            assert _same(gb, wb) and gi == wi, (label, B, int((gb != wb).sum()), gi, wi)
            assert gb.flat[at_nan] == 255 and gb.flat[at_inf] == 255
            if m is None:
                assert gi == V - 2 and gb.flat[at_min] == 0 and gb.flat[at_max] == B - 1 and gb.flat[at_out] != 255
            elif m is mask:
                assert gi == int(mask.sum()) - 2 and gb.flat[at_out] == 255 and gb.flat[at_min] == 0 and gb.flat[at_max] == B - 1
            else:
                assert gi == int(early.sum()) and (gb.flat[SECOND_TURN:] == 255).all()
    assert _same(v, before)


@pytest.mark.gpu
def test_resample_on_the_second_turn():
    """k_reg_linear and k_reg_nearest at 269 010 voxels under a turned map that leaves voxels of the second turn inside and outside:
    the samples and the fill out there are the model's."""
    n, m = LATE_SHAPE, (22, 19, 21)
    T = _turned(n, m, 25.0, 1.1)
    late_inside = _inside_from(T, n, m, SECOND_TURN)
    assert 0 < late_inside < int(np.prod(n)) - SECOND_TURN
    for dtype in (np.float32, np.float64):
        moving = _volume(m, 'noise', 32, dtype)
        for fill in (-7.5, float('nan')):
            got, want = R.resample(moving, T, n, order=1, fill=fill), M.resample(moving, T, n, order=1, fill=fill)
            assert got.dtype == np.float64 and got.shape == n
            assert got.tobytes() == want.tobytes(), (dtype, fill, int((_bits(got) != _bits(want)).sum()))
        late = got.ravel()[SECOND_TURN:]
        assert int(np.isnan(late).sum()) == len(late) - late_inside           # the fill shows, and so do samples
    for dtype in (np.uint8, np.int16, np.float32):
        moving = (_volume(m, 'noise', 33) * (1.0 if np.dtype(dtype).kind == 'f' else 0.5)).astype(dtype)
        assert not (moving == dtype(250)).any()                  # a fill that shows
        got, want = R.resample(moving, T, n, order=0, fill=250), M.resample(moving, T, n, order=0, fill=250)
        assert _same(got, want), dtype
        late = got.ravel()[SECOND_TURN:]
        assert 0 < int((late == dtype(250)).sum()) < len(late)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [(130, 128, 130), (131, 127, 129)], ids=['130x128x130', '131x127x129'])
def test_shrink_when_the_output_takes_a_second_turn(n):
    """k_reg_shrink strides over its OUTPUT: (65, 64, 65) = 270 400 and (66, 64, 65) = 274 560 voxels > 262 144.  The odd extents
    end in a clamped block on every axis."""
    o = tuple((e + 1) // 2 for e in n)
    assert int(np.prod(o)) > SECOND_TURN
    v = _volume(n, 'noise', 34, np.float32)
    got, want = R.shrink(v), M.shrink(v)
    assert got.dtype == np.float64 and got.shape == o
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    mask = (np.random.default_rng(35).random(n) < 0.1).astype(np.uint8)
    got, want = R.shrink(mask, mask=True), M.shrink(mask, mask=True)
    assert got.dtype == np.uint8 and _same(got, want)
    assert 0 < int(got.ravel()[SECOND_TURN:].sum()) < got.size - SECOND_TURN


# ------------------------------------------------------------------ GPU: the loop
def _assert_same_run(got, want, label):
    (W, trace), (Wm, tm) = got, want
    assert np.array_equal(_bits(W), _bits(Wm)), (label, W, Wm)
    assert np.array_equal(trace['evaluations'], tm['evaluations']), (label, trace['evaluations'], tm['evaluations'])
    assert trace['steps'].shape == tm['steps'].shape and np.array_equal(_bits(trace['steps']), _bits(tm['steps'])), label
    assert np.array_equal(_bits(trace['params']), _bits(tm['params'])), label


@pytest.mark.gpu
def test_register_is_the_model_on_the_phantom():
    """The whole loop - pyramid, extrema, bin images, every histogram of the search - at levels=2: W and the trace, evaluation
    counts included, bit for bit; and the result registers the phantom."""
    fixed, fA, moving, mA, W_true = _pair(6)
    kw = dict(fixedAffine=fA, movingAffine=mA, levels=2)
    got = R.register(fixed, moving, **kw)
    _assert_same_run(got, M.register(fixed, moving, **kw), 'phantom')
    err = M.corner_error(got[0], W_true, SHAPE, fA)
    print('levels=2: corner error {:.3f}, evaluations {}'.format(err, got[1]['evaluations'].tolist()))
    assert err < min(SPACING) and len(got[1]['evaluations']) == 2


@pytest.mark.gpu
def test_register_is_the_model_with_12_parameters_a_mask_a_budget_and_a_grid():
    fixed, fA, moving, mA, _ = _pair(6, small=True)
    moving32 = moving.astype(np.float32)
    mask = (fixed > 0).astype(np.uint8)
    before = (fixed.copy(), moving32.copy(), mask.copy())
    kw = dict(fixedAffine=fA, movingAffine=mA, levels=2)
    got = R.register(fixed, moving32, dof=12, fixedMask=mask, maxEvaluations=150, **kw)
    _assert_same_run(got, M.register(fixed, moving32, dof=12, fixedMask=mask, maxEvaluations=150, **kw), 'dof 12')
    assert got[1]['steps'].shape[1] == 14 and len(got[1]['steps']) > 5
    again = R.register(fixed, moving32, dof=12, fixedMask=mask, maxEvaluations=150, **kw)
    assert got[0].tobytes() == again[0].tobytes() and got[1]['steps'].tobytes() == again[1]['steps'].tobytes()       # repeats are identical
    # a budget that ends each level in its midst
    got = R.register(fixed, moving32, maxEvaluations=31, cost='mi', **kw)
    _assert_same_run(got, M.register(fixed, moving32, maxEvaluations=31, cost='mi', **kw), 'budget')
    assert got[1]['evaluations'].tolist() == [31, 31]
    # a grid of 27 rotations first, from a start that is 20 degrees off
    start = np.array([0.0, 0.0, 0.0, np.deg2rad(-12.0), np.deg2rad(14.0), np.deg2rad(-10.0)])
    got = R.register(fixed, moving32, search=(20.0, 20.0), initial=start, cost='nmi', maxEvaluations=60, **kw)
    want = M.register(fixed, moving32, search=(20.0, 20.0), initial=start, cost='nmi', maxEvaluations=60, **kw)
    _assert_same_run(got, want, 'grid')
    assert got[1]['evaluations'][0] > 27 + 1 and got[1]['steps'][0, 0] == 0.0          # the grid's evaluations are counted on top
    turned = (got[1]['steps'][0, 4:7] - start[3:6]) / np.deg2rad(20.0)
    assert np.abs(turned - np.round(turned)).max() < 1e-12 and np.abs(turned).max() < 1.5      # the first row is a rotation of the grid
    assert _same(fixed, before[0]) and _same(moving32, before[1]) and _same(mask, before[2])
    with pytest.raises(ValueError):
        R.register(fixed, moving32, fixedMask=np.zeros(fixed.shape, np.uint8), **kw)              # an empty mask is refused


@pytest.mark.gpu
def test_register_and_main_take_integer_volumes_as_volumes(tmp_path):
    """uint8 and int16 copies give the float copy's pyramid, trace and W - from ``register`` and from ``main`` on uint8 files."""
    from arterynetwork_amd import nifti
    copies, fA, mA = _integer_copies()
    kw = dict(fixedAffine=fA, movingAffine=mA, levels=2, maxEvaluations=120)
    (f, m) = copies[0]
    want = R.register(f, m, **kw)
    _assert_same_run(want, M.register(f, m, **kw), 'float64 copy')
    for fi, mi in copies[1:]:
        before = (fi.copy(), mi.copy())
        assert np.array_equal(_bits(R.shrink(fi)), _bits(R.shrink(f))) and np.array_equal(_bits(R.shrink(mi)), _bits(R.shrink(m)))
        _assert_same_run(R.register(fi, mi, **kw), want, str(fi.dtype))
        assert _same(fi, before[0]) and _same(mi, before[1])
    folder = str(tmp_path)
    nifti.saveVolume(copies[1][0], fA, os.path.join(folder, 'brainVolume.nii.gz'))                    # saveVolume's default: uint8
    nifti.saveVolume(copies[1][1], mA, os.path.join(folder, 'followUp.nii.gz'))
    W, result = R.main(folder, 'followUp.nii.gz', levels=2, maxEvaluations=120)
    fA32, mA32 = nifti.loadVolume(folder, 'brainVolume.nii.gz')[1], nifti.loadVolume(folder, 'followUp.nii.gz')[1]
    Wf, _ = R.register(f, m, fixedAffine=fA32, movingAffine=mA32, levels=2, maxEvaluations=120)
    assert W.tobytes() == Wf.tobytes()
    assert np.array_equal(_bits(result), _bits(R.resample(m, (W, fA32, mA32), f.shape, order=1, fill=0)))


# ------------------------------------------------------------------ GPU: device pointers, in a process of their own
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import registration as R
import registration_model as M
from test_registration import _refusals, _volume, _rotated, _pair, N_REFUSALS, SENTINEL
dev = torch.device('cuda', 0)
n, m = (12, 10, 9), (11, 9, 10)
fixed, mask = _volume(n, 'brain', 1), (np.random.default_rng(0).random(n) < 0.5).astype(np.uint8)
T = _rotated(n, m)
for dtype in (np.float32, np.float64):
    moving = _volume(m, 'noise', 2, dtype)
    tf, tm, tk = torch.as_tensor(fixed, device=dev), torch.as_tensor(moving, device=dev), torch.as_tensor(mask, device=dev)
    lo, hi = R.extrema(tf, tk)
    assert (lo, hi) == R.extrema(fixed, mask) == M.extrema(fixed, mask)
    s = R.binScale(lo, hi, 64)
    tb, inside = R.quantise(tf, lo, s, 64, tk)
    hb, hinside = R.quantise(fixed, lo, s, 64, mask)
    assert tb.is_cuda and tb.dtype == torch.uint8 and tb.cpu().numpy().tobytes() == hb.tobytes() and inside == hinside
    mlo, mhi = R.extrema(tm)
    H = R.jointHistogram(tb, tm, T, 64, mlo, R.binScale(mlo, mhi, 64))
    assert isinstance(H, np.ndarray) and np.array_equal(H, R.jointHistogram(hb, moving, T, 64, mlo, R.binScale(mlo, mhi, 64))) and H.sum() > 0
    assert np.array_equal(H, R.jointHistogram(hb, tm, T, 64, mlo, R.binScale(mlo, mhi, 64)))         # a host bin image and a device volume
    sh = R.shrink(tm)
    assert sh.is_cuda and sh.dtype == torch.float64 and sh.cpu().numpy().tobytes() == R.shrink(moving).tobytes()
    sk = R.shrink(tk, mask=True)
    assert sk.is_cuda and sk.dtype == torch.uint8 and sk.cpu().numpy().tobytes() == R.shrink(mask, mask=True).tobytes()
    out = R.resample(tm, T, n, order=1, fill=-1.0)
    assert out.is_cuda and out.dtype == torch.float64 and out.cpu().numpy().tobytes() == R.resample(moving, T, n, order=1, fill=-1.0).tobytes()
    out = R.resample(tm, T, n, order=0, fill=-1.0)
    assert out.is_cuda and out.dtype == tm.dtype and out.cpu().numpy().tobytes() == R.resample(moving, T, n, order=0, fill=-1.0).tobytes()
    assert tm.cpu().numpy().tobytes() == moving.tobytes() and tf.cpu().numpy().tobytes() == fixed.tobytes()       # the inputs are unchanged
labels = torch.as_tensor((moving * 0.5).astype(np.int16), device=dev)
assert R.resample(labels, T, n, order=0, fill=-3).cpu().numpy().tobytes() == R.resample((moving * 0.5).astype(np.int16), T, n, order=0, fill=-3).tobytes()
fx, fA, mv, mA, _ = _pair(6, small=True)
kw = dict(fixedAffine=fA, movingAffine=mA, levels=2, maxEvaluations=60)
fx, mv = np.array(fx), np.array(mv)
W, trace = R.register(torch.as_tensor(fx, device=dev), torch.as_tensor(mv, device=dev), fixedMask=torch.as_tensor((fx > 0), device=dev), **kw)
Wh, th = R.register(fx, mv, fixedMask=(fx > 0), **kw)
assert W.tobytes() == Wh.tobytes() and trace['steps'].tobytes() == th['steps'].tobytes() and np.array_equal(trace['evaluations'], th['evaluations'])
print('DEVICE RESIDENT OK')

shape, mshape = (4, 5, 6), (3, 4, 5)
a = dict(fb=torch.zeros(shape, dtype=torch.uint8, device=dev), f64=torch.ones(mshape, dtype=torch.float64, device=dev),
         f32=torch.ones(mshape, dtype=torch.float32, device=dev), u8=torch.ones(mshape, dtype=torch.uint8, device=dev),
         H=torch.full((128, 128), SENTINEL, dtype=torch.int64, device=dev), bins=torch.full(shape, SENTINEL, dtype=torch.uint8, device=dev),
         out=torch.full(shape, -12345.0, dtype=torch.float64, device=dev), lohi=torch.full((2,), -12345.0, dtype=torch.float64, device=dev))
torch.cuda.synchronize()
res = _refusals(R._lib(), {{k: v.data_ptr() for k, v in a.items()}}, shape, mshape)
assert len(res) == N_REFUSALS
for label, rc in res:
    assert rc == -1, label
torch.cuda.synchronize()
assert bool((a['H'] == SENTINEL).all()) and bool((a['bins'] == SENTINEL).all()) and bool((a['out'] == -12345.0).all()) and bool((a['lohi'] == -12345.0).all())
assert bool((a['f64'] == 1.0).all()) and bool((a['fb'] == 0).all())
print('REFUSALS OK')
"""


@functools.lru_cache(maxsize=None)
def _device_run():
    script = DEVICE_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    return out.returncode, out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_registration_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, bit-identical to the host
    call; the inputs are unchanged.  Own process: torch is imported before the HIP library there."""
    rc, stdout, tail = _device_run()
    assert 'DEVICE RESIDENT OK' in stdout, tail


@pytest.mark.gpu
def test_registration_refusals_with_device_pointers():
    """Every refused input of the C entries, with device pointers: VRG_E_ARG, the sentinels in the outputs untouched."""
    rc, stdout, tail = _device_run()
    assert rc == 0 and 'REFUSALS OK' in stdout, tail


# ------------------------------------------------------------------ GPU: the files
@pytest.mark.gpu
def test_main_writes_the_registered_volume_and_the_matrix_and_a_mask_follows(tmp_path, capsys):
    from arterynetwork_amd import nifti
    fixed, fA, moving, mA, W_true = _pair(6, small=True)
    folder = str(tmp_path)
    nifti.saveVolume(fixed, fA, os.path.join(folder, 'brainVolume.nii.gz'), astype=np.float32)
    nifti.saveVolume(moving, mA, os.path.join(folder, 'followUp.nii.gz'), astype=np.float32)
    label = (moving > 60.0).astype(np.uint8) * 7
    nifti.saveVolume(label, mA, os.path.join(folder, 'followUpMask.nii.gz'))
    kw = dict(levels=2, maxEvaluations=80)
    W, result = R.main(folder, 'followUp.nii.gz', **kw)
    printed = capsys.readouterr().out
    for name in ('followUpRegistered.nii.gz', 'followUpToFixed.mat'):
        assert '{} saved to {}.'.format(name, os.path.join(folder, name)) in printed
    f32, m32 = fixed.astype(np.float32), moving.astype(np.float32)
    fA32, mA32 = nifti.loadVolume(folder, 'brainVolume.nii.gz')[1], nifti.loadVolume(folder, 'followUp.nii.gz')[1]
    want_W, _ = R.register(f32, m32, fixedAffine=fA32, movingAffine=mA32, **kw)
    assert W.tobytes() == want_W.tobytes()
    stored = np.loadtxt(os.path.join(folder, 'followUpToFixed.mat'))
    assert stored.shape == (4, 4) and stored.tobytes() == W.tobytes()                      # %.17g round-trips every double
    vol, aff = nifti.loadVolume(folder, 'followUpRegistered.nii.gz')
    want = R.resample(m32, (W, fA32, mA32), fixed.shape, order=1, fill=0)
    assert result.dtype == np.float64 and np.array_equal(_bits(result), _bits(want))
    assert vol.dtype == np.float32 and np.array_equal(vol, want.astype(np.float32)) and np.allclose(aff, fA)
    out = R.applyTransform(folder, 'followUpMask.nii.gz', 'followUpToFixed.mat', 'brainVolume.nii.gz')
    stored_mask, aff = nifti.loadVolume(folder, 'followUpMaskTransformed.nii.gz')
    assert out.dtype == np.uint8 and stored_mask.dtype == np.uint8 and np.array_equal(stored_mask, out) and np.allclose(aff, fA)
    assert np.array_equal(out, R.resample(label, (W, fA32, mA32), fixed.shape, order=0, fill=0)) and set(np.unique(out)) == {0, 7}
    smooth = R.applyTransform(folder, 'followUp.nii.gz', 'followUpToFixed.mat', 'brainVolume.nii.gz', order=1, outputName='again.nii.gz')
    assert np.array_equal(_bits(smooth), _bits(want)) and np.array_equal(nifti.loadVolume(folder, 'again.nii.gz')[0], vol)
