"""The tube model ("f21 tube model"): the brute-force model of tests/tube_model.py against answers worked out
by hand - integer tubes, balls, the tie rule, the plane of equal power, closed-form volumes - on the CPU; then the GPU
(vmask_tubes / `tubes.tubeVolume` / `graphTubes`) against the model bit for bit, and the invariants of the real chain."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_compartments as TC
import tube_model as UM
from conftest import ROOT
from arterynetwork_amd import phantoms as P
from arterynetwork_amd import tubes as T

KEYS = ('label', 'field', 'nearest', 'sizes', 'overlap')


def _table(branches):
    """offsets, positions, radius of a list of (points K x 3, radii K) branches."""
    off = np.cumsum([0] + [len(p) for p, _ in branches]).astype(np.int64)
    if not branches:
        return off, np.zeros((0, 3)), np.zeros(0)
    return off, np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p, _ in branches]), np.concatenate([np.broadcast_to(np.asarray(r, np.float64), (len(p),)) for p, r in branches])


# ------------------------------------------------------------------ CPU: the model by hand
def test_model_integer_tube_ball_and_zero_radius():
    shape = (16, 12, 12)
    i0, i1, i2 = np.indices(shape)
    R = 3
    off, pos, rad = _table([([(3, 6, 5), (7, 6, 5), (12, 6, 5)], R)])
    got = UM.tubes(shape, off, pos, rad)
    along = np.maximum(np.maximum(3 - i0, i0 - 12), 0)                    # beyond the ends: the caps
    want = along ** 2 + (i1 - 6) ** 2 + (i2 - 5) ** 2 <= R * R
    assert np.array_equal(got['label'] != 0, want) and want[5, 3, 5] and want[5, 6, 8] and not want[5, 4, 2] and want[0, 6, 5] and not want[0, 6, 6]
    assert got['sizes'].tolist() == [int(want.sum())] and got['overlap'].tolist() == [0] and got['missed'] == 0
    assert np.array_equal(got['nearest'][want], np.where(i0 <= 7, 0, 1)[want])              # i0 == 7: both primitives hold it at the same f, the first wins
    assert np.array_equal(got['field'][want], ((along ** 2 + (i1 - 6) ** 2 + (i2 - 5) ** 2) - R * R)[want].astype(np.float64)) and np.isinf(got['field'][~want]).all()
    # two equal entries: dd = 0, a ball
    off, pos, rad = _table([([(8, 6, 6), (8, 6, 6)], 4)])
    got = UM.tubes(shape, off, pos, rad)
    assert np.array_equal(got['label'] != 0, (i0 - 8) ** 2 + (i1 - 6) ** 2 + (i2 - 6) ** 2 <= 16)
    # radius 0: only the voxels whose centre is exactly on the segment (t = k / 4 is exact)
    off, pos, rad = _table([([(2, 2, 2), (6, 6, 6)], 0.0), ([(9, 3, 1), (9, 3, 9)], 0.0)])
    got = UM.tubes(shape, off, pos, rad)
    want = ((i0 == i1) & (i1 == i2) & (i0 >= 2) & (i0 <= 6)) | ((i0 == 9) & (i1 == 3) & (i2 >= 1) & (i2 <= 9))
    assert np.array_equal(got['label'] != 0, want) and (got['field'][want] == 0).all() and got['sizes'].tolist() == [5, 9]
    # a spacing: the same tube in units of 0.5
    off, pos, rad = _table([([(1.5, 3.0, 2.5), (6.0, 3.0, 2.5)], 1.5)])
    got = UM.tubes(shape, off, pos, rad, spacing=(0.5, 0.5, 0.5))
    assert np.array_equal(got['label'] != 0, np.maximum(np.maximum(3 - i0, i0 - 12), 0) ** 2 + (i1 - 6) ** 2 + (i2 - 5) ** 2 <= 9)


def test_model_tie_rule_and_the_plane_of_equal_power():
    shape = (14, 16, 9)
    i0, i1, i2 = np.indices(shape)
    tube = lambda c1, R: ([(2, c1, 4), (11, c1, 4)], R)
    # equal radii: on the mid-plane f is exactly equal and the smaller primitive index wins
    off, pos, rad = _table([tube(5, 3), tube(9, 3)])
    got = UM.tubes(shape, off, pos, rad)
    both = (got['label'] != 0) & ((i1 - 5) ** 2 + (i2 - 4) ** 2 <= 9) & ((i1 - 9) ** 2 + (i2 - 4) ** 2 <= 9) & (i0 >= 2) & (i0 <= 11)
    assert both.any() and (both & (i1 == 7)).any()
    assert np.array_equal(got['label'][both], np.where(i1 <= 7, 1, 2)[both]) and np.array_equal(got['nearest'][both], np.where(i1 <= 7, 0, 2)[both])
    swapped = UM.tubes(shape, *_table([tube(9, 3), tube(5, 3)]))
    assert np.array_equal(swapped['label'][both], np.where(i1 >= 7, 1, 2)[both])
    # custom labels and a dropped branch
    named = UM.tubes(shape, off, pos, rad, labels=[7, 3])
    assert np.array_equal(named['label'], np.array([0, 7, 3])[got['label']])
    dropped = UM.tubes(shape, off, pos, rad, keep=[0, 1])
    assert dropped['sizes'][0] == 0 and set(np.unique(dropped['label'])) == {0, 2}
    assert np.array_equal(dropped['label'] == 2, UM.tubes(shape, *_table([tube(9, 3)]))['label'] == 1)
    # the same geometry twice goes wholly to the first
    twice = UM.tubes(shape, *_table([tube(6, 3), tube(6, 3)]))
    assert twice['sizes'][0] > 0 and twice['sizes'][1] == 0 and set(np.unique(twice['label'])) == {0, 1}
    # radii 3 and 5 about i1 = 5 and 9: (y - 5)^2 - 9 = (y - 9)^2 - 25 at y = (5 + 9) / 2 + (9 - 25) / (2 (9 - 5)) = 5
    off, pos, rad = _table([tube(5, 3), tube(9, 5)])
    got = UM.tubes(shape, off, pos, rad)
    in1, in2 = (i1 - 5) ** 2 + (i2 - 4) ** 2 <= 9, (i1 - 9) ** 2 + (i2 - 4) ** 2 <= 25
    both = in1 & in2 & (i0 >= 2) & (i0 <= 11)
    assert (both & (i1 < 5)).any() and (both & (i1 == 5)).any() and (both & (i1 > 5)).any()
    assert np.array_equal(got['label'][both], np.where(i1 <= 5, 1, 2)[both])
    m = np.zeros(shape, np.uint8)
    m[:, :6] = 1
    masked = UM.tubes(shape, off, pos, rad, mask=m)
    assert masked['overlap'].tolist() == [int(((got['label'] == 1) & (m != 0)).sum()), int(((got['label'] == 2) & (m != 0)).sum())]
    assert masked['missed'] == int(((got['label'] == 0) & (m != 0)).sum()) and masked['missed'] + masked['overlap'].sum() == m.sum()


@functools.lru_cache(maxsize=None)
def _volume_errors():
    """Relative error of the model's volume against the closed form at spacing 1 and 0.5: a capsule of radius 6 and a truncated cone
    from 3 to 7, both oblique and off the grid."""
    out = {}
    for name, (A, B, rA, rB) in {'capsule': ((9.3, 10.1, 9.7), (21.4, 17.2, 13.9), 6.0, 6.0), 'cone': ((10.2, 9.6, 10.4), (22.1, 15.3, 19.8), 3.0, 7.0)}.items():
        L = float(np.linalg.norm(np.subtract(B, A)))
        exact = UM.capsule_volume(rA, L) if name == 'capsule' else UM.cone_volume(rA, rB, L)
        for h in (1.0, 0.5):
            n = int(round(32 / h))
            got = UM.tubes((n, n, n), [0, 2], [A, B], [rA, rB], spacing=(h, h, h))
            out[name, h] = abs(float(got['sizes'][0]) * h ** 3 - exact) / exact
    return out


def test_model_volume_against_the_closed_form():
    """Recorded: capsule 7.9e-4 at spacing 1 and 5.0e-4 at 0.5; truncated cone 8.5e-5 and 2.6e-5 (the assertion is only that the
    error shrinks)."""
    e = _volume_errors()
    for name in ('capsule', 'cone'):
        print(name, 'relative volume error {:.3e} at spacing 1, {:.3e} at 0.5'.format(e[name, 1.0], e[name, 0.5]))
        assert e[name, 0.5] < e[name, 1.0]


def test_arguments_are_checked_before_the_library_is_asked(monkeypatch):
    monkeypatch.setattr(T, '_lib', lambda: (_ for _ in ()).throw(AssertionError('the library was asked')))
    off, pos, rad = _table([([(2, 2, 2), (5, 5, 5), (6, 6, 7)], 1.0), ([(1, 2, 3), (3, 2, 1)], 2.0)])
    ok = dict(shape=(8, 8, 8), offsets=off, positions=pos, radius=rad)
    bad = lambda k, v: dict(ok, **{k: v})
    nan_p, inf_r, neg_r, far_p, far_r = pos.copy(), rad.copy(), rad.copy(), pos.copy(), rad.copy()
    nan_p[1, 2], inf_r[0], neg_r[4], far_p[3, 0], far_r[2] = np.nan, np.inf, -1e-9, -(2.0 ** 20) * 1.0000001, 2.0 ** 21
    for kw in (bad('shape', (8, 8)), bad('shape', (0, 8, 8)), bad('shape', (2048, 2048, 512)), bad('spacing', (1.0, 0.0, 1.0)), bad('spacing', (1.0, np.nan, 1.0)),
               bad('spacing', (0.001, float(np.nextafter(1.0, 2.0)), 0.5)), bad('offsets', [1, 3, 5]), bad('offsets', [0, 4, 5]), bad('offsets', [0, 3, 4]), bad('offsets', [0, 3]),
               bad('offsets', []), bad('positions', pos[:4]), bad('radius', rad[:4]), bad('positions', nan_p), bad('radius', inf_r), bad('radius', neg_r), bad('positions', far_p),
               bad('radius', far_r), bad('keep', [1]), bad('labels', [1, 0]), bad('labels', [1, -2]), bad('labels', [1, 2, 3]), bad('labels', [1, 2 ** 31]),
               bad('mask', np.ones((8, 8, 7), np.uint8))):
        with pytest.raises(ValueError):
            T.tubeVolume(**kw)
    with pytest.raises(AssertionError, match='the library was asked'):
        T.tubeVolume(**ok)
    assert T.modelVolumes([2, 0, 5], (0.5, 0.5, 0.8)).tolist() == [2 * 0.2, 0.0, 5 * 0.2]
    assert np.allclose(T.cylinderVolumes([2.0, 3.0], [1.0, 0.5]), [2 * np.pi, 0.75 * np.pi], rtol=1e-15)
    lab = np.array([[0, 2], [1, 3]])
    assert T.paintBranches(lab, np.array([1.5, 2.5, 3.5]), fill=-1.0).tolist() == [[-1.0, 2.5], [1.5, 3.5]]
    with pytest.raises(ValueError):
        T.paintBranches(lab, np.array([1.5, 2.5]))
    m = T.TubeModel()
    m.sizes, m.overlap, m.missed, m.hasMask = np.array([4, 0, 6]), np.array([3, 0, 6]), 1, True
    a = T.agreement(m)
    assert a['precision'][[0, 2]].tolist() == [0.75, 1.0] and np.isnan(a['precision'][1]) and a['recall'] == 0.9 and a['dice'] == 18 / 20 and a['maskVoxels'] == 10


def test_main_refuses_tubes_without_its_stages(tmp_path):
    from arterynetwork_amd import skeletonization as S
    for kw in (dict(segments=True), dict(segments=True, prune=(0, 0.0)), dict(segments=True, morphometry=True)):
        with pytest.raises(ValueError):
            S.main(str(tmp_path), tubes=True, **kw)


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_tube_kernels_use_no_scratch(tmp_path):
    import re
    from arterynetwork_amd import build
    assert 'vtube_device.hip' in build.SOURCES
    out = tmp_path / 'vtube_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vtube_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
        recs[m.group(1)] = (f('private_segment_fixed_size'), f('vgpr_count'))
    for frag in ('k_tube_check', 'k_tube_owner', 'k_tube_binILb0', 'k_tube_binILb1', 'k_tube_stats', 'k_tube_occupied', 'k_tube_eval', 'k_tube_fillILi1', 'k_tube_fillILi4'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, (scratch, vgpr) in recs.items():
        if 'k_tube' not in name:                                          # (the library's scan kernels)
            continue
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        assert vgpr <= 64, '%s uses %d VGPRs' % (name, vgpr)               # eight waves per SIMD


# ------------------------------------------------------------------ GPU: exactly the model
def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, np.float64).view(np.uint64) if a.dtype == np.float64 else a


def _assert_equal_to_model(got, want):
    for k in KEYS:
        a, b = np.asarray(getattr(got, k)), want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        same = _bits(a) == _bits(b)
        assert same.all(), (k, int((~same).sum()), 'of', same.size, 'first at', np.argwhere(~same)[0].tolist(), a[~same][:3], b[~same][:3])
    assert got.missed == want['missed']


def _check(shape, table, spacing=None, **kw):
    off, pos, rad = table
    info = {}
    got = T.tubeVolume(shape, off, pos, rad, spacing=spacing, return_field=True, return_nearest=True, info=info, **kw)
    want = UM.tubes(shape, off, pos, rad, spacing=spacing, **kw)
    _assert_equal_to_model(got, want)
    assert got.counts['primitives'] == len(UM.primitives(off, kw.get('keep'))[0]) and info['pairs'] == got.counts['pairs'] >= got.counts['occupiedBricks']
    plain = T.tubeVolume(shape, off, pos, rad, spacing=spacing, **kw)       # without the optional outputs
    assert plain.field is None and plain.nearest is None and plain.label.tobytes() == got.label.tobytes() and plain.sizes.tobytes() == got.sizes.tobytes()
    return got, want


def _random_table(shape, nbranch, seed, rmin, rmax, spacing=(1.0, 1.0, 1.0), margin=0.0, most=5):
    """Branches of 2 to `most` entries: a start inside the volume (widened by `margin` of it on every side), steps of about two voxels."""
    rng = np.random.default_rng(seed)
    h, n = np.asarray(spacing, np.float64), np.asarray(shape, np.float64)
    out = []
    for _ in range(nbranch):
        k = int(rng.integers(2, most + 1))
        start = (rng.random(3) * (1 + 2 * margin) - margin) * (n - 1)
        pts = start + np.cumsum(np.vstack([np.zeros(3), rng.normal(0.0, 1.5, (k - 1, 3))]), axis=0)
        out.append((pts * h, rng.uniform(rmin, rmax, k) * h.min()))
    return _table(out)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(5, 6, 7), (19, 21, 26), (33, 16, 9), (40, 24, 72)])
def test_shapes_and_primitives_across_bricks(shape):
    """One partial brick, extents that are no multiple of 8, several bricks per axis; primitives that straddle brick faces, edges
    and corners, partly and wholly outside the volume, one of radius 9 whose box covers at least three bricks per axis."""
    n = np.asarray(shape, np.float64)
    m = (np.random.default_rng(5).random(shape) < 0.4).astype(np.uint8)
    got, want = _check(shape, _random_table(shape, 25, 11, 0.3, 3.0, margin=0.3), mask=m)
    assert got.sizes.sum() > 0 and got.missed > 0
    corner = np.minimum(np.array([8.0, 8.0, 8.0]), n - 1)                  # the corner that eight bricks share
    special = [([corner - 0.6, corner + 0.7], 1.2), ([corner * [1, 1, 0.5] - [0.5, 0.4, 0], corner * [1, 1, 0.5] + [0.5, 0.4, 0.3]], 0.9),
               ([corner * [1, 0.5, 0.5] - [0.5, 0, 0], corner * [1, 0.5, 0.5] + [0.5, 0.2, 0.1]], 0.8),
               ([n / 2 - 0.3, n / 2 + [1.1, 0.4, 0.2]], 9.0),                                        # radius 9: at least three bricks per axis where the volume has them
               ([[-3.0, -2.5, -4.0], [2.0, 1.5, 1.0]], [1.0, 2.5]), ([n + 1.5, n - 2.0], [2.0, 1.0]),  # partly outside, from either side
               ([[-30.0, 2.0, 2.0], [-20.0, 3.0, 2.0]], 2.0), ([n + 40.0, n + 45.0], 3.0),           # wholly outside
               ([[2.0, n[1] + 0.9, 3.0], [3.0, n[1] + 1.0, 3.0]], 1.0)]                              # outside, but its widened box touches the volume
    got, want = _check(shape, _table(special), mask=m)
    assert want['sizes'][3] > 0 and want['sizes'][6] == want['sizes'][7] == 0
    if min(shape) >= 24:
        assert got.counts['longestList'] >= 1 and got.counts['occupiedBricks'] >= 27
    _check(shape, _table(special), spacing=(0.5, 0.25, 2.0), mask=m)


def _coil(nprim):
    """nprim primitives of 0.02 voxels each on a circle of radius 1 about (3.5, 3.5, 3.5), drifting along axis 0; radius 0.9 to 1:
    every box stays inside the brick of the voxels 0 .. 7."""
    s = np.arange(nprim + 1) * 0.02
    pts = np.stack([3.2 + 0.0005 * np.arange(nprim + 1), 3.5 + np.cos(s), 3.5 + np.sin(s)], axis=1)
    return _table([(pts, 0.9 + 0.1 * np.cos(7 * s) ** 2)])


@pytest.mark.gpu
@pytest.mark.parametrize('nprim', [1, 255, 256, 257, 511, 512, 513, 600])
def test_list_lengths_around_the_lds_chunks(nprim):
    """A finely sampled branch inside one brick: its list is as long as the branch has primitives - fewer than, exactly and more than
    one and two chunks of 256 records."""
    got, want = _check((12, 10, 9), _coil(nprim))
    assert got.counts == {'primitives': nprim, 'occupiedBricks': 1, 'pairs': nprim, 'longestList': nprim}
    assert got.sizes[0] > 0 and len(np.unique(want['nearest'])) >= min(nprim, 4)


@pytest.mark.gpu
@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (0.5, 0.5, 0.8)])
def test_dense_random_graph(spacing):
    """About 300 branches on 40^3 with radii 0.5 to 4 voxels: every voxel has many candidates; with keep, labels and a mask."""
    shape = (40, 40, 40)
    table = _random_table(shape, 300, 23, 0.5, 4.0, spacing=spacing, margin=0.05, most=3)
    rng = np.random.default_rng(29)
    m = (rng.random(shape) < 0.5).astype(np.uint8)
    got, want = _check(shape, table, spacing=spacing, mask=m)
    assert (want['label'] != 0).mean() > 0.25 and got.counts['longestList'] > 8
    keep = (rng.random(300) < 0.6).astype(np.uint8)
    labels = rng.permutation(300).astype(np.int32) * 3 + 5
    kept, _ = _check(shape, table, spacing=spacing, mask=m, keep=keep, labels=labels)
    assert (kept.sizes[keep == 0] == 0).all() and set(np.unique(kept.label)) <= set(labels[keep != 0].tolist()) | {0}


@pytest.mark.gpu
def test_empty_cases():
    shape = (9, 17, 8)
    m = (np.random.default_rng(3).random(shape) < 0.3).astype(np.uint8)
    for table, kw in ((_table([]), {}), (_random_table(shape, 6, 2, 0.5, 2.0), dict(keep=np.zeros(6, np.uint8))),
                      (_table([([[-50.0, 0, 0], [-40.0, 1, 1]], 2.0), ([[0.0, 90, 0], [1.0, 95, 1], [2.0, 99, 3]], 3.0)]), {})):
        got, want = _check(shape, table, mask=m, **kw)
        assert (got.label == 0).all() and np.isposinf(got.field).all() and (got.nearest == -1).all() and got.missed == m.sum()
        assert (got.sizes == 0).all() and got.counts['occupiedBricks'] == got.counts['pairs'] == got.counts['longestList'] == 0
    assert got.counts['primitives'] == 3


CANARY = 0x5A


def _raw_call(dll, shape, off, pos, rad, spacing=(1.0, 1.0, 1.0), keep=None, labels=None, mask=None):
    """vmask_tubes through ctypes with host pointers: every output inside a larger buffer of canary bytes.  Returns rc, the message,
    the outputs, whether every output is untouched, whether every canary around them is intact."""
    V, B, pad = int(np.prod(shape)), len(off) - 1, 64
    spec = [('label', np.int32, V), ('field', np.float64, V), ('nearest', np.int64, V), ('sizes', np.int64, B), ('overlap', np.int64, B), ('missed', np.int64, 1),
            ('counts', np.int64, 4)]
    raw = {k: np.full(2 * pad + n * np.dtype(dt).itemsize, CANARY, np.uint8) for k, dt, n in spec}
    view = {k: raw[k][pad:pad + n * np.dtype(dt).itemsize].view(dt) for k, dt, n in spec}
    h = np.array(spacing, np.float64)
    off, pos, rad = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(rad, np.float64)
    opt = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in ((keep, np.uint8), (labels, np.int32), (mask, np.uint8))]
    at = lambda a: None if a is None or not a.size else a.ctypes.data
    rc = dll.vmask_tubes(0, *shape, h.ctypes.data, at(off) if B else None, B, at(pos), at(rad), *(at(a) for a in opt), *(at(view[k]) or raw[k].ctypes.data + pad for k, _, _ in spec), None)
    untouched = all((raw[k] == CANARY).all() for k in raw)
    fenced = all((raw[k][:pad] == CANARY).all() and (raw[k][pad + view[k].nbytes:] == CANARY).all() for k in raw)
    return rc, dll.vmask_last_error(), {k: v.copy() for k, v in view.items()}, untouched, fenced


@pytest.mark.gpu
def test_c_abi_host_pointers_canaries_and_refusals():
    dll = T._lib()
    shape = (13, 9, 10)
    off, pos, rad = _random_table(shape, 8, 31, 0.5, 2.5)
    m = (np.random.default_rng(7).random(shape) < 0.5).astype(np.uint8)
    keep, labels = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8), np.arange(11, 19, dtype=np.int32)
    rc, msg, out, untouched, fenced = _raw_call(dll, shape, off, pos, rad, keep=keep, labels=labels, mask=m)
    want = UM.tubes(shape, off, pos, rad, keep=keep, labels=labels, mask=m)
    assert rc == 0 and fenced and not untouched, (rc, msg)
    for k in KEYS:
        assert (_bits(out[k].reshape(want[k].shape)) == _bits(want[k])).all(), k
    assert out['missed'][0] == want['missed'] and out['counts'][0] == len(UM.primitives(off, keep)[0])
    bad = lambda **kw: _raw_call(dll, shape, **dict(dict(off=off, pos=pos, rad=rad, keep=keep, labels=labels, mask=m), **kw))
    nan_p, inf_p, nan_r, neg_r, far_p, far_r, zero_l, neg_l = pos.copy(), pos.copy(), rad.copy(), rad.copy(), pos.copy(), rad.copy(), labels.copy(), labels.copy()
    nan_p[3, 1], inf_p[0, 0], nan_r[5], neg_r[-1], far_p[2, 2], far_r[1], zero_l[2], neg_l[7] = np.nan, -np.inf, np.nan, -0.25, 2.0 ** 20 * 2.0000001, 2.0 ** 20 * 2.0000001, 0, -4
    short = off.copy(); short[3] = short[2] + 1
    late = off.copy(); late[0] = 1
    for kw, frag in ((dict(pos=nan_p), b'not finite'), (dict(pos=inf_p), b'not finite'), (dict(rad=nan_r), b'not finite'), (dict(rad=neg_r), b'negative'),
                     (dict(pos=far_p, spacing=(1.0, 2.0, 0.5)), b'2^20'), (dict(rad=far_r, spacing=(1.0, 2.0, 0.5)), b'2^20'), (dict(off=short), b'malformed'),
                     (dict(off=late), b'offsets'), (dict(labels=zero_l), b'label'), (dict(labels=neg_l), b'label'), (dict(spacing=(1.0, 0.0, 1.0)), b'spacing'),
                     (dict(spacing=(0.001, float(np.nextafter(1.0, 2.0)), 0.5)), b'spacing'), (dict(spacing=(1.0, float('inf'), 1.0)), b'spacing')):
        rc, msg, out, untouched, fenced = bad(**kw)
        assert rc == -1 and frag in msg and untouched, (kw.keys(), rc, msg)
    # the limit itself is accepted: |P| = r = 2^20 max(h); a spacing ratio of exactly 1000 too
    edge_p, edge_r = pos.copy(), rad.copy()
    edge_p[2, 2], edge_r[1] = -(2.0 ** 21), 2.0 ** 21
    rc, msg, out, untouched, fenced = bad(pos=edge_p, rad=edge_r, spacing=(1.0, 2.0, 0.5))
    assert rc == 0 and fenced, (rc, msg)
    want = UM.tubes(shape, off, edge_p, edge_r, spacing=(1.0, 2.0, 0.5), keep=keep, labels=labels, mask=m)
    assert np.array_equal(out['label'].reshape(shape), want['label']) and np.array_equal(out['nearest'].reshape(shape), want['nearest'])
    _check(shape, (off, pos, rad), spacing=(0.001, 1.0, 0.5))
    assert dll.vmask_tubes(0, 40000, 2, 2, None, None, 0, None, None, None, None, None, out['label'].ctypes.data, None, None, None, None, out['missed'].ctypes.data, None, None) == -1
    assert dll.vmask_tubes(0, *shape, None, None, 0, None, None, None, None, None, None, None, None, None, None, out['missed'].ctypes.data, None, None) == -1


@pytest.mark.gpu
def test_repeats_are_bit_identical():
    shape = (40, 40, 40)
    table = _random_table(shape, 300, 23, 0.5, 4.0, margin=0.05)
    m = (np.random.default_rng(29).random(shape) < 0.5).astype(np.uint8)
    a, b = (T.tubeVolume(shape, *table, mask=m, return_field=True, return_nearest=True) for _ in range(2))
    for k in KEYS:
        assert np.asarray(getattr(a, k)).tobytes() == np.asarray(getattr(b, k)).tobytes(), k
    assert a.missed == b.missed and a.counts == b.counts


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import ctypes as C
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import tubes as T
import test_tubes as TT
dev = torch.device('cuda', 0)
shape, h = (33, 16, 9), (0.5, 0.5, 0.8)
off, pos, rad = TT._random_table(shape, 40, 17, 0.5, 3.0, spacing=h, margin=0.1)
m = (np.random.default_rng(1).random(shape) < 0.5).astype(np.uint8)
keep = (np.arange(40) % 5 != 0).astype(np.uint8)
host = T.tubeVolume(shape, off, pos, rad, spacing=h, keep=keep, mask=m, return_field=True, return_nearest=True)
TT._assert_equal_to_model(host, TT.UM.tubes(shape, off, pos, rad, spacing=h, keep=keep, mask=m))
there = T.tubeVolume(shape, torch.as_tensor(off, device=dev), torch.as_tensor(pos, device=dev), torch.as_tensor(rad, device=dev), spacing=h,
                     keep=torch.as_tensor(keep, device=dev), mask=torch.as_tensor(m, device=dev), return_field=True, return_nearest=True)
for k in TT.KEYS:
    a, b = getattr(there, k), getattr(host, k)
    assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape, k
    assert a.cpu().numpy().tobytes() == b.tobytes(), k
assert there.missed == host.missed and there.counts == host.counts and there.label.dtype == torch.int32 and there.nearest.dtype == torch.int64
painted = T.paintBranches(there.label, torch.arange(40, dtype=torch.float64, device=dev) + 0.5, fill=-1.0)
assert painted.is_cuda and np.array_equal(painted.cpu().numpy(), T.paintBranches(host.label, np.arange(40) + 0.5, fill=-1.0))
# the C-ABI with device pointers: every output inside a larger device buffer of canary bytes; spacing on the device too.  (10, 9, 8) takes
# the fill of four voxels per thread when the outputs are 16-byte aligned (pad 64) and the one of one voxel when they are not (pad 72)
spec = lambda V, B: [('label', np.int32, V), ('field', np.float64, V), ('nearest', np.int64, V), ('sizes', np.int64, B), ('overlap', np.int64, B), ('missed', np.int64, 1), ('counts', np.int64, 4)]
for shp, pad, tab, kp, mk, want in ((shape, 64, (off, pos, rad), keep, m, host),) + tuple(
        ((10, 9, 8), pad, small, None, sm, T.tubeVolume((10, 9, 8), *small, spacing=h, mask=sm, return_field=True, return_nearest=True))
        for small, sm in ((TT._random_table((10, 9, 8), 3, 5, 0.5, 1.5, spacing=h), (np.random.default_rng(2).random((10, 9, 8)) < 0.5).astype(np.uint8)),) for pad in (64, 72)):
    V, B = int(np.prod(shp)), len(tab[0]) - 1
    raw = {{k: torch.full((2 * pad + n * np.dtype(dt).itemsize,), TT.CANARY, dtype=torch.uint8, device=dev) for k, dt, n in spec(V, B)}}
    ins = [torch.as_tensor(a, device=dev) for a in (np.array(h), tab[0], tab[1], tab[2], mk)]
    kd = None if kp is None else torch.as_tensor(kp, device=dev)
    torch.cuda.synchronize()
    assert all(raw[k].data_ptr() % 16 == 0 for k in raw)
    rc = T._lib().vmask_tubes(0, *shp, ins[0].data_ptr(), ins[1].data_ptr(), B, ins[2].data_ptr(), ins[3].data_ptr(), None if kd is None else kd.data_ptr(), None,
                              ins[4].data_ptr(), *(raw[k].data_ptr() + pad for k, _, _ in spec(V, B)), None)
    assert rc == 0, T._lib().vmask_last_error()
    for k, dt, n in spec(V, B):
        got = raw[k].cpu().numpy()
        nb = n * np.dtype(dt).itemsize
        assert (got[:pad] == TT.CANARY).all() and (got[pad + nb:] == TT.CANARY).all(), (shp, pad, k)
        ref = np.asarray(getattr(want, k)) if k in TT.KEYS else (np.array([want.missed]) if k == 'missed' else np.array([want.counts[c] for c in T.COUNT_NAMES]))
        assert got[pad:pad + nb].tobytes() == np.ascontiguousarray(ref, dt).tobytes(), (shp, pad, k)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_tubes_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call; the C-ABI
    with device pointers writes inside its outputs only.  Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


# ------------------------------------------------------------------ GPU: the real chain
def _phantom_mask():
    I, _ = P.tube_phantom(shape=(48, 40, 24), radius=3.0, noise=0.0, amp_y=8.0, amp_z=4.0)
    return (I > 0.5).astype(np.uint8)


@pytest.mark.gpu
def test_invariants_through_the_real_chain():
    """skeleton -> branchGraph -> morphometry -> splines -> graphTubes on the tube phantom.  The Dice and the precision are printed,
    not asserted: the EDT radius at a centre voxel overestimates a digitised cylinder."""
    from arterynetwork_amd import skeletonization as S
    m = _phantom_mask()
    graph = S.branchGraph(S.skeletonize(m), minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=m)
    B = len(graph.offsets) - 1
    assert B >= 1
    for h in ((1.0, 1.0, 1.0), (0.4, 0.4, 0.4)):
        measured = S.branchMorphometry(graph, vesselVolumeMask=m, spacing=h)
        splines = S.branchSplines(graph, spacing=h)
        for name, kw in (('voxel centres', {}), ('splines', dict(splines=splines)), ('dropped', dict(keep=np.arange(B) % 2 == 0))):
            model = T.graphTubes(graph, measured, mask=m, return_nearest=True, **kw)
            sizes, overlap, label = model.sizes, model.overlap, model.label
            assert sizes.sum() == np.count_nonzero(label) and (overlap <= sizes).all() and model.missed + overlap.sum() == m.sum()
            assert np.array_equal(np.bincount(label.ravel(), minlength=B + 1)[1:], sizes)
            a = T.agreement(model)
            print('{:14s} spacing {} Dice {:.4f} recall {:.4f} precision {}'.format(name, h[0], a['dice'], a['recall'], np.round(a['precision'], 4).tolist()))
            if 'splines' not in kw:
                # voxel-centre positions and positive radii: at a centre voxel of a kept branch some primitive has f = -r^2 <= 0
                keep = np.ones(B, bool) if 'keep' not in kw else kw['keep']
                owner = np.repeat(np.arange(B), np.diff(graph.offsets))
                on = graph.coords[keep[owner]]
                assert len(on) and (label[tuple(on.T)] != 0).all()
                assert (np.asarray(measured.entryRadius) > 0).all()
            assert model.minRadius == 0.5 * S.splineScale(h)[1] and model.splinePositions == ('splines' in kw)
    with pytest.raises(ValueError):
        T.graphTubes(graph, measured, minRadius=-1.0)


@pytest.mark.gpu
def test_main_writes_the_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    from arterynetwork_amd import skeletonization as S
    m = _phantom_mask()
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.4, 7.5], [0, 0, 0, 1.0]])
    plain, drawn, flowing = tmp_path / 'plain', tmp_path / 'drawn', tmp_path / 'flowing'
    for d in (plain, drawn, flowing):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    kw = dict(segments=True, prune=(3, 1.0), morphometry=True, curvature=True)
    before = S.main(str(plain), **kw)
    capsys.readouterr()
    after = S.main(str(drawn), tubes=True, **kw)
    said = capsys.readouterr().out
    new = [T.MODEL_FILE, T.MODEL_LABEL_FILE, T.MODEL_TABLE_FILE]
    assert sorted(os.listdir(str(drawn))) == sorted(os.listdir(str(plain)) + new)
    assert all('{} saved to {}.'.format(n, os.path.join(str(drawn), n)) in said for n in new)
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
    for name in os.listdir(str(plain)):
        assert TC._content(plain / name) == TC._content(drawn / name), name       # (without the containers' time stamps)
    graph = S.branchGraph(S.skeletonize(m), minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=m)
    _, stored = nifti.loadVolume(str(drawn), 'vesselVolumeMask.nii.gz')
    spacing = np.sqrt((np.asarray(stored, np.float64)[:3, :3] ** 2).sum(axis=0))
    measured = S.branchMorphometry(graph, vesselVolumeMask=m, spacing=spacing)
    want = T.graphTubes(graph, measured, splines=S.branchSplines(graph, spacing=spacing), mask=m)
    vol, _ = nifti.loadVolume(str(drawn), T.MODEL_FILE)
    lab, _ = nifti.loadVolume(str(drawn), T.MODEL_LABEL_FILE)
    assert vol.dtype == np.uint8 and lab.dtype == np.int32 and np.array_equal(lab, want.label) and np.array_equal(vol, want.label != 0)
    z = np.load(str(drawn / T.MODEL_TABLE_FILE))
    assert np.array_equal(z['sizes'], want.sizes) and np.array_equal(z['overlap'], want.overlap) and int(z['missed']) == want.missed
    assert np.array_equal(z['volumes'], T.modelVolumes(want.sizes, spacing)) and np.array_equal(z['cylinderVolumes'], T.cylinderVolumes(measured.pathLength, measured.meanRadius))
    assert z['counts'].tolist() == [want.counts[k] for k in T.COUNT_NAMES] and bool(z['splinePositions']) and float(z['dice']) == T.agreement(want)['dice']
    # with a flow: |flow| of the branch that holds the voxel
    ends = np.flatnonzero(np.asarray(graph.nodeKind) == 0)
    assert len(ends) >= 2
    flow = dict(pressureIn=13000.0, slope=-100.0, c=130.0)
    S.main(str(flowing), tubes=dict(radiusScale=0.8, minRadius=0.3), roots=[int(ends[0])], flow=flow, **kw)
    assert T.FLOW_VOLUME_FILE in os.listdir(str(flowing))
    painted, _ = nifti.loadVolume(str(flowing), T.FLOW_VOLUME_FILE)
    lab, _ = nifti.loadVolume(str(flowing), T.MODEL_LABEL_FILE)
    solved = np.load(str(flowing / 'flowResult.npz'))
    assert painted.dtype == np.float32 and np.array_equal(painted, T.paintBranches(lab, np.abs(solved['flow'][0]).astype(np.float32)))
    z = np.load(str(flowing / T.MODEL_TABLE_FILE))
    assert float(z['radiusScale']) == 0.8 and float(z['minRadius']) == 0.3
