"""Geodesic distance and territories inside the mask ("f9 geodesic"): the Dijkstra model
tests/geodesic_model.py is checked on the CPU (against scipy's Dijkstra, against a numpy Jacobi fixed point, by hand), then
vmask_geodesic / geodesic.geodesicDistance / skeletonization.geodesicTerritories must equal it exactly: the bits of dist, labels,
sizes and the counts of mask and reached voxels."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import geodesic_model as GM
import territory_model as TM
from conftest import ROOT
from arterynetwork_amd import geodesic as G
from arterynetwork_amd import phantoms
from arterynetwork_amd import skeletonization as S


# ------------------------------------------------------------------ inputs
def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _lin(shape, points):
    return np.ravel_multi_index(np.asarray(points, np.int64).reshape(-1, 3).T, shape).astype(np.int64)


def _corner_and_face_seeds(mask):
    """Mask voxels on the volume's corners and on the faces of the 8x8x8 bricks (coordinates 7 and 8), labels 1..3 in turn."""
    shape = mask.shape
    axes = [sorted({0, n - 1} | {c for c in (7, 8, 15, 16) if c < n}) for n in shape]
    pts = [(a, b, c) for a in axes[0] for b in axes[1] for c in axes[2] if mask[a, b, c]][::3]
    if not pts and mask.any():
        pts = [tuple(np.argwhere(mask)[0])]
    seeds = _lin(shape, pts) if pts else np.zeros(0, np.int64)
    return seeds, (1 + np.arange(len(seeds)) % 3).astype(np.int32)


def _serpentine(shape, width):
    """A one-voxel-wide corridor: runs along axis 2 over [0, width), every second row, joined at alternating ends; every second
    plane, joined where the plane's last run ends.  26-adjacency adds nothing but the corners' diagonals."""
    n0, n1, _ = shape
    m = np.zeros(shape, np.uint8)
    end = 0                                                            # the i2 where the next run starts
    for a in range(0, n0, 2):
        rows = list(range(0, n1, 2)) if (a // 2) % 2 == 0 else list(range(0, n1, 2))[::-1]
        for k, b in enumerate(rows):
            m[a, b, :width] = 1
            end = width - 1 - end
            if k + 1 < len(rows):
                m[a, (b + rows[k + 1]) // 2, end] = 1
        if a + 2 < n0:
            m[a + 1, rows[-1], end] = 1
    return m


def _line(axis, n):
    shape = [1, 1, 1]
    shape[axis] = n
    return np.ones(shape, np.uint8)


def _trunk_and_thin_vessel():
    """A trunk of radius 6.2 and a vessel of radius 1.2 beside it along axis 2, an empty plane between them; the centre lines."""
    shape = (24, 24, 40)
    z, y = np.indices(shape[:2])
    A = ((z - 8) ** 2 + (y - 12) ** 2 <= 6.2 ** 2)[:, :, None].repeat(40, axis=2)
    B = ((z - 17) ** 2 + (y - 12) ** 2 <= 1.2 ** 2)[:, :, None].repeat(40, axis=2)
    assert not (A | B)[15].any()
    vox = np.concatenate([_lin(shape, [(8, 12, x) for x in range(40)]), _lin(shape, [(17, 12, x) for x in range(40)])])
    return (A | B).astype(np.uint8), A, vox, np.asarray([0, 40, 80], np.int64)


@functools.lru_cache(maxsize=None)
def _model(key):
    """The model's (dist, labels, sizes) of a named case, computed once and shared (read-only)."""
    mask, seeds, labels, spacing = CASES[key]()
    out = GM.geodesic(mask, seeds, labels, spacing)
    for a in out:
        a.setflags(write=False)
    return (mask, seeds, labels, spacing) + out


def _assert_model(key, got=None, info=None):
    mask, seeds, labels, spacing, m_dist, m_labels, m_sizes = _model(key)
    if got is None:
        info = {}
        got = G.geodesicDistance(mask, seeds, labels, spacing=spacing, info=info, return_labels=True)
    dist, lab, sizes = got
    assert dist.dtype == np.float64 and lab.dtype == np.int32 and sizes.dtype == np.int64
    assert dist.shape == mask.shape and lab.shape == mask.shape and sizes.shape == m_sizes.shape
    wrong = np.flatnonzero(dist.ravel().view(np.int64) != m_dist.ravel().view(np.int64))
    assert wrong.size == 0, 'dist differs at {} voxels, first {}: {!r} for {!r}'.format(
        wrong.size, np.unravel_index(wrong[0], mask.shape), dist.ravel()[wrong[0]], m_dist.ravel()[wrong[0]])
    wrong = np.flatnonzero(lab.ravel() != m_labels.ravel())
    assert wrong.size == 0, 'labels differ at {} voxels, first {}: {} for {}'.format(
        wrong.size, np.unravel_index(wrong[0], mask.shape), lab.ravel()[wrong[0]], m_labels.ravel()[wrong[0]])
    assert np.array_equal(sizes, m_sizes) and int(sizes.sum()) == int(np.count_nonzero(mask))
    if info is not None:
        assert info['mask_voxels'] == int(np.count_nonzero(mask)) and info['reached'] == int(np.isfinite(m_dist[mask != 0]).sum())
        assert info['bricks'] == len({(a // 8, b // 8, c // 8) for a, b, c in np.argwhere(mask).tolist()})
    return dist, lab, sizes


CASES = {}
EXTENTS = [(7, 9, 17), (8, 8, 8), (9, 16, 23), (1, 40, 40), (40, 1, 33), (33, 40, 1)]
KINDS = {'full': None, 'd35': 0.35, 'd60': 0.6}


def _extent_case(shape, kind, spacing=None):
    mask = np.ones(shape, np.uint8) if KINDS[kind] is None else _random(shape, KINDS[kind], 200 + EXTENTS.index(shape))
    return (mask,) + _corner_and_face_seeds(mask) + (spacing,)


for _shape in EXTENTS:
    for _kind in KINDS:
        CASES['extent-%dx%dx%d-%s' % (_shape + (_kind,))] = functools.partial(_extent_case, _shape, _kind)
CASES['spacing-1-1-2.5'] = functools.partial(_extent_case, (9, 16, 23), 'd60', (1.0, 1.0, 2.5))
CASES['spacing-.5-.5-.8'] = functools.partial(_extent_case, (7, 9, 17), 'd35', (0.5, 0.5, 0.8))
# many rounds (the corridor crosses brick faces hundreds of times); inside one column of bricks the corridor stays longer in a
# brick than the inner sweeps reach in one round, so the brick flags itself
CASES['serpentine-24'] = lambda: (_serpentine((24, 24, 24), 24), _lin((24, 24, 24), [(0, 0, 0)]), None, None)
CASES['serpentine-8-wide'] = lambda: (_serpentine((24, 24, 24), 8), _lin((24, 24, 24), [(0, 0, 0)]), None, None)
for _axis in range(3):
    CASES['line-axis%d-end' % _axis] = functools.partial(lambda ax: (_line(ax, 6000), np.zeros(1, np.int64), None, None), _axis)
    CASES['line-axis%d-middle' % _axis] = functools.partial(lambda ax: (_line(ax, 6000), np.asarray([3000], np.int64), None, None), _axis)


def _mirror_case(axis):
    a, b = [4, 4, 4], [4, 4, 4]
    a[axis], b[axis] = 1, 7
    return np.ones((9, 9, 9), np.uint8), _lin((9, 9, 9), [a, b]), np.asarray([2, 1], np.int32), None


for _axis in range(3):
    CASES['mirror-axis%d' % _axis] = functools.partial(_mirror_case, _axis)
CASES['duplicate-seed'] = lambda: (np.ones((5, 9, 10), np.uint8), _lin((5, 9, 10), [(2, 2, 2), (3, 8, 9), (2, 2, 2), (2, 2, 2)]),
                                   np.asarray([5, 3, 2, 4], np.int32), None)
CASES['labels-none'] = lambda: (_random((9, 16, 23), 0.6, 77), _corner_and_face_seeds(_random((9, 16, 23), 0.6, 77))[0], None, None)
CASES['no-seed'] = lambda: (_random((9, 10, 11), 0.5, 78), np.zeros(0, np.int64), None, None)


# the spacing ratio at its limit, and spacings that are no representable sums: ties of fl(D + w) decide the labels
CASES['spacing-1-1000-1'] = functools.partial(_extent_case, (7, 9, 17), 'd60', (1.0, 1000.0, 1.0))
CASES['spacing-.1-.3-.7'] = functools.partial(_extent_case, (9, 16, 23), 'd60', (0.1, 0.3, 0.7))


def _trunk_case():
    mask, _, vox, _ = _trunk_and_thin_vessel()
    return mask, vox, np.repeat(np.asarray([1, 2], np.int32), 40), None


CASES['trunk-and-thin-vessel'] = _trunk_case


# ------------------------------------------------------------------ CPU: the model itself, and what needs no GPU
SMALL = [((7, 9, 11), 0.6, 1, None), ((6, 12, 5), 0.2, 2, (1.0, 1.0, 2.5)), ((10, 4, 9), 0.15, 3, (0.5, 0.5, 0.8))]


def _small(shape, density, seed):
    mask = _random(shape, density, seed)
    return mask, np.flatnonzero(mask.ravel())[::17].astype(np.int64)


@pytest.mark.parametrize('shape,density,seed,spacing', SMALL)
def test_model_equals_scipy_dijkstra(shape, density, seed, spacing):
    sp = pytest.importorskip('scipy.sparse')
    from scipy.sparse.csgraph import dijkstra
    mask, seeds = _small(shape, density, seed)
    idx = np.flatnonzero(mask.ravel())
    number = np.full(mask.size, -1, np.int64)
    number[idx] = np.arange(len(idx))
    pos = np.argwhere(mask)
    rows, cols, vals = [], [], []
    for off, w in zip(GM.OFFSETS, GM.weights(spacing)):
        q = pos + off
        ok = ((q >= 0) & (q < shape)).all(axis=1)
        ok[ok] = mask[tuple(q[ok].T)] != 0
        rows.append(number[idx[ok]]); cols.append(number[np.ravel_multi_index(q[ok].T, shape)]); vals.append(np.full(int(ok.sum()), w))
    graph = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(idx), len(idx)))
    want = dijkstra(graph, directed=True, indices=number[seeds], min_only=True)
    dist, labels, sizes = GM.geodesic(mask, seeds, spacing=spacing)
    assert np.array_equal(dist.ravel()[idx], want)
    assert (dist[mask == 0] == -1).all() and sizes.tolist() == [int(np.isinf(want).sum()), int(np.isfinite(want).sum())]


@pytest.mark.parametrize('shape,density,seed,spacing', SMALL)
def test_model_equals_jacobi_fixed_point(shape, density, seed, spacing):
    mask, seeds = _small(shape, density, seed)
    dist = GM.geodesic(mask, seeds, spacing=spacing)[0]
    assert dist.tobytes() == GM.jacobi(mask, seeds, spacing).tobytes()


def test_model_by_hand():
    # an open box, one seed: along an axis D = k h, with 26 neighbours the distance to (a, b, c) sorted a >= b >= c is
    # (a - b) h + (b - c) sqrt(2) h + c sqrt(3) h for h = 1
    mask = np.ones((6, 7, 8), np.uint8)
    dist, labels, sizes = GM.geodesic(mask, _lin(mask.shape, [(0, 0, 0)]), spacing=(1.5, 0.25, 2.0))
    assert dist[:, 0, 0].tolist() == [1.5 * k for k in range(6)] and dist[0, :, 0].tolist() == [0.25 * k for k in range(7)]
    assert dist[0, 0, :].tolist() == [2.0 * k for k in range(8)] and (labels == 1).all() and sizes.tolist() == [0, mask.size]
    dist = GM.geodesic(mask, _lin(mask.shape, [(0, 0, 0)]))[0]
    assert dist[1, 1, 1] == math.sqrt(3.0) and dist[0, 1, 1] == math.sqrt(2.0) and abs(dist[5, 2, 0] - (3 + 2 * math.sqrt(2.0))) < 1e-14
    # two seeds mirrored about a plane, labels 2 and 1: the mid-plane gets 1, each side its own
    for key in ('mirror-axis0', 'mirror-axis1', 'mirror-axis2'):
        mask, seeds, lab, _, dist, labels, sizes = _model(key)
        axis = int(key[-1])
        mid = np.take(labels, 4, axis=axis)
        assert (mid == 1).all() and (np.take(labels, 3, axis=axis) == 2).all() and (np.take(labels, 5, axis=axis) == 1).all()
        assert sizes.tolist() == [0, 5 * 81, 4 * 81]
    # a duplicate seed with several labels: the smallest
    mask, seeds, lab, _, dist, labels, sizes = _model('duplicate-seed')
    assert labels[2, 2, 2] == 2 and labels[3, 8, 9] == 3 and dist[2, 2, 2] == 0 and sizes[4] == sizes[5] == 0 and sizes[2] > sizes[3] > 0
    # unreachable components, no seed at all
    mask, seeds, lab, _, dist, labels, sizes = _model('no-seed')
    assert np.isinf(dist[mask != 0]).all() and (dist[mask == 0] == -1).all() and not labels.any() and sizes.tolist() == [int(mask.sum()), 0]
    m = np.zeros((3, 3, 7), np.uint8); m[1, 1, :3] = 1; m[1, 1, 4:] = 1
    dist, labels, sizes = GM.geodesic(m, _lin(m.shape, [(1, 1, 0)]), [4])
    assert dist[1, 1].tolist() == [0, 1, 2, -1, np.inf, np.inf, np.inf] and labels[1, 1].tolist() == [4, 4, 4, 0, 0, 0, 0] and sizes.tolist() == [3, 0, 0, 0, 3]


def test_model_trunk_keeps_its_rim():
    """What the feature exists for: Euclidean nearness gives 400 of the trunk's voxels to the thin vessel, geodesic nearness none."""
    mask, A, vox, off = _trunk_and_thin_vessel()
    sk = np.zeros(mask.shape, np.uint8)
    sk.ravel()[vox] = 1
    euclid = TM.territories(mask, sk, off, vox)[0]
    assert int((euclid[A] == 2).sum()) == 400
    labels = _model('trunk-and-thin-vessel')[5]
    assert not (labels[A] == 2).any() and (labels[A] == 1).all() and (labels[(mask != 0) & ~A] == 2).all()


def test_cases_stay_small():
    for key in CASES:
        assert np.count_nonzero(CASES[key]()[0]) <= 20000, key
    for key, least in (('serpentine-24', 3000), ('serpentine-8-wide', 1000)):     # corridors: every voxel has at most two neighbours but at the corners
        m = CASES[key]()[0]
        dist = _model(key)[4]
        assert np.count_nonzero(m) >= least and np.isfinite(dist[m != 0]).all() and dist.max() > 0.75 * np.count_nonzero(m)


def test_python_argument_checks():
    mask = np.ones((4, 5, 6), np.uint8)
    for bad in (lambda: G.geodesicDistance(np.ones((4, 5), np.uint8), [0]),                       # not a volume
                lambda: G.geodesicDistance(mask, np.zeros((2, 2), np.int64)),                      # neither N x 3 nor N
                lambda: G.geodesicDistance(mask, [[0, 0, 6]]),                                     # a coordinate outside the volume
                lambda: G.geodesicDistance(mask, [[0, -1, 0]]),
                lambda: G.geodesicDistance(mask, [0.5]),                                           # not integers
                lambda: G.geodesicDistance(mask, [0, 1], labels=[1]),                              # one label per seed
                lambda: G.geodesicDistance(mask, [0], labels=[1.5]),
                lambda: G.geodesicDistance(mask, [0], spacing=(1, 1)),
                lambda: S.geodesicTerritories(mask, np.ones((4, 5, 7), np.uint8)),
                lambda: S.geodesicTerritories(mask, mask, offsets=np.zeros(1, np.int64))):
        with pytest.raises(ValueError):
            bad()
    import arterynetwork_amd
    assert arterynetwork_amd.geodesicDistance is G.geodesicDistance and arterynetwork_amd.geodesicTerritories is S.geodesicTerritories


def test_main_geodesic_argument_check(tmp_path):
    with pytest.raises(ValueError):
        S.main(str(tmp_path), segments=True, geodesic=True)
    with pytest.raises(ValueError):
        S.main(str(tmp_path), geodesic=True)
    assert os.listdir(str(tmp_path)) == []


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
VGPR_BUDGET = 32                                                        # the first build reports 28 (k_geo_relax<0>), the other kernels 10-24


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_geodesic_kernels_use_no_scratch_and_few_registers(tmp_path):
    from arterynetwork_amd import build
    assert 'vgeo_device.hip' in build.SOURCES
    out = tmp_path / 'vgeo_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vgeo_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1)),
                            int(re.search(r'\.vgpr_count:\s+(\d+)', m.group(2)).group(1)))
    for frag in ('k_geo_mark', 'k_brick_slots', 'k_geo_init', 'k_geo_check', 'k_geo_seed', 'k_brick_list', 'k_geo_relaxILi0E', 'k_geo_relaxILi1E',
                 'k_geo_scatter'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, (scratch, vgprs) in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)
        assert vgprs <= VGPR_BUDGET, '%s uses %d VGPRs' % (name, vgprs)


# ------------------------------------------------------------------ GPU: exactly the model
@pytest.mark.gpu
@pytest.mark.parametrize('kind', sorted(KINDS))
@pytest.mark.parametrize('shape', EXTENTS)
def test_geodesic_brick_edges_and_extents_of_one(shape, kind):
    key = 'extent-%dx%dx%d-%s' % (shape + (kind,))
    dist, labels, sizes = _assert_model(key)
    assert int(sizes[0]) == int(np.isinf(dist).sum()) and (kind != 'full' or sizes[0] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['serpentine-24', 'serpentine-8-wide'] + ['line-axis%d-%s' % (a, w) for a in range(3) for w in ('end', 'middle')])
def test_geodesic_long_dependencies(key):
    info = {}
    mask, seeds, labels, spacing = _model(key)[:4]
    got = G.geodesicDistance(mask, seeds, labels, spacing=spacing, info=info, return_labels=True)
    dist = _assert_model(key, got, info)[0]
    if key.startswith('line'):
        assert dist.max() == (5999.0 if key.endswith('end') else 3000.0) and info['distance_rounds'] >= 375
        assert info['label_rounds'] >= 375                              # one label, carried a brick further per round
    else:
        assert info['distance_rounds'] >= (100 if key == 'serpentine-24' else 20)
        assert info['label_rounds'] >= (100 if key == 'serpentine-24' else 20)


@pytest.mark.gpu
def test_geodesic_trunk_keeps_its_rim():
    mask, A, vox, off = _trunk_and_thin_vessel()
    dist, labels, sizes = _assert_model('trunk-and-thin-vessel')
    assert not (labels[A] == 2).any()
    sk = np.zeros(mask.shape, np.uint8)
    sk.ravel()[vox] = 1
    coords = np.stack(np.unravel_index(vox, mask.shape), axis=1)
    euclid = S.branchTerritories(mask, sk, off, coords)[0]
    assert int((euclid[A] == 2).sum()) == 400
    labels2, sizes2, dist2 = S.geodesicTerritories(mask, sk, off, coords, return_distance=True)   # the same seeds through the segments
    assert np.array_equal(labels2, labels) and np.array_equal(sizes2, sizes) and dist2.tobytes() == dist.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['mirror-axis0', 'mirror-axis1', 'mirror-axis2', 'duplicate-seed', 'labels-none', 'no-seed'])
def test_geodesic_ties_and_labels(key):
    dist, labels, sizes = _assert_model(key)
    mask = _model(key)[0]
    if key.startswith('mirror'):
        assert (np.take(labels, 4, axis=int(key[-1])) == 1).all()
    if key == 'duplicate-seed':
        assert labels[2, 2, 2] == 2
    if key == 'labels-none':
        assert set(np.unique(labels).tolist()) == {0, 1} and sizes.shape == (2,)
    if key == 'no-seed':
        assert np.isinf(dist[mask != 0]).all() and not labels.any() and sizes.tolist() == [int(mask.sum()), 0]
        for seeds in (np.zeros((0, 3), np.int64), []):
            assert G.geodesicDistance(mask, seeds).tobytes() == dist.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['spacing-1-1-2.5', 'spacing-.5-.5-.8', 'spacing-1-1000-1', 'spacing-.1-.3-.7'])
def test_geodesic_spacing(key):
    _assert_model(key)
    mask, seeds, labels, spacing = _model(key)[:4]
    coords = np.stack(np.unravel_index(seeds, mask.shape), axis=1)      # coordinates in place of linear indices, distances only
    assert G.geodesicDistance(mask, coords, labels, spacing=spacing).tobytes() == _model(key)[4].tobytes()


@pytest.mark.gpu
def test_geodesic_bad_arguments_leave_the_outputs_alone():
    """A seed outside the mask or the volume, a label outside 1..max_label, a spacing ratio of 2000: VRG_E_ARG, nothing written."""
    dll = G._lib()
    shape = (9, 10, 11)
    mask = _random(shape, 0.5, 9)
    good = np.flatnonzero(mask.ravel())[::50].astype(np.int64)
    labels = (1 + np.arange(len(good)) % 4).astype(np.int32)
    one = np.ones(3)
    CANARY = -77

    def call(seeds, lab, spacing, max_label=4, shape=shape):
        out = np.full(shape, float(CANARY)), np.full(shape, CANARY, np.int32), np.full(max_label + 1, CANARY, np.int64), np.full(5, CANARY, np.int64)
        rc = dll.vmask_geodesic(0, mask.ctypes.data, *shape, seeds.ctypes.data, lab.ctypes.data if lab is not None else None, len(seeds),
                                spacing.ctypes.data if spacing is not None else None, out[0].ctypes.data, out[1].ctypes.data,
                                out[2].ctypes.data, max_label, out[3].ctypes.data)
        return rc, out

    def swapped(value, a=None):
        a = (good if a is None else a).copy()
        a[len(a) // 2] = value
        return a

    for seeds, lab, spacing, text in ((swapped(int(np.flatnonzero(mask.ravel() == 0)[3])), labels, one, b'seeds'),
                                      (swapped(mask.size), labels, one, b'seeds'), (swapped(-1), labels, None, b'seeds'),
                                      (good, swapped(0, labels), one, b'seeds'), (good, swapped(5, labels), one, b'seeds'),
                                      (good, labels, np.asarray([1.0, 2000.0, 1.0]), b'spacing'), (good, labels, np.asarray([1.0, 0.0, 1.0]), b'spacing'),
                                      (good, labels, np.asarray([1.0, np.inf, 1.0]), b'spacing'), (good, labels, np.asarray([1.0, np.nan, 1.0]), b'spacing')):
        rc, out = call(seeds, lab, spacing)
        assert rc == -1 and text in dll.vmask_last_error()
        assert all((a == CANARY).all() for a in out)
    rc, out = call(good, None, one, max_label=0)                         # the default label 1 exceeds max_label 0
    assert rc == -1 and all((a == CANARY).all() for a in out)
    rc, out = call(good, labels, one, shape=(40000, 2, 2))
    assert rc == -1 and b'shape' in dll.vmask_last_error()
    rc, out = call(good, labels, one)
    want = GM.geodesic(mask, good, labels, max_label=4)
    assert rc == 0 and out[0].tobytes() == want[0].tobytes() and np.array_equal(out[1], want[1]) and np.array_equal(out[2], want[2])
    assert out[3][0] == mask.sum() and out[3][1] == np.isfinite(want[0][mask != 0]).sum() and out[3][3] >= 1 and out[3][4] >= 1
    # every output is optional
    dist = np.full(shape, float(CANARY))
    assert dll.vmask_geodesic(0, mask.ctypes.data, *shape, good.ctypes.data, labels.ctypes.data, len(good), None, dist.ctypes.data, None, None, 4, None) == 0
    assert dist.tobytes() == want[0].tobytes()
    sizes = np.full(5, CANARY, np.int64)
    assert dll.vmask_geodesic(0, mask.ctypes.data, *shape, good.ctypes.data, labels.ctypes.data, len(good), None, None, None, sizes.ctypes.data, 4, None) == 0
    assert np.array_equal(sizes, want[2])
    with pytest.raises(Exception) as e:
        G.geodesicDistance(mask, swapped(int(np.flatnonzero(mask.ravel() == 0)[3])))
    assert 'seeds' in str(e.value)


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import geodesic as G
from arterynetwork_amd import skeletonization as S
import geodesic_model as GM
rng = np.random.default_rng(21)
mask = (rng.random((20, 26, 31)) < 0.55).astype(np.uint8)
seeds = np.flatnonzero(mask.ravel())[::301].astype(np.int64)
labels = (1 + np.arange(len(seeds)) % 5).astype(np.int32)
sp = (0.5, 0.5, 0.8)
want = GM.geodesic(mask, seeds, labels, sp)
host = G.geodesicDistance(mask, seeds, labels, spacing=sp, return_labels=True)
again = G.geodesicDistance(mask, seeds, labels, spacing=sp, return_labels=True)
assert all(a.tobytes() == b.tobytes() == c.tobytes() for a, b, c in zip(host, again, want))
dev = torch.device('cuda', 0)
tm = torch.as_tensor(mask * 255, device=dev)
info = {{}}
for s, l in ((torch.as_tensor(seeds, device=dev), torch.as_tensor(labels, device=dev)), (seeds, labels)):
    d, lab, siz = G.geodesicDistance(tm, s, l, spacing=sp, return_labels=True, info=info)
    assert d.is_cuda and lab.is_cuda and siz.is_cuda and d.device == dev
    assert d.dtype == torch.float64 and lab.dtype == torch.int32 and siz.dtype == torch.int64 and tuple(d.shape) == mask.shape
    assert d.cpu().numpy().tobytes() == want[0].tobytes() and lab.cpu().numpy().tobytes() == want[1].tobytes()
    assert siz.cpu().numpy().tobytes() == want[2].tobytes() and info['mask_voxels'] == mask.sum()
only = G.geodesicDistance(tm, torch.as_tensor(np.stack(np.unravel_index(seeds, mask.shape), axis=1), device=dev), spacing=sp)
assert only.is_cuda and only.cpu().numpy().tobytes() == want[0].tobytes()
# territories with device volumes
sk = np.zeros_like(mask); sk[3:17, 13, 15] = 1; sk[10, 2:20, 7] = 1
off, co = S.segmentArrays(sk)
lab_h, siz_h, d_h = S.geodesicTerritories(mask, sk, off, co, spacing=sp, return_distance=True)
lab_d, siz_d, d_d = S.geodesicTerritories(tm, torch.as_tensor(sk, device=dev), spacing=sp, return_distance=True)
assert lab_d.is_cuda and lab_d.cpu().numpy().tobytes() == lab_h.tobytes() and siz_d.cpu().numpy().tobytes() == siz_h.tobytes()
assert d_d.cpu().numpy().tobytes() == d_h.tobytes() and siz_h.sum() == mask.sum() and len(siz_h) == len(off)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_geodesic_device_resident_and_repeatable():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, bit-identical to the host
    call and to a second run.  Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


def _lattice_mask():
    """Four disjoint wiggling tubes (phantoms.tube_lattice) in a 40 x 40 x 48 volume, about 10^4 voxels."""
    nx, ny, nz = 48, 40, 40
    cen, rad, amp = phantoms.tube_lattice((nx, ny, nz), 4)
    zs, ys, xs = np.indices((nz, ny, nx)).astype(np.float64)
    wy, wz = amp * np.sin(2 * math.pi * xs / nx * 3.0), amp * np.cos(2 * math.pi * xs / nx * 3.0)
    m = np.zeros((nz, ny, nx), bool)
    for c_y, c_z in cen:
        m |= (ys - (c_y + wy)) ** 2 + (zs - (c_z + wz)) ** 2 <= rad ** 2
    return m.astype(np.uint8)


def _site_seeds(mask, off, co):
    vox = _lin(mask.shape, co)
    lab = np.repeat(np.arange(1, len(off), dtype=np.int32), np.diff(off))
    keep = mask.ravel()[vox] != 0
    return vox[keep], lab[keep]


@pytest.mark.gpu
def test_geodesic_territories_end_to_end():
    mask = _lattice_mask()
    sk = S.skeletonize(mask)
    off, co = S.segmentArrays(sk)
    info = {}
    labels, sizes, dist = S.geodesicTerritories(mask, sk, info=info, return_distance=True)        # traces the segments itself
    seeds, lab = _site_seeds(mask, off, co)
    want = GM.geodesic(mask, seeds, lab, max_label=len(off) - 1)
    assert dist.tobytes() == want[0].tobytes() and np.array_equal(labels, want[1]) and np.array_equal(sizes, want[2])
    assert info['segments'] == len(off) - 1 >= 4 and int(sizes.sum()) == int(np.count_nonzero(mask)) == info['mask_voxels']
    assert labels.dtype == np.int32 and sizes.dtype == np.int64 and sizes.shape == (len(off),) and labels.shape == mask.shape
    two = S.geodesicTerritories(mask, sk, off, co)
    assert len(two) == 2 and np.array_equal(two[0], labels) and np.array_equal(two[1], sizes)


@pytest.mark.gpu
def test_geodesic_main_writes_three_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    m = _lattice_mask()
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, geo = tmp_path / 'plain', tmp_path / 'geo'
    for d in (plain, geo):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    # geodesic=False: what the function always wrote - the Euclidean territories, and no distance file
    sk0, segs0, labels0, sizes0 = S.main(str(plain), segments=True, territories=True, geodesic=False)
    names = ['graphRepresentation.graphml', 'segmentLabels.nii.gz', 'segmentList.npz', 'segmentTerritories.npz', 'skeleton.nii.gz', 'vesselVolumeMask.nii.gz']
    assert sorted(os.listdir(str(plain))) == names
    off, co = S.segmentArrays(sk0)
    euclid = TM.territories(m, sk0, off, _lin(m.shape, co))
    assert np.array_equal(labels0, euclid[0]) and np.array_equal(sizes0, euclid[2])
    assert np.array_equal(nifti.loadVolume(str(plain), 'segmentLabels.nii.gz')[0], euclid[0])
    assert np.array_equal(np.load(str(plain / 'segmentTerritories.npz'))['sizes'], euclid[2])
    capsys.readouterr()
    sk, segs, labels, sizes, dist = S.main(str(geo), segments=True, territories=True, geodesic=True)
    said = capsys.readouterr().out
    assert sorted(os.listdir(str(geo))) == sorted(names + ['centrelineDistance.nii.gz'])
    for name in ('segmentLabels.nii.gz', 'segmentTerritories.npz', 'centrelineDistance.nii.gz'):
        assert '{} saved to {}.'.format(name, os.path.join(str(geo), name)) in said
    assert np.array_equal(sk, sk0) and segs == segs0
    for name in ('skeleton.nii.gz', 'graphRepresentation.graphml'):
        if name.endswith('.graphml'):
            assert (geo / name).read_bytes() == (plain / name).read_bytes()
        else:
            assert np.array_equal(nifti.loadVolume(str(geo), name)[0], nifti.loadVolume(str(plain), name)[0])
    seeds, lab = _site_seeds(m, off, co)
    # the spacing is the norms of the columns of the affine AS THE FILE STORES IT (NIfTI keeps float32: 0.4 comes back as 0.40000001)
    spacing = np.sqrt((nifti.loadVolume(str(geo), 'vesselVolumeMask.nii.gz')[1][:3, :3].astype(np.float64) ** 2).sum(axis=0))
    assert np.allclose(spacing, (0.4, 0.4, 0.6), rtol=1e-7, atol=0)
    want = GM.geodesic(m, seeds, lab, spacing=spacing, max_label=len(off) - 1)
    assert dist.tobytes() == want[0].tobytes() and np.array_equal(labels, want[1]) and np.array_equal(sizes, want[2])
    stored, aff2 = nifti.loadVolume(str(geo), 'segmentLabels.nii.gz')
    assert stored.dtype == np.int32 and np.array_equal(stored, labels) and np.allclose(aff2, aff)
    z = np.load(str(geo / 'segmentTerritories.npz'))
    assert z['sizes'].dtype == np.int64 and z['volumes'].dtype == np.float64 and np.array_equal(z['sizes'], sizes)
    assert len(sizes) == len(segs) + 1 and sizes.sum() == np.count_nonzero(m) and np.allclose(z['volumes'], sizes * 0.4 * 0.4 * 0.6)
    d32, aff3 = nifti.loadVolume(str(geo), 'centrelineDistance.nii.gz')
    assert d32.dtype == np.float32 and np.allclose(aff3, aff) and np.array_equal(d32, dist.astype(np.float32))
    assert (d32[m == 0] == -1).all() and (d32[sk != 0] == 0).all()


# ------------------------------------------------------------------ the paths that the cases above never enter
BYTES = np.asarray([1, 2, 0x7f, 0x80, 0xff], np.uint8)


def _byte_mask(shape, seed):
    """A random mask whose non-zero voxels hold 1, 2, 0x7f, 0x80 or 0xff, one aligned 16-byte word of 0x80 only and one of 0x02
    only, beside words of zeros; the first and the last voxel are set."""
    rng = np.random.default_rng(seed)
    m = ((rng.random(shape) < 0.6) * BYTES[rng.integers(0, len(BYTES), shape)]).astype(np.uint8)
    flat = m.reshape(-1)
    flat[16:32], flat[32:48], flat[48:64], flat[64:80], flat[80:96] = 0, 0x80, 0, 0x02, 0
    flat[0], flat[-1] = 0x80, 0x02
    return m


def _abi(dll, mask_ptr, shape, seeds, labels, spacing, max_label):
    """vmask_geodesic through the C-ABI with host seeds and outputs: (rc, dist, labels, sizes, counts), canaries where nothing is written."""
    CANARY = -77
    out = np.full(shape, float(CANARY)), np.full(shape, CANARY, np.int32), np.full(max_label + 1, CANARY, np.int64), np.full(5, CANARY, np.int64)
    sp = None if spacing is None else np.asarray(spacing, np.float64)
    rc = dll.vmask_geodesic(0, mask_ptr, *shape, seeds.ctypes.data, labels.ctypes.data, len(seeds), sp.ctypes.data if sp is not None else None,
                            out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, max_label, out[3].ctypes.data)
    return (rc,) + out


def _bricks(mask):
    return len({(a // 8, b // 8, c // 8) for a, b, c in np.argwhere(mask).tolist()})


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(8, 8, 8), (7, 9, 17), (5, 9, 11)])
def test_geodesic_mask_byte_values(shape):
    """The mask is "!= 0": bytes such as 0x80, 0x7f and 0x02 count like 1 (the Python wrapper hands on 0 / 1 only, so this goes
    through the C-ABI)."""
    mask = _byte_mask(shape, 60)
    seeds, labels = _corner_and_face_seeds(mask)
    want = GM.geodesic(mask, seeds, labels, max_label=3)
    rc, dist, lab, sizes, counts = _abi(G._lib(), mask.ctypes.data, shape, seeds, labels, None, 3)
    assert rc == 0 and counts[0] == np.count_nonzero(mask) and counts[2] == _bricks(mask)
    assert dist.tobytes() == want[0].tobytes() and np.array_equal(lab, want[1]) and np.array_equal(sizes, want[2])
    assert counts[1] == np.isfinite(want[0][mask != 0]).sum()


UNALIGNED_SHAPES = [(8, 8, 8), (7, 9, 17), (9, 9, 17)]                   # V % 16 = 0, 15, 1


UNALIGNED_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import geodesic as G
import geodesic_model as GM
import test_geodesic as T         # the inputs of the test that started this process
dll = G._lib()
dev = torch.device('cuda', 0)
done = 0
for shape in T.UNALIGNED_SHAPES:
    V = int(np.prod(shape))
    mask = T._byte_mask(shape, 61)
    seeds, labels = T._corner_and_face_seeds(mask)
    want = GM.geodesic(mask, seeds, labels, max_label=3)
    for off in (1, 5, 15, 16):
        buf = torch.full((V + 64,), 0xa5, dtype=torch.uint8, device=dev)      # non-zero bytes in front of and behind the view
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + V]
        view.copy_(torch.as_tensor(mask.reshape(-1), device=dev))
        torch.cuda.synchronize(dev)
        assert view.data_ptr() % 16 == off % 16
        rc, dist, lab, sizes, counts = T._abi(dll, view.data_ptr(), shape, seeds, labels, None, 3)
        what = (shape, off)
        assert rc == 0, (what, dll.vmask_last_error())
        assert counts[0] == np.count_nonzero(mask) and counts[2] == T._bricks(mask), (what, counts.tolist())
        assert dist.tobytes() == want[0].tobytes() and np.array_equal(lab, want[1]) and np.array_equal(sizes, want[2]), what
        back = buf.cpu().numpy()
        assert (back[:off] == 0xa5).all() and (back[off + V:] == 0xa5).all() and np.array_equal(back[off:off + V], mask.reshape(-1))
        done += 1
assert done == 12
print('UNALIGNED OK')
"""


def test_unaligned_shapes_cover_the_tails():
    assert [int(np.prod(shape)) % 16 for shape in UNALIGNED_SHAPES] == [0, 15, 1]
    m = _byte_mask((7, 9, 17), 61).reshape(-1)
    assert set(np.unique(m).tolist()) == {0, 1, 2, 0x7f, 0x80, 0xff} and (m[32:48] == 0x80).all() and (m[64:80] == 2).all() and m[0] and m[-1]


@pytest.mark.gpu
def test_geodesic_unaligned_device_mask():
    """A device mask that starts 1, 5, 15 and 16 bytes behind a 16-byte boundary, non-zero bytes in front of it and behind it:
    k_geo_mark must mask the head of its first aligned word and the tail of its last one (the counts of mask voxels and bricks
    show a byte too many or too few), and every other kernel reads the mask by the byte.  Own process: torch first."""
    script = UNALIGNED_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'UNALIGNED OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


SEED_SHAPE = (64, 64, 80)                                              # 327 680 voxels: more than the 1024 x 256 threads of k_geo_check / k_geo_seed


def _many_seeds():
    V = int(np.prod(SEED_SHAPE))
    seeds = np.random.default_rng(70).permutation(V).astype(np.int64)
    labels = (1 + np.arange(V) % 7).astype(np.int32)
    return np.concatenate([seeds, seeds[1000:6000]]), np.concatenate([labels, np.ones(5000, np.int32)])      # 5000 duplicates, label 1


@pytest.mark.gpu
def test_geodesic_more_seeds_than_threads():
    mask = np.ones(SEED_SHAPE, np.uint8)
    seeds, labels = _many_seeds()
    assert len(seeds) > 262144 + 5000
    want = np.full(mask.size, 8, np.int32)
    np.minimum.at(want, seeds, labels)                                  # of several labels given for one voxel the smallest holds
    assert (want[seeds[-5000:]] == 1).all() and want.max() == 7
    info = {}
    dist, lab, sizes = G.geodesicDistance(mask, seeds, labels, info=info, return_labels=True)
    assert not dist.any() and dist.dtype == np.float64 and np.array_equal(lab.ravel(), want)
    assert np.array_equal(sizes, np.bincount(want, minlength=8)) and info['mask_voxels'] == info['reached'] == mask.size and info['bricks'] == 8 * 8 * 10
    # a bad seed, or a bad label, behind the first trip of the loop: refused, nothing written
    dll = G._lib()
    for at, seed, label in ((300000, mask.size, 1), (len(seeds) - 1, -1, 1), (290000, None, 8), (len(seeds) - 1, None, 0)):
        s, l = seeds.copy(), labels.copy()
        if seed is not None:
            s[at] = seed
        l[at] = label if seed is None else l[at]
        rc, *out = _abi(dll, mask.ctypes.data, SEED_SHAPE, s, l, None, 7)
        assert rc == -1 and b'1 seeds' in dll.vmask_last_error() and all((a == -77).all() for a in out)


@pytest.mark.gpu
def test_geodesic_spacing_ratio_limit():
    """A ratio of exactly 1000 is accepted (and equals the model: 'spacing-1-1000-1' above), the next representable ratios above
    it are refused with the outputs untouched."""
    mask, seeds, labels, _ = CASES['spacing-1-1000-1']()
    dll = G._lib()
    for spacing in ((1.0, 1000.0000001, 1.0), (1.0, 1.0, float(np.nextafter(1000.0, 2000.0))), (0.001, 1.0, 1.0000000001)):
        rc, *out = _abi(dll, mask.ctypes.data, mask.shape, seeds, labels, spacing, 3)
        assert rc == -1 and b'spacing' in dll.vmask_last_error() and all((a == -77).all() for a in out)
    for spacing in ((1.0, 1000.0, 1.0), (0.5, 500.0, 0.5)):
        want = GM.geodesic(mask, seeds, labels, spacing, max_label=3)
        rc, dist, lab, sizes, counts = _abi(dll, mask.ctypes.data, mask.shape, seeds, labels, spacing, 3)
        assert rc == 0 and dist.tobytes() == want[0].tobytes() and np.array_equal(lab, want[1]) and np.array_equal(sizes, want[2])
