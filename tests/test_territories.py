"""Branch territories ("f8 territories"): the brute-force model tests/territory_model.py is checked on the
CPU (its distances against scipy's EDT, its tie rule by hand), then vmask_territories / skeletonization.branchTerritories must
equal it exactly: labels, nearest and sizes."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import segment_model as SM
import skeleton_model as M
import territory_model as TM
from conftest import ROOT
from arterynetwork_amd import skeletonization as S


# ------------------------------------------------------------------ inputs
def _vol(shape, points=()):
    v = np.zeros(shape, np.uint8)
    for p in points:
        v[tuple(p)] = 1
    return v


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _lin(shape, points):
    return np.ravel_multi_index(np.asarray(points, np.int64).reshape(-1, 3).T, shape).astype(np.int64)


def _made_up_segments(skeleton, seed):
    """Segment arrays as the C-ABI accepts them (every entry a skeleton voxel, nothing more): the sites in random order, about
    a tenth left out (label 0), cut into runs of 1-6, every other run starting with a voxel of an earlier one (a shared node)."""
    rng = np.random.default_rng(seed)
    sites = rng.permutation(np.flatnonzero(np.asarray(skeleton).ravel())).astype(np.int64)
    sites = sites[:len(sites) - len(sites) // 10]
    off, vox = [0], []
    at = 0
    while at < len(sites):
        n = int(rng.integers(1, 7))
        if vox and len(off) % 2 == 0:
            vox.append(int(vox[int(rng.integers(0, len(vox)))]))
        vox.extend(sites[at:at + n].tolist())
        off.append(len(vox))
        at += n
    return np.asarray(off, np.int64), np.asarray(vox, np.int64)


def _one_segment(skeleton):
    vox = np.flatnonzero(np.asarray(skeleton).ravel()).astype(np.int64)
    return np.asarray([0, len(vox)], np.int64), vox


def _run(mask, skeleton, off, vox):
    coords = np.stack(np.unravel_index(vox, mask.shape), axis=1).astype(np.int64).reshape(-1, 3)
    return S.branchTerritories(mask, skeleton, off, coords, return_nearest=True)


def _assert_model(mask, skeleton, off, vox, want=None, got=None):
    labels, sizes, nearest = got if got is not None else _run(mask, skeleton, off, vox)
    m_labels, m_nearest, m_sizes = want if want is not None else TM.territories(mask, skeleton, off, vox)
    assert labels.dtype == np.int32 and nearest.dtype == np.int64 and sizes.dtype == np.int64
    assert labels.shape == mask.shape and nearest.shape == mask.shape and sizes.shape == (len(off),)
    wrong = np.flatnonzero(nearest.ravel() != m_nearest.ravel())
    assert wrong.size == 0, 'nearest differs at {} voxels, first {}: {} for {}'.format(
        wrong.size, np.unravel_index(wrong[0], mask.shape), nearest.ravel()[wrong[0]], m_nearest.ravel()[wrong[0]])
    assert np.array_equal(labels, m_labels) and np.array_equal(sizes, m_sizes)
    assert int(sizes.sum()) == int(np.count_nonzero(mask))
    return labels, sizes, nearest


# ------------------------------------------------------------------ CPU: the model itself, and what needs no GPU
@pytest.mark.parametrize('shape,density,seed', [((7, 9, 11), 0.02, 1), ((16, 16, 16), 0.001, 2), ((5, 24, 25), 0.3, 3), ((1, 40, 40), 0.02, 4)])
def test_model_distances_equal_scipy(shape, density, seed):
    ndi = pytest.importorskip('scipy.ndimage')
    sk = _random(shape, density, seed)
    sk[tuple(n // 2 for n in shape)] = 1                               # (at least one site)
    nearest, d2 = TM.nearest_sites(np.ones(shape, np.uint8), sk)
    edt = ndi.distance_transform_edt(sk == 0)
    assert np.array_equal(d2, np.rint(edt ** 2).astype(np.int64))
    assert sk.ravel()[nearest.ravel()].all()
    p, q = np.indices(shape).reshape(3, -1), np.asarray(np.unravel_index(nearest.ravel(), shape))
    assert np.array_equal(((p - q) ** 2).sum(axis=0), d2.ravel())


def test_model_tie_rule_and_labels():
    shape = (3, 3, 3)
    corners = [(a, b, c) for a in (0, 2) for b in (0, 2) for c in (0, 2)]
    sk = _vol(shape, corners)
    nearest, d2 = TM.nearest_sites(np.ones(shape, np.uint8), sk)
    assert nearest[1, 1, 1] == 0 and d2[1, 1, 1] == 3
    assert nearest[1, 0, 0] == 0 and nearest[1, 2, 2] == _lin(shape, [(0, 2, 2)])[0] and nearest[2, 1, 2] == _lin(shape, [(2, 0, 2)])[0]
    mask = np.ones(shape, np.uint8); mask[0, 0, 1] = 0
    # segment 0 = the last two corners, segment 1 = the first corner and a shared one, the other corners in no segment
    vox = _lin(shape, [corners[7], corners[6], corners[0], corners[7]])
    off = np.asarray([0, 2, 4], np.int64)
    L = TM.site_labels(shape, off, vox)
    assert L[2, 2, 2] == 1 and L[2, 2, 0] == 1 and L[0, 0, 0] == 2 and L[0, 0, 2] == 0 and L.sum() == 4
    labels, nearest, sizes = TM.territories(mask, sk, off, vox)
    assert labels[1, 1, 1] == 2 and labels[0, 0, 1] == 0 and nearest[0, 0, 1] == -1 and labels[2, 2, 1] == 1 and labels[0, 1, 2] == 0
    assert sizes.tolist() == [int((labels[mask != 0] == l).sum()) for l in range(3)] and sizes.sum() == 26
    none = TM.territories(mask, np.zeros(shape, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int64))
    assert not none[0].any() and (none[1] == -1).all() and none[2].tolist() == [26]


def test_territory_volumes():
    aff = np.array([[0.5, 0.1, 0, -10.0], [0, -0.4, 0.2, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])       # sheared, scaled, one axis flipped
    sizes = np.array([7, 0, 12, 1], np.int64)
    vol = S.territoryVolumes(sizes, aff)
    assert vol.dtype == np.float64 and vol.shape == (4,)
    assert np.allclose(vol, sizes * 0.5 * 0.4 * 0.6, rtol=1e-14, atol=0)
    assert np.allclose(S.territoryVolumes([3], np.eye(4)), [3.0])


def test_main_argument_check(tmp_path):
    with pytest.raises(ValueError):
        S.main(str(tmp_path), territories=True)
    with pytest.raises(ValueError):
        S.main(str(tmp_path), segments=False, territories=True)
    assert os.listdir(str(tmp_path)) == []
    import arterynetwork_amd
    assert arterynetwork_amd.branchTerritories is S.branchTerritories and arterynetwork_amd.territoryVolumes is S.territoryVolumes


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_territory_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vter_device.hip' in build.SOURCES
    out = tmp_path / 'vter_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vter_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1))
    for frag in ('k_ter_sites', 'k_ter_rows', 'k_ter_envelopeIiLi1E', 'k_ter_envelopeIxLi1E', 'k_ter_envelopeIiLi0E', 'k_ter_envelopeIxLi0E'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, scratch in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)


# ------------------------------------------------------------------ GPU: exactly the model
@pytest.mark.gpu
def test_territories_degenerate():
    one = np.ones((1, 1, 1), np.uint8)
    labels, sizes, nearest = _assert_model(one, one, *_one_segment(one))
    assert labels.item() == 1 and nearest.item() == 0 and sizes.tolist() == [0, 1]
    sk = _random((6, 7, 8), 0.1, 5)
    labels, sizes, nearest = _assert_model(np.zeros((6, 7, 8), np.uint8), sk, *_made_up_segments(sk, 5))        # empty mask
    assert not labels.any() and (nearest == -1).all() and not sizes.any()
    mask = _random((6, 7, 8), 0.5, 6)
    labels, sizes, nearest = _assert_model(mask, np.zeros_like(mask), np.zeros(1, np.int64), np.zeros(0, np.int64))   # no site
    assert not labels.any() and (nearest == -1).all() and sizes.tolist() == [int(mask.sum())]
    iso = _vol((6, 7, 8), [(1, 1, 1), (4, 5, 6), (2, 6, 0)])           # nseg == 0, isolated skeleton voxels only
    labels, sizes, nearest = _assert_model(mask, iso, np.zeros(1, np.int64), np.zeros(0, np.int64))
    assert not labels.any() and sizes.tolist() == [int(mask.sum())] and (nearest[mask != 0] >= 0).all()


def _tie_cases():
    cases = {}
    for axis in range(3):                                               # two sites mirrored about a mask voxel
        a, b = [4, 4, 4], [4, 4, 4]
        a[axis], b[axis] = 1, 7
        cases['mirror-axis%d' % axis] = ((9, 9, 9), [a, b])
    cases['corners-3x3x3'] = ((3, 3, 3), [(a, b, c) for a in (0, 2) for b in (0, 2) for c in (0, 2)])
    for axis in range(3):                                               # four sites on a square in each coordinate plane
        pts = []
        for p, q in ((1, 1), (1, 7), (7, 1), (7, 7)):
            x = [p, q]
            x.insert(axis, 4)
            pts.append(x)
        cases['square-plane%d' % axis] = ((9, 9, 9), pts)
    cases['row-and-column'] = ((5, 11, 11), [(2, 2, c) for c in range(11)] + [(2, b, 8) for b in range(11)] + [(0, 5, 5), (4, 5, 5)])
    return cases


TIES = _tie_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(TIES))
def test_territories_ties(case):
    shape, pts = TIES[case]
    sk = _vol(shape, pts)
    mask = np.ones(shape, np.uint8)
    off = np.arange(len(pts) + 1, dtype=np.int64)                       # every site its own segment, in raster order
    vox = np.sort(_lin(shape, pts))
    labels, sizes, nearest = _assert_model(mask, sk, off, vox)
    if case.startswith('mirror') or case.startswith('square'):
        assert nearest[4, 4, 4] == vox[0] and labels[4, 4, 4] == 1
    if case == 'corners-3x3x3':
        assert nearest[1, 1, 1] == 0 and labels[1, 1, 1] == 1
    if case == 'row-and-column':
        assert nearest[2, 5, 5] == _lin(shape, [(0, 5, 5)])[0] and nearest[2, 4, 6] == _lin(shape, [(2, 2, 6)])[0]


EXTENTS = [(7, 9, 11), (16, 16, 16), (5, 64, 65), (33, 1, 70), (1, 40, 40), (2, 3, 130), (6, 7, 1), (1, 1, 9), (9, 1, 1), (1, 9, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('full', [False, True])
@pytest.mark.parametrize('density', [0.001, 0.02, 0.3])
@pytest.mark.parametrize('shape', EXTENTS)
def test_territories_extents(shape, density, full):
    seed = 100 + EXTENTS.index(shape)
    sk = _random(shape, density, seed)
    mask = np.ones(shape, np.uint8) if full else _random(shape, 0.5, seed + 50)
    _assert_model(mask, sk, *_made_up_segments(sk, seed))


def _line_case(axis, n, every):
    shape = [1, 1, 1]
    shape[axis] = n
    sk = np.zeros(n, np.uint8)
    if every:
        sk[1::every] = 1
    sk[0] = sk[-1] = 1
    return sk.reshape(shape)


def _diagonal_case(lead):
    """Sites on the diagonal of a 300 x 300 square: the envelope of every line across it keeps hundreds of parabolas on its
    stack, far more than the ring in LDS holds, so the chunked spill area is written and read back."""
    shape = (1, 300, 300) if lead else (300, 300, 1)
    sk = np.zeros((300, 300), np.uint8)
    sk[np.arange(300), np.arange(300)] = 1
    return sk.reshape(shape)


LONG = {}
for _axis in range(3):
    LONG['line-axis%d-ends' % _axis] = functools.partial(_line_case, _axis, 6000, 0)
    LONG['line-axis%d-third' % _axis] = functools.partial(_line_case, _axis, 6000, 3)
    # 23200^2 >= 2^29: the envelope passes run their 64-bit arithmetic
    LONG['line-axis%d-wide' % _axis] = functools.partial(_line_case, _axis, 23200, 97)
LONG['diagonal-1x300x300'] = functools.partial(_diagonal_case, True)
LONG['diagonal-300x300x1'] = functools.partial(_diagonal_case, False)


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(LONG))
def test_territories_long_lines_and_deep_envelopes(case):
    sk = LONG[case]()
    _assert_model(np.ones(sk.shape, np.uint8), sk, *_made_up_segments(sk, 7))


@pytest.mark.gpu
def test_territories_roles():
    shape = (12, 14, 16)
    # a site outside the mask, and a mask component without a site of its own
    mask = np.zeros(shape, np.uint8)
    mask[2:6, 2:6, 2:6] = 1
    mask[8:11, 9:13, 10:15] = 1
    sk = _vol(shape, [(3, 3, 3), (4, 4, 4), (6, 7, 8)])
    mask[3, 3, 3] = 0
    off, vox = np.asarray([0, 2, 3], np.int64), _lin(shape, [(3, 3, 3), (4, 4, 4), (6, 7, 8)])
    labels, sizes, nearest = _assert_model(mask, sk, off, vox)
    assert labels[3, 3, 3] == 0 and nearest[3, 3, 3] == -1 and (labels[8:11, 9:13, 10:15] == 2).all() and sizes[2] >= 60
    # an isolated skeleton voxel inside a blob: the blob gets label 0
    mask = np.zeros(shape, np.uint8)
    mask[1:6, 1:6, 1:6] = 1
    mask[8:11, 8:12, 2:14] = 1
    sk = _vol(shape, [(3, 3, 3)] + [(9, 10, c) for c in range(3, 13)])
    off, vox = _one_segment(_vol(shape, [(9, 10, c) for c in range(3, 13)]))
    labels, sizes, nearest = _assert_model(mask, sk, off, vox)
    assert not labels[1:6, 1:6, 1:6].any() and (nearest[1:6, 1:6, 1:6] == _lin(shape, [(3, 3, 3)])[0]).all() and sizes.tolist() == [125, 144]
    # a Y whose centre node lies in three segments: it gets the smallest label
    y = np.zeros((9, 15, 15), np.uint8)
    for j in range(1, 6):
        y[4, 7 - j, 7] = y[4, 7 + j, 7 - j] = y[4, 7 + j, 7 + j] = 1
    y[4, 7, 7] = 1
    off, co, counts = SM.arrays(y)
    vox = _lin(y.shape, co)
    centre = _lin(y.shape, [(4, 7, 7)])[0]
    assert len(off) == 4 and sum(centre in vox[off[k]:off[k + 1]] for k in range(3)) == 3
    mask = np.zeros_like(y); mask[3:6] = 1
    labels, sizes, nearest = _assert_model(mask, y, off, vox)
    assert labels[4, 7, 7] == 1 and nearest[4, 7, 7] == centre and sorted(np.unique(labels).tolist()) == [0, 1, 2, 3]


@pytest.mark.gpu
def test_territories_bad_entry_is_an_argument_error():
    """A segment entry that is no skeleton voxel, or lies outside the volume: VRG_E_ARG, counted on the device, outputs untouched."""
    dll = S._skeleton_lib()
    shape = (6, 7, 8)
    sk = _random(shape, 0.2, 9)
    mask = np.ones(shape, np.uint8)
    off, vox = _made_up_segments(sk, 9)
    CANARY = -77
    for bad in (int(np.flatnonzero(sk.ravel() == 0)[3]), sk.size, -1):
        v = vox.copy()
        v[len(v) // 2] = bad
        labels, nearest, sizes = np.full(shape, CANARY, np.int32), np.full(shape, CANARY, np.int64), np.full(len(off), CANARY, np.int64)
        rc = dll.vmask_territories(0, mask.ctypes.data, sk.ctypes.data, *shape, off.ctypes.data, len(off) - 1, v.ctypes.data,
                                   labels.ctypes.data, nearest.ctypes.data, sizes.ctypes.data)
        assert rc == -1 and b'segment entries' in dll.vmask_last_error()
        assert (labels == CANARY).all() and (nearest == CANARY).all() and (sizes == CANARY).all()
    labels, nearest, sizes = np.full(shape, CANARY, np.int32), np.full(shape, CANARY, np.int64), np.full(len(off), CANARY, np.int64)
    assert dll.vmask_territories(0, mask.ctypes.data, sk.ctypes.data, *shape, off.ctypes.data, len(off) - 1, vox.ctypes.data,
                                 labels.ctypes.data, None, sizes.ctypes.data) == 0                     # nearest is optional
    want = TM.territories(mask, sk, off, vox)
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[2]) and (nearest == CANARY).all()
    assert dll.vmask_territories(0, mask.ctypes.data, sk.ctypes.data, 40000, 2, 2, off.ctypes.data, 0, None, labels.ctypes.data, None, sizes.ctypes.data) == -1
    assert b'shape' in dll.vmask_last_error()
    assert dll.vmask_territories(0, None, sk.ctypes.data, *shape, off.ctypes.data, 0, None, labels.ctypes.data, None, sizes.ctypes.data) == -1
    with pytest.raises(ValueError):
        S.branchTerritories(mask, np.ones((6, 7, 9), np.uint8))
    with pytest.raises(ValueError):
        S.branchTerritories(mask, sk, offsets=off)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(48, 40, 32), (47, 41, 33)])
def test_territories_end_to_end(shape):
    mask = M.crossing_phantom(shape)
    sk = S.skeletonize(mask)
    off, co = S.segmentArrays(sk)
    vox = _lin(shape, co)
    info = {}
    got = S.branchTerritories(mask, sk, info=info, return_nearest=True)                 # traces the segments itself
    labels, sizes, nearest = _assert_model(mask, sk, off, vox, got=got)
    assert info['segments'] == len(off) - 1 > 0 and int(sizes.sum()) == int(np.count_nonzero(mask))
    two = S.branchTerritories(mask, sk, off, co)
    assert len(two) == 2 and np.array_equal(two[0], labels) and np.array_equal(two[1], sizes)
    deg = SM.degrees(sk)
    for k in range(len(off) - 1):
        inner = co[off[k] + 1:off[k + 1] - 1]
        if len(inner):
            at = tuple(inner.T)
            assert (deg[at] == 2).all() and (labels[at] == k + 1).all() and np.array_equal(nearest[at], vox[off[k] + 1:off[k + 1] - 1])


@pytest.mark.gpu
def test_territories_deterministic():
    shape = (40, 36, 30)
    sk, mask = _random(shape, 0.02, 31), _random(shape, 0.6, 32)
    off, vox = _made_up_segments(sk, 31)
    a, b = _run(mask, sk, off, vox), _run(mask, sk, off, vox)
    assert a[1].sum() == mask.sum() and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import territory_model as TM
rng = np.random.default_rng(21)
sk = (rng.random((40, 36, 31)) < 0.03).astype(np.uint8)
sk[3:37, 18, 15] = 1
mask = (rng.random(sk.shape) < 0.5).astype(np.uint8)
dev = torch.device('cuda', 0)
off_h, co_h = S.segmentArrays(sk)
lab_h, siz_h, near_h = S.branchTerritories(mask, sk, return_nearest=True)
want = TM.territories(mask, sk, off_h, np.ravel_multi_index(co_h.T, sk.shape))
assert len(off_h) > 10 and np.array_equal(lab_h, want[0]) and np.array_equal(near_h, want[1]) and np.array_equal(siz_h, want[2])
tm, ts = torch.as_tensor(mask * 255, device=dev), torch.as_tensor(sk, device=dev)
lab_d, siz_d, near_d = S.branchTerritories(tm, ts, return_nearest=True)
assert lab_d.is_cuda and siz_d.is_cuda and near_d.is_cuda and lab_d.device == dev
assert lab_d.dtype == torch.int32 and siz_d.dtype == torch.int64 and near_d.dtype == torch.int64 and tuple(lab_d.shape) == sk.shape
assert lab_d.cpu().numpy().tobytes() == lab_h.tobytes() and siz_d.cpu().numpy().tobytes() == siz_h.tobytes()
assert near_d.cpu().numpy().tobytes() == near_h.tobytes()
# device segments given, and host segments with device volumes
off_d, co_d = S.segmentArrays(ts)
for off, co in ((off_d, co_d), (off_h, co_h)):
    lab, siz = S.branchTerritories(tm, ts, off, co)
    assert lab.is_cuda and lab.cpu().numpy().tobytes() == lab_h.tobytes() and siz.cpu().numpy().tobytes() == siz_h.tobytes()
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_territories_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, bit-identical to the host
    call.  Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_territories_main_writes_labels_and_volumes(tmp_path, capsys):
    from arterynetwork_amd import nifti
    m = M.crossing_phantom()
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, both, three = tmp_path / 'plain', tmp_path / 'both', tmp_path / 'three'
    for d in (plain, both, three):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    sk0 = S.main(str(plain))                                            # the defaults: what they always wrote
    assert isinstance(sk0, np.ndarray) and sorted(os.listdir(str(plain))) == ['skeleton.nii.gz', 'vesselVolumeMask.nii.gz']
    sk1, segs1 = S.main(str(both), segments=True)
    assert sorted(os.listdir(str(both))) == ['graphRepresentation.graphml', 'segmentList.npz', 'skeleton.nii.gz', 'vesselVolumeMask.nii.gz']
    capsys.readouterr()
    sk, segs, labels, sizes = S.main(str(three), segments=True, territories=True)
    said = capsys.readouterr().out
    for name in ('skeleton.nii.gz', 'graphRepresentation.graphml', 'segmentList.npz', 'segmentLabels.nii.gz', 'segmentTerritories.npz'):
        assert os.path.exists(str(three / name)) and '{} saved to {}.'.format(name, os.path.join(str(three), name)) in said
    assert len(os.listdir(str(three))) == 6
    assert np.array_equal(sk, sk0) and np.array_equal(sk, sk1) and segs == segs1 == S.traceSegments(sk)
    for name in ('skeleton.nii.gz', 'segmentList.npz', 'graphRepresentation.graphml'):
        if name.endswith('.npz'):
            assert [list(s) for s in np.load(str(three / name), allow_pickle=True)['segmentList']] == [list(s) for s in np.load(str(both / name), allow_pickle=True)['segmentList']]
        elif name.endswith('.graphml'):
            assert (three / name).read_bytes() == (both / name).read_bytes()
        else:
            assert np.array_equal(nifti.loadVolume(str(three), name)[0], nifti.loadVolume(str(both), name)[0])
    stored, aff2 = nifti.loadVolume(str(three), 'segmentLabels.nii.gz')
    assert stored.dtype == np.int32 and labels.dtype == np.int32 and np.array_equal(stored, labels) and np.allclose(aff2, aff)
    z = np.load(str(three / 'segmentTerritories.npz'))
    assert z['sizes'].dtype == np.int64 and z['volumes'].dtype == np.float64 and np.array_equal(z['sizes'], sizes)
    assert len(sizes) == len(segs) + 1 and sizes.sum() == np.count_nonzero(m) and np.allclose(z['volumes'], sizes * 0.4 * 0.4 * 0.6)
    back = np.load(str(three / 'segmentList.npz'), allow_pickle=True)['segmentList']
    for k, seg in enumerate(back):                                      # label k + 1 is entry k of segmentList.npz
        for p in seg[1:-1]:
            assert stored[tuple(p)] == k + 1
    off, co = S.segmentArrays(sk)
    want = TM.territories(m, sk, off, _lin(m.shape, co))
    assert np.array_equal(labels, want[0]) and np.array_equal(sizes, want[2])
