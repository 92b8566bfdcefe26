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

import envelope_trace as ET
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


# ------------------------------------------------------------------ the paths that the cases above never enter
# Every case below is (skeleton, mask); the CPU tests state with tests/envelope_trace.py which branch of k_ter_envelope a case
# drives, the GPU tests demand exact equality with the model (or with a closed form where the model would be slow).
def _deep_square(k=0):
    """160 x 160: the diagonal with sites at (120, k) and (150, 20 + k) - they pop a deep stack below the ring while it is being
    built (the trace: depth 81, 195 chunk reloads in the build loop for k = 0, but no spill after them) - and, so that a line
    also spills AGAIN after such a reload, two runs of 50 sites: rows 0-49 in column c0 + 30, rows 50-99 in column c0.  Line c0
    stacks 50 parabolas of G = 900, the site (50, c0) pops those that start within 30 of it, rows 51-99 push 49 more."""
    s = np.zeros((160, 160), np.uint8)
    s[np.arange(160), np.arange(160)] = 1
    s[120, k] = s[150, 20 + k] = 1
    c0 = 120 - 8 * k
    s[0:50, c0 + 30] = 1
    s[50:100, c0] = 1
    return s


def _narrow_square():
    """160 x 65: a slanted line of sites and the two runs of _deep_square for column 64, the one active lane of the second
    64-lane item of an inner extent of 65."""
    s = np.zeros((160, 65), np.uint8)
    s[np.arange(160), np.arange(160) * 2 // 5] = 1
    s[0:50, 34] = 1
    s[50:160, 64] = 1
    return s


def _sparse_mask(shape, dense, every=97):
    """The voxels of the slices `dense`, plus every 97th voxel of the volume: the envelope work does not depend on the mask,
    the brute-force model costs mask voxels x sites."""
    mask = np.zeros(shape, np.uint8)
    mask.ravel()[::every] = 1
    mask[dense] = 1
    return mask


def _deep_case(name):
    if name == 'deep-1x160x160':
        sk = _deep_square().reshape(1, 160, 160)
    elif name == 'deep-160x160x1':
        sk = _deep_square().reshape(160, 160, 1)
    elif name == 'deep-3x160x160':
        sk = np.stack([_deep_square(k) for k in range(3)], axis=0)
    elif name == 'deep-160x160x3':
        sk = np.stack([_deep_square(k) for k in range(3)], axis=2)
    elif name == 'deep-160x3x160':
        sk = np.stack([_deep_square(k) for k in range(3)], axis=1)
    elif name == 'deep-1x160x65':
        sk = _narrow_square().reshape(1, 160, 65)
    elif name == 'deep-160x65x1':
        sk = _narrow_square().reshape(160, 65, 1)
    elif name == 'deep64-1x160x23200':
        sk = np.zeros((1, 160, 23200), np.uint8)
        sk[0, :, :160] = _deep_square()
        return sk, _sparse_mask(sk.shape, np.s_[:, :, :160])
    elif name == 'deep64-23200x160x1':
        sk = np.zeros((23200, 160, 1), np.uint8)
        sk[:160, :, 0] = _deep_square()
        return sk, _sparse_mask(sk.shape, np.s_[:320])
    return np.ascontiguousarray(sk), np.ones(sk.shape, np.uint8)


# name -> (the envelope pass that must go deep, the lines of it that are traced (None: all), the lines that must EACH meet the
# conditions (None: the pass as a whole))
DEEP = {
    'deep-1x160x160': (1, None, [(0, 120)]),
    'deep-160x160x1': (0, None, [(0, 120)]),
    'deep-3x160x160': (1, None, [(0, 120), (1, 112), (2, 104)]),       # (a spill region with o > 0 in every plane)
    'deep-160x160x3': (0, None, [(0, 120 * 3), (0, 112 * 3 + 1), (0, 104 * 3 + 2)]),
    'deep-160x3x160': (0, None, [(0, 120), (0, 160 + 112), (0, 320 + 104)]),
    'deep-1x160x65': (1, None, [(0, 64)]),                             # (lane 0 of the second item; its other 63 lanes are idle)
    'deep-160x65x1': (0, None, [(0, 64)]),
    'deep64-1x160x23200': (1, range(160), [(0, 120)]),
    'deep64-23200x160x1': (0, None, [(0, 120)]),
}


def _trace(name, reload=True):
    axis, inner, _ = DEEP[name]
    sk = _deep_case(name)[0]
    return ET.trace_pass((ET.axis1_lines if axis == 1 else ET.axis0_lines)(sk, inner), reload)


def _wide_case(axis, n=23200):
    """Sparse random sites (density 0.003) in n x 3 x 2 with sites placed at both ends and mid-way on different rows, the long
    axis moved to `axis`: the winning parabolas carry large, unequal G through the 64-bit arithmetic."""
    sk = _random((n, 3, 2), 0.003, 300 + axis)
    sk[0, 0, 0] = sk[n - 1, 2, 1] = sk[n // 2, 1, 0] = sk[n // 2 + 1, 2, 1] = sk[1, 2, 0] = sk[n - 2, 0, 1] = 1
    order = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0)}[axis]
    sk = np.ascontiguousarray(sk.transpose(order))
    return sk, _random(sk.shape, 0.5, 310 + axis)


LIMIT_PLANES = [0, 1, 2, 100, 101, 102, 1000, 1002, 5000, 5001, 8191, 8192, 11585, 16384, 21000, 23168, 23169]


def _limit_case(axis, n):
    """23170 x 3 x 2 (n = 23171: one empty plane more), the long axis moved to `axis`.  Sites in neighbouring planes (divisor 2)
    and thousands of planes apart, in cells of the 3 x 2 cross-section in turn, so that along the long axis the quotients of
    the start formula run into the thousands with G differences of 0 (exact multiples) and of a few units (just beside an
    integer), and across it a line of length 3 or 2 meets G differences of up to 23169^2 over a divisor of 2: quotients far
    above 32768, the entries that are not pushed.  A few random sites on top."""
    sk = np.zeros((n, 3, 2), np.uint8)
    for k, p in enumerate(LIMIT_PLANES):
        sk[p, k % 3, (k // 3) % 2] = 1
    sk[1000, 2, 1] = sk[21000, 2, 1] = sk[3000, 0, 0] = sk[13000, 0, 0] = 1
    sk[7000, 1, 0] = sk[7001, 1, 1] = sk[7100, 1, 0] = sk[7101, 1, 0] = 1          # neighbours in one row of the cross-section
    rng = np.random.default_rng(320)
    sk[rng.integers(0, 23170, 20), rng.integers(0, 3, 20), rng.integers(0, 2, 20)] = 1
    order = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0)}[axis]
    sk = np.ascontiguousarray(sk.transpose(order))
    return sk, np.ones(sk.shape, np.uint8)


NEW = {name: functools.partial(_deep_case, name) for name in DEEP}
for _axis in range(3):
    NEW['wide-axis%d' % _axis] = functools.partial(_wide_case, _axis)
    for _n in (23170, 23171):
        NEW['limit-%d-axis%d' % (_n, _axis)] = functools.partial(_limit_case, _axis, _n)


@functools.lru_cache(maxsize=None)
def _new_model(name):
    """(mask, skeleton, offsets, voxels, labels, nearest, sizes) of a case of NEW: the model runs once (read-only)."""
    sk, mask = NEW[name]()
    off, vox = _made_up_segments(sk, 7)
    out = (mask, sk, off, vox) + TM.territories(mask, sk, off, vox)
    for a in out:
        a.setflags(write=False)
    return out


def test_trace_equals_brute_force_on_random_lines():
    rng = np.random.default_rng(40)
    seen = {'ties': 0, 'gaps': 0, 'spilled': 0}
    for i in range(400):
        m = int(rng.integers(1, 48))
        G = rng.integers(-1, (3, 30, 2000)[i % 3], m)                    # few distinct values: equal values and ties abound
        if i % 7 == 0:
            G[:] = -1 if i % 2 else 0
        t = ET.trace_line(G)
        assert np.array_equal(t.winners, ET.brute_winners(G)), G.tolist()
        seen['gaps'] += bool((G < 0).any() and (G >= 0).any())
        seen['ties'] += len(set(G[G >= 0].tolist())) < int((G >= 0).sum())
        seen['spilled'] += t.spills > 0
    assert seen['gaps'] > 100 and seen['ties'] > 100 and seen['spilled'] > 5
    # a line of G = 0 is a stack as deep as the line, spilled and read back; one that pops and grows again
    t = ET.trace_line([0] * 100)
    assert (t.depth, t.spills, t.build_reloads, t.read_reloads) == (100, 11, 0, 11) and t.winners.tolist() == list(range(100))
    G = [900] * 50 + [0] * 50
    t = ET.trace_line(G)
    assert t.build_reloads >= 1 and t.spills_after_reload >= 1 and np.array_equal(t.winners, ET.brute_winners(G))


def test_existing_diagonals_never_reload_while_building():
    """Why the deep cases below exist: the 300 x 300 diagonals spill and read back 5100 chunks, but no pop of the build loop
    ever reaches below the ring."""
    for lead, lines in ((True, ET.axis1_lines), (False, ET.axis0_lines)):
        total, _ = ET.trace_pass(lines(_diagonal_case(lead)))
        assert total.counts() == {'depth': 151, 'spills': 5100, 'build_reloads': 0, 'read_reloads': 5100, 'spills_after_reload': 0}
    sq = np.zeros((160, 160), np.uint8)                                 # the diagonal and the two popping sites alone
    sq[np.arange(160), np.arange(160)] = 1
    sq[120, 0] = sq[150, 20] = 1
    total, _ = ET.trace_pass(ET.axis1_lines(sq.reshape(1, 160, 160)))
    assert total.counts() == {'depth': 81, 'spills': 1360, 'build_reloads': 195, 'read_reloads': 1165, 'spills_after_reload': 0}


@pytest.mark.parametrize('name', sorted(DEEP))
def test_deep_cases_reach_their_paths(name):
    """The conditions of a deep case, per pass and for every line that is named: a stack of at least 2 RING entries, a chunk
    reload in the build loop, a spill after it, a reload in the read-back loop; the trace's winners are the brute-force ones;
    and the mutation "load_top without its reload" changes the winners, so a kernel with that defect cannot pass the case."""
    total, each = _trace(name)
    for t in [total] + [each[key] for key in DEEP[name][2]]:
        assert t.depth >= 2 * ET.RING and t.build_reloads >= 1 and t.spills_after_reload >= 1 and t.read_reloads >= 1, t.counts()
    axis, inner, named = DEEP[name]
    sk = _deep_case(name)[0]
    lines = dict((ET.axis1_lines if axis == 1 else ET.axis0_lines)(sk, [c for _, c in named] if axis == 0 or sk.shape[0] == 1 else None))
    for key in named:
        want = ET.brute_winners(lines[key])
        assert np.array_equal(each[key].winners, want)
        assert not np.array_equal(ET.trace_line(lines[key], reload=False).winners, want)


def _kernel_is_32bit(shape):
    """The kernel's own rule, read from its source: 32-bit arithmetic where n0^2 + n1^2 + n2^2 < 2^bits."""
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vter_device.hip')).read()
    m = re.search(r'const bool small = \(int64_t\)d\.n0 \* d\.n0 \+ \(int64_t\)d\.n1 \* d\.n1 \+ \(int64_t\)d\.n2 \* d\.n2 < \(\(int64_t\)1 << (\d+)\);', src)
    assert m, 'the rule that chooses the arithmetic has moved'
    return sum(int(n) ** 2 for n in shape) < (1 << int(m.group(1)))


def test_new_cases_sides_of_the_arithmetic_rule_and_cost():
    for name in NEW:
        sk, mask = NEW[name]()
        assert sk.shape == mask.shape and sk.any()
        assert np.count_nonzero(mask) * np.count_nonzero(sk) <= 10 ** 8, name         # the model's distance entries
        small = _kernel_is_32bit(sk.shape)
        assert small == (not name.startswith(('deep64', 'wide', 'limit-23171'))), name
    assert _kernel_is_32bit((23170, 3, 2)) and not _kernel_is_32bit((23171, 3, 2)) and not _kernel_is_32bit((23171, 1, 1))


def test_limit_cases_hold_the_quotients_they_are_for():
    """Along the long axis: divisors of 2, exact multiples and near-multiples with quotients in the thousands (below 32768);
    across it: quotients of 32768 and more (the 32-bit floordiv's "do not push" answer)."""
    for axis, lines in ((0, ET.axis0_lines), (1, ET.axis1_lines)):
        div = []
        ET.trace_pass(lines(_limit_case(axis, 23170)[0]), divisions=div)
        q = [(a // b, a % b, b) for a, b in div]
        assert any(b == 2 for _, _, b in q)
        assert sum(1000 <= f < 32768 and r == 0 for f, r, _ in q) >= 5                # the float quotient may land on either side
        assert sum(1000 <= f < 32768 and r in (1, 2, b - 1, b - 2) and b > 1000 for f, r, b in q) >= 5
    for axis, lines in ((1, ET.axis0_lines), (2, ET.axis1_lines)):
        div = []
        ET.trace_pass(lines(_limit_case(axis, 23170)[0]), divisions=div)
        big = [a // b for a, b in div if a // b >= 32768]
        assert len(big) >= 100 and max(big) > 10 ** 6 and all(b <= 4 for _, b in div)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(NEW))
def test_territories_untested_paths(name):
    """Deep stacks with reloads while building and several outer lines; 64-bit arithmetic with content; the 32-bit arithmetic
    at its last extent and the first extent past it."""
    mask, sk, off, vox = _new_model(name)[:4]
    labels, sizes, nearest = _assert_model(mask, sk, off, vox, want=_new_model(name)[4:])
    if name.startswith('limit-23171'):                                  # the same sites one extent earlier: the same answer
        axis = int(name[-1])
        other = _new_model('limit-23170-axis%d' % axis)[5]
        cut = [slice(None)] * 3
        cut[axis] = slice(0, 23170)
        here = np.stack(np.unravel_index(nearest[tuple(cut)].ravel(), sk.shape))
        there = np.stack(np.unravel_index(other.ravel(), other.shape))
        assert np.array_equal(here, there)


STRIDE_SHAPE = (64, 64, 80)                                            # 327 680 voxels: more than the 1024 x 256 threads of k_ter_sites


def _stride_segments(variant):
    V = int(np.prod(STRIDE_SHAPE))
    perm = np.random.default_rng(50).permutation(V).astype(np.int64)
    if variant == 'all':
        return np.arange(V + 1, dtype=np.int64), perm
    # the last 70 000 voxels in no segment; the 5 000 earliest segments come again behind entry 262 144 as segments of their own
    # (the very last entry is segment 0's voxel): the smaller label must hold on the loop's second trip
    vox = perm[perm < V - 70000]
    vox = np.concatenate([vox, vox[:5000][::-1]])
    return np.arange(len(vox) + 1, dtype=np.int64), vox


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['all', 'repeats'])
def test_territories_more_entries_than_threads(variant):
    ones = np.ones(STRIDE_SHAPE, np.uint8)
    off, vox = _stride_segments(variant)
    assert len(vox) > 262144 and len(off) - 1 > 262144
    L = TM.site_labels(STRIDE_SHAPE, off, vox)
    if variant == 'repeats':
        assert L.ravel()[vox[-1]] == 1 and (L.ravel()[-70000:] == 0).all() and L.max() == len(vox) - 5000
    want = (L, np.arange(ones.size, dtype=np.int64).reshape(STRIDE_SHAPE), np.bincount(L.ravel(), minlength=len(off)).astype(np.int64))
    labels, sizes, nearest = _assert_model(ones, ones, off, vox, want=want)
    assert sizes[0] == (0 if variant == 'all' else 70000) and sizes[1:].max() == 1


@pytest.mark.gpu
def test_territories_bad_entry_behind_the_first_trip():
    dll = S._skeleton_lib()
    ones = np.ones(STRIDE_SHAPE, np.uint8)
    off, vox = _stride_segments('all')
    CANARY = -77
    for at, bad in ((300000, ones.size), (len(vox) - 1, -1)):
        v = vox.copy()
        v[at] = bad
        labels, nearest, sizes = np.full(STRIDE_SHAPE, CANARY, np.int32), np.full(STRIDE_SHAPE, CANARY, np.int64), np.full(len(off), CANARY, np.int64)
        rc = dll.vmask_territories(0, ones.ctypes.data, ones.ctypes.data, *STRIDE_SHAPE, off.ctypes.data, len(off) - 1, v.ctypes.data,
                                   labels.ctypes.data, nearest.ctypes.data, sizes.ctypes.data)
        assert rc == -1 and b'1 segment entries' in dll.vmask_last_error()
        assert (labels == CANARY).all() and (nearest == CANARY).all() and (sizes == CANARY).all()
    o = off.copy()
    o[290000] = o[290001] + 1                                           # offsets that descend, behind the first trip
    labels, nearest, sizes = np.full(STRIDE_SHAPE, CANARY, np.int32), np.full(STRIDE_SHAPE, CANARY, np.int64), np.full(len(off), CANARY, np.int64)
    rc = dll.vmask_territories(0, ones.ctypes.data, ones.ctypes.data, *STRIDE_SHAPE, o.ctypes.data, len(off) - 1, vox.ctypes.data,
                               labels.ctypes.data, nearest.ctypes.data, sizes.ctypes.data)
    assert rc == -1 and b'segment entries' in dll.vmask_last_error()
    assert (labels == CANARY).all() and (nearest == CANARY).all() and (sizes == CANARY).all()
