"""Segment tracing ("f6 segment tracing"): the sequential model tests/segment_model.py is checked for
soundness on the CPU, then the GPU tracing (vmask_segments / skeletonization.segmentArrays) must equal it exactly:
offsets, coordinates and all counts."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import segment_model as SM
import skeleton_model as M
from conftest import ROOT


# ------------------------------------------------------------------ the volumes
def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _line(axis, n=6000):
    shape = [1, 1, 1]
    shape[axis] = n
    return np.ones(shape, np.uint8)


def _diamond(tail=False):
    """|x| + |y| = 300 in one plane: 1200 voxels, every one of degree 2.  With `tail`: two more voxels in front of the corner
    of smallest index, which becomes a node with a loop hanging on it."""
    lead = 2 if tail else 0
    v = np.zeros((601 + lead, 601, 1), np.uint8)
    x, y = np.meshgrid(np.arange(-300, 301), np.arange(-300, 301), indexing='ij')
    v[lead:, :, 0] = (np.abs(x) + np.abs(y)) == 300
    if tail:
        v[0, 300, 0] = v[1, 300, 0] = 1
    return v


def _eye():
    """Two nodes (each with a stub, hence degree 3) joined by two different chains of nine path voxels."""
    v = np.zeros((9, 15, 9), np.uint8)
    v[4, 2, 4] = v[4, 12, 4] = 1                                       # the nodes
    v[4, 1, 4] = v[4, 13, 4] = 1                                       # their stubs
    v[3, 3:12, 4] = 1
    v[5, 3:12, 4] = 1
    return v


CHAIN_K = (0, 1, 2, 3, 4, 5, 63, 64, 65)


def _chains():
    """For every k of CHAIN_K: two junctions (a voxel with two stubs behind it) with k path voxels between them."""
    v = np.zeros((3 * len(CHAIN_K) + 1, 5, 75), np.uint8)
    for r, k in enumerate(CHAIN_K):
        x = 3 * r + 1
        v[x, 2, 2:4 + k] = 1                                             # junction, k path voxels, junction
        v[x, 1, 1] = v[x, 3, 1] = 1
        v[x, 1, 4 + k] = v[x, 3, 4 + k] = 1
    return v


def _cross():
    """A centre of degree 6 and six arms of length 3.  The arms leave along six of the eight space diagonals: the first
    voxels of arms along the axes would be 26-neighbours of each other, and the centre would not be the only junction."""
    v = np.zeros((9, 9, 9), np.uint8)
    v[4, 4, 4] = 1
    for d in [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)][1:7]:
        for j in (1, 2, 3):
            v[4 + j * d[0], 4 + j * d[1], 4 + j * d[2]] = 1
    return v


@functools.lru_cache(maxsize=None)
def _thinned_phantom(shape):
    return M.thin(M.crossing_phantom(shape))[0]


def _multi_tube(shape=(256, 256, 192)):
    """Nine disjoint wiggling tubes of different radii along axis 0 and a free ring (the phantom of the skeleton suite)."""
    x = np.arange(shape[0], dtype=np.float32)[:, None, None]
    y = np.arange(shape[1], dtype=np.float32)[None, :, None]
    z = np.arange(shape[2], dtype=np.float32)[None, None, :]
    m = np.zeros(shape, bool)
    k = 0
    for cy in (48, 112, 176):
        for cz in (40, 96, 152):
            r = 2.0 + 0.75 * k
            m |= ((y - cy - 12 * np.sin(2 * np.pi * x / shape[0] * (1 + k % 3))) ** 2 + (z - cz - 8 * np.cos(2 * np.pi * x / shape[0] * 2)) ** 2) <= r * r
            k += 1
    rho = np.sqrt((x - 128) ** 2 + (y - 230) ** 2)
    m |= ((rho - 14) ** 2 + (z - 96) ** 2) <= 9.0
    return m.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _multi_tube_skeleton():
    from arterynetwork_amd.skeletonization import skeletonize
    return skeletonize(_multi_tube())


CASES = {'line-1x1x6000': functools.partial(_line, 2), 'line-6000x1x1': functools.partial(_line, 0), 'line-1x6000x1': functools.partial(_line, 1),
         'ring-601x601x1': _diamond, 'ring-tail-603x601x1': functools.partial(_diamond, True),
         'eye': _eye, 'chains': _chains, 'cross': _cross,
         'phantom-48x40x32': functools.partial(_thinned_phantom, (48, 40, 32)),
         'phantom-47x41x33': functools.partial(_thinned_phantom, (47, 41, 33)),
         'empty-4x5x6': functools.partial(np.zeros, (4, 5, 6), np.uint8)}
for _d, _seed in ((0.02, 1), (0.05, 2), (0.1, 3), (0.35, 4)):
    CASES['random{}-40x36x30'.format(_d)] = functools.partial(_random, (40, 36, 30), _d, _seed)
for _s in [(7, 8, 9), (8, 9, 10), (2, 2, 2), (1, 1, 1), (1, 1, 40)]:
    CASES['random0.6-' + 'x'.join(map(str, _s))] = functools.partial(_random, _s, 0.6, 12)
for _s in [(96, 80, 72), (17, 64, 9), (3, 700, 5), (2, 6, 900)]:
    CASES['random0.1-' + 'x'.join(map(str, _s))] = functools.partial(_random, _s, 0.1, 10)
# The kernels over object voxels, darts and segment heads launch at most 256 blocks x 256 threads = 65 536 threads (GRID_LIST of
# vseg_device.hip): about 101 000 object voxels, twice as many darts and more segment heads than that give their grid-stride
# loops a second turn.
CASES['random0.3-260x260x5'] = functools.partial(_random, (260, 260, 5), 0.3, 16)
# The two kernels that read the volume launch at most 2048 x 256 threads of 16 voxels each = 8 388 608 voxels (GRID_VOLUME):
# 130 x 260 x 250 = 8 450 000 voxels take a second turn, sparse enough (about 17 000 object voxels) for the model.
CASES['random0.002-130x260x250'] = functools.partial(_random, (130, 260, 250), 0.002, 17)
GPU_ONLY_CASES = {'multi-tube-256x256x192': _multi_tube_skeleton}      # (its thinning is the GPU's own)
SLOW_ON_CPU = {'phantom-47x41x33'}                                       # (one thinned phantom is enough for the model's own tests)


@functools.lru_cache(maxsize=None)
def _volume(case):
    v = (CASES.get(case) or GPU_ONLY_CASES[case])()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _model(case):
    """The model's answer, computed once per case and shared."""
    off, co, counts = SM.arrays(_volume(case))
    off.setflags(write=False); co.setflags(write=False)
    return off, co, counts


def _edges(volume):
    """Every 26-adjacency edge of the object as a sorted pair of linear indices (numpy, independent of the model)."""
    obj = np.asarray(volume) != 0
    lin = np.arange(obj.size, dtype=np.int64).reshape(obj.shape)
    out = set()
    for a, b, c in SM.OFFSETS[13:]:                                      # the 13 offsets towards larger indices
        src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip((a, b, c), obj.shape))
        dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip((a, b, c), obj.shape))
        both = obj[src] & obj[dst]
        out.update(zip(lin[src][both].tolist(), lin[dst][both].tolist()))
    return out


# ------------------------------------------------------------------ CPU: the model itself
@pytest.mark.parametrize('case', sorted(set(CASES) - SLOW_ON_CPU))
def test_model_is_sound(case):
    v = _volume(case)
    segs, counts = SM.trace(v)
    deg = SM.degrees(v).ravel()
    obj = (v != 0).ravel()
    assert counts['nodes'] == int((obj & (deg != 2)).sum()) and counts['isolated'] == int((obj & (deg == 0)).sum())
    assert counts['path'] == int((obj & (deg == 2)).sum())
    seen = []
    for s in segs:
        assert len(s) >= 2 and all(deg[p] == 2 for p in s[1:-1])
        if s[0] != s[-1]:
            assert deg[s[0]] != 2 and deg[s[-1]] != 2 and s[0] < s[-1]
        else:
            assert len(s) >= 4 and s[1] < s[-2]
            if deg[s[0]] == 2:                                           # closed through the minimum of a free ring
                assert s[0] == min(s) and len(set(s)) == len(s) - 1
        seen.extend((min(p, q), max(p, q)) for p, q in zip(s[:-1], s[1:]))
    edges = _edges(v)
    assert len(seen) == len(set(seen)) and set(seen) == edges            # every edge in exactly one segment
    keys = [(s[0], s[1]) for s in segs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_model_known_answers():
    segs, counts = SM.trace(np.zeros((4, 5, 6), np.uint8))
    assert segs == [] and counts == {'nodes': 0, 'isolated': 0, 'path': 0}
    one = np.zeros((4, 5, 6), np.uint8); one[1, 2, 3] = 1
    segs, counts = SM.trace(one)
    assert segs == [] and counts['isolated'] == 1 and counts['nodes'] == 1
    two = one.copy(); two[2, 3, 4] = 1
    assert SM.trace(two)[0] == [[int(np.ravel_multi_index((1, 2, 3), two.shape)), int(np.ravel_multi_index((2, 3, 4), two.shape))]]
    for axis in range(3):
        line = np.zeros((9, 9, 9), np.uint8)
        at = [4, 4, 4]; at[axis] = slice(1, 8)
        line[tuple(at)] = 1
        assert SM.trace(line)[0] == [np.flatnonzero(line.ravel()).tolist()]
    diag = np.zeros((9, 9, 9), np.uint8)
    diag[np.arange(1, 8), np.arange(1, 8), np.arange(1, 8)] = 1
    assert SM.trace(diag)[0] == [np.flatnonzero(diag.ravel()).tolist()]
    off, co, counts = SM.arrays(_cross())
    assert len(off) == 7 and counts['nodes'] == 7 and counts['isolated'] == 0 and (np.diff(off) == 4).all()
    centre, tips = (4, 4, 4), set()
    for k in range(6):
        seg = [tuple(p) for p in co[off[k]:off[k + 1]].tolist()]
        assert centre in (seg[0], seg[-1])
        arm = seg if seg[0] == centre else seg[::-1]
        step = np.subtract(arm[1], arm[0])
        assert (np.abs(step) == 1).all() and all((np.subtract(q, p) == step).all() for p, q in zip(arm[:-1], arm[1:]))
        tips.add(arm[-1])
    assert len(tips) == 6
    ring = SM.trace(_diamond())[0]
    assert len(ring) == 1 and len(ring[0]) == 1201 and ring[0][0] == ring[0][-1] == min(ring[0])
    thin = _thinned_phantom((48, 40, 32))
    segs, counts = SM.trace(thin)
    print('thinned phantom:', int(thin.sum()), 'voxels,', len(segs), 'segments,', sum(len(s) == 2 for s in segs), 'of two voxels')
    assert len(segs) > 0 and counts['isolated'] == 0


def test_save_segment_list_round_trip(tmp_path):
    from arterynetwork_amd.skeletonization import saveSegmentList
    v = _volume('chains')
    off, co, _ = _model('chains')
    segs = [[tuple(p) for p in co[off[k]:off[k + 1]].tolist()] for k in range(len(off) - 1)]
    path = str(tmp_path / 'segmentList.npz')
    saveSegmentList(segs, path)
    back = np.load(path, allow_pickle=True)['segmentList']
    assert back.dtype == object and back.ndim == 1 and len(back) == len(segs) > len(CHAIN_K)
    assert [list(s) for s in back] == segs and all(type(c) is int for s in back for p in s for c in p)
    assert v[tuple(np.array(back[0]).T)].all()
    saveSegmentList([], path)
    assert len(np.load(path, allow_pickle=True)['segmentList']) == 0


def test_write_graphml_matches_networkx(tmp_path):
    nx = pytest.importorskip('networkx')
    from arterynetwork_amd.skeletonization import writeGraphml
    for case in ('chains', 'eye', 'ring-tail-603x601x1', 'random0.35-40x36x30'):
        off, co, _ = _model(case)
        segs = [[tuple(p) for p in co[off[k]:off[k + 1]].tolist()] for k in range(len(off) - 1)]
        path = str(tmp_path / 'graphRepresentation.graphml')
        writeGraphml(segs, path)
        got = nx.read_graphml(path)
        G = nx.Graph()
        for k, seg in enumerate(segs):
            nx.add_path(G, seg, segmentIndex=k)
        assert not got.is_directed() and set(got.nodes) == {str(v) for v in G.nodes}
        want = {frozenset((str(a), str(b))): d['segmentIndex'] for a, b, d in G.edges(data=True)}
        have = {frozenset((a, b)): d['segmentIndex'] for a, b, d in got.edges(data=True)}
        assert have == want and all(type(k) is int for k in have.values())


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_segment_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vseg_device.hip' in build.SOURCES
    out = tmp_path / 'vseg_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vseg_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1))
    for frag in ('k_seg_count', 'k_seg_compact', 'k_seg_gather', 'k_seg_link', 'k_seg_jump', 'k_seg_resolve', 'k_seg_heads', 'k_seg_scatter'):
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, scratch in recs.items():
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)


# ------------------------------------------------------------------ GPU: exactly the model
def _assert_equal_to_model(case, got, info):
    off, co, counts = _model(case)
    g_off, g_co = got
    assert g_off.dtype == np.int64 and g_co.dtype == np.int64 and g_co.shape == (int(off[-1]), 3)
    assert np.array_equal(g_off, off) and np.array_equal(g_co, co)
    assert info['segments'] == len(off) - 1 and info['nodes'] == counts['nodes'] and info['isolated'] == counts['isolated']


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(set(CASES) | set(GPU_ONLY_CASES)))
def test_segments_equal_the_model(case):
    from arterynetwork_amd.skeletonization import segmentArrays
    v = _volume(case)
    assert v.sum() < 2.2e5
    info = {}
    got = segmentArrays(v, info=info)
    print(case, 'voxels', int(v.sum()), 'segments', info['segments'], 'nodes', info['nodes'], 'isolated', info['isolated'], 'rounds', info['rounds'])
    _assert_equal_to_model(case, got, info)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['line-1x1x6000', 'line-6000x1x1', 'line-1x6000x1', 'ring-601x601x1'])
def test_segments_rounds_grow_with_the_logarithm(case):
    """A thread that walked a chain voxel by voxel would need thousands of rounds here; doubling needs about ceil(log2) of them
    (the bound leaves room for a ring that is cut and ranked a second time)."""
    from arterynetwork_amd.skeletonization import segmentArrays
    P = _model(case)[2]['path']
    info = {}
    segmentArrays(_volume(case), info=info)
    bound = 2 * math.ceil(math.log2(P + 1)) + 4
    print(case, 'path voxels', P, 'rounds', info['rounds'], 'bound', bound)
    assert P >= 1200 and 1 <= info['rounds'] <= bound


@pytest.mark.gpu
def test_segments_deterministic():
    from arterynetwork_amd.skeletonization import segmentArrays
    v = _volume('multi-tube-256x256x192')
    a, b = segmentArrays(v), segmentArrays(v)
    assert len(a[0]) > 10 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.gpu
def test_segments_input_encodings():
    """Any non-zero value is object: 0/255, bool, float and a Fortran-ordered view give the result of the 0/1 mask."""
    from arterynetwork_amd.skeletonization import segmentArrays
    case = 'random0.1-17x64x9'
    v = _volume(case)
    for w in (v * 255, v.astype(bool), v.astype(np.float32) * 0.25, np.asfortranarray(v)):
        info = {}
        _assert_equal_to_model(case, segmentArrays(w, info=info), info)


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import segment_model as SM
rng = np.random.default_rng(21)
m = (rng.random((40, 36, 31)) < 0.06).astype(np.uint8)
m[3:37, 18, 15] = 1
dev = torch.device('cuda', 0)
info_h, info_d = {{}}, {{}}
off_h, co_h = S.segmentArrays(m, info=info_h)
off_m, co_m, _ = SM.arrays(m)
assert len(off_h) > 10 and np.array_equal(off_h, off_m) and np.array_equal(co_h, co_m)
off_d, co_d = S.segmentArrays(torch.as_tensor(m * 255, device=dev), info=info_d)
assert off_d.is_cuda and co_d.is_cuda and off_d.device == dev and co_d.device == dev
assert off_d.dtype == torch.int64 and co_d.dtype == torch.int64 and tuple(co_d.shape) == co_h.shape
assert np.array_equal(off_d.cpu().numpy(), off_h) and np.array_equal(co_d.cpu().numpy(), co_h) and info_d == info_h
# (a volume that starts at an odd device address)
flat = torch.zeros(m.size + 1, dtype=torch.uint8, device=dev)
odd = flat[1:].view(m.shape); odd.copy_(torch.as_tensor(m, device=dev))
off_o, co_o = S.segmentArrays(odd)
assert odd.data_ptr() % 4 != 0 and np.array_equal(off_o.cpu().numpy(), off_h) and np.array_equal(co_o.cpu().numpy(), co_h)
assert S.traceSegments(odd) == S.traceSegments(m)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_segments_device_resident():
    """A tensor on the GPU goes in by its device pointer and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_segments_capacity_protocol():
    from arterynetwork_amd import skeletonization as S
    from arterynetwork_amd._capi import VrgError
    dll = S._skeleton_lib()
    case = 'random0.1-17x64x9'
    v = np.ascontiguousarray(_volume(case))
    off, co, counts = _model(case)
    nseg, total = len(off) - 1, int(off[-1])
    lin = np.ravel_multi_index(co.T, v.shape)
    only = np.full(5, -1, np.int64)
    assert dll.vmask_segments(0, v.ctypes.data, *v.shape, only.ctypes.data, None, 0, None, 0) == 0
    assert only[0] == nseg and only[1] == total and only[2] == counts['nodes'] and only[3] == counts['isolated']
    CANARY = -77
    for cap_seg, cap_vox, rc_want in ((nseg, total, 0), (nseg - 1, total, -1), (nseg, total - 1, -1)):
        cnt = np.full(5, -1, np.int64)
        offsets, voxels = np.full(nseg + 2, CANARY, np.int64), np.full(total + 1, CANARY, np.int64)
        rc = dll.vmask_segments(0, v.ctypes.data, *v.shape, cnt.ctypes.data, offsets.ctypes.data, cap_seg, voxels.ctypes.data, cap_vox)
        assert rc == rc_want and np.array_equal(cnt, only)                # the needed sizes either way
        if rc_want:
            assert (offsets == CANARY).all() and (voxels == CANARY).all()   # nothing written
            assert b'capacity' in dll.vmask_last_error()
        else:
            assert np.array_equal(offsets[:-1], off) and np.array_equal(voxels[:-1], lin) and offsets[-1] == CANARY and voxels[-1] == CANARY
    # an empty volume: zero segments, offsets[0] = 0
    e = np.zeros((4, 5, 6), np.uint8)
    cnt, offsets, voxels = np.full(5, -1, np.int64), np.full(2, CANARY, np.int64), np.full(1, CANARY, np.int64)
    assert dll.vmask_segments(0, e.ctypes.data, 4, 5, 6, cnt.ctypes.data, offsets.ctypes.data, 0, voxels.ctypes.data, 0) == 0
    assert (cnt == 0).all() and offsets[0] == 0 and offsets[1] == CANARY and voxels[0] == CANARY
    with pytest.raises(ValueError):
        S.segmentArrays(np.ones((8, 8), np.uint8))
    with pytest.raises(ValueError):
        S.segmentArrays(np.ones((2, 3, 4, 5), np.uint8))
    # over the 32-bit envelope: refused before any voxel is touched (the buffers here are tiny)
    buf = np.zeros(8, np.uint8)
    assert dll.vmask_segments(0, buf.ctypes.data, 2000, 2000, 600, cnt.ctypes.data, None, 0, None, 0) == -1      # VRG_E_ARG
    assert b'shape' in dll.vmask_last_error()
    with pytest.raises(VrgError):
        S._G._check(dll.vmask_segments(0, buf.ctypes.data, 40000, 2, 2, cnt.ctypes.data, None, 0, None, 0))
    assert dll.vmask_segments(0, None, 2, 2, 2, cnt.ctypes.data, None, 0, None, 0) == -1
    assert dll.vmask_segments(0, buf.ctypes.data, 2, 2, 2, None, None, 0, None, 0) == -1


@pytest.mark.gpu
def test_segments_main_writes_the_three_files(tmp_path, capsys):
    from arterynetwork_amd import nifti, skeletonization as S
    m = M.crossing_phantom()
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, both = tmp_path / 'plain', tmp_path / 'both'
    for d in (plain, both):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    sk0 = S.main(str(plain))                                            # without the keyword: today's behaviour
    assert isinstance(sk0, np.ndarray) and sorted(os.listdir(str(plain))) == ['skeleton.nii.gz', 'vesselVolumeMask.nii.gz']
    capsys.readouterr()
    sk, segs = S.main(str(both), segments=True)
    said = capsys.readouterr().out
    for name in ('skeleton.nii.gz', 'graphRepresentation.graphml', 'segmentList.npz'):
        assert os.path.exists(str(both / name)) and '{} saved to {}.'.format(name, os.path.join(str(both), name)) in said
    assert np.array_equal(sk, sk0) and np.array_equal(sk, _thinned_phantom((48, 40, 32)))
    info = {}
    assert segs == S.traceSegments(sk, info=info) and len(segs) == info['segments'] > 0
    back = np.load(str(both / 'segmentList.npz'), allow_pickle=True)['segmentList']
    assert [list(s) for s in back] == segs
    marked = np.zeros_like(sk)
    for s in segs:
        marked[tuple(np.array(s).T)] = 1
    stored, _ = nifti.loadVolume(str(both), 'skeleton.nii.gz')
    assert not (marked & ~stored).any() and int(stored.sum()) - int(marked.sum()) == info['isolated']
    assert np.array_equal(marked, stored & (SM.degrees(stored) > 0))
    with open(str(both / 'graphRepresentation.graphml')) as f:
        text = f.read()
    assert text.count('<edge ') == sum(len(s) - 1 for s in segs) and 'segmentIndex' in text
