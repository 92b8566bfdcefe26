"""Curve skeleton: the sequential model tests/skeleton_model.py is checked for soundness on the
CPU, then the GPU thinning (vmask_skeleton / skeletonization.skeletonize) must equal it bit for bit."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import skeleton_model as M
from conftest import ROOT
from oracle import mask_oracle as MO
from test_mask_stage import _volumes


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _neighbour_count(v):
    p = np.pad(np.asarray(v) != 0, 1).astype(np.int32)
    n = sum(p[a:a + v.shape[0], b:b + v.shape[1], c:c + v.shape[2]] for a in range(3) for b in range(3) for c in range(3))
    return n - p[1:-1, 1:-1, 1:-1]


# ------------------------------------------------------------------ CPU: the model itself
MODEL_CASES = {'phantom': lambda: M.crossing_phantom(),
               'random0.1': lambda: _random((20, 18, 16), 0.1, 1),
               'random0.35': lambda: _random((20, 18, 16), 0.35, 2),
               'random0.6': lambda: _random((20, 18, 16), 0.6, 3)}


@pytest.mark.parametrize('case', sorted(MODEL_CASES))
def test_model_preserves_topology_and_finishes(case):
    m = MODEL_CASES[case]()
    sk, cycles = M.thin(m)
    assert sk.dtype == np.uint8 and set(np.unique(sk)) <= {0, 1} and cycles >= 1
    assert not (sk & ~(m != 0)).any()                              # a subset of the object
    assert M.topology(sk) == M.topology(m)                         # 26-components, background 6-components
    assert M.deletable_left(sk) == []                              # nothing border, simple and not an end point is left
    again, c2 = M.thin(sk)
    assert np.array_equal(again, sk) and c2 == 1


def test_model_phantom_becomes_curves():
    m = M.crossing_phantom()
    sk, _ = M.thin(m)
    assert M.topology(m)[0] == 2 and 0 < sk.sum() < m.sum() // 5


def test_model_known_answers():
    sk, cycles = M.thin(np.zeros((5, 6, 7), np.uint8))
    assert not sk.any() and cycles == 1
    one = np.zeros((5, 6, 7), np.uint8); one[2, 3, 4] = 1
    assert np.array_equal(M.thin(one)[0], one)                      # an isolated voxel is not simple
    for axis in range(3):
        line = np.zeros((9, 9, 9), np.uint8)
        idx = [4, 4, 4]; idx[axis] = slice(1, 8)
        line[tuple(idx)] = 1
        assert np.array_equal(M.thin(line)[0], line)
    diag = np.zeros((9, 9, 9), np.uint8)
    diag[np.arange(1, 8), np.arange(1, 8), np.arange(1, 8)] = 1
    assert np.array_equal(M.thin(diag)[0], diag)
    ring = M.ring_phantom()
    sk, _ = M.thin(ring)
    assert sk.any() and _neighbour_count(sk)[sk != 0].min() >= 2    # a closed curve: no end point, nothing isolated
    assert M.topology(sk) == M.topology(ring) == (1, 1)


# ------------------------------------------------------------------ GPU: bit-exact against the model
def _vessel(seed, shape):
    brain, ves = _volumes(seed, shape)
    return MO.vesselVolumeMask(brain, ves)


def _block(shape):
    return np.ones(shape, np.uint8)


def _faces(shape, seed):
    """An object that touches every face of the volume: the six faces' centre lines through a random interior."""
    v = _random(shape, 0.2, seed)
    c = [n // 2 for n in shape]
    v[:, c[1], c[2]] = 1; v[c[0], :, c[2]] = 1; v[c[0], c[1], :] = 1
    return v


SHAPES = [(40, 36, 30), (17, 64, 9), (1, 50, 33), (3, 700, 5), (2, 6, 900), (96, 80, 72)]
GPU_CASES = {}
for _s in SHAPES:
    _name = 'x'.join(map(str, _s))
    _d = 0.35 if _s != (96, 80, 72) else 0.1             # (the model stays in seconds)
    GPU_CASES['random{}-{}'.format(_d, _name)] = functools.partial(_random, _s, _d, 10)
    GPU_CASES['faces-' + _name] = functools.partial(_faces, _s, 11)
    if _s != (96, 80, 72):
        GPU_CASES['block-' + _name] = functools.partial(_block, _s)
for _s in [(7, 8, 9), (8, 9, 10), (9, 7, 8), (6, 6, 6), (5, 5, 5), (1, 1, 1), (1, 1, 40), (2, 2, 2)]:   # odd and even extents on every axis
    _name = 'x'.join(map(str, _s))
    GPU_CASES['block-' + _name] = functools.partial(_block, _s)
    GPU_CASES['random0.6-' + _name] = functools.partial(_random, _s, 0.6, 12)
GPU_CASES['random0.1-40x36x30'] = functools.partial(_random, (40, 36, 30), 0.1, 13)
GPU_CASES['random0.6-40x36x30'] = functools.partial(_random, (40, 36, 30), 0.6, 14)
GPU_CASES['random0.6-33x31x29'] = functools.partial(_random, (33, 31, 29), 0.6, 15)
GPU_CASES['vessel-40x36x30'] = functools.partial(_vessel, 0, (40, 36, 30))
GPU_CASES['vessel-96x80x72'] = functools.partial(_vessel, 5, (96, 80, 72))
GPU_CASES['phantom-48x40x32'] = M.crossing_phantom
GPU_CASES['phantom-47x41x33'] = functools.partial(M.crossing_phantom, (47, 41, 33))
GPU_CASES['empty-4x5x6'] = functools.partial(np.zeros, (4, 5, 6), np.uint8)
# 260 * 260 * ceil(5 / 64) = 67 600 items of one wave each, more than the 16384 blocks x 4 waves = 65 536 that the whole-volume
# kernels (pad, mark, unpad) launch at most: their grid-stride loops take a second turn.  Thin along i2 so that the object, about
# 100 000 voxels, stays under the cap below and the sequential model stays affordable.
GPU_CASES['random0.3-260x260x5'] = functools.partial(_random, (260, 260, 5), 0.3, 16)


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(GPU_CASES))
def test_skeleton_bit_exact(case):
    from arterynetwork_amd.skeletonization import skeletonize
    m = GPU_CASES[case]()
    assert m.sum() < 2.2e5
    ref, ref_cycles = M.thin(m)
    info = {}
    got = skeletonize(m, info=info)
    print(case, 'voxels', int(m.sum()), '->', info['kept'], 'cycles', info['cycles'], '(model', int(ref.sum()), ref_cycles, ')')
    assert got.dtype == np.uint8 and got.shape == m.shape
    assert np.array_equal(got, ref)
    assert info['kept'] == int(ref.sum()) and info['cycles'] == ref_cycles


@pytest.mark.gpu
def test_skeleton_input_encodings():
    """Any non-zero value is object: 0/255, bool, float and a non-contiguous view give the skeleton of the 0/1 mask."""
    from arterynetwork_amd.skeletonization import skeletonize
    m = _vessel(0, (40, 36, 30))
    ref, _ = M.thin(m)
    assert np.array_equal(skeletonize(m * 255), ref)
    assert np.array_equal(skeletonize(m.astype(bool)), ref)
    assert np.array_equal(skeletonize(m.astype(np.float32) * 0.25), ref)
    assert np.array_equal(skeletonize(np.asfortranarray(m)), ref)


def _multi_tube(shape=(256, 256, 192)):
    """Nine disjoint wiggling tubes of different radii along axis 0 and a free ring."""
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
    m |= ((rho - 14) ** 2 + (z - 96) ** 2) <= 9.0                     # a free ring: a tunnel to keep
    return m.astype(np.uint8)


@pytest.mark.gpu
def test_skeleton_large_phantom_properties():
    from arterynetwork_amd.skeletonization import skeletonize
    from arterynetwork_amd.generateVesselVolume import labelVolume
    m = _multi_tube()
    info = {}
    sk = skeletonize(m, info=info)
    print('256x256x192: voxels', int(m.sum()), '->', info['kept'], 'cycles', info['cycles'])
    assert sk.dtype == np.uint8 and set(np.unique(sk)) <= {0, 1} and sk.any()
    assert not (sk & ~m).any() and info['kept'] == int(sk.sum()) < m.sum() // 10
    lab_m, res_m = labelVolume(m)
    lab_s, res_s = labelVolume(sk)
    assert len(res_s) == len(res_m) == 11                                # background + 9 tubes + the ring
    inside = {}
    for ls, lm in zip(lab_s[sk != 0], lab_m[sk != 0]):
        inside.setdefault(int(ls), set()).add(int(lm))
    assert all(len(v) == 1 for v in inside.values()) and len(inside) == 10
    assert len({next(iter(v)) for v in inside.values()}) == 10           # ... and no two in the same one
    info2 = {}
    again = skeletonize(sk, info=info2)
    assert np.array_equal(again, sk) and info2['cycles'] == 1 and info2['kept'] == info['kept']
    assert skeletonize(m).tobytes() == sk.tobytes()


# ------------------------------------------------------------------ GPU: the layers
DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
rng = np.random.default_rng(21)
m = (rng.random((40, 36, 31)) < 0.45).astype(np.uint8)
m[5:30, 8:20, 6:25] = 1
dev = torch.device('cuda', 0)
host = S.skeletonize(m)
assert 0 < host.sum() < m.sum()
t = S.skeletonize(torch.as_tensor(m * 255, device=dev))
assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == m.shape and np.array_equal(t.cpu().numpy(), host)
# (a volume that starts at an odd device address)
flat = torch.zeros(m.size + 1, dtype=torch.uint8, device=dev)
odd = flat[1:].view(m.shape); odd.copy_(torch.as_tensor(m, device=dev))
assert odd.data_ptr() % 4 != 0 and np.array_equal(S.skeletonize(odd).cpu().numpy(), host)
co_h, r_h = S.skeletonRadii(host, m)
co_d, r_d = S.skeletonRadii(t, torch.as_tensor(m, device=dev))
assert np.array_equal(co_h, co_d) and np.array_equal(r_h, r_d)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_skeleton_device_resident():
    """A tensor on the GPU goes in by its device pointer and a uint8 tensor on the same device comes out, equal to the host
    call.  Own process: torch is imported before the HIP library there."""
    out = subprocess.run([sys.executable, '-c', DEVICE_RESIDENT_SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_skeleton_main_round_trip(tmp_path, capsys):
    from arterynetwork_amd import nifti, skeletonization as S
    m = _vessel(7, (48, 40, 32))
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    nifti.saveVolume(m, aff, str(tmp_path / 'vesselVolumeMask.nii.gz'))
    sk = S.main(str(tmp_path))
    path = os.path.join(str(tmp_path), 'skeleton.nii.gz')
    assert 'skeleton.nii.gz saved to {}.'.format(path) in capsys.readouterr().out
    out, aff2 = nifti.loadVolume(str(tmp_path), 'skeleton.nii.gz')
    assert out.dtype == np.uint8 and np.array_equal(out, sk) and np.allclose(aff2, aff)
    assert np.array_equal(sk, M.thin(m)[0])


@pytest.mark.gpu
def test_skeleton_radii():
    from arterynetwork_amd.skeletonization import skeletonize, skeletonRadii
    m = _vessel(3, (40, 36, 30))
    sk = skeletonize(m)
    coords, radii = skeletonRadii(sk, m)
    ref = MO.distance_transform_edt(m)
    assert coords.dtype == np.int64 and radii.dtype == np.float64 and len(coords) == int(sk.sum()) > 0
    assert np.array_equal(coords, np.argwhere(sk))
    assert np.array_equal(radii, ref[tuple(np.argwhere(sk).T)]) and (radii >= 1).all()


@pytest.mark.gpu
def test_skeleton_rejects_bad_shapes():
    from arterynetwork_amd import skeletonization as S
    from arterynetwork_amd._capi import VrgError
    with pytest.raises(ValueError):
        S.skeletonize(np.ones((8, 8), np.uint8))
    with pytest.raises(ValueError):
        S.skeletonize(np.ones((2, 3, 4, 5), np.uint8))
    # over the 32-bit envelope of vmask_label: refused before any voxel is touched (the buffers here are tiny)
    buf, out = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    dll = S._skeleton_lib()
    assert dll.vmask_skeleton(0, buf.ctypes.data, 2000, 2000, 600, out.ctypes.data, None, None) == -1      # VRG_E_ARG
    assert b'shape' in dll.vmask_last_error()
    with pytest.raises(VrgError):
        S._G._check(dll.vmask_skeleton(0, buf.ctypes.data, 40000, 2, 2, out.ctypes.data, None, None))
    assert dll.vmask_skeleton(0, None, 2, 2, 2, out.ctypes.data, None, None) == -1


# ------------------------------------------------------------------ no GPU needed: the kernels' resource records
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_skeleton_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vskel_device.hip' in build.SOURCES
    out = tmp_path / 'vskel_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vskel_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):
        f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, m.group(2)).group(1))
        recs[m.group(1)] = (f('private_segment_fixed_size'), f('vgpr_count'))
    for frag in ('10k_skel_pad', '11k_skel_mark', '11k_skel_step', '12k_skel_unpad'):
        hit = [v for k, v in recs.items() if frag in k]
        assert len(hit) == 1, 'kernel not found: ' + frag
        assert hit[0][0] == 0, '%s uses %d bytes of scratch per thread' % (frag, hit[0][0])
        assert hit[0][1] <= 64, '%s uses %d VGPRs (8 waves per SIMD need <= 64)' % (frag, hit[0][1])
