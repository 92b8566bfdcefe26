"""Curve skeleton: the sequential model tests/skeleton_model.py is checked for soundness on the
CPU, its predicate and the kernel's (csrc/vskel_simple.h) are compared with the definition - the kernel's on every one of the
2^26 neighbourhoods - then the GPU thinning (vmask_skeleton / skeletonization.skeletonize) must equal it bit for bit."""
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


# ------------------------------------------------------------------ CPU: the thinning predicate, every neighbourhood
# A stand-alone host program: csrc/vskel_simple.h's `deletable` (the code k_skel_step runs) against a plain restatement of the
# definition - explicit 3x3x3 arrays and a stack, nothing shared with the header - on all 2^26 settings of the 26 neighbours.
# argv: a file of 27-bit words (uint32, centre bit clear), and where to write the plain predicate's answers for them (one byte each:
# bit 0 simple, bit 1 end point).
SIMPLE_PROGRAM = r"""
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>
#include "vskel_simple.h"

namespace plain {
struct Cell { int a, b, c; };

// near[l1][a][b][c]: the cells of the 3x3x3 block one step from (a, b, c), a step changing every coordinate by at most 1 and at most
// l1 of them (l1 = 1: 6-connected, l1 = 3: 26-connected); built once, by the loops that define it
struct Near { Cell to[26]; int n; };
static Near near[4][3][3][3];
static void build_near() {
    for (int l1 = 1; l1 <= 3; l1++)
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 3; c++) {
            Near& q = near[l1][a][b][c];
            q.n = 0;
            for (int da = -1; da <= 1; da++) for (int db = -1; db <= 1; db++) for (int dc = -1; dc <= 1; dc++) {
                const int d = (da != 0) + (db != 0) + (dc != 0);
                if (d == 0 || d > l1) continue;
                const int x = a + da, y = b + db, z = c + dc;
                if (x < 0 || x > 2 || y < 0 || y > 2 || z < 0 || z > 2) continue;
                q.to[q.n++] = Cell{x, y, z};
            }
        }
}

// marks in `seen` the cells of `in` (3x3x3, 0/1) that such steps inside `in` reach from `from`, and returns how many they are
static int flood(const int in[3][3][3], Cell from, int l1, int seen[3][3][3]) {
    Cell stack[27];
    int top = 0, n = 0;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 3; c++) seen[a][b][c] = 0;
    seen[from.a][from.b][from.c] = 1;
    stack[top++] = from;
    while (top) {
        const Cell p = stack[--top];
        n++;
        const Near& q = near[l1][p.a][p.b][p.c];
        for (int k = 0; k < q.n; k++) {
            const Cell t = q.to[k];
            if (!in[t.a][t.b][t.c] || seen[t.a][t.b][t.c]) continue;
            seen[t.a][t.b][t.c] = 1;
            stack[top++] = t;
        }
    }
    return n;
}

// bit 0: the centre is simple; bit 1: it is an end point
static int judge(uint32_t word) {
    int obj[3][3][3], bg18[3][3][3], seen[3][3][3];
    int count = 0, nbg = 0;
    Cell first_obj{-1, -1, -1}, first_face{-1, -1, -1};
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 3; c++) {
        const int off = (a != 1) + (b != 1) + (c != 1);              // 0: the centre, 1: a face, 2: an edge, 3: a corner neighbour
        const int bit = (int)((word >> (a * 9 + b * 3 + c)) & 1u);
        obj[a][b][c] = off != 0 && bit;
        bg18[a][b][c] = (off == 1 || off == 2) && !bit;
        if (obj[a][b][c]) { if (!count) first_obj = Cell{a, b, c}; count++; }
        if (off == 1 && !bit) { if (!nbg) first_face = Cell{a, b, c}; nbg++; }
    }
    const int end_point = count == 1 ? 2 : 0;
    if (count == 0) return end_point;                               // an isolated voxel: no object component at all
    if (flood(obj, first_obj, 3, seen) != count) return end_point;  // more than one 26-component of the object
    if (nbg == 0) return end_point;                                 // no background face neighbour: an interior voxel
    flood(bg18, first_face, 1, seen);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) for (int c = 0; c < 3; c++)
        if ((a != 1) + (b != 1) + (c != 1) == 1 && bg18[a][b][c] && !seen[a][b][c]) return end_point;
    return end_point | 1;
}
}  // namespace plain

static uint32_t word_of(uint32_t n) { return (n & 0x1fffu) | ((n >> 13) << 14); }   // the 26 neighbour bits around a clear centre bit

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    plain::build_near();
    const uint32_t total = 1u << 26;
    unsigned T = std::thread::hardware_concurrency();
    T = std::max(1u, std::min(16u, T));                             // never more than 16, whatever the machine reports
    std::vector<unsigned long long> differ(T, 0), del(T, 0), simple(T, 0);
    std::vector<std::vector<uint32_t>> firsts(T);
    std::atomic<uint32_t> next{0};
    const uint32_t piece = 1u << 16;
    auto work = [&](unsigned t) {
        for (;;) {
            const uint32_t lo = next.fetch_add(piece);
            if (lo >= total) break;
            for (uint32_t n = lo; n < lo + piece; n++) {
                const uint32_t w = word_of(n);
                const int j = plain::judge(w);
                const bool want = j == 1, got = deletable(w);
                simple[t] += (unsigned long long)(j & 1);
                del[t] += got ? 1u : 0u;
                if (want != got) { if (firsts[t].size() < 5) firsts[t].push_back(w); differ[t]++; }
            }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < T; t++) pool.emplace_back(work, t);
    for (auto& th : pool) th.join();
    unsigned long long d = 0, k = 0, s = 0;
    for (unsigned t = 0; t < T; t++) {
        d += differ[t]; k += del[t]; s += simple[t];
        for (uint32_t w : firsts[t]) std::printf("differs at %#x: plain %d, header %d\n", (unsigned)w, plain::judge(w), (int)deletable(w));
    }
    std::printf("threads %u\nchecked %u\ndiffer %llu\ndeletable %llu\nsimple %llu\n", T, (unsigned)total, d, k, s);

    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = in ? std::fopen(argv[2], "wb") : nullptr;
    if (!out) return 3;
    uint32_t w;
    unsigned long listed = 0;
    while (std::fread(&w, sizeof w, 1, in) == 1) {
        if (w >> 27 || (w & N_CENTRE)) return 4;
        std::fputc(plain::judge(w), out);
        listed++;
    }
    std::fclose(in);
    if (std::fclose(out)) return 3;
    std::printf("listed %lu\n", listed);
    return d ? 1 : 0;
}
"""

N_DELETABLE = 25985118           # simple and not an end point, of the 2^26 neighbourhoods
N_SIMPLE = 25985144              # the published number of 26-simple points; the 26 more are the one-neighbour end points


def _sample_words():
    """27-bit words (bit a*9 + b*3 + c, centre clear): 20 000 from a seeded generator, and every word with at most 2 or at least
    24 object neighbours - the 6 + 12 + 8 single-neighbour words among them."""
    places = [b for b in range(27) if b != 13]
    few = [0] + [1 << a for a in places] + [(1 << a) | (1 << b) for i, a in enumerate(places) for b in places[i + 1:]]
    everything = sum(1 << a for a in places)
    rng = np.random.default_rng(26)
    drawn = rng.integers(0, 1 << 26, 20000, dtype=np.uint64)
    drawn = (drawn & np.uint64(0x1fff)) | ((drawn >> np.uint64(13)) << np.uint64(14))
    words = np.concatenate((drawn.astype(np.uint32), np.array(few, np.uint32), np.array([everything ^ f for f in few], np.uint32)))
    assert len(words) == 20000 + 2 * (1 + 26 + 325) and not (words & (1 << 13)).any()
    return words


@functools.lru_cache(maxsize=None)
def _enumeration():
    """Compiles and runs SIMPLE_PROGRAM once; -> (return code, its output, the sample words, the plain answers for them)."""
    import tempfile
    cxx = os.environ.get('CXX', 'g++')
    words = _sample_words()
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, listed, answers = (os.path.join(tmp, f) for f in ('simple.cpp', 'simple', 'words.bin', 'answers.bin'))
        open(src, 'w').write(SIMPLE_PROGRAM)
        words.tofile(listed)
        p = subprocess.run([cxx, '-O2', '-std=c++17', '-pthread', '-I', os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), '-o', exe, src], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        r = subprocess.run([exe, listed, answers], capture_output=True, text=True)
        got = np.fromfile(answers, np.uint8) if os.path.exists(answers) else np.zeros(0, np.uint8)
    return r.returncode, r.stdout, words, got


def test_deletable_is_the_definition_on_every_neighbourhood():
    """All 2^26 neighbourhoods, none sampled: `deletable` of csrc/vskel_simple.h - the shift-and-mask flood fills that k_skel_step
    runs - against the definition written out with 3x3x3 arrays and a stack (SIMPLE_PROGRAM): at least 2 object neighbours, one
    26-component of them, a background face neighbour, and every background face neighbour in one 6-component inside N18*.
    0 may differ; 25 985 118 are deletable, and the plain predicate finds the published 25 985 144 simple points.
    Wall time, compile included: 13 s on 8 threads when this was written, 94 s of processor time in all (the program starts as many
    threads as the machine has processors, 16 at the most); the plain predicate, about 1.3 microseconds a word, is what takes it."""
    rc, out, words, _ = _enumeration()
    print(out[-3000:])
    fields = dict(line.split() for line in out.splitlines() if len(line.split()) == 2)
    assert 1 <= int(fields['threads']) <= 16
    assert int(fields['checked']) == 1 << 26
    assert int(fields['differ']) == 0 and 'differs at' not in out and rc == 0, out[-3000:]
    assert int(fields['deletable']) == N_DELETABLE
    assert int(fields['simple']) == N_SIMPLE and N_SIMPLE - N_DELETABLE == 26
    assert int(fields['listed']) == len(words)


def test_model_predicate_is_the_definition_on_a_fixed_sample():
    """skeleton_model.is_simple / is_end_point - what the GPU tests compare the thinning with - against the same plain predicate, on
    20 000 seeded words, every word with at most 2 or at least 24 object neighbours, the 26 single-neighbour words: none left out."""
    rc, out, words, plain = _enumeration()
    assert rc == 0 and len(plain) == len(words), out[-3000:]
    ends = 0
    for w, j in zip(words.tolist(), plain.tolist()):
        block = np.array([(w >> b) & 1 for b in range(27)], bool).reshape(3, 3, 3)
        assert (bool(M.is_simple(block)), bool(M.is_end_point(block))) == (bool(j & 1), bool(j & 2)), hex(w)
        block[1, 1, 1] = True                                  # the centre's own value is ignored
        assert (bool(M.is_simple(block)), bool(M.is_end_point(block))) == (bool(j & 1), bool(j & 2)), hex(w)
        ends += j == 3
    assert ends == 26                                          # a voxel with one neighbour is simple, and an end point
    assert 0.3 < np.mean(plain[:20000] == 1) < 0.5             # about 25 985 118 / 2^26 = 0.387 of the drawn words are deletable


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
