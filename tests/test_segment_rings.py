"""Segment tracing on closed curves, exact round counts and hash collisions ("f6 segment tracing").

On the CPU: the rings of tests/ring_family.py are what they claim to be; the parallel restatement tests/segment_rounds.py (link,
synchronous jump, the host loop, resolve, scatter) gives the segments of the sequential tests/segment_model.py on every ring in
every orientation, on the traced cases of test_segments and on random volumes, and each of four wrong lines in it is noticed;
the volumes of the hash test put their keys where the test says.  On the GPU: vmask_segments equals the sequential model
exactly and reports the restatement's number of rounds; the idx -> slot table of csrc/vseg_slots.h is driven into long probe
chains that wrap round its end, for vseg_device.hip and vbr_device.hip alike; free rings go through the branch graph and
morphometry with step counts known from their construction.  Every comparison is exact."""
import functools
import math
import os
import re

import numpy as np
import pytest

import branch_model as BM
import ring_family as RF
import segment_model as SM
import segment_rounds as SR
import test_branches as TB
import test_segments as TS
from conftest import ROOT

ALL_ORIENTATIONS = range(len(RF.ORIENTATIONS))
# test_segments.CASES with 20 000 object voxels or more (about 55 000 and 101 000): left to the sequential model alone
LARGE_CASES = {'random0.1-96x80x72', 'random0.3-260x260x5'}
ROUNDS_CASES = ('line-1x1x6000', 'ring-601x601x1', 'ring-tail-603x601x1', 'chains', 'eye')


# ------------------------------------------------------------------ CPU: the ring family
def _assert_one_ring(v, L):
    deg = SM.degrees(v)
    assert int(v.sum()) == L and (deg[v != 0] == 2).all()
    segs, counts = SM.trace(v)
    assert len(segs) == 1 and len(segs[0]) == L + 1 and segs[0][0] == segs[0][-1] == min(segs[0])
    assert counts == {'nodes': 0, 'isolated': 0, 'path': L}


def test_octagons_are_the_lengths_they_should_be():
    octs = RF.octagons()
    assert sorted(octs) == [8] + list(range(10, 31)) + [32]
    assert all(RF.closes(e) and sum(e) == L and 1 <= min(e) and max(e) <= 4 for L, e in octs.items())
    assert not RF.closes((1, 1, 1, 1, 1, 1, 1, 2)) and not RF.closes((1, 0, 1, 1, 1, 0, 1, 1))
    assert sorted({r.L for r in RF.family()}) == [3, 4, 5, 6, 7] + list(range(8, 31)) + [32]
    assert len(RF.family()) == len(RF.SMALL) + 2 * len(octs)


@pytest.mark.parametrize('ring', RF.family(), ids=lambda r: r.name)
def test_ring_family_is_sound(ring):
    """Every member: all voxels of degree 2 and one closed segment of L + 1 entries through the minimum - tight in its box, with a
    margin, and in all 48 orientations; a lifted ring is not planar, and the runs of steps describe the walk."""
    _assert_one_ring(ring.volume(), ring.L)
    _assert_one_ring(ring.volume(1), ring.L)
    images = set()
    for k in ALL_ORIENTATIONS:
        w = RF.orient(ring.volume(), k)
        assert w.flags['C_CONTIGUOUS'] and w.dtype == np.uint8
        _assert_one_ring(w, ring.L)
        assert w[tuple(RF.orient_coords(ring.points, ring.extent, k).T)].all()
        images.add((w.shape, w.tobytes()))
    assert len(images) >= 3                                              # (the ring of four voxels looks the same from both sides of each plane)
    assert sum(k for _, k in ring.steps) == ring.L and all(max(abs(c) for c in s) == 1 for s, _ in ring.steps)
    assert np.array_equal(np.sum([np.array(s) * k for s, k in ring.steps], axis=0), [0, 0, 0])
    if ring.lifted:
        assert min(ring.extent) > 1 and np.array_equal(ring.points[:, 2], ring.points[:, 0])
    if ring.e is not None:
        assert [k for _, k in ring.steps] == list(ring.e)


def test_orientations_move_the_minimum_and_turn_the_ring():
    """Over the 48 images of one octagon the voxel of smallest index is many different voxels of the ring, and its smaller
    neighbour is the next voxel of the walk in some images and the previous one in others."""
    ring = RF.octagon(RF.octagons()[11])
    at, forward = set(), set()
    for k in ALL_ORIENTATIONS:
        c = RF.orient_coords(ring.points, ring.extent, k)
        shape = RF.orient(ring.volume(), k).shape
        lin = np.ravel_multi_index(c.T, shape)
        m = int(np.argmin(lin))
        at.add(m)
        forward.add(bool(lin[(m + 1) % ring.L] < lin[(m - 1) % ring.L]))
    assert len(at) >= 6 and forward == {False, True}


@functools.lru_cache(maxsize=None)
def _packed(k):
    v = RF.packed(k)
    v.setflags(write=False)
    return v


def test_packed_volume_holds_what_it_should():
    items = RF.packed_items(0)
    kinds = [it[0] for it in items]
    n_rings = len(RF.SMALL) + len(RF.octagons())
    assert kinds.count('ring') == n_rings and kinds.count('chain') == len(RF.CHAIN_PATH_VOXELS) == 4 and kinds.count('lollipop') == 2
    v = _packed(0)
    assert v.size < 500_000 and int(v.sum()) == sum(len(it[3]) for it in items) < 2500
    deg = SM.degrees(v)
    for kind, name, ring, vox in items:
        d = deg[tuple(vox.T)]
        if kind == 'ring':
            assert (d == 2).all() and len(vox) == ring.L, name
            assert (name.endswith('-lifted')) == (ring.e is not None and ring.L % 2 == 1)
        elif kind == 'chain':
            assert d[0] == d[-1] == 1 and (d[1:-1] == 2).all() and len(vox) - 2 in RF.CHAIN_PATH_VOXELS
        else:                                                            # one node of degree 3 on the ring, a tail of TAIL voxels behind it
            L, at = ring
            assert sorted(d[:L].tolist()) == [2] * (L - 1) + [3] and d[L:].tolist() == [2] * (RF.TAIL - 1) + [1]
            ring_lin, node = np.ravel_multi_index(vox[:L].T, v.shape), int(np.argmax(d[:L]))
            assert (ring_lin[node] == ring_lin.min()) == name.endswith('minimum')
    for k in ALL_ORIENTATIONS:
        w = _packed(k)
        segs, counts = SM.trace(w)
        closed = [s for s in segs if s[0] == s[-1]]
        assert len(closed) == n_rings + 2 and len(segs) - len(closed) == 4 + 2
        assert counts['nodes'] == 2 * 4 + 2 * 2 and counts['isolated'] == 0
        assert sorted(len(s) - 1 for s in closed) == sorted([it[2].L for it in items if it[0] == 'ring'] + [sum(RF.LOLLIPOP_E)] * 2)
        assert sorted(len(s) - 2 for s in segs if s[0] != s[-1]) == sorted(list(RF.CHAIN_PATH_VOXELS) + [RF.TAIL - 1] * 2)
        for kind, name, ring, vox in RF.packed_items(k):
            assert w[tuple(vox.T)].all()


# ------------------------------------------------------------------ the small rings, alone and in the corners of a small volume
SMALL_ALONE = [(name, k) for name in ('ring3-plane', 'ring3-space', 'ring4') for k in (0, 8, 16, 24, 32, 40, 7, 47)]       # every axis order, two flips
# (ring, orientation, offset) in a 5 x 6 x 7 volume: seven corners and one face
CORNER_SHAPE = (5, 6, 7)
CORNERS = (('ring3-plane', 0, (0, 0, 0)), ('ring3-plane', 7, (3, 4, 6)), ('ring3-plane', 8, (0, 5, 0)), ('ring3-plane', 39, (4, 0, 5)),
           ('ring3-space', 1, (0, 0, 5)), ('ring3-plane', 6, (3, 4, 0)), ('ring3-plane', 2, (0, 4, 6)), ('ring4', 32, (4, 1, 1)))


def _small_alone(name, k):
    return RF.orient(RF.small(name).volume(), k)


@functools.lru_cache(maxsize=None)
def _corner_volume():
    v = np.zeros(CORNER_SHAPE, np.uint8)
    for name, k, at in CORNERS:
        w = RF.orient(RF.small(name).volume(), k)
        box = tuple(slice(a, a + s) for a, s in zip(at, w.shape))
        assert v[box].shape == w.shape and not (v[box] & w).any()
        v[box] |= w
    v.setflags(write=False)
    return v


def test_small_ring_volumes_are_sound():
    shapes = set()
    for name, k in SMALL_ALONE:
        w = _small_alone(name, k)
        _assert_one_ring(w, RF.small(name).L)
        shapes.add(w.shape)
    assert {(2, 2, 1), (2, 1, 2), (1, 2, 2), (2, 2, 2), (3, 3, 1), (3, 1, 3), (1, 3, 3)} <= shapes
    v = _corner_volume()
    segs, counts = SM.trace(v)
    assert (SM.degrees(v)[v != 0] == 2).all() and counts['nodes'] == 0
    assert sorted(len(s) for s in segs) == [4] * 7 + [5] and all(s[0] == s[-1] for s in segs)
    corners = [v[a, b, c] for a in (0, -1) for b in (0, -1) for c in (0, -1)]
    assert sum(int(x) for x in corners) == 7
    assert all(f.any() for f in (v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]))


# ------------------------------------------------------------------ CPU: the parallel model against the sequential one
@functools.lru_cache(maxsize=None)
def _rounds_of_case(case):
    """(segments equal the sequential model's, rounds) of a case of test_segments by the parallel model, computed once."""
    v = TS._volume(case)
    segs, rounds = SR.run(v)
    return segs == SM.trace(v)[0], rounds


@pytest.mark.parametrize('ring', RF.family(), ids=lambda r: r.name)
def test_parallel_model_equals_the_sequential_on_rings(ring):
    """All 48 orientations; a ring of L voxels alone takes ceil(log2 L) + 1 rounds wherever its minimum sits."""
    for k in ALL_ORIENTATIONS:
        w = RF.orient(ring.volume(), k)
        segs, rounds = SR.run(w)
        assert segs == SM.trace(w)[0], k
        assert rounds == math.ceil(math.log2(ring.L)) + 1, k


def test_parallel_model_equals_the_sequential_on_the_packed_volume():
    for k in ALL_ORIENTATIONS:
        segs, rounds = SR.run(_packed(k))
        assert segs == SM.trace(_packed(k))[0], k
        assert rounds == math.ceil(math.log2(max(RF.CHAIN_PATH_VOXELS))) == 9, k        # the longest chain decides; the rings settled long before
    for name, k in SMALL_ALONE:
        w = _small_alone(name, k)
        assert SR.run(w) == (SM.trace(w)[0], 3)
    assert SR.run(_corner_volume()) == (SM.trace(_corner_volume())[0], 3)


@pytest.mark.parametrize('case', sorted(set(TS.CASES) - LARGE_CASES))
def test_parallel_model_equals_the_sequential_on_the_traced_cases(case):
    assert TS._volume(case).sum() < 20000
    same, rounds = _rounds_of_case(case)
    print(case, 'rounds', rounds)
    assert same


def test_the_cases_left_out_are_the_large_ones():
    assert LARGE_CASES <= set(TS.CASES) and all(TS._volume(c).sum() >= 20000 for c in LARGE_CASES)


def test_parallel_model_equals_the_sequential_on_random_volumes():
    rng = np.random.default_rng(2024)
    closed = 0
    for _ in range(300):
        shape = tuple(int(s) for s in rng.integers(1, 9, 3))
        v = (rng.random(shape) < rng.uniform(0.05, 0.6)).astype(np.uint8)
        want = SM.trace(v)[0]
        assert SR.run(v)[0] == want, (shape, v.ravel().tolist())
        closed += sum(s[0] == s[-1] for s in want)
    assert closed > 0


MIXED = {3: 6, 60: 6, 64: 6, 65: 7, 300: 9}                             # path voxels of the chain -> rounds; the ring alone takes 6


@functools.lru_cache(maxsize=None)
def _ring_and_chain(P):
    """The octagon of 32 voxels and, two rows behind it, a straight chain of P path voxels."""
    ring = RF.octagon(RF.octagons()[32]).volume(1)[:, :, 1:2]
    v = np.zeros((ring.shape[0] + 2, max(ring.shape[1], P + 2), 1), np.uint8)
    v[:ring.shape[0], :ring.shape[1]] = ring
    v[-1, :P + 2, 0] = 1
    v.setflags(write=False)
    return v


def test_round_counts_of_chains_and_rings():
    """A straight chain of P path voxels takes ceil(log2 P) rounds (none for P = 1: nothing is open after the link), a ring of L
    voxels ceil(log2 L) + 1; in a mixed volume the slower of the two decides - the loop ends only when both tests say so."""
    for P in (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 420):
        assert SR.run(np.ones((1, 1, P + 2), np.uint8))[1] == math.ceil(math.log2(P))
    assert _rounds_of_case('line-1x1x6000')[1] == math.ceil(math.log2(5998)) == 13
    assert _rounds_of_case('ring-601x601x1')[1] == math.ceil(math.log2(1200)) + 1 == 12
    assert _rounds_of_case('ring-tail-603x601x1')[1] == math.ceil(math.log2(1199)) == 11        # the loop of 1199 path voxels is a chain from the node to itself
    for P, want in MIXED.items():                                        # the ring settles after the chain, with it, before it
        v = _ring_and_chain(P)
        segs, rounds = SR.run(v)
        assert segs == SM.trace(v)[0] and len(segs) == 2 and rounds == want == max(6, math.ceil(math.log2(P))), P


@pytest.mark.parametrize('mutation', SR.MUTATIONS)
def test_mutations_of_the_parallel_model_are_noticed(mutation):
    """<= for < when the successor's minimum is taken, the direction bit inverted in the ring branch of resolve, the unsettled
    minima counted before the jump, a ring's length without the + 1: each gives other segments or another number of rounds on
    the volumes that the GPU is compared on - the cases can tell the difference."""
    volumes = [('packed-0', _packed(0)), ('packed-29', _packed(29)), ('corners', _corner_volume())]
    volumes += [(r.name, r.volume()) for r in RF.family()] + [(c, TS._volume(c)) for c in ROUNDS_CASES]
    volumes += [('ring-and-chain-{}'.format(P), _ring_and_chain(P)) for P in MIXED]
    noticed = []
    for name, v in volumes:
        good, bad = SR.run(v), SR.run(v, mutation)
        assert good[0] == SM.trace(v)[0]
        if bad != good:
            noticed.append(name)
    print(mutation, 'noticed by', len(noticed), 'of', len(volumes), noticed[:8])
    assert noticed and any(n.startswith('packed') for n in noticed)      # the 48 GPU cases are images of the packed volume


# ------------------------------------------------------------------ CPU: the hash table's homes
def hash_bits(n):
    bits = 4
    while (1 << bits) < 2 * n:
        bits += 1
    return bits


def h_home(key, bits):
    return ((key * 2654435761) & 0xffffffff) >> (32 - bits)


def _fib_run():
    """A straight run of 60 voxels along axis 1 in a volume whose rows are 987 = F(16) voxels long."""
    v = np.zeros((1, 64, 987), np.uint8)
    v[0, 2:62, 788] = 1
    return v


def _fib_run_with_arms():
    """The same run with a perpendicular arm and a diagonal stub of two voxels each: junction clusters whose nodes and
    node-to-node edges are looked up as well.  64 object voxels: the table of 128 entries is exactly half full."""
    v = _fib_run()
    v[0, 30, 789:791] = 1
    v[0, 11, 787] = v[0, 12, 786] = 1
    return v


def _fib_plane_run():
    """Planes of 48 * 966 = 46368 = F(24) voxels: a run of 120 voxels along axis 0 through row 4, column 317."""
    v = np.zeros((124, 48, 966), np.uint8)
    v[2:122, 4, 317] = 1
    return v


# name -> (maker, object voxels, table bits, at most so many distinct homes, at least so many homes in the last two slots)
HASH_CASES = {'fib-987-run': (_fib_run, 60, 7, 8, 30), 'fib-987-run-arms': (_fib_run_with_arms, 64, 7, 12, 30),
              'fib-46368-planes': (_fib_plane_run, 120, 8, 11, 60)}


@functools.lru_cache(maxsize=None)
def _hash_volume(case):
    v = HASH_CASES[case][0]()
    v.setflags(write=False)
    return v


def test_hash_restatement_is_the_headers():
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vseg_slots.h')).read()
    assert re.search(r'h_home\(const Hash& h, uint32_t key\) \{ return \(key \* 2654435761u\) >> h\.shift; \}', src)
    assert re.search(r'int bits = 4;\s*while \(\(1ull << bits\) < 2ull \* n\) bits\+\+;', src)
    for name in ('vseg_device.hip', 'vbr_device.hip'):
        text = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', name)).read()
        assert '#include "vseg_slots.h"' in text and 'hash_bits(n)' in text and '32u - (uint32_t)' in text


@pytest.mark.parametrize('case', sorted(HASH_CASES))
def test_hash_volumes_collide_and_wrap(case):
    """The keys of each volume have a handful of home slots, most of them in the table's last two: whatever the order of
    insertion, all but a few entries are displaced, and past the table's end."""
    _, n, bits, max_homes, min_last = HASH_CASES[case]
    v = _hash_volume(case)
    keys = np.flatnonzero(v.ravel()).tolist()
    homes = [h_home(k, bits) for k in keys]
    last = sum(h >= (1 << bits) - 2 for h in homes)
    print(case, 'n', len(keys), 'table', 1 << bits, 'homes', sorted(set(homes)), 'in the last two slots', last)
    assert len(keys) == n and hash_bits(n) == bits and v.size < 10 ** 7
    assert len(set(homes)) <= max_homes and last >= min_last
    assert last - 2 >= 28                                # more entries than the two slots hold: the rest wrap to slot 0 and on
    if case == 'fib-987-run':
        assert len(set(homes)) == 5 and last == 35                       # 5 homes for 60 keys
    if case == 'fib-46368-planes':
        assert len(set(homes)) * 10 < n and min(homes) >= (1 << bits) - 4 and len(set(homes)) == 4 and last == 77
    assert int((SM.degrees(v) >= 3).sum()) == (0 if case != 'fib-987-run-arms' else 8)


# ------------------------------------------------------------------ GPU: exactly the models
@functools.lru_cache(maxsize=None)
def _models(kind, key):
    """(offsets, coords, counts, rounds) - the sequential model's arrays and the parallel model's rounds, once per volume."""
    v = _volume_of(kind, key)
    off, co, counts = SM.arrays(v)
    off.setflags(write=False); co.setflags(write=False)
    return off, co, counts, SR.run(v)[1]


def _volume_of(kind, key):
    if kind == 'packed':
        return _packed(key)
    if kind == 'ring':
        return RF.family()[key].volume()
    if kind == 'alone':
        return _small_alone(*key)
    if kind == 'corners':
        return _corner_volume()
    if kind == 'hash':
        return _hash_volume(key)
    if kind == 'mixed':
        return _ring_and_chain(key)
    return TS._volume(key)


def _assert_gpu_equals_the_models(kind, key, rounds=True):
    from arterynetwork_amd.skeletonization import segmentArrays
    v = _volume_of(kind, key)
    assert v.sum() < 2.2e5 and v.size < 10 ** 7
    off, co, counts, want_rounds = _models(kind, key)
    info = {}
    g_off, g_co = segmentArrays(v, info=info)
    print(kind, key, 'shape', v.shape, 'voxels', int(v.sum()), 'segments', info['segments'], 'rounds: GPU', info['rounds'], 'model', want_rounds)
    assert g_off.dtype == np.int64 and g_co.dtype == np.int64 and g_co.shape == (int(off[-1]), 3)
    assert np.array_equal(g_off, off) and np.array_equal(g_co, co)
    assert info['segments'] == len(off) - 1 and info['nodes'] == counts['nodes'] and info['isolated'] == counts['isolated']
    if rounds:
        assert info['rounds'] == want_rounds
    return info


@pytest.mark.gpu
@pytest.mark.parametrize('orientation', ALL_ORIENTATIONS)
def test_rings_equal_the_model(orientation):
    _assert_gpu_equals_the_models('packed', orientation)


@pytest.mark.gpu
def test_each_ring_alone():
    """Every member of the family in a volume of its own: the segments, and the rounds of a ring of its length."""
    for key, ring in enumerate(RF.family()):
        print(ring.name, 'L', ring.L, end=': ')
        info = _assert_gpu_equals_the_models('ring', key)
        assert info['segments'] == 1 and info['rounds'] == math.ceil(math.log2(ring.L)) + 1


@pytest.mark.gpu
def test_small_rings():
    for key in SMALL_ALONE:
        assert _assert_gpu_equals_the_models('alone', key)['segments'] == 1
    assert _assert_gpu_equals_the_models('corners', None)['segments'] == len(CORNERS)


@pytest.mark.gpu
@pytest.mark.parametrize('P', sorted(MIXED))
def test_ring_and_chain_settle_in_either_order(P):
    """Both ways through the host loop's two tests: the chain closes while the ring's windows have not lapped it yet, and the ring
    knows its minimum while the chain is still open."""
    assert _assert_gpu_equals_the_models('mixed', P)['rounds'] == MIXED[P]


@pytest.mark.gpu
@pytest.mark.parametrize('case', ROUNDS_CASES)
def test_rounds_are_the_models(case):
    assert _rounds_of_case(case)[0]
    _assert_gpu_equals_the_models('case', case)


@functools.lru_cache(maxsize=None)
def _branch_model(kind, key):
    sk, g = BM.branch_graph(_volume_of(kind, key), **TB.NO_PRUNE)
    for a in (sk, g.nodes, g.ends, g.offsets, g.voxels):
        a.setflags(write=False)
    return sk, g


def _assert_branches_equal_the_model(kind, key):
    from arterynetwork_amd.skeletonization import branchGraph
    v = _volume_of(kind, key)
    got = branchGraph(v)
    sk, g = _branch_model(kind, key)
    TB._assert_equal_to_model(got, sk, g, v.shape)
    return got, g


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(HASH_CASES))
def test_hash_collisions_and_wrap(case):
    """What test_hash_volumes_collide_and_wrap shows about the keys, the kernels have to live with: segment tracing and the branch
    graph (the same table, built by vbr_device.hip) equal their models."""
    _assert_gpu_equals_the_models('hash', case)
    got, g = _assert_branches_equal_the_model('hash', case)
    print(case, got.counts)
    assert got.counts['branches'] == (1 if case != 'fib-987-run-arms' else 5)


@pytest.mark.gpu
@pytest.mark.parametrize('orientation', [0, 21, 46])
def test_rings_through_the_branch_graph_and_morphometry(orientation):
    """The packed volume's free rings are branches without nodes; their step counts by class follow from the sides of each ring and
    the orientation alone, and the path length is pathLengths of the integer outputs, to the bit."""
    from arterynetwork_amd.skeletonization import branchMorphometry, pathLengths
    v = _packed(orientation)
    got, g = _assert_branches_equal_the_model('packed', orientation)
    spacing = (0.5, 0.7, 1.3)
    mor = branchMorphometry(got, dist=np.ones(v.shape), spacing=spacing)
    first = {int(np.ravel_multi_index(tuple(got.coords[a]), v.shape)): b for b, a in enumerate(got.offsets[:-1].tolist())
             if got.branchEnds[b].tolist() == [-1, -1]}
    rings = [(ring, vox) for kind, _, ring, vox in RF.packed_items(orientation) if kind == 'ring']
    assert len(first) == len(rings) == int((got.branchEnds[:, 0] < 0).sum()) == len(RF.SMALL) + len(RF.octagons())
    for ring, vox in rings:
        b = first[int(np.ravel_multi_index(vox.T, v.shape).min())]
        assert got.offsets[b + 1] - got.offsets[b] == ring.L + 1 and np.array_equal(got.coords[got.offsets[b]], got.coords[got.offsets[b + 1] - 1])
        assert mor.stepCounts[b].tolist() == RF.expected_step_counts(ring, orientation), ring.name
        assert mor.jumps[b] == 0 and not mor.jumpOffset[b].any() and not mor.chord[b].any()
    assert mor.stepCounts.sum() == len(got.coords) - len(got.offsets) + 1 - int(mor.jumps.sum())
    assert np.array_equal(mor.pathLength, pathLengths(mor.stepCounts, mor.jumpOffset, spacing))
