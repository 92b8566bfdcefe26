"""Minimal-cost bridges between vessel fragments ("f19 bridges"): the numpy model tests/bridge_model.py is
checked on the CPU against a heap Dijkstra, then vmask_bridge / reconnect.bridgeCandidates must equal it exactly - the bits of
dist, root, pred, pairs, costs, offsets, voxels and counts[0..6] - on shapes off the brick grid, under ties, at the bound,
across brick seams, through long corridors and with thousands of pairs, with storage on a fraction of a non-cubic brick grid, a
pair table whose probes wrap and a result beyond the first call's capacity; then the recovery phantom and the file-level driver."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bridge_model as BM
from conftest import ROOT
from arterynetwork_amd import reconnect as R

E_ARG = -1


# ------------------------------------------------------------------ inputs
def _lin(shape, p):
    return int(np.ravel_multi_index(tuple(p), shape))


def _points(shape, pts):
    m = np.zeros(shape, np.uint8)
    for p in pts:
        m[tuple(p)] = 1
    return m


def _blobs(shape, seed):
    """Random blobs, random cost in [0.5, 4], a 0.9-dense random domain, random tips."""
    rng = np.random.default_rng(seed)
    seeds = rng.random(shape) < 0.02
    grow = seeds & (rng.random(shape) < 0.5)
    mask = seeds | BM.shifted(grow, (0, 0, -1), False) | BM.shifted(grow & (rng.random(shape) < 0.5), (0, -1, 1), False)
    return mask.astype(np.uint8), rng.uniform(0.5, 4.0, shape), (rng.random(shape) < 0.9).astype(np.uint8), (rng.random(shape) < 0.5).astype(np.uint8)


def _serpentine(n):
    """A one-voxel-wide corridor through an n x n x n volume: runs along axis 2 in every second row of every second plane,
    joined at alternating ends.  Returns the corridor (uint8) and its voxels in order."""
    order = []
    flip = False
    for a in range(0, n, 2):
        rows = list(range(0, n, 2))
        if (a // 2) % 2:
            rows = rows[::-1]
        for k, b in enumerate(rows):
            run = [(a, b, c) for c in range(n)]
            order += run[::-1] if flip else run
            flip = not flip
            if k + 1 < len(rows):
                order.append((a, (b + rows[k + 1]) // 2, order[-1][2]))
        if a + 2 < n:
            order.append((a + 1, rows[-1], order[-1][2]))
    return _points((n, n, n), order), order


def phantom(g):
    """The recovery phantom: tube 1 along axis 2 at (8, 8), radius 1.5, missing for z in [18, 18 + g); tube 2 parallel at
    (8, 16) for 4 < z < 36; vesselness max(exp(-r1^2 / 4), exp(-r2^2 / 4)) (0.6 + 0.4 noise)."""
    shape = (20, 24, 40)
    i0, i1, i2 = np.indices(shape)
    r1, r2 = (i0 - 8) ** 2 + (i1 - 8) ** 2, (i0 - 8) ** 2 + (i1 - 16) ** 2
    t1 = (r1 <= 2.25) & ~((i2 >= 18) & (i2 < 18 + g))
    t2 = (r2 <= 2.25) & (i2 > 4) & (i2 < 36)
    v = np.maximum(np.exp(-r1 / 4.0), np.exp(-r2 / 4.0)) * (0.6 + 0.4 * np.random.default_rng(1).random(shape))
    return (t1 | t2).astype(np.uint8), v


# ------------------------------------------------------------------ device against model
def _run(mask, cost, domain=None, tips=None, spacing=None, max_cost=16.0, tip_rule=1):
    info = {}
    b = R.bridgeCandidates(mask, cost, domain=domain, tips=tips, maxCost=max_cost, tipRule=tip_rule, spacing=spacing, info=info, return_fields=True)
    return b, info


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def _same(b, info, ref):
    assert [info[k] for k in R.COUNT_KEYS[:7]] == ref.counts.tolist()
    assert np.array_equal(_host(b.comp), ref.comp)
    assert np.array_equal(_bits(_host(b.dist)), _bits(ref.dist))
    assert np.array_equal(_host(b.root), ref.root)
    assert np.array_equal(_host(b.pred), ref.pred)
    assert np.array_equal(np.hstack((b.pairs, b.ends, b.roots)), ref.pairs)
    assert np.array_equal(_bits(b.cost), _bits(ref.costs))
    assert np.array_equal(b.offsets, ref.offsets)
    assert np.array_equal(b.voxels, ref.voxels)
    assert b.ncomp == ref.counts[0]


def _check(mask, cost, domain=None, tips=None, spacing=None, max_cost=16.0, tip_rule=1):
    b, info = _run(mask, cost, domain, tips, spacing, max_cost, tip_rule)
    ref = BM.model(mask, cost, domain, tips, spacing, max_cost, tip_rule)
    _same(b, info, ref)
    return b, info, ref


def _adjacent(b):
    for i in range(len(b)):
        p = b.path(i)
        assert np.abs(np.diff(p, axis=0)).max() == 1


# ------------------------------------------------------------------ CPU: the model, the host-only layer
@pytest.mark.parametrize('trial', range(8))
def test_model_equals_dijkstra(trial):
    """Integer costs and unit spacing give ties everywhere; random ones none.  D, Root and Pred agree bit for bit."""
    rng = np.random.default_rng(100 + trial)
    shape = [(5, 6, 7), (1, 9, 9), (4, 4, 11), (6, 6, 6)][trial % 4]
    mask = (rng.random(shape) < 0.06).astype(np.uint8)
    dom = (rng.random(shape) < 0.85).astype(np.uint8)
    ties = trial % 2 == 1
    cost = rng.integers(1, 3, shape).astype(np.float64) if ties else rng.uniform(0.5, 4.0, shape)
    spacing = None if ties else (0.5, 0.5, 0.8)
    r = BM.model(mask, cost, dom, None, spacing, max_cost=9.0, tip_rule=0)
    d, root, pred = BM.dijkstra(mask, cost, dom, spacing, 9.0)
    assert np.array_equal(_bits(d), _bits(r.dist)) and np.array_equal(root, r.root) and np.array_equal(pred, r.pred)
    assert r.counts[2] > 0
    for i in range(len(r.costs)):                                      # a path runs from the mask voxel Root(u) to Root(v)
        p = r.voxels[r.offsets[i]:r.offsets[i + 1]]
        assert p[0] == r.pairs[i, 4] and p[-1] == r.pairs[i, 5] and mask.reshape(-1)[p[0]] and mask.reshape(-1)[p[-1]]
        assert not mask.reshape(-1)[p[1:-1]].any()


def _table(rows):
    pairs = np.array([r[:2] for r in rows], np.int64).reshape(-1, 2)
    cost = np.array([r[2] for r in rows], np.float64)
    z = np.zeros((len(rows), 2), np.int64)
    return R.Bridges(pairs, z, z, cost, np.zeros(len(rows) + 1, np.int64), np.zeros(0, np.int64), 9, (1, 1, 1))


def test_select_bridges():
    tri = _table([(1, 2, 3.0), (1, 3, 1.0), (2, 3, 2.0)])
    assert R.selectBridges(tri).tolist() == [1, 2]                     # the two cheapest of a triangle
    assert R.selectBridges(tri, forest=False).tolist() == [0, 1, 2]
    tie = _table([(2, 3, 1.0), (1, 3, 1.0), (1, 2, 1.0)])
    assert R.selectBridges(tie).tolist() == [1, 2]                     # equal costs go by (a, b): (1, 2), (1, 3)
    two = _table([(1, 2, 5.0), (3, 4, 1.0), (2, 3, 2.0), (1, 4, 3.0), (5, 6, 9.0)])
    assert R.selectBridges(two).tolist() == [1, 2, 3, 4]
    assert R.selectBridges(_table([])).tolist() == []


def test_python_argument_checks():
    m = np.zeros((3, 4, 5), np.uint8)
    c = np.ones((3, 4, 5))
    for kw in (dict(maxCost=0.0), dict(maxCost=float('nan')), dict(maxCost=float('inf')), dict(tipRule=3), dict(tipRule=-1), dict(spacing=(1, 1)),
               dict(domain=np.ones((3, 4, 6), np.uint8)), dict(tips=np.ones((3, 4), np.uint8))):
        with pytest.raises(ValueError):
            R.bridgeCandidates(m, c, **kw)
    with pytest.raises(ValueError):
        R.bridgeCandidates(m, np.ones((3, 4, 6)))
    with pytest.raises(ValueError):
        R.bridgeCandidates(np.zeros((3, 4), np.uint8), np.ones((3, 4)))
    for bad in (dict(floor=0.0), dict(floor=float('nan')), dict(brainVolumeMask=np.ones((3, 4, 6)))):
        with pytest.raises(ValueError):
            R.vesselCost(c, **bad)
    with pytest.raises(ValueError):
        R.vesselCost(-c)
    v = np.zeros((2, 2, 2))
    v[0, 0, 0], v[1, 1, 1] = 2.0, 1.0
    cost = R.vesselCost(v, floor=0.25)
    assert cost.dtype == np.float64 and cost[0, 0, 0] == 1.0 / 1.25 and cost[1, 1, 1] == 1.0 / 0.75 and cost[0, 0, 1] == 4.0
    assert R.vesselCost(v, floor=0.25, brainVolumeMask=(v == 1.0))[0, 0, 0] == 4.0
    empty = _table([])
    with pytest.raises(ValueError):
        R.applyBridges(np.zeros((2, 2, 2), np.uint8), empty, [])       # another shape
    with pytest.raises(ValueError):
        R.applyBridges(np.zeros((1, 1, 1), np.uint8), empty, [0])      # no such bridge
    with pytest.raises(ValueError):
        R.applyBridges(np.zeros((1, 1, 1), np.uint8), empty, [], thicken=-1)
    with pytest.raises(ValueError):
        R.tipRegions(m, reach=-1.0)


# ------------------------------------------------------------------ CPU: what the sparse, wrapped and resized cases rest on
# Storage on the 5 x 3 x 9 brick grid of a 40 x 24 x 72 volume.  name: mask points, max_cost, spacing, float32 cost, domain with
# two empty slabs, then what the header's rule gives: reach, bricks with storage, bricks that hold a domain voxel
SPARSE_SHAPE = (40, 24, 72)
SPARSE = {
    'interior': ([(17, 9, 30), (17, 9, 35)], 6.0, None, False, False, (1, 36, 135)),
    'interior_float32': ([(17, 9, 30), (17, 9, 35)], 6.0, None, True, False, (1, 36, 135)),
    'reach_2': ([(17, 9, 30), (17, 9, 38)], 9.5, None, False, False, (2, 90, 135)),
    'volume_corners': ([(0, 0, 0), (3, 2, 4), (39, 23, 71), (36, 21, 68)], 6.0, None, False, False, (1, 16, 135)),
    'brick_corner_seam': ([(23, 15, 39), (24, 16, 43), (23, 15, 47)], 6.0, None, False, False, (1, 42, 135)),
    'empty_domain_bricks': ([(17, 9, 30), (17, 9, 35), (20, 4, 33)], 6.0, None, False, True, (1, 22, 104)),
    'anisotropic': ([(17, 9, 30), (17, 9, 42), (18, 11, 31)], 2.5, (2.0, 1.0, 0.25), False, False, (2, 105, 135)),
}


@functools.lru_cache(maxsize=None)
def _sparse(name):
    """The inputs of one case, the model's result and the header's storage rule (BM.expected_bricks); tip_rule 0."""
    pts, max_cost, spacing, f32, cut, _ = SPARSE[name]
    cost = np.random.default_rng(21).uniform(0.5, 1.0, SPARSE_SHAPE)
    if f32:
        cost = cost.astype(np.float32)
    dom = None
    if cut:
        dom = np.ones(SPARSE_SHAPE, np.uint8)
        dom[8:16] = 0                                                  # brick plane 1 of axis 0
        dom[:, 16:24, 24:32] = 0                                       # and the bricks (., 2, 3)
    mask = _points(SPARSE_SHAPE, pts)
    ref = BM.model(mask, cost, dom, None, spacing, max_cost, 0)
    stored, facts = BM.expected_bricks(mask, cost, dom, spacing, max_cost)
    return mask, cost, dom, spacing, max_cost, ref, stored, facts


@pytest.mark.parametrize('name', list(SPARSE))
def test_sparse_cases_are_sparse_and_sufficient(name):
    """Before any device runs: the rule leaves domain bricks without storage (else the case tests nothing), its floor and ceil
    are a margin away from where rounding could move them, and no brick that the model uses - one with a mask voxel or a reached
    one - is left out."""
    mask, cost, dom, spacing, max_cost, ref, stored, facts = _sparse(name)
    reach, nstored, ndomain = SPARSE[name][5]
    assert abs(facts['ratio'] - round(facts['ratio'])) >= 0.005 and facts['steps'] not in (8, 9, 16, 17)
    assert stored.shape == (5, 3, 9) and facts['reach'] == reach
    assert int(stored.sum()) < facts['domain_bricks']
    assert (int(stored.sum()), facts['domain_bricks']) == (nstored, ndomain)
    used = BM.brick_any((ref.dist >= 0.0) & np.isfinite(ref.dist))     # D = 0 in the mask, finite where reached
    assert used.any() and not (used & ~stored).any()
    if name == 'interior':
        assert not stored[0, 0, 0] and ref.dist[2, 2, 2] == np.inf and ref.root[2, 2, 2] == -1 and ref.pred[2, 2, 2] == 255
    if name == 'reach_2':                                              # axis 0: all 5, axis 1: its 3 (the clamp bites), axis 2: 6 of 9
        assert [int(stored.any(axis=ax).sum()) for ax in ((1, 2), (0, 2), (0, 1))] == [5, 3, 6]
    if name == 'volume_corners':                                       # clamped at both ends of every axis
        assert stored[0, 0, 0] and stored[4, 2, 8] and stored[1, 1, 1] and stored[3, 1, 7] and not stored[2].any()
    if name == 'brick_corner_seam':
        assert ref.counts[5] == 2 and ref.counts[3] == 605 and int(used.sum()) == 12
    if name == 'empty_domain_bricks':                                  # bricks within reach that hold no domain voxel get no slot
        whole, wfacts = BM.expected_bricks(mask, cost, None, spacing, max_cost)
        assert wfacts['reach'] == reach and int((whole & ~stored).sum()) == 36 - 22 and ref.counts[5] == 3
    if name == 'anisotropic':                                          # the lightest edge runs along axis 2
        assert int(np.argmin(BM.half_weights(spacing))) in (12, 13) and ref.counts[4] == 3 and ref.counts[5] == 2


def _pair_table_source():
    """The pair table's hash and its smallest size, read from the kernel source: hash(key, bits), the minimum of bits."""
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vbridge_device.hip')).read()
    mo = re.search(r'hash_of\(u64 key, uint32_t bits\) \{ return \(uint32_t\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> \((\d+)u - bits\)\); \}', src)
    mult, width = int(mo.group(1), 16), int(mo.group(2))
    assert width == 64
    least = int(re.search(r'uint32_t tbits = (\d+);\s*while \(\(\(u64\)1 << tbits\) < 2 \* most\) tbits\+\+;', src).group(1))
    return (lambda key, bits: ((key * mult) & ((1 << 64) - 1)) >> (width - bits)), least


@functools.lru_cache(maxsize=None)
def _line(npairs):
    """1 x 1 x N, cost 1, max_cost 4 (R = 2): 1100 single-voxel components; component i (1-based) is followed by 3 free voxels
    if i is among the first `npairs` i with hash(i << 32 | i + 1, 6) >= 62, else by 6.  Three free voxels have D = 1, 2, 1 and one
    contact; of six the third would need D = 3 > R: no contact.  Returns the mask, those i and the model's result."""
    hash_of, least = _pair_table_source()
    assert least == 6
    late = [i for i in range(1, 1100) if hash_of(i << 32 | i + 1, 6) >= 62]
    assert len(late) == 34 and late[:3] == [38, 64, 90] and late[-1] == 1079
    chosen = late[:npairs]
    at, z = [], 0
    for i in range(1, 1101):
        at.append(z)
        z += 4 if i in chosen else 7
    mask = np.zeros((1, 1, z), np.uint8)
    mask[0, 0, at] = 1
    return mask, chosen, BM.model(mask, np.ones(mask.shape), None, None, None, 4.0, 0)


def _probed(homes, entries):
    """Linear probing of `homes` in this order into an empty table: the occupied entries, the longest probe."""
    taken, longest = set(), 0
    for h in homes:
        steps = 0
        while (h + steps) % entries in taken:
            steps += 1
        taken.add((h + steps) % entries)
        longest = max(longest, steps)
    return taken, longest


def test_pair_table_certificate():
    """What test_pair_table_wraps rests on: 32 pairs make the smallest table (64 entries) exactly half full, every pair's home
    is entry 62 or 63, so whatever the order of insertion 30 entries wrap past the table's end and the last pair probes 30 or 31
    times - and phase 2 has to walk the same way to find it.  33 pairs take the sizing loop's first step, to 128 entries."""
    hash_of, least = _pair_table_source()
    mask, chosen, ref = _line(32)
    assert mask.shape == (1, 1, 7604) and ref.counts.tolist() == [1100, 7604, 4366, 32, 32, 32, 160]
    assert ref.pairs[:, :2].tolist() == [[i, i + 1] for i in chosen]
    most = min(int(ref.counts[3]), 1100 * 1099 // 2)
    assert most == 32 and 2 * 32 == 64 == 1 << least                   # the loop `while (1 << tbits) < 2 * most` stays at 6
    homes = [hash_of(int(a) << 32 | int(b), 6) for a, b in ref.pairs[:, :2]]
    assert sorted(set(homes)) == [62, 63] and homes.count(62) == 15 and homes.count(63) == 17
    rng = np.random.default_rng(0)
    for order in (homes, homes[::-1], sorted(homes), sorted(homes)[::-1], rng.permutation(homes).tolist()):
        taken, longest = _probed(order, 64)
        assert taken == {62, 63} | set(range(30)) and longest in (30, 31)
        assert sum(e < 62 for e in taken) == 30                       # 30 entries wrap past the table's end
    mask, chosen, ref = _line(33)
    assert mask.shape == (1, 1, 7601) and ref.counts[3:6].tolist() == [33, 33, 33]
    assert (1 << 6) < 2 * 33 <= (1 << 7)                              # 128 entries
    homes = [hash_of(int(a) << 32 | int(b), 7) for a, b in ref.pairs[:, :2]]
    assert all(h >> 1 in (62, 63) for h in homes) and _probed(homes, 128)[0] <= set(range(124, 128)) | set(range(29))


@functools.lru_cache(maxsize=None)
def _lattice_36():
    """Single-voxel components on a 3-spaced lattice in 36^3: more bridges than the tables of the first call hold."""
    shape = (36, 36, 36)
    mask = np.zeros(shape, np.uint8)
    mask[1::3, 1::3, 1::3] = 1
    cost = np.random.default_rng(5).uniform(0.5, 1.0, shape)
    return mask, cost, BM.model(mask, cost, None, None, None, 4.5, 0)


def test_second_call_case_crosses_the_pair_capacity_only():
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'reconnect.py')).read()
    mo = re.search(r'cap_pair, cap_vox = (\d+), 1 << (\d+) ', src)
    assert (int(mo.group(1)), int(mo.group(2))) == (4096, 18)
    mask, cost, ref = _lattice_36()
    assert ref.counts[[0, 4, 5, 6]].tolist() == [1728, 18781, 18433, 73732]
    assert ref.counts[5] > 4096 and ref.counts[6] < 1 << 18


# ------------------------------------------------------------------ GPU
SHAPES = [(8, 8, 8), (9, 17, 23), (1, 1, 40), (3, 5, 70), (20, 24, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('tip_rule,max_cost,dtype', [(0, 3.0, np.float64), (1, 6.0, np.float32), (2, 12.0, np.float64)])
def test_random_shapes(shape, tip_rule, max_cost, dtype):
    mask, cost, dom, tips = _blobs(shape, 7 + shape[1])
    if shape[0] * shape[1] == 1:
        mask = (np.arange(40) % 5 == 2).astype(np.uint8).reshape(shape)
    cost = cost.astype(dtype)                                          # the float32 values go to the model as they are
    b, info, ref = _check(mask, cost, dom, tips, (0.5, 0.5, 0.8), max_cost, tip_rule)
    assert info['components'] > 1 and info['reached'] > 0
    _adjacent(b)


@pytest.mark.gpu
def test_ties():
    """Constant cost 1 and unit spacing: D ties everywhere, so the Root rule, the Pred rule and the contact order decide."""
    shape = (12, 13, 14)
    mask = _points(shape, [(2, 2, 2), (2, 2, 3), (2, 8, 2), (8, 2, 2), (8, 8, 8), (6, 6, 3), (10, 11, 12), (10, 11, 13), (4, 9, 10)])
    for max_cost, least in ((8.0, 4), (6.5, 1)):
        b, info, ref = _check(mask, np.ones(shape), None, None, None, max_cost, 0)
        assert info['bridges'] >= least and info['contacts'] > 10 * info['pairs']


@pytest.mark.gpu
def test_bound_is_inclusive():
    """Axis steps weigh exactly 1.  R = 4: the voxel four steps out is kept, the fifth is not; K == max_cost is kept."""
    shape = (1, 1, 20)
    ones = np.ones(shape)
    b, info, ref = _check(_points(shape, [(0, 0, 0), (0, 0, 8)]), ones, None, None, None, 8.0, 0)
    d = b.dist[0, 0]
    assert d[4] == 4.0 and d[12] == 4.0 and np.isinf(d[13]) and d[9] == 1.0
    assert len(b) == 1 and b.cost[0] == 8.0 and b.voxels.tolist() == list(range(9))
    b, info, ref = _check(_points(shape, [(0, 0, 0), (0, 0, 9)]), ones, None, None, None, 8.0, 0)
    assert info['pairs'] == 1 and len(b) == 0 and b.dist[0, 0, 4] == 4.0 and b.dist[0, 0, 5] == 4.0


@pytest.mark.gpu
@pytest.mark.parametrize('a,c,through', [((6, 6, 6), (10, 10, 10), [(7, 7, 7), (8, 8, 8)]), ((6, 4, 4), (10, 4, 4), [(7, 4, 4), (8, 4, 4)]),
                                         ((6, 6, 4), (10, 10, 4), [(7, 7, 4), (8, 8, 4)])], ids=['corner', 'face', 'edge'])
def test_brick_seams(a, c, through):
    shape = (16, 16, 16)
    b, info, ref = _check(_points(shape, [a, c]), np.ones(shape), None, None, None, 8.0, 0)
    assert len(b) == 1 and info['bricks'] == 8
    path = [tuple(p) for p in b.path(0).tolist()]
    assert path[0] == a and path[-1] == c and all(p in path for p in through)


@pytest.mark.gpu
def test_more_sweeps_than_one_round():
    """A serpentine corridor of domain inside one brick, a source at each end: either flood runs for more steps than a
    workgroup sweeps in one round, so the brick has to flag itself."""
    src = open(os.path.join(ROOT, 'arterynetwork_amd', 'csrc', 'vbrick.h')).read()
    cap = int(re.search(r'constexpr int MAX_SWEEPS = (\d+);', src).group(1))
    dom, order = _serpentine(8)
    assert len(order) // 2 > cap + 8
    mask = _points((8, 8, 8), [order[0], order[-1]])
    b, info, ref = _check(mask, np.ones((8, 8, 8)), dom, None, None, 2.0 * len(order), 0)
    assert info['bricks'] == 1 and info['flood_rounds'] >= 2 and len(b) == 1
    assert info['root_rounds'] >= 2                                    # Root moves one voxel a sweep along either chain: that pass runs out too
    half = b.voxels.tolist().index(int(b.ends[0, 0])) + 1              # the entries of u's chain; the rest is v's
    assert half - 1 > cap and len(b.voxels) - half - 1 > cap


@pytest.mark.gpu
def test_corridor_through_many_bricks():
    shape = (3, 3, 120)
    dom = np.zeros(shape, np.uint8)
    dom[1, 1, :] = 1
    mask = _points(shape, [(1, 1, 0), (1, 1, 119)])
    b, info, ref = _check(mask, np.full(shape, 0.25), dom, None, None, 40.0, 0)
    assert len(b) == 1 and b.voxels.tolist() == [_lin(shape, (1, 1, z)) for z in range(120)]
    assert info['flood_rounds'] >= 7 and info['bricks'] == 15


@pytest.mark.gpu
def test_wall_with_a_hole():
    shape = (12, 12, 12)
    dom = np.ones(shape, np.uint8)
    dom[6] = 0
    dom[6, 2, 9] = 1
    b, info, ref = _check(_points(shape, [(3, 6, 6), (9, 6, 6)]), np.ones(shape), dom, None, None, 30.0, 0)
    assert len(b) == 1 and _lin(shape, (6, 2, 9)) in b.voxels.tolist()
    assert (b.dist[6] == -1.0).sum() == 143


@pytest.mark.gpu
def test_many_pairs():
    """Single-voxel components on a 4-spaced lattice in 48^3: 1728 components, thousands of pairs in the table."""
    shape = (48, 48, 48)
    mask = np.zeros(shape, np.uint8)
    mask[1::4, 1::4, 1::4] = 1
    cost = np.random.default_rng(5).uniform(0.5, 1.0, shape)
    b, info, ref = _check(mask, cost, None, None, None, 4.5, 0)
    assert info['components'] == 1728 and info['pairs'] > 4000 and len(b) > 2000


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SPARSE))
def test_sparse_storage(name):
    """Storage on a 5 x 3 x 9 brick grid where most domain bricks get none: the three axes of the dilation with their strides
    and clamps, bricks within reach without a domain voxel, halo loads from neighbours without a slot, +inf for domain voxels
    without storage.  Exactly the bricks of the header's rule have a slot (stored / domain bricks, as observed: interior 36 / 135,
    also with a float32 cost; reach 2 90 / 135; volume corners 16 / 135; brick corner seam 42 / 135; empty domain bricks
    22 / 104; anisotropic 105 / 135) and every output equals the model's (_check's comparison, on the model kept by _sparse)."""
    mask, cost, dom, spacing, max_cost, ref, stored, facts = _sparse(name)
    b, info = _run(mask, cost, dom, None, spacing, max_cost, 0)
    _same(b, info, ref)
    assert info['bricks'] == int(stored.sum()) and info['bricks'] < facts['domain_bricks']
    assert len(b) >= 1
    _adjacent(b)
    if name == 'interior':                                             # a domain voxel in a brick without storage: out of reach
        assert not stored[0, 0, 0] and b.dist[2, 2, 2] == np.inf and b.root[2, 2, 2] == -1 and b.pred[2, 2, 2] == 255


@pytest.mark.gpu
def test_pair_table_wraps():
    """The 64-entry table at exactly half its entries, every home in its last two (test_pair_table_certificate): probes run
    past the last entry to entry 0, up to 31 steps long, and phase 2 finds after the same walk what phase 1 entered - a pair it
    missed would come back with the tie word it was initialised with, and _same would see its (u, v)."""
    mask, chosen, ref = _line(32)
    b, info = _run(mask, np.ones(mask.shape), None, None, None, 4.0, 0)
    _same(b, info, ref)
    assert info['contacts'] == info['pairs'] == info['bridges'] == 32
    assert b.pairs.tolist() == [[i, i + 1] for i in chosen]


@pytest.mark.gpu
def test_pair_table_grows_at_33_pairs():
    """One pair more than half of 64 entries: the sizing loop takes its first step."""
    mask, chosen, ref = _line(33)
    b, info = _run(mask, np.ones(mask.shape), None, None, None, 4.0, 0)
    _same(b, info, ref)


@pytest.mark.gpu
def test_second_call_after_the_capacity_error():
    """More than 4096 bridges, fewer than 2^18 path entries: bridgeCandidates learns the sizes from the VRG_E_ARG of its first
    call and runs again; nothing of the first call shows in the tables, the fields or the counts."""
    mask, cost, ref = _lattice_36()
    b, info = _run(mask, cost, None, None, None, 4.5, 0)
    _same(b, info, ref)
    assert len(b) > 4096 and len(b.voxels) < 1 << 18 and info['bridges'] == len(b)


@pytest.mark.gpu
def test_empty_cases():
    shape = (9, 10, 11)
    cost = np.random.default_rng(2).uniform(0.5, 2.0, shape)
    b, info, ref = _check(np.zeros(shape, np.uint8), cost, None, None, None, 6.0, 0)
    assert len(b) == 0 and b.ncomp == 0 and b.offsets.tolist() == [0]
    one = np.zeros(shape, np.uint8)
    one[2:5, 3:6, 4] = 1
    b, info, ref = _check(one, cost, None, None, None, 6.0, 0)
    assert len(b) == 0 and b.ncomp == 1 and info['reached'] > 0
    b, info, ref = _check(_points(shape, [(0, 0, 0), (8, 9, 10)]), cost, None, None, None, 2.0, 0)
    assert len(b) == 0 and b.ncomp == 2 and info['contacts'] == 0
    b, info, ref = _check(_points(shape, [(0, 0, 0), (0, 0, 3)]), cost, np.zeros(shape, np.uint8), None, None, 50.0, 0)
    assert len(b) == 0 and info['domain_voxels'] == 2


def _raw(mask, cost, domain=None, tips=None, spacing=None, max_cost=8.0, tip_rule=0, cap_pair=None, cap_vox=None, dims=None, dtype=None):
    """One call of the C entry with every output pre-filled, so that 'nothing is written' can be seen."""
    dll = R._lib()
    shape = mask.shape if dims is None else dims
    counts = np.full(10, -7, np.int64)
    lists = cap_pair is not None
    pairs, costs = np.full((max(1, cap_pair or 0), 6), -7, np.int64), np.full(max(1, cap_pair or 0), -7.0)
    offsets, voxels = np.full(max(1, cap_pair or 0) + 1, -7, np.int64), np.full(max(1, cap_vox or 0), -7, np.int64)
    dist, root, pred, comp = np.full(mask.shape, -7.0), np.full(mask.shape, -7, np.int32), np.full(mask.shape, 7, np.uint8), np.full(mask.shape, -7, np.int32)
    p = lambda a: a.ctypes.data if a is not None else None
    sp = None if spacing is None else np.asarray(spacing, np.float64)
    rc = dll.vmask_bridge(0, p(mask), p(domain), p(cost), (5 if cost.dtype == np.float32 else 6) if dtype is None else dtype, p(tips), *shape, p(sp),
                          float(max_cost), int(tip_rule), p(counts), p(pairs) if lists else None, p(costs) if lists else None, cap_pair or 0,
                          p(offsets) if lists else None, p(voxels) if lists else None, cap_vox or 0, p(dist), p(root), p(pred), p(comp))
    untouched = all((a == -7).all() for a in (pairs, costs, offsets, voxels, dist, root, comp)) and (pred == 7).all()
    return rc, counts, untouched, (pairs, costs, offsets, voxels)


@functools.lru_cache(maxsize=None)
def _small():
    shape = (10, 10, 12)
    mask = _points(shape, [(2, 2, 2), (2, 2, 6), (6, 3, 2), (7, 7, 9)])
    return mask, np.random.default_rng(3).uniform(0.5, 1.5, shape)


@pytest.mark.gpu
def test_tip_rule_corners():
    """tips == NULL counts every root as a tip, under rule 2 as well; all-zero tips leave rule 0 as it is and give rule 1
    nothing: no contact although the flood reached voxels and every slot is there."""
    mask, cost = _small()
    ones, zeros = np.ones(mask.shape, np.uint8), np.zeros(mask.shape, np.uint8)
    b1, info1, ref1 = _check(mask, cost, None, ones, None, 8.0, 2)
    b0, info0, ref0 = _check(mask, cost, None, None, None, 8.0, 2)
    assert len(b1) >= 3
    _same(b0, info0, ref1)
    b, info, ref = _check(mask, cost, None, zeros, None, 8.0, 1)
    assert info['contacts'] == 0 and len(b) == 0 and b.offsets.tolist() == [0] and info['reached'] > 0 and info['bricks'] > 0
    plain = BM.model(mask, cost, None, None, None, 8.0, 0)
    b, info, ref = _check(mask, cost, None, zeros, None, 8.0, 0)
    assert len(b) >= 3
    _same(b, info, plain)


@pytest.mark.gpu
def test_capacity_protocol():
    mask, cost = _small()
    ref = BM.model(mask, cost, None, None, None, 8.0, 0)
    nb, nv = int(ref.counts[5]), int(ref.counts[6])
    assert nb >= 3
    rc, counts, _, _ = _raw(mask, cost)                                # all four NULL: counts (and the dense fields) only
    assert rc == 0 and counts[:7].tolist() == ref.counts.tolist()
    for cp, cv in ((nb - 1, nv), (nb, nv - 1), (0, 0)):
        rc, counts, untouched, _ = _raw(mask, cost, cap_pair=cp, cap_vox=cv)
        assert rc == E_ARG and untouched and counts[:7].tolist() == ref.counts.tolist()
        assert b'capacity' in R._lib().vmask_last_error()
    rc, counts, untouched, (pairs, costs, offsets, voxels) = _raw(mask, cost, cap_pair=nb, cap_vox=nv)
    assert rc == 0 and not untouched
    assert np.array_equal(pairs, ref.pairs) and np.array_equal(_bits(costs), _bits(ref.costs))
    assert np.array_equal(offsets, ref.offsets) and np.array_equal(voxels, ref.voxels)


@pytest.mark.gpu
def test_argument_errors_write_nothing():
    mask, cost = _small()
    dom = np.ones(mask.shape, np.uint8)
    dom[0, 0, 0] = 0
    bad = []
    for value in (0.0, -1.0, float('nan'), float('inf')):
        c = cost.copy()
        c[5, 5, 5] = value
        bad.append(dict(cost=c))
    c32 = cost.astype(np.float32)
    c32[2, 2, 2] = 0.0                                                 # a mask voxel is in the domain whatever `domain` says
    bad.append(dict(cost=c32, domain=np.zeros(mask.shape, np.uint8)))
    bad += [dict(max_cost=v) for v in (0.0, -2.0, float('nan'), float('inf'))]
    bad.append(dict(cost=np.full(mask.shape, 1e-14), max_cost=1.0))    # R / w_min > 2^40
    bad += [dict(spacing=s) for s in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float('nan'), 1.0), (1.0, float('inf'), 1.0), (1.0, 1.0, 1001.0))]
    bad += [dict(tip_rule=3), dict(tip_rule=-1), dict(dtype=4)]
    bad += [dict(dims=(0, 10, 12)), dict(dims=(40000, 1, 1)), dict(dims=(2000, 2000, 2000))]
    for kw in bad:
        args = dict(cost=cost)
        args.update(kw)
        rc, counts, untouched, _ = _raw(mask, cap_pair=16, cap_vox=256, **args)
        assert rc == E_ARG and untouched and (counts == -7).all(), kw
    c = cost.copy()
    c[0, 0, 0] = float('nan')                                          # outside the domain a cost is never read
    rc, counts, untouched, _ = _raw(mask, c, domain=dom, cap_pair=16, cap_vox=256)
    assert rc == 0 and not untouched
    rc, counts, _, _ = _raw(mask, np.full(mask.shape, 1e-11), max_cost=1.0, cap_pair=16, cap_vox=256)      # R / w_min = 2^-1 10^11 < 2^40
    assert rc == 0 and counts[:7].tolist() == BM.model(mask, np.full(mask.shape, 1e-11), None, None, None, 1.0, 0).counts.tolist()


@pytest.mark.gpu
def test_repeat_is_bit_identical():
    mask, cost, dom, tips = _blobs((20, 24, 40), 11)
    first, info1 = _run(mask, cost, dom, tips, (0.5, 0.5, 0.8), 6.0, 1)
    again, info2 = _run(mask, cost, dom, tips, (0.5, 0.5, 0.8), 6.0, 1)
    assert len(first) > 0 and [info1[k] for k in R.COUNT_KEYS[:8]] == [info2[k] for k in R.COUNT_KEYS[:8]]
    for name in ('pairs', 'ends', 'roots', 'offsets', 'voxels', 'root', 'pred', 'comp'):
        assert np.array_equal(getattr(first, name), getattr(again, name)), name
    assert np.array_equal(_bits(first.cost), _bits(again.cost)) and np.array_equal(_bits(first.dist), _bits(again.dist))


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import reconnect as R
import test_bridge as T
mask, cost, dom, tips = T._blobs((9, 17, 23), 13)
ref = T.BM.model(mask, cost, dom, tips, (0.5, 0.5, 0.8), 6.0, 1)
dev = torch.device('cuda', 0)
info = {{}}
b = R.bridgeCandidates(torch.as_tensor(mask * 255, device=dev), torch.as_tensor(cost, device=dev), domain=dom, tips=torch.as_tensor(tips, device=dev),
                       maxCost=6.0, tipRule=1, spacing=(0.5, 0.5, 0.8), info=info, return_fields=True)
assert b.dist.is_cuda and b.root.is_cuda and b.pred.is_cuda and b.comp.is_cuda and isinstance(b.pairs, np.ndarray) and len(b) > 0
T._same(b, info, ref)
h, hinfo = T._run(mask, cost, dom, tips, (0.5, 0.5, 0.8), 6.0, 1)
T._same(h, hinfo, ref)
keep = R.selectBridges(b)
bridged, only = R.applyBridges(torch.as_tensor(mask, device=dev), b, keep, thicken=1, domain=dom)
host, host_only = R.applyBridges(mask, h, keep, thicken=1, domain=dom)
assert bridged.is_cuda and np.array_equal(bridged.cpu().numpy(), host) and np.array_equal(only.cpu().numpy(), host_only)
assert host_only.sum() > len(b.voxels) - 2 * len(b) and not (host_only & mask).any() and not (host_only & (dom == 0)).any()
c = R.vesselCost(torch.as_tensor(cost, device=dev), floor=0.1, brainVolumeMask=dom)
# torch divides by a scalar through its rounded reciprocal: v / top is within 1.5 ulp of numpy's quotient, and the sum and the final
# quotient add at most an ulp each: 4 ulp = 8.9e-16 relative
assert c.is_cuda and np.allclose(c.cpu().numpy(), R.vesselCost(cost, floor=0.1, brainVolumeMask=dom), rtol=1e-15, atol=0.0)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_tensors_give_the_same():
    """Mask, cost and tips as tensors on the GPU go in by their device pointers and give what the numpy call gives; the dense
    fields come back as tensors.  Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize('g,entries', [(3, 5), (5, 7), (8, 10)])
def test_recovery_phantom(g, entries):
    """The required outcome, with the costs this implementation's model gives (a heap prototype gave 5.42, 8.07, 11.59 across
    the gap and 35.7, 36.0-36.2 sideways): K = 5.365 (g = 3), 7.996 (g = 5), 11.484 (g = 8) across the gap; the cheapest contacts
    sideways to tube 2 cost 35.50 and 35.81-36.05 without the tip rule.  With maxCost = 16 exactly one bridge comes back, between
    the halves of tube 1; reconnect leaves two components; with maxCost = 40 three candidates, of which a forest takes two."""
    from arterynetwork_amd import generateVesselVolume as G
    mask, v = phantom(g)
    cost = R.vesselCost(v, floor=0.05)
    dom = np.ones(mask.shape, np.uint8)
    comp, n = BM.components(mask != 0)
    assert n == 3 and comp[8, 8, 0] == 1 and comp[8, 8, 39] == 2 and comp[8, 16, 20] == 3
    tips = R.tipRegions(mask, reach=3.0)
    assert tips[8, 8, 17] and tips[8, 8, 18 + g] and not tips[8, 8, 10] and not (tips & (mask == 0)).any()
    info = {}
    b = R.bridgeCandidates(mask, cost, domain=dom, tips=tips, maxCost=16.0, info=info, return_fields=True)
    _same(b, info, BM.model(mask, cost, dom, tips, None, 16.0, 1))
    print('g = %d: K = %r, %d path entries' % (g, b.cost.tolist(), len(b.voxels)))
    assert len(b) == 1 and b.pairs.tolist() == [[1, 2]] and len(b.voxels) == entries
    assert b.cost[0] == BM.model(mask, cost, dom, None, None, 16.0, 0).costs[0]              # the tip rule does not change this bridge
    bridged, only, bridges, keep = R.reconnect(mask, v, brainVolumeMask=dom, maxCost=16.0)
    assert keep.tolist() == [0] and int(only.sum()) == g and G.labelVolume(bridged)[1][-1][0] == 2
    assert int(bridged.sum()) == int(mask.sum()) + g and not (only & mask).any()
    wide = R.bridgeCandidates(mask, cost, domain=dom, tips=tips, maxCost=40.0)
    print('maxCost = 40: K = %r' % (wide.cost.tolist(),))
    assert wide.pairs.tolist() == [[1, 2], [1, 3], [2, 3]]
    assert len(R.selectBridges(wide, forest=True)) == 2 and len(R.selectBridges(wide, forest=False)) == 3


@pytest.mark.gpu
def test_main_end_to_end(tmp_path):
    """A round-ended tube with a gap, as files: the bridged mask traces to one branch where the unbridged one gives two."""
    from arterynetwork_amd import nifti, skeletonization as S
    shape = (16, 16, 40)
    i0, i1, i2 = np.indices(shape)
    r = (i0 - 8) ** 2 + (i1 - 8) ** 2
    capsule = lambda z0, z1: r + (np.clip(i2, z0, z1) - i2) ** 2 <= 2.25          # round ends: the skeleton has no corner spurs
    mask = (capsule(4, 16) | capsule(23, 35)).astype(np.uint8)                      # z = 18 .. 21 is missing
    v = np.exp(-r / 4.0) * (0.6 + 0.4 * np.random.default_rng(4).random(shape))
    affine = np.diag([0.5, 0.5, 0.5, 1.0])
    nifti.write(str(tmp_path / 'vesselVolumeMask.nii.gz'), mask, affine)
    nifti.write(str(tmp_path / 'vesselnessFiltered.nii.gz'), v, affine)
    nifti.write(str(tmp_path / 'brainVolumeMask.nii.gz'), np.ones(shape, np.uint8), affine)
    bridged, bridges, keep = R.main(str(tmp_path), maxCost=16.0)
    out, aff, _ = nifti.read(str(tmp_path / 'vesselVolumeMaskBridged.nii.gz'))
    assert out.dtype == np.uint8 and np.array_equal(out, bridged) and np.allclose(aff, affine)
    assert np.array_equal(nifti.read(str(tmp_path / 'vesselVolumeMask.nii.gz'))[0], mask)    # the input stays as it was
    z = np.load(str(tmp_path / 'bridges.npz'))
    assert z['keep'].tolist() == [0] and z['pairs'].tolist() == [[1, 2]] and len(z['voxels']) == 6
    assert len(S.traceSegments(S.skeletonize(mask))) == 2
    assert len(S.traceSegments(S.skeletonize(out))) == 1
