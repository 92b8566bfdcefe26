"""Compartment partition ("f12 compartments"): the sequential model tests/compartment_model.py is checked
against answers written out by hand and against networkx's shortest-path lengths on the CPU, then the GPU (vmask_compartments /
skeletonization.partitionCompartments) must equal it: every output is an integer."""
import functools
import gzip
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import branch_model as BM
import compartment_model as CM
import skeleton_model as M
from conftest import GOLDEN_DIR, ROOT
from test_morphometry import Tables, _double_tee, _helix, _path
from arterynetwork_amd import skeletonization as S
from arterynetwork_amd.skeletonization import COMPARTMENT_ARRAYS, compartmentSummary, compartmentTerritories, partitionCompartments


# ------------------------------------------------------------------ graphs
def _of_volume(volume):
    sk, g = BM.branch_graph(np.asarray(volume), 0, 0.0, None, 64)
    return Tables(np.shape(volume), g.offsets, g.voxels, g.ends, g.nodes[:, 0], g.nodes[:, 1], g.nodes[:, 3])


def _table(branches, closed=(), size=None):
    """A table written by hand: `branches` are lists of voxel numbers (any distinct numbers: the partition looks at the table
    alone), the branches in `closed` have no node; the nodes are the open branches' end voxels, ascending."""
    nodes = sorted({v for k, br in enumerate(branches) if k not in closed for v in (br[0], br[-1])})
    ends = [[-1, -1] if k in closed else [nodes.index(br[0]), nodes.index(br[-1])] for k, br in enumerate(branches)]
    voxels = [v for br in branches for v in br]
    size = size or max(voxels + [0]) + 1
    degree = np.bincount(np.asarray(ends, np.int64).ravel()[np.asarray(ends, np.int64).ravel() >= 0], minlength=len(nodes))
    return Tables((1, 1, size), np.cumsum([0] + [len(br) for br in branches]), voxels, np.asarray(ends, np.int64).reshape(-1, 2), nodes,
                  kind=(degree != 1).astype(np.int64), degree=degree)


def _line(n):
    return _path((1, 1, n), [(0, 0, k) for k in range(n)])


def _tee():
    """A straight line with a perpendicular arm: a cluster of four junction voxels represented by the arm's foot (5, 6, 1)."""
    v = np.zeros((11, 11, 3), np.uint8)
    v[0:11, 5, 1] = 1
    v[5, 6:11, 1] = 1
    return v


RING = dict(branches=[[0, 1, 2, 10], [0, 3, 4, 5, 6, 10]])               # two nodes 0 and 10, three and five edges between them
TRIANGLE = dict(branches=[[0, 1, 2, 3, 10], [0, 4, 20], [20, 5, 10]])     # 0 - 10 by four edges, and by two and two through the node 20
LOLLIPOP = dict(branches=[[0, 1, 2, 3], [3, 4, 5, 6, 7, 3]])              # a stalk from the end point 0 and a loop on the node 3
CLOSED = dict(branches=[[5, 6, 7, 8, 9, 10, 5]], closed=(0,))


def _comb(teeth):
    """A backbone of `teeth` junctions four edges apart, entered at the end point 0, one tooth of two edges per junction.
    Junction k is voxel 10 k + 10, its tooth's tip 10 k + 16."""
    branches, at = [], 0
    for k in range(teeth):
        j = 10 * k + 10
        branches.append([at, j - 9, j - 8, j - 7, j])
        branches.append([j, j + 5, j + 6])
        at = j
    branches.append([at, at + 1, at + 2])
    return _table(branches)


def _two_components():
    return _table([[0, 1, 2, 3], [3, 4, 5], [3, 6, 7, 8], [20, 21, 22, 23, 24], [24, 25, 26], [24, 27, 28]])


def _y_phantom():
    """A thick Y in 24 x 24 x 40: a trunk along axis 2 that splits into two arms."""
    v = np.zeros((24, 24, 40), np.uint8)
    v[10:14, 10:14, 2:20] = 1
    for k in range(18):
        v[10:14, 10 + k // 2:14 + k // 2, 20 + k] = 1
        v[10:14, 10 - k // 2:14 - k // 2, 20 + k] = 1
    return v


def _model(t, comps):
    return CM.partition(t.offsets, t.voxels, t.ends, t.node_voxel, comps)


def _coords(t, comps):
    """Lists of linear indices as the coordinate triples that `partitionCompartments` takes."""
    co = lambda v: [tuple(int(c) for c in p) for p in np.stack(np.unravel_index(np.asarray(v, np.int64), t.shape), axis=1)] if len(v) else []
    return [(co(a), co(b)) for a, b in comps]


def _parts(t, comps, names=None):
    """A `Compartments` of the model's arrays."""
    m = _model(t, comps)
    return S.Compartments(names or [str(k + 1) for k in range(len(comps))], t.kind, **{k: m[k] for k in COMPARTMENT_ARRAYS})


def _entry(t, b, i):
    return int(t.voxels[t.offsets[b] + i])


# ------------------------------------------------------------------ CPU: the model against answers written by hand
def test_line_cut_by_a_boundary():
    t = _line(9)
    m = _model(t, [([0], [5])])
    assert m['entryCompartment'].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert m['entryDepth'].tolist() == [0, 1, 2, 3, 4, -1, -1, -1, -1] and m['entryLevel'].tolist() == [0, 0, 0, 0, 0, -1, -1, -1, -1]
    assert m['nodeCompartment'].tolist() == [1, 0] and m['nodeDepth'].tolist() == [0, -1] and m['nodeLevel'].tolist() == [0, -1]
    assert m['branchCompartment'].tolist() == [0] and m['branchLevel'].tolist() == [-1]      # a prefix is reached: the branch is nobody's
    assert m['compartmentCounts'].tolist() == [[4, 0, 1], [5, 5, 0]]
    m = _model(t, [([0], [])])                                            # without the boundary: the far end is a node, level 1
    assert m['entryDepth'].tolist() == list(range(9)) and m['entryLevel'].tolist() == [0] * 8 + [1]
    assert m['branchCompartment'].tolist() == [1] and m['branchLevel'].tolist() == [0] and m['compartmentCounts'].tolist() == [[0, 0, 0], [9, 9, 1]]
    m = _model(t, [([4], [])])                                            # from the middle: both ends at depth 4, level 1
    assert m['entryDepth'].tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4] and m['entryLevel'].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1]


def test_tee_with_the_boundary_on_the_representative():
    t = _of_volume(_tee())
    lin = lambda p: int(np.ravel_multi_index(p, t.shape))
    rep, start, far, tip = t.node_at((5, 6, 1)), t.node_at((0, 5, 1)), t.node_at((10, 5, 1)), t.node_at((5, 10, 1))
    assert len(t.node_voxel) == 4 and sorted(np.diff(t.offsets).tolist()) == [5, 6, 6] and lin((5, 5, 1)) not in t.voxels
    m = _model(t, [([lin((0, 5, 1))], [lin((5, 6, 1))])])
    own = m['entryCompartment'] == 1
    assert sorted(t.voxels[own].tolist()) == [lin((k, 5, 1)) for k in range(5)] and m['entryDepth'][own].tolist() == [0, 1, 2, 3, 4]
    assert m['nodeCompartment'].tolist() == [int(v == start) for v in range(4)] and (m['branchCompartment'] == 0).all()
    assert m['compartmentCounts'].tolist() == [[10, 0, 3], [5, 5, 0]]    # 4 nodes and 4 + 4 + 3 interior entries
    m = _model(t, [([lin((0, 5, 1))], [])])                               # without it: through the cluster into the two other branches
    assert m['nodeDepth'][[start, rep, far, tip]].tolist() == [0, 5, 10, 9] and m['nodeLevel'][[start, rep, far, tip]].tolist() == [0, 1, 2, 2]
    first = [b for b in range(3) if t.ends[b].tolist() in ([start, rep], [rep, start])][0]
    assert m['branchCompartment'].tolist() == [1, 1, 1] and m['branchLevel'].tolist() == [0 if b == first else 1 for b in range(3)]
    assert sorted(m['entryLevel'].tolist()) == [0] * 5 + [1] * 10 + [2] * 2


def test_ring_takes_the_smaller_level():
    t = _table(**RING)
    m = _model(t, [([0], [])])
    assert m['nodeDepth'].tolist() == [0, 3] and m['nodeLevel'].tolist() == [0, 1]
    # the entry of voxel 6 is four edges from the start either way: behind 5 (level 0) and behind the node 10 (level 1)
    assert m['entryDepth'].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4, 3] and m['entryLevel'].tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    assert m['branchCompartment'].tolist() == [1, 1] and m['branchLevel'].tolist() == [0, 0]
    t = _table(**TRIANGLE)
    m = _model(t, [([0], [])])                                            # the node 10: level 1 behind the long branch, 2 behind the node 20
    assert m['nodeDepth'].tolist() == [0, 4, 2] and m['nodeLevel'].tolist() == [0, 1, 1]
    assert m['entryLevel'].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 1] and m['branchLevel'].tolist() == [0, 0, 1]
    t = _table(**LOLLIPOP)
    m = _model(t, [([0], [])])
    assert m['entryDepth'].tolist() == [0, 1, 2, 3, 3, 4, 5, 5, 4, 3] and m['entryLevel'].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    assert m['branchCompartment'].tolist() == [1, 1] and m['branchLevel'].tolist() == [0, 1]


@pytest.mark.parametrize('n', [8, 9])
def test_two_compartments_meet_on_a_line(n):
    t = _line(n)
    m = _model(t, [([0], []), ([n - 1], [])])
    half = (n + 1) // 2                                                   # n = 9: entry 4 is four edges from both, the smaller label holds
    assert m['entryCompartment'].tolist() == [1] * half + [2] * (n - half)
    assert m['entryDepth'].tolist() == list(range(half)) + list(range(n - half))[::-1]
    assert m['branchCompartment'].tolist() == [0] and m['compartmentCounts'].tolist() == [[0, n, 1], [half, n, 0], [n - half, n, 0]]
    m = _model(t, [([n - 1], []), ([0], [])])                             # the labels swapped: the tie goes the other way
    assert m['entryCompartment'].tolist() == [2] * (n // 2) + [1] * (n - n // 2)


def test_closed_curve():
    t = _table(**CLOSED)
    m = _model(t, [([7], [9])])
    assert m['entryCompartment'].tolist() == [1, 1, 1, 1, 0, 1, 1] and m['entryDepth'].tolist() == [2, 1, 0, 1, -1, 3, 2]
    assert m['entryLevel'].tolist() == [0, 0, 0, 0, -1, 0, 0] and m['branchCompartment'].tolist() == [0]
    assert m['compartmentCounts'].tolist() == [[1, 0, 1], [5, 5, 0]]     # six vertices: the private one counts once
    m = _model(t, [([5], [])])                                            # from the private vertex
    assert m['entryDepth'].tolist() == [0, 1, 2, 3, 2, 1, 0] and m['branchCompartment'].tolist() == [1] and m['branchLevel'].tolist() == [0]
    m = _model(t, [([8], [5])])                                           # the private vertex blocked
    assert m['entryDepth'].tolist() == [-1, 2, 1, 0, 1, 2, -1] and m['compartmentCounts'].tolist() == [[1, 0, 1], [5, 5, 0]]


# ------------------------------------------------------------------ random volumes: the cases, and that they are not hollow
# density -> (seed of the volume, seed of the lists); at 0.6 nearly everything is one junction cluster: volume 53 is the first from 43 on
# whose graph (four loops on the one node) lets the three properties of test_random_cases_are_not_hollow hold together
RANDOM = {0.1: (41, 0), 0.3: (42, 0), 0.6: (53, 66)}


def _random_volume(density):
    return (np.random.default_rng(RANDOM[density][0]).random((24, 24, 24)) < density).astype(np.uint8)


@functools.lru_cache(None)
def _random_case(density):
    seed, draw = RANDOM[density]
    t = _of_volume(_random_volume(density))
    rng = np.random.default_rng(draw)
    comps = []
    for _ in range(3):                                                    # two initial voxels, eight boundary voxels (fewer in a small graph)
        initial = rng.choice(t.voxels, 2).tolist()
        comps.append((initial, [int(v) for v in rng.choice(t.voxels, max(1, min(8, len(t.voxels) // 4))) if v not in initial]))
    return t, comps, _model(t, comps)


@pytest.mark.parametrize('density', sorted(RANDOM))
def test_random_cases_are_not_hollow(density):
    t, comps, m = _random_case(density)
    own = [m['entryCompartment'][t.offsets[b]:t.offsets[b + 1]] for b in range(len(t.offsets) - 1)]
    assert any((o > 0).any() and (o == 0).any() for o in own), 'no partly reached branch'
    assert any((o == 0).all() for o in own), 'no unreached branch'
    assert m['compartmentCounts'][0, 1] > 0, 'no vertex reached twice'


@pytest.mark.parametrize('density', sorted(RANDOM))
def test_model_depths_against_networkx(density):
    nx = pytest.importorskip('networkx')
    t, comps, m = _random_case(density)
    g = m['graph']
    G = nx.Graph()
    G.add_nodes_from(range(len(g.voxel)))
    G.add_edges_from((x, y) for x in range(len(g.voxel)) for y in g.adj[x])
    for c, (initial, boundary) in enumerate(comps):
        H = G.subgraph(np.flatnonzero(~np.isin(g.voxel, boundary)).tolist())
        want = nx.multi_source_dijkstra_path_length(H, set(np.flatnonzero(np.isin(g.voxel, initial) & ~np.isin(g.voxel, boundary)).tolist()))
        depth, level = CM.traverse(g, initial, boundary)
        assert {x: int(d) for x, d in enumerate(depth) if d >= 0} == want
        assert (m['reached'][c] == (depth >= 0)).all() and ((level >= 0) == (depth >= 0)).all() and (level <= depth).all()
    for t2 in (_table(**RING), _table(**TRIANGLE), _table(**LOLLIPOP), _comb(5)):
        g = CM.VertexGraph(t2.offsets, t2.voxels, t2.ends, t2.node_voxel)
        G = nx.Graph((x, y) for x in range(len(g.voxel)) for y in g.adj[x])
        assert {x: int(d) for x, d in enumerate(CM.traverse(g, [0], [])[0])} == dict(nx.single_source_shortest_path_length(G, 0))


# ------------------------------------------------------------------ CPU: the host layer
def test_host_errors_and_partition_info():
    t = _of_volume(_tee())
    g = t.graph()
    g.skeleton = _tee()                                                   # (with the cluster's members that are no entries)
    names, lists = S._compartment_lists(g, {'LMCA': {'initialVoxels': [(0, 5, 1), t.node_at((5, 6, 1))], 'boundaryVoxels': [[3, 5, 1]]},
                                            'ACA': {'initialVoxels': [], 'boundaryVoxels': np.array([[5, 8, 1]])}})
    lin = lambda p: int(np.ravel_multi_index(p, t.shape))
    assert names == ['LMCA', 'ACA'] and [[a.tolist(), b.tolist()] for a, b in lists] == [[[lin((0, 5, 1)), lin((5, 6, 1))], [lin((3, 5, 1))]], [[], [lin((5, 8, 1))]]]
    assert S._compartment_lists(g, [([0], []), ([], [1])])[0] == ['1', '2']
    with pytest.raises(ValueError, match=r'\(5, 5, 1\).*junction cluster'):       # a member of the cluster, not its representative
        S._compartment_lists(g, [([(5, 5, 1)], [])])
    with pytest.raises(ValueError, match=r'\(1, 1, 1\) is no voxel of the centre line'):
        S._compartment_lists(g, [([], [(1, 1, 1)])])
    with pytest.raises(ValueError, match='outside the volume'):
        S._compartment_lists(g, [([(0, 5, 3)], [])])
    with pytest.raises(ValueError, match='no node index'):
        S._compartment_lists(g, [([4], [])])
    with pytest.raises(ValueError, match='1 to 255'):
        S._compartment_lists(g, [])
    with pytest.raises(ValueError, match='1 to 255'):
        S._compartment_lists(g, [([], [])] * 256)
    # partitionInfo: the reference's layout; a vertex once, by depth and then by entry
    t = _line(9)
    info = _parts(t, [([0], []), ([8], [])], ['LMCA', 'RMCA']).partitionInfo(t.graph())
    assert info == {'LMCA': {'visitedVoxels': [(0, 0, k) for k in range(5)], 'segmentIndexList': []},
                    'RMCA': {'visitedVoxels': [(0, 0, k) for k in (8, 7, 6, 5)], 'segmentIndexList': []}}
    assert all(type(c) is int for v in info['LMCA']['visitedVoxels'] for c in v)
    t = _table(**RING)
    info = _parts(t, [([0], [])]).partitionInfo(t.graph())
    assert info['1']['visitedVoxels'] == [(0, 0, v) for v in (0, 1, 3, 2, 4, 10, 5, 6)] and info['1']['segmentIndexList'] == [0, 1]
    t = _table(**CLOSED)
    info = _parts(t, [([5], [])]).partitionInfo(t.graph())
    assert info['1']['visitedVoxels'] == [(0, 0, v) for v in (5, 6, 10, 7, 9, 8)] and info['1']['segmentIndexList'] == [0]
    assert pickle.loads(pickle.dumps(info, protocol=2)) == info


def test_summary_groups_by_compartment():
    t = _two_components()
    parts = _parts(t, [([0], []), ([20], [(24)])], ['A', 'B'])
    class Measured:
        pathLength = np.array([3.0, 2.0, 0.1, 4.0, 2.0, 2.0])
        meanRadius = np.array([1.0, 2.0, 3.0, 5.0, 1.0, 1.0])
    s = compartmentSummary(parts, Measured, sizes=np.array([7, 30, 10]), affine=np.diag([0.5, 0.5, 2.0, 1.0]))
    assert s['A'] == {'branches': 3, 'terminalNodes': 3, 'maxLevel': 1, 'totalLength': 5.1, 'meanRadius': 2.0, 'volume': 15.0}
    assert s['B']['branches'] == 0 and s['B']['terminalNodes'] == 1 and s['B']['maxLevel'] == -1 and s['B']['totalLength'] == 0.0 and np.isnan(s['B']['meanRadius'])
    assert set(compartmentSummary(parts)['A']) == {'branches', 'terminalNodes', 'maxLevel'}


# ------------------------------------------------------------------ the reference's own traversal, recorded
TREE = os.path.join(GOLDEN_DIR, 'compartments', 'tree.npz')


def _tree_case():
    z = np.load(TREE)
    t = Tables(tuple(z['shape']), z['offsets'], z['voxels'], z['ends'], z['node_voxel'])
    comps = [(z['initial'][z['initial_off'][k]:z['initial_off'][k + 1]].tolist(), z['boundary'][z['boundary_off'][k]:z['boundary_off'][k + 1]].tolist())
             for k in range(len(z['initial_off']) - 1)]
    return z, t, comps


def _assert_equals_the_recording(z, t, k, got):
    """`got`: the arrays of a K = 1 run of compartment k; the recording: visited voxels with depthVoxel and depthLevel, the branches."""
    lo, hi = z['visited_off'][k], z['visited_off'][k + 1]
    want = {int(v): (int(d), int(l)) for v, d, l in zip(z['visited'][lo:hi], z['depthVoxel'][lo:hi], z['depthLevel'][lo:hi])}
    own = np.asarray(got['entryCompartment']) == 1
    mine = {int(v): (int(d), int(l)) for v, d, l in zip(t.voxels[own], np.asarray(got['entryDepth'])[own], np.asarray(got['entryLevel'])[own])}
    assert mine == want
    assert np.flatnonzero(np.asarray(got['branchCompartment']) == 1).tolist() == z['segments'][z['segments_off'][k]:z['segments_off'][k + 1]].tolist()


def test_model_equals_the_reference_on_a_tree():
    z, t, comps = _tree_case()
    assert len(comps) >= 3
    for k, comp in enumerate(comps):
        _assert_equals_the_recording(z, t, k, _model(t, [comp]))


# ------------------------------------------------------------------ GPU: exactly the model
def _assert_equal_to_model(got, m):
    for k in COMPARTMENT_ARRAYS:
        a, b = np.asarray(getattr(got, k)), m[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a, b), k


def _check(t, comps):
    got = partitionCompartments(t.graph(), _coords(t, comps))
    m = _model(t, comps)
    _assert_equal_to_model(got, m)
    return got, m


def _line_compartments(t):
    """Initial at an end, in the middle, at both; boundary at entry 1, in the middle, at the last entry: nine compartments (a
    voxel drawn for both lists stays a boundary voxel only)."""
    n = len(t.voxels)
    comps = []
    for initial in ([0], [n // 2], [0, n - 1]):
        for boundary in (1, n // 2, n - 1):
            comps.append(([int(t.voxels[i]) for i in initial if i != boundary], [int(t.voxels[boundary])]))
    return comps


@pytest.mark.gpu
@pytest.mark.parametrize('n', [2, 3, 17, 18, 64, 65, 130, 1000])
def test_lines(n):
    for t in (_line(n), _helix(n)):
        assert np.diff(t.offsets).tolist() == [n]
        comps = _line_compartments(t)
        _check(t, comps)
        for comp in comps[:3] + comps[6:]:
            _check(t, [comp])                                             # K = 1: the compartment's own traversal
        _check(t, [([int(t.voxels[0])], []), ([int(t.voxels[-1])], [])])


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['tee', 'double-tee', 'ring', 'triangle', 'lollipop', 'closed'])
def test_shapes(case):
    t = {'tee': lambda: _of_volume(_tee()), 'double-tee': lambda: _of_volume(_double_tee()), 'ring': lambda: _table(**RING),
         'triangle': lambda: _table(**TRIANGLE), 'lollipop': lambda: _table(**LOLLIPOP), 'closed': lambda: _table(**CLOSED)}[case]()
    E = len(t.voxels)
    if case == 'double-tee':
        assert sum(np.abs(np.diff(np.stack(np.unravel_index(t.voxels[a:b], t.shape), axis=1), axis=0)).max() > 1 for a, b in zip(t.offsets[:-1], t.offsets[1:])) == 2
    start = int(t.node_voxel[0]) if len(t.node_voxel) else _entry(t, 0, 0)
    _check(t, [([start], [])])
    for i in range(E):                                                    # every entry as the one initial voxel, then as the one boundary voxel
        v = int(t.voxels[i])
        _check(t, [([v], [])])
        if v != start:
            _check(t, [([start], [v])])
    _check(t, [([int(t.voxels[i])], [int(t.voxels[(i + 3) % E])]) for i in range(0, E, 2) if t.voxels[i] != t.voxels[(i + 3) % E]])


@pytest.mark.gpu
def test_comb():
    t = _comb(40)
    N = len(t.node_voxel)
    assert N == 82
    info = {}
    got = partitionCompartments(t.graph(), [([(0, 0, 0)], [])], info=info)
    _assert_equal_to_model(got, _model(t, [([0], [])]))
    print('comb of 40 junctions: depth rounds', info['depthRounds'], 'level rounds', info['levelRounds'])
    assert 1 <= info['depthRounds'] <= N + 1 and 1 <= info['levelRounds'] <= N + 1 and got.depthRounds == info['depthRounds']
    assert got.nodeLevel.max() == 41 and got.branchLevel.max() == 40
    # 255 compartments, one tooth each: from the tip; every other one shut in by its junction
    t = _comb(255)
    comps = [([10 * k + 16], [10 * k + 10] if k % 2 else []) for k in range(255)]
    got, m = _check(t, comps)
    assert (m['compartmentCounts'][1:, 0] > 0).all() and m['compartmentCounts'][0, 1] > 0 and len(set(got.branchCompartment.tolist())) > 128


@pytest.mark.gpu
def test_lists_and_counts():
    t = _two_components()
    got, m = _check(t, [([0], [])])                                       # no boundary: the whole component, the other one stays 0
    assert got.entryCompartment.tolist() == [1] * 11 + [0] * 11 and got.branchCompartment.tolist() == [1, 1, 1, 0, 0, 0]
    assert got.compartmentCounts.tolist() == [[9, 0, 3], [9, 9, 3]]
    got, m = _check(t, [([], []), ([0, 0, 2], [5, 5]), ([], [24])])       # empty lists, duplicates, an initial list that is empty
    assert got.compartmentCounts[1].tolist() == [0, 0, 0] and got.compartmentCounts[3].tolist() == [0, 0, 0] and got.compartmentCounts[2, 0] == 8
    got, m = _check(t, [([0], []), ([8], []), ([20], [24])])              # overlapping compartments
    assert got.compartmentCounts[0, 1] == 9 and got.compartmentCounts[0, 1] == m['compartmentCounts'][0, 1]
    empty = Tables((4, 5, 6), [0], [], np.zeros((0, 2), np.int64), [])
    got, m = _check(empty, [([], []), ([], [])])
    assert got.entryCompartment.shape == (0,) and got.nodeDepth.shape == (0,) and got.compartmentCounts.tolist() == [[0, 0, 0]] * 3


@pytest.mark.gpu
@pytest.mark.parametrize('density', sorted(RANDOM))
def test_random_volumes(density):
    t, comps, m = _random_case(density)
    got = partitionCompartments(t.graph(), _coords(t, comps))
    _assert_equal_to_model(got, m)
    again = partitionCompartments(t.graph(), _coords(t, comps))           # repeats are bit-identical
    for k in COMPARTMENT_ARRAYS:
        assert np.asarray(getattr(got, k)).tobytes() == np.asarray(getattr(again, k)).tobytes(), k


@pytest.mark.gpu
def test_kernel_equals_the_reference_on_a_tree():
    z, t, comps = _tree_case()
    for k, comp in enumerate(comps):
        got = partitionCompartments(t.graph(), _coords(t, [comp]))
        _assert_equals_the_recording(z, t, k, {name: getattr(got, name) for name in COMPARTMENT_ARRAYS})


CANARY = 119


def _raw(t, K, ioff, ivox, boff, bvox, shape=None):
    """vmask_compartments on host arrays, every output filled beforehand: (return code, message, the outputs)."""
    dll = S._skeleton_lib()
    B, N, E = len(t.offsets) - 1, len(t.node_voxel), len(t.voxels)
    i64 = lambda a: np.ascontiguousarray(a, np.int64)
    off, vox, ends, nodes, ioff, ivox, boff, bvox = (i64(a) for a in (t.offsets, t.voxels, t.ends, t.node_voxel, ioff, ivox, boff, bvox))
    outs = [np.full(k, CANARY, dt) for k, dt in ((E, np.uint8), (E, np.int64), (E, np.int64), (N, np.uint8), (N, np.int64), (N, np.int64), (B, np.uint8),
                                                 (B, np.int64), (3 * (max(K, 0) + 1), np.int64), (2, np.int64))]
    rc = dll.vmask_compartments(0, *(shape or t.shape), off.ctypes.data, B, vox.ctypes.data, ends.ctypes.data, nodes.ctypes.data, N, K, ioff.ctypes.data, ivox.ctypes.data,
                                boff.ctypes.data, bvox.ctypes.data, *(a.ctypes.data for a in outs))
    return rc, dll.vmask_last_error(), outs


@pytest.mark.gpu
def test_refused_inputs_leave_the_outputs_alone():
    t = _table(**LOLLIPOP, size=40)
    rc, msg, outs = _raw(t, 1, [0, 1], [0], [0, 1], [5])
    assert rc == 0 and outs[0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]  # the call as such is sound
    def mutant(**change):
        m = _table(**LOLLIPOP, size=40)
        for k, v in change.items():
            setattr(m, k, np.asarray(v, np.int64))
        return m
    refused = {
        'no compartment': (t, 0, [0], [], [0], []),
        '256 compartments': (t, 256, [0] * 257, [], [0] * 257, []),
        'offsets from 1': (t, 1, [1, 1], [0], [0, 0], []),
        'offsets descend': (t, 2, [0, 1, 0], [0], [0, 0, 0], []),
        'boundary offsets descend': (t, 2, [0, 0, 0], [], [0, 1, 0], [5]),
        'initial outside the volume': (t, 1, [0, 1], [40], [0, 0], []),
        'initial negative': (t, 1, [0, 1], [-1], [0, 0], []),
        'boundary outside the volume': (t, 1, [0, 1], [0], [0, 1], [1 << 40]),
        'no vertex': (t, 1, [0, 1], [0], [0, 1], [30]),
        'both lists': (t, 2, [0, 1, 3], [0, 2, 5], [0, 1, 2], [1, 5]),
        'a branch of one entry': (mutant(offsets=[0, 4, 5]), 1, [0, 1], [0], [0, 0], []),
        'a voxel outside the volume': (mutant(voxels=[0, 1, 40, 3, 3, 4, 5, 6, 7, 3]), 1, [0, 1], [0], [0, 0], []),
        'an end that is no node': (mutant(ends=[[0, 2], [1, 1]]), 1, [0, 1], [0], [0, 0], []),
        'half closed': (mutant(ends=[[0, 1], [-1, 1]]), 1, [0, 1], [0], [0, 0], []),
        'first entry is not the node': (mutant(voxels=[1, 1, 2, 3, 3, 4, 5, 6, 7, 3]), 1, [0, 1], [3], [0, 0], []),
        'last entry is not the node': (mutant(voxels=[0, 1, 2, 3, 3, 4, 5, 6, 7, 0]), 1, [0, 1], [3], [0, 0], []),
        'closed but open-ended': (mutant(ends=[[0, 1], [-1, -1]], voxels=[0, 1, 2, 3, 3, 4, 5, 6, 7, 8]), 1, [0, 1], [0], [0, 0], []),
    }
    for name, (table, K, ioff, ivox, boff, bvox) in refused.items():
        rc, msg, outs = _raw(table, K, ioff, ivox, boff, bvox)
        assert rc == -1 and msg, name
        assert all((a == CANARY).all() for a in outs), name
    rc, msg, outs = _raw(t, 1, [0, 1], [0], [0, 0], [], shape=(1, 1, 1 << 40))
    assert rc == -1 and all((a == CANARY).all() for a in outs)


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import test_compartments as T
t, comps, m = T._random_case(0.3)
v = T._random_volume(0.3)
dev = torch.device('cuda', 0)
gh, gd = S.branchGraph(v), S.branchGraph(torch.as_tensor(v, device=dev))
lists = T._coords(t, comps)
h, d = S.partitionCompartments(gh, lists), S.partitionCompartments(gd, lists)
T._assert_equal_to_model(h, m)
for name in S.COMPARTMENT_ARRAYS:
    a, b = getattr(d, name), getattr(h, name)
    assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape, name
    assert a.cpu().numpy().dtype == b.dtype and a.cpu().numpy().tobytes() == b.tobytes(), name
assert d.partitionInfo(gd) == h.partitionInfo(gh)
mask = torch.as_tensor(v, device=dev)
lh, sh = S.compartmentTerritories(v, gh, h)
ld, sd = S.compartmentTerritories(mask, gd, d)
assert ld.is_cuda and ld.dtype == torch.uint8 and np.array_equal(ld.cpu().numpy(), lh) and np.array_equal(sd.cpu().numpy(), sh)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_compartments_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_territories_of_a_y_phantom():
    from arterynetwork_amd.geodesic import geodesicDistance
    mask = _y_phantom()
    graph = S.branchGraph(S.skeletonize(mask))
    n1, n2 = mask.shape[1:]
    lin = lambda c: (c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2]
    t = Tables(mask.shape, graph.offsets, lin(graph.coords), graph.branchEnds, lin(graph.nodeCoords), graph.nodeKind, graph.nodeDegree)
    assert len(t.offsets) - 1 >= 3
    tips = t.node_voxel[t.kind == 0]
    comps = [([int(tips[0])], []), ([int(tips[-1])], []), ([int(tips[1])], [int(t.node_voxel[t.kind == 1][0])])]
    parts, m = _check(t, comps)
    spacing = (0.5, 0.5, 1.25)
    labels, sizes, distance = compartmentTerritories(mask, graph, parts, spacing=spacing, return_distance=True)
    own = m['entryCompartment'] > 0                                       # the model's seeds
    want_d, want_l, want_s = geodesicDistance(mask, t.voxels[own], labels=m['entryCompartment'][own].astype(np.int32), spacing=spacing, return_labels=True)
    assert labels.dtype == np.uint8 and labels.shape == mask.shape and sizes.dtype == np.int64 and sizes.shape == (4,)
    assert np.array_equal(labels, want_l) and np.array_equal(sizes[:want_s.size], want_s) and not sizes[want_s.size:].any() and np.array_equal(distance, want_d)
    assert sizes.sum() == np.count_nonzero(mask) and (sizes[1:] > 0).all()
    s = compartmentSummary(parts, sizes=sizes, affine=np.diag([0.5, 0.5, 1.25, 1.0]))
    assert [s[k]['volume'] for k in parts.names] == (sizes[1:] * 0.3125).tolist()


def _content(path):
    """What a file holds, without the time stamps of its container: a .gz unpacked, an .npz as its arrays, anything else as it is."""
    raw = path.read_bytes()
    if path.name.endswith('.gz'):
        return gzip.decompress(raw)
    if path.name.endswith('.npz'):
        with np.load(str(path), allow_pickle=True) as z:
            arrays = {k: z[k] for k in z.files}
        if 'countNames' in arrays:                                        # (branchGraph.npz: labelRounds describes the run and differs between two)
            arrays['counts'] = arrays['counts'][arrays['countNames'] != 'labelRounds']
        return {k: (a.dtype.str, a.shape, a.tobytes() if a.dtype != object else a.tolist()) for k, a in arrays.items()}
    return raw


@pytest.mark.gpu
def test_main_writes_the_files(tmp_path, capsys):
    from arterynetwork_amd import nifti
    m = M.crossing_phantom((48, 48, 32))
    m[10, 33:45, 15:17] = 1
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, parted = tmp_path / 'plain', tmp_path / 'parted'
    for d in (plain, parted):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    graph = S.branchGraph(S.skeletonize(m))
    tips = graph.nodeCoords[graph.nodeKind == 0]
    junction = graph.nodeCoords[graph.nodeKind == 1][0]
    chosen = {'LMCA': {'initialVoxels': [tuple(tips[0].tolist())], 'boundaryVoxels': [tuple(junction.tolist())]},
              'RMCA': {'initialVoxels': [tuple(tips[-1].tolist())], 'boundaryVoxels': []}}
    with open(str(tmp_path / 'chosenVoxelsForPartition.pkl'), 'wb') as f:
        pickle.dump(chosen, f, protocol=2)
    with pytest.raises(ValueError):
        S.main(str(parted), segments=True, compartments=chosen)
    before = S.main(str(plain), segments=True, territories=True, prune=(0, 0.0), morphometry=True, roots=[0])
    capsys.readouterr()
    after = S.main(str(parted), segments=True, territories=True, prune=(0, 0.0), morphometry=True, roots=[0], compartments=str(tmp_path / 'chosenVoxelsForPartition.pkl'))
    said = capsys.readouterr().out
    new = ['partitionInfo.pkl', 'compartments.npz', 'compartmentLabels.nii.gz']
    assert sorted(os.listdir(str(parted))) == sorted(os.listdir(str(plain)) + new)
    for name in os.listdir(str(plain)):                                   # every other file byte for byte, but the two that gain the names
        if name not in ('segmentInfoDict.pkl', 'nodeInfoDict.pkl'):
            assert _content(plain / name) == _content(parted / name), name
    for name in new:
        assert '{} saved to {}.'.format(name, os.path.join(str(parted), name)) in said
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
    want = partitionCompartments(graph, chosen)
    load = lambda d, name: pickle.load(open(str(d / name), 'rb'))
    assert load(parted, 'partitionInfo.pkl') == want.partitionInfo(graph) and set(load(parted, 'partitionInfo.pkl')) == {'LMCA', 'RMCA'}
    z = np.load(str(parted / 'compartments.npz'))
    assert z['names'].tolist() == ['LMCA', 'RMCA']
    for k in COMPARTMENT_ARRAYS:
        assert z[k].dtype == getattr(want, k).dtype and np.array_equal(z[k], getattr(want, k)), k
    _, stored = nifti.loadVolume(str(parted), 'vesselVolumeMask.nii.gz')
    spacing = np.sqrt((np.asarray(stored, np.float64)[:3, :3] ** 2).sum(axis=0))
    labels, sizes = compartmentTerritories(m, graph, want, spacing=spacing)
    got, _ = nifti.loadVolume(str(parted), 'compartmentLabels.nii.gz')
    assert np.asarray(got).dtype == np.uint8 and np.array_equal(got, labels) and np.array_equal(z['sizes'], sizes) and sizes.sum() == np.count_nonzero(m)
    assert z['volumes'] == pytest.approx(sizes * 0.4 * 0.4 * 0.6, rel=1e-6) and np.array_equal(z['summary_volume'], z['volumes'][1:])
    assert z['summary_branches'].tolist() == [int((want.branchCompartment == k).sum()) for k in (1, 2)] and {'summary_totalLength', 'summary_meanRadius', 'summary_maxLevel'} <= set(z.files)
    seg0, seg1, node0, node1 = load(plain, 'segmentInfoDict.pkl'), load(parted, 'segmentInfoDict.pkl'), load(plain, 'nodeInfoDict.pkl'), load(parted, 'nodeInfoDict.pkl')
    assert sorted(seg0) == sorted(seg1) and sorted(node0) == sorted(node1) and (want.branchCompartment > 0).any()
    for k, d in seg1.items():
        c = int(want.branchCompartment[k])
        base = dict(seg0[k])
        if c:
            base.update(partitionName=want.names[c - 1], segmentLevel=int(want.branchLevel[k]))
        assert d == base, k
    for v, c in enumerate(graph.nodeCoords.tolist()):
        base = dict(node0[tuple(c)])
        if want.nodeCompartment[v]:
            base['partitionName'] = want.names[int(want.nodeCompartment[v]) - 1]
        assert node1[tuple(c)] == base
    # a run without `compartments` writes what it always wrote
    again = tmp_path / 'again'
    again.mkdir()
    nifti.saveVolume(m, aff, str(again / 'vesselVolumeMask.nii.gz'))
    S.main(str(again), segments=True, territories=True, prune=(0, 0.0), morphometry=True, roots=[0], compartments=None)
    assert sorted(os.listdir(str(again))) == sorted(os.listdir(str(plain)))
    for name in os.listdir(str(plain)):
        assert _content(plain / name) == _content(again / name), name
