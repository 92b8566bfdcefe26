"""Branch graph ("f10 branch graph"): the sequential model tests/branch_model.py is checked for soundness
and against answers written out by hand on the CPU, then the GPU (vmask_branches / skeletonization.branchGraph) must equal it
exactly: the pruned skeleton, the node table, the branch ends, offsets, coordinates and every count but the labelling rounds."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

import branch_model as BM
import segment_model as SM
import skeleton_model as M
from conftest import ROOT

S26 = np.ones((3, 3, 3), bool)


# ------------------------------------------------------------------ the volumes
def _arm(v, start, step, length):
    """`length` voxels from start + step on; returns the last one."""
    p = np.array(start)
    for _ in range(length):
        p = p + step
        v[tuple(p)] = 1
    return tuple(int(c) for c in p)


def _star(lengths, shape=(14, 14, 14), centre=(6, 6, 6)):
    """One junction voxel with arms along space diagonals (their first voxels are no neighbours of each other)."""
    v = np.zeros(shape, np.uint8)
    v[centre] = 1
    for d, n in zip([(-1, -1, -1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)], lengths):
        _arm(v, centre, d, n)
    return v


def _clique2():
    """Two adjacent junction voxels a, b with two arms each (an X): the cluster {a, b}."""
    v = np.zeros((10, 9, 9), np.uint8)
    v[4, 4, 4] = v[5, 4, 4] = 1
    _arm(v, (4, 4, 4), (-1, -1, 0), 2); _arm(v, (4, 4, 4), (-1, 1, 0), 2)
    _arm(v, (5, 4, 4), (1, -1, 0), 2); _arm(v, (5, 4, 4), (1, 1, 0), 2)
    return v


def _triangle(lengths=(2, 2, 2)):
    """Three mutually adjacent junction voxels a, b, t with one arm each."""
    v = np.zeros((12, 12, 9), np.uint8)
    v[5, 5, 4] = v[6, 5, 4] = v[5, 6, 4] = 1
    _arm(v, (5, 5, 4), (-1, -1, 0), lengths[0]); _arm(v, (6, 5, 4), (1, -1, 0), lengths[1]); _arm(v, (5, 6, 4), (-1, 1, 0), lengths[2])
    return v


def _clique4():
    """A 2 x 2 square of junction voxels with one diagonal arm per corner."""
    v = np.zeros((10, 10, 5), np.uint8)
    v[4:6, 4:6, 2] = 1
    _arm(v, (4, 4, 2), (-1, -1, 0), 2); _arm(v, (4, 5, 2), (-1, 1, 0), 2); _arm(v, (5, 4, 2), (1, -1, 0), 2); _arm(v, (5, 5, 2), (1, 1, 0), 2)
    return v


def _tee():
    """A straight line with a perpendicular arm: the junction is a cluster of four voxels that is no clique."""
    v = np.zeros((11, 11, 3), np.uint8)
    v[0:11, 5, 1] = 1
    v[5, 6:11, 1] = 1
    return v


def _comb():
    """A backbone with four junction voxels that carry 1, 2, 3 and 4 teeth of two voxels along the diagonals of the cross plane."""
    v = np.zeros((45, 9, 9), np.uint8)
    v[:, 4, 4] = 1
    steps = [(0, 1, 1), (0, -1, -1), (0, 1, -1), (0, -1, 1)]
    for k, x in enumerate((8, 18, 28, 38)):
        for s in steps[:k + 1]:
            _arm(v, (x, 4, 4), s, 2)
    return v


def _free_ring():
    v = np.zeros((9, 9, 3), np.uint8)
    v[2, 3:6, 1] = v[6, 3:6, 1] = v[3:6, 2, 1] = v[3:6, 6, 1] = 1
    return v


def _loop_on_cluster():
    """The ring above with a tail: a loop that starts and ends in one cluster."""
    v = _free_ring()
    v[0:2, 4, 1] = 1
    return v


def _faces():
    """Objects on every face of the volume and in its corners."""
    v = np.zeros((7, 8, 9), np.uint8)
    v[0, :, 4] = v[6, :, 4] = v[:, 0, 2] = v[:, 7, 6] = v[3, :, 0] = v[3, 2, :] = v[:, 4, 8] = 1
    v[0, 0, 0] = v[6, 7, 8] = 1
    return v


def _bar(shape):
    return np.ones(shape, np.uint8)


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _dist_of(volume, value):
    """A case's `dist`: a number fills the volume, a function makes it from the volume."""
    return value(volume) if callable(value) else np.full(np.shape(volume), value, np.float64)


def _dist_but(at, there, elsewhere):
    """`there` at the voxel `at`, `elsewhere` everywhere else: a read at any other voxel lands on the other side of the bound."""
    def make(volume):
        d = np.full(np.shape(volume), elsewhere, np.float64)
        d[at] = there
        return d
    return make


def _dist_pattern(volume):
    """1, 1.5 .. 3 by raster index mod 5: neighbouring voxels differ, every product with 1.0 is exact."""
    return (1.0 + 0.5 * (np.arange(np.size(volume)) % 5)).reshape(np.shape(volume))


def _segments_case(name):
    import test_segments as TS
    return TS.CASES[name]()


# name -> (volume maker, keyword arguments of the model / of vmask_branches)
NO_PRUNE = dict(min_len=0, radius_factor=0.0, dist=None, max_rounds=64)
CASES = {}
for _n, _f in (('clique2', _clique2), ('clique3', _triangle), ('clique4', _clique4), ('tee', _tee), ('star-2-3-4', functools.partial(_star, (2, 3, 4))),
               ('comb', _comb), ('free-ring', _free_ring), ('loop-on-cluster', _loop_on_cluster), ('faces', _faces),
               ('empty', functools.partial(np.zeros, (4, 5, 6), np.uint8)), ('one-voxel', functools.partial(np.ones, (1, 1, 1), np.uint8)),
               ('extent-1x9x10', functools.partial(_random, (1, 9, 10), 0.5, 5)), ('extent-9x1x10', functools.partial(_random, (9, 1, 10), 0.5, 6)),
               ('extent-9x10x1', functools.partial(_random, (9, 10, 1), 0.5, 7)), ('extent-1x1x30', functools.partial(_random, (1, 1, 30), 0.7, 8)),
               ('diamond', functools.partial(_segments_case, 'ring-601x601x1')), ('diamond-tail', functools.partial(_segments_case, 'ring-tail-603x601x1')),
               ('eye', functools.partial(_segments_case, 'eye')), ('chains', functools.partial(_segments_case, 'chains')),
               ('cross', functools.partial(_segments_case, 'cross'))):
    CASES[_n] = (_f, NO_PRUNE)
for _d, _seed in ((0.1, 31), (0.3, 32), (0.6, 33)):
    CASES['random{}-12x13x14'.format(_d)] = (functools.partial(_random, (12, 13, 14), _d, _seed), NO_PRUNE)
    CASES['random{}-12x13x14-pruned'.format(_d)] = (functools.partial(_random, (12, 13, 14), _d, _seed), dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
# spur lengths exactly at the bound and one above it: by min_len, and by radius_factor * dist[rep] with an exact product
CASES['star-at-min-len'] = (functools.partial(_star, (3, 6, 6)), dict(min_len=3, radius_factor=0.0, dist=None, max_rounds=64))
CASES['star-above-min-len'] = (functools.partial(_star, (3, 6, 6)), dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
CASES['star-at-radius'] = (functools.partial(_star, (5, 6, 6)), dict(min_len=0, radius_factor=2.0, dist=2.5, max_rounds=64))
CASES['star-above-radius'] = (functools.partial(_star, (6, 6, 6)), dict(min_len=0, radius_factor=2.0, dist=2.5, max_rounds=64))
CASES['star-at-radius-3'] = (functools.partial(_star, (3, 6, 6)), dict(min_len=0, radius_factor=1.5, dist=2.0, max_rounds=64))
CASES['star-above-radius-3'] = (functools.partial(_star, (4, 6, 6)), dict(min_len=0, radius_factor=1.5, dist=2.0, max_rounds=64))
CASES['star-equal-spurs'] = (functools.partial(_star, (2, 2, 5)), dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
CASES['star-three-short'] = (functools.partial(_star, (2, 3, 4)), dict(min_len=10, radius_factor=0.0, dist=None, max_rounds=64))
CASES['triangle-three-short'] = (_triangle, dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
CASES['clique2-pruned'] = (_clique2, dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
CASES['clique4-pruned'] = (_clique4, dict(min_len=0, radius_factor=1.0, dist=2.0, max_rounds=64))
CASES['tee-pruned'] = (_tee, dict(min_len=5, radius_factor=0.0, dist=None, max_rounds=64))
CASES['comb-pruned'] = (_comb, dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=64))
CASES['comb-two-rounds'] = (_comb, dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=2))
CASES['comb-no-rounds'] = (_comb, dict(min_len=2, radius_factor=0.0, dist=None, max_rounds=0))
# dist that differs from voxel to voxel: the tee's three spurs have L = 4 and end at the voxels (4, 5, 1), (6, 5, 1) and at the
# representative (5, 6, 1) itself; only dist[rep] is on the pruning side of the bound (2.0 * 2.0 = 4 prunes, 2.0 * 1.75 = 3.5 does not)
CASES['tee-radius-at-rep'] = (_tee, dict(min_len=0, radius_factor=2.0, dist=_dist_but((5, 6, 1), 2.0, 1.0), max_rounds=64))
CASES['tee-radius-above-rep'] = (_tee, dict(min_len=0, radius_factor=2.0, dist=_dist_but((5, 6, 1), 1.75, 100.0), max_rounds=64))
CASES['random0.1-12x13x14-dist'] = (functools.partial(_random, (12, 13, 14), 0.1, 31), dict(min_len=0, radius_factor=1.0, dist=_dist_pattern, max_rounds=64))
CASES['random0.3-12x13x14-dist'] = (functools.partial(_random, (12, 13, 14), 0.3, 32), dict(min_len=0, radius_factor=1.0, dist=_dist_pattern, max_rounds=64))
BARS = {'bar-1x2x3000': (1, 2, 3000), 'bar-2x1x3000': (2, 1, 3000), 'bar-3000x2x1': (3000, 2, 1)}
for _n, _s in BARS.items():
    CASES[_n] = (functools.partial(_bar, _s), NO_PRUNE)
THIN = ('clique2', 'clique3', 'clique4', 'star-2-3-4', 'comb', 'free-ring', 'loop-on-cluster', 'diamond', 'diamond-tail', 'eye', 'chains', 'cross',
        'star-equal-spurs', 'star-three-short', 'triangle-three-short', 'comb-pruned')      # every branch ends at a representative itself


@functools.lru_cache(maxsize=None)
def _volume(case):
    v = CASES[case][0]()
    v.setflags(write=False)
    return v


def _params(case):
    v, kw = _volume(case), dict(CASES[case][1])
    if kw['dist'] is not None:
        kw['dist'] = _dist_of(v, kw['dist'])
    return kw


@functools.lru_cache(maxsize=None)
def _model(case):
    """The model's answer, computed once per case and shared."""
    sk, g = BM.branch_graph(_volume(case), **_params(case))
    for a in (sk, g.nodes, g.ends, g.offsets, g.voxels):
        a.setflags(write=False)
    return sk, g


def _components(volume):
    return ndimage.label(np.asarray(volume) != 0, structure=S26)[1]


# ------------------------------------------------------------------ CPU: the model itself
def _check_sound(sk, g, strict, nx):
    obj = sk.ravel() != 0
    deg = SM.degrees(sk).ravel()
    lab = ndimage.label((sk != 0) & (SM.degrees(sk) >= 3), structure=S26)[0].ravel()
    c = g.counts
    assert c['nodes'] == c['clusters'] + c['endPoints'] == len(g.nodes) and c['clusters'] == int(lab.max()) and c['endPoints'] == int((obj & (deg == 1)).sum())
    assert c['isolated'] == int((obj & (deg == 0)).sum()) and c['branches'] == len(g.ends) == len(g.offsets) - 1 and c['entries'] == len(g.voxels)
    assert (np.diff(g.nodes[:, 0]) > 0).all() and int(g.nodes[g.nodes[:, 1] == 1, 2].sum()) == int((lab > 0).sum())
    assert c['passThrough'] == int(((g.nodes[:, 1] == 1) & (g.nodes[:, 3] == 2)).sum())
    # every voxel: a cluster member, in exactly one branch, or isolated; every edge: inside a cluster or in exactly one branch
    times = np.zeros(obj.size, np.int64)
    edges_seen = []
    degree = np.zeros(len(g.nodes), np.int64)
    parent = list(range(len(g.nodes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for k, s in enumerate(g.seg):
        b = g.branches[k]
        assert len(s) >= 2 and b[int(b[0] != s[0]):len(b) - int(b[-1] != s[-1])] == list(s)
        inner = s[1:-1] if s[0] != s[-1] or deg[s[0]] != 2 else s[:-1]
        assert all(deg[p] == 2 for p in inner)
        np.add.at(times, np.array(inner, np.int64), 1)
        edges_seen.extend((min(p, q), max(p, q)) for p, q in zip(s[:-1], s[1:]))
        ea, eb = g.ends[k]
        if ea < 0:
            assert ea == eb == -1 and s[0] == s[-1] and deg[s[0]] == 2
            continue
        for e, v in ((ea, s[0]), (eb, s[-1])):
            degree[e] += 1
            rep = int(g.nodes[e, 0])
            assert deg[v] != 2 and (rep == v if g.nodes[e, 1] == 0 else lab[rep] == lab[v] > 0)
        assert b[0] == g.nodes[ea, 0] and b[-1] == g.nodes[eb, 0]
        parent[find(ea)] = find(eb)
    assert (times[obj & (deg == 2)] == 1).all() and times[~(obj & (deg == 2))].sum() == 0
    assert np.array_equal(degree, g.nodes[:, 3])
    import test_segments as TS
    all_edges = TS._edges(sk)
    inside = {(p, q) for p, q in all_edges if lab[p] > 0 and lab[p] == lab[q]}
    assert len(edges_seen) == len(set(edges_seen)) and set(edges_seen) == all_edges - inside
    assert c['droppedSegments'] == len(inside)
    # the contracted graph has the components of S, isolated voxels aside
    rings = int((g.ends[:, 0] < 0).sum()) if len(g.ends) else 0
    assert len({find(x) for x in range(len(g.nodes))}) + rings == _components(sk) - c['isolated']
    G = nx.Graph()
    for b in g.branches:
        nx.add_path(G, b)
    through = {int(r) for r, kind, _, d in g.nodes.tolist() if kind == 1 and d == 2}
    for b in g.branches:
        assert all(G.degree[p] == 2 or lab[p] > 0 for p in b[1:-1])
        if strict and (b[0] != b[-1] or deg[b[0]] != 2):
            assert all(G.degree[p] != 2 or p in through for p in (b[0], b[-1]))


@pytest.mark.parametrize('case', sorted(CASES))
def test_model_is_sound(case):
    """The networkx check: in the graph of the branches' paths every interior voxel has degree 2, but for the members of a cluster
    that are not its representative - such a voxel is interior to every branch that ends at it.  The end voxels (the
    representatives) have another degree, pass-through clusters aside; that half is checked on the thin cases only: in an
    unthinned volume two branches may leave a representative through the same member."""
    nx = pytest.importorskip('networkx')
    sk, g = _model(case)
    _check_sound(sk, g, case in THIN, nx)


def _lin(v, p):
    return int(np.ravel_multi_index(p, v.shape))


def test_known_junctions():
    # an X: the cluster {a, b} of two voxels, represented by a (equal degree, smaller index); b's arms get a in front
    v = _volume('clique2')
    sk, g = _model('clique2')
    a, b = _lin(v, (4, 4, 4)), _lin(v, (5, 4, 4))
    assert np.array_equal(sk, v) and g.counts == dict(nodes=5, clusters=1, endPoints=4, passThrough=0, branches=4, entries=14, isolated=0,
                                                      droppedSegments=1, pruneRounds=0, spursRemoved=0, voxelsRemoved=0)
    tips = [_lin(v, p) for p in ((2, 2, 4), (2, 6, 4), (7, 2, 4), (7, 6, 4))]
    assert g.nodes.tolist() == [[tips[0], 0, 1, 1], [tips[1], 0, 1, 1], [a, 1, 2, 4], [tips[2], 0, 1, 1], [tips[3], 0, 1, 1]]
    assert g.branches == [[tips[0], _lin(v, (3, 3, 4)), a], [tips[1], _lin(v, (3, 5, 4)), a],
                          [a, b, _lin(v, (6, 3, 4)), tips[2]], [a, b, _lin(v, (6, 5, 4)), tips[3]]]
    assert g.ends.tolist() == [[0, 2], [1, 2], [2, 3], [2, 4]]
    # a triangle of junction voxels: three segments inside the cluster are dropped, three branches of L = 2 stay
    v = _volume('clique3')
    sk, g = _model('clique3')
    assert g.counts['clusters'] == 1 and g.counts['droppedSegments'] == 3 and g.counts['branches'] == 3 and g.counts['entries'] == 3 + 4 + 4
    assert g.nodes[g.nodes[:, 1] == 1].tolist() == [[_lin(v, (5, 5, 4)), 1, 3, 3]]
    # a 2 x 2 square: six segments inside the cluster, four branches; a tee: four junction voxels, no clique, represented
    # by the arm's first voxel (degree 4)
    sk, g = _model('clique4')
    assert g.counts['clusters'] == 1 and g.counts['droppedSegments'] == 6 and g.counts['branches'] == 4 and g.nodes[g.nodes[:, 1] == 1, 2:].tolist() == [[4, 4]]
    v = _volume('tee')
    sk, g = _model('tee')
    assert g.nodes[g.nodes[:, 1] == 1].tolist() == [[_lin(v, (5, 6, 1)), 1, 4, 3]] and g.counts['droppedSegments'] == 5 and g.counts['branches'] == 3
    assert sorted(len(b) for b in g.branches) == [5, 6, 6]               # the two halves of the line get the representative attached
    # a free ring is a branch without nodes; a loop on a cluster counts twice at its node
    sk, g = _model('free-ring')
    assert g.ends.tolist() == [[-1, -1]] and g.counts['nodes'] == 0 and g.branches[0][0] == g.branches[0][-1]
    sk, g = _model('loop-on-cluster')
    loops = [k for k, e in enumerate(g.ends.tolist()) if e[0] == e[1]]
    assert len(loops) == 1 and g.nodes[g.ends[loops[0], 0], 3] == 3 and g.counts['endPoints'] == 1


def test_known_pruning():
    # two spurs of L = 2 on one junction voxel: the one of smaller branch index goes, the other continues the long arm
    v = _volume('star-equal-spurs')
    sk, g = _model('star-equal-spurs')
    want = v.copy(); want[5, 5, 5] = want[4, 4, 4] = 0
    assert np.array_equal(sk, want)
    assert g.counts == dict(nodes=2, clusters=0, endPoints=2, passThrough=0, branches=1, entries=8, isolated=0, droppedSegments=0,
                            pruneRounds=1, spursRemoved=1, voxelsRemoved=2)
    assert g.branches == [[_lin(v, p) for p in ((4, 8, 8), (5, 7, 7), (6, 6, 6), (7, 7, 7), (8, 8, 8), (9, 9, 9), (10, 10, 10), (11, 11, 11))]]
    # a star of three short arms (2, 3, 4): the shortest goes, the next build finds no junction - the longest path stays
    v = _volume('star-three-short')
    sk, g = _model('star-three-short')
    want = v.copy(); want[5, 5, 5] = want[4, 4, 4] = 0
    assert np.array_equal(sk, want) and g.counts['pruneRounds'] == 1 and g.counts['spursRemoved'] == 1 and g.counts['branches'] == 1 and len(g.branches[0]) == 8
    # a triangle cluster with three arms of L = 2: the first arm goes, its corner is thinned away, a path is left - no ring
    v = _volume('triangle-three-short')
    sk, g = _model('triangle-three-short')
    want = v.copy(); want[5, 5, 4] = want[4, 4, 4] = want[3, 3, 4] = 0
    assert np.array_equal(sk, want)
    assert g.counts == dict(nodes=2, clusters=0, endPoints=2, passThrough=0, branches=1, entries=6, isolated=0, droppedSegments=0,
                            pruneRounds=1, spursRemoved=1, voxelsRemoved=2)
    # the bounds: L == min_len goes, L == min_len + 1 stays; L == radius_factor * dist goes, one more stays
    for at, above in (('star-at-min-len', 'star-above-min-len'), ('star-at-radius', 'star-above-radius'), ('star-at-radius-3', 'star-above-radius-3')):
        assert _model(at)[1].counts['spursRemoved'] == 1 and _model(at)[1].counts['clusters'] == 0
        assert _model(above)[1].counts['spursRemoved'] == 0 and np.array_equal(_model(above)[0], _volume(above))
    # dist is read at the cluster's representative, not at the spur's own end voxel or anywhere else
    sk, g = _model('tee-radius-at-rep')
    assert g.counts['spursRemoved'] == 1 and g.counts['pruneRounds'] == 1 and g.counts['voxelsRemoved'] == 4 and g.counts['clusters'] == 0
    assert _model('tee-radius-above-rep')[1].counts['spursRemoved'] == 0 and np.array_equal(_model('tee-radius-above-rep')[0], _volume('tee'))
    assert _model('random0.1-12x13x14-dist')[1].counts['spursRemoved'] > 0 and _model('random0.3-12x13x14-dist')[1].counts['spursRemoved'] > 0
    # the comb: its four junctions carry 1 .. 4 teeth, one tooth per junction and round
    assert _model('comb-pruned')[1].counts['pruneRounds'] == 4 and _model('comb-pruned')[1].counts['spursRemoved'] == 10
    assert _model('comb-two-rounds')[1].counts['pruneRounds'] == 2 and _model('comb-two-rounds')[1].counts['spursRemoved'] == 4 + 3
    assert _model('comb-no-rounds')[1].counts['pruneRounds'] == 0 and np.array_equal(_model('comb-no-rounds')[0], _volume('comb'))
    assert _components(_model('comb-pruned')[0]) == 1


HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
KERNELS = ('k_seg_count', 'k_seg_compact', 'k_br_binary', 'k_br_gather', 'k_br_adjacent', 'k_br_hook', 'k_br_members', 'k_br_classify', 'k_br_clear',
           'k_br_nodes', 'k_br_nodeid', 'k_br_emit')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_branch_kernels_use_no_scratch(tmp_path):
    from arterynetwork_amd import build
    assert 'vbr_device.hip' in build.SOURCES
    out = tmp_path / 'vbr_device.s'
    p = subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', '-o', str(out), 'vbr_device.hip'],
                       cwd=os.path.join(ROOT, 'arterynetwork_amd', 'csrc'), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    recs = {}
    for m in re.finditer(r'\.name:\s+(\S+)\n(.*?)\.wavefront_size', out.read_text(), re.S):      # the metadata records only
        recs[m.group(1)] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', m.group(2)).group(1))
    for frag in KERNELS:
        assert sum(frag in k for k in recs) == 1, 'kernel not found: ' + frag
    for name, scratch in recs.items():                                   # (the library's scan kernels included)
        assert scratch == 0, '%s uses %d bytes of scratch per thread' % (name, scratch)


# ------------------------------------------------------------------ GPU: exactly the model
def _lin_of(coords, shape):
    c = np.asarray(coords).reshape(-1, 3)
    return np.ravel_multi_index(c.T, shape) if len(c) else np.zeros(0, np.int64)


def _assert_equal_to_model(got, sk, g, shape):
    assert got.skeleton.dtype == np.uint8 and np.array_equal(got.skeleton, sk)
    for a in (got.nodeCoords, got.nodeKind, got.nodeSize, got.nodeDegree, got.branchEnds, got.offsets, got.coords):
        assert a.dtype == np.int64
    assert got.nodeCoords.shape == (len(g.nodes), 3) and got.coords.shape == (len(g.voxels), 3) and got.branchEnds.shape == (len(g.ends), 2)
    assert np.array_equal(_lin_of(got.nodeCoords, shape), g.nodes[:, 0]) and np.array_equal(got.nodeKind, g.nodes[:, 1])
    assert np.array_equal(got.nodeSize, g.nodes[:, 2]) and np.array_equal(got.nodeDegree, g.nodes[:, 3])
    assert np.array_equal(got.branchEnds, g.ends) and np.array_equal(got.offsets, g.offsets) and np.array_equal(_lin_of(got.coords, shape), g.voxels)
    assert {k: got.counts[k] for k in BM.COUNTS} == g.counts


def _run(case, **extra):
    from arterynetwork_amd.skeletonization import branchGraph
    kw = _params(case)
    return branchGraph(_volume(case), minSpurLength=kw['min_len'], radiusFactor=kw['radius_factor'], dist=kw['dist'], maxRounds=kw['max_rounds'], **extra)


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_branches_equal_the_model(case):
    got = _run(case)
    sk, g = _model(case)
    print(case, got.counts)
    _assert_equal_to_model(got, sk, g, _volume(case).shape)
    if case in BARS:                                                     # one cluster of 6000 voxels: plain minimum propagation needs about 3000 rounds
        assert g.nodes[0, 2] == 6000
        assert g.counts['clusters'] == 1 and 1 <= got.counts['labelRounds'] <= 64


@pytest.mark.gpu
def test_branches_deterministic_and_idempotent():
    case = 'random0.1-12x13x14-pruned'                                    # (five pruning rounds by the model; the dense volumes have no end point to prune)
    a, b = _run(case), _run(case)
    for x, y in zip((a.skeleton, a.nodeCoords, a.nodeKind, a.nodeSize, a.nodeDegree, a.branchEnds, a.offsets, a.coords),
                    (b.skeleton, b.nodeCoords, b.nodeKind, b.nodeSize, b.nodeDegree, b.branchEnds, b.offsets, b.coords)):
        assert x.tobytes() == y.tobytes()
    assert a.counts['spursRemoved'] == _model(case)[1].counts['spursRemoved'] > 0 and a.counts['pruneRounds'] > 1


def _bumpy_tubes(shape=(96, 96, 64)):
    """Four wiggling tubes along axis 0 with one-voxel-wide bumps on their surface."""
    x = np.arange(shape[0], dtype=np.float32)[:, None, None]
    y = np.arange(shape[1], dtype=np.float32)[None, :, None]
    z = np.arange(shape[2], dtype=np.float32)[None, None, :]
    m = np.zeros(shape, bool)
    k = 0
    for cy in (26, 68):
        for cz in (18, 46):
            r = 2.5 + 0.75 * k
            yy = cy + 6 * np.sin(2 * np.pi * x / shape[0] * (1 + k % 3)); zz = cz + 4 * np.cos(2 * np.pi * x / shape[0] * 2)
            m |= ((y - yy) ** 2 + (z - zz) ** 2) <= r * r
            for bx in range(8 + 3 * k, shape[0] - 8, 17):                 # a bump: a short rod standing on the surface
                by, bz = int(round(float(yy[bx, 0, 0]))), int(round(float(zz[bx, 0, 0])))
                m[bx, by:by + int(r) + 4, bz] = True
            k += 1
    return m.astype(np.uint8)


@pytest.mark.gpu
def test_branches_end_to_end():
    from arterynetwork_amd import skeletonization as S
    mask = _bumpy_tubes()
    sk0 = S.skeletonize(mask)
    dist = S._G.distance_transform_edt(mask)
    raw = S.branchGraph(sk0)
    assert np.array_equal(raw.skeleton, sk0) and raw.counts['pruneRounds'] == 0
    got = S.branchGraph(sk0, minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=mask)
    sk, g = BM.branch_graph(sk0, 3, 1.0, dist, 64)
    print('raw', raw.counts, 'pruned', got.counts)
    _assert_equal_to_model(got, sk, g, mask.shape)
    assert g.counts['spursRemoved'] > 0 and got.counts['endPoints'] < raw.counts['endPoints']
    again = S.branchGraph(got.skeleton, minSpurLength=3, radiusFactor=1.0, dist=dist)
    assert again.counts['spursRemoved'] == 0 and again.counts['pruneRounds'] == 0 and np.array_equal(again.skeleton, got.skeleton)
    assert np.array_equal(again.coords, got.coords) and np.array_equal(again.branchEnds, got.branchEnds)
    assert np.array_equal(S.skeletonize(got.skeleton), got.skeleton)
    assert _components(got.skeleton) == _components(sk0)
    assert S.branchSegments(got) == [[tuple(p) for p in got.coords[a:b].tolist()] for a, b in zip(got.offsets[:-1], got.offsets[1:])]


@pytest.mark.gpu
def test_branches_capacity_protocol_and_errors():
    from arterynetwork_amd import skeletonization as S
    dll = S._skeleton_lib()
    case = 'random0.3-12x13x14'
    v = np.ascontiguousarray(_volume(case))
    sk, g = _model(case)
    nn, nb, total = len(g.nodes), len(g.ends), len(g.voxels)
    call = lambda vol, min_len, rf, dist, rounds, out, cnt, nodes, cn, ends, off, cb, vox, cv: dll.vmask_branches(
        0, vol, *v.shape, min_len, rf, dist, rounds, out, cnt, nodes, cn, ends, off, cb, vox, cv)
    only = np.full(12, -1, np.int64)
    out = np.full(v.shape, 9, np.uint8)
    assert call(v.ctypes.data, 0, 0.0, None, 64, out.ctypes.data, only.ctypes.data, None, 0, None, None, 0, None, 0) == 0
    assert np.array_equal(out, sk) and [int(c) for c in only[:11]] == [g.counts[k] for k in BM.COUNTS]
    CANARY = -77
    for cn, cb, cv, rc_want in ((nn, nb, total, 0), (nn - 1, nb, total, -1), (nn, nb - 1, total, -1), (nn, nb, total - 1, -1)):
        cnt = np.full(12, -1, np.int64)
        nodes, ends, off, vox = (np.full(k, CANARY, np.int64) for k in (4 * nn + 1, 2 * nb + 1, nb + 2, total + 1))
        out = np.full(v.shape, 9, np.uint8)
        rc = call(v.ctypes.data, 0, 0.0, None, 64, out.ctypes.data, cnt.ctypes.data, nodes.ctypes.data, cn, ends.ctypes.data, off.ctypes.data, cb, vox.ctypes.data, cv)
        assert rc == rc_want and np.array_equal(cnt[:11], only[:11])      # the needed sizes either way
        if rc_want:
            assert all((a == CANARY).all() for a in (nodes, ends, off, vox)) and (out == 9).all() and b'capacity' in dll.vmask_last_error()
        else:
            assert np.array_equal(nodes[:-1].reshape(nn, 4), g.nodes) and np.array_equal(ends[:-1].reshape(nb, 2), g.ends)
            assert np.array_equal(off[:-1], g.offsets) and np.array_equal(vox[:-1], g.voxels) and np.array_equal(out, sk)
            assert nodes[-1] == ends[-1] == off[-1] == vox[-1] == CANARY
    cnt = np.full(12, -1, np.int64)
    args = (out.ctypes.data, cnt.ctypes.data, None, 0, None, None, 0, None, 0)
    assert call(v.ctypes.data, -1, 0.0, None, 64, *args) == -1 and b'min_len' in dll.vmask_last_error()
    assert call(v.ctypes.data, 0, -0.5, None, 64, *args) == -1 and b'radius_factor' in dll.vmask_last_error()
    assert call(v.ctypes.data, 0, float('inf'), None, 64, *args) == -1 and call(v.ctypes.data, 0, float('nan'), None, 64, *args) == -1
    assert call(v.ctypes.data, 0, 0.0, None, -1, *args) == -1
    assert call(None, 0, 0.0, None, 64, *args) == -1 and call(v.ctypes.data, 0, 0.0, None, 64, out.ctypes.data, None, None, 0, None, None, 0, None, 0) == -1
    some = np.zeros(8, np.int64)
    assert call(v.ctypes.data, 0, 0.0, None, 64, out.ctypes.data, cnt.ctypes.data, some.ctypes.data, 1, None, None, 0, None, 0) == -1   # all four or none
    assert (cnt == -1).all()
    buf = np.zeros(8, np.uint8)
    assert dll.vmask_branches(0, buf.ctypes.data, 2000, 2000, 600, 0, 0.0, None, 64, None, cnt.ctypes.data, None, 0, None, None, 0, None, 0) == -1
    assert b'shape' in dll.vmask_last_error()
    with pytest.raises(ValueError):
        S.branchGraph(np.ones((8, 8), np.uint8))
    with pytest.raises(ValueError):
        S.branchGraph(v, radiusFactor=1.0, dist=np.ones((2, 2, 2)))
    # an empty volume: nothing, offsets[0] = 0
    e = S.branchGraph(np.zeros((4, 5, 6), np.uint8), minSpurLength=3)
    assert e.offsets.tolist() == [0] and len(e.coords) == 0 and len(e.nodeKind) == 0 and not e.skeleton.any() and S.branchSegments(e) == []


DEVICE_RESIDENT_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np
import torch                      # before the HIP library: one ROCm runtime per process (INTEGRATION.md)
from arterynetwork_amd import skeletonization as S
import test_branches as T
case = 'random0.3-12x13x14-dist'
v = T._volume(case)
dist = T._params(case)['dist']                                      # (differs from voxel to voxel)
dev = torch.device('cuda', 0)
h = S.branchGraph(v, minSpurLength=1, radiusFactor=1.0, dist=dist)
d = S.branchGraph(torch.as_tensor(v * 255, device=dev), minSpurLength=1, radiusFactor=1.0, dist=torch.as_tensor(dist, device=dev))
m = S.branchGraph(torch.as_tensor(v, device=dev), minSpurLength=1, radiusFactor=1.0, dist=dist)          # (a host dist beside a device volume)
sk, g = T.BM.branch_graph(v, 1, 1.0, dist, 64)
assert g.counts['spursRemoved'] > 0 and np.array_equal(h.skeleton, sk) and {{k: h.counts[k] for k in T.BM.COUNTS}} == g.counts
for g in (d, m):
    for name in ('skeleton', 'nodeCoords', 'nodeKind', 'nodeSize', 'nodeDegree', 'branchEnds', 'offsets', 'coords'):
        a, b = getattr(g, name), getattr(h, name)
        assert a.is_cuda and a.device == dev and tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b), name
    assert {{k: g.counts[k] for k in T.BM.COUNTS}} == {{k: h.counts[k] for k in T.BM.COUNTS}}
assert d.skeleton.dtype == torch.uint8 and d.coords.dtype == torch.int64
assert S.branchSegments(d) == S.branchSegments(h)
print('DEVICE RESIDENT OK')
"""


@pytest.mark.gpu
def test_branches_device_resident():
    """Tensors on the GPU go in by their device pointers and tensors on the same device come out, equal to the host call.
    Own process: torch is imported before the HIP library there."""
    script = DEVICE_RESIDENT_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, 'tests'))
    out = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'DEVICE RESIDENT OK' in out.stdout, out.stdout[-1500:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_branches_main_writes_the_files(tmp_path, capsys):
    nx = pytest.importorskip('networkx')
    from arterynetwork_amd import nifti, skeletonization as S
    m = M.crossing_phantom()
    m[24, 20:27, 16] = 1                                                  # a rod through the tube's surface: a spur of the skeleton
    aff = np.array([[0.4, 0, 0, -10.0], [0, 0.4, 0, 3.0], [0, 0, 0.6, 7.5], [0, 0, 0, 1.0]])
    plain, pruned = tmp_path / 'plain', tmp_path / 'pruned'
    for d in (plain, pruned):
        d.mkdir()
        nifti.saveVolume(m, aff, str(d / 'vesselVolumeMask.nii.gz'))
    sk0, segs0 = S.main(str(plain), segments=True)
    # without `prune`: the files of before, byte for byte what saveSegmentList writes for the traced skeleton
    assert sorted(os.listdir(str(plain))) == ['graphRepresentation.graphml', 'segmentList.npz', 'skeleton.nii.gz', 'vesselVolumeMask.nii.gz']
    S.saveSegmentList(S.traceSegments(S.skeletonize(m)), str(tmp_path / 'expected.npz'))
    assert (plain / 'segmentList.npz').read_bytes() == (tmp_path / 'expected.npz').read_bytes()
    capsys.readouterr()
    sk, segs, labels, sizes = S.main(str(pruned), segments=True, territories=True, prune=(3, 1.0))
    said = capsys.readouterr().out
    for name in ('skeleton.nii.gz', 'graphRepresentation.graphml', 'segmentList.npz', 'branchGraph.npz', 'segmentLabels.nii.gz', 'segmentTerritories.npz'):
        assert os.path.exists(str(pruned / name)) and '{} saved to {}.'.format(name, os.path.join(str(pruned), name)) in said
    want = S.branchGraph(sk0, minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=m)
    stored, _ = nifti.loadVolume(str(pruned), 'skeleton.nii.gz')
    assert np.array_equal(sk, want.skeleton) and np.array_equal(stored, sk) and segs == S.branchSegments(want)
    assert want.counts['spursRemoved'] > 0 and int(sk.sum()) < int(sk0.sum()) and len(segs) < len(segs0)
    tables = np.load(str(pruned / 'branchGraph.npz'))
    for name in ('nodeCoords', 'nodeKind', 'nodeSize', 'nodeDegree', 'branchEnds', 'offsets', 'coords'):
        assert np.array_equal(tables[name], getattr(want, name))
    stored_counts = dict(zip(tables['countNames'].tolist(), tables['counts'].tolist()))
    assert set(stored_counts) == set(want.counts) and all(stored_counts[k] == want.counts[k] for k in BM.COUNTS)      # (labelRounds describes the run)
    assert len(sizes) == len(segs) + 1 and int(sizes.sum()) == int(m.sum()) and labels.shape == m.shape
    # what the later stages do with the list: the graph of its paths has interior voxels of degree 2 and branch ends of another degree
    back = np.load(str(pruned / 'segmentList.npz'), allow_pickle=True)['segmentList']
    assert [list(s) for s in back] == segs
    G = nx.Graph()
    for k, seg in enumerate(back):
        nx.add_path(G, seg, segmentIndex=k)
    through = {tuple(c) for c, kind, d in zip(want.nodeCoords.tolist(), want.nodeKind.tolist(), want.nodeDegree.tolist()) if kind == 1 and d == 2}
    for seg, (ea, eb) in zip(back, want.branchEnds.tolist()):
        assert all(G.degree[p] == 2 for p in seg[1:-1])
        assert ea < 0 or all(G.degree[p] != 2 or p in through for p in (seg[0], seg[-1]))
    assert set(nx.read_graphml(str(pruned / 'graphRepresentation.graphml')).nodes) == {str(p) for p in G.nodes}
