#!/usr/bin/env python3
"""Record the reference's own branch morphometry on small trees, for tests/test_morphometry_reference.py.

Runs only where the reference is at hand (it never ships):
    python tests/golden/make_morphometry_goldens.py <the reference's Code directory>
Three functions are imported from the reference as they are and run one after the other, the way its pipeline does:
manualCorrectionGUI.calculateBranchInfo (per-branch lengths and radii, the graph), myFunctions.randomWalkBFS from the roots with no
boundary (depthVoxel, depthLevel, pathDistance) and graphRelated.calculateProperty (segmentInfoDict, nodeInfoDict).  Every module
they import and this machine lacks becomes an empty stand-in that may also serve as a base class; networkx 3 is given back the
``G.node`` and ``G.add_path`` of networkx 1 on ``nx.Graph`` itself, because the reference builds its graphs with ``nx.Graph()``.
The distance transform is written as vesselVolumeDistanceTransform.npz into a temporary directory, where calculateBranchInfo
finds it.

The cases (each a tree in a 44 x 44 x 48 volume; tubes of radius 1 .. 3 are painted around the branches and `dist` is scipy's
Euclidean distance transform of that mask):
  straight   axis-parallel, face-diagonal and space-diagonal branches, every step class; three chained bifurcations
  curved     the same topology with a helix of more than 20 entries, an arc of 18 entries and a shorter arc
  short      a two-entry branch between two junctions and a three-entry branch at a tabulated bifurcation
  two-roots  the walk starts from two end points that are equally many voxels from the node between them
Every case holds a branch between two tabulated bifurcations and a terminating branch and has more than 50 graph voxels:
calculateProperty returns nothing, or raises in its closing report, otherwise.  Every consecutive pair is 26-adjacent.

Output (data only): tests/golden/morphometry/<case>.npz
  shape, offsets, voxels, ends, node_voxel, node_kind, roots     the branch table (f10's layout) and the root node indices
  dist                          the distance transform at `voxels` (the test scatters it into a zero volume)
  seg_keys, seg_has, seg_<key>  per branch: which keys of segmentInfoDict the reference wrote, and their values (type: 0 / 1 for
                                'terminating' / 'bifurcating'; NaN or -1 where the key is absent)
  node_keys, node_has, node_<key>   the same per node voxel of nodeInfoDict (radiusList and normalVector are N x 3)
  entry_depthVoxel, entry_depthLevel, entry_pathDistance     the walk's three attributes at every entry of `voxels`
  ref_order                     N x 3 branch indices (child, child, parent) as the reference ordered them, -1 where untabulated
  straight_branch               per branch: all its steps are the same
  exact_<q>, refdist_<q>        per node (torque: per branch) for the angles and normalVector: the reference's formulas evaluated in
                                np.longdouble from the integer coordinates, in the reference's branch order, rounded to double, and the
                                distance of the reference's own value from it.  A local quantity has one only where the three
                                branches are straight (the step is then the direction); NaN elsewhere.
Asserted while recording: every angle that is not 0, 90 or 180 degrees by construction lies between 10 and 170 degrees."""
import contextlib
import importlib.abc
import importlib.machinery
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (44, 44, 48)
LD = np.longdouble
SEG_FLOAT = ('pathLength', 'eculideanLength', 'tortuosity', 'meanRadius', 'sigma', 'aspectRatio', 'localBifurcationTorque')
SEG_INT = ('voxelLength', 'type', 'segmentLevel')
SEG_OTHER = ('partitionName',)                                            # (never written here: no partition)
NODE_FLOAT = ('pathDistance', 'radius', 'localBifurcationAmplitude', 'remoteBifurcationAmplitude', 'localBifurcationTilt', 'remoteBifurcationTilt',
              'cubicLawResult', 'squareLawResult', 'minRadius', 'minRadiusRatio', 'maxRadiusRatio', 'lengthRatio')
NODE_INT = ('depthVoxel', 'depthLevel', 'type')
NODE_VEC = ('radiusList', 'normalVector')
NODE_OTHER = ('partitionName',)
ANGLES = ('localBifurcationAmplitude', 'remoteBifurcationAmplitude', 'localBifurcationTilt', 'remoteBifurcationTilt')
TYPE_CODE = {'terminating': 0, 'bifurcating': 1}


# ------------------------------------------------------------------ the trees
def lin(p):
    return (p[0] * SHAPE[1] + p[1]) * SHAPE[2] + p[2]


def line(a, step, n):
    """n steps of `step` from a: n + 1 voxels."""
    return [tuple(int(a[k] + i * step[k]) for k in range(3)) for i in range(n + 1)]


def curve(f, t0, t1, first=None, last=None):
    """The voxels that f(t), t0 <= t <= t1, passes through: sampled finely, rounded, no voxel twice in a row, corners cut (a voxel
    whose two neighbours along the curve are 26-adjacent is dropped), pinned to `first` and `last`."""
    pts = []
    for t in np.linspace(t0, t1, 4001):
        p = tuple(int(round(float(c))) for c in f(t))
        if not pts or p != pts[-1]:
            pts.append(p)
    if first is not None:
        assert pts[0] == tuple(first), (pts[0], first)
    if last is not None:
        assert pts[-1] == tuple(last), (pts[-1], last)
    k = 1
    while k < len(pts) - 1:
        if max(abs(a - b) for a, b in zip(pts[k - 1], pts[k + 1])) <= 1:
            del pts[k]
            k = max(k - 1, 1)
        else:
            k += 1
    return pts


def arc(start, u, v, radius, angle):
    """From `start` along a circle of `radius` in the plane of the unit vectors u (the first direction) and v (towards the centre)."""
    s, u, v = (np.asarray(x, np.float64) for x in (start, u, v))
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    return lambda t: s + radius * (np.sin(t) * u + (1 - np.cos(t)) * v), 0.0, angle


def helix(start, axis, u, v, radius, pitch, turns):
    """Around the line through start - radius u along `axis`: u and v span the plane across it."""
    s, a, u, v = (np.asarray(x, np.float64) for x in (start, axis, u, v))
    return lambda t: s + radius * ((np.cos(t) - 1) * u + np.sin(t) * v) + pitch * t / (2 * np.pi) * a, 0.0, 2 * np.pi * turns


def straight_tree():
    R, J1 = (2, 20, 20), (14, 20, 20)
    a = line(R, (1, 0, 0), 12)                                            # class (1, 0, 0)
    b = line(J1, (1, 1, 0), 10)                                           # (1, 1, 0) to J2 = (24, 30, 20)
    c = line(J1, (1, -1, 1), 9)                                           # (1, 1, 1) to an end point
    J2 = b[-1]
    d = line(J2, (0, 0, 1), 12)                                           # (0, 0, 1) to an end point
    e = line(J2, (1, 0, -1), 8)                                           # (1, 0, 1) to J3 = (32, 30, 12)
    J3 = e[-1]
    f = line(J3, (0, 1, 0), 10)                                           # (0, 1, 0) to an end point
    g = line(J3, (0, -1, -1), 8)                                          # (0, 1, 1) to an end point
    return [a, b, c, d, e, f, g], [R], [2.0, 2.0, 1.0, 3.0, 2.0, 1.0, 1.0]


def curved_tree():
    R, J1 = (2, 20, 20), (12, 20, 20)
    a = line(R, (1, 0, 0), 10)
    b = line(J1, (1, 1, 0), 7)                                            # straight to J2 = (19, 27, 20)
    c = line(J1, (1, -1, 1), 8)                                           # straight to an end point: J1's three branches are straight
    J2 = b[-1]
    d = curve(*helix(J2, (0, 0, 1), (0, -1, 0), (1, 0, 0), 4.0, 9.0, 2.0), first=J2)               # a helix upwards: more than 20 entries
    e = curve(*arc(J2, (1, 0, -1), (0, 1, 0), 14.0, 0.5 * np.pi), first=J2)                            # a quarter circle to J3
    J3 = e[-1]
    f = curve(*arc(J3, (1, 0, 0), (0, 0, 1), 7.0, 0.4 * np.pi), first=J3)                            # a shorter arc to an end point
    g = line(J3, (0, -1, -1), 8)
    assert len(d) > 20 and len(e) in (18, 19), (len(d), len(e))
    return [a, b, c, d, e, f, g], [R], [2.0, 2.0, 1.0, 3.0, 2.0, 1.0, 1.0]


def short_tree():
    R, J3 = (2, 8, 8), (10, 8, 8)
    a = line(R, (1, 0, 0), 8)
    b = line(J3, (0, -1, 1), 6)                                           # an end point
    c = line(J3, (1, 1, 0), 8)                                            # to J4 = (18, 16, 8)
    J4 = c[-1]
    d = line(J4, (0, 0, -1), 2)                                           # THREE entries, an end point: J4 stays tabulated
    e = line(J4, (0, 1, 1), 9)                                            # to J1 = (18, 25, 17)
    J1 = e[-1]
    f = line(J1, (-1, 0, 1), 8)                                           # an end point
    g = line(J1, (1, 1, 1), 1)                                            # TWO entries, to J2 = (19, 26, 18)
    J2 = g[-1]
    h = line(J2, (1, 0, 0), 10)                                           # an end point
    i = line(J2, (0, 1, 1), 9)                                            # an end point
    return [a, b, c, d, e, f, g, h, i], [R], [3.0, 1.0, 2.0, 1.0, 2.0, 1.0, 2.0, 3.0, 1.0]


def two_roots_tree():
    M = (20, 20, 20)
    a = line(M, (-1, 1, 0), 8)                                            # to the FIRST root: eight voxels away, 8 sqrt(2) long
    b = line(M, (-1, 0, 0), 8)                                            # to the SECOND root: eight voxels away, 8 long
    c = line(M, (1, 0, 1), 9)                                             # to J2 = (29, 20, 29)
    J2 = c[-1]
    d = line(J2, (0, 1, 0), 10)
    e = line(J2, (1, -1, 0), 8)                                           # to J3 = (37, 12, 29)
    J3 = e[-1]
    f = line(J3, (0, 0, 1), 10)
    g = line(J3, (0, -1, -1), 8)
    return [a, b, c, d, e, f, g], [a[-1], b[-1]], [2.0, 2.0, 3.0, 1.0, 2.0, 1.0, 1.0]


CASES = (('straight', straight_tree), ('curved', curved_tree), ('short', short_tree), ('two-roots', two_roots_tree))


def table(paths):
    """f10's layout: a branch runs from its end of smaller raster index, the branches ascend by (first, second) voxel, the nodes by
    raster index.  Returns the branches and the position of every given path among them."""
    oriented = [p if lin(p[0]) < lin(p[-1]) else p[::-1] for p in paths]
    order = sorted(range(len(paths)), key=lambda k: (lin(oriented[k][0]), lin(oriented[k][1])))
    branches = [oriented[k] for k in order]
    nodes = sorted({p[0] for p in branches} | {p[-1] for p in branches}, key=lin)
    return branches, nodes, [order.index(k) for k in range(len(paths))]


def check_tree(branches, nodes):
    for s in branches:
        assert all(max(abs(x - y) for x, y in zip(p, q)) == 1 for p, q in zip(s[:-1], s[1:])), 'a pair that is not 26-adjacent'
        assert all(0 <= c < n for p in s for c, n in zip(p, SHAPE))
    inner = [p for s in branches for p in s[1:-1]]
    assert len(set(inner)) == len(inner) and not set(inner) & set(nodes), 'a voxel in two branches'
    assert len(set(inner)) + len(nodes) > 50


def paint(branches, radii):
    """Balls of the branch's radius around each of its voxels; the distance transform of their union."""
    from scipy import ndimage
    mask = np.zeros(SHAPE, bool)
    grid = np.indices(SHAPE)
    for s, r in zip(branches, radii):
        for p in s:
            lo = [max(int(c - r - 1), 0) for c in p]
            hi = [min(int(c + r + 2), n) for c, n in zip(p, SHAPE)]
            sl = tuple(slice(l, h) for l, h in zip(lo, hi))
            mask[sl] |= sum((grid[k][sl] - p[k]) ** 2 for k in range(3)) <= r * r
    return mask, ndimage.distance_transform_edt(mask)


# ------------------------------------------------------------------ the reference, imported as it is
class Stub(types.ModuleType):
    """An importable nothing: any attribute is another one, it may be called, and a class may name it as a base."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return Stub(self.__name__ + '.' + name)

    def __call__(self, *a, **k):
        return self

    def __mro_entries__(self, bases):
        return (object,)


UNUSED = ('nibabel', 'skimage', 'pyqtgraph', 'PyQt5', 'matplotlib', 'mpl_toolkits', 'pygraphviz', 'graphviz')


class StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """The last finder: the packages of `UNUSED` that are not installed, and whatever is asked of them."""

    def __init__(self):
        self.missing = {name for name in UNUSED if importlib.util.find_spec(name) is None}

    def find_spec(self, name, path=None, target=None):
        if name.split('.')[0] not in self.missing:
            return None
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return Stub(spec.name)

    def exec_module(self, module):
        pass


def load_reference(code_dir):
    import networkx as nx
    nx.Graph.node = property(lambda self: self.nodes)
    nx.Graph.add_path = lambda self, nodes, **attr: nx.add_path(self, nodes, **attr)
    sys.path.insert(0, code_dir)
    finder = StubFinder()
    sys.meta_path.append(finder)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import graphRelated
            import manualCorrectionGUI
            import myFunctions
    finally:
        sys.meta_path.remove(finder)
    return manualCorrectionGUI.calculateBranchInfo, myFunctions.randomWalkBFS, graphRelated.calculateProperty


# ------------------------------------------------------------------ the reference's formulas in long double
def ld_norm(v):
    return np.sqrt((v * v).sum(dtype=LD))


def ld_angle(a, b, clip=True):
    c = (a * b).sum(dtype=LD) / (ld_norm(a) * ld_norm(b))
    if clip:
        c = min(max(c, LD(-1)), LD(1))
    return np.arccos(c) / ld_pi() * LD(180)


def ld_pi():
    return LD(4) * np.arctan(LD(1))


def ld_tilt(c1, c2, parent_local):
    half = c1 / ld_norm(c1) + c2 / ld_norm(c2)
    return ld_angle(half, -parent_local, clip=False)


def ld_normal(c1, c2):
    n = np.cross(c1, c2)                                                  # (integers in long double: exact)
    return n / ld_norm(n)


def by_construction(x):
    return any(abs(x - s) < LD(1e-15) for s in (0, 90, 180))


# ------------------------------------------------------------------ one case
def record(name, build, reference):
    branch_info, walk, properties = reference
    paths, roots, radii = build()
    branches, nodes, where = table(paths)
    check_tree(branches, nodes)
    radii = [radii[where.index(k)] for k in range(len(branches))]
    mask, dist = paint(branches, radii)
    B, N = len(branches), len(nodes)
    node_of = {p: k for k, p in enumerate(nodes)}
    ends = np.array([[node_of[s[0]], node_of[s[-1]]] for s in branches], np.int64)
    degree = np.bincount(ends.ravel(), minlength=N)
    assert set(degree.tolist()) <= {1, 3}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()) as said:
        np.savez_compressed(os.path.join(tmp, 'vesselVolumeDistanceTransform.npz'), distanceTransform=dist)
        segment_list = [list(s) for s in branches]
        G = branch_info(segment_list, segment_list, mask.astype(np.uint8), tmp)
        G, visited, _ = walk(G, [list(p) for p in roots], [])
        node_info, seg_info = properties(G, segment_list)
    assert set(visited) == set(G.nodes) and sorted(seg_info) == list(range(B))
    assert all(abs(G.nodes[p]['radius'] - dist[p]) == 0 for p in G.nodes)

    out = {}
    # ---- per branch
    keys = SEG_FLOAT + SEG_INT + SEG_OTHER
    assert all(set(d) <= set(keys) for d in seg_info.values()), 'a key of segmentInfoDict that is not recorded'
    out['seg_keys'] = np.array(keys)
    out['seg_has'] = np.array([[k in seg_info[b] for k in keys] for b in range(B)], bool)
    for k in SEG_FLOAT:
        out['seg_' + k] = np.array([float(seg_info[b].get(k, np.nan)) for b in range(B)], np.float64)
    for k in SEG_INT:
        code = (lambda x: TYPE_CODE[x]) if k == 'type' else int
        out['seg_' + k] = np.array([code(seg_info[b][k]) if k in seg_info[b] else -1 for b in range(B)], np.int64)
    # ---- per node voxel
    keys = NODE_FLOAT + NODE_INT + NODE_VEC + NODE_OTHER
    assert all(set(node_info[p]) <= set(keys) for p in nodes), 'a key of nodeInfoDict that is not recorded'
    out['node_keys'] = np.array(keys)
    out['node_has'] = np.array([[k in node_info[p] for k in keys] for p in nodes], bool)
    for k in NODE_FLOAT:
        out['node_' + k] = np.array([float(node_info[p].get(k, np.nan)) for p in nodes], np.float64)
    for k in NODE_INT:
        code = (lambda x: TYPE_CODE[x]) if k == 'type' else int
        out['node_' + k] = np.array([code(node_info[p][k]) if k in node_info[p] else -1 for p in nodes], np.int64)
    for k in NODE_VEC:
        out['node_' + k] = np.array([np.asarray(node_info[p].get(k, [np.nan] * 3), np.float64) for p in nodes], np.float64).reshape(N, 3)
    entries = [p for s in branches for p in s]
    out['entry_depthVoxel'] = np.array([G.nodes[p]['depthVoxel'] for p in entries], np.int64)
    out['entry_depthLevel'] = np.array([G.nodes[p]['depthLevel'] for p in entries], np.int64)
    out['entry_pathDistance'] = np.array([G.nodes[p]['pathDistance'] for p in entries], np.float64)
    # ---- the reference's order, from radiusList (the three mean radii must differ for that)
    order = np.full((N, 3), -1, np.int64)
    straight = np.array([len({tuple(np.subtract(q, p)) for p, q in zip(s[:-1], s[1:])}) == 1 for s in branches])
    for v, p in enumerate(nodes):
        if 'radiusList' not in node_info[p]:
            continue
        mine = [b for b in range(B) if v in ends[b]]
        radius_of = {b: seg_info[b]['meanRadius'] for b in mine}
        assert len(set(radius_of.values())) == 3, 'two branches of a bifurcation have the same meanRadius: the order cannot be read'
        order[v] = [[b for b in mine if radius_of[b] == r][0] for r in node_info[p]['radiusList']]
    out['ref_order'], out['straight_branch'] = order, straight
    # ---- long double
    exact = {k: np.full(N, np.nan) for k in ANGLES}
    refdist = {k: np.full(N, np.nan) for k in ANGLES}
    exact['normalVector'], refdist['normalVector'] = np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    normal_ld = {}
    for v, p in enumerate(nodes):
        if order[v, 0] < 0:
            continue
        away = [branches[b] if ends[b, 0] == v else branches[b][::-1] for b in order[v]]
        remote = [np.array(s[-1], LD) - np.array(p, LD) for s in away]
        values = {'remoteBifurcationAmplitude': ld_angle(remote[0], remote[1])}
        all_straight = bool(straight[order[v]].all())
        if straight[order[v, 2]]:                                         # (the reference takes the remote tilt against the parent's LOCAL direction)
            values['remoteBifurcationTilt'] = ld_tilt(remote[0], remote[1], np.array(away[2][1], LD) - np.array(p, LD))
        if all_straight:
            local = [np.array(s[1], LD) - np.array(p, LD) for s in away]
            values['localBifurcationAmplitude'] = ld_angle(local[0], local[1])
            values['localBifurcationTilt'] = ld_tilt(local[0], local[1], local[2])
            normal_ld[v] = ld_normal(local[0], local[1])
            exact['normalVector'][v] = normal_ld[v].astype(np.float64)
            refdist['normalVector'][v] = np.abs(np.asarray(node_info[p]['normalVector'], LD) - normal_ld[v]).astype(np.float64)
        for k, x in values.items():
            assert k in node_info[p], (name, p, k)
            exact[k][v], refdist[k][v] = float(x), float(abs(LD(node_info[p][k]) - x))
            assert by_construction(x) or 10 < x < 170, (name, p, k, float(x))
        for k in ANGLES:
            if k in node_info[p]:
                assert by_construction(LD(round(node_info[p][k], 6))) or 10 < node_info[p][k] < 170, (name, p, k, node_info[p][k])
    torque_exact, torque_dist = np.full(B, np.nan), np.full(B, np.nan)
    for b in range(B):
        u, v = ends[b]
        if u in normal_ld and v in normal_ld:
            t = ld_angle(normal_ld[u], normal_ld[v])
            t = LD(180) - t if t > 90 else t
            torque_exact[b], torque_dist[b] = float(t), float(abs(LD(seg_info[b]['localBifurcationTorque']) - t))
            assert by_construction(t) or 10 < t < 170
    for k in ANGLES + ('normalVector',):
        out['exact_' + k], out['refdist_' + k] = exact[k], refdist[k]
    out['exact_localBifurcationTorque'], out['refdist_localBifurcationTorque'] = torque_exact, torque_dist

    path = os.path.join(HERE, 'morphometry', name + '.npz')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, shape=np.array(SHAPE, np.int64), offsets=np.cumsum([0] + [len(s) for s in branches]).astype(np.int64),
                        voxels=np.array([lin(p) for p in entries], np.int64), ends=ends, node_voxel=np.array([lin(p) for p in nodes], np.int64),
                        node_kind=(degree > 1).astype(np.int64), roots=np.array([node_of[tuple(p)] for p in roots], np.int64),
                        dist=np.array([dist[p] for p in entries], np.float64), **out)
    print('{:10s} {} branches of {} entries, {} nodes, {} graph voxels; tabulated {}; two-entry meanRadius {}'.format(
        name, B, [len(s) for s in branches], N, len(G.nodes), np.flatnonzero(order[:, 0] >= 0).tolist(),
        [seg_info[b]['meanRadius'] for b in range(B) if len(branches[b]) == 2]))
    print('           order', order[order[:, 0] >= 0].tolist())
    for k in ANGLES + ('normalVector', 'localBifurcationTorque'):
        d = out['refdist_' + k]
        if np.isfinite(d).any():
            print('           the reference\'s distance from long double, {}: at most {:.3e}'.format(k, np.nanmax(d)))
    print('wrote', path, os.path.getsize(path), 'bytes')


def main(code_dir):
    reference = load_reference(code_dir)
    for name, build in CASES:
        record(name, build, reference)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
