#!/usr/bin/env python3
"""Record the reference's own compartment traversal (myFunctions.randomWalkBFS) on a small tree, for tests/test_compartments.py.

Runs only where the reference is at hand (it never ships):
    python tests/golden/make_compartment_goldens.py <the reference's Code directory>
The function is imported from the reference as it is.  What it does not use is stubbed - every module that myFunctions.py
imports and this machine lacks becomes an empty stand-in - and networkx 3 is given back the ``G.node`` of networkx 1 that the
function indexes.  The graph is built the way the reference builds it (skeletonization.py:765-769: one path per segment with
the attribute segmentIndex) from a tree written out below: six nodes, five branches, every junction a single voxel.

Output (data only): tests/golden/compartments/tree.npz - the branch table (shape, offsets, voxels, ends, node_voxel), the lists
of every compartment (initial / boundary with their offsets) and, per compartment, what one call returned: the visited voxels
(as a set, ascending), their depthVoxel and depthLevel, and the segment indices (unique, ascending).

The compartments cover a boundary at entry 1 of a branch, in the middle of one and at its last entry, and initial voxels at an end
point, in the middle of a branch, at a junction, and at two end points at once.  Two initial voxels are placed so that their
fronts meet ON a node: the reference lists a segment only when the walk arrives at one of its ends, so a branch inside which two
fronts meet is in none of its lists although every voxel of it is visited (Not claimed)."""
import contextlib
import importlib.abc
import importlib.machinery
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (16, 20, 20)
R, J1, J2, E1, E2, E3 = (0, 10, 10), (8, 10, 10), (8, 16, 10), (8, 2, 10), (14, 16, 10), (8, 16, 17)


def straight(a, b):
    """The voxels from a to b along the one axis in which they differ."""
    axis = [k for k in range(3) if a[k] != b[k]][0]
    step = 1 if b[axis] > a[axis] else -1
    return [tuple(a[k] if k != axis else x for k in range(3)) for x in range(a[axis], b[axis] + step, step)]


def lin(p):
    return (p[0] * SHAPE[1] + p[1]) * SHAPE[2] + p[2]


def tree():
    """Branches from the end of smaller raster index, ascending by (first, second) voxel; nodes ascending."""
    branches = sorted((min(straight(a, b), straight(b, a), key=lambda s: lin(s[0])) for a, b in ((R, J1), (J1, E1), (J1, J2), (J2, E2), (J2, E3))),
                      key=lambda s: (lin(s[0]), lin(s[1])))
    nodes = sorted((R, J1, J2, E1, E2, E3), key=lin)
    return branches, nodes


class Stub(types.ModuleType):
    """An importable nothing: any attribute is another one, and it may be called."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return Stub(self.__name__ + '.' + name)

    def __call__(self, *a, **k):
        return self


UNUSED = ('nibabel', 'skimage', 'pyqtgraph', 'matplotlib', 'mpl_toolkits', 'scipy')     # what myFunctions.py imports and randomWalkBFS does not use


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
    sys.path.insert(0, code_dir)
    finder = StubFinder()
    sys.meta_path.append(finder)
    try:
        import myFunctions
    finally:
        sys.meta_path.remove(finder)

    class Graph(nx.Graph):
        node = property(lambda self: self.nodes)
    return myFunctions.randomWalkBFS, Graph, nx


def main(code_dir):
    walk, Graph, nx = load_reference(code_dir)
    branches, nodes = tree()
    middle = lambda b: branches[b][len(branches[b]) // 2]
    of = {frozenset((s[0], s[-1])): k for k, s in enumerate(branches)}
    trunk, up, side = of[frozenset((R, J1))], of[frozenset((J1, J2))], of[frozenset((J2, E2))]
    compartments = [([R], [branches[up][1]]),                             # a boundary at entry 1
                    ([middle(trunk)], [middle(up)]),                      # from the middle of a branch; a boundary in the middle of one
                    ([R, E1], [branches[side][-1]]),                      # two end points, eight edges from J1 each; a boundary at a last entry
                    ([J1], [J2]),                                         # from a junction, shut in by the next one
                    ([E3], [])]                                           # the whole tree
    assert branches[up][0] == J1 and branches[side][-1] == E2 and len(straight(R, J1)) == len(straight(E1, J1))
    out = {'visited': [], 'depthVoxel': [], 'depthLevel': [], 'segments': [], 'visited_off': [0], 'segments_off': [0]}
    for initial, boundary in compartments:
        G = Graph()
        for k, s in enumerate(branches):
            nx.add_path(G, s, segmentIndex=k)
        with contextlib.redirect_stdout(io.StringIO()):
            G, visited, segments = walk(G, [list(p) for p in initial], [list(p) for p in boundary])
        seen = sorted(set(visited), key=lin)
        out['visited'] += [lin(p) for p in seen]
        out['depthVoxel'] += [G.nodes[p]['depthVoxel'] for p in seen]
        out['depthLevel'] += [G.nodes[p]['depthLevel'] for p in seen]
        out['segments'] += sorted(set(segments))
        out['visited_off'].append(len(out['visited']))
        out['segments_off'].append(len(out['segments']))
        print('initial', initial, 'boundary', boundary, '->', len(seen), 'voxels, segments', sorted(set(segments)))
    node_of = {p: k for k, p in enumerate(nodes)}
    cat = lambda which: [lin(p) for c in compartments for p in c[which]]
    off = lambda which: np.cumsum([0] + [len(c[which]) for c in compartments])
    path = os.path.join(HERE, 'compartments', 'tree.npz')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, shape=np.array(SHAPE, np.int64), offsets=np.cumsum([0] + [len(s) for s in branches]).astype(np.int64),
                        voxels=np.array([lin(p) for s in branches for p in s], np.int64), ends=np.array([[node_of[s[0]], node_of[s[-1]]] for s in branches], np.int64),
                        node_voxel=np.array([lin(p) for p in nodes], np.int64), initial=np.array(cat(0), np.int64), initial_off=off(0).astype(np.int64),
                        boundary=np.array(cat(1), np.int64), boundary_off=off(1).astype(np.int64), **{k: np.array(v, np.int64) for k, v in out.items()})
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
