#!/usr/bin/env python3
"""Record the reference's own network equations (fluidSimulation.computeNetworkDetail, method 'HW') on a small tree, for
tests/test_flow.py.

Runs only where the reference is at hand (it never ships):
    python tests/golden/make_flow_goldens.py <the reference's Code directory>
The function is imported from the reference as it is; every module that fluidSimulation.py and myFunctions.py import and this
machine lacks becomes an empty stand-in.  The equation list is laid out the way the reference lays it out (fluidSimulation.py:
880-888): one 'flow' equation per free node with the velocity indices and radii of the branches that arrive and leave, one
'pressure' equation per branch with its radius, length, c, k and the head's and the tail's pressure - a value where the node is
fixed, an index into the unknowns where it is free.  The unknowns are the B velocities, then the pressures of the free nodes
ascending.

The network: a binary tree of depth 3 - node 0 the inlet, nodes 1 .. 6 free, nodes 7 .. 14 terminals, 14 branches, each given
from the end nearer the inlet (the head) to the other.  The terminal pressures (0.70 - 0.01 i) P_in are such that NO BRANCH FLOWS
AGAINST ITS DEPTH ORDER: the reference's equations take |velocity| and cannot express that.

Output (data only): tests/golden/flow/tree.npz - ends, radius, length, c, k, fixed, pressure (the fixed values, 0 elsewhere),
probes (3 x (B + F): the solution of tests/flow_model.solve_direct, the same scaled by 1.01, a random positive vector) and
residuals (3 x (F + B): what the reference returned at each, flow rows first)."""
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
sys.path.insert(0, os.path.dirname(HERE))

K = 1.852
P_IN = 13560 * 9.8 * 0.1                                                  # 100 mmHg in Pa


def tree():
    ends = [[(i - 1) // 2, i] for i in range(1, 15)]
    level = [int(np.log2(i + 1)) for i in range(1, 15)]                   # 1, 2 or 3
    rng = np.random.default_rng(13)
    radius = np.array([{1: 2.0e-3, 2: 1.5e-3, 3: 1.0e-3}[l] for l in level]) * (0.9 + 0.2 * rng.random(14))
    length = np.array([{1: 0.05, 2: 0.03, 3: 0.02}[l] for l in level]) * (0.8 + 0.4 * rng.random(14))
    c = 100.0 + 40.0 * rng.random(14)
    fixed = np.ones(15, np.uint8)
    fixed[1:7] = 0
    pressure = np.zeros(15)
    pressure[0] = P_IN
    pressure[7:] = (0.70 - 0.01 * np.arange(8)) * P_IN
    return np.array(ends, np.int64), radius, length, c, fixed, pressure


class Stub(types.ModuleType):
    """An importable nothing: any attribute is another one, and it may be called."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return Stub(self.__name__ + '.' + name)

    def __call__(self, *a, **k):
        return self


UNUSED = ('nibabel', 'skimage', 'pyqtgraph', 'graphviz', 'pygraphviz', 'matplotlib', 'mpl_toolkits', 'networkx', 'scipy')


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
    sys.path.insert(0, code_dir)
    finder = StubFinder()
    sys.meta_path.append(finder)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            import fluidSimulation
    finally:
        sys.meta_path.remove(finder)
    return fluidSimulation.computeNetworkDetail


def equations(ends, radius, length, c, fixed, pressure):
    B = len(ends)
    free = np.flatnonzero(fixed == 0)
    index_of = {int(v): B + j for j, v in enumerate(free)}
    eqns = []
    for i in free.tolist():
        arrive, leave = np.flatnonzero(ends[:, 1] == i).tolist(), np.flatnonzero(ends[:, 0] == i).tolist()
        eqns.append({'type': 'flow', 'velocityInIndexList': arrive, 'radiusInList': [float(radius[b]) for b in arrive],
                     'velocityOutIndexList': leave, 'radiusOutList': [float(radius[b]) for b in leave], 'coord': i, 'nodeIndex': i})
    for b in range(B):
        d = {'type': 'pressure', 'radius': float(radius[b]), 'length': float(length[b]), 'velocityIndex': b, 'c': float(c[b]), 'k': K, 'edgeIndex': b}
        for key, v in (('headPressureInfo', int(ends[b, 0])), ('tailPressureInfo', int(ends[b, 1]))):
            d[key] = {'pressure': float(pressure[v])} if fixed[v] else {'pressureIndex': index_of[v], 'nodeIndex': v}
        eqns.append(d)
    return eqns, free


def main(code_dir):
    import flow_model as FM
    compute = load_reference(code_dir)
    ends, radius, length, c, fixed, pressure = tree()
    R = 10.67 * length / c ** K / (2.0 * radius) ** 4.8704
    solved = FM.solve_direct(ends, fixed, R, pressure, k=K)
    assert solved.converged and (solved.flow > 0).all(), 'a branch flows against its depth order'
    eqns, free = equations(ends, radius, length, c, fixed, pressure)
    velocity = solved.flow / (np.pi * radius ** 2)
    at_solution = np.concatenate([velocity, solved.pressure[free]])
    rng = np.random.default_rng(14)
    random = np.concatenate([velocity.mean() * (0.2 + rng.random(len(ends))), P_IN * (0.5 + 0.5 * rng.random(len(free)))])
    probes = np.stack([at_solution, 1.01 * at_solution, random])
    with contextlib.redirect_stdout(io.StringIO()):
        residuals = np.array([[float(x) for x in compute(list(p), eqns, method='HW')] for p in probes])
    for name, row in zip(('solution', 'x 1.01', 'random'), residuals):
        print('{:9s} largest residual {:.3e} (flow rows {:.3e}, pressure rows {:.3e})'.format(name, row.max(), row[:len(free)].max(), row[len(free):].max()))
    path = os.path.join(HERE, 'flow', 'tree.npz')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, ends=ends, radius=radius, length=length, c=c, k=np.float64(K), fixed=fixed, pressure=pressure, probes=probes, residuals=residuals)
    print('wrote', path)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
