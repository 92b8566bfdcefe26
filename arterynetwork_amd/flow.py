"""Blood flow on the branch graph (``vmask_flow``, DESIGN.md section 9 "f13 flow"): the stage of the reference's
``fluidSimulation.py``.  Given a pressure at the inlet and at every terminal node, `simulateFlow` finds the pressure at every
other node and the flow in every branch under the law ``P_u - P_v = R |Q|^(k-1) Q`` - for S scenarios of one graph (perturbed
radii, perturbed terminal pressures, time steps) in one launch, one workgroup per scenario, as a signed network solve: a branch
may flow against its depth order, which the reference's ``|velocity|`` formulation cannot express.  HIP only; no CPU path.

`branchResistance` and `terminalPressures` turn `branchMorphometry`'s ``pathLength`` / ``meanRadius`` / ``pathDistance`` into the
solver's inputs with the reference's formulas; `referenceResiduals` restates the residual list of the reference's
``computeNetworkDetail`` so that a solution can be read in the reference's own terms.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import generateVesselVolume as _G
from ._capi import bind_flow

FLOW_FILE = 'flowResult.npz'


def _lib():
    return bind_flow(_G._lib())


class FlowResult:
    """What `simulateFlow` returns, S scenarios of N nodes and B branches: ``pressure`` (S x N, float64; NaN in a component
    without a fixed node), ``flow`` (S x B, float64, from the branch's first end to its second; computed from ``pressure`` by
    the law), ``converged`` (S, bool), ``outerIterations`` / ``innerIterations`` (S, int64), ``residual`` (S, float64: the largest
    flow imbalance at a free node over the largest flow) and ``floating``: the number of components without a fixed node."""
    names = ('pressure', 'flow', 'converged', 'outerIterations', 'innerIterations', 'residual')


def branchResistance(length, radius, law='HW', c=None, k=1.852, viscosity=3.5e-3):
    """The resistance R of ``dP = R |Q|^(k-1) Q`` per branch, SI units (metres, Pa s), float64, host numpy.
    ``'HW'`` (Hazen-Williams, fluidSimulation.py:530): ``10.67 L / c^k / (2 r)^4.8704``; `c` is required, a scalar or one per branch
    (the reference reads it from a table that does not ship).  ``'poiseuille'``: ``8 mu L / (pi r^4)``, and `k` must be 1."""
    L, r = np.asarray(length, np.float64), np.asarray(radius, np.float64)
    if law == 'HW':
        if c is None:
            raise ValueError('the Hazen-Williams law needs the coefficient c')
        return 10.67 * L / np.asarray(c, np.float64) ** float(k) / (2.0 * r) ** 4.8704
    if law == 'poiseuille':
        if float(k) != 1.0:
            raise ValueError('Poiseuille\'s law is linear: k must be 1')
        return 8.0 * float(viscosity) * L / (np.pi * r ** 4)
    raise ValueError('law: \'HW\' or \'poiseuille\'')


def terminalPressures(pathDistance, pressureIn, slope, factor=0.8):
    """``pressureIn + pathDistance * slope * factor`` (fluidSimulation.py:1442) on `branchMorphometry`'s ``pathDistance``."""
    return float(pressureIn) + np.asarray(pathDistance, np.float64) * float(slope) * float(factor)


def referenceResiduals(ends, radius, length, c, k, fixed, pressure, velocity):
    """The residual list of the reference's ``computeNetworkDetail`` (fluidSimulation.py:4636-4728, method 'HW', errorNorm 0)
    restated in numpy from its formulas, constants and weights, the head of a branch being the end given first.
    `pressure` (N) holds the fixed and the free pressures, `velocity` (B) one per branch; the reference takes ``|velocity|``.
    Returns ``(flowRows, pressureRows)``: per free node ascending ``|Q_in - Q_out| * 1e6 * 20000`` with Q = |v| pi r^2, in over the
    branches whose second end is the node and out over those whose first end it is; per branch
    ``2 |dP - dP_HW|`` where the head's pressure is the larger and ``10 |P_tail + dP_HW - P_head|`` otherwise, times
    ``1000 / 13560 / 9.8 * 500``, with ``dP_HW = 10.67 (|v| pi r^2)^k L / c^k / (2 r)^4.8704``."""
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    r, L = np.asarray(radius, np.float64), np.asarray(length, np.float64)
    cc = np.broadcast_to(np.asarray(c, np.float64), r.shape)
    P, v = np.asarray(pressure, np.float64), np.abs(np.asarray(velocity, np.float64))
    free = np.flatnonzero(~np.asarray(fixed).astype(bool))
    q = v * np.pi * r ** 2
    rows = []
    for i in free.tolist():
        q_in = np.sum(q[ends[:, 1] == i])
        q_out = np.sum(q[ends[:, 0] == i])
        rows.append(np.abs(q_in - q_out))
    flow_rows = np.array(rows, np.float64) * (10 ** 6 * 20000)
    head, tail = P[ends[:, 0]], P[ends[:, 1]]
    by_hw = 10.67 * (v * np.pi * r ** 2) ** k * L / cc ** k / (2 * r) ** 4.8704
    pressure_rows = np.where(head > tail, np.abs((head - tail) - by_hw) * 2, 10 * np.abs(tail + by_hw - head)) * (1000 / 13560 / 9.8 * 500)
    return flow_rows, pressure_rows


def _graph_tables(graph):
    """branch ends and the node count of a `BranchGraph`, or of a pair (branchEnds, nnode)."""
    if hasattr(graph, 'branchEnds'):
        return graph.branchEnds, int(graph.nodeCoords.shape[0])
    ends, nnode = graph
    return ends, int(nnode)


def _host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


class _HostArrays:
    """The array operations of `simulateFlow` on numpy arrays; `device` is the GPU that the library uses."""

    def __init__(self, device):
        self.device = int(device)

    def f64(self, a):
        return np.asarray(_host(a), np.float64)

    def empty(self, shape, dtype):
        return np.empty(shape, dtype)

    def zeros(self, shape):
        return np.zeros(shape, np.float64)

    def array(self, a):
        return a

    def ptr(self, a):
        return a.ctypes.data if a.size else None

    def contiguous(self, a):
        return np.ascontiguousarray(a)

    def isfinite(self, a):
        return np.isfinite(a)

    def first(self, mask):
        """The index of the first True of `mask`, as a list."""
        return [int(x) for x in np.argwhere(mask)[0]]

    def ready(self):
        pass


class _DeviceTensors:
    """The same on torch tensors of the device of `ref`: that device is the GPU that the library uses."""

    def __init__(self, ref):
        import torch
        self.torch, self.where, self.device = torch, ref.device, _G._dev_index(ref)

    def f64(self, a):
        t = a if _G._on_device(a) else self.torch.as_tensor(np.asarray(_host(a), np.float64), device=self.where)
        return t.to(device=self.where, dtype=self.torch.float64)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.where)

    def zeros(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.float64, device=self.where)

    def array(self, a):
        return self.torch.as_tensor(a, device=self.where)

    def ptr(self, a):
        return a.data_ptr() if a.numel() else None

    def contiguous(self, a):
        return a.contiguous()

    def isfinite(self, a):
        return self.torch.isfinite(a)

    def first(self, mask):
        return [int(x) for x in mask.nonzero()[0].tolist()]

    def ready(self):
        self.torch.cuda.synchronize(self.where)


def _checked_ends(graph):
    """(ends as B x 2 int64 on the host, N, which branches take part); ``ValueError`` at the first end that is no node id."""
    ends_in, N = _graph_tables(graph)
    ends = np.ascontiguousarray(_host(ends_in), dtype=np.int64).reshape(-1, 2)
    closed = (ends[:, 0] == -1) & (ends[:, 1] == -1)
    wrong = ~closed & ((ends < 0) | (ends >= N)).any(axis=1)
    if wrong.any():
        b = int(np.flatnonzero(wrong)[0])
        raise ValueError('branch {}: the ends {} are no node ids (the graph has {} nodes) and not -1 -1'.format(b, ends[b].tolist(), N))
    return ends, N, ~closed & (ends[:, 0] != ends[:, 1])


def _fixed_flags(fixedNodes, N):
    """(the 0 / 1 flag per node, the index list or None where a mask was given)."""
    fn = _host(fixedNodes)
    if fn.dtype == np.bool_:
        if fn.shape != (N,):
            raise ValueError('fixedNodes: a boolean mask has one entry per node')
        return np.ascontiguousarray(fn, dtype=np.uint8), None
    index = np.asarray(fn).reshape(-1)
    if index.size and index.dtype.kind not in 'iu':
        raise ValueError('fixedNodes: a boolean mask or integer node indices')
    index = index.astype(np.int64)
    outside = (index < 0) | (index >= N)
    if outside.any():
        raise ValueError('fixed node {} is no node index (the graph has {} nodes)'.format(int(index[outside][0]), N))
    fixed = np.zeros(N, np.uint8)
    fixed[index] = 1
    return fixed, index


def _refuse(xp, ok, values, what, why):
    """``ValueError`` naming the first entry of `values` (B- or N-long, or S x that) where `ok` is False."""
    if bool(ok.all()):
        return
    at = xp.first(~ok)
    scenario = ' of scenario {}'.format(at[0]) if len(at) > 1 else ''
    raise ValueError('{} {}{}: {} {} {}'.format(what, at[-1], scenario, why[0], float(values[tuple(at)]), why[1]))


def simulateFlow(graph, resistance, fixedNodes, fixedPressure, k=1.852, tol=1e-10, maxIter=50, device=0, info=None):
    """Solve S scenarios of one graph (``vmask_flow``; include/vmask.h has the definition, the iteration and its summation order).

    `graph`: a `BranchGraph`, or a pair ``(branchEnds, nnode)``; a closed curve (ends -1 -1) and a loop on one node carry no flow.
    `resistance`: B values used by every scenario, or S x B.  `fixedNodes`: a boolean mask over the nodes, or node indices.
    `fixedPressure`: with a mask, N values or S x N (read at the fixed nodes); with indices, one value per index or S x that many.
    S is the leading size of whichever input has one, 1 otherwise.  `k` in [1, 3], `tol` in (0, 1), `maxIter` >= 1.
    Host arrays give host arrays, computed on GPU `device`.  Where `resistance` or `fixedPressure` is a tensor on a GPU the
    results are tensors on that GPU and the solve runs there: `device` then plays no part, as in the other wrappers.
    ``ValueError`` names the first branch or node that the library would refuse.  A scenario that does not converge is reported
    in ``converged``, holds its last iterate and does not fail the call.  `info`, when a dict, receives ``floatingComponents``
    and ``floatingNodes``."""
    if not 1.0 <= float(k) <= 3.0:
        raise ValueError('k must be in [1, 3]')
    if not 0.0 < float(tol) < 1.0:
        raise ValueError('tol must be in (0, 1)')
    if int(maxIter) < 1:
        raise ValueError('maxIter must be at least 1')
    ends, N, takes_part = _checked_ends(graph)
    B = len(ends)
    fixed, index = _fixed_flags(fixedNodes, N)
    on_device = [a for a in (resistance, fixedPressure) if _G._on_device(a)]
    xp = _DeviceTensors(on_device[0]) if on_device else _HostArrays(device)
    R, pf = xp.f64(resistance), xp.f64(fixedPressure)
    if R.ndim not in (1, 2) or R.shape[-1] != B:
        raise ValueError('resistance: {} values, or S x {}'.format(B, B))
    width = N if index is None else len(index)
    if pf.ndim not in (1, 2) or pf.shape[-1] != width:
        raise ValueError('fixedPressure: {} values, or S x {}'.format(width, width))
    sizes = {int(a.shape[0]) for a in (R, pf) if a.ndim == 2}
    if len(sizes) > 1:
        raise ValueError('resistance and fixedPressure disagree about the number of scenarios')
    S = sizes.pop() if sizes else 1
    if S < 1:
        raise ValueError('at least one scenario is needed')
    if index is not None:                                                 # one value per index: scattered to the nodes
        full = xp.zeros(tuple(pf.shape[:-1]) + (N,))
        full[..., xp.array(index)] = pf
        pf = full
    _refuse(xp, (xp.isfinite(R) & (R > 0)) | ~xp.array(takes_part), R, 'branch', ('the resistance', 'is not finite and positive'))
    _refuse(xp, xp.isfinite(pf) | ~xp.array(fixed.astype(bool)), pf, 'node', ('the fixed pressure', 'is not finite'))
    R, pf, ends_in, fixed_in = xp.contiguous(R), xp.contiguous(pf), xp.array(ends), xp.array(fixed)
    pressure, flow = xp.empty((S, N), np.float64), xp.empty((S, B), np.float64)
    status, residual = xp.empty((S, 3), np.int64), xp.empty((S,), np.float64)
    counts = np.zeros(2, np.int64)
    xp.ready()
    _G._check(_lib().vmask_flow(xp.device, N, B, xp.ptr(ends_in), xp.ptr(fixed_in), S, xp.ptr(R), B if R.ndim == 2 else 0, xp.ptr(pf), N if pf.ndim == 2 else 0,
                                float(k), float(tol), int(maxIter), xp.ptr(pressure), xp.ptr(flow), xp.ptr(status), xp.ptr(residual), counts.ctypes.data))
    out = FlowResult()
    out.pressure, out.flow, out.residual = pressure, flow, residual
    out.converged = status[:, 0] != 0
    out.outerIterations, out.innerIterations = xp.contiguous(status[:, 1]), xp.contiguous(status[:, 2])
    out.floating = int(counts[0])
    if info is not None:
        info['floatingComponents'], info['floatingNodes'] = int(counts[0]), int(counts[1])
    return out


def writeFlow(result, baseFolder, **extra):
    """``flowResult.npz``: the arrays of a host `FlowResult`, ``floating`` and whatever `extra` names; returns the file's name."""
    import os
    np.savez_compressed(os.path.join(baseFolder, FLOW_FILE), floating=np.int64(result.floating), **{k: getattr(result, k) for k in FlowResult.names},
                        **{k: np.asarray(v) for k, v in extra.items()})
    return FLOW_FILE
