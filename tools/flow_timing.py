"""Time vmask_flow on the branch graphs of the bench masks and on one large synthetic tree (profiles/flow_timing.md).

    python tools/flow_timing.py [--shape 512x512x170 ...] [--out FILE] [--md FILE]

Per mask of tools/segments_timing.py: the skeleton, its branch graph (vmask_branches without pruning) and its morphometry; the end
points are fixed - the first one the inlet at 100 mmHg, the others at 0 -, the resistances Hazen-Williams (a voxel of 0.5 mm,
c = 120, k = 1.852) of pathLength and meanRadius.  Then HIP events around `simulateFlow` with device-resident resistances, one warm
call and the median of five: one scenario, and 256 and 1024 scenarios whose radii are perturbed by +-10 %.  Beside them the direct
model of tests/flow_model.py (scipy's spsolve per outer step) on the host for the same systems: timed on the first scenarios and
multiplied out.  Last, one scenario of a binary tree of depth 16 (131 070 branches, 65 534 free nodes): the case that one workgroup
per scenario may be too slow for.  No threshold is set."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np
import torch

from arterynetwork_amd import flow as F, skeletonization as S
from segments_timing import masks, timed
import flow_model as FM

K, TOL = 1.852, 1e-10
HOST_SCENARIOS = 4


def scenarios(length, radius, count, seed):
    r = radius * (0.9 + 0.2 * np.random.default_rng(seed).random((count, len(radius))))
    return F.branchResistance(length, r, c=120.0, k=K)


def measure(ends, fixed, P, length, radius, dev, row):
    N = len(fixed)
    for count in (1, 256, 1024):
        R = scenarios(length, radius, count, count) if count > 1 else F.branchResistance(length, radius, c=120.0, k=K)[None]
        Rd = torch.as_tensor(R, device=dev)
        last = {}

        def call():
            last['r'] = F.simulateFlow((ends, N), Rd, fixed.astype(bool), P, k=K, tol=TOL)
        row['gpu_ms_%d' % count] = timed(call, 1, 5)
        r = last['r']
        row['converged_%d' % count] = int(r.converged.sum())
        row['outer_%d' % count], row['inner_%d' % count] = float(r.outerIterations.double().mean()), float(r.innerIterations.double().mean())
        t0 = time.perf_counter()
        for s in range(min(count, HOST_SCENARIOS)):
            FM.solve_direct(ends, fixed, R[s], P, k=K, tol=TOL)
        row['host_ms_%d' % count] = (time.perf_counter() - t0) / min(count, HOST_SCENARIOS) * count * 1e3


def binary_tree(depth):
    n = 2 ** (depth + 1) - 1
    ends = np.array([[(i - 1) // 2, i] for i in range(1, n)], np.int64)
    level = np.floor(np.log2(np.arange(1, n) + 1)).astype(np.int64)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    fixed[2 ** depth - 1:] = 1
    rng = np.random.default_rng(16)
    radius = 2e-3 * 0.8 ** (level - 1) * (0.9 + 0.2 * rng.random(n - 1))
    length = 0.05 * 0.85 ** (level - 1) * (0.8 + 0.4 * rng.random(n - 1))
    P = np.zeros(n)
    P[0] = 13328.0
    return ends, fixed, P, length, radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    rows = []
    for text in a.shape or ['512x512x170']:
        shape = tuple(int(x) for x in text.split('x'))
        for name, m in masks(shape, dev):
            graph = S.branchGraph(S.skeletonize(m))
            measured = S.branchMorphometry(graph, vesselVolumeMask=m)
            ends, kind = graph.branchEnds.cpu().numpy(), graph.nodeKind.cpu().numpy()
            length = np.maximum(measured.pathLength.cpu().numpy(), 0.5) * 0.5e-3
            radius = np.maximum(measured.meanRadius.cpu().numpy(), 0.5) * 0.5e-3
            fixed = (kind == 0).astype(np.uint8)
            if not fixed.any():
                fixed[0] = 1
            P = np.zeros(len(fixed))
            P[np.flatnonzero(fixed)[0]] = 13328.0
            top = FM.Topology(ends, fixed, len(fixed))
            row = {'volume': text, 'mask': name, 'branches': len(ends), 'nodes': len(fixed), 'free': len(top.free), 'floating': top.floating_components}
            measure(ends, fixed, P, length, radius, dev, row)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, graph, measured
            torch.cuda.empty_cache()
    ends, fixed, P, length, radius = binary_tree(16)
    R = F.branchResistance(length, radius, c=120.0, k=K)
    big = {'branches': len(ends), 'nodes': len(fixed), 'free': int((fixed == 0).sum())}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = F.simulateFlow((ends, len(fixed)), R, fixed.astype(bool), P, k=K, tol=TOL)
    big['gpu_ms'] = (time.perf_counter() - t0) * 1e3
    big.update(converged=bool(r.converged[0]), outer=int(r.outerIterations[0]), inner=int(r.innerIterations[0]), residual=float(r.residual[0]))
    t0 = time.perf_counter()
    d = FM.solve_direct(ends, fixed, R, P, k=K, tol=TOL)
    big['host_ms'] = (time.perf_counter() - t0) * 1e3
    big.update(host_converged=bool(d.converged), host_outer=int(d.outer))
    print(json.dumps(big), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'graphs': rows, 'tree': big}, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# vmask_flow: timing\n\n`python tools/flow_timing.py` on one MI355X: HIP events around `simulateFlow` with device-resident resistances, one warm call,\n'
                    'median of five (ms); k = 1.852, tol = 1e-10.  The masks are the bench masks of `tools/segments_timing.py`, the graph is `vmask_branches`\n'
                    'without pruning, the end points are fixed (the first at 100 mmHg, the others at 0), the resistances Hazen-Williams of the graph\'s own\n'
                    'morphometry; the scenarios perturb the radii by +-10 %.  "host" is the direct model of `tests/flow_model.py` (spsolve per outer step)\n'
                    'on the same systems, timed on the first {} scenarios and multiplied out.  One run, one machine: figures to about two digits.\n'
                    'No threshold is set.\n\n'.format(HOST_SCENARIOS))
            f.write('| volume | mask | branches | nodes | free nodes | S = 1 | outer / inner | host | S = 256 | converged | host | S = 1024 | converged | outer / inner (mean) | host |\n')
            f.write('|' + '---|' * 15 + '\n')
            for r in rows:
                f.write('| {volume} | {mask} | {branches} | {nodes} | {free} | {a:.2f} | {outer_1:.0f} / {inner_1:.0f} | {host_ms_1:.1f} | {b:.2f} | {converged_256} | {host_ms_256:.0f} '
                        '| {c:.2f} | {converged_1024} | {outer_1024:.1f} / {inner_1024:.0f} | {host_ms_1024:.0f} |\n'.format(a=r['gpu_ms_1'][0], b=r['gpu_ms_256'][0], c=r['gpu_ms_1024'][0], **r))
            f.write('\nOne scenario of a binary tree of depth 16 ({branches} branches, {free} free nodes), wall time of one call with host arrays: {gpu_ms:.0f} ms on the GPU '
                    '(converged: {converged}, {outer} outer and {inner} inner iterations, residual {residual:.1e}); the direct model on the host: {host_ms:.0f} ms '
                    '(converged: {host_converged}, {host_outer} outer iterations).\n'.format(**big))


if __name__ == '__main__':
    main()
