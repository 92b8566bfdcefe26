"""Time vmask_centrelines on a synthetic branch table (profiles/centreline_timing.md).

    python tools/centreline_timing.py [--branches 10000] [--mean 100] [--seed 7] [--md FILE]

The table: `branches` branches whose lengths are max(2, round(exp(N(ln(mean) - 1/2, 1)))) - a lognormal mix with that mean, drawn
by np.random.default_rng(seed) - each the first n voxels of one winding path (the seven steps of tests/test_morphometry.py's HELIX
in turn, from (0, 1, 1): no voxel twice, never straight, so the search runs its 24 steps).  The branches overlap in the volume;
the fit looks at one branch at a time.  Spacing 0.4 0.4 0.7.  `kernel_ms` is the library's own figure (hipEvents around its two
kernels); one warm call, then the median of five.  Rows: the default (branches of up to 256 entries in LDS), 512 in LDS, every
branch through the global work space, and a fixed lambda (one solve per branch where the search has 26).  No threshold is set."""
import argparse
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from arterynetwork_amd import skeletonization as S

HELIX = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, -1), (0, -1, 0), (1, 1, 1), (1, -1, -1)]
SPACING = (0.4, 0.4, 0.7)


def table(branches, mean, seed):
    n = np.maximum(2, np.rint(np.exp(np.random.default_rng(seed).normal(np.log(mean) - 0.5, 1.0, branches)))).astype(np.int64)
    longest = int(n.max())
    path = np.cumsum(np.vstack([[0, 1, 1], np.array([HELIX[i % 7] for i in range(longest - 1)], np.int64).reshape(-1, 3)]), axis=0)
    offsets = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    coords = np.concatenate([path[:k] for k in n.tolist()])
    shape = tuple(int(k) for k in path.max(axis=0) + 1)
    return types.SimpleNamespace(offsets=offsets, coords=coords, skeleton=np.zeros(shape, np.uint8)), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--branches', type=int, default=10000)
    ap.add_argument('--mean', type=float, default=100.0)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    graph, n = table(a.branches, a.mean, a.seed)
    l2, l, lo, hi = S.splineScale(SPACING)
    rows = []
    for name, kw in (('default: n <= 256 in LDS', {}), ('n <= 512 in LDS', dict(ldsEntries=512)), ('all through the global work space', dict(ldsEntries=1)),
                     ('fixed lambda, default LDS', dict(smoothing=64.0 * l2 * l))):
        times, info = [], {}
        for k in range(6):
            got = S.branchSplines(graph, spacing=SPACING, info=info, **kw)
            if k:
                times.append(info['kernel_ms'])
        rows.append((name, float(np.median(times)), min(times), max(times), info['solves'], info['capped']))
        print(rows[-1], flush=True)
    head = '{} branches, {} entries, lengths {} .. {} (median {}), {} longer than 256, {} longer than 512'.format(
        len(n), int(n.sum()), int(n.min()), int(n.max()), int(np.median(n)), int((n > 256).sum()), int((n > 512).sum()))
    print(head)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# vmask_centrelines: timing\n\n`python tools/centreline_timing.py` on one MI355X: ' + head + '; host tables in, `kernel_ms` (hipEvents around the two\n'
                    'kernels), one warm call, median of five (ms).  One run, one machine: figures to about two digits.  No threshold is set.\n\n')
            f.write('| run | kernel_ms median | min | max | trial solves | capped branches |\n|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| {} | {:.2f} | {:.2f} | {:.2f} | {} | {} |\n'.format(*r))


if __name__ == '__main__':
    main()
