"""Time vmask_morphometry on the branch graphs of the bench masks (profiles/morphometry_timing.md).

    python tools/morphometry_timing.py [--shape 512x512x170 ...] [--out FILE] [--md FILE]

Per mask of tools/segments_timing.py: the skeleton, its branch graph (vmask_branches without pruning) and the distance transform of
the mask, all device-resident; then HIP events around the C-ABI calls, one warm call and the median of five: one vmask_branches
build, one vmask_morphometry call without roots and one with node 0 as the root, and one streaming read of `dist` (a sum over the
volume) on the same run.  Reported beside them: depthRounds and the branch, entry and node counts.  No threshold is set."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, skeletonization as S
from segments_timing import masks, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['512x512x170']:
        shape = tuple(int(x) for x in text.split('x'))
        for name, m in masks(shape, dev):
            sk = S.skeletonize(m)
            dist = G.distance_transform_edt(m)
            graph = S.branchGraph(sk)
            B, N, total = int(graph.offsets.numel()) - 1, int(graph.nodeCoords.shape[0]), int(graph.coords.shape[0])
            n1, n2 = shape[1], shape[2]
            lin = lambda c: ((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2]).contiguous()
            vox, nodevox = lin(graph.coords), lin(graph.nodeCoords)
            off, ends = graph.offsets.contiguous(), graph.branchEnds.contiguous()
            i64 = lambda *k: torch.empty(k, dtype=torch.int64, device=dev)
            f64 = lambda *k: torch.empty(k, dtype=torch.float64, device=dev)
            bi, bf, rad, inc = i64(B + 1, 24), f64(B + 1, 5), f64(N + 1), i64(N + 1, 3)          # (never empty: an empty tensor has no address)
            pd, nd, bl = f64(N + 1), i64(N + 1, 3), i64(B + 1)
            roots = torch.zeros(1, dtype=torch.int64, device=dev)
            counts, bc = np.zeros(2, np.int64), np.zeros(12, np.int64)
            h = np.array([0.4, 0.4, 0.6])

            def measure(nroots):
                return lambda: G._check(dll.vmask_morphometry(0, *shape, dist.data_ptr(), off.data_ptr(), B, vox.data_ptr(), ends.data_ptr(), nodevox.data_ptr(), N,
                                                              h.ctypes.data, roots.data_ptr() if nroots else None, nroots if N else 0, 5, bi.data_ptr(), bf.data_ptr(),
                                                              rad.data_ptr(), inc.data_ptr(), None, pd.data_ptr(), nd.data_ptr(), bl.data_ptr(), counts.ctypes.data))
            nodes, e2, o2, v2, out = i64(4 * N + 1), i64(2 * B + 1), i64(B + 2), i64(total + 1), torch.empty_like(sk)
            build = lambda: G._check(dll.vmask_branches(0, sk.data_ptr(), *shape, 0, 0.0, None, 64, out.data_ptr(), bc.ctypes.data, nodes.data_ptr(), N,
                                                        e2.data_ptr(), o2.data_ptr(), B, v2.data_ptr(), total))
            row = {'volume': text, 'mask': name, 'branches': B, 'entries': total, 'nodes': N}
            row['branches_ms'] = timed(build, 1, 5)
            row['morphometry_ms'] = timed(measure(0), 1, 5)
            row['morphometry_root_ms'] = timed(measure(1), 1, 5)
            row['depthRounds'], row['levelRounds'] = int(counts[0]), int(counts[1])
            row['dist_read_ms'] = timed(lambda: dist.sum(), 1, 5)
            row['dist_GB'] = round(dist.numel() * 8 / 1e9, 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, dist, graph
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# vmask_morphometry: timing\n\n`python tools/morphometry_timing.py` on one MI355X, device-resident input and output, HIP events around the C-ABI\n'
                    'calls, one warm call, median of five (ms).  The masks are the bench masks of `tools/segments_timing.py`; the graph is `vmask_branches`\n'
                    'without pruning.  One run, one machine: figures to about two digits.  No threshold is set.\n\n')
            f.write('| volume | mask | branches | entries | nodes | `vmask_branches` build | morphometry, no root | morphometry, one root | depthRounds | level rounds | one read of `dist` | `dist` GB |\n')
            f.write('|' + '---|' * 12 + '\n')
            for r in rows:
                f.write('| {volume} | {mask} | {branches} | {entries} | {nodes} | {b:.2f} | {m0:.2f} | {m1:.2f} | {depthRounds} | {levelRounds} | {d:.2f} | {dist_GB} |\n'.format(
                    b=r['branches_ms'][0], m0=r['morphometry_ms'][0], m1=r['morphometry_root_ms'][0], d=r['dist_read_ms'][0], **r))


if __name__ == '__main__':
    main()
