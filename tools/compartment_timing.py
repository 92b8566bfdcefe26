"""Time vmask_compartments on the branch graphs of the bench masks (profiles/compartment_timing.md).

    python tools/compartment_timing.py [--shape 512x512x170 ...] [--out FILE] [--md FILE]

Per mask of tools/segments_timing.py: the skeleton and its branch graph (vmask_branches without pruning), device-resident; then HIP
events around the C-ABI calls, one warm call and the median of five: one vmask_compartments call with five compartments - each
entered at one node, shut in by four entries spread over the table - and, beside it, one vmask_morphometry call with node 0 as the
root on the same graph: the same kind of chain of short launches, each round read back by the host.  Reported with them: the depth
and level rounds, the kernel launches of the call (9 and one per round), the longest branch and what the partition found.  The
"clean" mask is the graph with long branches: its figure against the others says whether the thread-per-pair walks weigh.
No threshold is set."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, skeletonization as S
from segments_timing import masks, timed

K = 5


def lists_for(vox, nodevox):
    """Five compartments: compartment k starts at node k N / 5 and has four boundary entries; a voxel drawn for both stays initial."""
    N, E = len(nodevox), len(vox)
    ioff, ivox, boff, bvox = [0], [], [0], []
    for k in range(K):
        start = int(nodevox[k * N // K]) if N else int(vox[0])
        ivox.append(start)
        bvox += sorted({int(vox[(7 * k + 3 + j * (E // 4)) % E]) for j in range(4)} - {start})
        ioff.append(len(ivox)); boff.append(len(bvox))
    return [np.array(a, np.int64) for a in (ioff, ivox, boff, bvox)]


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
            u8 = lambda *k: torch.empty(k, dtype=torch.uint8, device=dev)
            ioff, ivox, boff, bvox = lists_for(vox.cpu().numpy(), nodevox.cpu().numpy())
            ec, ed, el, nc, nd, nl, bc, bl = u8(total + 1), i64(total + 1), i64(total + 1), u8(N + 1), i64(N + 1), i64(N + 1), u8(B + 1), i64(B + 1)      # (never empty)
            cc, counts = np.zeros((K + 1, 3), np.int64), np.zeros(2, np.int64)
            part = lambda: G._check(dll.vmask_compartments(0, *shape, off.data_ptr(), B, vox.data_ptr(), ends.data_ptr(), nodevox.data_ptr(), N, K, ioff.ctypes.data,
                                                           ivox.ctypes.data, boff.ctypes.data, bvox.ctypes.data, ec.data_ptr(), ed.data_ptr(), el.data_ptr(), nc.data_ptr(),
                                                           nd.data_ptr(), nl.data_ptr(), bc.data_ptr(), bl.data_ptr(), cc.ctypes.data, counts.ctypes.data))
            bi, bf, rad, inc, pd, dp, lv = i64(B + 1, 24), f64(B + 1, 5), f64(N + 1), i64(N + 1, 3), f64(N + 1), i64(N + 1, 3), i64(B + 1)
            roots, mc, h = torch.zeros(1, dtype=torch.int64, device=dev), np.zeros(2, np.int64), np.array([0.4, 0.4, 0.6])
            measure = lambda: G._check(dll.vmask_morphometry(0, *shape, dist.data_ptr(), off.data_ptr(), B, vox.data_ptr(), ends.data_ptr(), nodevox.data_ptr(), N,
                                                             h.ctypes.data, roots.data_ptr(), 1 if N else 0, 5, bi.data_ptr(), bf.data_ptr(), rad.data_ptr(), inc.data_ptr(),
                                                             None, pd.data_ptr(), dp.data_ptr(), lv.data_ptr(), mc.ctypes.data))
            row = {'volume': text, 'mask': name, 'branches': B, 'entries': total, 'nodes': N, 'longest': int((off[1:] - off[:-1]).max()) if B else 0}
            row['compartments_ms'] = timed(part, 1, 5)
            row['depthRounds'], row['levelRounds'] = int(counts[0]), int(counts[1])
            row['launches'] = 9 + row['depthRounds'] + row['levelRounds']
            row['owned'], row['reachedTwice'], row['branchesOwned'] = int(cc[1:, 0].sum()), int(cc[0, 1]), int(cc[1:, 2].sum())
            row['morphometry_root_ms'] = timed(measure, 1, 5)
            row['morphometryRounds'] = int(mc[0]) + int(mc[1])
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, dist, graph
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# vmask_compartments: timing\n\n`python tools/compartment_timing.py` on one MI355X, device-resident tables and outputs, HIP events around the C-ABI\n'
                    'calls, one warm call, median of five (ms).  The masks are the bench masks of `tools/segments_timing.py`; the graph is `vmask_branches`\n'
                    'without pruning; five compartments, each entered at one node and shut in by four entries.  Beside it `vmask_morphometry` with one\n'
                    'root on the same graph.  One run, one machine: figures to about two digits.  No threshold is set.\n\n')
            f.write('| volume | mask | branches | entries | nodes | longest branch | compartments, K = 5 | depth rounds | level rounds | launches | vertices owned | reached twice '
                    '| branches owned | morphometry, one root | its rounds |\n')
            f.write('|' + '---|' * 15 + '\n')
            for r in rows:
                f.write('| {volume} | {mask} | {branches} | {entries} | {nodes} | {longest} | {c:.2f} | {depthRounds} | {levelRounds} | {launches} | {owned} | {reachedTwice} '
                        '| {branchesOwned} | {m:.2f} | {morphometryRounds} |\n'.format(c=r['compartments_ms'][0], m=r['morphometry_root_ms'][0], **r))


if __name__ == '__main__':
    main()
