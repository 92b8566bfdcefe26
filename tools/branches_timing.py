"""Time vmask_branches on the skeletons of the bench masks (profiles/branches_timing.md).

    python tools/branches_timing.py [--shape 512x512x170 ...] [--out FILE]

Per mask: the skeleton, then with device-resident input and output, HIP events around the C-ABI calls, one warm call and the
median of five: vmask_segments and vmask_skeleton (of the skeleton itself: one thinning call of a pruning round), vmask_branches
without pruning (one graph build) and with prune = (3, 1.0) on the distance transform of the mask.  The graph build is given as
a multiple of vmask_segments, a pruning round as a multiple of one thinning call plus one trace."""
import argparse
import ctypes as C
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
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        for name, m in masks(shape, dev):
            sk, again = torch.empty_like(m), torch.empty_like(m)
            G._check(dll.vmask_skeleton(0, m.data_ptr(), *m.shape, sk.data_ptr(), None, None))
            dist = G.distance_transform_edt(m)
            nobj = int(torch.count_nonzero(sk))
            sc, bc = np.zeros(5, np.int64), np.zeros(12, np.int64)
            alloc = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
            out = torch.empty_like(m)
            # the sizes first (counts-only calls, not timed); the pruned graph is measured with the larger of the two
            G._check(dll.vmask_segments(0, sk.data_ptr(), *sk.shape, sc.ctypes.data, None, 0, None, 0))
            cap_seg, cap_ent = int(sc[0]), int(sc[1])
            cn = cb = cv = 0
            for min_len, factor, d in ((0, 0.0, None), (3, 1.0, dist.data_ptr())):
                G._check(dll.vmask_branches(0, sk.data_ptr(), *sk.shape, min_len, factor, d, 64, None, bc.ctypes.data, None, 0, None, None, 0, None, 0))
                cn, cb, cv = max(cn, int(bc[0])), max(cb, int(bc[4])), max(cv, int(bc[5]))
            soff, svox = alloc(cap_seg + 1), alloc(cap_ent + 1)
            nodes, ends, off, vox = alloc(4 * cn + 1), alloc(2 * cb + 1), alloc(cb + 1), alloc(cv + 1)       # (never empty: an empty tensor has no address)
            seg = lambda: G._check(dll.vmask_segments(0, sk.data_ptr(), *sk.shape, sc.ctypes.data, soff.data_ptr(), cap_seg, svox.data_ptr(), cap_ent))
            thin = lambda: G._check(dll.vmask_skeleton(0, sk.data_ptr(), *sk.shape, again.data_ptr(), None, None))

            def graph(min_len, factor, d):
                return lambda: G._check(dll.vmask_branches(0, sk.data_ptr(), *sk.shape, min_len, factor, d, 64, out.data_ptr(), bc.ctypes.data,
                                                           nodes.data_ptr(), cn, ends.data_ptr(), off.data_ptr(), cb, vox.data_ptr(), cv))
            row = {'volume': text, 'mask': name, 'skeleton_voxels': nobj}
            row['segments_ms'] = timed(seg, 1, 5)
            row['thinning_ms'] = timed(thin, 1, 5)
            row['graph_ms'] = timed(graph(0, 0.0, None), 1, 5)
            row.update(segments=int(sc[0]), **{k: int(c) for k, c in zip(S.BRANCH_COUNTS, bc)})
            row['pruned_ms'] = timed(graph(3, 1.0, dist.data_ptr()), 1, 5)
            row['pruned'] = {k: int(c) for k, c in zip(S.BRANCH_COUNTS, bc)}
            rounds = row['pruned']['pruneRounds']
            row['graph_over_segments'] = round(row['graph_ms'][0] / row['segments_ms'][0], 2)
            if rounds:                                                   # (rounds + 1 graph builds, rounds thinning calls)
                row['round_over_thin_plus_trace'] = round((row['pruned_ms'][0] - row['graph_ms'][0]) / rounds / (row['thinning_ms'][0] + row['segments_ms'][0]), 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, again, dist, soff, svox, nodes, ends, off, vox, out
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
