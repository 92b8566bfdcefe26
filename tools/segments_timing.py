"""Time vmask_segments on the skeletons of the bench masks (profiles/segments_timing.md).

    python tools/segments_timing.py [--shape 512x512x170 ...] [--once] [--out FILE]

Per mask: the skeleton (vmask_skeleton, timed the same way for scale), then vmask_segments with device-resident input and
output: three warm calls, the median of ten, HIP events around the C-ABI call.  --once: one call per mask and nothing else,
for a `rocprofv3 --kernel-trace --stats -- python tools/segments_timing.py --once` run of its own."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, phantoms, skeletonization as S


def masks(shape, dev):
    for tubes, kind in ((1, 'stage-1'), (16, 'stage-1'), (16, 'clean')):
        I, vm = phantoms.bench_volume_torch(shape, dev, tubes=tubes, seed_mode='whole')
        if kind == 'clean':
            m = (vm == 0)
        else:
            m = G.vesselVolumeMask((vm != 4).to(torch.uint8).contiguous(), I.contiguous())
        del I, vm
        yield '{}, {} tube{}'.format(kind, tubes, 's' if tubes > 1 else ''), (m != 0).to(torch.uint8).contiguous()


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        for name, m in masks(shape, dev):
            sk = torch.empty_like(m)
            kept, cycles = C.c_int64(), C.c_int64()
            skel = lambda: G._check(dll.vmask_skeleton(0, m.data_ptr(), *m.shape, sk.data_ptr(), C.byref(kept), C.byref(cycles)))
            torch.cuda.synchronize()
            skel()
            counts = np.zeros(5, np.int64)
            G._check(dll.vmask_segments(0, sk.data_ptr(), *sk.shape, counts.ctypes.data, None, 0, None, 0))
            nseg, total = int(counts[0]), int(counts[1])
            offsets = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
            voxels = torch.empty(max(1, total), dtype=torch.int64, device=dev)
            seg = lambda: G._check(dll.vmask_segments(0, sk.data_ptr(), *sk.shape, counts.ctypes.data, offsets.data_ptr(), nseg, voxels.data_ptr(), total))
            row = {'volume': text, 'mask': name, 'voxels_in': int(m.sum()), 'skeleton_voxels': int(kept.value), 'segments': nseg, 'entries': total,
                   'nodes': int(counts[2]), 'isolated': int(counts[3])}
            if a.once:
                seg()
                torch.cuda.synchronize()
            else:
                row['segments_ms'] = timed(seg, 3, 10)
                row['skeleton_ms'] = timed(skel, 1, 5)
                flat = m.view(-1)
                row['read_ms'] = timed(lambda: flat.view(torch.int64).sum(), 2, 10)
            row['rounds'] = int(counts[4])
            longest = int((offsets[1:] - offsets[:-1]).max()) if nseg else 0
            row['longest_segment'] = longest
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, offsets, voxels
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
