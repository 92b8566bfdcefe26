"""Time vmask_territories on the skeletons of the bench masks (profiles/territories_timing.md).

    python tools/territories_timing.py [--shape 512x512x170 ...] [--once] [--out FILE] [--md FILE]

Per mask: the skeleton and its segments (not timed), then vmask_territories with device-resident input and output: three warm
calls, the median of ten, HIP events around the C-ABI call.  In the same process, as the yardstick: vmask_edt on the same mask
and one streaming read of the volume.  --once: one call per mask and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/territories_timing.py --once` run of its own."""
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

HBM_PEAK = 8.0e12                                        # bytes per second
WARM, REPS = 3, 10
# what the passes must move per voxel: clearing the site labels 4, rows 1 + 2, axis 1 2 + 6, axis 0 4 + 1 + 4 + 8
BYTES_PER_VOXEL = 4 + 3 + 8 + 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        V = int(np.prod(shape))
        for name, m in masks(shape, dev):
            sk = S.skeletonize(m)
            off, co = S.segmentArrays(sk)
            vox = ((co[:, 0] * shape[1] + co[:, 1]) * shape[2] + co[:, 2]).contiguous()
            nseg = int(off.numel()) - 1
            labels = torch.empty(shape, dtype=torch.int32, device=dev)
            nearest = torch.empty(shape, dtype=torch.int64, device=dev)
            sizes = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
            ter = lambda: G._check(dll.vmask_territories(0, m.data_ptr(), sk.data_ptr(), *shape, off.data_ptr(), nseg, vox.data_ptr() if len(vox) else None,
                                                         labels.data_ptr(), nearest.data_ptr(), sizes.data_ptr()))
            torch.cuda.synchronize()
            row = {'volume': text, 'mask': name, 'voxels_in': int(m.sum()), 'skeleton_voxels': int(sk.sum()), 'segments': nseg}
            if a.once:
                ter()
                torch.cuda.synchronize()
            else:
                row['territories_ms'] = timed(ter, WARM, REPS)
                dist = torch.empty(shape, dtype=torch.float64, device=dev)
                row['edt_ms'] = timed(lambda: G._check(dll.vmask_edt(0, m.data_ptr(), *shape, dist.data_ptr())), WARM, REPS)
                del dist
                flat = m.view(-1)
                row['read_ms'] = timed(lambda: flat.view(torch.int64).sum(), WARM, REPS)
                row['ratio_to_edt'] = row['territories_ms'][0] / row['edt_ms'][0]
                row['bytes_per_voxel'] = BYTES_PER_VOXEL
                row['share_of_8TBps'] = BYTES_PER_VOXEL * V / HBM_PEAK / (row['territories_ms'][0] * 1e-3)
            row['unassigned'] = int(sizes[0])
            row['largest_territory'] = int(sizes[1:].max()) if nseg else 0
            assert int(sizes.sum()) == row['voxels_in']
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, labels, nearest, sizes
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if a.md and not a.once:
        with open(a.md, 'w') as f:
            f.write('# vmask_territories: timing on one MI355X\n\n')
            f.write('`python tools/territories_timing.py`: device-resident input and output, HIP events around the C-ABI call, {} warm calls, '
                    'then the median (min - max) of {}. `vmask_edt` on the same mask and one streaming read of the mask (`int64` view, `sum`) '
                    'run in the same process and are unchanged by this feature: they are the yardstick. Bytes that the passes must move: '
                    '{} per voxel (DESIGN.md section 9, f8); the share is those bytes over the median time against 8 TB/s.\n\n'.format(WARM, REPS, BYTES_PER_VOXEL))
            f.write('| volume | mask | mask voxels | skeleton voxels | segments | territories ms | edt ms | ratio | read ms | share of 8 TB/s |\n|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                ms = lambda t: '{:.3f} ({:.3f} - {:.3f})'.format(*t)
                f.write('| {} | {} | {} | {} | {} | {} | {} | {:.2f} | {} | {:.3f} |\n'.format(
                    r['volume'], r['mask'], r['voxels_in'], r['skeleton_voxels'], r['segments'], ms(r['territories_ms']), ms(r['edt_ms']),
                    r['ratio_to_edt'], ms(r['read_ms']), r['share_of_8TBps']))


if __name__ == '__main__':
    main()
