"""Time vmask_geodesic on the bench masks (profiles/geodesic_timing.md).

    python tools/geodesic_timing.py [--shape 512x512x170 ...] [--out FILE] [--md FILE]

Per mask: the skeleton and its segments (not timed), then two workloads with device-resident input and output, a host clock
around the C-ABI call (it ends in a device synchronise: the call reads one counter per round): (1) geodesicTerritories - every
centre-line voxel of a segment a seed, labels, sizes and distance; (2) one seed at the end of the longest segment, distance only.
One warm call, then the median of three.  In the same process, as the yardstick: vmask_territories on the same mask and one
streaming read of the volume."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, geodesic as Geo, skeletonization as S
from segments_timing import masks, timed

WARM, REPS = 1, 3
BRICK_BYTES = {True: 512 * 8 + 512 * 4 + 16, False: 512 * 8 + 16}      # per occupied brick, with and without labels


def clocked(fn):
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        for name, m in masks(shape, dev):
            sk = S.skeletonize(m)
            off, co = S.segmentArrays(sk)
            nseg = int(off.numel()) - 1
            row = {'volume': text, 'mask': name, 'voxels_in': int(m.sum()), 'skeleton_voxels': int(sk.sum()), 'segments': nseg,
                   'brick_grid_bytes': 4 * int(np.prod([(n + 7) // 8 for n in shape]))}
            # workload 1: the territories
            info = {}
            row['territories_geodesic_ms'] = clocked(lambda: S.geodesicTerritories(m, sk, off, co, info=info, return_distance=True))
            labels, sizes, dist = S.geodesicTerritories(m, sk, off, co, info=info, return_distance=True)
            assert int(sizes.sum()) == row['voxels_in'] == info['mask_voxels']
            row.update(bricks=info['bricks'], all_seeds_rounds=[info['distance_rounds'], info['label_rounds']],
                       all_seeds_work_bytes=info['bricks'] * BRICK_BYTES[True] + row['brick_grid_bytes'],
                       all_seeds_ms_per_round=row['territories_geodesic_ms'][0] / max(1, info['distance_rounds'] + info['label_rounds']),
                       unreached=int(sizes[0]))
            del labels, sizes, dist
            # workload 2: one seed at the end of the longest segment
            lengths = off[1:] - off[:-1]
            k = int(torch.argmax(lengths))
            seed = co[int(off[k + 1]) - 1].reshape(1, 3)
            info = {}
            row['single_seed_ms'] = clocked(lambda: Geo.geodesicDistance(m, seed, info=info))
            d = Geo.geodesicDistance(m, seed, info=info)
            reached = torch.isfinite(d) & (d >= 0)
            row.update(longest_segment=int(lengths[k]), single_seed_rounds=info['distance_rounds'], single_seed_reached=info['reached'],
                       single_seed_farthest=float(d[reached].max()), single_seed_work_bytes=info['bricks'] * BRICK_BYTES[False] + row['brick_grid_bytes'],
                       single_seed_ms_per_round=row['single_seed_ms'][0] / max(1, info['distance_rounds']))
            del d, reached
            # the yardsticks
            vox = ((co[:, 0] * shape[1] + co[:, 1]) * shape[2] + co[:, 2]).contiguous()
            lab = torch.empty(shape, dtype=torch.int32, device=dev)
            siz = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
            row['territories_euclidean_ms'] = timed(lambda: G._check(dll.vmask_territories(0, m.data_ptr(), sk.data_ptr(), *shape, off.data_ptr(), nseg,
                                                                                           vox.data_ptr() if len(vox) else None, lab.data_ptr(), None, siz.data_ptr())), WARM, REPS)
            flat = m.view(-1)
            row['read_ms'] = timed(lambda: flat.view(torch.int64).sum(), WARM, REPS)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del m, sk, lab, siz
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            ms = lambda t: '{:.2f} ({:.2f} - {:.2f})'.format(*t)
            f.write('# vmask_geodesic: timing on one MI355X\n\n')
            f.write('`python tools/geodesic_timing.py{}`: device-resident input and output, a host clock around the call (it ends in a device '
                    'synchronise), {} warm call, then the median (min - max) of {}. Workload 1 is `geodesicTerritories` with every centre-line voxel of a '
                    'segment as a seed (labels, sizes and distance); workload 2 is `geodesicDistance` from one seed at the end of the longest segment '
                    '(distance only). `vmask_territories` on the same mask and one streaming read of the mask (`int64` view, `sum`) run in the same '
                    'process (HIP events) as the yardstick. Rounds: distance / label rounds, each one `k_brick_list` (csrc/vbrick.h) + one `k_geo_relax` launch and one 8-byte '
                    'read-back. Work space: 4 bytes per brick of the volume plus 6160 (4112 without labels) per occupied brick; the dense outputs are the '
                    'caller\'s. No time was set as a target.\n\n'.format(''.join(' --shape ' + s for s in a.shape), WARM, REPS))
            f.write('| volume | mask | mask voxels | segments | occupied bricks | all seeds ms | rounds D / labels | ms per round | work MB | one seed ms | rounds | ms per round | '
                    'reached | farthest | work MB | Euclidean territories ms | read ms |\n' + '|---' * 17 + '|\n')
            for r in rows:
                f.write('| {} | {} | {} | {} | {} | {} | {} / {} | {:.3f} | {:.1f} | {} | {} | {:.3f} | {} | {:.1f} | {:.1f} | {} | {} |\n'.format(
                    r['volume'], r['mask'], r['voxels_in'], r['segments'], r['bricks'], ms(r['territories_geodesic_ms']), r['all_seeds_rounds'][0],
                    r['all_seeds_rounds'][1], r['all_seeds_ms_per_round'], r['all_seeds_work_bytes'] / 1e6, ms(r['single_seed_ms']), r['single_seed_rounds'],
                    r['single_seed_ms_per_round'], r['single_seed_reached'], r['single_seed_farthest'], r['single_seed_work_bytes'] / 1e6,
                    ms(r['territories_euclidean_ms']), ms(r['read_ms'])))


if __name__ == '__main__':
    main()
