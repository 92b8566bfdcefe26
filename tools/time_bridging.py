"""Time vmask_bridge on a tube phantom with gaps (profiles/vessel_bridging.json).

    python tools/time_bridging.py [--shape 880x880x640] [--gap 4] [--period 80] [--max-cost 16] [--once] [--out FILE]

The phantom: 16 tubes of radius 4 along axis 2 on a 4 x 4 lattice, each winding three turns of amplitude 6 about its axis,
with every voxel whose index i2 has period / 2 <= i2 % period < period / 2 + gap taken out of the mask, so every tube breaks
wherever it crosses one of those slabs; the vesselness is 1 in the uncut tubes and 0 outside, times (0.6 + 0.4 uniform noise); the cost is
vesselCost(floor=0.05) as float32; the domain is the whole volume, every mask voxel a tip (tipRule 0).
Device-resident input, a host clock around reconnect.bridgeCandidates (the call ends in a device synchronise): one warm call,
then the median (min, max) of three.  In the same process, as the yardstick for the brick machinery: geodesicDistance from one
seed on the same mask, and one streaming read of the mask.  --once: one call and nothing else, for a profiler run of its own."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import geodesic as Geo, reconnect as R

BRICK_BYTES = 512 * (8 + 8 + 4 + 1 + 4) + 12       # D, cost, Root, Pred, component word; two flags and a list entry
GRID_BYTES = 12                                    # per brick of the volume: slot grid, brick list, marks


def clocked(fn, warm=1, reps=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def phantom(shape, dev, gap, period, lattice=4, radius=4.0, amp=6.0):
    n0, n1, n2 = shape
    full = torch.zeros(shape, dtype=torch.bool, device=dev)
    z = torch.arange(n2, device=dev, dtype=torch.float32)
    turn = 2.0 * math.pi * 3.0 * z / n2
    reach = int(math.ceil(amp + radius)) + 1
    for a in range(lattice):
        for b in range(lattice):
            c0, c1 = (a + 0.5) * n0 / lattice, (b + 0.5) * n1 / lattice
            lo0, hi0, lo1, hi1 = max(0, int(c0) - reach), min(n0, int(c0) + reach + 2), max(0, int(c1) - reach), min(n1, int(c1) + reach + 2)
            i0 = torch.arange(lo0, hi0, device=dev, dtype=torch.float32)[:, None, None]
            i1 = torch.arange(lo1, hi1, device=dev, dtype=torch.float32)[None, :, None]
            full[lo0:hi0, lo1:hi1, :] |= (i0 - (c0 + amp * torch.sin(turn))) ** 2 + (i1 - (c1 + amp * torch.cos(turn))) ** 2 <= radius ** 2
    k = torch.arange(n2, device=dev) % period
    cut = (k >= period // 2) & (k < period // 2 + gap)
    mask = (full & ~cut[None, None, :]).to(torch.uint8).contiguous()
    noise = torch.rand(shape, device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(1))
    cost = R.vesselCost(full.to(torch.float32) * (0.6 + 0.4 * noise), floor=0.05).to(torch.float32).contiguous()
    return mask, cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='880x880x640')
    ap.add_argument('--gap', type=int, default=4)
    ap.add_argument('--period', type=int, default=80)
    ap.add_argument('--max-cost', type=float, default=R.DEFAULT_MAX_COST)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    shape = tuple(int(x) for x in a.shape.split('x'))
    mask, cost = phantom(shape, dev, a.gap, a.period)
    info = {}
    call = lambda: R.bridgeCandidates(mask, cost, maxCost=a.max_cost, tipRule=0, info=info)
    if a.once:
        call()
        torch.cuda.synchronize()
        print(json.dumps(info))
        return
    row = {'volume': a.shape, 'gap': a.gap, 'period': a.period, 'max_cost': a.max_cost, 'mask_voxels': int(mask.sum())}
    row['bridge_ms'] = clocked(call)
    b = call()
    nbricks = int(np.prod([(n + 7) // 8 for n in shape]))
    row.update(info)
    row.update(volume_bricks=nbricks, brick_storage_bytes=info['bricks'] * BRICK_BYTES + nbricks * GRID_BYTES,
               stored_fraction=info['bricks'] / nbricks, reached_fraction_of_domain=info['reached'] / max(1, info['domain_voxels'] - row['mask_voxels']),
               cost_quartiles=[float(x) for x in np.quantile(b.cost, [0.0, 0.25, 0.5, 0.75, 1.0])] if len(b) else [],
               taken_by_forest=int(len(R.selectBridges(b))))
    seed = torch.nonzero(mask)[:1]
    ginfo = {}
    row['geodesic_one_seed_ms'] = clocked(lambda: Geo.geodesicDistance(mask, seed, info=ginfo))
    row.update(geodesic_bricks=ginfo['bricks'], geodesic_rounds=ginfo['distance_rounds'])
    flat = mask.view(-1)
    n8 = flat.numel() // 8 * 8
    row['read_mask_ms'] = clocked(lambda: flat[:n8].view(torch.int64).sum(), 2, 5)
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(row, f, indent=1)


if __name__ == '__main__':
    main()
