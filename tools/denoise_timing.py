"""Time vmask_diffuse and vmask_median (profiles/denoise_timing.md).

    python tools/denoise_timing.py [--shape 512x512x170 ...] [--once] [--no-cpu] [--out FILE]

Per volume: a float32 bench volume that lives on the GPU; the C-ABI calls with device-resident input and output, two warm
calls, the median (min, max) of five, HIP events around the call.  A diffusion call allocates and frees its float64 work
volume, so a step is timed as the difference of a call of 5 steps and a call of 1 step over 4 - float64 to float64 steps; the
call of 1 step (the float32 first step and everything a call does besides) is given beside it.  The bytes are what must move
at least once - 16 per voxel and step (12 on a float32 first step), 2 sizeof(T) per voxel for the median - and the fractions
are bytes / time over the 8 TB/s specification and over the 6.29 TB/s measured for a plain copy.  The CPU line is the numpy
model and scipy's median at 128^3 on this host.  --once: one call of each kind per volume and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/denoise_timing.py --once` run of its own, which gives the milliseconds
per kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, phantoms, denoise as DN

PEAK, COPY = 8.0e12, 6.29e12
K = 15.0


def timed(fn, warm=2, reps=5):
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


def rates(nbytes, ms):
    return {'bytes': int(nbytes), 'TBs': round(nbytes / (ms * 1e-3) / 1e12, 3), 'of_8TBs': round(nbytes / (ms * 1e-3) / PEAK, 3),
            'of_copy': round(nbytes / (ms * 1e-3) / COPY, 3), 'times_bytes_over_copy': round(ms * 1e-3 / (nbytes / COPY), 2)}


def cpu_baseline():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import denoise_model as M
    I = np.random.default_rng(0).normal(0.0, 5.0, (128, 128, 128))
    I[:, 64:, :] += 100.0
    row = {'volume': '128x128x128', 'threads': os.cpu_count()}
    for function in ('rational', 'exponential'):
        t0 = time.perf_counter()
        M.diffuse(I, K, 1, function=function)
        row['model_step_{}_s'.format(function)] = round(time.perf_counter() - t0, 3)
    for radius in ((1, 1, 1), (1, 1, 0)):
        for dtype in (np.float32, np.float64):
            v = I.astype(dtype)
            t0 = time.perf_counter()
            M.median_scipy(v, radius)
            row['scipy_median_{}_{}_s'.format(''.join(map(str, radius)), np.dtype(dtype).name)] = round(time.perf_counter() - t0, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = DN._lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        I, vm = phantoms.bench_volume_torch(shape, dev, tubes=16, seed_mode='whole')
        del vm
        vol = {4: I.to(torch.float32).contiguous()}
        del I
        V = vol[4].numel()
        out64 = torch.empty(shape, dtype=torch.float64, device=dev)

        def diffuse(iterations, function):
            G._check(dll.vmask_diffuse(0, vol[4].data_ptr(), 5, *shape, None, K, iterations, 0.0, function, out64.data_ptr()))

        def median(size, radius, to):
            G._check(dll.vmask_median(0, vol[size].data_ptr(), 5 if size == 4 else 6, *shape, *radius, to.data_ptr()))
        torch.cuda.synchronize()
        row = {'volume': text, 'voxels': V}
        if a.once:
            for function in (0, 1):
                diffuse(2, function)
        else:
            for function, name in ((0, 'rational'), (1, 'exponential')):
                one, five = timed(lambda: diffuse(1, function)), timed(lambda: diffuse(5, function))
                step = (five[0] - one[0]) / 4.0
                row['diffuse_' + name] = {'call_1_step_ms': one, 'call_5_steps_ms': five, 'step_ms': round(step, 4), 'step': rates(16 * V, step),
                                          'first_step_call': rates(12 * V, one[0])}
            row['diffuse_checksum'] = float(out64.sum())
        out32 = torch.empty(shape, dtype=torch.float32, device=dev)
        for size in (4, 8):
            if size == 8:
                vol[8] = vol[4].to(torch.float64)
            to = out32 if size == 4 else out64
            for radius in ((1, 1, 1), (1, 1, 0)):
                if a.once:
                    median(size, radius, to)
                else:
                    ms = timed(lambda: median(size, radius, to))
                    row['median_{}_float{}'.format(''.join(map(str, radius)), 8 * size)] = {'call_ms': ms, 'call': rates(2 * size * V, ms[0])}
        torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        rows.append(row)
        del vol, out32, out64
        torch.cuda.empty_cache()
    if not a.no_cpu and not a.once:
        row = cpu_baseline()
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
