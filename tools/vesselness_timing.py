"""Time vmask_vesselness (profiles/vesselness_timing.md).

    python tools/vesselness_timing.py [--shape 512x512x170 ...] [--once] [--no-cpu] [--out FILE]

Per volume: a float32 bench volume that lives on the GPU, four scales, automatic gamma and a brain mask; the C-ABI call with
device-resident input and output, two warm calls, the median of five, HIP events around the call.  Then each scale alone,
with automatic and with fixed gamma: their difference is the norm-only run of the axis-0 pass.  The bytes are what the
passes must move (computed from the shape, below); the fraction is bytes / time over 8 TB/s - of the whole call, not of a
kernel.  The CPU baseline is the scipy model of the test suite at 128^3 on this host.  --once: one call per volume and
nothing else, for a `rocprofv3 --kernel-trace --stats -- python tools/vesselness_timing.py --once` run of its own, which
gives the milliseconds per kernel."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, phantoms, vesselness as VS

SIGMAS = np.array([0.6, 1.0, 1.6, 2.5])
PEAK = 8.0e12


def pass_bytes(V, in_bytes, auto, masked, scale_out=True):
    """Bytes per scale that each pass has to move at least once."""
    b = {'axis2': V * (in_bytes + 3 * 8), 'axis1': V * (3 * 8 + 6 * 8)}
    if auto:
        b['axis0_norm'] = V * (6 * 8 + (1 if masked else 0))
    b['axis0_measure'] = V * (6 * 8 + (1 if masked else 0) + 2 * 8 + (1 if scale_out else 0))     # (out is read and, where it grows, written)
    return b


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


def cpu_baseline():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import vesselness_model as M
    I = np.random.default_rng(0).normal(0.0, 10.0, (128, 128, 128))
    I[:, 60:68, 60:68] += 100.0
    t0 = time.perf_counter()
    M.vesselness(I, SIGMAS)
    return {'volume': '128x128x128', 'scipy_model_s': round(time.perf_counter() - t0, 3), 'scales': len(SIGMAS), 'threads': os.cpu_count()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = VS._lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        I, vm = phantoms.bench_volume_torch(shape, dev, tubes=16, seed_mode='whole')
        I = I.to(torch.float32).contiguous()
        brain = (vm != 4).to(torch.uint8).contiguous()
        del vm
        V = I.numel()
        out = torch.empty(shape, dtype=torch.float64, device=dev)
        scale = torch.empty(shape, dtype=torch.uint8, device=dev)
        gammas = np.zeros(len(SIGMAS))

        def call(sig, gamma):
            sig = np.ascontiguousarray(sig, dtype=np.float64)
            G._check(dll.vmask_vesselness(0, I.data_ptr(), 5, *shape, brain.data_ptr(), sig.ctypes.data, len(sig), None, 0.5, 0.5, float(gamma), 1,
                                          out.data_ptr(), scale.data_ptr(), gammas.ctypes.data))
        torch.cuda.synchronize()
        row = {'volume': text, 'voxels': V, 'scales': [float(s) for s in SIGMAS], 'radii': [int(4 * s + 0.5) for s in SIGMAS]}
        if a.once:
            call(SIGMAS, 0.0)
            torch.cuda.synchronize()
        else:
            row['call_ms'] = timed(lambda: call(SIGMAS, 0.0), 2, 5)
            total = sum(sum(pass_bytes(V, 4, True, True).values()) for _ in SIGMAS)
            row['call_bytes'] = total
            row['call_fraction_of_8TBs'] = round(total / (row['call_ms'][0] * 1e-3) / PEAK, 4)
            row['per_scale'] = []
            for s in SIGMAS:
                auto = timed(lambda: call([s], 0.0), 1, 5)
                fixed = timed(lambda: call([s], 15.0), 1, 5)
                b = pass_bytes(V, 4, True, True)
                row['per_scale'].append({'sigma': float(s), 'radius': int(4 * s + 0.5), 'auto_gamma_ms': auto, 'fixed_gamma_ms': fixed,
                                         'norm_pass_ms': round(auto[0] - fixed[0], 3), 'bytes': b,
                                         'auto_fraction_of_8TBs': round(sum(b.values()) / (auto[0] * 1e-3) / PEAK, 4)})
            row['gammas'] = [float(g) for g in gammas]
            row['max'] = float(out.max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del I, brain, out, scale
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
