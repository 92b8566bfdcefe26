"""Times the stages of the nonlinear registration (arterynetwork_amd/registration.py, DESIGN.md section 9 entry f18) on an analytic
phantom that is built on the device: a soft-edged ellipsoid head with a smooth texture, float32, and the same head displaced by a
smooth field of a few voxels with other intensities as the moving volume.

    python tools/time_nonlinear.py [--sizes 512x512x170 880x880x640] [--repeats 5] [--out profiles/nonlinear_registration.json]

Per size: one warm-up, then the median over `--repeats` runs, HIP events around each stage on device tensors: the force pass
(``forcePass``), the three-numerator fit (``fitForces``), one whole iteration (``warpLevel(iterations=1)``: force pass, fit,
evaluation and update, the copies to the host), the warp of the next level (``upsampleWarp`` from half the extents) and the
resampled volume (``warpResample``, trilinear); the bytes that each stage has to move at the least; and one whole
``registerNonlinear`` (wall time)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the HIP library: one ROCm runtime per process)

from arterynetwork_amd import registration as R  # noqa: E402

SPANS = (8, 8, 8)                                           # the finest level of the defaults: splineSpans (2, 2, 2) at level 2
STAGES = ('force', 'fit', 'iteration', 'upsample', 'resample')


def head(shape, device, shift):
    """The head on the grid of `shape`, its coordinates displaced by `shift` times a smooth field (voxels), float32."""
    c = [(torch.arange(n, dtype=torch.float32, device=device) + 0.5) / n * 2.0 - 1.0 for n in shape]
    x, y, z = c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]
    if shift:
        x = x + (2.0 * shift / shape[0]) * torch.sin(1.5 * y) * torch.cos(1.2 * z)
        y = y + (2.0 * shift / shape[1]) * torch.cos(1.4 * x) * torch.sin(1.1 * z)
    rho = torch.sqrt(x * x + y * y + z * z)
    out = 100.0 * torch.sigmoid((0.9 - rho) * (0.25 * min(shape))) + 60.0 * torch.sigmoid((0.6 - rho) * (0.25 * min(shape)))
    out = out * (1.0 + 0.15 * torch.sin(x * (shape[0] / 6.0)) * torch.sin(y * (shape[1] / 6.0) + 1.0) * torch.sin(z * (shape[2] / 6.0) + 2.0))
    return out.contiguous()


def least_bytes(shape):
    """What each stage has to read and write at the least, in bytes (float32 volumes, no mask, float64 warp and forces; the 8 gathered
    moving values of a voxel counted as the moving volume read once; the lattices and the column sums left out)."""
    V = shape[0] * shape[1] * shape[2]
    K0 = SPANS[0] + 3
    plane = shape[1] * shape[2]
    force = (4 + 24 + 4 + 24 + 1) * V
    fit = (24 + 1) * V + 32 * K0 * plane
    add = 24 * K0 * plane + 48 * V
    return {'force': force, 'fit': fit, 'iteration': force + fit + add, 'upsample': 24 * V + 3 * V, 'resample': (4 + 24 + 8) * V}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def measure(shape, repeats, device):
    fixed, moving = head(shape, device, 0.0), 0.7 * head(shape, device, 2.0) + 20.0
    flo, fhi = R.extrema(fixed)
    mlo, mhi = R.extrema(moving)
    scales = (flo, R.binScale(flo, fhi, 1), mlo, R.binScale(mlo, mhi, 1))
    T = np.eye(4)
    u = torch.zeros((3,) + shape, dtype=torch.float64, device=device)
    coarse = torch.zeros((3,) + tuple((n + 1) // 2 for n in shape), dtype=torch.float64, device=device)
    ms = {k: [] for k in STAGES}
    count = cost = None
    for i in range(repeats + 1):                           # (the first run warms up)
        t, (delta, part, S, count) = timed(lambda: R.forcePass(fixed, moving, T, u, *scales))
        cost = S / count
        t_fit, _ = timed(lambda: R.fitForces(delta, part, SPANS))
        del delta, part
        w = torch.zeros_like(u)
        t_it, _ = timed(lambda: R.warpLevel(fixed, moving, T, w, *scales, SPANS, iterations=1))
        t_up, _ = timed(lambda: R.upsampleWarp(coarse, shape))
        t_re, _ = timed(lambda: R.warpResample(moving, None, w, order=1))
        del w
        if i:
            for k, v in zip(STAGES, (t, t_fit, t_it, t_up, t_re)):
                ms[k].append(v)
    med = {k: statistics.median(v) for k, v in ms.items()}
    least = least_bytes(shape)
    del u, coarse
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    warp, trace = R.registerNonlinear(fixed, moving, iterations=10)
    torch.cuda.synchronize()
    whole = time.perf_counter() - t0
    return {'shape': list(shape), 'voxels': shape[0] * shape[1] * shape[2], 'input': 'float32', 'repeats': repeats, 'spans': list(SPANS),
            'stage_ms': med, 'least_bytes': least, 'least_GB_per_s': {k: (least[k] / 1e9) / (med[k] / 1e3) for k in STAGES},
            'voxels_taking_part': int(count), 'cost_at_zero_warp': cost,
            'register_nonlinear': {'levels': 3, 'iterations': 10, 'seconds': whole, 'rows': int(len(trace)), 'first_cost': float(trace[0, 1]),
                                   'last_cost': float(trace[-1, 1]), 'max_abs_warp': float(warp.abs().max())}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', nargs='+', default=['512x512x170', '880x880x640'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nonlinear_registration.json'))
    a = ap.parse_args()
    device = torch.device('cuda', 0)
    result = {'device': torch.cuda.get_device_name(0), 'parameters': dict(maxStep=0.5, mask=None), 'sizes': []}
    for s in a.sizes:
        shape = tuple(int(x) for x in s.split('x'))
        r = measure(shape, a.repeats, device)
        result['sizes'].append(r)
        print(json.dumps(r), flush=True)
        with open(a.out, 'w') as f:                         # (after every size: a later size that fails leaves the earlier ones)
            json.dump(result, f, indent=1)
            f.write('\n')
    print('written to {}'.format(a.out))


if __name__ == '__main__':
    main()
