"""Time the bias-field correction (profiles/bias_timing.md).

    python tools/bias_timing.py [--shape 512x512x170 ...] [--once] [--out FILE]

Per volume: a float32 three-class phantom under a smooth field that lives on the GPU; the C-ABI calls with device-resident
input and output, one warm call, the median (min, max) of three, HIP events around the call.  A call allocates its work
volumes, takes the logarithm and the exponential and copies nothing, so an iteration is timed as the difference of a call
of 6 iterations and a call of 1 iteration over 5, on one level, with a threshold that never ends the level; once with the
lattice of the first default level (1 span per axis, 4 control points) and once with that of the third (4 spans, 7).  The fit
and the evaluation are also timed alone through their own entries (calls: tables, allocations and the three launches each).
The bytes are what must move at least once.  --once: one call of two iterations per volume and nothing else, for a
`rocprofv3 --kernel-trace --stats -- python tools/bias_timing.py --once` run of its own, which gives the milliseconds per
kernel."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, bias as B

COPY = 6.29e12


def timed(fn, warm=1, reps=3):
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
    return round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)


def rates(nbytes, ms):
    return {'bytes': int(nbytes), 'TBs': round(nbytes / (ms * 1e-3) / 1e12, 3), 'times_bytes_over_copy': round(ms * 1e-3 / (nbytes / COPY), 2)}


def phantom(shape, dev):
    """Three classes in blocks of 8 voxels and a background of 0 outside an ellipsoid, times a smooth field; float32."""
    ax = [(torch.arange(n, device=dev, dtype=torch.float32) + 0.5) / n * 2.0 - 1.0 for n in shape]
    x, y, z = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    idx = [torch.arange(n, device=dev) // 8 for n in shape]
    cls = (idx[0][:, None, None] + 2 * idx[1][None, :, None] + idx[2][None, None, :]) % 3
    I = (100.0 + 60.0 * cls.to(torch.float32)) * torch.exp(0.3 * (0.8 * x - 0.5 * y + 0.6 * z * z - 0.4 * x * y))
    I = I * ((x * x + y * y + z * z) < 0.9).to(torch.float32)
    return I.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = B._lib()
    rows = []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        I = phantom(shape, dev)
        V = I.numel()
        out = torch.empty(shape, dtype=torch.float64, device=dev)
        trace = np.zeros((64, 4))
        count = np.zeros(1, np.int64)

        def correct(spans, iterations):
            m0 = np.array(spans, dtype=np.intc)
            G._check(dll.vmask_bias_correct(0, I.data_ptr(), 5, None, *shape, m0.ctypes.data, 1, iterations, 1e-300, 200, 0.15, 0.01,
                                            out.data_ptr(), None, trace.ctypes.data, count.ctypes.data))
            assert count[0] == iterations
        torch.cuda.synchronize()
        row = {'volume': text, 'voxels': V}
        if a.once:
            correct((1, 1, 1), 2)
        else:
            plane = shape[1] * shape[2]
            for spans in ((1, 1, 1), (4, 4, 4)):
                K0 = spans[0] + 3
                one, six = timed(lambda: correct(spans, 1)), timed(lambda: correct(spans, 6))
                it = (six[0] - one[0]) / 5.0
                # min / max 17, histogram 17, residual 25, axis-0 fit 9 and 16 K0 per column, last expansion 16 and 8 K0 per column
                nbytes = (17 + 17 + 25 + 9 + 16) * V + 24 * K0 * plane
                row['spans_{}'.format(spans[0])] = {'call_1_iteration_ms': one, 'call_6_iterations_ms': six, 'iteration_ms': round(it, 3),
                                                    'iteration': rates(nbytes, it), 'max_phi_last': float(trace[5, 1])}
            r = torch.empty(shape, dtype=torch.float64, device=dev).normal_()
            m = (I > 0).to(torch.uint8)
            for spans in ((1, 1, 1), (4, 4, 4)):
                K = [s + 3 for s in spans]
                M = np.array(spans, dtype=np.intc)
                phi = torch.empty(K, dtype=torch.float64, device=dev)
                fit = timed(lambda: G._check(dll.vmask_bias_fit(0, r.data_ptr(), m.data_ptr(), *shape, M.ctypes.data, phi.data_ptr())))
                ev = timed(lambda: G._check(dll.vmask_bias_eval(0, phi.data_ptr(), M.ctypes.data, *shape, out.data_ptr())))
                row['fit_call_spans_{}'.format(spans[0])] = {'call_ms': fit, 'axis0_pass': rates(9 * V + 16 * K[0] * plane, fit[0])}
                row['eval_call_spans_{}'.format(spans[0])] = {'call_ms': ev, 'last_expansion': rates(8 * V + 8 * K[0] * plane, ev[0])}
            del r, m
        torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        rows.append(row)
        del I, out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
