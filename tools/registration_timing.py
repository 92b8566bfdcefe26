"""Time the registration (profiles/registration_timing.md).

    python tools/registration_timing.py [--shape 512x512x170 ...] [--out FILE] [--no-register]

Per volume: a float32 head that lives on the GPU - an ellipsoid that holds about half of the voxels, classes in blocks of 8 voxels
with Gaussian noise, background exactly 0, so half of the fixed voxels fall into bin 0 - and as the moving volume the same head
turned by 3 degrees and shifted, resampled by the library, with noise of its own.  One joint-histogram evaluation is the C entry
with device-resident bin image and moving volume under a 10 degree rotation about the grid's centre: the memset of the counts,
one launch, the synchronisation and the copy of bins^2 counts, HIP events around the call; two warm calls, then the median
(min - max) of seven; a second histogram of the same call must equal the first.  The time is set against the bin
image's bytes (1 per voxel) over the 6.29 TB/s of a plain copy.  A whole register(levels=3) of the pair, device tensors in, is
timed by the host clock, twice.  Writes the tables as markdown; what the file holds below its marker line (a hand-kept record of variants
that were measured once and taken out of the code) is kept as it is."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, registration as R

COPY = 6.29e12
BINS = 64
KEPT = '<!-- hand-kept record below this line: tools/registration_timing.py does not write it and keeps it when it rewrites the file -->'
PREAMBLE = """# Registration: timing (MI355X)

Written by `python tools/registration_timing.py` (one run, one GPU, run separately from the suite).  A float32 head resident on the device: an
ellipsoid that holds about half of the voxels, classes in blocks of 8 voxels with Gaussian noise, background exactly 0 ("in bin 0": the share of
the fixed voxels in bin 0); the moving volume is the same head turned by 3 degrees and shifted, resampled by the library, with noise of its own.
One joint-histogram evaluation is `vmask_reg_joint_hist` with device-resident bin image and moving volume, 64 bins, under a 10 degree
rotation about each axis around the grid's centre ("counted": the share of the fixed voxels whose sample is inside): the memset of the counts, one
launch, the synchronisation and the copy of 4096 counts, HIP events around the call; two warm calls, then the median (min – max) of seven.  "×" is
the time over the bin image's bytes (1 per voxel) at the 6.29 TB/s measured for a plain copy; the eight gathers per voxel come on top of those
bytes.  `register(levels=3)` of the pair, device tensors in, default parameters, by the host clock, twice.  No threshold is set and no test asserts a time; the parent commit has nothing to compare with.

"""


def head(shape, dev, seed):
    ax = [(torch.arange(n, device=dev, dtype=torch.float32) + 0.5) / n * 2.0 - 1.0 for n in shape]
    x, y, z = ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :]
    idx = [torch.arange(n, device=dev) // 8 for n in shape]
    cls = (idx[0][:, None, None] + 2 * idx[1][None, :, None] + idx[2][None, None, :]) % 3
    gen = torch.Generator(device=dev).manual_seed(seed)
    I = 100.0 + 60.0 * cls.to(torch.float32) + 8.0 * torch.randn(shape, device=dev, generator=gen)
    inside = (x * x + 1.2 * y * y + 0.9 * z * z) < 1.0             # about half of the box
    return (I * inside.to(torch.float32)).contiguous()


def centred(shape, params):
    c = (np.array(shape, dtype=np.float64) - 1.0) / 2.0
    return R.paramsToMatrix(params, 6, c)


def timed(fn, warm=2, reps=7):
    ms = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'registration_timing.md'))
    ap.add_argument('--no-register', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = R._lib()
    rows, runs = [], []
    for text in a.shape or ['512x512x170', '880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        fixed = head(shape, dev, 1)
        W_true = centred(shape, [3.0, -2.0, 1.5] + list(np.deg2rad([3.0, -2.0, 2.5])))
        moving = R.resample(fixed, W_true, shape, order=1, fill=0).to(torch.float32)     # moving(v) = fixed(W_true v): identity affines
        moving = (moving + (moving > 0).to(torch.float32) * 8.0 * torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(2))).contiguous()
        flo, fhi = R.extrema(fixed)
        fb, inside = R.quantise(fixed, flo, R.binScale(flo, fhi, BINS), BINS)
        mlo, mhi = R.extrema(moving)
        ms = R.binScale(mlo, mhi, BINS)
        background = float((fb == 0).sum().item()) / fb.numel()
        T = np.ascontiguousarray(np.linalg.inv(centred(shape, [0.0, 0.0, 0.0] + [np.deg2rad(10.0)] * 3))[:3])
        H = [np.zeros((BINS, BINS), np.uint64) for _ in range(2)]

        def call(k):
            G._check(dll.vmask_reg_joint_hist(0, fb.data_ptr(), *shape, moving.data_ptr(), 5, *shape, T.ctypes.data, BINS, mlo, ms, H[k].ctypes.data))
        torch.cuda.synchronize()
        call(1)
        ms_eval = timed(lambda: call(0))
        assert np.array_equal(H[0], H[1]) and H[0].sum() > 0
        V = fb.numel()
        floor_ms = V / COPY * 1e3
        rows.append((text, V, background, int(H[0].sum()) / V, floor_ms, ms_eval))
        print(rows[-1], flush=True)
        if not a.no_register:
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                W, trace = R.register(fixed, moving, levels=3)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                d = np.abs(W - W_true).max()
                runs.append((text, dt, trace['evaluations'].tolist(), len(trace['steps']), float(d)))
                print(runs[-1], flush=True)
        del fixed, moving, fb
        torch.cuda.empty_cache()

    def f(t):
        return '{:.3f} ms ({:.3f} – {:.3f})'.format(*t)
    lines = ['| volume | voxels | in bin 0 | counted | bin image / 6.29 TB/s | one evaluation | × | voxels per ns |', '|---|---|---|---|---|---|---|---|']
    for text, V, bg, counted, floor_ms, t in rows:
        lines.append('| {} | {:.2e} | {:.2f} | {:.2f} | {:.3f} ms | {} | {:.1f} | {:.1f} |'.format(text.replace('x', '×'), V, bg, counted, floor_ms, f(t), t[0] / floor_ms, V / (t[0] * 1e6)))
    if runs:
        lines += ['', '| volume | register(levels=3) | evaluations per level | accepted steps | max abs(W − W_true) |', '|---|---|---|---|---|']
        for text, dt, ev, steps, d in runs:
            lines.append('| {} | {:.2f} s | {} | {} | {:.3g} |'.format(text.replace('x', '×'), dt, ev, steps, d))
    out = PREAMBLE + '\n'.join(lines) + '\n'
    print(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if os.path.exists(a.out):                      # what stands below the marker is a hand-kept record: it stays
        old = open(a.out).read()
        if KEPT in old:
            out += '\n' + old[old.index(KEPT):]
    with open(a.out, 'w') as fh:
        fh.write(out)


if __name__ == '__main__':
    main()
