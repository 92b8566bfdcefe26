"""Times the skull stripping (arterynetwork_amd/brain.py, DESIGN.md section 9 entry f17) on an analytic head phantom that is
built on the device: nested ellipsoids - brain 90 / 110, a dark gap, scalp, air - plus a one-voxel bridge, float32.

    python tools/time_brain.py [--sizes 512x512x170 880x880x640] [--repeats 5] [--out profiles/brain_extraction.json]

Per size: one warm-up, then the median over `--repeats` runs of the histogram (HIP events around ``intensityFloor``) and of the
stages of ``vmask_brain_extract`` (the HIP events inside the call, info[8..14]); the least bytes that each stage has to move;
the peak of the call's device allocations."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the HIP library: one ROCm runtime per process)

from arterynetwork_amd import brain as BR  # noqa: E402


def phantom(shape, device):
    """(volume float32, true brain) on the device."""
    grids = [((torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2.0) / (0.38 * n)) ** 2 for n in shape]
    q = grids[0][:, None, None] + grids[1][None, :, None] + grids[2][None, None, :]
    I = torch.zeros(shape, dtype=torch.float32, device=device)
    I[q <= 1.32] = 85.0
    I[q <= 1.12] = 15.0
    I[q <= 1.0] = 90.0
    I[q <= 0.5] = 110.0
    c = [n // 2 for n in shape]
    line = q[c[0], c[1], c[2]:]
    I[c[0], c[1], c[2]:] = torch.where(line <= 1.32, torch.full_like(line, 90.0), torch.zeros_like(line))
    return I, q <= 1.0


def least_bytes(shape, radius, erosion, closing):
    """What each timed stage has to read and write at least, in bytes (float32 in, float64 between the edge passes, 4-byte parents
    and roots in the labellings, 1 bit per voxel in the packed volumes)."""
    V = shape[0] * shape[1] * shape[2]
    words = shape[0] * shape[1] * ((shape[2] + 63) // 64) * 8
    step = 2 * words                                       # a cross step: the packed volume read once and written once
    label = V // 8 + V + 5 * V + 16 * V + 8 * V            # unpack; init; union (own parent and 3 forward neighbours); flatten
    return {'edges': (4 + 16) * V + (16 + 24) * V + (24 + 4) * V + words, 'erosion': erosion * step,
            'mainComponent': label + 4 * V + 4 * V + words, 'dilationClosing': (erosion + 2 * closing) * step,
            'fillHoles': label + 4 * V + 2 * words, 'unpack': words + V, 'sizePass': 4 * V}


def measure(shape, repeats, device):
    I, brain = phantom(shape, device)
    torch.cuda.synchronize()
    runs, hist_ms, total_ms = [], [], []
    info = {}
    for i in range(repeats + 1):                           # (the first run warms up)
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        BR.intensityFloor(I)
        b.record()
        info = {}
        mask = BR.brainExtraction(I, info=info)
        c.record()
        torch.cuda.synchronize()
        if i:
            runs.append(info['microseconds'])
            hist_ms.append(a.elapsed_time(b))
            total_ms.append(b.elapsed_time(c))
    inter = int((mask.bool() & brain).sum())
    dice = 2.0 * inter / (int(mask.sum()) + int(brain.sum()))
    ms = {k: statistics.median(r[k] for r in runs) / 1000.0 for k in BR.TIMED}
    least = least_bytes(shape, 4, 1, 1)
    return {'shape': list(shape), 'voxels': shape[0] * shape[1] * shape[2], 'input': 'float32', 'repeats': repeats,
            'histogram_ms': statistics.median(hist_ms), 'extraction_ms_with_histogram': statistics.median(total_ms),
            'stage_ms': ms, 'least_bytes': least, 'least_GB_per_s': {k: (least[k] / 1e9) / (ms[k] / 1e3) if ms[k] > 0 else None for k in BR.TIMED},
            'peak_device_bytes': info['peakBytes'], 'counts': info['counts'], 'components_after_erosion': info['components'], 'dice': dice}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', nargs='+', default=['512x512x170', '880x880x640'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'brain_extraction.json'))
    a = ap.parse_args()
    device = torch.device('cuda', 0)
    result = {'device': torch.cuda.get_device_name(0), 'parameters': dict(sigma=1.0, edge=0.05, erosion=1, closing=1, diffusion=None), 'sizes': []}
    for s in a.sizes:
        shape = tuple(int(x) for x in s.split('x'))
        r = measure(shape, a.repeats, device)
        result['sizes'].append(r)
        print(json.dumps(r), flush=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print('written to {}'.format(a.out))


if __name__ == '__main__':
    main()
