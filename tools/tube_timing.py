"""Time vmask_tubes on the branch graphs of the bench masks and measure how well the model agrees with the mask (profiles/tube_timing.md).

    python tools/tube_timing.py [--shape 880x880x640 ...] [--only K ...] [--no-agreement] [--out FILE] [--md FILE]

Per mask (--only: its index among the three bench masks): skeleton, `branchGraph`, `branchMorphometry` (not timed), then `graphTubes` with
device-resident tables and outputs: two warm calls, then per step - check, count, scan, list fill, evaluate, empty-brick fill, by the
hipEvents inside the call - the median of five, once with the label alone and once with field and nearest stored as well.  In the
same process, as the yardstick: vmask_territories on the same mask and skeleton and one streaming read of the volume.
The agreement part runs the real chain (skeleton -> branchGraph -> morphometry -> splines -> graphTubes) on the tube phantom and on
tubes about an arc and a helix, with voxel-centre and with spline positions, and records Dice, recall and the per-branch precision."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from arterynetwork_amd import generateVesselVolume as G, phantoms, skeletonization as S, tubes as T
from segments_timing import masks, timed

WARM, REPS = 2, 5
# f64 operations of one (voxel, primitive) evaluation as vmask.h writes it, the division counted as one: 6 subtractions, 11
# multiplications, 9 additions, 1 division, 2 selects
OPS = 29


def steps(run):
    for _ in range(WARM):
        run({})
    rows = []
    for _ in range(REPS):
        info = {}
        run(info)
        rows.append([info[k] for k in T.STEP_NAMES])
    return dict(zip(T.STEP_NAMES, np.median(np.array(rows), axis=0).tolist())), info


def time_mask(text, name, m, dev, dll):
    shape = tuple(m.shape)
    sk = S.skeletonize(m)
    graph = S.branchGraph(sk, vesselVolumeMask=m)
    measured = S.branchMorphometry(graph, vesselVolumeMask=m)
    row = {'volume': text, 'mask': name, 'voxels_in': int(m.sum()), 'branches': int(graph.offsets.numel()) - 1, 'entries': int(graph.coords.shape[0])}
    step = (graph.coords[1:] - graph.coords[:-1]).abs().max(dim=1).values if row['entries'] > 1 else torch.zeros(0, dtype=torch.int64, device=dev)
    step[(graph.offsets[1:-1] - 1).long()] = 0                            # (the pairs that straddle two branches are no primitives)
    row['jump_primitives'], row['longest_step'] = int((step > 1).sum()), int(step.max()) if step.numel() else 0
    holder = {}

    def run(info, **kw):
        holder['model'] = T.graphTubes(graph, measured, mask=m, info=info, **kw)
    row['label_only'], info = steps(run)
    row['all_outputs'], _ = steps(lambda info: run(info, return_field=True, return_nearest=True))
    model = holder['model']
    row.update({k: info[k] for k in T.COUNT_NAMES})
    a = T.agreement(model)
    row.update(dice=a['dice'], recall=a['recall'], model_voxels=a['modelVoxels'], precision_min=float(np.nanmin(a['precision'])), precision_median=float(np.nanmedian(a['precision'])))
    evaluations = 512.0 * info['pairs']
    row['evaluations'] = evaluations
    row['evaluations_per_s'] = evaluations / (row['label_only']['evaluate_ms'] * 1e-3)
    row['f64_ops_per_s'] = OPS * row['evaluations_per_s']
    del model, holder
    # the yardsticks, in the same process
    off = graph.offsets.contiguous()
    co = graph.coords
    vox = ((co[:, 0] * shape[1] + co[:, 1]) * shape[2] + co[:, 2]).contiguous()
    nseg = int(off.numel()) - 1
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    nearest = torch.empty(shape, dtype=torch.int64, device=dev)
    sizes = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
    skel = graph.skeleton.contiguous()
    row['territories_ms'] = timed(lambda: G._check(dll.vmask_territories(0, m.data_ptr(), skel.data_ptr(), *shape, off.data_ptr(), nseg, vox.data_ptr() if len(vox) else None,
                                                                     labels.data_ptr(), nearest.data_ptr(), sizes.data_ptr())), WARM, REPS)
    flat = m.view(-1)
    row['read_ms'] = timed(lambda: flat.view(torch.int64).sum(), WARM, REPS)
    return row


def chain(name, m, spacing=(1.0, 1.0, 1.0)):
    graph = S.branchGraph(S.skeletonize(m), minSpurLength=3, radiusFactor=1.0, vesselVolumeMask=m)
    measured = S.branchMorphometry(graph, vesselVolumeMask=m, spacing=spacing)
    splines = S.branchSplines(graph, spacing=spacing)
    rows = []
    for positions, kw in (('voxel centres', {}), ('splines', dict(splines=splines))):
        a = T.agreement(T.graphTubes(graph, measured, mask=m, **kw))
        rows.append({'phantom': name, 'positions': positions, 'branches': len(graph.offsets) - 1, 'mean_entry_radius': float(np.mean(measured.entryRadius)),
                     'mask_voxels': a['maskVoxels'], 'model_voxels': a['modelVoxels'],
                     'dice': a['dice'], 'recall': a['recall'], 'precision': [round(float(p), 4) for p in a['precision']]})
    return rows


def curve_mask(points, radius, shape):
    """The voxels within `radius` of a finely sampled curve: the tube model of the curve itself."""
    return (T.tubeVolume(shape, [0, len(points)], points, np.full(len(points), radius)).label != 0).astype(np.uint8)


def agreement_rows():
    I, _ = phantoms.tube_phantom(noise=0.0)
    rows = chain('tube phantom 128x128x64, radius 3.5', (I > 0.5).astype(np.uint8))
    arc, helix = phantoms.arc_curve(12.0, per_voxel=4), phantoms.helix_curve(10.0, per_voxel=4)
    for name, pts in (('arc of radius 12, tube radius 3', arc), ('helix of radius 10, tube radius 3', helix)):
        pts = pts + 4.0
        shape = tuple(int(k) for k in np.ceil(pts.max(axis=0)) + 6)
        rows += chain(name, curve_mask(pts, 3.0, shape))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', action='append', default=[])
    ap.add_argument('--only', action='append', type=int, default=[])
    ap.add_argument('--no-agreement', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    dll = S._skeleton_lib()
    rows = []
    for text in a.shape or ['880x880x640']:
        shape = tuple(int(x) for x in text.split('x'))
        for k, (name, m) in enumerate(masks(shape, dev)):
            if a.only and k not in a.only:
                continue
            rows.append(time_mask(text, name, m, dev, dll))
            print(json.dumps(rows[-1]), flush=True)
            del m
            torch.cuda.empty_cache()
    agree = [] if a.no_agreement else agreement_rows()
    for r in agree:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'timing': rows, 'agreement': agree}, f, indent=1)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# vmask_tubes: timing and model-mask agreement on one MI355X\n\n')
            f.write('`python tools/tube_timing.py`: the branch graph of the bench mask (skeleton, `branchGraph`, `branchMorphometry`; voxel-centre positions, radii from '
                    'the distance transform, floor 0.5), device-resident tables and outputs; {} warm calls, then per step the median of {} by the hipEvents inside '
                    'the call. `vmask_territories` on the same mask and skeleton and one streaming read of the mask (`int64` view, `sum`) run in the same process: '
                    'they are the yardstick. There is no parent to compare with and no target.\n\n'.format(WARM, REPS))
            f.write('| volume | mask | branches | primitives | occupied bricks | pairs | longest list | outputs | check ms | count ms | scan ms | lists ms | evaluate ms | fill ms | '
                    'territories ms | read ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                for which in ('label_only', 'all_outputs'):
                    s = r[which]
                    f.write('| {} | {} | {} | {} | {} | {} | {} | {} | {} | {:.3f} | {:.3f} |\n'.format(
                        r['volume'], r['mask'], r['branches'], r['primitives'], r['occupiedBricks'], r['pairs'], r['longestList'], which.replace('_', ' '),
                        ' | '.join('{:.3f}'.format(s[k]) for k in T.STEP_NAMES), r['territories_ms'][0], r['read_ms'][0]))
            f.write('\nThe evaluate step, label alone: ')
            f.write('; '.join('{} / {}: {:.3g} (voxel, primitive) evaluations in {:.3f} ms = {:.3g} per second, {:.3g} f64 operations per second at {} per evaluation '
                              '(the division counted as one)'.format(r['volume'], r['mask'], r['evaluations'], r['label_only']['evaluate_ms'], r['evaluations_per_s'],
                                                                   r['f64_ops_per_s'], OPS) for r in rows) + '.\n')
            f.write('\nModel against mask on the same graphs (unpruned; a jump primitive joins a cluster\'s representative to a voxel that is no 26-neighbour): ' +
                    '; '.join('{} / {}: Dice {:.4f}, recall {:.4f}, precision min {:.4f} median {:.4f}, {} jump primitives, the longest step {} voxels'.format(
                        r['volume'], r['mask'], r['dice'], r['recall'], r['precision_min'], r['precision_median'], r['jump_primitives'], r['longest_step']) for r in rows) + '.\n')
            if agree:
                f.write('\n## Agreement through the real chain\n\nskeleton -> `branchGraph(minSpurLength=3, radiusFactor=1)` -> `branchMorphometry` -> `branchSplines` -> '
                        '`graphTubes` (defaults), spacing 1. No threshold is asserted anywhere: the radius is the distance transform at the skeleton voxel, above the true radius where that voxel is on the axis '
                        '(radius 4 gives sqrt(17)) and below it by the voxel\'s distance from the axis where it is not.\n\n')
                f.write('| phantom | positions | branches | mean entry radius | mask voxels | model voxels | Dice | recall | precision per branch |\n|---|---|---|---|---|---|---|---|---|\n')
                for r in agree:
                    f.write('| {} | {} | {} | {:.3f} | {} | {} | {:.4f} | {:.4f} | {} |\n'.format(r['phantom'], r['positions'], r['branches'], r['mean_entry_radius'], r['mask_voxels'], r['model_voxels'],
                                                                                    r['dice'], r['recall'], r['precision']))


if __name__ == '__main__':
    main()
