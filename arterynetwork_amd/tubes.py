"""The tube model: the branch graph with its centre points and radii rasterised back to a volume on the GPU.

Every stage from the head volume to the flow solve turns voxels into tables; ``vmask_tubes`` (include/vmask.h, DESIGN.md section 9,
"f21 tube model") is the way back.  Primitive e joins two consecutive entries of a branch: a segment swept by a ball whose radius
runs linearly between the entries' radii.  A voxel belongs to the primitive with the least power distance f = |x - c|^2 - rho^2
among those with f <= 0 (then the smaller e), so where two vessels overlap it goes to the one it lies deeper in.

    tubeVolume      the C-ABI call on plain tables: label, sizes, overlap with a mask, missed mask voxels, optionally f and e
    graphTubes      the same from a `BranchGraph`, its `BranchMorphometry` and optionally its `BranchSplines`
    paintBranches   a per-branch quantity (flow, pressure drop, compartment, curvature, radius) painted into the label volume
    modelVolumes, cylinderVolumes, agreement
                    the model's volume per branch, the reference's pi r^2 L beside it, and how well model and mask agree

numpy in gives numpy out, tensors on the GPU give tensors on the same device.  HIP only: there is no CPU path.  Not claimed:
anti-aliased (partial-volume) voxels, any treatment of junctions beyond the union of the tubes, smoothing of the radii."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import generateVesselVolume as _G

COUNT_NAMES = ('primitives', 'occupiedBricks', 'pairs', 'longestList')
STEP_NAMES = ('check_ms', 'count_ms', 'scan_ms', 'lists_ms', 'evaluate_ms', 'fill_ms')
MOST = 2.0 ** 20            # |P| and r are at most this many times the largest spacing
MODEL_FILE = 'vesselVolumeModel.nii.gz'
MODEL_LABEL_FILE = 'branchLabelsModel.nii.gz'
MODEL_TABLE_FILE = 'tubeModel.npz'
FLOW_VOLUME_FILE = 'branchFlow.nii.gz'


class TubeModel:
    """What `tubeVolume` returns: ``label`` (int32 volume: the label of the winning primitive's branch, 0 where no primitive holds
    the voxel), ``sizes`` and ``overlap`` (int64 per branch: the voxels won, and those of them inside the mask - zeros without a
    mask), ``missed`` (int: mask voxels with label 0), ``field`` (float64 volume: the winner's f, +inf where none) and ``nearest``
    (int64 volume: the winner's entry index, -1 where none) when asked for, else None, ``counts`` (a dict with `COUNT_NAMES`),
    ``spacing`` and ``hasMask``."""


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_tubes, 'argtypes', None):
        p, i64 = C.c_void_p, C.c_int64
        dll.vmask_tubes.argtypes = [C.c_int, i64, i64, i64, p, p, i64, p, p, p, p, p, p, p, p, p, p, p, p, p]
    return dll


def _spacing(spacing):
    h = np.ones(3, np.float64) if spacing is None else np.ascontiguousarray(np.asarray(spacing, np.float64).reshape(3))
    if not (np.isfinite(h).all() and (h > 0).all()) or h.max() / h.min() > 1000.0:
        raise ValueError('spacing must be finite and positive with max / min <= 1000')
    return h


def tubeVolume(shape, offsets, positions, radius, spacing=None, keep=None, labels=None, mask=None, device=0, info=None, return_field=False,
               return_nearest=False):
    """Rasterise a branch table (``vmask_tubes``) into a volume of `shape`; returns a `TubeModel`.  ``offsets`` (B + 1, from 0, every
    branch at least two entries), ``positions`` (E x 3, in the units of `spacing`: voxel i sits at i * spacing), ``radius`` (E, the
    same units), `keep` (B, a branch with 0 contributes nothing), `labels` (B, > 0; default b + 1), `mask` (a volume of `shape`;
    non-zero counts).  include/vmask.h states every operation; the GPU equals tests/tube_model.py to the bit.
    Host arrays give host arrays; when ``positions`` is a tensor on the GPU every table and the mask are taken to that device and
    the outputs are tensors there.  `info`, when a dict, receives the counts and the steps' times (`STEP_NAMES`, hipEvents).
    ``ValueError``, before the library is asked: a shape that is not three positive extents of fewer than 2^31 voxels, a spacing
    outside the rules, tables that do not fit each other, offsets that do not start at 0 or leave a branch fewer than two entries, a
    coordinate or radius that is not finite or above 2^20 times the largest spacing, a negative radius, a label <= 0, a mask of
    another shape."""
    shape = tuple(int(k) for k in shape)
    if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('shape must be three positive extents of fewer than 2^31 voxels')
    h = _spacing(spacing)
    on_device = _G._on_device(positions)
    if on_device:
        import torch
        tdev = positions.device
        dev = _G._dev_index(positions)
        take = lambda a, dt: (a if hasattr(a, 'data_ptr') else torch.as_tensor(np.asarray(a))).to(device=tdev, dtype=getattr(torch, np.dtype(dt).name)).contiguous()
        alloc = lambda shp, dt: torch.empty(shp, dtype=getattr(torch, np.dtype(dt).name), device=tdev)
        ptr = lambda a: a.data_ptr() if a is not None and a.numel() else None
        finite, every, some = torch.isfinite, lambda a: bool(a.all()), lambda a: bool(a.any())
    else:
        dev = device
        take = lambda a, dt: np.ascontiguousarray(a.cpu().numpy() if hasattr(a, 'data_ptr') else a, dtype=dt)
        alloc = lambda shp, dt: np.empty(shp, dt)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        finite, every, some = np.isfinite, lambda a: bool(np.all(a)), lambda a: bool(np.any(a))
    off, P, r = take(offsets, np.int64).reshape(-1), take(positions, np.float64), take(radius, np.float64).reshape(-1)
    if off.shape[0] < 1:
        raise ValueError('offsets needs at least one entry')
    B, E = int(off.shape[0]) - 1, int(r.shape[0])
    P = P.reshape(E, 3) if int(np.prod(tuple(P.shape))) == 3 * E else P
    if tuple(P.shape) != (E, 3):
        raise ValueError('positions must be E x 3 and radius E')
    if int(off[0]) != 0 or int(off[-1]) != E or (B and some(off[1:] - off[:-1] < 2)):
        raise ValueError('offsets must start at 0, end at the number of entries and give every branch at least two entries')
    if not (every(finite(P)) and every(finite(r))):
        raise ValueError('a coordinate or radius is not finite')
    if some(r < 0):
        raise ValueError('a radius is negative')
    if some(abs(P) > MOST * h.max()) or some(r > MOST * h.max()):
        raise ValueError('a coordinate or radius is above 2^20 times the largest spacing')
    kp = lb = mk = None
    if keep is not None:
        kp = take(take(keep, np.int64).reshape(-1) != 0, np.uint8)
        if int(kp.shape[0]) != B:
            raise ValueError('keep must have one entry per branch')
    if labels is not None:
        lb = take(labels, np.int64).reshape(-1)
        if int(lb.shape[0]) != B:
            raise ValueError('labels must have one entry per branch')
        if some(lb <= 0) or some(lb >= 2 ** 31):
            raise ValueError('labels must be positive int32 values')
        lb = take(lb, np.int32)
    if mask is not None:
        if tuple(mask.shape) != shape:
            raise ValueError('mask must have the shape of the volume')
        if on_device:
            mk = _G._u8t((mask if hasattr(mask, 'data_ptr') else torch.as_tensor(np.asarray(mask))).to(tdev))
        else:
            mk = _G._u8c(mask.cpu().numpy() if hasattr(mask, 'data_ptr') else mask)
    label = alloc(shape, np.int32)
    field = alloc(shape, np.float64) if return_field else None
    nearest = alloc(shape, np.int64) if return_nearest else None
    sizes, overlap = alloc((B,), np.int64), alloc((B,), np.int64)
    missed, counts, ms = np.zeros(1, np.int64), np.zeros(4, np.int64), np.zeros(6, np.float64)
    dll = _lib()
    if on_device:
        torch.cuda.synchronize(tdev)
    _G._check(dll.vmask_tubes(dev, *shape, h.ctypes.data, ptr(off) if B else None, B, ptr(P), ptr(r), ptr(kp), ptr(lb), ptr(mk), ptr(label), ptr(field),
                              ptr(nearest), ptr(sizes), ptr(overlap), missed.ctypes.data, counts.ctypes.data, ms.ctypes.data))
    model = TubeModel()
    model.label, model.field, model.nearest, model.sizes, model.overlap, model.missed = label, field, nearest, sizes, overlap, int(missed[0])
    model.counts = dict(zip(COUNT_NAMES, (int(c) for c in counts)))
    model.spacing, model.hasMask = h, mask is not None
    if info is not None:
        info.update(model.counts)
        info.update(zip(STEP_NAMES, (float(x) for x in ms)))
    return model


def graphTubes(graph, measured, splines=None, spacing=None, minRadius=None, radiusScale=1.0, keep=None, mask=None, labels=None, device=0, info=None,
               return_field=False, return_nearest=False):
    """The tube model of a `BranchGraph`: `tubeVolume` on the graph's branch table in the volume of ``graph.skeleton``.  The centre
    points are ``splines.position`` when a `BranchSplines` of this graph is given, else the voxel centres ``graph.coords * spacing``.
    The radii are ``measured.entryRadius * l * radiusScale`` with l = ``splineScale(spacing)[1]`` (the distance transform is in voxel
    units; the factor is exact for isotropic voxels), floored at `minRadius` (default l / 2), so a one-voxel-thin branch still
    draws.  `spacing` defaults to ``measured.spacing``.  The floor and the scale are the caller's: the radii are not smoothed."""
    from . import skeletonization as _S
    h = _spacing(measured.spacing if spacing is None else spacing)
    l = _S.splineScale(h)[1]
    floor = 0.5 * l if minRadius is None else float(minRadius)
    if not (np.isfinite(floor) and floor >= 0) or not (np.isfinite(radiusScale) and radiusScale > 0):
        raise ValueError('minRadius must be finite and not negative, radiusScale finite and positive')
    on_device = _G._on_device(graph.offsets)
    if on_device:
        import torch
        tdev = graph.offsets.device
        as_f64 = lambda a: (a if hasattr(a, 'data_ptr') else torch.as_tensor(np.asarray(a))).to(device=tdev, dtype=torch.float64)
        floor_at = lambda a: torch.clamp(a, min=floor)
    else:
        as_f64 = lambda a: np.asarray(a.cpu().numpy() if hasattr(a, 'data_ptr') else a, dtype=np.float64)
        floor_at = lambda a: np.maximum(a, floor)
    if splines is not None:
        positions = as_f64(splines.position).reshape(-1, 3)
    else:
        positions = as_f64(graph.coords).reshape(-1, 3) * as_f64(h)
    radius = floor_at(as_f64(measured.entryRadius).reshape(-1) * (l * float(radiusScale)))
    if int(positions.shape[0]) != int(radius.shape[0]) or int(radius.shape[0]) != int(graph.coords.reshape(-1, 3).shape[0]):
        raise ValueError('measured or splines do not belong to this graph')
    shape = tuple(int(k) for k in graph.skeleton.shape)
    model = tubeVolume(shape, graph.offsets, positions, radius, spacing=h, keep=keep, labels=labels, mask=mask, device=device, info=info,
                       return_field=return_field, return_nearest=return_nearest)
    model.minRadius, model.radiusScale, model.splinePositions = floor, float(radiusScale), splines is not None
    return model


def paintBranches(label, values, fill=0.0):
    """A per-branch quantity as a volume: ``values[label - 1]`` where ``label > 0``, `fill` elsewhere, in the dtype of `values`
    (labels are the default b + 1).  A tensor `label` gives a tensor on its device."""
    if hasattr(label, 'data_ptr'):
        import torch
        v = (values if hasattr(values, 'data_ptr') else torch.as_tensor(np.asarray(values))).to(label.device).reshape(-1)
        if int(label.max()) > int(v.shape[0]):
            raise ValueError('a label has no value')
        padded = torch.cat((torch.full((1,), fill, dtype=v.dtype, device=v.device), v))
        return padded[label.clamp(min=0).to(torch.int64)]
    label, v = np.asarray(label), np.asarray(values).reshape(-1)
    if label.size and int(label.max()) > len(v):
        raise ValueError('a label has no value')
    padded = np.concatenate((np.array([fill], dtype=v.dtype), v))
    return padded[np.maximum(label, 0)]


def modelVolumes(sizes, spacing):
    """Voxel counts as volumes in the units of the spacing cubed: ``sizes * ((h0 * h1) * h2)``, float64."""
    h = _spacing(spacing)
    sizes = sizes.cpu().numpy() if hasattr(sizes, 'data_ptr') else sizes
    return np.asarray(sizes, dtype=np.float64) * ((h[0] * h[1]) * h[2])


def cylinderVolumes(pathLength, meanRadius):
    """The reference's volume of a branch (getVolumePerPartition, fluidSimulation.py:814-842): ``pi * meanRadius^2 * pathLength``,
    for comparison with `modelVolumes` - it counts the overlap at a junction once per branch and knows no taper."""
    L, r = (np.asarray(a.cpu().numpy() if hasattr(a, 'data_ptr') else a, dtype=np.float64) for a in (pathLength, meanRadius))
    return np.pi * r * r * L


def agreement(model):
    """How well the model and the mask it was compared with agree: a dict with ``precision`` (per branch ``overlap / sizes``, NaN
    for a branch without voxels), ``recall`` (mask voxels that the model holds / mask voxels), ``dice`` (2 |model and mask| /
    (|model| + |mask|)), ``modelVoxels``, ``maskVoxels`` and ``missed``.  The EDT radius at a centre voxel overestimates a digitised
    cylinder (radius 4 gives sqrt(17)), so a Dice below 1 is expected; no threshold is claimed."""
    if not model.hasMask:
        raise ValueError('the model was made without a mask')
    sizes, overlap = (np.asarray(a.cpu().numpy() if hasattr(a, 'data_ptr') else a, dtype=np.int64) for a in (model.sizes, model.overlap))
    both, drawn = int(overlap.sum()), int(sizes.sum())
    there = both + int(model.missed)
    with np.errstate(divide='ignore', invalid='ignore'):
        precision = overlap / sizes.astype(np.float64)
    return {'precision': precision, 'recall': both / there if there else float('nan'), 'dice': 2.0 * both / (drawn + there) if drawn + there else float('nan'),
            'modelVoxels': drawn, 'maskVoxels': there, 'missed': int(model.missed)}


def writeTubes(model, baseFolder, affine, measured=None, flow=None):
    """The files of ``skeletonization.main(..., tubes=...)`` for a host `TubeModel`: `MODEL_FILE` (uint8: label != 0),
    `MODEL_LABEL_FILE` (int32), `MODEL_TABLE_FILE` (sizes, overlap, missed, volumes, cylinderVolumes when `measured` is given,
    counts, the parameters, and `agreement` when the model has a mask) and, with `flow` (per branch), `FLOW_VOLUME_FILE`
    (float32: |flow| painted).  Returns the names written."""
    import os
    names = [MODEL_FILE, MODEL_LABEL_FILE, MODEL_TABLE_FILE]
    _G.saveVolume((model.label != 0).astype(np.uint8), affine, os.path.join(baseFolder, MODEL_FILE), astype=np.uint8)
    _G.saveVolume(model.label, affine, os.path.join(baseFolder, MODEL_LABEL_FILE), astype=np.int32)
    table = {'sizes': model.sizes, 'overlap': model.overlap, 'missed': np.int64(model.missed), 'volumes': modelVolumes(model.sizes, model.spacing),
             'counts': np.array([model.counts[k] for k in COUNT_NAMES], np.int64), 'countNames': np.array(COUNT_NAMES), 'spacing': model.spacing,
             'minRadius': np.float64(getattr(model, 'minRadius', np.nan)), 'radiusScale': np.float64(getattr(model, 'radiusScale', np.nan)),
             'splinePositions': np.bool_(getattr(model, 'splinePositions', False))}
    if measured is not None:
        table['cylinderVolumes'] = cylinderVolumes(measured.pathLength, measured.meanRadius)
    if model.hasMask:
        a = agreement(model)
        table.update(precision=a['precision'], recall=np.float64(a['recall']), dice=np.float64(a['dice']))
    np.savez_compressed(os.path.join(baseFolder, MODEL_TABLE_FILE), **table)
    if flow is not None:
        painted = paintBranches(model.label, np.abs(np.asarray(flow, dtype=np.float64)).astype(np.float32), fill=0.0)
        _G.saveVolume(painted, affine, os.path.join(baseFolder, FLOW_VOLUME_FILE), astype=np.float32)
        names.append(FLOW_VOLUME_FILE)
    return names
