"""Geodesic distance inside the vessel mask (``vmask_geodesic``, DESIGN.md section 9 "f9 geodesic").

The path length from chosen seed voxels through the vessels - the "depth" of the reference's ``partitionCompartmentGUI.py`` and
the "path length" of ``fluidSimulation.py``'s terminating-pressure relation, which the reference computes on the centre-line
graph only - for every voxel of the mask: shortest paths in the 26-adjacency graph of the mask's voxels, an edge weighing the
Euclidean length of its step in the given spacing.  A block-based label-correcting iteration in HIP; no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import generateVesselVolume as _G

COUNT_KEYS = ('mask_voxels', 'reached', 'bricks', 'distance_rounds', 'label_rounds')


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_geodesic, 'argtypes', None):
        p, i64 = C.c_void_p, C.c_int64
        dll.vmask_geodesic.argtypes = [C.c_int, p, i64, i64, i64, p, p, i64, p, p, p, p, i64, p]
    return dll


def _spacing(spacing):
    if spacing is None:
        return None
    sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64))
    if sp.shape != (3,):
        raise ValueError('spacing: three numbers, one per axis')
    return sp


def _linear_seeds(seeds, shape, on_device, ref=None):
    """Seeds as a contiguous int64 vector of C-order linear indices: an N x 3 coordinate array or the indices themselves."""
    if on_device:
        import torch
        s = seeds if _G._on_device(seeds) else torch.as_tensor(np.asarray(seeds), device=ref.device)
        if s.numel() == 0 and s.dim() <= 2:
            return torch.zeros(0, dtype=torch.int64, device=ref.device)
        if s.dtype.is_floating_point or s.dtype == torch.bool:
            raise ValueError('seeds must be integers')
        s = s.to(torch.int64)
        if s.dim() == 2 and s.shape[1] == 3:
            lim = torch.as_tensor(shape, dtype=torch.int64, device=s.device)
            if s.numel() and bool(((s < 0) | (s >= lim)).any()):
                raise ValueError('seed coordinates outside the volume')
            s = (s[:, 0] * shape[1] + s[:, 1]) * shape[2] + s[:, 2]
        elif s.dim() != 1:
            raise ValueError('seeds: an N x 3 coordinate array or N linear indices')
        return s.contiguous()
    s = np.asarray(seeds)
    if s.size == 0 and s.ndim <= 2:
        return np.zeros(0, np.int64)
    if s.dtype.kind not in 'iu':
        raise ValueError('seeds must be integers')
    s = s.astype(np.int64)
    if s.ndim == 2 and s.shape[1] == 3:
        if ((s < 0) | (s >= np.asarray(shape, np.int64))).any():
            raise ValueError('seed coordinates outside the volume')
        s = (s[:, 0] * shape[1] + s[:, 1]) * shape[2] + s[:, 2]
    elif s.ndim != 1:
        raise ValueError('seeds: an N x 3 coordinate array or N linear indices')
    return np.ascontiguousarray(s)


def _run(m, seeds, labels, max_label, spacing, device, want_dist, want_labels, info):
    """One call of vmask_geodesic.  `m`: the uint8 mask (numpy, or a tensor on the GPU), `seeds` / `labels`: linear indices and
    int32 labels of the same kind as `m` (labels may be None).  Returns (dist or None, labels or None, sizes or None)."""
    dll = _lib()
    counts = np.full(5, -1, np.int64)
    sp = _spacing(spacing)
    nseed = int(seeds.shape[0])
    if _G._on_device(m):
        import torch
        dev = _G._dev_index(m)
        new = lambda shape, dt: torch.empty(shape, dtype=getattr(torch, dt), device=m.device)
        ptr = lambda a: a.data_ptr()
        torch.cuda.synchronize(m.device)
    else:
        dev = device
        new = lambda shape, dt: np.empty(shape, getattr(np, dt))
        ptr = lambda a: a.ctypes.data
    shape = tuple(int(n) for n in m.shape)
    dist = new(shape, 'float64') if want_dist else None
    lab = new(shape, 'int32') if want_labels else None
    sizes = new(max_label + 1, 'int64') if want_labels else None
    opt = lambda a: ptr(a) if a is not None else None
    _G._check(dll.vmask_geodesic(dev, ptr(m), *shape, ptr(seeds) if nseed else None, opt(labels) if nseed else None, nseed,
                                 sp.ctypes.data if sp is not None else None, opt(dist), opt(lab), opt(sizes), max_label,
                                 counts.ctypes.data))
    if info is not None:
        info.update(zip(COUNT_KEYS, (int(c) for c in counts)))
    return dist, lab, sizes


def geodesicDistance(mask, seeds, labels=None, spacing=None, device=0, info=None, return_labels=False):
    """Shortest-path distance (float64, the mask's shape) from the `seeds` to every voxel of ``mask != 0`` through the mask:
    steps between 26-neighbours that are both in the mask, a step (d0, d1, d2) weighing sqrt((d0 h0)^2 + (d1 h1)^2 + (d2 h2)^2)
    for ``spacing = (h0, h1, h2)`` (default 1 1 1), the sums rounded as IEEE double additions along the path (what Dijkstra's
    algorithm computes).  0 at the seeds, ``+inf`` at mask voxels that no seed reaches, -1 outside the mask.

    `seeds`: an N x 3 integer coordinate array or N C-order linear indices, every one a voxel of the mask; N = 0 is legal.
    `labels`: N integers >= 1 (default: all 1); of several labels given for one voxel the smallest holds.
    ``return_labels=True`` returns ``(distance, labels, sizes)``: ``labels`` (int32) is the label of the seed that the voxel's
    shortest paths come from - where paths of equal length arrive from seeds of different labels, THE SMALLEST LABEL wins (not the
    smallest voxel index) -, 0 outside the mask and where the distance is ``+inf``; ``sizes[l]`` (int64, max(labels) + 1) counts
    the mask voxels with label l, ``sizes[0]`` the unreached ones.
    numpy in gives numpy out; a mask tensor that lives on the GPU gives tensors on the same device.  `info`, when a dict,
    receives ``mask_voxels``, ``reached``, ``bricks`` (occupied 8x8x8 bricks), ``distance_rounds`` and ``label_rounds``."""
    on_device = _G._on_device(mask)
    m = _G._u8t(mask) if on_device else _G._u8c(mask)
    shape = tuple(int(n) for n in m.shape)
    s = _linear_seeds(seeds, shape, on_device, ref=m)
    nseed = int(s.shape[0])
    lab = None
    max_label = 1
    if labels is not None:
        if on_device:
            import torch
            lab = (labels if _G._on_device(labels) else torch.as_tensor(np.asarray(labels), device=m.device)).reshape(-1)
            if lab.dtype.is_floating_point:
                raise ValueError('labels must be integers')
            lab = lab.to(torch.int32).contiguous()
        else:
            lab = np.asarray(labels).reshape(-1)
            if lab.size and lab.dtype.kind not in 'iu':
                raise ValueError('labels must be integers')
            lab = np.ascontiguousarray(lab, dtype=np.int32)
        if int(lab.shape[0]) != nseed:
            raise ValueError('labels: one per seed')
        if nseed:
            max_label = max(1, int(lab.max()))
    _spacing(spacing)
    dist, out_labels, sizes = _run(m, s, lab, max_label, spacing, device, True, return_labels, info)
    return (dist, out_labels, sizes) if return_labels else dist
