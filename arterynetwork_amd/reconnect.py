"""Reconnect vessel fragments (``vmask_bridge``, DESIGN.md section 9 "f19 bridges").

The reference mends a vessel that the mask lost across a dip of the vesselness by hand: the *Reconnect* operation of
``manualCorrectionGUI.py`` (Usage, step 5) joins two branches along a spline that the user anchors by four clicks.  This module
is the headless, deterministic stand-in: between every two components of the vessel mask the cheapest path through a cost
volume derived from the vesselness, accepted when it is cheap enough; a ridge of faint vesselness across a gap is cheap to
follow, a jump sideways to a parallel vessel is not.  The flood, the contacts and the paths run in HIP; which bridges to take
(`selectBridges`) is decided on the host.  No CPU path.

Not claimed: the reference's spline geometry, its *Grow* and *Cut*, sub-voxel paths, bridges inside one component.  (A smooth
sub-voxel curve through every branch of the graph - not through a bridge's path - is `skeletonization.branchSplines`, a smoothing
spline of our own definition; the bridges themselves stay voxel paths.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G

COUNT_KEYS = ('components', 'domain_voxels', 'reached', 'contacts', 'pairs', 'bridges', 'path_entries', 'bricks', 'flood_rounds', 'root_rounds')
BRIDGE_FILE = 'bridges.npz'
DEFAULT_MAX_COST = 16.0
_E_ARG = -1


def _lib():
    dll = _G._lib()
    if not getattr(dll.vmask_bridge, 'argtypes', None):
        p, i64 = C.c_void_p, C.c_int64
        dll.vmask_bridge.argtypes = [C.c_int, p, p, p, C.c_int, p, i64, i64, i64, p, C.c_double, C.c_int, p, p, p, i64, p, p, i64, p, p, p, p]
    return dll


def _spacing(spacing):
    if spacing is None:
        return None
    sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64))
    if sp.shape != (3,):
        raise ValueError('spacing: three numbers, one per axis')
    return sp


def _host(a):
    return a.cpu().numpy() if _G._on_device(a) else np.asarray(a)


class Bridges:
    """What `bridgeCandidates` returns, the bridges ascending by ``(a, b)``: ``pairs`` (int64 B x 2: the two components, a < b,
    numbered as `labelVolume` numbers them), ``ends`` (int64 B x 2: the linear indices of the two voxels u, v where the halves
    of the path meet), ``roots`` (int64 B x 2: the mask voxels the path starts and ends at), ``cost`` (float64 B), ``offsets``
    (int64 B + 1) and ``voxels`` (int64 C-order linear indices): path i is ``voxels[offsets[i]:offsets[i + 1]]``, from the mask
    voxel of a to the mask voxel of b, both included; ``ncomp``, ``shape``; and - with ``return_fields=True``, else ``None`` -
    the dense ``dist``, ``root``, ``pred`` and ``comp`` of include/vmask.h."""

    def __init__(self, pairs, ends, roots, cost, offsets, voxels, ncomp, shape, dist=None, root=None, pred=None, comp=None):
        self.pairs, self.ends, self.roots, self.cost, self.offsets, self.voxels = pairs, ends, roots, cost, offsets, voxels
        self.ncomp, self.shape = ncomp, shape
        self.dist, self.root, self.pred, self.comp = dist, root, pred, comp

    def __len__(self):
        return int(self.cost.shape[0])

    def path(self, i):
        """Path i as an int64 L x 3 coordinate array."""
        v = self.voxels[self.offsets[i]:self.offsets[i + 1]]
        return np.stack(np.unravel_index(v, self.shape), axis=1).astype(np.int64).reshape(len(v), 3)


def vesselCost(vesselness, floor=0.05, brainVolumeMask=None):
    """The cost volume of a vesselness volume: float64 ``1 / (floor + v / max v)`` - between 1 / (1 + floor) on the strongest
    ridge and 1 / floor where there is no vesselness at all -, the maximum taken inside `brainVolumeMask` when one is given
    (voxels outside it get the cost of v = 0).  Computed once: the same array goes to the device and to a model."""
    floor = float(floor)
    if not np.isfinite(floor) or not floor > 0.0:
        raise ValueError('floor: finite and positive')
    on_device = _G._on_device(vesselness)
    if on_device:
        import torch
        v = vesselness.to(torch.float64)
        if brainVolumeMask is not None:
            b = brainVolumeMask if _G._on_device(brainVolumeMask) else torch.as_tensor(np.asarray(brainVolumeMask), device=v.device)
            if tuple(b.shape) != tuple(v.shape):
                raise ValueError('brainVolumeMask and vesselness must have the same shape')
            v = torch.where(b != 0, v, torch.zeros_like(v))
        if v.dim() != 3:
            raise ValueError('expected a 3-D volume')
        if not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
            raise ValueError('vesselness: finite and not negative')
        top = float(v.max()) if v.numel() else 0.0
        return (1.0 / (floor + (v / top if top > 0.0 else torch.zeros_like(v)))).contiguous()
    v = np.asarray(vesselness, dtype=np.float64)
    if v.ndim != 3:
        raise ValueError('expected a 3-D volume')
    if brainVolumeMask is not None:
        b = np.asarray(brainVolumeMask)
        if b.shape != v.shape:
            raise ValueError('brainVolumeMask and vesselness must have the same shape')
        v = np.where(b != 0, v, 0.0)
    if not np.isfinite(v).all() or (v < 0).any():
        raise ValueError('vesselness: finite and not negative')
    top = float(v.max()) if v.size else 0.0
    return np.ascontiguousarray(1.0 / (floor + (v / top if top > 0.0 else np.zeros_like(v))))


def _isolated(points, shape):
    """Those of the voxels `points` (N x 3) that have none of the others among their 26 neighbours."""
    if len(points) == 0:
        return points
    lin = np.ravel_multi_index(tuple(points.T), shape)
    alone = np.ones(len(points), bool)
    for d0 in (-1, 0, 1):
        for d1 in (-1, 0, 1):
            for d2 in (-1, 0, 1):
                if d0 == d1 == d2 == 0:
                    continue
                q = points + np.array([d0, d1, d2])
                ok = ((q >= 0) & (q < np.asarray(shape))).all(axis=1)
                hit = np.zeros(len(points), bool)
                hit[ok] = np.isin(np.ravel_multi_index(tuple(q[ok].T), shape), lin)
                alone &= ~hit
    return points[alone]


def tipRegions(vesselVolumeMask, reach=3.0, spacing=None, skeleton=None, device=0):
    """The vessel ends: a uint8 0/1 volume of the mask voxels within geodesic distance `reach` (through the mask, in `spacing`)
    of an end point of the curve skeleton - the end-point nodes of `skeletonization.branchGraph`, and the skeleton voxels
    without any neighbour (a fragment that thins to one voxel is all end).  `skeleton` defaults to
    ``skeletonization.skeletonize(vesselVolumeMask)``.  A mask tensor on the GPU gives a tensor on the same device."""
    from . import geodesic as _geo, skeletonization as _S
    reach = float(reach)
    if not np.isfinite(reach) or reach < 0.0:
        raise ValueError('reach: finite and not negative')
    _spacing(spacing)                                # (only checked here: geodesicDistance takes it as given)
    if skeleton is None:
        skeleton = _S.skeletonize(vesselVolumeMask, device=device)
    graph = _S.branchGraph(skeleton, device=device)
    shape = tuple(int(n) for n in vesselVolumeMask.shape)
    ends = _host(graph.nodeCoords)[_host(graph.nodeKind) == 0].reshape(-1, 3)
    if graph.counts['isolated']:
        ends = np.concatenate((ends, _isolated(np.argwhere(_host(skeleton) != 0).astype(np.int64), shape)))
    dist = _geo.geodesicDistance(vesselVolumeMask, ends.astype(np.int64), spacing=spacing, device=device)
    if _G._on_device(dist):
        import torch
        return ((dist >= 0) & (dist <= reach)).to(torch.uint8)
    return ((dist >= 0) & (dist <= reach)).astype(np.uint8)


def bridgeCandidates(mask, cost, domain=None, tips=None, maxCost=DEFAULT_MAX_COST, tipRule=1, spacing=None, device=0, info=None, return_fields=False):
    """The cheapest bridge between every two 26-connected components of ``mask != 0`` that a path of cost at most `maxCost`
    joins, as a `Bridges` record (include/vmask.h, ``vmask_bridge``, has the definition).  A path runs through voxels of
    ``domain != 0`` outside the mask (default: the whole volume); a step between the 26-neighbours u, v costs
    ``(cost[u] + cost[v]) / 2`` times its Euclidean length in `spacing`.  `cost`: float32 or float64, finite and positive inside
    the domain (`vesselCost` makes one).  `tips` (default: every voxel) marks the vessel ends; a bridge needs at least `tipRule`
    (0, 1, 2) of the two mask voxels it starts and ends at among them.
    numpy in gives numpy out; where the mask is a tensor on the GPU the other volumes are used on that device and the dense
    fields come back as tensors (the bridge tables are always numpy).  `info`, when a dict, receives the names of `COUNT_KEYS`.
    The tables are sized for 4096 bridges and 262144 path entries; a result larger than that learns its sizes from the first
    call and RUNS THE WHOLE DEVICE COMPUTATION A SECOND TIME (``vmask_bridge`` keeps no state between calls)."""
    on_device = _G._on_device(mask)
    m = _G._u8t(mask) if on_device else _G._u8c(mask)
    shape = tuple(int(n) for n in m.shape)
    maxCost = float(maxCost)
    if not np.isfinite(maxCost) or not maxCost > 0.0:
        raise ValueError('maxCost: finite and positive')
    if tipRule not in (0, 1, 2):
        raise ValueError('tipRule: 0, 1 or 2')
    sp = _spacing(spacing)
    if on_device:
        import torch
        dev = _G._dev_index(m)
        there = lambda a: a if _G._on_device(a) else torch.as_tensor(np.asarray(a), device=m.device)
        c = there(cost)
        c = (c if c.dtype in (torch.float32, torch.float64) else c.to(torch.float64)).contiguous()
        code = 5 if c.dtype == torch.float32 else 6
        u8 = lambda a: _G._u8t(there(a))
        new = lambda dt: torch.empty(shape, dtype=getattr(torch, dt), device=m.device)
        ptr = lambda a: a.data_ptr()
    else:
        dev = device
        c = np.ascontiguousarray(_host(cost))
        if c.dtype not in (np.float32, np.float64):
            c = c.astype(np.float64)
        code = 5 if c.dtype == np.float32 else 6
        u8 = lambda a: _G._u8c(_host(a))
        new = lambda dt: np.empty(shape, getattr(np, dt))
        ptr = lambda a: a.ctypes.data
    if tuple(c.shape) != shape:
        raise ValueError('cost and mask must have the same shape')
    dom = u8(domain) if domain is not None else None
    tip = u8(tips) if tips is not None else None
    for name, a in (('domain', dom), ('tips', tip)):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(name + ' and mask must have the same shape')
    fields = [new(dt) for dt in ('float64', 'int32', 'uint8', 'int32')] if return_fields else [None] * 4
    opt = lambda a: ptr(a) if a is not None else None
    if on_device:
        torch.cuda.synchronize(m.device)
    dll = _lib()
    counts = np.full(10, -1, np.int64)
    cap_pair, cap_vox = 4096, 1 << 18                # most masks have fewer; anything else learns its sizes from the first call
    for _ in range(2):
        pairs, costs, offsets, voxels = np.empty((cap_pair, 6), np.int64), np.empty(cap_pair, np.float64), np.empty(cap_pair + 1, np.int64), np.empty(cap_vox, np.int64)
        rc = dll.vmask_bridge(dev, ptr(m), opt(dom), ptr(c), code, opt(tip), *shape, sp.ctypes.data if sp is not None else None, maxCost, int(tipRule),
                              counts.ctypes.data, pairs.ctypes.data, costs.ctypes.data, cap_pair, offsets.ctypes.data, voxels.ctypes.data, cap_vox,
                              *(opt(f) for f in fields))
        if rc == _E_ARG and counts[0] >= 0 and (counts[5] > cap_pair or counts[6] > cap_vox):
            cap_pair, cap_vox = int(counts[5]), int(counts[6])
            continue
        break
    _G._check(rc)
    nb, total = int(counts[5]), int(counts[6])
    if info is not None:
        info.update(zip(COUNT_KEYS, (int(x) for x in counts)))
    pairs = pairs[:nb]
    return Bridges(pairs[:, 0:2].copy(), pairs[:, 2:4].copy(), pairs[:, 4:6].copy(), costs[:nb].copy(), offsets[:nb + 1].copy(), voxels[:total].copy(),
                   int(counts[0]), shape, *fields)


def selectBridges(bridges, forest=True):
    """Which bridges to take (host only): Kruskal over the bridges in the order (cost, a, b).  With ``forest=True`` a bridge is
    taken only if it joins two different trees of what was taken before it, so bridging never closes a loop; ``False`` takes
    all.  Returns the indices taken (int64, ascending)."""
    n = len(bridges)
    pairs = np.asarray(bridges.pairs, np.int64).reshape(n, 2)
    if not forest:
        return np.arange(n, dtype=np.int64)
    order = np.lexsort((pairs[:, 1], pairs[:, 0], np.asarray(bridges.cost, np.float64)))
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    for i in order.tolist():
        ra, rb = find(int(pairs[i, 0])), find(int(pairs[i, 1]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            taken.append(i)
    return np.array(sorted(taken), dtype=np.int64)


def applyBridges(mask, bridges, keep, thicken=0, domain=None, device=0):
    """``(bridged, bridgeOnly)``, both uint8 0/1: the mask plus the path voxels of the bridges `keep` (indices, as
    `selectBridges` returns them), the paths thickened by `thicken` steps of `brain.binaryDilation` inside `domain` (default:
    the whole volume); ``bridgeOnly`` holds what was added.  Tensors on the GPU give tensors."""
    from . import brain as _B
    thicken = int(thicken)
    if thicken < 0:
        raise ValueError('thicken: not negative')
    on_device = _G._on_device(mask)
    m = _G._u8t(mask) if on_device else _G._u8c(mask)
    shape = tuple(int(n) for n in m.shape)
    if shape != tuple(bridges.shape):
        raise ValueError('mask and bridges must have the same shape')
    keep = np.asarray(keep, np.int64).reshape(-1)
    if keep.size and (keep.min() < 0 or keep.max() >= len(bridges)):
        raise ValueError('keep: indices of bridges')
    line = np.zeros(shape, np.uint8)
    for i in keep.tolist():
        line.reshape(-1)[bridges.voxels[bridges.offsets[i]:bridges.offsets[i + 1]]] = 1
    if on_device:
        import torch
        line = torch.as_tensor(line, device=m.device)
    if thicken and keep.size:
        line = _B.binaryDilation(line, steps=thicken, device=device)
        if domain is not None:
            d = domain if on_device == _G._on_device(domain) else (torch.as_tensor(np.asarray(domain), device=m.device) if on_device else _host(domain))
            if tuple(d.shape) != shape:
                raise ValueError('domain and mask must have the same shape')
            line = line * ((d != 0) | (m != 0))
    only = line * (m == 0)
    return (m | line), only


def reconnect(vesselVolumeMask, vesselness, brainVolumeMask=None, floor=0.05, maxCost=DEFAULT_MAX_COST, tipRule=1, tipReach=3.0, forest=True, thicken=0,
              spacing=None, device=0, info=None):
    """`vesselCost`, `tipRegions` (for ``tipRule > 0``), `bridgeCandidates` inside the brain mask, `selectBridges` and
    `applyBridges` in one call.  Returns ``(bridged, bridgeOnly, bridges, keep)``."""
    cost = vesselCost(vesselness, floor=floor, brainVolumeMask=brainVolumeMask)
    tips = tipRegions(vesselVolumeMask, reach=tipReach, spacing=spacing, device=device) if tipRule else None
    bridges = bridgeCandidates(vesselVolumeMask, cost, domain=brainVolumeMask, tips=tips, maxCost=maxCost, tipRule=tipRule, spacing=spacing,
                               device=device, info=info)
    keep = selectBridges(bridges, forest=forest)
    bridged, only = applyBridges(vesselVolumeMask, bridges, keep, thicken=thicken, domain=brainVolumeMask, device=device)
    return bridged, only, bridges, keep


def main(baseFolder, maskName='vesselVolumeMask.nii.gz', outputName='vesselVolumeMaskBridged.nii.gz', **parameters):
    """File-level driver: reads `maskName`, ``vesselnessFiltered.nii.gz`` and ``brainVolumeMask.nii.gz`` from `baseFolder`, writes
    the bridged mask as `outputName` (uint8, the input's affine) and ``bridges.npz`` (pairs, ends, roots, cost, offsets, voxels,
    keep).  The spacing is the affine's column norms unless given.  The input mask is overwritten only when `outputName` names it."""
    if baseFolder is None:
        raise ValueError('baseFolder: the folder that holds the three volumes')
    mask, affine = _G.loadVolume(baseFolder, maskName)
    vesselness, _ = _G.loadVolume(baseFolder, 'vesselnessFiltered.nii.gz')
    brain, _ = _G.loadVolume(baseFolder, 'brainVolumeMask.nii.gz')
    if 'spacing' not in parameters:
        parameters['spacing'] = np.sqrt((np.asarray(affine, np.float64)[:3, :3] ** 2).sum(axis=0))
    info = {}
    bridged, _, bridges, keep = reconnect(mask, vesselness, brainVolumeMask=brain, info=info, **parameters)
    _G.saveVolume(bridged, affine, os.path.join(baseFolder, outputName), astype=np.uint8)
    np.savez_compressed(os.path.join(baseFolder, BRIDGE_FILE), pairs=bridges.pairs, ends=bridges.ends, roots=bridges.roots, cost=bridges.cost,
                        offsets=bridges.offsets, voxels=bridges.voxels, keep=keep)
    print('Bridges: {} candidates between {} components, {} taken'.format(len(bridges), bridges.ncomp, len(keep)))
    return bridged, bridges, keep
