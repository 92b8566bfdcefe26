"""Hand-off to the external skeletoniser.

The reference's ``skeletonization.analyze()`` (skeletonization.py:97-146) prepares three files for A. Tabb's
curve-skeleton tool before it starts the Docker image (:148-162, host plumbing outside this path).  This module
produces the same three files from a vessel mask; only their *format* is the contract:

``BB.txt``      three lines - ``1``, the lower corner ``0 0 0``, the upper corner = the volume's shape in the tool's
                axis order (z, y, x: the reference swaps axes 0 and 2 first); no trailing newline
``xyz.txt``     first line the number of vessel voxels, then one ``z y x`` row per voxel in raster order of the
                swapped volume, unsigned integers
``vesselVolumeMaskLabelInfo.npz``
                the 26-connected component labels of the swapped volume and the per-component (label, size) table,
                under the reference's key names (its later stages read them back)

Component labelling runs on the GPU (``vmask_label``).

The centrelines themselves - what the reference reads back from that tool and saves as ``skeleton.nii.gz`` (:783-790) -
are computed here on the GPU: ``skeletonize`` (``vmask_skeleton``: subfield-sequential thinning),
``skeletonRadii`` and the file-level ``main``.  They work in the caller's axis order; the axis swap above belongs to
the external tool's file format and is not applied.

The other two files of that stage (:771-781), ``segmentList.npz`` and ``graphRepresentation.graphml``, come from
``traceSegments`` (``vmask_segments``: the 26-adjacency graph of the skeleton voxels traced into segments on the GPU by
pointer jumping), ``saveSegmentList`` and ``writeGraphml``; ``main(..., segments=True)`` writes them.

``branchTerritories`` (``vmask_territories``: an exact Euclidean feature transform on the GPU) carries the
segments back to the voxels: every voxel of the mask gets the label of the segment that owns its nearest skeleton voxel, every
segment its voxel count; ``territoryVolumes`` turns the counts into volumes and ``main(..., segments=True, territories=True)``
writes ``segmentLabels.nii.gz`` and ``segmentTerritories.npz``.

``geodesicTerritories`` (``vmask_geodesic``: shortest paths inside the mask) is the same map with nearness
measured through the vessels and in the volume's spacing: a thin vessel beside a thick one no longer takes the thick one's rim.
``main(..., segments=True, territories=True, geodesic=True)`` writes the two files from it, and ``centrelineDistance.nii.gz``.

``branchGraph`` (``vmask_branches``: DESIGN.md section 9, "f10 branch graph") turns the traced skeleton into the graph the later
stages expect: every cluster of junction voxels is one node, short spurs are pruned by a stated rule, the result is again a thin
skeleton.  ``branchSegments`` gives its branches as the reference's ``segmentList``; ``main(..., segments=True, prune=(3, 1.0))``
writes the files from them.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import generateVesselVolume as _G
from . import geodesic as _geo
from .generateVesselVolume import labelVolume, loadVolume, saveVolume

RESULT_DIR = 'skeletonizationResult'
LABEL_CACHE = 'vesselVolumeMaskLabelInfo.npz'


def to_tool_axes(vesselVolumeMask):
    """Binary uint8 volume in the skeletoniser's (z, y, x) axis order."""
    return np.swapaxes((np.asarray(vesselVolumeMask) != 0).astype(np.uint8), 0, 2)


def write_bb(path, shape):
    """Bounding-box file: one box, from the origin to `shape`."""
    lines = ['1', '0 0 0', ' '.join(str(int(n)) for n in shape)]
    with open(path, 'w') as f:
        f.write('\n'.join(lines))


def write_xyz(path, mask):
    """Voxel list: count, then the coordinates of every non-zero voxel of `mask` in raster order."""
    coords = np.argwhere(mask)
    with open(path, 'w') as f:
        f.write('%d\n' % len(coords))
        np.savetxt(f, coords, fmt='%1u')
    return len(coords)


def write_label_cache(path, labeled, label_result):
    np.savez_compressed(path, vesselVolumeMaskLabeled=labeled, vesselVolumeMaskLabelResult=label_result)


def analyze_export(vesselVolumeMask, baseFolder, device=0):
    """Write BB.txt, xyz.txt and the label cache into <baseFolder>/skeletonizationResult; returns that directory."""
    mask = to_tool_axes(vesselVolumeMask)
    out_dir = os.path.join(baseFolder, RESULT_DIR)
    if not os.path.isdir(out_dir):
        os.makedirs(out_dir)
        print('Directory {} created.'.format(out_dir))
    labeled, label_result = labelVolume(mask, minSize=1, device=device)
    cache = os.path.join(out_dir, LABEL_CACHE)
    write_label_cache(cache, labeled, label_result)
    print('{} saved to {}.'.format(LABEL_CACHE, cache))
    write_bb(os.path.join(out_dir, 'BB.txt'), mask.shape)
    write_xyz(os.path.join(out_dir, 'xyz.txt'), mask)
    return out_dir


SKELETON_FILE = 'skeleton.nii.gz'


def _skeleton_lib():
    dll = _G._lib()
    if not getattr(dll.vmask_skeleton, 'argtypes', None):
        p, i64 = C.c_void_p, C.c_int64
        dll.vmask_skeleton.argtypes = [C.c_int, p, i64, i64, i64, p, C.POINTER(i64), C.POINTER(i64)]
        dll.vmask_segments.argtypes = [C.c_int, p, i64, i64, i64, p, p, i64, p, i64]
        dll.vmask_territories.argtypes = [C.c_int, p, p, i64, i64, i64, p, i64, p, p, p, p]
        dll.vmask_branches.argtypes = [C.c_int, p, i64, i64, i64, i64, C.c_double, p, i64, p, p, p, i64, p, p, i64, p, i64]
    return dll


def skeletonize(vesselVolumeMask, device=0, info=None):
    """Curve skeleton of ``vesselVolumeMask != 0``: a uint8 0/1 volume of the same shape, a subset of the mask with the
    mask's 26-components, cavities and tunnels, one voxel thin, curve end points kept.  A tensor
    that lives on the GPU gives a uint8 tensor on the same device.  `info`, when a dict, receives ``kept`` (voxels left)
    and ``cycles`` (thinning cycles run)."""
    dll = _skeleton_lib()
    kept, cycles = C.c_int64(), C.c_int64()
    if _G._on_device(vesselVolumeMask):
        import torch
        m = _G._u8t(vesselVolumeMask)
        out = torch.empty(m.shape, dtype=torch.uint8, device=m.device)
        torch.cuda.synchronize(m.device)
        _G._check(dll.vmask_skeleton(_G._dev_index(m), m.data_ptr(), *m.shape, out.data_ptr(), C.byref(kept), C.byref(cycles)))
    else:
        m = _G._u8c(vesselVolumeMask)
        out = np.empty(m.shape, np.uint8)
        _G._check(dll.vmask_skeleton(device, m.ctypes.data, *m.shape, out.ctypes.data, C.byref(kept), C.byref(cycles)))
    if info is not None:
        info['kept'], info['cycles'] = kept.value, cycles.value
    return out


def skeletonRadii(skeleton, vesselVolumeMask, device=0):
    """Vessel radius at every skeleton voxel, by the convention of manualCorrectionGUI.py:248: the Euclidean distance
    transform of the mask (on the GPU) looked up at the voxel.  Returns (coords int64 N x 3 in raster order, radii float64 N)."""
    sk = np.asarray(skeleton.cpu() if _G._on_device(skeleton) else skeleton)
    if sk.ndim != 3:
        raise ValueError('expected a 3-D volume')
    dt = _G.distance_transform_edt(vesselVolumeMask, device=device)
    if _G._on_device(dt):
        dt = dt.cpu().numpy()
    if dt.shape != sk.shape:
        raise ValueError('skeleton and vesselVolumeMask must have the same shape')
    coords = np.argwhere(sk).astype(np.int64)
    return coords, dt[tuple(coords.T)].astype(np.float64)


SEGMENT_FILE = 'segmentList.npz'
GRAPH_FILE = 'graphRepresentation.graphml'
_E_ARG = -1


def segmentArrays(skeleton, device=0, info=None):
    """The segments of the 26-adjacency graph of ``skeleton != 0`` as two arrays: ``offsets``
    (int64, segments + 1) and ``coords`` (int64, total x 3, the caller's axis order); segment k is
    ``coords[offsets[k]:offsets[k + 1]]``.  A segment ends at voxels with other than two neighbours and runs through voxels
    with exactly two; a closed curve of such voxels alone starts and ends at its voxel of smallest raster index.  Open
    segments run from the end of smaller raster index, closed ones towards the smaller second voxel; segments ascend by
    (first, second).  A tensor that lives on the GPU gives tensors on the same device.  `info`, when a dict, receives
    ``segments``, ``nodes``, ``isolated`` and ``rounds`` (pointer-jumping rounds run)."""
    dll = _skeleton_lib()
    counts = np.full(5, -1, np.int64)
    on_device = _G._on_device(skeleton)
    if on_device:
        import torch
        m = _G._u8t(skeleton)
        dev = _G._dev_index(m)
        nobj = int(torch.count_nonzero(m))
        alloc = lambda k: torch.empty(k, dtype=torch.int64, device=m.device)
        ptr = lambda a: a.data_ptr()
        torch.cuda.synchronize(m.device)
    else:
        m = _G._u8c(skeleton)
        dev = device
        nobj = int(np.count_nonzero(m))
        alloc = lambda k: np.empty(k, np.int64)
        ptr = lambda a: a.ctypes.data
    # a curve skeleton has about as many segment entries as voxels: one call; anything denser learns its sizes from the first
    cap_seg, cap_vox = nobj + 16, 2 * nobj + 16
    for _ in range(2):
        offsets, voxels = alloc(cap_seg + 1), alloc(cap_vox)
        rc = dll.vmask_segments(dev, ptr(m), *m.shape, counts.ctypes.data, ptr(offsets), cap_seg, ptr(voxels), cap_vox)
        if rc == _E_ARG and counts[0] >= 0 and (counts[0] > cap_seg or counts[1] > cap_vox):
            cap_seg, cap_vox = int(counts[0]), int(counts[1])
            continue
        break
    _G._check(rc)
    nseg, total = int(counts[0]), int(counts[1])
    offsets, voxels = offsets[:nseg + 1], voxels[:total]
    n1, n2 = int(m.shape[1]), int(m.shape[2])
    if on_device:
        import torch
        rows = torch.div(voxels, n2, rounding_mode='floor')
        coords = torch.stack((torch.div(rows, n1, rounding_mode='floor'), rows % n1, voxels % n2), dim=1)
        offsets = offsets.clone()
    else:
        coords = np.stack(np.unravel_index(voxels, m.shape), axis=1).astype(np.int64).reshape(total, 3)
        offsets = offsets.copy()
    if info is not None:
        info['segments'], info['nodes'], info['isolated'], info['rounds'] = nseg, int(counts[2]), int(counts[3]), int(counts[4])
    return offsets, coords


def traceSegments(skeleton, device=0, info=None):
    """The reference's ``segmentList``: a list of segments, each a list of ``(i0, i1, i2)`` tuples of Python ints, in the
    canonical form and order of `segmentArrays`."""
    offsets, coords = segmentArrays(skeleton, device=device, info=info)
    if _G._on_device(offsets):
        offsets, coords = offsets.cpu().numpy(), coords.cpu().numpy()
    points = [tuple(c) for c in coords.tolist()]
    offsets = offsets.tolist()
    return [points[offsets[k]:offsets[k + 1]] for k in range(len(offsets) - 1)]


def saveSegmentList(segmentList, path):
    """``segmentList.npz`` as the reference's later stages load it (``np.load(path, allow_pickle=True)['segmentList']``):
    a 1-D object array with one list of tuples per segment."""
    arr = np.empty(len(segmentList), dtype=object)          # (np.array of a ragged list raises)
    for k, seg in enumerate(segmentList):
        arr[k] = [tuple(int(c) for c in p) for p in seg]
    np.savez_compressed(path, segmentList=arr)


def writeGraphml(segmentList, path):
    """The graph of skeletonization.py:765-769 (``G.add_path(segment, segmentIndex=i)`` for every segment) as GraphML that
    ``networkx.read_graphml`` parses: the nodes are the voxels, with the id ``str((i0, i1, i2))`` that networkx writes for a
    tuple node; one edge per consecutive pair of a segment, with the integer attribute ``segmentIndex``."""
    nodes, edges = {}, {}
    for k, seg in enumerate(segmentList):
        ids = [str(tuple(int(c) for c in p)) for p in seg]
        for a in ids:
            nodes.setdefault(a, None)
        for a, b in zip(ids[:-1], ids[1:]):
            key = (a, b) if (b, a) not in edges else (b, a)   # (an undirected graph keeps one edge per pair: the last index wins)
            edges[key] = k
    with open(path, 'w', encoding='utf-8') as f:
        f.write('<?xml version=\'1.0\' encoding=\'utf-8\'?>\n')
        f.write('<graphml xmlns="http://graphml.graphdrawing.org/xmlns" xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
                'xsi:schemaLocation="http://graphml.graphdrawing.org/xmlns http://graphml.graphdrawing.org/xmlns/1.0/graphml.xsd">\n')
        f.write('  <key id="d0" for="edge" attr.name="segmentIndex" attr.type="long" />\n')
        f.write('  <graph edgedefault="undirected">\n')
        for a in nodes:
            f.write('    <node id="{}" />\n'.format(a))
        for (a, b), k in edges.items():
            f.write('    <edge source="{}" target="{}">\n      <data key="d0">{}</data>\n    </edge>\n'.format(a, b, k))
        f.write('  </graph>\n</graphml>\n')


BRANCH_FILE = 'branchGraph.npz'
BRANCH_COUNTS = ('nodes', 'clusters', 'endPoints', 'passThrough', 'branches', 'entries', 'isolated', 'droppedSegments',
                 'pruneRounds', 'spursRemoved', 'voxelsRemoved', 'labelRounds')


class BranchGraph:
    """What `branchGraph` returns.  ``skeleton`` (uint8 0/1, the input's shape: the skeleton after pruning); per node, ascending
    by the raster index of its representative voxel: ``nodeCoords`` (int64 N x 3), ``nodeKind`` (0 end point, 1 junction
    cluster), ``nodeSize`` (voxels of the cluster, 1 for an end point), ``nodeDegree`` (branch ends at the node; a loop counts
    twice); per branch, in the order of `segmentArrays`: ``branchEnds`` (int64 B x 2 node indices, -1 -1 for a closed curve that
    touches no node); branch k is ``coords[offsets[k]:offsets[k + 1]]`` and starts and ends at its nodes' representatives;
    ``counts``: a dict with the keys of `BRANCH_COUNTS`."""

    def __init__(self, skeleton, nodeCoords, nodeKind, nodeSize, nodeDegree, branchEnds, offsets, coords, counts):
        self.skeleton, self.nodeCoords, self.nodeKind, self.nodeSize, self.nodeDegree = skeleton, nodeCoords, nodeKind, nodeSize, nodeDegree
        self.branchEnds, self.offsets, self.coords, self.counts = branchEnds, offsets, coords, counts


def branchGraph(skeleton, minSpurLength=0, radiusFactor=0.0, vesselVolumeMask=None, dist=None, maxRounds=64, device=0, info=None):
    """The branch graph of ``skeleton != 0`` ("f10 branch graph") as a `BranchGraph`.  Junction voxels
    (more than two neighbours) that touch form one node, represented by the member with the most neighbours (then the smallest
    raster index); an end point is a node too.  The branches are the segments of `segmentArrays` without the two-voxel segments
    inside a junction cluster, each starting and ending at its nodes' representatives.  A branch from an end point to a junction
    cluster is a spur when its length L (voxels - 1) is at most `minSpurLength`, or at most `radiusFactor` times `dist` at the
    cluster's representative; per round every cluster loses at most one spur (the shortest, then the first), the volume is
    thinned again and the graph rebuilt, until a round finds none or `maxRounds` rounds have run.  `dist` defaults to
    ``distance_transform_edt(vesselVolumeMask)`` when a mask is given.  With the default parameters nothing is pruned.
    Host arrays give host arrays, tensors on the GPU give tensors on the same device.  `info`, when a dict, receives the counts."""
    dll = _skeleton_lib()
    if dist is None and vesselVolumeMask is not None:
        dist = _G.distance_transform_edt(vesselVolumeMask, device=device)
    on_device = _G._on_device(skeleton)
    counts = np.full(len(BRANCH_COUNTS), -1, np.int64)
    if on_device:
        import torch
        m = _G._u8t(skeleton)
        dev = _G._dev_index(m)
        nobj = int(torch.count_nonzero(m))
        alloc = lambda k, dt=torch.int64: torch.empty(k, dtype=dt, device=m.device)
        ptr = lambda a: a.data_ptr()
        if dist is not None:
            dist = (dist if _G._on_device(dist) else torch.as_tensor(np.asarray(dist), device=m.device)).to(torch.float64).contiguous()
        out = alloc(tuple(m.shape), torch.uint8)
        torch.cuda.synchronize(m.device)
    else:
        m = _G._u8c(skeleton)
        dev = device
        nobj = int(np.count_nonzero(m))
        alloc = lambda k, dt=np.int64: np.empty(k, dt)
        ptr = lambda a: a.ctypes.data
        if dist is not None:
            dist = np.ascontiguousarray(dist.cpu().numpy() if _G._on_device(dist) else dist, dtype=np.float64)
        out = alloc(m.shape, np.uint8)
    if dist is not None and tuple(dist.shape) != tuple(m.shape):
        raise ValueError('dist and skeleton must have the same shape')
    # a curve skeleton has fewer nodes and branches than voxels and about as many entries: one call; anything denser learns its sizes from the first
    cap_node, cap_branch, cap_vox = nobj + 16, nobj + 16, 3 * nobj + 16
    for _ in range(2):
        nodes, ends, offsets, voxels = alloc(4 * cap_node), alloc(2 * cap_branch), alloc(cap_branch + 1), alloc(cap_vox)
        rc = dll.vmask_branches(dev, ptr(m), *m.shape, int(minSpurLength), float(radiusFactor), ptr(dist) if dist is not None else None,
                                int(maxRounds), ptr(out), counts.ctypes.data, ptr(nodes), cap_node, ptr(ends), ptr(offsets), cap_branch,
                                ptr(voxels), cap_vox)
        if rc == _E_ARG and counts[0] >= 0 and (counts[0] > cap_node or counts[4] > cap_branch or counts[5] > cap_vox):
            cap_node, cap_branch, cap_vox = int(counts[0]), int(counts[4]), int(counts[5])
            continue
        break
    _G._check(rc)
    nn, nb, total = int(counts[0]), int(counts[4]), int(counts[5])
    nodes, ends, offsets, voxels = nodes[:4 * nn].reshape(nn, 4), ends[:2 * nb].reshape(nb, 2), offsets[:nb + 1], voxels[:total]
    n1, n2 = int(m.shape[1]), int(m.shape[2])
    if on_device:
        unravel = lambda v: torch.stack((torch.div(torch.div(v, n2, rounding_mode='floor'), n1, rounding_mode='floor'),
                                         torch.div(v, n2, rounding_mode='floor') % n1, v % n2), dim=1)
        copy = lambda a: a.clone()
    else:
        unravel = lambda v: np.stack(np.unravel_index(v, m.shape), axis=1).astype(np.int64).reshape(len(v), 3)
        copy = lambda a: a.copy()
    named = dict(zip(BRANCH_COUNTS, (int(c) for c in counts)))
    if info is not None:
        info.update(named)
    return BranchGraph(out, unravel(nodes[:, 0]), copy(nodes[:, 1]), copy(nodes[:, 2]), copy(nodes[:, 3]), copy(ends), copy(offsets),
                       unravel(voxels), named)


def branchSegments(result):
    """The branches of a `BranchGraph` as the reference's ``segmentList``: a list of lists of ``(i0, i1, i2)`` tuples of Python ints."""
    offsets, coords = result.offsets, result.coords
    if _G._on_device(offsets):
        offsets, coords = offsets.cpu().numpy(), coords.cpu().numpy()
    points = [tuple(c) for c in np.asarray(coords).tolist()]
    offsets = np.asarray(offsets).tolist()
    return [points[offsets[k]:offsets[k + 1]] for k in range(len(offsets) - 1)]


LABEL_FILE = 'segmentLabels.nii.gz'
TERRITORY_FILE = 'segmentTerritories.npz'


def branchTerritories(vesselVolumeMask, skeleton, offsets=None, coords=None, device=0, info=None, return_nearest=False):
    """The territory map of the segments of `skeleton`: ``labels`` (int32, the mask's shape) and
    ``sizes`` (int64, segments + 1).  The sites are the voxels with ``skeleton != 0``; a site's label is 1 + the smallest index
    of a segment it occurs in (a node shared by several segments belongs to the first), 0 for a site in no segment (an
    isolated voxel).  A voxel with ``vesselVolumeMask != 0`` gets the label of its nearest site by squared Euclidean distance in
    voxel units, among equidistant sites the one of smallest raster index; 0 outside the mask and where there is no site.
    ``sizes[l]`` counts the mask voxels with label l (``sizes[0]``: those left unassigned); ``sizes.sum()`` is the mask's voxel
    count.  `offsets` / `coords` are what `segmentArrays` returns for `skeleton` (computed here when not given).
    ``return_nearest=True`` adds ``nearest`` (int64: the raster index of the nearest site, -1 outside the mask or without a
    site).  Tensors that live on the GPU give tensors on the same device.  `info`, when a dict, receives ``segments``."""
    dll = _skeleton_lib()
    on_device = _G._on_device(vesselVolumeMask) or _G._on_device(skeleton)
    if (offsets is None) != (coords is None):
        raise ValueError('offsets and coords: both or neither')
    if on_device:
        import torch
        ref = vesselVolumeMask if _G._on_device(vesselVolumeMask) else skeleton
        as_t = lambda a: a if _G._on_device(a) else torch.as_tensor(np.asarray(a), device=ref.device)
        m, sk = _G._u8t(as_t(vesselVolumeMask)), _G._u8t(as_t(skeleton))
    else:
        m, sk = _G._u8c(vesselVolumeMask), _G._u8c(skeleton)
    if tuple(m.shape) != tuple(sk.shape):
        raise ValueError('skeleton and vesselVolumeMask must have the same shape')
    if offsets is None:
        offsets, coords = segmentArrays(sk, device=device)
    n1, n2 = int(m.shape[1]), int(m.shape[2])
    if on_device:
        dev = _G._dev_index(m)
        off = as_t(offsets).to(torch.int64).contiguous()
        co = as_t(coords).to(torch.int64).reshape(-1, 3)
        vox = ((co[:, 0] * n1 + co[:, 1]) * n2 + co[:, 2]).contiguous()
        nseg = int(off.numel()) - 1
        labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
        sizes = torch.empty(max(nseg, 0) + 1, dtype=torch.int64, device=m.device)
        nearest = torch.empty(m.shape, dtype=torch.int64, device=m.device) if return_nearest else None
        ptr = lambda a: a.data_ptr()
        torch.cuda.synchronize(m.device)
    else:
        dev = device
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        co = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
        vox = np.ascontiguousarray((co[:, 0] * n1 + co[:, 1]) * n2 + co[:, 2])
        nseg = int(off.size) - 1
        labels = np.empty(m.shape, np.int32)
        sizes = np.empty(max(nseg, 0) + 1, np.int64)
        nearest = np.empty(m.shape, np.int64) if return_nearest else None
        ptr = lambda a: a.ctypes.data
    if nseg < 0 or off.ndim != 1:
        raise ValueError('offsets must hold segments + 1 entries')
    _G._check(dll.vmask_territories(dev, ptr(m), ptr(sk), *m.shape, ptr(off), nseg, ptr(vox) if len(vox) else None,
                                    ptr(labels), ptr(nearest) if return_nearest else None, ptr(sizes)))
    if info is not None:
        info['segments'] = nseg
    return (labels, sizes, nearest) if return_nearest else (labels, sizes)


def geodesicTerritories(vesselVolumeMask, skeleton, offsets=None, coords=None, spacing=None, device=0, info=None, return_distance=False):
    """The territory map of `branchTerritories` with nearness measured INSIDE the mask ("f9 geodesic"):
    ``labels`` (int32, the mask's shape) and ``sizes`` (int64, segments + 1).  The seeds are the skeleton voxels that lie in the
    mask and occur in a segment, with the site labels of `branchTerritories` (1 + the smallest index of a segment the voxel
    occurs in); skeleton voxels in no segment and skeleton voxels outside the mask are not seeds.  A voxel with
    ``vesselVolumeMask != 0`` gets the label of the seed at the smallest path length through the 26-adjacency graph of the
    mask's voxels, a step weighing its Euclidean length in `spacing` (default 1 1 1); where paths of equal length arrive from
    seeds of different labels the smallest label wins (not the smallest raster index, as in `branchTerritories`).  0 outside the
    mask and where no seed is reached; ``sizes[0]`` counts the mask voxels left unassigned, ``sizes.sum()`` is the mask's voxel
    count.  `offsets` / `coords` are what `segmentArrays` returns for `skeleton` (computed here when not given).
    ``return_distance=True`` adds ``distance`` (float64: the path length to that seed, ``+inf`` where none is reached, -1 outside
    the mask).  Tensors that live on the GPU give tensors on the same device.  `info`, when a dict, receives ``segments`` and
    the counts of `geodesic.geodesicDistance`."""
    on_device = _G._on_device(vesselVolumeMask) or _G._on_device(skeleton)
    if (offsets is None) != (coords is None):
        raise ValueError('offsets and coords: both or neither')
    if on_device:
        import torch
        ref = vesselVolumeMask if _G._on_device(vesselVolumeMask) else skeleton
        as_t = lambda a: a if _G._on_device(a) else torch.as_tensor(np.asarray(a), device=ref.device)
        m, sk = _G._u8t(as_t(vesselVolumeMask)), _G._u8t(as_t(skeleton))
    else:
        m, sk = _G._u8c(vesselVolumeMask), _G._u8c(skeleton)
    if tuple(m.shape) != tuple(sk.shape):
        raise ValueError('skeleton and vesselVolumeMask must have the same shape')
    if offsets is None:
        offsets, coords = segmentArrays(sk, device=device)
    n1, n2 = int(m.shape[1]), int(m.shape[2])
    # every segment entry inside the mask is a seed with the label k + 1 of its segment: the smallest label of a voxel holds
    if on_device:
        off = as_t(offsets).to(torch.int64).reshape(-1)
        co = as_t(coords).to(torch.int64).reshape(-1, 3)
        nseg = int(off.numel()) - 1
        if nseg < 0:
            raise ValueError('offsets must hold segments + 1 entries')
        vox = (co[:, 0] * n1 + co[:, 1]) * n2 + co[:, 2]
        lab = torch.repeat_interleave(torch.arange(1, nseg + 1, dtype=torch.int32, device=m.device), off[1:] - off[:-1])
        keep = m.reshape(-1)[vox] != 0
        vox, lab = vox[keep].contiguous(), lab[keep].contiguous()
    else:
        off = np.asarray(offsets, dtype=np.int64).reshape(-1)
        co = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
        nseg = int(off.size) - 1
        if nseg < 0:
            raise ValueError('offsets must hold segments + 1 entries')
        vox = (co[:, 0] * n1 + co[:, 1]) * n2 + co[:, 2]
        lab = np.repeat(np.arange(1, nseg + 1, dtype=np.int32), np.diff(off))
        keep = m.ravel()[vox] != 0
        vox, lab = np.ascontiguousarray(vox[keep]), np.ascontiguousarray(lab[keep])
    distance, labels, sizes = _geo._run(m, vox, lab, max(nseg, 0), spacing, device, return_distance, True, info)
    if info is not None:
        info['segments'] = nseg
    return (labels, sizes, distance) if return_distance else (labels, sizes)


def territoryVolumes(sizes, affine):
    """Voxel counts as volumes in the affine's units cubed: ``sizes * |det(affine[:3, :3])|``, float64."""
    return np.asarray(sizes, dtype=np.float64) * abs(float(np.linalg.det(np.asarray(affine, dtype=np.float64)[:3, :3])))


DISTANCE_FILE = 'centrelineDistance.nii.gz'


def main(baseFolder=None, segments=False, territories=False, geodesic=False, prune=None):
    """File-level equivalent of what the reference's skeleton stage leaves behind (:771-790): the skeleton of
    ``vesselVolumeMask.nii.gz`` as ``skeleton.nii.gz`` (uint8, the mask's affine) in the same folder; returns the skeleton.
    With ``segments=True`` also ``segmentList.npz`` and ``graphRepresentation.graphml`` beside it; returns
    ``(skeleton, segmentList)``.  With ``territories=True`` as well: ``segmentLabels.nii.gz`` (int32, the mask's affine; label
    k + 1 is entry k of ``segmentList.npz``, 0 is background or unassigned) and ``segmentTerritories.npz`` (``sizes``: voxels
    per label, ``volumes``: the same in the affine's units cubed); returns ``(skeleton, segmentList, labels, sizes)``.
    With ``geodesic=True`` as well those two files come from `geodesicTerritories` (nearness inside the mask, the spacing being
    the norms of the affine's columns) instead of `branchTerritories`, and ``centrelineDistance.nii.gz`` (float32, the mask's
    affine: the path length to the centre line in the affine's units, ``inf`` where none is reached, -1 outside the mask) is
    written too; returns ``(skeleton, segmentList, labels, sizes, distance)``.
    With ``prune=(minSpurLength, radiusFactor)`` and ``segments=True`` the skeleton goes through `branchGraph` first (`dist` being
    the distance transform of the mask): ``skeleton.nii.gz`` is the pruned skeleton, ``segmentList.npz`` and
    ``graphRepresentation.graphml`` hold its branches, ``branchGraph.npz`` the node and branch tables and the counts, and the
    territories are those of the pruned skeleton's branches.  A voxel of a junction cluster at which no branch ends occurs in no
    branch: as a site of the territories it has label 0, and the mask voxels nearest to it are counted in ``sizes[0]``.
    ``prune=None`` writes every file as before."""
    if prune is not None and not segments:
        raise ValueError('prune needs segments=True')
    if territories and not segments:
        raise ValueError('territories=True needs segments=True')
    if geodesic and not territories:
        raise ValueError('geodesic=True needs territories=True')
    if baseFolder is None:
        baseFolder = os.getcwd()
    vesselVolumeMask, affine = loadVolume(baseFolder, 'vesselVolumeMask.nii.gz')
    skeleton = skeletonize(vesselVolumeMask)
    if prune is not None:
        graph = branchGraph(skeleton, minSpurLength=prune[0], radiusFactor=prune[1], vesselVolumeMask=vesselVolumeMask)
        skeleton = graph.skeleton
    path = os.path.join(baseFolder, SKELETON_FILE)
    saveVolume(skeleton, affine, path, astype=np.uint8)
    print('{} saved to {}.'.format(SKELETON_FILE, path))
    if not segments:
        return skeleton
    if prune is not None:
        offsets, coords = graph.offsets, graph.coords
        path = os.path.join(baseFolder, BRANCH_FILE)
        np.savez_compressed(path, nodeCoords=graph.nodeCoords, nodeKind=graph.nodeKind, nodeSize=graph.nodeSize, nodeDegree=graph.nodeDegree,
                            branchEnds=graph.branchEnds, offsets=offsets, coords=coords,
                            counts=np.array([graph.counts[k] for k in BRANCH_COUNTS], np.int64), countNames=np.array(BRANCH_COUNTS))
        print('{} saved to {}.'.format(BRANCH_FILE, path))
    else:
        offsets, coords = segmentArrays(skeleton)
    points = [tuple(c) for c in coords.tolist()]
    segmentList = [points[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
    path = os.path.join(baseFolder, GRAPH_FILE)
    writeGraphml(segmentList, path)
    print('{} saved to {}.'.format(GRAPH_FILE, path))
    path = os.path.join(baseFolder, SEGMENT_FILE)
    saveSegmentList(segmentList, path)
    print('{} saved to {}.'.format(SEGMENT_FILE, path))
    if not territories:
        return skeleton, segmentList
    if geodesic:
        spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
        labels, sizes, distance = geodesicTerritories(vesselVolumeMask, skeleton, offsets, coords, spacing=spacing, return_distance=True)
    else:
        labels, sizes = branchTerritories(vesselVolumeMask, skeleton, offsets, coords)
    path = os.path.join(baseFolder, LABEL_FILE)
    saveVolume(labels, affine, path, astype=np.int32)
    print('{} saved to {}.'.format(LABEL_FILE, path))
    path = os.path.join(baseFolder, TERRITORY_FILE)
    np.savez_compressed(path, sizes=sizes, volumes=territoryVolumes(sizes, affine))
    print('{} saved to {}.'.format(TERRITORY_FILE, path))
    if not geodesic:
        return skeleton, segmentList, labels, sizes
    path = os.path.join(baseFolder, DISTANCE_FILE)
    saveVolume(distance, affine, path, astype=np.float32)
    print('{} saved to {}.'.format(DISTANCE_FILE, path))
    return skeleton, segmentList, labels, sizes, distance
