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

``branchMorphometry`` (``vmask_morphometry``: DESIGN.md section 9, "f11 branch morphometry") measures that graph: per branch the
path length, the chord, the tortuosity and the radius statistics, per node the radius, per three-branch bifurcation the angles and
the radius laws, and from roots the path distance and depth of every node.  ``main(..., segments=True, prune=(3, 1.0),
morphometry=True)`` writes ``branchMorphometry.npz``, ``graphRepresentationWithEdgeInfo.graphml``, ``segmentInfoDict.pkl`` and
``nodeInfoDict.pkl`` from it.

``partitionCompartments`` (``vmask_compartments``: DESIGN.md section 9, "f12 compartments") is the reference's compartment
partition: the graph walked from every compartment's initial voxels, never onto one of its boundary voxels; every vertex and
branch gets its compartment, depth and level.  ``compartmentTerritories`` carries the compartments back to the voxels of the
mask, ``compartmentSummary`` groups the morphometry by them, and ``main(..., segments=True, prune=(3, 1.0), compartments=...)``
writes ``partitionInfo.pkl`` and ``compartments.npz``.

``flowOnGraph`` (``vmask_flow`` through `flow.simulateFlow`: DESIGN.md section 9, "f13 flow") is the reference's flow stage on the
measured graph: the roots held at the inlet pressure, every reached end point at its terminal pressure, Hazen-Williams
resistances from ``pathLength`` and ``meanRadius``; ``main(..., morphometry=True, roots=..., flow=dict(...))`` writes
``flowResult.npz`` and the ``simulationData`` entries of the two info files.

``branchSplines`` (``vmask_centrelines``: DESIGN.md section 9, "f20 centreline splines") puts a smooth sub-voxel curve through every
branch of that graph - a natural cubic smoothing spline per branch, its smoothing parameter searched per branch - and returns position,
tangent, second derivative and curvature at every entry and the reference's three-point curvature statistic per branch
(``graphRelated.calculateCurvature``); ``branchMorphometry(..., localDirection='spline')`` takes its local directions from it, and
``main(..., prune=(3, 1.0), curvature=True)`` writes ``branchSplines.npz`` and the curvature keys of ``segmentInfoDict.pkl``.

``tubes.graphTubes`` (``vmask_tubes``: DESIGN.md section 9, "f21 tube model") is the way back from that graph to the voxels: the centre points
and radii rasterised to a label volume with per-branch voxel counts and their overlap with the mask;
``main(..., prune=(3, 1.0), morphometry=True, tubes=True)`` writes ``vesselVolumeModel.nii.gz``, ``branchLabelsModel.nii.gz`` and ``tubeModel.npz``.
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
        dll.vmask_morphometry.argtypes = [C.c_int, i64, i64, i64, p, p, i64, p, p, p, i64, p, p, i64, i64, p, p, p, p, p, p, p, p, p]
        dll.vmask_compartments.argtypes = [C.c_int, i64, i64, i64, p, i64, p, p, p, i64, i64, p, p, p, p] + [p] * 10
        dll.vmask_centrelines.argtypes = [C.c_int, i64, i64, i64, p, i64, p, p, C.c_double, C.c_double, C.c_double, C.c_double, i64, p, p, p, C.POINTER(C.c_double)]
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


MORPHOMETRY_FILE = 'branchMorphometry.npz'
EDGE_INFO_GRAPH_FILE = 'graphRepresentationWithEdgeInfo.graphml'
SEGMENT_INFO_FILE = 'segmentInfoDict.pkl'
NODE_INFO_FILE = 'nodeInfoDict.pkl'
# the columns of vmask_morphometry's two per-branch tables (include/vmask.h)
_MOR_INT, _MOR_F64 = 24, 5
MORPHOMETRY_RAW = ('stepCounts', 'jumps', 'jumpOffset', 'radiusCount', 'radiusSum', 'radiusDevSq', 'radiusMin', 'radiusMax', 'endDir', 'chord',
                   'pathLength', 'nodeRadius', 'incidentBranch', 'incidentEnd', 'entryRadius')
MORPHOMETRY_DEPTH = ('pathDistance', 'parentBranch', 'depthLevel', 'depthVoxel', 'branchLevel')
MORPHOMETRY_BRANCH = ('eculideanLength', 'tortuosity', 'voxelLength', 'meanRadius', 'sigma', 'aspectRatio', 'type', 'localBifurcationTorque')
MORPHOMETRY_BIFURCATION = ('bifurcationNode', 'bifurcationBranches', 'localBifurcationAmplitude', 'remoteBifurcationAmplitude', 'localBifurcationTilt',
                           'remoteBifurcationTilt', 'cubicLawResult', 'squareLawResult', 'minRadiusRatio', 'maxRadiusRatio', 'lengthRatio', 'normalVector')


class BranchMorphometry:
    """What `branchMorphometry` returns: one attribute per name of `MORPHOMETRY_RAW`, `MORPHOMETRY_BRANCH`, `MORPHOMETRY_BIFURCATION`
    and - ``None`` without roots - `MORPHOMETRY_DEPTH`; ``spacing`` (float64, 3), ``localSteps``, ``roots`` (int64 node indices) and
    ``depthRounds``.  ``names()`` lists the arrays that are set."""

    def names(self):
        return [k for k in MORPHOMETRY_RAW + MORPHOMETRY_DEPTH + MORPHOMETRY_BRANCH + MORPHOMETRY_BIFURCATION if getattr(self, k, None) is not None]


def stepWeights(spacing):
    """The length of a step of every class c = 4 |d0| + 2 |d1| + |d2| - 1: the square root of the squared spacings of the set axes,
    summed in the order of the axes (float64, 7)."""
    h = np.asarray(spacing, np.float64)
    bits = np.array([[(c + 1) >> 2 & 1, (c + 1) >> 1 & 1, (c + 1) & 1] for c in range(7)], np.float64)
    return _norm3(bits * h)


def _norm3(v):
    """sqrt((v0^2 + v1^2) + v2^2) along the last axis: one stated order (np.linalg.norm leaves it open)."""
    v = np.asarray(v, np.float64)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def pathLengths(stepCounts, jumpOffset, spacing):
    """``pathLength`` from the integer outputs: ((0 + stepCounts[0] w_0) + .. + stepCounts[6] w_6) + |front jump| + |back jump| with
    the weights of `stepWeights` and a jump's length being `_norm3` of its offset times the spacing - each product and sum one
    IEEE double operation, in this order.  The library does the same on the host; the two agree to the bit."""
    h = np.asarray(spacing, np.float64)
    w = stepWeights(h)
    sc = np.asarray(stepCounts, np.int64).reshape(-1, 7)
    jo = np.asarray(jumpOffset, np.int64).reshape(-1, 2, 3)
    out = np.zeros(len(sc), np.float64)
    for c in range(7):
        out = out + sc[:, c].astype(np.float64) * w[c]
    out = out + _norm3(jo[:, 0].astype(np.float64) * h)
    return out + _norm3(jo[:, 1].astype(np.float64) * h)


def interiorJumps(jumps, jumpOffset):
    """Per branch, the pairs that are no 26-neighbours other than its first and its last pair: ``jumps`` less the front and the back pair
    where ``jumpOffset`` is set (a branch of two entries has one pair, the front one).  f10's tables have none."""
    jo = np.asarray(jumpOffset, np.int64).reshape(-1, 2, 3)
    return np.asarray(jumps, np.int64) - (jo != 0).any(axis=2).sum(axis=1)


def _angle(a, b):
    """The angle between the rows of a and b in degrees, from the clipped cosine."""
    with np.errstate(invalid='ignore', divide='ignore'):
        c = (a * b).sum(axis=-1) / (_norm3(a) * _norm3(b))
    return np.arccos(np.clip(c, -1.0, 1.0)) / np.pi * 180


def _two_entry_radii(meanRadius, sigma, n, ends):
    """A branch of two entries has no interior to sample: its ``meanRadius`` becomes what the reference gives it
    (manualCorrectionGUI.py:315-334) and its ``sigma`` NaN, in place.  Per end: ``np.mean`` of the meanRadius of every other branch end
    at that node whose branch has a value - the longer branches, and the two-entry branches of smaller index, which the reference
    has handled by then - or 0 without one; then the mean of the two ends' values, or the one that is not 0, or 0."""
    short = np.flatnonzero(n == 2)
    if not len(short):
        return
    flat = ends.ravel()
    by_node = np.argsort(flat, kind='stable')                             # the branch ends (2 b + e) grouped by node
    nodes = flat[by_node]
    known = n != 2
    for b in short.tolist():
        side = []
        for v in ends[b].tolist():
            there = by_node[np.searchsorted(nodes, v, 'left'):np.searchsorted(nodes, v, 'right')] >> 1 if v >= 0 else np.zeros(0, np.int64)
            values = [float(meanRadius[k]) for k in there.tolist() if k != b and known[k]]
            side.append(float(np.mean(values)) if values else 0.0)
        head, tail = side
        meanRadius[b] = (head + tail) / 2 if head != 0 and tail != 0 else head if head != 0 else tail
        sigma[b] = np.nan
        known[b] = True


def deriveMorphometry(raw, offsets, branchEnds, nodeKind, spacing):
    """The quantities that follow from vmask_morphometry's outputs by B- or N-sized numpy work; `raw` maps the names of
    `MORPHOMETRY_RAW` (and of `MORPHOMETRY_DEPTH`, or None) to host arrays.  Returns a dict with the names of `MORPHOMETRY_BRANCH` and
    `MORPHOMETRY_BIFURCATION`; the formulas are those of `branchMorphometry`'s docstring.  An optional key ``localDirection`` of `raw`
    (float64, B x 2 x 3: per branch end a direction from the node inwards, in the spacing's units) replaces ``endDir * spacing`` as
    the local direction; everything after the direction is unchanged."""
    h = np.asarray(spacing, np.float64)
    off = np.asarray(offsets, np.int64)
    ends = np.asarray(branchEnds, np.int64).reshape(-1, 2)
    kind = np.asarray(nodeKind, np.int64)
    B = len(off) - 1
    n = np.diff(off)
    out = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        out['eculideanLength'] = _norm3(raw['chord'].astype(np.float64) * h)
        out['tortuosity'] = raw['pathLength'] / out['eculideanLength']
        out['voxelLength'] = n.astype(np.int64)
        out['meanRadius'] = raw['radiusSum'] / raw['radiusCount'].astype(np.float64)
        out['sigma'] = np.sqrt(raw['radiusDevSq'] / raw['radiusCount'].astype(np.float64))
        _two_entry_radii(out['meanRadius'], out['sigma'], n, ends)
        out['aspectRatio'] = raw['pathLength'] / out['meanRadius']
    open_ = ends[:, 0] >= 0 if B else np.zeros(0, bool)
    terminating = np.zeros(B, bool)
    terminating[open_] = (kind[ends[open_, 0]] == 0) | (kind[ends[open_, 1]] == 0)
    out['type'] = np.where(open_, np.where(terminating, 0, 1), -1).astype(np.int64)
    # ---- the bifurcation table
    ib, ie = np.asarray(raw['incidentBranch'], np.int64).reshape(-1, 3), np.asarray(raw['incidentEnd'], np.int64).reshape(-1, 3)
    rows = np.flatnonzero((ib[:, 0] >= 0) & (n[np.maximum(ib, 0)] >= 3).all(axis=1)) if len(ib) and B else np.zeros(0, np.int64)
    K = len(rows)
    b3, e3 = ib[rows], ie[rows]                                           # K x 3, ascending branch index
    if raw.get('localDirection') is not None:                             # (float directions per branch end, in the spacing's units)
        local = np.asarray(raw['localDirection'], np.float64).reshape(-1, 2, 3)[b3, e3]
    else:
        local = raw['endDir'].reshape(-1, 2, 3)[b3, e3].astype(np.float64) * h         # K x 3 x 3: from the node inwards
    remote = (raw['chord'][b3] * np.where(e3 == 0, 1, -1)[..., None]).astype(np.float64) * h   # from the node to the far end
    with np.errstate(invalid='ignore', divide='ignore'):
        unit = local / _norm3(local)[..., None]
    cos = np.stack([(unit[:, 0] * unit[:, 1]).sum(-1), (unit[:, 1] * unit[:, 2]).sum(-1), (unit[:, 2] * unit[:, 0]).sum(-1)], axis=1).reshape(K, 3)
    order = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])[np.argmax(cos, axis=1) if K else np.zeros(0, np.int64)].reshape(K, 3)
    if raw.get('parentBranch') is not None and K:
        pb = np.asarray(raw['parentBranch'], np.int64)[rows]
        is_parent = b3 == pb[:, None]
        known = is_parent.any(axis=1)
        by_depth = np.argsort(is_parent, axis=1, kind='stable')          # the two children in ascending order, the parent last
        order = np.where(known[:, None], by_depth, order)
    take = lambda a: np.take_along_axis(a, order[..., None] if a.ndim == 3 else order, axis=1)
    b3, local, remote = take(b3), take(local), take(remote)
    out['bifurcationNode'], out['bifurcationBranches'] = rows.astype(np.int64), b3.reshape(K, 3)
    out['localBifurcationAmplitude'] = _angle(local[:, 0], local[:, 1])
    out['remoteBifurcationAmplitude'] = _angle(remote[:, 0], remote[:, 1])
    against = -local[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        for name, v in (('localBifurcationTilt', local), ('remoteBifurcationTilt', remote)):
            half = v[:, 0] / _norm3(v[:, 0])[:, None] + v[:, 1] / _norm3(v[:, 1])[:, None]
            out[name] = np.where(_norm3(half) > 1e-4, _angle(half, against), np.nan)
        r, l = out['meanRadius'][b3].reshape(K, 3), raw['pathLength'][b3].reshape(K, 3)
        out['cubicLawResult'] = (r[:, 0] ** 3 + r[:, 1] ** 3) / r[:, 2] ** 3
        out['squareLawResult'] = (r[:, 0] ** 2 + r[:, 1] ** 2) / r[:, 2] ** 2
        out['minRadiusRatio'] = np.minimum(r[:, 0], r[:, 1]) / r[:, 2]
        out['maxRadiusRatio'] = np.maximum(r[:, 0], r[:, 1]) / r[:, 2]
        out['lengthRatio'] = np.minimum(l[:, 0], l[:, 1]) / l[:, 2]
        normal = np.cross(local[:, 0], local[:, 1]).reshape(K, 3)
        out['normalVector'] = normal / _norm3(normal)[:, None]
    # ---- per branch between two tabulated bifurcations: the angle of their normals, folded to at most 90 degrees
    row_of = np.full(max(len(kind), 1), -1, np.int64)                     # (a closed curve alone: no node to look up)
    row_of[rows] = np.arange(K)
    torque = np.full(B, np.nan)
    both = np.flatnonzero(open_ & (row_of[np.maximum(ends[:, 0], 0)] >= 0) & (row_of[np.maximum(ends[:, 1], 0)] >= 0)) if B else np.zeros(0, np.int64)
    if len(both):
        t = _angle(out['normalVector'][row_of[ends[both, 0]]], out['normalVector'][row_of[ends[both, 1]]])
        torque[both] = np.where(t > 90, 180 - t, t)
    out['localBifurcationTorque'] = torque
    return out


def _root_indices(roots, nodeCoords):
    """Node indices from `roots`: an item that is a sequence of three numbers is a coordinate and must be a node's representative."""
    if roots is None:
        return np.zeros(0, np.int64)
    nc = np.asarray(nodeCoords.cpu() if _G._on_device(nodeCoords) else nodeCoords, np.int64).reshape(-1, 3)
    items = roots.tolist() if hasattr(roots, 'tolist') else roots
    items = list(items) if isinstance(items, (list, tuple)) else [items]
    out = []
    for r in items:
        if np.ndim(r) == 0:
            k = int(r)
            if not 0 <= k < len(nc):
                raise ValueError('root {} is no node index (the graph has {} nodes)'.format(k, len(nc)))
        else:
            if len(r) != 3:
                raise ValueError('a root is a node index or a coordinate triple')
            hit = np.flatnonzero((nc == np.asarray(r, np.int64)).all(axis=1))
            if not len(hit):
                raise ValueError('root {} is no node representative'.format(tuple(int(c) for c in r)))
            k = int(hit[0])
        out.append(k)
    return np.array(out, np.int64)


SPLINE_FILE = 'branchSplines.npz'
# the columns of vmask_centrelines' tables (include/vmask.h)
SPLINE_ENTRY = ('u', 'position', 'second', 'tangent', 'curvature')
SPLINE_BRANCH = ('smoothing', 'residual', 'splineLength', 'maxCurvature', 'meanCurvature', 'solves', 'capped', 'samples')
_SPL_ENTRY, _SPL_F64, _SPL_INT = 11, 5, 3


class BranchSplines:
    """What `branchSplines` returns: one attribute per name of `SPLINE_ENTRY` (per entry of ``graph.coords``: ``u`` the parameter,
    ``position``, ``second`` and ``tangent`` x 3, ``curvature``) and of `SPLINE_BRANCH` (per branch: ``smoothing`` the lambda used,
    ``residual``, ``splineLength``, ``maxCurvature``, ``meanCurvature``, float64; ``solves``, ``capped``, ``samples``, int64); ``spacing``
    and the parameters used: ``endWeight``, ``residualPerPoint``, ``sampleStep``, ``fixedSmoothing`` (None in search mode)."""

    def names(self):
        return list(SPLINE_ENTRY + SPLINE_BRANCH)


def splineScale(spacing):
    """``(l2, l, lambda_lo, lambda_hi)`` of a spacing: l2 = ((h0^2 + h1^2) + h2^2) / 3, l = sqrt(l2), and 2^-24, 2^24 times l2 l - the
    range of the smoothing parameter.  The library forms the same four on the host."""
    h = np.asarray(spacing, np.float64).reshape(3)
    l2 = ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]) / 3.0
    l = np.sqrt(l2)
    l3 = l2 * l
    return float(l2), float(l), float(l3 * 2.0 ** -24), float(l3 * 2.0 ** 24)


def branchSplines(graph, spacing=None, smoothing=None, residualPerPoint=None, endWeight=20.0, sampleStep=None, device=0, info=None, ldsEntries=0):
    """A smooth sub-voxel curve through every branch of a `BranchGraph` (``vmask_centrelines``, DESIGN.md section 9, "f20
    centreline splines") as a `BranchSplines`: per branch the natural cubic smoothing spline (Reinsch) through its entries in
    the parameter u = the cumulated step length in `spacing`, minimising sum_i w_i |y_i - f(u_i)|^2 + lambda int |f''|^2 du with
    w = 1 and `endWeight` at the first and last entry.  include/vmask.h states every operation; the GPU equals
    tests/centreline_model.py to the bit.
    `smoothing` fixes lambda (inside the range of `splineScale`); the default searches, per branch, the largest lambda of 24
    bisection steps on the geometric mean whose weighted residual is at most ``residualPerPoint * n`` (default 0.25 l2: an RMS
    deviation of half a voxel per entry).  ``capped`` is 1 where the branch took lambda_hi (its least-squares line already meets the
    target: every digitally straight branch, every branch of two entries), 2 where even lambda_lo misses it.  `sampleStep` (default
    0.5 l) is the spacing of the resampling behind ``splineLength``, ``maxCurvature`` and ``meanCurvature`` - the three-point
    curvature 4 S / (a b c) of the reference's ``curvature_by_triangle`` over consecutive samples; ``curvature`` per entry is the
    analytic |f' x f''| / |f'|^3.  Positions are in the units of `spacing`, curvatures in their inverse.
    A closed curve (first entry = last entry) is fitted as an OPEN curve with natural ends: no periodic spline.  FITPACK's knot
    placement (``splprep(s=...)``, which the reference calls) is not reproduced; parity with it is not claimed.
    A host graph gives host arrays, a graph of tensors on the GPU gives tensors on the same device.  `info`, when a dict, receives
    ``capped`` (branches with a cap flag), ``solves`` (their total) and ``kernel_ms`` (the kernels' time by hipEvents).  `ldsEntries`
    (0: the default of 256, at most 512) is the longest branch fitted in LDS; it changes no output bit.
    ``ValueError``: a spacing that is not finite and positive or with max / min > 1000, `endWeight` or `sampleStep` not finite and
    positive, `residualPerPoint` likewise, `smoothing` outside the range."""
    h = np.ones(3, np.float64) if spacing is None else np.ascontiguousarray(np.asarray(spacing, np.float64).reshape(3))
    if not (np.isfinite(h).all() and (h > 0).all()) or h.max() / h.min() > 1000.0:
        raise ValueError('spacing must be finite and positive with max / min <= 1000')
    l2, l, lam_lo, lam_hi = splineScale(h)
    if not (np.isfinite(endWeight) and endWeight > 0):
        raise ValueError('endWeight must be finite and positive')
    rho = 0.25 * l2 if residualPerPoint is None else float(residualPerPoint)
    step = 0.5 * l if sampleStep is None else float(sampleStep)
    if not (np.isfinite(rho) and rho > 0):
        raise ValueError('residualPerPoint must be finite and positive')
    if not (np.isfinite(step) and step > 0):
        raise ValueError('sampleStep must be finite and positive')
    if smoothing is not None and not (np.isfinite(smoothing) and lam_lo <= float(smoothing) <= lam_hi):
        raise ValueError('smoothing must lie in [{!r}, {!r}] (2^-24 .. 2^24 times l^3 of the spacing)'.format(lam_lo, lam_hi))
    on_device = _G._on_device(graph.offsets)
    shape = tuple(int(k) for k in graph.skeleton.shape)
    n1, n2 = shape[1], shape[2]
    B = int(graph.offsets.shape[0]) - 1
    if on_device:
        import torch
        tdev = graph.offsets.device
        dev = _G._dev_index(graph.offsets)
        lin = lambda c: ((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2]).to(torch.int64).contiguous()
        off = graph.offsets.to(torch.int64).contiguous()
        alloc = lambda shp, dt: torch.empty(shp, dtype=torch.int64 if dt is np.int64 else torch.float64, device=tdev)
        ptr = lambda a: a.data_ptr() if a.numel() else None
        host = lambda a: a.cpu().numpy()
        torch.cuda.synchronize(tdev)
    else:
        dev = device
        lin = lambda c: np.ascontiguousarray((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2], dtype=np.int64)
        off = np.ascontiguousarray(graph.offsets, dtype=np.int64)
        alloc = lambda shp, dt: np.empty(shp, dt)
        ptr = lambda a: a.ctypes.data if a.size else None
        host = lambda a: a
    vox = lin(graph.coords.reshape(-1, 3))
    E = int(vox.shape[0])
    ef, bf, bi = alloc((E, _SPL_ENTRY), np.float64), alloc((B, _SPL_F64), np.float64), alloc((B, _SPL_INT), np.int64)
    ms = C.c_double(0.0)
    _G._check(_skeleton_lib().vmask_centrelines(dev, *shape, ptr(off) if B else None, B, ptr(vox), h.ctypes.data, float(endWeight),
                                                0.0 if smoothing is None else float(smoothing), rho, step, int(ldsEntries), ptr(ef), ptr(bf), ptr(bi), C.byref(ms)))
    out = {'u': ef[:, 0], 'position': ef[:, 1:4], 'second': ef[:, 4:7], 'tangent': ef[:, 7:10], 'curvature': ef[:, 10],
           'smoothing': bf[:, 0], 'residual': bf[:, 1], 'splineLength': bf[:, 2], 'maxCurvature': bf[:, 3], 'meanCurvature': bf[:, 4],
           'solves': bi[:, 0], 'capped': bi[:, 1], 'samples': bi[:, 2]}
    result = BranchSplines()
    for k, v in out.items():
        setattr(result, k, v.contiguous() if on_device else np.ascontiguousarray(v))
    result.spacing, result.endWeight, result.residualPerPoint, result.sampleStep = h, float(endWeight), rho, step
    result.fixedSmoothing = None if smoothing is None else float(smoothing)
    if info is not None:
        hbi = host(bi)
        info['capped'], info['solves'], info['kernel_ms'] = int((hbi[:, 1] != 0).sum()), int(hbi[:, 0].sum()), float(ms.value)
    return result


def branchMorphometry(graph, dist=None, vesselVolumeMask=None, spacing=None, roots=None, localSteps=5, device=0, info=None, localDirection='chord',
                      splines=None):
    """The morphometry of a `BranchGraph` (``vmask_morphometry``, DESIGN.md section 9, "f11 branch morphometry") as a
    `BranchMorphometry`.  `dist` is the radius volume (default ``distance_transform_edt(vesselVolumeMask)``), `spacing` the voxel
    size per axis (default 1 1 1; positive, finite, max / min <= 1000), `roots` node indices or coordinate triples of node
    representatives (``ValueError`` when a triple is none), `localSteps` the reach of the local direction.  A host graph gives
    host arrays, a graph of tensors on the GPU gives tensors on the same device (the derived quantities are computed from host
    copies of the B- and N-sized outputs and sent back).  `info`, when a dict, receives ``depthRounds``, ``levelRounds`` and
    ``interiorJumps``: the pairs of consecutive entries INSIDE a branch (not its first or last pair) that are no 26-neighbours.
    `branchGraph` emits none; a table that has one is refused with a ``ValueError`` after the kernels have run, because
    ``pathLength`` counts the two end pairs only and would come out short (the reference sums every pair).

    From the kernels, for a branch b of n entries (include/vmask.h has the summation order):
      stepCounts[b, c]   consecutive entry pairs of class c = 4 |d0| + 2 |d1| + |d2| - 1;  jumps[b]: pairs that are not 26-adjacent
      jumpOffset[b]      the offset of the first / the last pair where it is a jump (inside a cluster that is no clique), else 0
      radiusCount, radiusSum, radiusDevSq, radiusMin, radiusMax
                         of dist at the interior entries 1 .. n - 2 (both entries when n == 2); radiusDevSq = sum (r - mean)^2
      endDir[b, e]       the offset from the end entry e (0 first, 1 last) to the entry min(localSteps, n - 1) positions inwards
      chord[b]           last entry - first entry
      pathLength[b]      `pathLengths`: sum over the classes 0 .. 6 of stepCounts w_c, plus the two jump lengths
      entryRadius        dist at every entry of ``graph.coords``
      nodeRadius         dist at the representative;  incidentBranch / incidentEnd[v]: the three branches that end at a node with
                         exactly three ends of three distinct branches, ascending, and which end (0 first, 1 last); else -1
      pathDistance       with roots: D(root) = 0, D(v) = min over branches b between u != v of fl(D(u) + pathLength[b]); inf unreached
      parentBranch       the smallest b with fl(D(u) + pathLength[b]) == D(v), D(u) < D(v); -1 at roots and unreached nodes
      depthLevel, depthVoxel   0 at the roots, + 1 / + (n_b - 1) along parentBranch, -1 unreached; branchLevel[b]: the larger
                         depthLevel of its ends, -1 where either is unreached
    Derived here (`deriveMorphometry`):
      eculideanLength = |chord * spacing| (sic, the reference's spelling); tortuosity = pathLength / eculideanLength (inf for a closed
      branch); voxelLength = n; meanRadius = radiusSum / radiusCount; sigma = sqrt(radiusDevSq / radiusCount) (np.std's population
      form); a branch of TWO entries takes the reference's rule instead (`_two_entry_radii`: the mean over its two ends of the mean
      meanRadius of the other branches there) and has sigma NaN, the raw radius outputs staying what the kernel sampled; aspectRatio =
      pathLength / meanRadius; type: 0 terminating (an end is an end point), 1 bifurcating, -1 a closed curve without a node
      (graphRelated.py:81-84).
    The bifurcation table covers the nodes with incident branches whose three branches have n >= 3 (bifurcationNode: node index;
    bifurcationBranches: child, child, parent).  The parent is the node's parentBranch when that is one of the three, the children
    then ascend by branch index; otherwise, with the unit local directions u0, u1, u2 in ascending branch index, the first maximum
    of u0.u1, u1.u2, u2.u0 names the children - orders [0, 1, 2], [1, 2, 0], [2, 0, 1], the third being the parent
    (graphRelated.py:190-207).  THE LOCAL DIRECTION IS THE CHORD endDir * spacing OVER localSteps VOXELS, NOT THE REFERENCE'S
    WEIGHTED SPLINE DERIVATIVE - UNLESS ``localDirection='spline'``: then it is the unit tangent of `branchSplines` at the branch's
    first entry for end 0 and minus the tangent at its last entry for end 1 (both point into the branch), `splines` being a
    `BranchSplines` of this graph (default ``branchSplines(graph, spacing=spacing)``: end weight 20, as the reference weights the
    ends for this purpose).  That is a smoothing-spline derivative of our own definition, not FITPACK's; ``'chord'``, the default,
    returns what it always did.  The remote direction runs from the node's representative to the far end of the branch.
    local / remoteBifurcationAmplitude: the angle between the children's directions, degrees, from the clipped cosine;
    local / remoteBifurcationTilt: the angle between the children's half-angle vector (sum of the unit directions) and minus the
    parent's local direction, NaN when that vector's norm is <= 1e-4; cubicLawResult = (r1^3 + r2^3) / r3^3, squareLawResult
    likewise, min / maxRadiusRatio = min / max(r1, r2) / r3, lengthRatio = min(l1, l2) / l3 with the branches' meanRadius and
    pathLength; normalVector = the unit cross product of the children's local directions.  localBifurcationTorque (per branch
    whose two ends are both in the table, else NaN): the angle between the two normals, folded to at most 90 degrees."""
    if int(localSteps) < 1:
        raise ValueError('localSteps must be at least 1')
    if localDirection not in ('chord', 'spline'):
        raise ValueError('localDirection is \'chord\' or \'spline\'')
    on_device = _G._on_device(graph.offsets)
    shape = tuple(int(k) for k in graph.skeleton.shape)
    if dist is None:
        if vesselVolumeMask is None:
            raise ValueError('dist or vesselVolumeMask is needed')
        dist = _G.distance_transform_edt(vesselVolumeMask, device=device)
    if tuple(dist.shape) != shape:
        raise ValueError('dist and the graph\'s skeleton must have the same shape')
    h = np.ones(3, np.float64) if spacing is None else np.ascontiguousarray(np.asarray(spacing, np.float64).reshape(3))
    root_ix = _root_indices(roots, graph.nodeCoords)
    n1, n2 = shape[1], shape[2]
    B, N, R = int(graph.offsets.shape[0]) - 1, int(graph.nodeCoords.shape[0]), len(root_ix)
    if on_device:
        import torch
        tdev = graph.offsets.device
        dev = _G._dev_index(graph.offsets)
        dist = (dist if _G._on_device(dist) else torch.as_tensor(np.asarray(dist), device=tdev)).to(torch.float64).contiguous()
        lin = lambda c: ((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2]).to(torch.int64).contiguous()
        off, ends = graph.offsets.to(torch.int64).contiguous(), graph.branchEnds.to(torch.int64).contiguous()
        rt = torch.as_tensor(root_ix, device=tdev)
        alloc = lambda shp, dt: torch.empty(shp, dtype=torch.int64 if dt is np.int64 else torch.float64, device=tdev)
        ptr = lambda a: a.data_ptr() if a.numel() else None
        host = lambda a: a.cpu().numpy()
        torch.cuda.synchronize(tdev)
    else:
        dev = device
        dist = np.ascontiguousarray(dist.cpu().numpy() if _G._on_device(dist) else dist, dtype=np.float64)
        lin = lambda c: np.ascontiguousarray((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2], dtype=np.int64)
        off, ends = np.ascontiguousarray(graph.offsets, dtype=np.int64), np.ascontiguousarray(graph.branchEnds, dtype=np.int64)
        rt = root_ix
        alloc = lambda shp, dt: np.empty(shp, dt)
        ptr = lambda a: a.ctypes.data if a.size else None
        host = lambda a: a
    vox, nodevox = lin(graph.coords.reshape(-1, 3)), lin(graph.nodeCoords.reshape(-1, 3))
    bi, bf = alloc((B, _MOR_INT), np.int64), alloc((B, _MOR_F64), np.float64)
    radius, incident = alloc((N,), np.float64), alloc((N, 3), np.int64)
    entry = alloc((int(vox.shape[0]),), np.float64)
    distance, depth, level = (alloc((N,), np.float64), alloc((N, 3), np.int64), alloc((B,), np.int64)) if R else (None, None, None)
    counts = np.zeros(2, np.int64)
    _G._check(_skeleton_lib().vmask_morphometry(dev, *shape, dist.data_ptr() if on_device else dist.ctypes.data, ptr(off) if B else None, B, ptr(vox), ptr(ends),
                                    ptr(nodevox), N, h.ctypes.data, ptr(rt) if R else None, R, int(localSteps), ptr(bi), ptr(bf), ptr(radius), ptr(incident), ptr(entry),
                                    ptr(distance) if R else None, ptr(depth) if R else None, ptr(level) if R else None, counts.ctypes.data))
    raw = {'stepCounts': bi[:, 0:7], 'jumps': bi[:, 7], 'jumpOffset': bi[:, 8:14].reshape(B, 2, 3), 'radiusCount': bi[:, 14],
           'endDir': bi[:, 15:21].reshape(B, 2, 3), 'chord': bi[:, 21:24], 'radiusSum': bf[:, 0], 'radiusDevSq': bf[:, 1], 'radiusMin': bf[:, 2],
           'radiusMax': bf[:, 3], 'pathLength': bf[:, 4], 'nodeRadius': radius, 'entryRadius': entry,
           'incidentBranch': incident >> 1, 'incidentEnd': (incident & 1) - 2 * (incident < 0)}      # (-1 stays -1 in both)
    if R:
        raw.update(pathDistance=distance, parentBranch=depth[:, 0], depthLevel=depth[:, 1], depthVoxel=depth[:, 2], branchLevel=level)
    hraw = {k: np.ascontiguousarray(host(v)) for k, v in raw.items()}
    interior = interiorJumps(hraw['jumps'], hraw['jumpOffset'])
    if info is not None:
        info['depthRounds'], info['levelRounds'], info['interiorJumps'] = int(counts[0]), int(counts[1]), int(interior.sum())
    if interior.any():
        k = int(np.flatnonzero(interior)[0])
        raise ValueError('branch {} has {} pairs of consecutive entries inside it that are no 26-neighbours ({} such pairs in the table): pathLength leaves '
                         'them out, so the table is refused'.format(k, int(interior[k]), int(interior.sum())))
    if localDirection == 'spline':
        if splines is None:
            splines = branchSplines(graph, spacing=spacing, device=device)
        tangent = splines.tangent
        tangent = np.asarray(tangent.cpu().numpy() if _G._on_device(tangent) else tangent, np.float64).reshape(-1, 3)
        if len(tangent) != int(vox.shape[0]):
            raise ValueError('splines does not belong to this graph: {} entries, the graph has {}'.format(len(tangent), int(vox.shape[0])))
        hoff = host(off)
        hraw = dict(hraw, localDirection=np.stack([tangent[hoff[:-1]], -tangent[hoff[1:] - 1]], axis=1).reshape(B, 2, 3))
    derived = deriveMorphometry(hraw, host(off), host(ends), host(graph.nodeKind), h)
    result = BranchMorphometry()
    result.localDirection = localDirection
    for k in MORPHOMETRY_DEPTH:
        setattr(result, k, None)
    for k, v in raw.items():
        setattr(result, k, v.contiguous() if on_device else hraw[k])
    for k, v in derived.items():
        setattr(result, k, torch.as_tensor(v, device=tdev) if on_device else v)
    result.spacing, result.localSteps, result.roots, result.depthRounds = h, int(localSteps), root_ix, int(counts[0])
    return result


def _plain(x):
    """A numpy scalar or array as plain Python numbers and lists."""
    return x.tolist() if hasattr(x, 'tolist') else x


def writeSplines(splines, baseFolder):
    """``branchSplines.npz`` for a host `BranchSplines`: every array of ``splines.names()``, ``names``, ``spacing``, ``endWeight``,
    ``residualPerPoint``, ``sampleStep`` and ``fixedSmoothing`` (NaN in search mode); returns the file's name."""
    s = splines
    np.savez_compressed(os.path.join(baseFolder, SPLINE_FILE), names=np.array(s.names()), spacing=s.spacing, endWeight=np.float64(s.endWeight),
                        residualPerPoint=np.float64(s.residualPerPoint), sampleStep=np.float64(s.sampleStep),
                        fixedSmoothing=np.float64(np.nan if s.fixedSmoothing is None else s.fixedSmoothing), **{k: getattr(s, k) for k in s.names()})
    return SPLINE_FILE


def writeMorphometry(graph, measured, baseFolder, parts=None, splines=None):
    """The files of ``main(..., morphometry=True)`` for a host `BranchGraph` and its `BranchMorphometry`; returns their names.
    ``branchMorphometry.npz``: every array of ``measured.names()``, ``names``, ``spacing``, ``localSteps``, ``roots``.
    ``graphRepresentationWithEdgeInfo.graphml``: the graph of `writeGraphml` with the edge attributes pathLength, eculideanLength,
    tortuosity, voxelLength, meanRadius, sigma (not for a branch of two entries) and segmentIndex of the edge's branch, the node attribute radius at every voxel of a
    branch, and depthVoxel / depthLevel / pathDistance at the reached node representatives.
    ``segmentInfoDict.pkl`` (keyed by branch index, closed branches left out as graphRelated.py:64 does) and ``nodeInfoDict.pkl``
    (keyed by coordinate tuple: every node representative) with the reference's key names and plain Python values, pickle
    protocol 2: per entry the keys that `calculateProperty` writes and no others - a branch of two entries has no ``sigma``, and
    ``segmentLevel`` comes from a partition alone.  With `parts` (a `Compartments` of host arrays) the entries of owned branches and
    nodes gain ``partitionName``, and the segments ``segmentLevel`` - the partition's, as graphRelated.py:72-74,108-110 reads them.
    With `splines` (a host `BranchSplines` of this graph) every segment's entry gains ``maxCurvature``, ``meanCurvature`` and
    ``splineLength``, and the first two again under ``maxCurvatureAveragedInmm`` / ``meanCurvatureAveragedInmm``, the names the
    reference's plotting code reads - here PER BRANCH and in 1 / unit of the spacing, where the reference averages over its
    root-to-terminal path fits.  Without `splines` the files are byte for byte what they were."""
    import pickle
    m = measured
    names = m.names()
    np.savez_compressed(os.path.join(baseFolder, MORPHOMETRY_FILE), names=np.array(names), spacing=m.spacing, localSteps=np.int64(m.localSteps),
                        roots=m.roots, depthRounds=np.int64(m.depthRounds), **{k: getattr(m, k) for k in names})
    off = np.asarray(graph.offsets, np.int64)
    B = len(off) - 1
    ids = np.array([str(tuple(p)) for p in np.asarray(graph.coords).tolist()], dtype=object)
    node_ids = [str(tuple(p)) for p in np.asarray(graph.nodeCoords).tolist()]
    reached = m.depthLevel is not None
    edge_keys = ('pathLength', 'eculideanLength', 'tortuosity', 'voxelLength', 'meanRadius', 'sigma')
    columns = [_plain(getattr(m, k)) for k in edge_keys]
    radius = dict(zip(ids.tolist(), m.entryRadius.tolist()))              # (a voxel in several branches has one radius)
    depth = {}
    if reached:
        for v in np.flatnonzero(m.depthLevel >= 0).tolist():
            depth[node_ids[v]] = (int(m.depthVoxel[v]), int(m.depthLevel[v]), float(m.pathDistance[v]))
    edges = {}
    for k in range(B):
        seg = ids[off[k]:off[k + 1]].tolist()
        for a, b in zip(seg[:-1], seg[1:]):
            key = (a, b) if (b, a) not in edges else (b, a)               # (an undirected graph keeps one edge per pair: the last index wins)
            edges[key] = k
    with open(os.path.join(baseFolder, EDGE_INFO_GRAPH_FILE), 'w', encoding='utf-8') as f:
        f.write('<?xml version=\'1.0\' encoding=\'utf-8\'?>\n')
        f.write('<graphml xmlns="http://graphml.graphdrawing.org/xmlns" xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
                'xsi:schemaLocation="http://graphml.graphdrawing.org/xmlns http://graphml.graphdrawing.org/xmlns/1.0/graphml.xsd">\n')
        f.write('  <key id="d0" for="edge" attr.name="segmentIndex" attr.type="long" />\n')
        for i, k in enumerate(edge_keys):
            f.write('  <key id="d{}" for="edge" attr.name="{}" attr.type="{}" />\n'.format(i + 1, k, 'long' if k == 'voxelLength' else 'double'))
        f.write('  <key id="d7" for="node" attr.name="radius" attr.type="double" />\n')
        f.write('  <key id="d8" for="node" attr.name="depthVoxel" attr.type="long" />\n  <key id="d9" for="node" attr.name="depthLevel" attr.type="long" />\n')
        f.write('  <key id="d10" for="node" attr.name="pathDistance" attr.type="double" />\n')
        f.write('  <graph edgedefault="undirected">\n')
        for a, r in radius.items():
            f.write('    <node id="{}">\n      <data key="d7">{!r}</data>\n'.format(a, r))
            if a in depth:
                f.write('      <data key="d8">{}</data>\n      <data key="d9">{}</data>\n      <data key="d10">{!r}</data>\n'.format(*depth[a]))
            f.write('    </node>\n')
        for (a, b), k in edges.items():
            f.write('    <edge source="{}" target="{}">\n      <data key="d0">{}</data>\n'.format(a, b, k))
            for i, col in enumerate(columns):
                if edge_keys[i] != 'sigma' or off[k + 1] - off[k] != 2:
                    f.write('      <data key="d{}">{!r}</data>\n'.format(i + 1, col[k]))
            f.write('    </edge>\n')
        f.write('  </graph>\n</graphml>\n')
    ends = np.asarray(graph.branchEnds, np.int64).reshape(-1, 2)
    segment_info = {}
    for k in range(B):
        if ends[k, 0] < 0 or (ends[k, 0] == ends[k, 1]):                  # (same head and tail)
            continue
        d = {key: col[k] for key, col in zip(edge_keys, columns) if key != 'sigma' or off[k + 1] - off[k] != 2}      # (no sigma for two entries)
        d['aspectRatio'] = float(m.aspectRatio[k])
        d['type'] = 'terminating' if m.type[k] == 0 else 'bifurcating'
        if not np.isnan(m.localBifurcationTorque[k]):
            d['localBifurcationTorque'] = float(m.localBifurcationTorque[k])
        if parts is not None and parts.branchCompartment[k]:
            d['partitionName'], d['segmentLevel'] = parts.names[int(parts.branchCompartment[k]) - 1], int(parts.branchLevel[k])
        if splines is not None:
            d['maxCurvature'], d['meanCurvature'], d['splineLength'] = (float(getattr(splines, key)[k]) for key in ('maxCurvature', 'meanCurvature', 'splineLength'))
            d['maxCurvatureAveragedInmm'], d['meanCurvatureAveragedInmm'] = d['maxCurvature'], d['meanCurvature']
        segment_info[k] = d
    node_info = {}
    kinds, degrees = _plain(graph.nodeKind), _plain(graph.nodeDegree)
    for v, c in enumerate(np.asarray(graph.nodeCoords).tolist()):
        d = {'radius': float(m.nodeRadius[v])}
        if kinds[v] == 0:
            d['type'] = 'terminating'
        elif degrees[v] >= 3:
            d['type'] = 'bifurcating'
        if node_ids[v] in depth:
            d['depthVoxel'], d['depthLevel'], d['pathDistance'] = depth[node_ids[v]]
        if parts is not None and parts.nodeCompartment[v]:
            d['partitionName'] = parts.names[int(parts.nodeCompartment[v]) - 1]
        node_info[tuple(c)] = d
    for row, v in enumerate(_plain(m.bifurcationNode)):
        d = node_info[tuple(np.asarray(graph.nodeCoords)[v].tolist())]
        for key in ('localBifurcationAmplitude', 'remoteBifurcationAmplitude', 'localBifurcationTilt', 'remoteBifurcationTilt', 'cubicLawResult',
                    'squareLawResult', 'minRadiusRatio', 'maxRadiusRatio', 'lengthRatio'):
            x = float(getattr(m, key)[row])
            if not np.isnan(x):                                           # (an absent tilt is an absent key, as in the reference)
                d[key] = x
        r = [float(m.meanRadius[b]) for b in _plain(m.bifurcationBranches[row])]
        d['radiusList'], d['minRadius'] = r, min(r)
        d['normalVector'] = _plain(m.normalVector[row])
    for name, obj in ((SEGMENT_INFO_FILE, segment_info), (NODE_INFO_FILE, node_info)):
        with open(os.path.join(baseFolder, name), 'wb') as f:
            pickle.dump(obj, f, protocol=2)
    return [MORPHOMETRY_FILE, EDGE_INFO_GRAPH_FILE, SEGMENT_INFO_FILE, NODE_INFO_FILE]


PARTITION_FILE = 'partitionInfo.pkl'
COMPARTMENT_FILE = 'compartments.npz'
COMPARTMENT_LABEL_FILE = 'compartmentLabels.nii.gz'
COMPARTMENT_ARRAYS = ('entryCompartment', 'entryDepth', 'entryLevel', 'nodeCompartment', 'nodeDepth', 'nodeLevel', 'branchCompartment', 'branchLevel',
                      'compartmentCounts')


class Compartments:
    """What `partitionCompartments` returns: ``names`` (labels 1 .. K in this order) and one attribute per name of
    `COMPARTMENT_ARRAYS` - per entry of ``graph.coords``, per node and per branch the owning compartment (uint8, 0: none) and the
    depth and level in it (int64, -1 without an owner); ``compartmentCounts`` (int64, (K + 1) x 3: vertices owned, vertices
    reached, branches; row 0: owned by none, reached by two or more, the remaining branches).  ``nodeKind`` is the graph's (host),
    ``depthRounds`` / ``levelRounds`` describe the run."""

    def __init__(self, names, nodeKind, **arrays):
        self.names, self.nodeKind = list(names), nodeKind
        for k in COMPARTMENT_ARRAYS:
            setattr(self, k, arrays[k])

    def partitionInfo(self, graph):
        """The reference's ``partitionInfo`` (partitionCompartmentGUIDetail.py:316-343): ``{name: {'visitedVoxels': [tuples],
        'segmentIndexList': [ints]}}``.  ``visitedVoxels`` holds the voxels of the vertices the compartment owns, every vertex once,
        ascending by depth and then by the index of its first entry; ``segmentIndexList`` the branches that belong to it, ascending."""
        host = lambda a: np.asarray(a.cpu() if _G._on_device(a) else a)
        off, ends = host(graph.offsets).astype(np.int64), host(graph.branchEnds).astype(np.int64).reshape(-1, 2)
        coords = host(graph.coords).reshape(-1, 3)
        comp, depth, bcomp = host(self.entryCompartment), host(self.entryDepth), host(self.branchCompartment)
        E = len(comp)
        # one entry per vertex: the first at which it occurs (a node at several branch ends, a closed branch's vertex at both of its ends)
        vertex = np.arange(E, dtype=np.int64)
        if len(off) > 1:
            first, last = off[:-1], off[1:] - 1
            is_open = ends[:, 0] >= 0
            vertex[first[is_open]], vertex[last[is_open]] = E + ends[is_open, 0], E + ends[is_open, 1]
            vertex[last[~is_open]] = first[~is_open]
        _, once = np.unique(vertex, return_index=True)                    # (the first occurrence of every vertex)
        info = {}
        for k, name in enumerate(self.names):
            mine = once[comp[once] == k + 1]
            mine = mine[np.lexsort((mine, depth[mine]))]
            info[name] = {'visitedVoxels': [tuple(c) for c in coords[mine].tolist()], 'segmentIndexList': np.flatnonzero(bcomp == k + 1).tolist()}
        return info


def _compartment_lists(graph, compartments):
    """``(names, [(initial indices, boundary indices), ..])`` as C-order linear indices from either form of `compartments`."""
    if isinstance(compartments, dict):
        names = [str(k) for k in compartments]
        pairs = [(v['initialVoxels'], v['boundaryVoxels']) for v in compartments.values()]
    else:
        pairs = [tuple(pr) for pr in compartments]
        if any(len(pr) != 2 for pr in pairs):
            raise ValueError('compartments: a dict in the layout of chosenVoxelsForPartition.pkl or a sequence of (initial, boundary) pairs')
        names = [str(k + 1) for k in range(len(pairs))]
    if not 1 <= len(pairs) <= 255:
        raise ValueError('1 to 255 compartments, not {}'.format(len(pairs)))
    host = lambda a: np.asarray(a.cpu() if _G._on_device(a) else a)
    shape = tuple(int(k) for k in graph.skeleton.shape)
    nc = host(graph.nodeCoords).astype(np.int64).reshape(-1, 3)
    lin = lambda c: (c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2]
    vertices = set(lin(host(graph.coords).astype(np.int64).reshape(-1, 3)).tolist()) | set(lin(nc).tolist())
    skeleton = None

    def index_of(item):
        nonlocal skeleton
        if np.ndim(item) == 0:
            k = int(item)
            if not 0 <= k < len(nc):
                raise ValueError('{} is no node index (the graph has {} nodes)'.format(k, len(nc)))
            return int(lin(nc[k:k + 1])[0])
        if len(item) != 3:
            raise ValueError('a listed voxel is a node index or a coordinate triple')
        c = tuple(int(x) for x in item)
        if not all(0 <= x < n for x, n in zip(c, shape)):
            raise ValueError('voxel {} lies outside the volume {}'.format(c, shape))
        v = (c[0] * shape[1] + c[1]) * shape[2] + c[2]
        if v not in vertices:
            if skeleton is None:
                skeleton = host(graph.skeleton)
            if skeleton[c]:
                raise ValueError('voxel {} is a skeleton voxel but no entry of the branch table: a member of a junction cluster other '
                                 'than its representative, or an isolated voxel'.format(c))
            raise ValueError('voxel {} is no voxel of the centre line'.format(c))
        return v
    as_items = lambda x: list(x.tolist() if hasattr(x, 'tolist') else x)
    return names, [(np.array([index_of(i) for i in as_items(a)], np.int64), np.array([index_of(i) for i in as_items(b)], np.int64)) for a, b in pairs]


def partitionCompartments(graph, compartments, device=0, info=None):
    """The compartment partition of a `BranchGraph` (``vmask_compartments``, DESIGN.md section 9, "f12 compartments") as a
    `Compartments`.  `compartments`: the reference's ``chosenVoxelsForPartition.pkl`` layout ``{name: {'initialVoxels': [..],
    'boundaryVoxels': [..]}}`` - insertion order gives the labels 1 .. K - or a sequence of ``(initial, boundary)`` pairs, named
    '1' .. 'K'; an item is a coordinate triple or a scalar node index (as `branchMorphometry`'s roots).  ``ValueError`` for a
    coordinate that is the voxel of no vertex.
    The vertices are the nodes, the interior entries of the branches and one vertex per closed branch; consecutive entries are
    joined.  Compartment c reaches what a path from one of its initial vertices reaches without a vertex on one of its boundary
    voxels; depth = the fewest edges of such a path (the reference's depthVoxel), level = 0 at the initial vertices and, elsewhere,
    the smallest level of a neighbour one edge nearer, plus one at a node (depthLevel on trees).  A vertex belongs to the
    compartment of smallest (depth, label) that reaches it, a branch to the compartment that owns every one of its entries
    (segmentIndexList on trees), its level being the smallest of its entries' (segmentLevel).
    A host graph gives host arrays, a graph of tensors on the GPU gives tensors on the same device.  `info`, when a dict,
    receives ``depthRounds`` and ``levelRounds``."""
    names, lists = _compartment_lists(graph, compartments)
    K = len(lists)
    on_device = _G._on_device(graph.offsets)
    shape = tuple(int(k) for k in graph.skeleton.shape)
    n1, n2 = shape[1], shape[2]
    B, N = int(graph.offsets.shape[0]) - 1, int(graph.nodeCoords.shape[0])
    ioff = np.concatenate(([0], np.cumsum([len(a) for a, _ in lists]))).astype(np.int64)
    boff = np.concatenate(([0], np.cumsum([len(b) for _, b in lists]))).astype(np.int64)
    ivox = np.ascontiguousarray(np.concatenate([a for a, _ in lists]), dtype=np.int64)
    bvox = np.ascontiguousarray(np.concatenate([b for _, b in lists]), dtype=np.int64)
    if on_device:
        import torch
        tdev = graph.offsets.device
        dev = _G._dev_index(graph.offsets)
        lin = lambda c: ((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2]).to(torch.int64).contiguous()
        off, ends = graph.offsets.to(torch.int64).contiguous(), graph.branchEnds.to(torch.int64).contiguous()
        alloc = lambda shp, dt: torch.empty(shp, dtype=torch.uint8 if dt is np.uint8 else torch.int64, device=tdev)
        ptr = lambda a: a.data_ptr() if a.numel() else None
        kind = graph.nodeKind.cpu().numpy()
        torch.cuda.synchronize(tdev)
    else:
        dev = device
        lin = lambda c: np.ascontiguousarray((c[:, 0] * n1 + c[:, 1]) * n2 + c[:, 2], dtype=np.int64)
        off, ends = np.ascontiguousarray(graph.offsets, dtype=np.int64), np.ascontiguousarray(graph.branchEnds, dtype=np.int64)
        alloc = lambda shp, dt: np.empty(shp, dt)
        ptr = lambda a: a.ctypes.data if a.size else None
        kind = np.asarray(graph.nodeKind)
    vox, nodevox = lin(graph.coords.reshape(-1, 3)), lin(graph.nodeCoords.reshape(-1, 3))
    E = int(vox.shape[0])
    out = {'entryCompartment': alloc((E,), np.uint8), 'entryDepth': alloc((E,), np.int64), 'entryLevel': alloc((E,), np.int64),
           'nodeCompartment': alloc((N,), np.uint8), 'nodeDepth': alloc((N,), np.int64), 'nodeLevel': alloc((N,), np.int64),
           'branchCompartment': alloc((B,), np.uint8), 'branchLevel': alloc((B,), np.int64), 'compartmentCounts': alloc((K + 1, 3), np.int64)}
    counts = np.zeros(2, np.int64)
    _G._check(_skeleton_lib().vmask_compartments(dev, *shape, ptr(off) if B else None, B, ptr(vox), ptr(ends), ptr(nodevox), N, K, ioff.ctypes.data,
                                                 ivox.ctypes.data if ivox.size else None, boff.ctypes.data, bvox.ctypes.data if bvox.size else None,
                                                 *(ptr(out[k]) for k in COMPARTMENT_ARRAYS[:8]), out['compartmentCounts'].data_ptr() if on_device else
                                                 out['compartmentCounts'].ctypes.data, counts.ctypes.data))
    parts = Compartments(names, kind, **out)
    parts.depthRounds, parts.levelRounds = int(counts[0]), int(counts[1])
    if info is not None:
        info['depthRounds'], info['levelRounds'] = int(counts[0]), int(counts[1])
    return parts


def compartmentTerritories(vesselVolumeMask, graph, parts, spacing=None, device=0, info=None, return_distance=False):
    """The compartments carried back to the voxels: ``labels`` (uint8, the mask's shape) and ``sizes`` (int64, K + 1).  The seeds
    are the entries of ``graph.coords`` that a compartment owns and that lie in the mask, labelled by their owner; a voxel with
    ``vesselVolumeMask != 0`` gets the label of the seed at the smallest path length inside the mask (`geodesic.geodesicDistance`
    with these seeds: steps in `spacing`, ties to the smallest label), 0 outside the mask and where no seed is reached.
    ``sizes.sum()`` is the mask's voxel count.  ``return_distance=True`` adds ``distance`` (float64).  A mask tensor on the GPU gives
    tensors on the same device.  `info`, when a dict, receives the counts of `geodesic.geodesicDistance`."""
    on_device = _G._on_device(vesselVolumeMask)
    K = len(parts.names)
    if on_device:
        import torch
        m = _G._u8t(vesselVolumeMask)
        as_t = lambda a: a if _G._on_device(a) else torch.as_tensor(np.asarray(a), device=m.device)
        co, lab = as_t(graph.coords).to(torch.int64).reshape(-1, 3), as_t(parts.entryCompartment).to(torch.int32)
    else:
        m = _G._u8c(vesselVolumeMask)
        host = lambda a: np.asarray(a.cpu() if _G._on_device(a) else a)
        co, lab = host(graph.coords).astype(np.int64).reshape(-1, 3), host(parts.entryCompartment).astype(np.int32)
    if tuple(m.shape) != tuple(int(k) for k in graph.skeleton.shape):
        raise ValueError('the graph\'s skeleton and vesselVolumeMask must have the same shape')
    vox = (co[:, 0] * int(m.shape[1]) + co[:, 1]) * int(m.shape[2]) + co[:, 2]
    keep = (lab > 0) & (m.reshape(-1)[vox] != 0)
    vox, lab = vox[keep], lab[keep]
    if on_device:
        vox, lab = vox.contiguous(), lab.contiguous()
    else:
        vox, lab = np.ascontiguousarray(vox), np.ascontiguousarray(lab)
    distance, labels, sizes = _geo._run(m, vox, lab, K, spacing, device, return_distance, True, info)
    labels = labels.to(torch.uint8) if on_device else labels.astype(np.uint8)
    return (labels, sizes, distance) if return_distance else (labels, sizes)


def compartmentSummary(parts, measured=None, sizes=None, affine=None):
    """Per compartment name a dict: ``branches`` (the branches that belong to it), ``terminalNodes`` (the end points it owns) and
    ``maxLevel`` (the largest ``branchLevel`` of its branches, -1 without one); with a `BranchMorphometry` ``totalLength``
    (``math.fsum`` of ``pathLength`` over its branches: exactly rounded, whatever the order) and ``meanRadius`` (the mean of the
    branches' ``meanRadius``, NaN without a branch); with `sizes` (of `compartmentTerritories`) and `affine` ``volume``
    (`territoryVolumes`)."""
    import math
    host = lambda a: np.asarray(a.cpu() if _G._on_device(a) else a)
    bcomp, blevel, ncomp, kind = host(parts.branchCompartment), host(parts.branchLevel), host(parts.nodeCompartment), np.asarray(parts.nodeKind)
    volumes = territoryVolumes(host(sizes), affine if affine is not None else np.eye(4)) if sizes is not None else None
    out = {}
    for k, name in enumerate(parts.names):
        mine = np.flatnonzero(bcomp == k + 1)
        d = {'branches': int(len(mine)), 'terminalNodes': int(np.count_nonzero((ncomp == k + 1) & (kind == 0))),
             'maxLevel': int(blevel[mine].max()) if len(mine) else -1}
        if measured is not None:
            d['totalLength'] = math.fsum(host(measured.pathLength)[mine].tolist())
            d['meanRadius'] = float(np.mean(host(measured.meanRadius)[mine])) if len(mine) else float('nan')
        if volumes is not None:
            d['volume'] = float(volumes[k + 1])
        out[name] = d
    return out


def writeCompartments(graph, parts, baseFolder, measured=None, sizes=None, affine=None):
    """``partitionInfo.pkl`` (`Compartments.partitionInfo`, pickle protocol 2) and ``compartments.npz``: ``names``, every array of
    `COMPARTMENT_ARRAYS`, the columns of `compartmentSummary` as ``summary_<key>`` (one value per compartment) and, with `sizes`,
    ``sizes`` and ``volumes``; returns the two file names."""
    import pickle
    with open(os.path.join(baseFolder, PARTITION_FILE), 'wb') as f:
        pickle.dump(parts.partitionInfo(graph), f, protocol=2)
    summary = compartmentSummary(parts, measured, sizes, affine)
    keys = list(summary[parts.names[0]])
    extra = {'summary_' + k: np.array([summary[n][k] for n in parts.names]) for k in keys}
    if sizes is not None:
        extra.update(sizes=np.asarray(sizes), volumes=territoryVolumes(sizes, affine))
    np.savez_compressed(os.path.join(baseFolder, COMPARTMENT_FILE), names=np.array(parts.names), **{k: getattr(parts, k) for k in COMPARTMENT_ARRAYS}, **extra)
    return [PARTITION_FILE, COMPARTMENT_FILE]


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


def flowOnGraph(graph, measured, spacing, pressureIn, slope, c, k=1.852, metresPerUnit=1e-3, factor=0.8, inlet=None, tol=1e-10, maxIter=50, device=0):
    """The flow solve of ``main(..., flow=...)`` on a host `BranchGraph` and its `BranchMorphometry` (measured with roots).
    Fixed nodes: `inlet` (node indices or coordinate triples; default: the roots) at `pressureIn`, every reached end point at
    ``terminalPressures(pathDistance * metresPerUnit, pressureIn, slope, factor)``.  Resistances: ``branchResistance`` ('HW', `c`,
    `k`) of the length ``pathLength * metresPerUnit`` and the radius ``meanRadius * voxel * metresPerUnit`` - the distance
    transform is in voxels and ignores the spacing, so a `spacing` that is not isotropic to 1e-6 relative is a ``ValueError``, not
    a guess.  Returns ``(FlowResult, extra)``; `extra` holds ``velocity`` (flow / (pi r^2), per branch), ``resistance``,
    ``fixed``, ``fixedPressure``, ``radius`` and ``length``."""
    from . import flow as F
    h = np.asarray(spacing, np.float64).reshape(3)
    if not (h.max() - h.min()) <= 1e-6 * h.min():
        raise ValueError('flow needs an isotropic spacing (the radii are in voxels): got {}'.format(h.tolist()))
    if measured.depthLevel is None:
        raise ValueError('flow needs a morphometry measured with roots')
    inlets = measured.roots if inlet is None else _root_indices(inlet, graph.nodeCoords)
    if not len(inlets):
        raise ValueError('flow needs at least one inlet')
    N = int(graph.nodeCoords.shape[0])
    fixed = (np.asarray(graph.nodeKind) == 0) & (np.asarray(measured.depthLevel) >= 0)
    distance = np.where(fixed, measured.pathDistance, 0.0)
    pressure = F.terminalPressures(distance * float(metresPerUnit), pressureIn, slope, factor)
    fixed[inlets] = True
    pressure[inlets] = float(pressureIn)
    length = np.asarray(measured.pathLength, np.float64) * float(metresPerUnit)
    radius = np.asarray(measured.meanRadius, np.float64) * (float(h[0]) * float(metresPerUnit))
    R = F.branchResistance(length, radius, law='HW', c=c, k=k)
    result = F.simulateFlow(graph, R, fixed, pressure, k=k, tol=tol, maxIter=maxIter, device=device)
    with np.errstate(divide='ignore', invalid='ignore'):
        velocity = result.flow[0] / (np.pi * radius ** 2)
    return result, {'velocity': velocity, 'resistance': R, 'fixed': fixed, 'fixedPressure': pressure, 'radius': radius, 'length': length}


def _add_simulation_data(graph, result, extra, baseFolder):
    """``simulationData`` into the entries of ``segmentInfoDict.pkl`` (velocity, flow) and ``nodeInfoDict.pkl`` (pressure), as the
    reference's updateNetworkWithSimulationResult leaves them; nodes of a component without a fixed node get none."""
    import pickle
    for name in (SEGMENT_INFO_FILE, NODE_INFO_FILE):
        path = os.path.join(baseFolder, name)
        with open(path, 'rb') as f:
            info = pickle.load(f)
        if name == SEGMENT_INFO_FILE:
            for k, d in info.items():
                d['simulationData'] = {'velocity': float(extra['velocity'][k]), 'flow': float(result.flow[0, k])}
        else:
            for v, c in enumerate(np.asarray(graph.nodeCoords).tolist()):
                if not np.isnan(result.pressure[0, v]):
                    info[tuple(c)]['simulationData'] = {'pressure': float(result.pressure[0, v])}
        with open(path, 'wb') as f:
            pickle.dump(info, f, protocol=2)


def main(baseFolder=None, segments=False, territories=False, geodesic=False, prune=None, morphometry=False, roots=None, compartments=None, flow=None,
         curvature=False, tubes=None):
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
    ``prune=None`` writes every file as before.
    With ``morphometry=True`` as well (it needs `prune`; ``prune=(0, 0.0)`` prunes nothing) the branches are measured by
    `branchMorphometry` - `dist` being the distance transform of the mask, the spacing the norms of the affine's columns, `roots`
    node indices or coordinate triples - and `writeMorphometry` writes ``branchMorphometry.npz``,
    ``graphRepresentationWithEdgeInfo.graphml``, ``segmentInfoDict.pkl`` and ``nodeInfoDict.pkl`` beside the others; every other
    file and the returned values are those of a run without it.
    With `compartments` as well (it needs `prune`): a dict in the layout of the reference's ``chosenVoxelsForPartition.pkl``, or the
    path of such a file.  `partitionCompartments` divides the branch graph, and ``partitionInfo.pkl`` and ``compartments.npz``
    (`writeCompartments`) are written; with ``territories=True`` also ``compartmentLabels.nii.gz`` (uint8, the mask's affine:
    `compartmentTerritories` in the affine's spacing) and the territories' ``sizes`` and ``volumes`` into the npz; with
    ``morphometry=True`` the entries of ``segmentInfoDict.pkl`` / ``nodeInfoDict.pkl`` of owned branches and nodes gain
    ``partitionName``, the segments ``segmentLevel``.  The returned values are those of a run without it; without `compartments`
    every file is what it was.
    With `flow` as well (it needs ``morphometry=True`` and `roots`): a dict of `flowOnGraph`'s arguments - ``pressureIn``, ``slope``,
    ``c``, and optionally ``k``, ``metresPerUnit`` (default 1e-3: the affine is in millimetres), ``factor``, ``inlet``, ``tol``,
    ``maxIter``.  ``flowResult.npz`` (the `FlowResult` and `flowOnGraph`'s extras) is written, and the entries of
    ``segmentInfoDict.pkl`` / ``nodeInfoDict.pkl`` gain ``simulationData`` with ``velocity`` and ``flow`` / ``pressure``.  The
    returned values are those of a run without it; without `flow` every file is byte for byte what it was.
    With ``curvature=True`` as well (it needs `prune`): `branchSplines` in the affine's spacing with its defaults, written as
    ``branchSplines.npz`` (`writeSplines`); with ``morphometry=True`` the entries of ``segmentInfoDict.pkl`` gain ``maxCurvature``,
    ``meanCurvature``, ``splineLength`` and the first two under the reference's ``maxCurvatureAveragedInmm`` /
    ``meanCurvatureAveragedInmm`` (`writeMorphometry`).  The returned values are those of a run without it; without `curvature`
    every file is byte for byte what it was.
    With `tubes` as well (``True`` or a dict; it needs `prune` and ``morphometry=True``): the tube model of the branch graph
    (`tubes.graphTubes`: DESIGN.md section 9, "f21 tube model") in the affine's spacing, compared with the mask - the centre points
    being the splines' when ``curvature=True``, the voxel centres otherwise; a dict may give ``minRadius``, ``radiusScale`` and
    ``keep``.  ``vesselVolumeModel.nii.gz`` (uint8), ``branchLabelsModel.nii.gz`` (int32: branch k has label k + 1) and
    ``tubeModel.npz`` (`tubes.writeTubes`) are written, with `flow` also ``branchFlow.nii.gz`` (float32: |flow| of the branch that
    holds the voxel).  The returned values are those of a run without it; without `tubes` every file is byte for byte what it was."""
    if tubes is not None and tubes is not False and (prune is None or not morphometry):
        raise ValueError('tubes needs prune and morphometry=True (prune=(0, 0.0) prunes nothing)')
    if flow is not None and (not morphometry or roots is None):
        raise ValueError('flow needs morphometry=True and roots')
    if curvature and prune is None:
        raise ValueError('curvature=True needs prune (prune=(0, 0.0) prunes nothing)')
    if compartments is not None and prune is None:
        raise ValueError('compartments needs prune (prune=(0, 0.0) prunes nothing)')
    if morphometry and prune is None:
        raise ValueError('morphometry=True needs prune (prune=(0, 0.0) prunes nothing)')
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
    parts = measured = None
    if compartments is not None:
        if isinstance(compartments, (str, bytes, os.PathLike)):
            import pickle
            with open(compartments, 'rb') as f:
                compartments = pickle.load(f)
        parts = partitionCompartments(graph, compartments)
    extra = {}
    if curvature:
        spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
        extra['splines'] = branchSplines(graph, spacing=spacing)
        name = writeSplines(extra['splines'], baseFolder)
        print('{} saved to {}.'.format(name, os.path.join(baseFolder, name)))
    if morphometry:
        spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
        measured = branchMorphometry(graph, vesselVolumeMask=vesselVolumeMask, spacing=spacing, roots=roots)
        if parts is not None:
            extra['parts'] = parts
        for name in writeMorphometry(graph, measured, baseFolder, **extra):
            print('{} saved to {}.'.format(name, os.path.join(baseFolder, name)))
    splines = extra.get('splines')
    solved = None
    if flow is not None:
        from . import flow as _flow
        solved, extra = flowOnGraph(graph, measured, spacing, **flow)
        _add_simulation_data(graph, solved, extra, baseFolder)
        name = _flow.writeFlow(solved, baseFolder, **extra)
        print('{} saved to {}.'.format(name, os.path.join(baseFolder, name)))
    if tubes is not None and tubes is not False:
        from . import tubes as _tubes
        model = _tubes.graphTubes(graph, measured, splines=splines, spacing=spacing, mask=vesselVolumeMask, **(tubes if isinstance(tubes, dict) else {}))
        for name in _tubes.writeTubes(model, baseFolder, affine, measured=measured, flow=None if solved is None else solved.flow[0]):
            print('{} saved to {}.'.format(name, os.path.join(baseFolder, name)))
    if parts is not None:
        compartmentSizes = None
        if territories:
            spacing = np.sqrt((np.asarray(affine, dtype=np.float64)[:3, :3] ** 2).sum(axis=0))
            compartmentLabels, compartmentSizes = compartmentTerritories(vesselVolumeMask, graph, parts, spacing=spacing)
            path = os.path.join(baseFolder, COMPARTMENT_LABEL_FILE)
            saveVolume(compartmentLabels, affine, path, astype=np.uint8)
            print('{} saved to {}.'.format(COMPARTMENT_LABEL_FILE, path))
        for name in writeCompartments(graph, parts, baseFolder, measured, compartmentSizes, affine):
            print('{} saved to {}.'.format(name, os.path.join(baseFolder, name)))
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
