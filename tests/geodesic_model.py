"""Sequential model of vmask_geodesic (include/vmask.h, DESIGN.md section 9 "f9 geodesic"): a heapq Dijkstra over the mask's voxels
with float64 addition, the labels from one pass in ascending distance.  Test code only."""
import heapq
import math

import numpy as np

OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def weights(spacing=None):
    """w(delta) for the 26 offsets, in the order of OFFSETS: float64, the squares summed in the order of the axes."""
    h = (1.0, 1.0, 1.0) if spacing is None else tuple(float(x) for x in spacing)
    return [math.sqrt((a * h[0]) ** 2 + (b * h[1]) ** 2 + (c * h[2]) ** 2) for a, b, c in OFFSETS]


def _padded(mask):
    m = np.zeros(tuple(n + 2 for n in mask.shape), bool)
    m[1:-1, 1:-1, 1:-1] = np.asarray(mask) != 0
    return m


def geodesic(mask, seeds, seed_labels=None, spacing=None, max_label=None):
    """(dist float64, labels int32, sizes int64[max_label + 1]) by the definition: `seeds` are C-order linear indices of mask
    voxels, `seed_labels` (default: all 1) values >= 1, the smallest of a voxel's labels holds."""
    mask = np.asarray(mask)
    shape = mask.shape
    seeds = np.asarray(seeds, np.int64).reshape(-1)
    seed_labels = np.ones(len(seeds), np.int32) if seed_labels is None else np.asarray(seed_labels, np.int32).reshape(-1)
    assert len(seeds) == len(seed_labels) and (seed_labels >= 1).all()
    if max_label is None:
        max_label = int(seed_labels.max()) if len(seeds) else 1
    m = _padded(mask)
    p1, p2 = m.shape[1], m.shape[2]
    flat = m.ravel().tolist()
    step = [(a * p1 + b) * p2 + c for a, b, c in OFFSETS]
    w = weights(spacing)
    inf = math.inf
    D = [inf] * m.size
    lab = [0] * m.size
    i0, i1, i2 = np.unravel_index(seeds, shape)
    at = (((i0 + 1) * p1 + (i1 + 1)) * p2 + (i2 + 1)).tolist()
    heap = []
    for v, l in zip(at, seed_labels.tolist()):
        assert flat[v], 'seed outside the mask'
        if D[v] != 0.0:
            D[v] = 0.0
            heap.append((0.0, v))
        lab[v] = l if lab[v] == 0 else min(lab[v], l)
    is_seed = set(at)
    heapq.heapify(heap)
    order = []
    while heap:
        d, v = heapq.heappop(heap)
        if d > D[v]:
            continue
        order.append(v)
        for s, ws in zip(step, w):
            u = v + s
            if flat[u]:
                nd = d + ws
                if nd < D[u]:
                    D[u] = nd
                    heapq.heappush(heap, (nd, u))
    order.sort(key=D.__getitem__)                                       # (a voxel can be popped once only: d > D[v] skips the rest; ties in any order)
    for v in order:
        if v in is_seed:
            continue
        dv, best = D[v], 0
        for s, ws in zip(step, w):
            u = v + s
            if flat[u] and D[u] + ws == dv and (best == 0 or lab[u] < best):
                best = lab[u]
        lab[v] = best
    Dp = np.asarray(D, np.float64).reshape(m.shape)[1:-1, 1:-1, 1:-1]
    dist = np.where(mask != 0, Dp, -1.0)
    labels = np.asarray(lab, np.int32).reshape(m.shape)[1:-1, 1:-1, 1:-1].copy()
    sizes = np.bincount(labels[mask != 0].ravel(), minlength=max_label + 1).astype(np.int64)
    return dist, labels, sizes


def jacobi(mask, seeds, spacing=None):
    """The same distances as the least fixed point of whole-volume numpy sweeps (checks the model, not the product)."""
    mask = np.asarray(mask)
    m = _padded(mask)
    D = np.full(m.shape, np.inf)
    core = D[1:-1, 1:-1, 1:-1]
    idx = np.unravel_index(np.asarray(seeds, np.int64).reshape(-1), mask.shape)
    core[idx] = 0.0
    n0, n1, n2 = mask.shape
    inside = m[1:-1, 1:-1, 1:-1]
    w = weights(spacing)
    while True:
        best = core.copy()
        for (a, b, c), ws in zip(OFFSETS, w):
            np.minimum(best, D[1 + a:1 + a + n0, 1 + b:1 + b + n1, 1 + c:1 + c + n2] + ws, out=best)
        best[~inside] = np.inf
        if np.array_equal(best, core):
            break
        core[...] = best
    return np.where(mask != 0, core, -1.0)
