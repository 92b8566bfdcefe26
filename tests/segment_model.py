"""Sequential model of segment tracing ("f6 segment tracing"): the yardstick of tests/test_segments.py.
Plain Python / numpy, no graph library: a table of neighbours, a walk from every node along every incident edge through
voxels of degree 2, then a walk round every curve of degree-2 voxels that no node touches.

Definitions.  S = the voxels != 0 of a 3-D volume (outside the volume is background); deg(v) = voxels of S among the 26
neighbours of v; node: deg != 2; path voxel: deg == 2; isolated: deg == 0; idx(v) = C-order linear index.
  1. every pair of 26-adjacent nodes is a segment of two voxels
  2. a maximal run of path voxels p1..pk (k >= 1) is a segment [a, p1, .., pk, b] with the nodes a, b at its ends (a == b allowed)
  3. a component of path voxels only is one closed segment [m, .., m], m its voxel of smallest idx
  4. isolated voxels belong to no segment
Canonical form: idx(first) < idx(last); when first == last, idx(second) < idx(second-to-last).  Segments ascend by
(idx(first), idx(second)).
"""
import numpy as np

OFFSETS = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]   # ascending idx


def neighbour_table(volume):
    """-> (idx int64 [n] ascending, nb: list of n lists of positions into idx, ascending)."""
    obj = np.asarray(volume) != 0
    assert obj.ndim == 3
    coords = np.argwhere(obj)
    n = len(coords)
    lut = np.full(tuple(s + 2 for s in obj.shape), -1, np.int64)
    lut[1:-1, 1:-1, 1:-1][obj] = np.arange(n)
    cols = [lut[coords[:, 0] + 1 + a, coords[:, 1] + 1 + b, coords[:, 2] + 1 + c] for a, b, c in OFFSETS]
    table = np.stack(cols, axis=1) if n else np.zeros((0, 26), np.int64)
    nb = [[j for j in row if j >= 0] for row in table.tolist()]
    idx = np.ravel_multi_index(coords.T, obj.shape).astype(np.int64) if n else np.zeros(0, np.int64)
    return idx, nb


def trace(volume):
    """-> (segments: list of lists of linear indices, canonical form and order; counts: dict nodes / isolated / path)."""
    idx, nb = neighbour_table(volume)
    n = len(idx)
    deg = [len(x) for x in nb]
    visited = [False] * n
    segs = []
    for a in range(n):                                     # positions ascend with idx: comparing positions compares idx
        if deg[a] == 2:
            continue
        for u in nb[a]:
            if deg[u] != 2:
                if a < u:
                    segs.append([a, u])
                continue
            seg, prev, cur = [a, u], a, u
            while deg[cur] == 2:
                visited[cur] = True
                nxt = nb[cur][0] if nb[cur][0] != prev else nb[cur][1]
                seg.append(nxt)
                prev, cur = cur, nxt
            if seg[0] < seg[-1] or (seg[0] == seg[-1] and seg[1] < seg[-2]):
                segs.append(seg)                           # (met again from the other end, or in the other direction)
    for m in range(n):
        if deg[m] != 2 or visited[m]:
            continue
        seg, prev, cur = [m, nb[m][0]], m, nb[m][0]        # the smallest of its ring, towards its smaller neighbour
        visited[m] = True
        while cur != m:
            visited[cur] = True
            nxt = nb[cur][0] if nb[cur][0] != prev else nb[cur][1]
            seg.append(nxt)
            prev, cur = cur, nxt
        segs.append(seg)
    segs.sort(key=lambda s: (s[0], s[1]))
    lin = idx.tolist()
    counts = {'nodes': sum(1 for x in deg if x != 2), 'isolated': sum(1 for x in deg if x == 0), 'path': sum(1 for x in deg if x == 2)}
    return [[lin[p] for p in s] for s in segs], counts


def arrays(volume):
    """-> (offsets int64 [segments + 1], coords int64 [total, 3], counts): the form of skeletonization.segmentArrays."""
    segs, counts = trace(volume)
    offsets = np.zeros(len(segs) + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in segs])
    flat = np.array([v for s in segs for v in s], np.int64)
    coords = np.stack(np.unravel_index(flat, np.asarray(volume).shape), axis=1).astype(np.int64).reshape(len(flat), 3)
    return offsets, coords, counts


def degrees(volume):
    """Direct numpy count: deg(v) for every voxel (0 where background as well)."""
    obj = np.asarray(volume) != 0
    p = np.pad(obj, 1).astype(np.int32)
    n = sum(p[1 + a:1 + a + obj.shape[0], 1 + b:1 + b + obj.shape[1], 1 + c:1 + c + obj.shape[2]] for a, b, c in OFFSETS)
    return np.where(obj, n, 0)
