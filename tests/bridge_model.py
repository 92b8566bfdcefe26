"""The definition of vmask_bridge (include/vmask.h) restated in numpy, and a heap Dijkstra beside it.

`model` is the oracle of tests/test_bridge.py: Jacobi sweeps over the 26 shifted arrays until nothing changes - the least fixed
point of D, then Root, Pred, the contacts and the paths exactly as the header defines them, every float64 operation one
numpy operation (numpy never fuses).  `dijkstra` computes D, Root and Pred with a heap and Python loops: on tiny volumes with
ties the two agree, which is what "the fixed point is unique" means in practice."""
import heapq

import numpy as np

OFFSETS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
BIG = np.int64(1) << 40


def half_weights(spacing=None):
    h = np.ones(3) if spacing is None else np.asarray(spacing, np.float64)
    hw = np.empty(26)
    for k, (x, y, z) in enumerate(OFFSETS):
        a, b, c = np.float64(x) * h[0], np.float64(y) * h[1], np.float64(z) * h[2]
        hw[k] = 0.5 * np.sqrt((a * a + b * b) + c * c)
    return hw


def shifted(A, off, fill):
    """B[v] = A[v + off], `fill` where v + off lies outside the volume."""
    P = np.full(tuple(n + 2 for n in A.shape), fill, A.dtype)
    P[1:-1, 1:-1, 1:-1] = A
    x, y, z = off
    n0, n1, n2 = A.shape
    return P[1 + x:1 + x + n0, 1 + y:1 + y + n1, 1 + z:1 + z + n2]


def components(m):
    """The 26-connected components of the boolean volume m, numbered 1..n in raster order of their first voxel."""
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    low = np.where(m, idx, BIG)
    while True:
        new = low
        for off in OFFSETS:
            new = np.minimum(new, shifted(low, off, BIG))
        new = np.where(m, new, BIG)
        if np.array_equal(new, low):
            break
        low = new
    firsts = np.unique(low[m])
    comp = np.zeros(m.shape, np.int32)
    comp[m] = np.searchsorted(firsts, low[m]) + 1
    return comp, len(firsts)


def setup(mask, domain, cost, spacing):
    m = np.asarray(mask) != 0
    dom = m | (np.ones(m.shape, bool) if domain is None else np.asarray(domain) != 0)
    c = np.where(dom, np.asarray(cost).astype(np.float64), 1.0)
    hw = half_weights(spacing)
    W = [(c + shifted(c, off, 1.0)) * hw[k] for k, off in enumerate(OFFSETS)]        # fl(fl(c(u) + c(v)) hw[k])
    return m, dom, c, hw, W


class Result:
    pass


def model(mask, cost, domain=None, tips=None, spacing=None, max_cost=16.0, tip_rule=1):
    m, dom, c, hw, W = setup(mask, domain, cost, spacing)
    shape = m.shape
    R = 0.5 * max_cost
    free = dom & ~m
    idx = np.arange(m.size, dtype=np.int64).reshape(shape)
    D = np.where(m, 0.0, np.inf)
    while True:
        best = D
        for k, off in enumerate(OFFSETS):
            cand = shifted(D, off, np.inf) + W[k]
            best = np.minimum(best, np.where(cand <= R, cand, np.inf))
        new = np.where(free, best, D)
        if np.array_equal(new, D):
            break
        D = new
    reached = free & np.isfinite(D)
    tight = [reached & (shifted(D, off, np.inf) + W[k] == D) for k, off in enumerate(OFFSETS)]
    root = np.where(m, idx, BIG)
    while True:
        new = root
        for k, off in enumerate(OFFSETS):
            new = np.minimum(new, np.where(tight[k], shifted(root, off, BIG), BIG))
        if np.array_equal(new, root):
            break
        root = new
    pred = np.full(shape, 255, np.uint8)
    for k, off in enumerate(OFFSETS):
        hit = tight[k] & (shifted(root, off, BIG) == root) & (pred == 255)
        pred[hit] = k
    assert not (reached & (pred == 255)).any() and not (reached & (root == BIG)).any()
    comp, ncomp = components(m)
    fin = m | reached
    tipv = np.ones(shape, bool) if tips is None else np.asarray(tips) != 0
    cr = np.zeros(shape, np.int64)                 # component of the root, tip of the root
    tr = np.zeros(shape, np.int64)
    cr[fin] = comp.reshape(-1)[root[fin]]
    tr[fin] = tipv.reshape(-1)[root[fin]]
    rows = []
    for k, off in enumerate(OFFSETS):              # u = here, v = u + off
        cv, tv, fv, Dv = shifted(cr, off, 0), shifted(tr, off, 0), shifted(fin, off, False), shifted(D, off, np.inf)
        q = fin & fv & (cr < cv) & (tr + tv >= tip_rule)
        if not q.any():
            continue
        K = (D[q] + Dv[q]) + W[k][q]
        rows.append(np.stack((cr[q].astype(np.float64), cv[q].astype(np.float64), K, idx[q].astype(np.float64), np.full(int(q.sum()), float(k))), axis=1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 5))
    order = np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    rows = rows[order]
    first = np.ones(len(rows), bool)
    first[1:] = (rows[1:, 0] != rows[:-1, 0]) | (rows[1:, 1] != rows[:-1, 1])
    best = rows[first]
    kept = best[best[:, 2] <= max_cost]
    flat_pred, flat_root = pred.reshape(-1), root.reshape(-1)
    strides = np.array([shape[1] * shape[2], shape[2], 1], np.int64)

    def chain(v):
        out = [int(v)]
        while flat_pred[out[-1]] != 255:
            out.append(out[-1] + int(np.dot(OFFSETS[flat_pred[out[-1]]], strides)))
        return out

    pairs, costs, offsets, voxels = [], [], [0], []
    for a, b, K, u, k in kept:
        u = int(u)
        v = u + int(np.dot(OFFSETS[int(k)], strides))
        path = chain(u)[::-1] + chain(v)
        pairs.append((int(a), int(b), u, v, int(flat_root[u]), int(flat_root[v])))
        costs.append(K)
        voxels += path
        offsets.append(len(voxels))
    r = Result()
    r.dist = np.where(dom, D, -1.0)
    r.root = np.where(fin, root, -1).astype(np.int32)
    r.pred = pred
    r.comp = comp
    r.pairs = np.array(pairs, np.int64).reshape(-1, 6)
    r.costs = np.array(costs, np.float64)
    r.offsets = np.array(offsets, np.int64)
    r.voxels = np.array(voxels, np.int64)
    r.counts = np.array([ncomp, int(dom.sum()), int(reached.sum()), len(rows), len(best), len(kept), len(voxels)], np.int64)
    return r


def brick_any(a):
    """Which 8x8x8 bricks of the boolean volume a hold a set voxel: a boolean array over the brick grid."""
    B = tuple((n + 7) // 8 for n in a.shape)
    P = np.zeros(tuple(8 * b for b in B), bool)
    P[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return P.reshape(B[0], 8, B[1], 8, B[2], 8).any(axis=(1, 3, 5))


def expected_bricks(mask, cost, domain=None, spacing=None, max_cost=16.0):
    """The storage rule that include/vmask.h states under VRG_E_MEM, from its text: storage goes to the bricks that hold a voxel
    of the effective domain and lie within `reach` bricks (Chebyshev) of one that holds a mask voxel, reach =
    min(max(B0, B1, B2), ceil(steps / 8)), steps = floor(1.001 R / w_min) + 1, w_min = fl(fl(2 c_min) min hw), c_min the
    smallest cost in the effective domain.  Returns (stored, facts): the boolean brick grid, and a dict with `ratio` =
    1.001 R / w_min as computed here (the caller keeps it away from the integers: floor and ceil are then the host's whatever
    the order of its roundings), `steps`, `reach` and `domain_bricks`."""
    m, dom, c, hw, W = setup(mask, domain, cost, spacing)
    mb, db = brick_any(m), brick_any(dom)
    B = mb.shape
    ratio, steps, reach = 0.0, 0, 0
    if dom.any():
        c_min = c[dom].min()
        w_min = (c_min + c_min) * hw.min()
        ratio = float(1.001 * (0.5 * max_cost) / w_min)
        steps = int(np.floor(ratio)) + 1
        reach = min(max(B), -(-steps // 8))
    b0, b1, b2 = np.nonzero(mb)
    g0, g1, g2 = np.indices(B)
    close = np.zeros(B, bool)
    for p, q, r in zip(b0, b1, b2):                # one box per mask brick: nothing here is separable, strided or clamped
        close |= np.maximum(np.maximum(np.abs(g0 - p), np.abs(g1 - q)), np.abs(g2 - r)) <= reach
    return close & db, dict(ratio=ratio, steps=steps, reach=reach, domain_bricks=int(db.sum()))


def dijkstra(mask, cost, domain=None, spacing=None, max_cost=16.0):
    """(dist, root, pred) as `model` gives them, by a heap over (D, voxel) and Python loops; Root and Pred in the order of
    increasing D, which is well founded because every weight is positive.  Nothing is shared with `model` but OFFSETS: the
    domain, the half-weights and w(p, q) are written out again here, edge by edge, from the header's text."""
    m = np.asarray(mask) != 0
    dom = np.ones(m.shape, bool) if domain is None else (m | (np.asarray(domain) != 0))
    c = np.asarray(cost).astype(np.float64)
    h = (1.0, 1.0, 1.0) if spacing is None else tuple(float(x) for x in spacing)
    shape = m.shape
    R = max_cost / 2.0
    D = np.where(m, 0.0, np.inf)
    heap = [(0.0, p) for p in zip(*np.nonzero(m))]
    heapq.heapify(heap)
    done = np.zeros(shape, bool)

    def weight(p, q, off):
        a, b, e = off[0] * h[0], off[1] * h[1], off[2] * h[2]
        length = float(np.sqrt(np.float64(a * a + b * b) + np.float64(e * e)))
        return float(np.float64(c[p] + c[q]) * np.float64(length / 2.0))

    def neighbours(p):
        for k, off in enumerate(OFFSETS):
            q = (p[0] + off[0], p[1] + off[1], p[2] + off[2])
            if all(0 <= q[a] < shape[a] for a in range(3)) and dom[q]:
                yield k, q, weight(p, q, off)

    while heap:
        d, p = heapq.heappop(heap)
        if done[p] or d > D[p]:
            continue
        done[p] = True
        for k, q, w in neighbours(p):
            if m[q]:
                continue
            cand = d + w
            if cand <= R and cand < D[q]:
                D[q] = cand
                heapq.heappush(heap, (cand, q))
    root = np.full(shape, -1, np.int64)
    pred = np.full(shape, 255, np.uint8)
    root[m] = np.ravel_multi_index(np.nonzero(m), shape)
    todo = sorted((D[p], p) for p in zip(*np.nonzero(~m & np.isfinite(D))))
    for d, p in todo:
        tightk = [(k, q) for k, q, w in neighbours(p) if D[q] + w == d]
        root[p] = min(root[q] for _, q in tightk)
        pred[p] = min(k for k, q in tightk if root[q] == root[p])
    return np.where(dom, D, -1.0), root.astype(np.int32), pred
