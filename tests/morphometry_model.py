"""Sequential model of the branch morphometry ("f11 branch morphometry"): the yardstick of
tests/test_morphometry.py.  Pure Python floats (IEEE doubles) and loops, the rules of include/vmask.h (vmask_morphometry) taken
literally.

For a branch of n entries e_0 .. e_(n-1) (linear indices into a volume of `shape`):
  stepCounts[c]   the consecutive pairs whose offset d has (|d0|, |d1|, |d2|) in {0,1}^3 without 0, c = 4 |d0| + 2 |d1| + |d2| - 1
  jumps           every other pair; jumpOffset: d of the first pair / of the last pair (n > 2) where that pair is a jump
  radius sample   dist at e_1 .. e_(n-2) for n >= 3, at both entries for n == 2
  the sum of x_0 .. x_(m-1):  a_j = ((x_j + x_(j+64)) + x_(j+128)) + .. for j in [0, 64), 0.0 where there is none;
                  for s = 32, 16, 8, 4, 2, 1: a_j <- a_j + a_(j xor s); the sum is a_0          (`ordered_sum`)
  radiusSum = that sum of the sample, radiusDevSq = that sum of ((x - mean) * (x - mean)), mean = radiusSum / m
  endDir          e_k - e_0 and e_(n-1-k) - e_(n-1), k = min(localSteps, n - 1);  chord = e_(n-1) - e_0
  pathLength      ((0 + stepCounts[0] w_0) + ..) + stepCounts[6] w_6, + |front jump| + |back jump|; w and | | = sqrt((g0^2 + g1^2) + g2^2)
Per node: nodeRadius = dist[representative]; incident = the three (branch, end) that end there when exactly three ends of three
distinct branches do, ascending.
Depth from roots: Dijkstra (heapq) over the branches with fl(D(u) + pathLength[b]); parentBranch = the smallest tight b with
D(u) < D(v); depthLevel / depthVoxel along it; branchLevel = the larger depthLevel of the ends."""
import heapq
import math

import numpy as np

NAN = float('nan')


def ordered_sum(xs):
    a = [0.0] * 64
    for j in range(min(64, len(xs))):
        acc = xs[j]
        for k in range(j + 64, len(xs), 64):
            acc = acc + xs[k]
        a[j] = acc
    for s in (32, 16, 8, 4, 2, 1):
        a = [a[j] + a[j ^ s] for j in range(64)]
    return a[0]


def length_of(o, h):
    g = [float(o[0]) * h[0], float(o[1]) * h[1], float(o[2]) * h[2]]
    return math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])


def morphometry(shape, dist, offsets, voxels, ends, node_voxel, spacing=(1.0, 1.0, 1.0), roots=(), local_steps=5):
    """-> dict of numpy arrays under the names of skeletonization.MORPHOMETRY_RAW (and MORPHOMETRY_DEPTH when there are roots)."""
    h = [float(x) for x in spacing]
    d = np.asarray(dist, np.float64).ravel().tolist()
    off = [int(x) for x in offsets]
    vox = [int(x) for x in voxels]
    ends = np.asarray(ends, np.int64).reshape(-1, 2).tolist()
    B, N = len(off) - 1, len(node_voxel)
    co = lambda v: np.unravel_index(v, shape)
    sub = lambda q, p: [int(x) - int(y) for x, y in zip(co(q), co(p))]
    out = {k: [] for k in ('stepCounts', 'jumps', 'jumpOffset', 'radiusCount', 'radiusSum', 'radiusDevSq', 'radiusMin', 'radiusMax', 'endDir', 'chord', 'pathLength')}
    w = [length_of(((c + 1) >> 2 & 1, (c + 1) >> 1 & 1, (c + 1) & 1), h) for c in range(7)]
    for b in range(B):
        e = vox[off[b]:off[b + 1]]
        n = len(e)
        steps, jumps, jo = [0] * 7, 0, [[0, 0, 0], [0, 0, 0]]
        for i in range(n - 1):
            o = sub(e[i + 1], e[i])
            a = [abs(x) for x in o]
            if max(a) == 1:
                steps[4 * a[0] + 2 * a[1] + a[2] - 1] += 1
            else:
                jumps += 1
                if i == 0:
                    jo[0] = o
                elif i == n - 2:
                    jo[1] = o
        xs = [d[v] for v in (e[1:-1] if n >= 3 else e)]
        m = len(xs)
        total = ordered_sum(xs)
        mean = total / m
        devsq = ordered_sum([(x - mean) * (x - mean) for x in xs])
        k = min(int(local_steps), n - 1)
        length = 0.0
        for c in range(7):
            length = length + float(steps[c]) * w[c]
        length = length + length_of(jo[0], h)
        length = length + length_of(jo[1], h)
        for name, val in (('stepCounts', steps), ('jumps', jumps), ('jumpOffset', jo), ('radiusCount', m), ('radiusSum', total),
                          ('radiusDevSq', NAN if devsq != devsq else devsq), ('radiusMin', min(xs)), ('radiusMax', max(xs)),
                          ('endDir', [sub(e[k], e[0]), sub(e[n - 1 - k], e[n - 1])]), ('chord', sub(e[-1], e[0])), ('pathLength', length)):
            out[name].append(val)
    ints = {'stepCounts': (B, 7), 'jumps': (B,), 'jumpOffset': (B, 2, 3), 'radiusCount': (B,), 'endDir': (B, 2, 3), 'chord': (B, 3)}
    res = {k: (np.array(v, np.int64).reshape(ints[k]) if k in ints else np.array(v, np.float64).reshape(B)) for k, v in out.items()}
    res['nodeRadius'] = np.array([d[int(v)] for v in node_voxel], np.float64)
    res['entryRadius'] = np.array([d[v] for v in vox], np.float64)
    at = [[] for _ in range(N)]
    for b in range(B):
        for end in (0, 1):
            if ends[b][end] >= 0:
                at[ends[b][end]].append((b, end))
    ib, ie = np.full((N, 3), -1, np.int64), np.full((N, 3), -1, np.int64)
    for v in range(N):
        if len(at[v]) == 3 and len({b for b, _ in at[v]}) == 3:
            ib[v], ie[v] = [b for b, _ in sorted(at[v])], [e_ for _, e_ in sorted(at[v])]
    res['incidentBranch'], res['incidentEnd'] = ib, ie
    if len(roots):
        res.update(depth(N, off, ends, res['pathLength'].tolist(), [int(r) for r in roots]))
    return res


def depth(N, off, ends, w, roots):
    B = len(off) - 1
    D = [math.inf] * N
    heap = []
    for r in roots:
        D[r] = 0.0
        heap.append((0.0, r))
    heapq.heapify(heap)
    nbr = [[] for _ in range(N)]
    for b in range(B):
        u, v = ends[b]
        if u >= 0 and v >= 0 and u != v:
            nbr[u].append((v, b)); nbr[v].append((u, b))
    while heap:
        du, u = heapq.heappop(heap)
        if du > D[u]:
            continue
        for v, b in nbr[u]:
            c = du + w[b]
            if c < D[v]:
                D[v] = c
                heapq.heappush(heap, (c, v))
    parent = [-1] * N
    for v in range(N):
        if D[v] == math.inf or D[v] == 0.0 and v in roots:
            continue
        tight = [b for u, b in nbr[v] if D[u] < D[v] and D[u] + w[b] == D[v]]
        parent[v] = min(tight) if tight else -1
    level, voxel = [-1] * N, [-1] * N
    for r in roots:
        level[r] = voxel[r] = 0
    for v in sorted((v for v in range(N) if parent[v] >= 0), key=lambda v: D[v]):      # a parent's D is smaller: it comes first
        b = parent[v]
        u = ends[b][1] if ends[b][0] == v else ends[b][0]
        level[v], voxel[v] = level[u] + 1, voxel[u] + (off[b + 1] - off[b] - 1)
    blevel = [max(level[u], level[v]) if u >= 0 and v >= 0 and level[u] >= 0 and level[v] >= 0 else -1 for u, v in ends]
    return dict(pathDistance=np.array(D, np.float64), parentBranch=np.array(parent, np.int64), depthLevel=np.array(level, np.int64),
                depthVoxel=np.array(voxel, np.int64), branchLevel=np.array(blevel, np.int64).reshape(B))
