"""Sequential model of the branch graph ("f10 branch graph"): the yardstick of tests/test_branches.py.
Plain Python / numpy: clusters from scipy.ndimage.label, tracing from segment_model, re-thinning from skeleton_model, the
rules of include/vmask.h (vmask_branches) taken literally.

S = the voxels != 0; deg, node, path voxel, idx and the segments as in segment_model.
  junction voxel  deg >= 3
  cluster         a 26-connected component of junction voxels; representative: largest deg, then smallest idx
  nodes           the clusters and the end points (deg == 1), numbered ascending by idx(representative)
  branches        the segments other than the two-voxel ones inside one cluster, in the segments' order; voxels = the segment's
                  with the representative in front / behind where the end voxel is not the representative; L = voxels of the
                  segment - 1; ends = node ids, -1 -1 for a closed curve without a node
  spur            end point at one end, cluster C at the other, L <= min_len or (dist given and L <= radius_factor * dist[rep(C)])
  pruning round   per cluster the spur of smallest (L, branch index) goes: all its voxels but the one in C are cleared; then
                  the volume is thinned again and the graph rebuilt; stop at the first round without a spur or after max_rounds
"""
import numpy as np
from scipy import ndimage

import segment_model as SM
import skeleton_model as M

COUNTS = ('nodes', 'clusters', 'endPoints', 'passThrough', 'branches', 'entries', 'isolated', 'droppedSegments',
          'pruneRounds', 'spursRemoved', 'voxelsRemoved')


class Graph:
    pass


def build(volume):
    """One graph build -> Graph with nodes (N x 4 int64: rep idx, kind, members, degree), ends (B x 2), offsets (B + 1),
    voxels (linear indices), counts (dict, the first eight of COUNTS) and, for the pruning, per branch: seg (the underlying
    segment), spur_at (None, or (cluster label, position in seg of the voxel that belongs to the cluster))."""
    obj = np.asarray(volume) != 0
    deg = SM.degrees(obj).ravel()
    segs, sc = SM.trace(obj)
    lab = ndimage.label(obj & (SM.degrees(obj) >= 3), structure=np.ones((3, 3, 3), bool))[0].ravel()
    rep, members = {}, {}                                    # node key -> representative idx / member count
    for v in np.flatnonzero(lab).tolist():
        key = ('c', int(lab[v]))
        members[key] = members.get(key, 0) + 1
        if key not in rep or (deg[v], -v) > (deg[rep[key]], -rep[key]):
            rep[key] = v
    for v in np.flatnonzero(obj.ravel() & (deg == 1)).tolist():
        rep[('e', v)], members[('e', v)] = v, 1

    def node_of(v):
        return ('e', v) if deg[v] == 1 else ('c', int(lab[v]))

    degree = dict.fromkeys(rep, 0)
    g = Graph()
    g.seg, g.spur_at, branches, ends_key, dropped = [], [], [], [], 0
    for s in segs:
        a, b = s[0], s[-1]
        if len(s) == 2 and deg[a] >= 3 and deg[b] >= 3 and lab[a] == lab[b]:
            dropped += 1
            continue
        if a == b and deg[a] == 2:                            # a closed curve that touches no node
            branches.append(list(s)); ends_key.append(None); g.seg.append(s); g.spur_at.append(None)
            continue
        ka, kb = node_of(a), node_of(b)
        degree[ka] += 1; degree[kb] += 1
        branches.append(([rep[ka]] if rep[ka] != a else []) + list(s) + ([rep[kb]] if rep[kb] != b else []))
        ends_key.append((ka, kb))
        g.seg.append(s)
        if deg[a] == 1 and deg[b] >= 3:
            g.spur_at.append((kb, len(s) - 1))
        elif deg[b] == 1 and deg[a] >= 3:
            g.spur_at.append((ka, 0))
        else:
            g.spur_at.append(None)
    order = sorted(rep, key=lambda k: rep[k])
    ids = {k: i for i, k in enumerate(order)}
    g.keys, g.rep = order, rep
    g.nodes = np.array([[rep[k], 0 if k[0] == 'e' else 1, members[k], degree[k]] for k in order], np.int64).reshape(len(order), 4)
    g.ends = np.array([[-1, -1] if e is None else [ids[e[0]], ids[e[1]]] for e in ends_key], np.int64).reshape(len(branches), 2)
    g.offsets = np.zeros(len(branches) + 1, np.int64)
    g.offsets[1:] = np.cumsum([len(b) for b in branches])
    g.voxels = np.array([v for b in branches for v in b], np.int64)
    g.branches = branches
    g.counts = {'nodes': len(order), 'clusters': sum(k[0] == 'c' for k in order), 'endPoints': sum(k[0] == 'e' for k in order),
                'passThrough': sum(k[0] == 'c' and degree[k] == 2 for k in order), 'branches': len(branches),
                'entries': int(g.offsets[-1]), 'isolated': sc['isolated'], 'droppedSegments': dropped}
    return g


def select_spurs(g, min_len, radius_factor, dist):
    """-> {cluster key: branch index} of the spurs that one round removes."""
    best = {}
    d = None if dist is None else np.asarray(dist, np.float64).ravel()
    for k, (s, at) in enumerate(zip(g.seg, g.spur_at)):
        if at is None:
            continue
        L = len(s) - 1
        if L <= min_len or (d is not None and float(L) <= np.float64(radius_factor) * d[g.rep[at[0]]]):
            if at[0] not in best or (L, k) < best[at[0]]:
                best[at[0]] = (L, k)
    return {c: k for c, (L, k) in best.items()}


def branch_graph(volume, min_len=0, radius_factor=0.0, dist=None, max_rounds=64):
    """-> (skeleton uint8 0/1, Graph of the final build with all COUNTS in .counts)."""
    vol = (np.asarray(volume) != 0).astype(np.uint8)
    rounds = spurs = removed = 0
    while True:
        g = build(vol)
        if rounds >= max_rounds:
            break
        chosen = select_spurs(g, min_len, radius_factor, dist)
        if not chosen:
            break
        flat = vol.reshape(-1)
        for c, k in chosen.items():
            s, keep = g.seg[k], g.spur_at[k][1]
            for p, v in enumerate(s):
                if p != keep:
                    flat[v] = 0
                    removed += 1
            spurs += 1
        rounds += 1
        vol = M.thin(vol)[0]
    g.counts.update(pruneRounds=rounds, spursRemoved=spurs, voxelsRemoved=removed)
    return vol, g
