"""Sequential model of vmask_compartments (include/vmask.h, DESIGN.md section 9 "f12 compartments").

It builds the vertex graph of the definition explicitly - one vertex per node, per interior entry and per closed branch, one edge
per pair of consecutive entries - and runs a plain breadth-first search with a deque per compartment; the levels come from one
pass over the vertices in ascending depth, then the owner rule.  Nothing here knows that an interior entry has two neighbours:
the kernel's per-branch shortcuts (hop counts to the ends, rounds over the nodes, closed forms between two sources) have no
counterpart, which is the point."""
from collections import deque

import numpy as np


class VertexGraph:
    """``entry_vertex`` (E): the vertex of every entry; ``voxel`` / ``is_node`` per vertex; ``adj``: neighbour lists.  The nodes
    are the vertices 0 .. N - 1."""

    def __init__(self, offsets, voxels, ends, node_voxel):
        off, vox = np.asarray(offsets, np.int64), np.asarray(voxels, np.int64)
        ends, node_voxel = np.asarray(ends, np.int64).reshape(-1, 2), np.asarray(node_voxel, np.int64)
        N, B = len(node_voxel), len(off) - 1
        voxel, entry_vertex = node_voxel.tolist(), np.full(len(vox), -1, np.int64)
        for b in range(B):
            a, z = int(off[b]), int(off[b + 1])
            if ends[b, 0] >= 0:
                entry_vertex[a], entry_vertex[z - 1] = ends[b]
            else:
                entry_vertex[a] = entry_vertex[z - 1] = len(voxel)
                voxel.append(int(vox[a]))
            for e in range(a + 1, z - 1):
                entry_vertex[e] = len(voxel)
                voxel.append(int(vox[e]))
        self.N, self.B, self.off, self.ends = N, B, off, ends
        self.entry_vertex, self.voxel = entry_vertex, np.array(voxel, np.int64)
        self.is_node = np.arange(len(voxel)) < N
        self.adj = [[] for _ in voxel]
        for b in range(B):
            for e in range(int(off[b]), int(off[b + 1]) - 1):
                x, y = int(entry_vertex[e]), int(entry_vertex[e + 1])
                if x != y:
                    self.adj[x].append(y)
                    self.adj[y].append(x)


def traverse(g, initial, boundary):
    """Depth and level of every vertex of `g` for one compartment (-1: not reached)."""
    blocked = np.isin(g.voxel, np.asarray(boundary, np.int64))
    start = np.flatnonzero(np.isin(g.voxel, np.asarray(initial, np.int64)) & ~blocked)
    depth = np.full(len(g.voxel), -1, np.int64)
    depth[start] = 0
    queue = deque(start.tolist())
    while queue:
        x = queue.popleft()
        for y in g.adj[x]:
            if depth[y] < 0 and not blocked[y]:
                depth[y] = depth[x] + 1
                queue.append(y)
    level = np.full(len(g.voxel), -1, np.int64)
    for x in np.argsort(depth, kind='stable').tolist():
        if depth[x] == 0:
            level[x] = 0
        elif depth[x] > 0:
            level[x] = min(level[y] for y in g.adj[x] if depth[y] == depth[x] - 1) + int(g.is_node[x])      # (a blocked y has depth -1)
    return depth, level


def partition(offsets, voxels, ends, node_voxel, compartments):
    """`compartments`: a list of (initial, boundary) lists of linear indices.  Returns a dict with vmask_compartments' outputs
    under the names of skeletonization.COMPARTMENT_ARRAYS, and ``reached`` (K x vertices, bool) with the `VertexGraph` ``graph``."""
    g = VertexGraph(offsets, voxels, ends, node_voxel)
    K, nv = len(compartments), len(g.voxel)
    owner, depth, level = np.zeros(nv, np.uint8), np.full(nv, -1, np.int64), np.full(nv, -1, np.int64)
    reached = np.zeros((K, nv), bool)
    for c, (initial, boundary) in enumerate(compartments):
        d, l = traverse(g, initial, boundary)
        reached[c] = d >= 0
        take = (d >= 0) & ((owner == 0) | (d < depth))                    # (ascending c: an equal depth keeps the smaller label)
        owner[take], depth[take], level[take] = c + 1, d[take], l[take]
    ev = g.entry_vertex
    out = {'entryCompartment': owner[ev], 'entryDepth': depth[ev], 'entryLevel': level[ev],
           'nodeCompartment': owner[:g.N], 'nodeDepth': depth[:g.N], 'nodeLevel': level[:g.N]}
    bcomp, blevel = np.zeros(g.B, np.uint8), np.full(g.B, -1, np.int64)
    for b in range(g.B):
        mine = ev[g.off[b]:g.off[b + 1]]
        if owner[mine[0]] and (owner[mine] == owner[mine[0]]).all():
            bcomp[b], blevel[b] = owner[mine[0]], level[mine].min()
    counts = np.zeros((K + 1, 3), np.int64)
    counts[:, 0] = np.bincount(owner, minlength=K + 1)
    counts[1:, 1] = reached.sum(axis=1)
    counts[0, 1] = np.count_nonzero(reached.sum(axis=0) >= 2)
    counts[:, 2] = np.bincount(bcomp, minlength=K + 1)
    out.update(branchCompartment=bcomp, branchLevel=blevel, compartmentCounts=counts, reached=reached, graph=g)
    return out
