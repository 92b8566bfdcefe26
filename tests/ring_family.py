"""Closed curves for the segment-tracing tests ("f6 segment tracing"): free rings of every small length, planar
and non-planar, in all 48 orientations of the lattice, and one packed volume that holds them beside open chains and lollipops.

Octagons.  A closed lattice walk in the plane that turns 45 degrees at every corner: sides E, NE, N, NW, W, SW, S, SE of lengths
e[0..7] >= 1.  It closes when e0 + e1 + e7 == e3 + e4 + e5 and e1 + e2 + e3 == e5 + e6 + e7.  No side may be missing between two
axis-parallel sides: a right-angle corner makes the two voxels beside it diagonal neighbours, and they would have degree 3.
`octagons(maxL)` gives, for every length L = sum(e) that has one, the first such e (lexicographic) with sides in 1..4:
L = 8, 10, 11, .., 30, 32 (9 and 31 have none: one side longer or shorter than all the others cannot close).
`lift=True` puts voxel (x, y) at z = x: |dz| = |dx|, so the adjacencies are those of the planar ring and the ring is not planar.

Small rings, by hand or by exhaustive search for induced cycles of the 26-adjacency in a small box (every one passes the check
of tests/test_segment_rings.py: all voxels of degree 2, one closed segment of L + 1 entries):
  3   three mutually adjacent voxels: {(0,0,0), (1,0,0), (0,1,0)} in a plane, {(0,0,0), (1,1,0), (0,1,1)} in space
  4   |x| + |y| = 1
  5   no planar one exists in a 5 x 5 box; the one here is the first found in 3 x 3 x 3
  6, 7, 9   planar: diagonal sides may meet at a right angle, which the octagons above leave out

A member is a `Ring`: its name, the voxels in walking order and, per run of equal steps, (step, count) - from which the step
classes of branch morphometry follow without tracing anything.
"""
import functools
import itertools

import numpy as np

DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))          # E NE N NW W SW S SE as (dx, dy)
CHAIN_PATH_VOXELS = (255, 256, 257, 420)
TAIL = 3


class Ring:
    def __init__(self, name, points, e=None, lifted=False):
        pts = np.array(points, np.int64).reshape(-1, 3)
        self.name, self.e, self.lifted = name, e, lifted
        self.points = pts - pts.min(axis=0)                                            # walking order, the box starts at 0
        self.L = len(pts)
        self.extent = tuple(int(k) for k in self.points.max(axis=0) + 1)
        steps = np.roll(self.points, -1, axis=0) - self.points                          # the step that closes the ring included
        self.steps = [(tuple(int(c) for c in s), len(list(g))) for s, g in itertools.groupby(steps.tolist())]

    def volume(self, margin=0):
        v = np.zeros(tuple(k + 2 * margin for k in self.extent), np.uint8)
        v[tuple((self.points + margin).T)] = 1
        return v


def closes(e):
    return len(e) == 8 and min(e) >= 1 and e[0] + e[1] + e[7] == e[3] + e[4] + e[5] and e[1] + e[2] + e[3] == e[5] + e[6] + e[7]


def walk(e, lift=False):
    """The voxels of the octagon with sides e, in walking order from the start of the E side."""
    assert closes(e)
    x = y = 0
    out = []
    for (dx, dy), k in zip(DIRS, e):
        for _ in range(k):
            out.append((x, y, x if lift else 0))
            x, y = x + dx, y + dy
    assert (x, y) == (0, 0)
    return out


@functools.lru_cache(maxsize=None)
def octagons(maxL=32):
    """{L: e} - for every length up to maxL the first closing e with sides in 1..4."""
    found = {}
    for e in itertools.product(range(1, 5), repeat=8):
        if sum(e) <= maxL and sum(e) not in found and closes(e):
            found[sum(e)] = e
    return dict(sorted(found.items()))


def octagon(e, lift=False):
    return Ring('octagon{}{}'.format(sum(e), '-lifted' if lift else ''), walk(e, lift), e=tuple(e), lifted=lift)


SMALL = {
    'ring3-plane': [(0, 0, 0), (1, 0, 0), (0, 1, 0)],
    'ring3-space': [(0, 0, 0), (1, 1, 0), (0, 1, 1)],
    'ring4': [(1, 0, 0), (2, 1, 0), (1, 2, 0), (0, 1, 0)],
    'ring5': [(0, 0, 1), (1, 1, 2), (2, 2, 1), (2, 1, 0), (1, 0, 0)],
    'ring6': [(0, 1, 0), (1, 2, 0), (2, 2, 0), (3, 1, 0), (2, 0, 0), (1, 0, 0)],
    'ring7': [(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 2, 0), (3, 1, 0), (2, 0, 0), (1, 0, 0)],
    'ring9': [(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 4, 0), (4, 3, 0), (4, 2, 0), (3, 1, 0), (2, 0, 0), (1, 0, 0)],
}


def small(name):
    return Ring(name, SMALL[name])


@functools.lru_cache(maxsize=None)
def family():
    """Every ring: the small ones, and every octagon planar and lifted."""
    out = [small(n) for n in SMALL]
    for e in octagons().values():
        out += [octagon(e), octagon(e, True)]
    return tuple(out)


# ------------------------------------------------------------------ the 48 orientations
ORIENTATIONS = tuple((perm, flips) for perm in itertools.permutations(range(3)) for flips in itertools.product((False, True), repeat=3))


def orient(v, k):
    """Image k of a volume: axis a of the image is axis perm[a] of v, reversed where flips[a]; C-contiguous."""
    perm, flips = ORIENTATIONS[k]
    w = np.transpose(v, perm)
    return np.ascontiguousarray(np.flip(w, [a for a in range(3) if flips[a]]))


def orient_coords(coords, shape, k):
    """Where the voxels `coords` of a volume of `shape` lie in `orient(v, k)`."""
    perm, flips = ORIENTATIONS[k]
    c = np.asarray(coords, np.int64).reshape(-1, 3)[:, list(perm)]
    ext = np.array(shape, np.int64)[list(perm)]
    return np.where(np.array(flips), ext - 1 - c, c)


def orient_step(step, k):
    """|step| per axis of the image (a flip changes the sign only)."""
    return tuple(abs(int(step[p])) for p in ORIENTATIONS[k][0])


def oriented(v):
    for k in range(len(ORIENTATIONS)):
        yield orient(v, k)


# ------------------------------------------------------------------ the packed volume
LOLLIPOP_E = (2, 2, 2, 2, 2, 2, 2, 2)


def _adjacent(p, q):
    return max(abs(a - b) for a, b in zip(p, q)) == 1


def lollipop(at_minimum):
    """The octagon LOLLIPOP_E with a straight tail of TAIL voxels that touches the ring at one voxel only: the ring's voxel of
    smallest index, or the corner half way round.  -> (ring voxels in walking order, tail voxels from the ring outwards)."""
    ring = walk(LOLLIPOP_E)
    at = min(ring) if at_minimum else ring[len(ring) // 2]
    for dx, dy in DIRS:
        tail = [(at[0] + j * dx, at[1] + j * dy, 0) for j in range(1, TAIL + 1)]
        if not any(_adjacent(t, r) for t in tail for r in ring if r != at) and not set(tail) & set(ring):
            return ring, at, tail
    raise AssertionError('no free direction for the tail')


@functools.lru_cache(maxsize=None)
def _layout():
    """-> (shape, items); an item is (kind, name, ring or None, voxels int64 [k, 3] in the identity orientation, walking order)."""
    n1 = max(CHAIN_PATH_VOXELS) + 4
    items = []
    x = 0
    for p in CHAIN_PATH_VOXELS:                                                        # p path voxels between two end points
        vox = np.array([(x, 1 + j, 0) for j in range(p + 2)], np.int64)
        items.append(('chain', 'chain{}'.format(p), None, vox))
        x += 2
    rings = [small(n) for n in SMALL] + [octagon(e, lift=bool(L % 2)) for L, e in octagons().items()]
    boxes = [('ring', r.name, r, r.points) for r in rings]
    for at_min in (True, False):
        ring, at, tail = lollipop(at_min)
        pts = np.array(ring + tail, np.int64)
        boxes.append(('lollipop', 'lollipop-' + ('minimum' if at_min else 'elsewhere'), (len(ring), at), pts - pts.min(axis=0)))
    y, shelf = 0, 0
    for kind, name, ring, pts in boxes:                                                # shelves along axis 1, boxes one free voxel apart
        ext = pts.max(axis=0) + 1
        if y + ext[1] > n1:
            x, y, shelf = x + shelf + 1, 0, 0
        items.append((kind, name, ring, pts + np.array([x, y, 0])))
        y, shelf = y + int(ext[1]) + 1, max(shelf, int(ext[0]))
    n0 = x + shelf
    n2 = max(int(it[3][:, 2].max()) for it in items) + 1
    return (n0, n1, n2), tuple(items)


def packed_items(orientation=0):
    """The items of `packed` with their voxels where that orientation puts them."""
    shape, items = _layout()
    return [(kind, name, ring, orient_coords(vox, shape, orientation)) for kind, name, ring, vox in items]


def packed(orientation=0):
    """Every ring of the family once (planar or lifted by the parity of L) a free voxel apart, open straight chains of
    CHAIN_PATH_VOXELS path voxels, and two lollipops (a ring with a tail of TAIL voxels: at the ring's voxel of smallest
    index, and elsewhere)."""
    shape, items = _layout()
    v = np.zeros(shape, np.uint8)
    for _, _, _, vox in items:
        assert not v[tuple(vox.T)].any()
        v[tuple(vox.T)] = 1
    return orient(v, orientation)


def expected_step_counts(ring, orientation):
    """stepCounts of branch morphometry for a free ring: pairs of consecutive entries by class 4 |d0| + 2 |d1| + |d2| - 1, from the
    ring's runs of equal steps and the orientation alone."""
    counts = [0] * 7
    for step, k in ring.steps:
        d = orient_step(step, orientation)
        counts[4 * d[0] + 2 * d[1] + d[2] - 1] += k
    return counts
