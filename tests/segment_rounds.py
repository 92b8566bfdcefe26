"""A second model of segment tracing ("f6 segment tracing"): not the sequential walk of tests/segment_model.py
but what csrc/vseg_device.hip does, restated one dart at a time - k_seg_link, k_seg_jump (synchronous: every dart of a round
reads the state of the round before), the host loop with its two counters, k_seg_resolve, the sorted heads and k_seg_scatter.
It yields the segments and the number of pointer-jumping rounds; the rounds are deterministic (double-buffered darts, one
launch per round), so a GPU run must report exactly this number.

Slots here are the object voxels in ascending index, so comparing slots compares indices; the GPU's slot order is whatever
its atomics gave and no result depends on it.  Dart 2 i + s: at path voxel i, heading to its smaller (s = 0) or larger (s = 1)
neighbour.  A dart's state is [x successor dart, terminal flag, y hops to it, z smallest voxel in the window behind the hops,
w = 2 * (hops to that voxel) + (direction bit of the dart met there)].

`mutation` swaps one line for a wrong one (tests/test_segment_rings.py shows that the test volumes notice each):
  'le'          the successor's minimum taken on <= instead of <
  'direction'   the direction bit of A.w inverted in the ring branch of resolve
  'exit-before' the unsettled minima counted over the darts open before the jump, not over those still open after it
  'length'      a ring's length without the + 1
"""
import segment_model as SM

MAX_ROUNDS = 72
MUTATIONS = ('le', 'direction', 'exit-before', 'length')
NONE = -1


def link(nb, deg):
    st, n_open = [], 0
    for i in range(len(nb)):
        for s in (0, 1):
            a = [2 * i + s, True, 0, i, s]
            if deg[i] == 2:
                j = nb[i][s]
                if deg[j] == 2:
                    a[0], a[1], a[2] = 2 * j + (1 if nb[j][0] == i else 0), False, 1
                    n_open += 1
            st.append(a)
    return st, n_open


def jump(st, mutation=None):
    out, n_open, unsettled = [], 0, 0
    for a in st:
        a = list(a)
        if not a[1]:
            b = st[a[0]]                                                 # a terminal dart is its own successor with 0 hops
            differ = b[3] != a[3]
            if b[3] < a[3] or (mutation == 'le' and b[3] == a[3]):
                a[4] = 2 * a[2] + b[4]
                a[3] = b[3]
            a[0], a[1] = b[0], b[1]
            a[2] += b[2]
            if not a[1]:
                n_open += 1
            if differ and (mutation == 'exit-before' or not a[1]):
                unsettled += 1
        out.append(a)
    return out, n_open, unsettled


def resolve(nb, deg, st, mutation=None):
    """-> (info: per slot [first, second, position, length] or the list of larger adjacent nodes; tail: per slot the last voxel)."""
    info, tail = [], []
    for i in range(len(nb)):
        o, last = [0, 0, NONE, 0], 0
        if deg[i] == 2:
            A, B = st[2 * i], st[2 * i + 1]
            if A[1] and B[1]:                                            # on a chain between two nodes
                ta, tb = A[0], B[0]
                enda, lasta, endb, lastb = nb[ta >> 1][ta & 1], ta >> 1, nb[tb >> 1][tb & 1], tb >> 1
                froma = enda < endb or (enda == endb and lasta < lastb)
                o = [enda, lasta, 1 + A[2], A[2] + B[2] + 3] if froma else [endb, lastb, 1 + B[2], A[2] + B[2] + 3]
                last = endb if froma else enda
            elif i != A[3]:                                              # on a free ring; the minimum is written by the voxel behind it
                m = A[3]
                bit = A[4] & 1
                if mutation == 'direction':
                    bit ^= 1
                o = [m, nb[m][0], A[4] >> 1 if bit else B[4] >> 1, (A[4] >> 1) + (B[4] >> 1) + (0 if mutation == 'length' else 1)]
                last = m
        else:
            o = [j for j in nb[i] if j > i and deg[j] != 2]
        info.append(o)
        tail.append(last)
    return info, tail


def run(volume, mutation=None):
    """-> (segments: lists of linear indices in canonical form and order, or None where the bookkeeping does not add up (the
    library's internal error); rounds)."""
    idx, nb = SM.neighbour_table(volume)
    n = len(idx)
    deg = [len(x) for x in nb]
    st, n_open = link(nb, deg)
    rounds = 0
    while n_open:                                                        # until every dart is at a terminal or on a ring that knows its minimum
        if rounds == MAX_ROUNDS:
            return None, rounds
        st, n_open, unsettled = jump(st, mutation)
        rounds += 1
        if not unsettled:
            break
    info, tail = resolve(nb, deg, st, mutation)
    heads = []
    for i in range(n):
        if deg[i] == 2:
            if info[i][2] == 1:
                heads.append(((info[i][0], info[i][1]), info[i][3]))
        else:
            heads.extend(((i, j), 2) for j in info[i])
    heads.sort()
    keys = {h[0]: k for k, h in enumerate(heads)}
    if len(keys) != len(heads):
        return None, rounds
    segs = [[NONE] * h[1] for h in heads]
    for i in range(n):                                                   # the scatter: every path voxel at its position, the one at 1 also both ends
        if deg[i] == 2:
            first, second, pos, length = info[i]
            k = keys.get((first, second))
            if pos == NONE or k is None or length != len(segs[k]) or pos >= length:
                continue
            segs[k][pos] = i
            if pos == 1:
                segs[k][0], segs[k][length - 1] = first, tail[i]
        else:
            for j in info[i]:
                segs[keys[(i, j)]][:] = [i, j]
    lin = idx.tolist()
    return [[lin[p] if p != NONE else NONE for p in s] for s in segs], rounds
