"""One wave of one item of k_edt_envelope (csrc/vmask_device.hip), restated sequentially: 64 lanes in lockstep per batch of
AHEAD sites, each with its stack (q, low, eb, ue, the top entry, dn_t / dn_v), its ring of RING slots and its spill entries;
the wave-collective write-out of final spilled chunks, the write-out from the bottom of the ring, the pop with its chunk
reload, the push with its spill, the reset of an emptied stack and the read-back down to ue.  The storage is modelled, not
only the decisions, so a mutation of the bookkeeping gives wrong rows here as it would in the kernel.  Arithmetic is exact
(Python integers): the model says WHICH PATHS an input drives and what the rows must be, not how wide a register is.
Lanes whose lines are equal behave alike (the collective decisions are functions of all lanes), so each distinct line is
run once and counted with its multiplicity: the counters are over all 64 lanes, as the kernel would count them.
Test code only."""
import numpy as np

from oracle import mask_oracle as MO

RING, CHUNK, AHEAD, LANES = 16, 8, 8, 64
INF32, INF64 = 1 << 29, (1 << 32) - 1                # the "no zero voxel" value of the two arithmetic widths
COUNTERS = ('depth', 'spills', 'build_reloads', 'read_reloads', 'chunk_flush', 'chunk_flush_next_spilled', 'flush_blocked',
            'bottom_leaves', 'reset', 'spill_after_reload', 'spill_after_flush', 'not_pushed')
MUTATIONS = ('pop_without_reload', 'stale_dn_after_flush', 'read_back_to_zero')


def new_counts():
    return dict.fromkeys(COUNTERS, 0)


def add_counts(total, other):
    """depth: the maximum; everything else: the sum"""
    for k in COUNTERS:
        total[k] = max(total[k], other[k]) if k == 'depth' else total[k] + other[k]
    return total


class _Lane:
    __slots__ = ('G', 'mult', 'q', 'low', 'eb', 'ue', 'ts', 'tt', 'tg', 'tv', 'dn_t', 'dn_v', 'ring', 'spill', 'out',
                 'reloaded', 'flushed')


def trace_wave(lines, inf, mutation=None, divisions=None):
    """lines: [lanes][m] values >= 0 (inf: no zero voxel in that column); returns (rows [lanes][m], counters).
    depth counts the entries that are not yet written out (q - eb + 1).  `divisions`, when a list, receives the
    (numerator, divisor) of every start formula, once per distinct line."""
    assert mutation is None or mutation in MUTATIONS
    lines = np.asarray(lines, np.int64)
    nl, m = lines.shape
    mp = (m + CHUNK - 1) // CHUNK * CHUNK
    cnt = new_counts()
    uniq, inverse, mult = np.unique(lines, axis=0, return_inverse=True, return_counts=True)
    inverse = np.asarray(inverse).reshape(-1)
    lanes = []
    for G, k in zip(uniq.tolist(), mult.tolist()):
        a = _Lane()
        a.G, a.mult = G, k
        a.q = a.low = a.eb = a.ue = 0
        a.ts = a.tt = 0
        a.tg = a.tv = G[0]
        a.dn_t = a.dn_v = 0
        a.ring = [(0, 0, 0)] * RING                 # (site, start, G(site))
        a.ring[0] = (0, 0, G[0])
        a.spill = [(0, 0, 0)] * mp
        a.out = [-1] * m
        a.reloaded = a.flushed = False
        lanes.append(a)

    def clamp(v):
        return inf if v >= inf else v

    def rows_out(a, s0, g0, r0, r1):
        for r in range(r0, r1):
            a.out[r] = clamp((r - s0) ** 2 + g0)

    def pop(a, build):
        if a.q < a.low and mutation != 'pop_without_reload':
            a.low -= CHUNK
            for i in range(CHUNK):
                a.ring[(a.low + i) % RING] = a.spill[a.low + i]
            cnt['build_reloads' if build else 'read_reloads'] += a.mult
            a.reloaded = a.reloaded or build
        a.ts, a.tt, a.tg = a.ring[a.q % RING]
        a.tv = (a.tt - a.ts) ** 2 + a.tg

    def set_dn(a, e):
        a.dn_t = e[1]
        a.dn_v = (e[1] - e[0]) ** 2 + e[2]

    for u0 in range(1, m, AHEAD):
        while True:                                                      # the wave's collective loop over ballots
            has = [a.low > a.eb for a in lanes]
            fin = [h and u0 - a.dn_t >= 0 and a.dn_v <= (u0 - a.dn_t) ** 2 for a, h in zip(lanes, has)]
            if not any(has):
                break
            if fin != has:
                cnt['flush_blocked'] += sum(a.mult for a, f in zip(lanes, fin) if f)
                break
            for a, h in zip(lanes, has):
                if not h:
                    continue
                e = a.spill[a.eb:a.eb + CHUNK]
                for i in range(CHUNK):
                    rows_out(a, e[i][0], e[i][2], e[i][1], e[i + 1][1] if i + 1 < CHUNK else a.dn_t)
                a.ue = a.dn_t
                a.eb += CHUNK
                cnt['chunk_flush'] += a.mult
                a.flushed = True
                if a.low > a.eb:
                    spilled = a.eb + CHUNK < a.low
                    cnt['chunk_flush_next_spilled'] += a.mult * spilled
                    if mutation != 'stale_dn_after_flush':
                        set_dn(a, a.spill[a.eb + CHUNK] if spilled else a.ring[a.low % RING])
        for a in lanes:
            if a.low == a.eb and a.low < a.q:                            # the final bottom of the ring leaves
                p0 = a.ring[a.low % RING]
                while True:
                    p1 = a.ring[(a.low + 1) % RING]
                    dd = u0 - p1[1]
                    if not (dd >= 0 and (p1[1] - p1[0]) ** 2 + p1[2] <= dd * dd):
                        break
                    rows_out(a, p0[0], p0[2], p0[1], p1[1])
                    a.ue = p1[1]
                    a.low += 1
                    a.eb += 1
                    cnt['bottom_leaves'] += a.mult
                    p0 = p1
                    if a.low >= a.q:
                        break
            for u in range(u0, min(u0 + AHEAD, m)):
                Gu = a.G[u]
                while a.q >= a.eb:
                    if a.tv <= (a.tt - u) ** 2 + Gu:
                        break
                    a.q -= 1
                    if a.q >= a.eb:
                        pop(a, True)
                if a.q < a.eb:
                    if mutation is None:
                        assert a.eb == 0 and a.low == 0, 'a final entry was popped'
                    a.q = a.low = 0
                    a.ts, a.tt, a.tg, a.tv = u, 0, Gu, u * u + Gu
                    a.ring[0] = (u, 0, Gu)
                    cnt['reset'] += a.mult
                    continue
                num, den = (u + a.ts) * (u - a.ts) + Gu - a.tg, 2 * (u - a.ts)
                if divisions is not None:
                    divisions.append((num, den))
                w = 1 + num // den
                if mutation is None:
                    assert w > a.tt
                if w >= m:
                    cnt['not_pushed'] += a.mult
                    continue
                a.q += 1
                if a.q - a.low >= RING:
                    for i in range(CHUNK):
                        a.spill[a.low + i] = a.ring[(a.low + i) % RING]
                    a.low += CHUNK
                    cnt['spills'] += a.mult
                    cnt['spill_after_reload'] += a.mult * a.reloaded
                    cnt['spill_after_flush'] += a.mult * a.flushed
                    if a.low - a.eb == CHUNK:
                        set_dn(a, a.ring[a.low % RING])
                a.ts, a.tt, a.tg, a.tv = u, w, Gu, (w - u) ** 2 + Gu
                a.ring[a.q % RING] = (u, w, Gu)
                cnt['depth'] = max(cnt['depth'], a.q - a.eb + 1)
    for a in lanes:
        for u in range(m - 1, (0 if mutation == 'read_back_to_zero' else a.ue) - 1, -1):
            a.out[u] = clamp((u - a.ts) ** 2 + a.tg)
            if u == a.tt:
                a.q -= 1
                if a.q >= a.eb:
                    pop(a, False)
    cnt['depth'] = max(cnt['depth'], 1)
    rows = np.array([a.out for a in lanes], np.int64)[inverse]
    return rows, cnt


def brute_rows(lines, inf):
    """min_i (u - i)^2 + G(i), clamped at inf, for every line of [lanes][m]"""
    G = np.asarray(lines, np.int64)
    u = np.arange(G.shape[1], dtype=np.int64)
    return np.minimum(((u[:, None] - u[None, :]) ** 2 + G[:, None, :]).min(axis=2), inf)


def is_32bit(shape):
    """edt_squared's rule: 32-bit arithmetic where the squared diagonal is below 2^29"""
    return sum(int(n) ** 2 for n in shape) < INF32


def edt_inf(shape):
    return INF32 if is_32bit(shape) else INF64


def axis0_squared(mask, inf):
    """k_edt_axis0: the squared distance along axis 0 to the column's nearest zero voxel, inf for a column without one"""
    z = np.asarray(mask) == 0
    n0 = z.shape[0]
    idx = np.arange(n0, dtype=np.int64).reshape(-1, 1, 1)
    far = 1 << 40
    above = np.maximum.accumulate(np.where(z, idx, -far), axis=0)
    below = np.minimum.accumulate(np.where(z, idx, far)[::-1], axis=0)[::-1]
    g = np.minimum(idx - above, below - idx)
    return np.where(g >= far // 2, inf, g * g)


def plane_squared(mask, inf):
    """What pass 1 must leave: the squared distance to the nearest zero voxel of the voxel's own i2 plane (the oracle's
    transform of every plane: a correctly rounded root of an integer below 2^32, squared and rounded), inf without one."""
    nz = np.asarray(mask) != 0
    out = np.empty(nz.shape, np.int64)
    for i2 in range(nz.shape[2]):
        if nz[:, :, i2].all():
            out[:, :, i2] = inf
        else:
            d = MO.distance_transform_edt(nz[:, :, i2])
            out[:, :, i2] = np.rint(d * d).astype(np.int64)
    return out


def volume_squared(mask):
    d = MO.distance_transform_edt(mask)
    return np.rint(d * d).astype(np.int64)


def wave_items(vol, planes=None):
    """The items of an envelope pass over vol [n0][m][n2] (lines along axis 1, lanes on axis 2): ((i0, c), lines [64][m]),
    the lanes past the end of a row on its last line."""
    n0, m, n2 = vol.shape
    for i0 in (range(n0) if planes is None else planes):
        for c in range((n2 + LANES - 1) // LANES):
            i2 = np.minimum(c * LANES + np.arange(LANES), n2 - 1)
            yield (i0, c), np.ascontiguousarray(vol[i0][:, i2].T)


def pass_input(mask, which):
    """(volume the pass reads, volume it must write), both [n0][line][lanes], and the width's inf"""
    mask = np.asarray(mask)
    inf = edt_inf(mask.shape)
    if which == 1:
        return axis0_squared(mask, inf), plane_squared(mask, inf), inf
    return plane_squared(mask, inf).transpose(0, 2, 1), volume_squared(mask).transpose(0, 2, 1), inf


def trace_pass(mask, which, planes=None, mutation=None, divisions=None):
    """Trace the items of pass `which` (1: along axis 1, 2: along axis 2 on the transposed volume) in the given i0 planes.
    Returns (counters, wrong): wrong = the number of items whose rows differ from what the pass must write."""
    vin, vout, inf = pass_input(mask, which)
    total, wrong = new_counts(), 0
    for (i0, c), lines in wave_items(vin, planes):
        rows, cnt = trace_wave(lines, inf, mutation, divisions)
        add_counts(total, cnt)
        i2 = np.minimum(c * LANES + np.arange(LANES), vin.shape[2] - 1)
        wrong += not np.array_equal(rows, vout[i0][:, i2].T)
    return total, wrong
