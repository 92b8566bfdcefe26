"""The bookkeeping of one line of k_ter_envelope (csrc/vter_device.hip), restated sequentially: the stack of (site, start, G),
the pop rule, the start formula, the ring of RING entries in LDS, the spill area in chunks of CHUNK entries, `low` and `q`.
No arithmetic width, no lanes: what it answers is WHICH PATHS a line takes - how deep the stack gets, how often a chunk is
spilled, how often one comes back while the stack is still being built and how often while it is read back - so that a test
case can state on the CPU which branch of the kernel it drives.  The storage is modelled too (ring slots, spill entries), so a
mutation of the bookkeeping (``reload=False``: load_top without its reload) gives the wrong winners here as it would there.
Test code only."""
import numpy as np

RING, CHUNK = 16, 8


class Trace:
    """depth: most entries on the stack at once; spills / build_reloads / read_reloads: chunks moved to the spill area, brought
    back by the pop loop of the build phase, brought back by the read-back loop; spills_after_reload: spills that follow the
    first build-phase reload; winners: per position the site whose parabola is lowest there (-1: the line has no site)."""
    __slots__ = ('depth', 'spills', 'build_reloads', 'read_reloads', 'spills_after_reload', 'winners')

    def __init__(self):
        self.depth = self.spills = self.build_reloads = self.read_reloads = self.spills_after_reload = 0
        self.winners = None

    def add(self, other):
        self.depth = max(self.depth, other.depth)
        for k in ('spills', 'build_reloads', 'read_reloads', 'spills_after_reload'):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        return self

    def counts(self):
        return {k: getattr(self, k) for k in self.__slots__ if k != 'winners'}


def trace_line(G, reload=True, divisions=None):
    """One line: G[u] >= 0 is the value that position u enters with, G[u] < 0 a position that enters no parabola.
    `divisions`, when a list, receives the (numerator, divisor) of every start formula that is evaluated."""
    G = [int(x) for x in G]
    m = len(G)
    ring = [None] * RING
    spill = [None] * ((m + CHUNK - 1) // CHUNK * CHUNK)
    t = Trace()
    q, low = -1, 0
    ts = tt = tg = 0

    def load_top(build):
        nonlocal low, ts, tt, tg
        if q < low and reload:
            low -= CHUNK
            for i in range(CHUNK):
                ring[(low + i) % RING] = spill[low + i]
            if build:
                t.build_reloads += 1
            else:
                t.read_reloads += 1
        ts, tt, tg = ring[q % RING]

    for u in [u for u in range(m) if G[u] >= 0]:
        Gu = G[u]
        while q >= 0 and (tt - ts) ** 2 + tg > (tt - u) ** 2 + Gu:
            q -= 1
            if q >= 0:
                load_top(True)
        w = 0
        if q >= 0:
            w = 1 + ((u + ts) * (u - ts) + Gu - tg) // (2 * (u - ts))
            if divisions is not None:
                divisions.append(((u + ts) * (u - ts) + Gu - tg, 2 * (u - ts)))
        if w < m:
            q += 1
            if q - low >= RING:
                for i in range(CHUNK):
                    spill[low + i] = ring[(low + i) % RING]
                low += CHUNK
                t.spills += 1
                t.spills_after_reload += t.build_reloads > 0
            ts, tt, tg = u, w, Gu
            ring[q % RING] = (u, w, Gu)
            t.depth = max(t.depth, q + 1)
    winners = np.full(m, -1, np.int64)
    end = m                                                            # the kernel walks u = m - 1 .. 0 and leaves the top at u == tt
    while q >= 0:
        winners[tt:end] = ts
        end = tt
        q -= 1
        if q >= 0:
            load_top(False)
    t.winners = winners
    return t


def brute_winners(G):
    """Per position the argmin over the sites s (G[s] >= 0) of (u - s)^2 + G[s], the smaller s of equal values."""
    G = np.asarray(G, np.int64)
    sites = np.flatnonzero(G >= 0)
    if not len(sites):
        return np.full(len(G), -1, np.int64)
    u = np.arange(len(G), dtype=np.int64)
    return sites[((u[:, None] - sites[None, :]) ** 2 + G[sites][None, :]).argmin(axis=1)]


def _row_d2(sites, cs):
    """min over the sites of a row of (c - s)^2 for every c of cs, -1 for a row without a site"""
    if not len(sites):
        return np.full(len(cs), -1, np.int64)
    return ((cs[:, None] - sites[None, :]) ** 2).min(axis=1)


def axis1_lines(skeleton, inner=None):
    """The lines of the axis-1 pass: ((o, c), G) with G[u] = (c - f)^2, f the nearest site of row (o, u), for every plane o and
    every c of `inner` (default: all i2)."""
    sk = np.asarray(skeleton) != 0
    n0, n1, n2 = sk.shape
    cs = np.arange(n2, dtype=np.int64) if inner is None else np.asarray(inner, np.int64)
    for o in range(n0):
        g = np.stack([_row_d2(np.flatnonzero(sk[o, u]).astype(np.int64), cs) for u in range(n1)])      # [u][c]
        for k, c in enumerate(cs.tolist()):
            yield (o, c), g[:, k]


def axis0_lines(skeleton, inner=None):
    """The lines of the axis-0 pass: ((0, c), G), c = i1 * n2 + i2 over `inner` (default: all), G[u] = the squared distance
    inside plane u from (i1, i2) to the plane's nearest site, -1 for a plane without one (a direct minimum over its sites)."""
    sk = np.asarray(skeleton) != 0
    n0, n1, n2 = sk.shape
    cs = np.arange(n1 * n2, dtype=np.int64) if inner is None else np.asarray(inner, np.int64)
    i1, i2 = cs // n2, cs % n2
    g = np.full((n0, len(cs)), -1, np.int64)
    for u in range(n0):
        s1, s2 = np.nonzero(sk[u])
        if len(s1):
            g[u] = ((i1[:, None] - s1[None, :]) ** 2 + (i2[:, None] - s2[None, :]) ** 2).min(axis=1)
    for k, c in enumerate(cs.tolist()):
        yield (0, c), g[:, k]


def trace_pass(lines, reload=True, divisions=None):
    """The sum of the lines' traces (depth: the maximum), and the traces by (o, c)."""
    total, each = Trace(), {}
    for key, G in lines:
        each[key] = trace_line(G, reload, divisions)
        total.add(each[key])
    return total, each
