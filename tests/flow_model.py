"""Models of the network flow solve ("f13 flow"; include/vmask.h, vmask_flow).

Two variants of one outer iteration (Todini's global gradient algorithm) for the law P_u - P_v = R |Q|^(k-1) Q:

  solve_direct   (a) the inner linear systems by scipy.sparse.linalg.spsolve, run to a tolerance of 1e-13: the yardstick for k != 1
  solve          (b) a sequential restatement of the kernel's own arithmetic - the incidence order, the summation orders of
                 include/vmask.h, the same Jacobi-preconditioned conjugate gradients; numpy where every elementwise operation is
                 one IEEE operation and every sum is formed in the stated order.  At k = 1 it equals the kernel bit for bit.

Both take one scenario: ends (B x 2), fixed (N, 0/1), R (B), pressure (N, read at the fixed nodes)."""
import numpy as np

T = 256                                                                   # the workgroup's thread count
EPS_INNER = 1e-8                                                          # the inner rule: sqrt(r.z) down by this factor
FLOOR_FACTOR = 0.01                                                       # the floor of |Q| in g: FLOOR_FACTOR * tol * max |Q|


class Topology:
    """What the library derives from the graph on the host: which branches take part, the components without a fixed node, the
    free nodes ascending, every free node's anchor (the smallest fixed node of its component) and the node-major incidence list
    (per node its participating branches in ascending branch index)."""

    def __init__(self, ends, fixed, nnode):
        ends = np.asarray(ends, np.int64).reshape(-1, 2)
        fixed = np.asarray(fixed).astype(bool).reshape(-1)
        N, B = int(nnode), len(ends)
        assert len(fixed) == N
        part = (ends[:, 0] >= 0) & (ends[:, 0] != ends[:, 1])
        parent = list(range(N))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for u, v in ends[part].tolist():
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
        root = np.array([find(v) for v in range(N)], np.int64)
        anchor_of = np.full(N, -1, np.int64)
        for v in np.flatnonzero(fixed)[::-1].tolist():
            anchor_of[root[v]] = v
        self.anchor = anchor_of[root] if N else np.zeros(0, np.int64)
        self.floating = self.anchor < 0
        self.fixed = fixed
        self.free = np.flatnonzero(~fixed & ~self.floating)
        self.floating_components = int(len(np.unique(root[self.floating])))
        self.part = part.copy()
        self.part[part] = ~self.floating[ends[part, 0]]
        self.ends, self.N, self.B = ends, N, B
        b = np.flatnonzero(self.part)
        node = np.concatenate([ends[b, 0], ends[b, 1]])
        branch = np.concatenate([b, b])
        side = np.concatenate([np.zeros(len(b), np.int64), np.ones(len(b), np.int64)])
        other = np.concatenate([ends[b, 1], ends[b, 0]])
        order = np.lexsort((side, branch, node))
        self.inc_branch, self.inc_sign, self.inc_other = branch[order], (1.0 - 2.0 * side[order]), other[order]
        self.inc_off = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=N))]).astype(np.int64)
        self.degree = np.diff(self.inc_off)


def block_sum(v):
    """The sum of v_0 .. v_(n-1) as the workgroup forms it: thread t adds v_t, v_(t+T), .. to 0.0 in sequence; every wave of 64
    threads runs the xor tree 32, 16, .. 1; the four wave sums w are added as ((w0 + w1) + w2) + w3."""
    v = np.asarray(v, np.float64)
    rows = -(-len(v) // T) if len(v) else 0
    pad = np.zeros(max(rows, 1) * T)
    pad[:len(v)] = v
    acc = np.zeros(T)
    for row in pad.reshape(-1, T)[:rows]:
        acc = acc + row
    a = acc.reshape(T // 64, 64)
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ s]
    w = a[:, 0]
    total = w[0]
    for x in w[1:]:
        total = total + x
    return float(total)


def row_sums(top, nodes, terms):
    """Per node of `nodes` the sum of its incidence entries' `terms` (one per entry of the incidence list), added to 0.0 in the
    list's order."""
    acc = np.zeros(len(nodes))
    off, deg = top.inc_off[nodes], top.degree[nodes]
    for d in range(int(deg.max()) if len(nodes) else 0):
        has = deg > d
        acc[has] = acc[has] + terms[off[has] + d]
    return acc


def law_flow(delta, R, k):
    if k == 1.0:
        return delta / R
    return np.copysign(np.power(np.abs(delta) / R, 1.0 / k), delta)


def conductance(Q, R, k, tol, qm):
    """g = 1 / (k R max(|Q|, floor)^(k-1)); 1 / R where the floor is 0."""
    floor = (FLOOR_FACTOR * tol) * qm
    a = np.maximum(np.abs(Q), floor)
    with np.errstate(divide='ignore'):
        return np.where(a > 0.0, 1.0 / ((k * R) * np.power(a, k - 1.0)), 1.0 / R)


class Result:
    pass


def _finish(top, P, flow, converged, outer, inner, rel):
    out = Result()
    out.pressure, out.flow, out.converged, out.outer, out.inner, out.residual = P, flow, converged, outer, inner, rel
    out.floating = top.floating_components
    return out


def _start(top, pressure):
    P = np.full(top.N, np.nan)
    P[top.fixed] = np.asarray(pressure, np.float64)[top.fixed]
    P[top.free] = np.asarray(pressure, np.float64)[top.anchor[top.free]]
    return P


def solve(ends, fixed, R, pressure, k=1.852, tol=1e-10, max_iter=50, nnode=None):
    """Variant (b): the kernel's arithmetic, one scenario."""
    k, tol = float(k), float(tol)
    top = Topology(ends, fixed, len(np.asarray(fixed).reshape(-1)) if nnode is None else nnode)
    R = np.asarray(R, np.float64)
    P = _start(top, pressure)
    free, part = top.free, top.part
    u, v = top.ends[:, 0], top.ends[:, 1]
    c = 1.0 - 1.0 / k
    cap = 2 * len(free) + 64
    e_lo, e_hi = top.inc_off[:-1], top.inc_off[1:]
    ent_node = np.repeat(np.arange(top.N), top.degree)
    eb, es, eo = top.inc_branch, top.inc_sign, top.inc_other
    Q = np.zeros(top.B)
    flow = np.zeros(top.B)
    g = np.zeros(top.B)
    qm = 0.0
    outer = inner = 0
    converged, rel = False, np.inf
    while outer < max_iter:
        linear = k == 1.0 or outer == 0
        if linear:
            g[part] = 1.0 / R[part]
        else:
            g[part] = conductance(Q[part], R[part], k, tol, qm)
        sd = row_sums(top, free, g[eb] * (P[ent_node] - P[eo]))
        diag = row_sums(top, free, g[eb])
        if linear:
            r = 0.0 - sd
        else:
            r = (0.0 - c * row_sums(top, free, es * Q[eb])) - sd
        z = r / diag
        p = np.zeros(top.N)
        p[free] = z
        rz = block_sum(r * z)
        thresh = (EPS_INNER * EPS_INNER) * rz
        it = 0
        while it < cap and rz > thresh:
            Ap = row_sums(top, free, g[eb] * (p[ent_node] - p[eo]))
            pAp = block_sum(p[free] * Ap)
            if not pAp > 0.0:
                break
            alpha = rz / pAp
            P[free] = P[free] + alpha * p[free]
            r = r - alpha * Ap
            z = r / diag
            rz_new = block_sum(r * z)
            beta = rz_new / rz
            rz = rz_new
            p[free] = z + beta * p[free]
            it += 1
        inner += it
        delta = P[u[part]] - P[v[part]]
        flow[part] = law_flow(delta, R[part], k)
        if k != 1.0:
            Q[part] = flow[part] if outer == 0 else c * Q[part] + g[part] * delta
            qm = float(np.abs(Q[part]).max()) if part.any() else 0.0
        qmax = float(np.abs(flow[part]).max()) if part.any() else 0.0
        res = row_sums(top, free, es * flow[eb])
        res = float(np.abs(res).max()) if len(free) else 0.0
        outer += 1
        rel = res / qmax if qmax > 0.0 else (0.0 if res == 0.0 else np.inf)
        if res <= tol * qmax:
            converged = True
            break
    return _finish(top, P, flow, converged, outer, inner, rel)


def solve_direct(ends, fixed, R, pressure, k=1.852, tol=1e-13, max_iter=100, nnode=None):
    """Variant (a): the same outer iteration, the linear systems assembled and solved by spsolve; the floor of |Q| is 1e-20 of the
    largest, sums by numpy."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    k = float(k)
    top = Topology(ends, fixed, len(np.asarray(fixed).reshape(-1)) if nnode is None else nnode)
    R = np.asarray(R, np.float64)
    P = _start(top, pressure)
    free, part = top.free, top.part
    b = np.flatnonzero(part)
    u, v = top.ends[b, 0], top.ends[b, 1]
    col = np.full(top.N, -1, np.int64)
    col[free] = np.arange(len(free))
    nf = len(free)
    inc = sp.csr_matrix((np.concatenate([np.ones(len(b)), -np.ones(len(b))]), (np.concatenate([u, v]), np.concatenate([np.arange(len(b))] * 2))),
                        shape=(top.N, len(b)))                           # node x branch, +1 at the first end
    inc_free = inc[free]
    c = 1.0 - 1.0 / k
    Q = np.zeros(len(b))
    flow = np.zeros(top.B)
    outer = 0
    converged, rel = False, np.inf
    best = None
    while outer < max_iter:
        if k == 1.0 or outer == 0:
            g = 1.0 / R[b]
            rhs_q = np.zeros(nf)
        else:
            a = np.maximum(np.abs(Q), 1e-20 * np.abs(Q).max())
            with np.errstate(divide='ignore'):
                g = np.where(a > 0.0, 1.0 / (k * R[b] * np.power(a, k - 1.0)), 1.0 / R[b])
            rhs_q = -c * (inc_free @ Q)
        if nf:
            A = (inc_free @ sp.diags(g) @ inc_free.T).tocsc()
            known = np.where(top.fixed, P, 0.0)
            rhs = rhs_q - inc_free @ (g * (inc.T @ known))
            P[free] = np.atleast_1d(spsolve(A, rhs))
        delta = P[u] - P[v]
        q_law = law_flow(delta, R[b], k)
        if k != 1.0:
            Q = q_law.copy() if outer == 0 else c * Q + g * delta
        qmax = float(np.abs(q_law).max()) if len(b) else 0.0
        res = float(np.abs(inc_free @ q_law).max()) if nf else 0.0
        outer += 1
        this = res / qmax if qmax > 0.0 else 0.0
        if best is None or this < best[0]:
            best = (this, P.copy(), q_law.copy())
        rel = this
        if res <= tol * qmax:
            converged = True
            break
        if outer > 12 and this > best[0]:                                 # rounding level reached: the best iterate stands
            break
    rel, P, q_law = best
    flow[b] = q_law
    return _finish(top, P, flow, converged, outer, 0, rel)


# ---------------------------------------------------------------------- graphs for the tests
def random_tree(nfree, seed, extra=0):
    """A random tree of `nfree` inner nodes, every one with at least one leaf: node 0 is the inlet, the inner nodes follow, the
    leaves last.  `extra` more branches between inner nodes close loops.  Returns ends, fixed."""
    rng = np.random.default_rng(seed)
    ends = [[0, 1]]
    for i in range(2, nfree + 1):
        ends.append([int(rng.integers(1, i)), i])
    n = nfree + 1
    for i in range(1, nfree + 1):
        for _ in range(1 + int(rng.integers(0, 2))):
            ends.append([i, n] if rng.integers(0, 2) else [n, i])
            n += 1
    for _ in range(extra):
        a, b = rng.choice(np.arange(1, nfree + 1), 2, replace=False)
        ends.append([int(a), int(b)])
    fixed = np.ones(n, np.uint8)
    fixed[1:nfree + 1] = 0
    return np.array(ends, np.int64), fixed


def comb(nfree):
    """A backbone of `nfree` inner nodes behind the inlet (node 0), a tooth to a terminal at every one."""
    ends = [[i, i + 1] for i in range(nfree)] + [[i + 1, nfree + 1 + i] for i in range(nfree)]
    fixed = np.ones(2 * nfree + 1, np.uint8)
    fixed[1:nfree + 1] = 0
    return np.array(ends, np.int64), fixed


def inputs_for(ends, fixed, seed, level=0.0):
    """Resistances in [0.5, 2) and fixed pressures: 1 at node 0 (the inlet), `level` (1 - i / n) at the i-th of the n other fixed
    nodes."""
    R = 0.5 + 1.5 * np.random.default_rng(seed).random(len(ends))
    where = np.flatnonzero(np.asarray(fixed))
    P = np.zeros(len(fixed))
    P[where] = level * (1.0 - np.arange(len(where)) / len(where))
    P[0] = 1.0
    return R, P


def balance_limit(result, ends, R, k):
    """What the number format leaves of the flow balance: a stored pressure is uncertain by half a unit in its last place, and
    the law turns that into a flow error of dQ/dD = 1 / (k R |Q|^(k-1)) times as much - without bound where a branch is close to
    balance (Q -> 0) and k > 1.  Returns the largest such error over the branches, relative to the largest flow.  A tolerance
    below it cannot be met by any solver that returns the pressures as doubles."""
    ends = np.asarray(ends, np.int64).reshape(-1, 2)
    Q, P = np.abs(result.flow), result.pressure
    b = np.flatnonzero(Q > 0)
    if not len(b):
        return 0.0
    ulp = 2.0 ** -53 * np.nanmax(np.abs(P[ends[b]]), axis=1)
    return float((ulp / (k * np.asarray(R)[b] * Q[b] ** (k - 1.0))).max() / Q.max())
