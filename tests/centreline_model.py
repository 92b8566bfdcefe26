"""Sequential model of the centreline splines ("f20 centreline splines"): the yardstick of
tests/test_centrelines.py.  The rules of include/vmask.h (vmask_centrelines) taken literally: numpy element-wise operations
where the contract is element-wise, Python loops over the recurrences, `morphometry_model.ordered_sum` wherever a wave sums.
Every function takes the number type `T` - np.float64 (the contract) or np.longdouble (the yardstick of the float64 run).

For a branch of n entries e_0 .. e_(n-1) (voxel coordinates) in the spacing h, end weight W, mu = 1 / lambda:
  y_i = (e_i - e_0) h;  u_0 = 0, u_(i+1) = u_i + sqrt((d0^2 + d1^2) + d2^2) with d = y_(i+1) - y_i;  hh_i = u_(i+1) - u_i, r_i = 1 / hh_i
  w = (W, 1, .., 1, W), v_i = 1 / w_i;  m = n - 2 unknowns j = 0 .. m - 1, s_j = r_j + r_(j+1)
  a0_j = ((r_j r_j) v_j + (s_j s_j) v_(j+1)) + (r_(j+1) r_(j+1)) v_(j+2)
  a1_j = -((s_j r_(j+1)) v_(j+1) + (r_(j+1) s_(j+1)) v_(j+2))  (j < m - 1),  a2_j = (r_(j+1) r_(j+2)) v_(j+2)  (j < m - 2), else 0
  R0_j = (hh_j + hh_(j+1)) / 3,  R1_j = hh_(j+1) / 6,  b_j = (y_(j+2) - y_(j+1)) r_(j+1) - (y_(j+1) - y_j) r_j  per axis
  d0 = mu R0 + a0, d1 = mu R1 + a1, d2 = a2; with L2_i = 0 for i < 2, L1_0 = 0 and 1 for a D, 0 for a z' before the first:
    L2_i = d2_(i-2) / D_(i-2);  L1_i = (d1_(i-1) - (L2_i D_(i-2)) L1_(i-1)) / D_(i-1);  D_i = (d0_i - (L1_i L1_i) D_(i-1)) - (L2_i L2_i) D_(i-2)
    z'_i = (b_i - L1_i z'_(i-1)) - L2_i z'_(i-2);  z_i = z'_i / D_i;  c_i = (z_i - L1_(i+1) c_(i+1)) - L2_(i+2) c_(i+2), 0 past the last
  q_i = rp_(i-1) (c_(i-2) - c_(i-1)) + rp_i (c_i - c_(i-1)), rp = r inside 0 .. n - 2 and c inside 0 .. m - 1, 0 elsewhere
  e_i = v_i q_i,  g_i = y_i - e_i,  gamma_(j+1) = mu c_j, gamma_0 = gamma_(n-1) = 0,  F = ordered sum of w_i ((e_i0^2 + e_i1^2) + e_i2^2)."""
import math

import numpy as np

from morphometry_model import ordered_sum

STEPS = 24
NAN = float('nan')


def scale(spacing):
    """-> (l2, l, lambda_lo, lambda_hi) of a spacing: l2 = ((h0^2 + h1^2) + h2^2) / 3, l = sqrt(l2), 2^-24 and 2^24 times l2 l."""
    h = [float(x) for x in spacing]
    l2 = ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]) / 3.0
    l = math.sqrt(l2)
    l3 = l2 * l
    return l2, l, l3 * 2.0 ** -24, l3 * 2.0 ** 24


def _norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _osum(x):
    return ordered_sum(list(x)) if len(x) else x.dtype.type(0)


class Prepared:
    pass


def prepare(coords, spacing, end_weight, T=np.float64):
    """The lambda-independent part of a branch: y, u, hh, r, w, v and the bands."""
    e = np.asarray(coords, np.int64).reshape(-1, 3)
    n = len(e)
    p = Prepared()
    p.T, p.n, p.m = T, n, n - 2
    h = np.asarray(spacing, np.float64).astype(T)
    p.y = (e - e[0]).astype(T) * h
    s = _norm3(p.y[1:] - p.y[:-1])
    u = np.zeros(n, T)
    for i in range(n - 1):
        u[i + 1] = u[i] + s[i]
    p.u = u
    p.hh = u[1:] - u[:-1]
    p.r = T(1) / p.hh
    p.w = np.ones(n, T)
    p.w[0] = p.w[-1] = T(end_weight)
    p.v = T(1) / p.w
    m, r, v, hh, y = p.m, p.r, p.v, p.hh, p.y
    if m > 0:
        s1 = r[:-1] + r[1:]
        p.a0 = ((r[:m] * r[:m]) * v[:m] + (s1 * s1) * v[1:m + 1]) + (r[1:m + 1] * r[1:m + 1]) * v[2:m + 2]
        p.a1, p.a2 = np.zeros(m, T), np.zeros(m, T)
        p.a1[:m - 1] = -((s1[:m - 1] * r[1:m]) * v[1:m] + (r[1:m] * s1[1:m]) * v[2:m + 1])
        p.a2[:m - 2] = (r[1:m - 1] * r[2:m]) * v[2:m]
        p.R0 = (hh[:m] + hh[1:m + 1]) / T(3)
        p.R1 = hh[1:m + 1] / T(6)
        p.b = (y[2:] - y[1:-1]) * r[1:, None] - (y[1:-1] - y[:-2]) * r[:-1, None]
    return p


def solve(p, lam):
    """-> (g, gamma, F) of the prepared branch at lambda."""
    T, n, m = p.T, p.n, p.m
    if m == 0:
        return p.y.copy(), np.zeros((n, 3), T), T(0)
    mu = T(1) / T(lam)
    d0, d1, d2 = mu * p.R0 + p.a0, mu * p.R1 + p.a1, p.a2
    L1, L2, z = np.zeros(m + 2, T), np.zeros(m + 2, T), np.zeros((m, 3), T)
    one, zero = T(1), T(0)
    Dm1 = Dm2 = one
    zm1 = zm2 = np.zeros(3, T)
    l1m1 = zero
    for i in range(m):
        l2 = d2[i - 2] / Dm2 if i >= 2 else zero
        l1 = (d1[i - 1] - (l2 * Dm2) * l1m1) / Dm1 if i >= 1 else zero
        D = (d0[i] - (l1 * l1) * Dm1) - (l2 * l2) * Dm2
        zz = (p.b[i] - l1 * zm1) - l2 * zm2
        z[i] = zz / D
        L1[i], L2[i] = l1, l2
        Dm2, Dm1, zm2, zm1, l1m1 = Dm1, D, zm1, zz, l1
    c = np.zeros((m + 2, 3), T)
    for i in range(m - 1, -1, -1):
        c[i] = (z[i] - L1[i + 1] * c[i + 1]) - L2[i + 2] * c[i + 2]
    cpad = np.zeros((n + 2, 3), T)
    cpad[2:n] = c[:m]
    rpad = np.zeros(n + 1, T)
    rpad[1:n] = p.r
    q = rpad[:n, None] * (cpad[:n] - cpad[1:n + 1]) + rpad[1:n + 1, None] * (cpad[2:n + 2] - cpad[1:n + 1])
    e = p.v[:, None] * q
    g = p.y - e
    gamma = np.zeros((n, 3), T)
    gamma[1:n - 1] = mu * c[:m]
    F = _osum(p.w * ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))
    return g, gamma, F


def search(p, lam_lo, lam_hi, target, trace=None):
    """-> (lambda, solves, capped): the largest trial value with F <= target.  `trace`, a list, receives (lambda, F) per trial and,
    last, the upper bracket kept (hi, F(hi))."""
    T = p.T
    if p.m == 0:
        return T(lam_hi), 1, 1
    F = solve(p, lam_hi)[2]
    if trace is not None:
        trace.append((lam_hi, F))
    if F <= target:
        return T(lam_hi), 1, 1
    lo, hi, F_up, moved = T(lam_lo), T(lam_hi), F, False
    for _ in range(STEPS):
        mid = np.sqrt(lo * hi)
        F = solve(p, mid)[2]
        if trace is not None:
            trace.append((mid, F))
        if F > target:
            hi, F_up = mid, F
        else:
            lo, moved = mid, True
    if trace is not None:
        trace.append((hi, F_up))
    capped = 0
    if not moved and solve(p, lo)[2] > target:
        capped = 2
    return lo, STEPS + 1, capped


def _canon(x):
    x = np.array(x)
    x[np.isnan(x)] = np.nan
    return x


def evaluate(p, g, gamma, origin):
    """-> (position, tangent, curvature, first derivative) at the entries; origin = e_0 h."""
    T, n = p.T, p.n
    hh = p.hh[:, None]
    d = np.zeros((n, 3), T)
    d[:-1] = (g[1:] - g[:-1]) / hh - (hh * (T(2) * gamma[:-1] + gamma[1:])) / T(6)
    d[-1] = (g[-1] - g[-2]) / hh[-1] + (hh[-1] * (gamma[-2] + T(2) * gamma[-1])) / T(6)
    nrm = _norm3(d)
    with np.errstate(invalid='ignore', divide='ignore'):
        tangent = _canon(d / nrm[:, None])
        s = gamma
        cr = np.stack([d[:, 1] * s[:, 2] - d[:, 2] * s[:, 1], d[:, 2] * s[:, 0] - d[:, 0] * s[:, 2], d[:, 0] * s[:, 1] - d[:, 1] * s[:, 0]], axis=1)
        curvature = _canon(_norm3(cr) / ((nrm * nrm) * nrm))
    return origin + g, tangent, curvature, d


def point(p, g, gamma, d, uk):
    """The cubic at the parameter uk: on the interval i = the last knot of 0 .. n - 2 with u_i <= uk, t = uk - u_i,
    g_i + t (d_i + t (gamma_i / 2 + t ((gamma_(i+1) - gamma_i) / (6 hh_i))))."""
    T = p.T
    i = min(max(int(np.searchsorted(p.u, uk, 'right')) - 1, 0), p.n - 2)
    t = uk - p.u[i]
    k3 = (gamma[i + 1] - gamma[i]) / (T(6) * p.hh[i])
    return g[i] + t * (d[i] + t * (T(0.5) * gamma[i] + t * k3))


def triangle(A, B, C):
    """curvature_by_triangle of the reference: the sides sorted a >= b >= c, (t > 0 ? sqrt(t) : 0) / ((a b) c)."""
    c, b, a = sorted([_norm3(A - B), _norm3(A - C), _norm3(B - C)])
    t = (((a + (b + c)) * (c - (a - b))) * (c + (a - b))) * (a + (b - c))
    s4 = np.sqrt(t) if t > 0 else type(t)(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return s4 / ((a * b) * c)


def sample(p, g, gamma, d, step):
    """-> (splineLength, maxCurvature, meanCurvature, samples)."""
    T = p.T
    U = p.u[-1]
    m = max(3, int(math.ceil(float(U / T(step)))) + 1)
    P = [point(p, g, gamma, d, (T(k) * U) / T(m - 1) if k < m - 1 else U) for k in range(m)]
    chords = [_norm3(P[k + 1] - P[k]) for k in range(m - 1)]
    kappa = [triangle(P[k - 1], P[k], P[k + 1]) for k in range(1, m - 1)]
    mx = T(0)
    for x in kappa:
        mx = np.fmax(mx, x)
    mean = ordered_sum(kappa) / T(m - 2)
    return ordered_sum(chords), mx, (T(NAN) if mean != mean else mean), m


def fit_branch(coords, spacing, end_weight=20.0, smoothing=None, residual_per_point=None, sample_step=None, T=np.float64, trace=None):
    """One branch -> dict: u, position, second, tangent, curvature (per entry), lambda, residual, splineLength, maxCurvature,
    meanCurvature, solves, capped, samples, and g (the centred fit)."""
    l2, l, lam_lo, lam_hi = scale(spacing)
    rho = 0.25 * l2 if residual_per_point is None else float(residual_per_point)
    step = 0.5 * l if sample_step is None else float(sample_step)
    p = prepare(coords, spacing, end_weight, T)
    if smoothing is None:
        lam, solves, capped = search(p, lam_lo, lam_hi, T(rho * float(p.n)), trace)
    else:
        lam, solves, capped = T(smoothing), 1, 0
    g, gamma, F = solve(p, lam)
    e0 = np.asarray(coords, np.int64).reshape(-1, 3)[0]
    origin = e0.astype(T) * np.asarray(spacing, np.float64).astype(T)
    pos, tangent, curvature, d = evaluate(p, g, gamma, origin)
    length, mx, mean, m = sample(p, g, gamma, d, step)
    return {'u': p.u, 'position': pos, 'second': gamma, 'tangent': tangent, 'curvature': curvature, 'lambda': lam, 'residual': F,
            'splineLength': length, 'maxCurvature': mx, 'meanCurvature': mean, 'solves': solves, 'capped': capped, 'samples': m, 'g': g, 'y': p.y}


ENTRY = ('u', 'position', 'second', 'tangent', 'curvature')
BRANCH_F64 = ('lambda', 'residual', 'splineLength', 'maxCurvature', 'meanCurvature')
BRANCH_INT = ('solves', 'capped', 'samples')


def centrelines(shape, offsets, voxels, spacing=(1.0, 1.0, 1.0), **kw):
    """Every branch of a table of linear indices -> dict of float64 / int64 arrays under the names above."""
    off = [int(x) for x in offsets]
    co = np.stack(np.unravel_index(np.asarray(voxels, np.int64), shape), axis=1).reshape(-1, 3) if len(voxels) else np.zeros((0, 3), np.int64)
    rows = [fit_branch(co[off[b]:off[b + 1]], spacing, **kw) for b in range(len(off) - 1)]
    out = {}
    for k in ENTRY:
        width = () if k in ('u', 'curvature') else (3,)
        out[k] = np.concatenate([np.asarray(r[k], np.float64).reshape((-1,) + width) for r in rows]) if rows else np.zeros((0,) + width)
    for k in BRANCH_F64:
        out[k] = np.array([float(r[k]) for r in rows], np.float64)
    for k in BRANCH_INT:
        out[k] = np.array([int(r[k]) for r in rows], np.int64)
    return out
