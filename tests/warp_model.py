"""numpy restatement of the nonlinear-registration entries of include/vmask.h (``vmask_warp_*``, DESIGN.md section 9 entry f18): one
elementwise numpy operation per IEEE operation of the definition, sums as explicit ascending loops over an axis.  The fit and the
evaluation are those of tests/bias_model.py, the pyramid and the extrema those of tests/registration_model.py;
``register_nonlinear`` is the library's own host code (``registration.registerNonlinearWith``) over these functions instead of the
GPU's."""
import functools
import types

import numpy as np

import bias_model as B
import registration_model as RM
from arterynetwork_amd import registration as R


def _coords(T, u):
    """p_a at every voxel of the grid of the warp u [3, n0, n1, n2]."""
    T = np.asarray(T, dtype=np.float64)
    idx = RM._indices(tuple(u.shape[1:]))
    with np.errstate(invalid='ignore', over='ignore'):
        q = [idx[c] + u[c] for c in range(3)]
        return [((T[a, 0] * q[0] + T[a, 1] * q[1]) + T[a, 2] * q[2]) + T[a, 3] for a in range(3)]


def interpolant(moving, p):
    """(value, ok, (g0, g1, g2)) at the points p (three arrays of moving-voxel coordinates): the trilinear sample, where it is
    inside and finite, and the interpolant's gradient from the same 8 corners."""
    m = moving.shape
    shape = p[0].shape
    with np.errstate(invalid='ignore', over='ignore'):
        inside = np.ones(shape, bool)
        for a in range(3):
            inside &= (p[a] >= 0.0) & (p[a] <= float(m[a] - 1))
        f = [np.floor(np.where(inside, x, 0.0)) for x in p]
        t = [np.where(inside, x, 0.0) - fa for x, fa in zip(p, f)]
        lo = [fa.astype(np.int64) for fa in f]
        hi = [np.minimum(l + 1, n - 1) for l, n in zip(lo, m)]
        v = [[[moving[a, b, c].astype(np.float64) for c in (lo[2], hi[2])] for b in (lo[1], hi[1])] for a in (lo[0], hi[0])]
        x = [[v[a][b][0] + t[2] * (v[a][b][1] - v[a][b][0]) for b in (0, 1)] for a in (0, 1)]
        y = [x[a][0] + t[1] * (x[a][1] - x[a][0]) for a in (0, 1)]
        value = y[0] + t[0] * (y[1] - y[0])
        g0 = y[1] - y[0]
        e = [x[a][1] - x[a][0] for a in (0, 1)]
        g1 = e[0] + t[0] * (e[1] - e[0])
        d = [[v[a][b][1] - v[a][b][0] for b in (0, 1)] for a in (0, 1)]
        h = [d[a][0] + t[1] * (d[a][1] - d[a][0]) for a in (0, 1)]
        g2 = h[0] + t[0] * (h[1] - h[0])
    return value, inside & np.isfinite(value), (g0, g1, g2)


def sample(moving, T, u):
    """(value, ok) of the moving volume through T and the warp at every voxel of the warp's grid."""
    value, ok, _ = interpolant(moving, _coords(T, u))
    return value, ok


def force(fixed, moving, T, u, flo, fs, mlo, ms, maxStep=0.5, mask=None):
    """(delta [3, n0, n1, n2], part uint8, S, count) of ``vmask_warp_force``."""
    T = np.asarray(R._map12(T), dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    F = np.asarray(fixed).astype(np.float64)
    n0, n1, n2 = F.shape
    value, ok, g = interpolant(moving, _coords(T, u))
    part = ok & np.isfinite(F)
    if mask is not None:
        part &= np.asarray(mask) != 0
    a2 = 1.0 / ((4.0 * maxStep) * maxStep)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        r = (F - flo) * fs - (value - mlo) * ms
        G = [((g[0] * T[0, c] + g[1] * T[1, c]) + g[2] * T[2, c]) * ms for c in range(3)]
        rr = r * r
        den = ((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]) + rr * a2
        good = part & (den > 0.0) & np.isfinite(den)
        safe = np.where(good, den, 1.0)
        delta = np.stack([np.where(good, (r * G[c]) / safe, 0.0) for c in range(3)])
        colS = np.zeros((n1, n2))
        for x in range(n0):
            colS = np.where(part[x], colS + rr[x], colS)
        rowS = np.zeros(n2)
        for y in range(n1):
            rowS = rowS + colS[y]
        S = np.float64(0.0)
        for z in range(n2):
            S = S + rowS[z]
    return delta, part.astype(np.uint8), float(S), int(part.sum())


def fit3(delta, part, spans):
    """phi [3, K0, K1, K2]: the fit of bias_model per component."""
    return np.stack([B.fit(delta[c], part, spans) for c in range(3)])


def upsample(coarse, shape):
    """The warp of the next finer level: 2 x the trilinear sample of the coarse warp at clamp((i - 0.5) * 0.5, 0, c - 1)."""
    coarse = np.asarray(coarse, dtype=np.float64)
    c = coarse.shape[1:]
    lo, hi, t = [], [], []
    for a in range(3):
        x = np.clip((np.arange(shape[a], dtype=np.float64) - 0.5) * 0.5, 0.0, float(c[a] - 1))
        f = np.floor(x)
        lo.append(f.astype(np.int64))
        hi.append(np.minimum(f.astype(np.int64) + 1, c[a] - 1))
        t.append(x - f)
    t0, t1, t2 = t[0][:, None, None], t[1][None, :, None], t[2][None, None, :]
    out = []
    for comp in range(3):
        v = [[[coarse[comp][np.ix_(a, b, cc)] for cc in (lo[2], hi[2])] for b in (lo[1], hi[1])] for a in (lo[0], hi[0])]
        x = [[v[a][b][0] + t2 * (v[a][b][1] - v[a][b][0]) for b in (0, 1)] for a in (0, 1)]
        y = [x[a][0] + t1 * (x[a][1] - x[a][0]) for a in (0, 1)]
        out.append(2.0 * (y[0] + t0 * (y[1] - y[0])))
    return np.stack(out)


def resample(moving, T, u, order=1, fill=0):
    """``vmask_warp_resample``: the moving volume on the warp's grid."""
    T = R._map12(T)
    u = np.asarray(u, dtype=np.float64)
    p = _coords(T, u)
    if order == 1:
        value, ok, _ = interpolant(moving, p)
        return np.where(ok, value, float(fill))
    m = moving.shape
    with np.errstate(invalid='ignore', over='ignore'):
        q = [np.floor(x + 0.5) for x in p]
        inside = np.ones(u.shape[1:], bool)
        for a in range(3):
            inside &= (q[a] >= 0.0) & (q[a] <= float(m[a] - 1))
        at = [np.where(inside, x, 0.0).astype(np.int64) for x in q]
    return np.where(inside, moving[at[0], at[1], at[2]], np.asarray(fill).astype(moving.dtype)).astype(moving.dtype)


def level(fixed, moving, T, u, flo, fs, mlo, ms, spans, iterations=30, maxStep=0.5, threshold=0.01, mask=None):
    """``vmask_warp_field``: (the warp, rows (cost, count, max |dphi|))."""
    u = np.array(u, dtype=np.float64)
    rows = []
    for it in range(iterations):
        delta, part, S, count = force(fixed, moving, T, u, flo, fs, mlo, ms, maxStep, mask)
        if it == 0 and count == 0:
            raise ValueError('no voxel takes part')
        phi = fit3(delta, part, spans)
        u = u + np.stack([B.evaluate(phi[c], spans, u.shape[1:]) for c in range(3)])
        top = float(np.fmax.reduce(np.abs(phi).ravel(), initial=0.0))
        with np.errstate(invalid='ignore', divide='ignore'):
            rows.append((float(np.float64(S) / np.float64(count)), float(count), top))
        if top < threshold:
            break
    return u, np.array(rows, dtype=np.float64).reshape(-1, 3)


OPS = types.SimpleNamespace(extrema=RM.extrema, shrink=RM.shrink, zeros=lambda f: np.zeros((3,) + tuple(f.shape)), upsample=upsample,
                            level=level, result=lambda u: u)


def register_nonlinear(fixed, moving, **kw):
    return R.registerNonlinearWith(OPS, np.asarray(fixed), np.asarray(moving), **kw)


# ------------------------------------------------------------------ the phantom of the tests
RIMS = ((0.90, 100.0), (0.68, 60.0), (0.42, 60.0))          # three tissue classes: nested shells at these radii, each this much brighter
TEXTURE = 25.0                                              # a smooth pattern inside the head, about 9 voxels per period: structure in every direction
VESSELS = (((0.30, 0.35, 0.50), (0.70, 0.60, 0.45), 0.05, 80.0), ((0.55, 0.25, 0.30), (0.45, 0.75, 0.70), 0.04, 80.0))


def tissue(x, shape):
    """The three-class phantom with two vessels as a function of continuous voxel coordinates x (three arrays) of a grid of
    `shape`: classes 100 / 160 / 220 as nested ellipsoid shells with a wavy rim, edges two voxels soft, a smooth texture inside, background 0
    (shells alone would leave every displacement along a rim unobservable)."""
    c = [(np.asarray(x[a], dtype=np.float64) + 0.5) / shape[a] * 2.0 - 1.0 for a in range(3)]
    rho = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + 0.06 * np.sin(5.0 * c[0]) * np.cos(4.0 * c[1] + 3.0 * c[2])
    soft = 2.0 / min(shape)
    out = np.zeros(np.shape(c[0]))
    for radius, step in RIMS:
        out = out + step / (1.0 + np.exp((rho - radius) / soft))
    head = 1.0 / (1.0 + np.exp((rho - RIMS[0][0]) / soft))
    out = out + TEXTURE * head * np.sin(np.pi * c[0] * shape[0] / 9.0) * np.sin(np.pi * c[1] * shape[1] / 8.0 + 1.0) * np.sin(np.pi * c[2] * shape[2] / 8.5 + 2.0)
    for a, b, radius, step in VESSELS:                        # a soft tube between two points (fractions of the extent)
        a, b = np.array(a) * 2.0 - 1.0, np.array(b) * 2.0 - 1.0
        ab = b - a
        s = np.clip(sum((c[k] - a[k]) * ab[k] for k in range(3)) / float(ab @ ab), 0.0, 1.0)
        dist = np.sqrt(sum((c[k] - (a[k] + s * ab[k])) ** 2 for k in range(3)))
        out = out + step / (1.0 + np.exp((dist - radius) / (0.5 * soft)))
    return out


def true_warp(x, shape, peak=2.5):
    """A smooth known deformation at continuous fixed-voxel coordinates x: half a period of a sine per axis and component - far
    coarser than the finest lattice -, `peak` voxels at its largest."""
    s = [np.pi * (np.asarray(x[a], dtype=np.float64) + 0.5) / shape[a] for a in range(3)]
    return np.stack([peak * np.sin(s[0]) * np.sin(s[1] + 0.4) * np.cos(s[2]),
                     -0.8 * peak * np.cos(s[0] + 0.3) * np.sin(s[1]) * np.sin(s[2]),
                     0.6 * peak * np.sin(s[0] + 0.2) * np.cos(s[1]) * np.sin(s[2] + 0.5)])


@functools.lru_cache(maxsize=None)
def deformed_pair(shape=(40, 36, 33), mshape=None, seed=0, noise=0.01, other_grid=False):
    """(fixed, fixedAffine, moving, movingAffine, W, truth): the phantom, and the moving image another session makes of it - the
    tissue displaced by ``true_warp``, seen through the matrix W on a grid of its own (other_grid: another shape, spacing and a
    rotation), intensities 0.7 v + 20 and Gaussian noise of `noise` of the range.  truth [3, n0, n1, n2]: the warp in fixed voxels
    for which moving(T (v + truth(v))) = 0.7 fixed(v) + 20."""
    shape = tuple(shape)
    idx = RM._indices(shape)
    fixed = tissue(idx, shape)
    if other_grid:
        mshape = tuple(mshape or (44, 34, 38))
        fA, mA = RM.affine_of((1.0, 1.0, 1.2), shape), RM.affine_of((0.95, 1.1, 1.05), mshape, centre_at=(0.6, -0.4, 0.3))
        W = R.paramsToMatrix([1.2, -0.8, 0.6, np.deg2rad(4.0), np.deg2rad(-3.0), np.deg2rad(5.0)], 6, np.zeros(3))
    else:
        mshape = tuple(mshape or shape)
        fA, mA, W = np.eye(4), np.eye(4), np.eye(4)
    T = R.voxelMap(W, fA, mA)
    Tinv = np.linalg.inv(T)
    y = RM._indices(mshape)
    base = [((Tinv[a, 0] * y[0] + Tinv[a, 1] * y[1]) + Tinv[a, 2] * y[2]) + Tinv[a, 3] for a in range(3)]
    x = [b.copy() for b in base]
    for _ in range(40):                                       # x + truth(x) = T^-1 y: a contraction (|d truth| < 0.3)
        w = true_warp(x, shape)
        x = [base[a] - w[a] for a in range(3)]
    top = float(fixed.max())
    moving = 0.7 * tissue(x, shape) + 20.0 + noise * top * np.random.default_rng(seed).standard_normal(mshape)
    truth = true_warp(idx, shape)
    for a in (fixed, moving, fA, mA, W, truth):
        a.setflags(write=False)
    return fixed, fA, moving, mA, W, truth


def end_point_error(warp, truth, T, mask=None):
    """The mean distance, in moving voxels, between T (v + warp(v)) and T (v + truth(v)) over the mask."""
    T = np.asarray(T, dtype=np.float64)[:3, :3]
    d = np.asarray(warp) - np.asarray(truth)
    e = np.sqrt(sum((T[a, 0] * d[0] + T[a, 1] * d[1] + T[a, 2] * d[2]) ** 2 for a in range(3)))
    return float(e.mean() if mask is None else e[np.asarray(mask) != 0].mean())
