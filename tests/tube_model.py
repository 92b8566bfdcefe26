"""Brute-force model of vmask_tubes (include/vmask.h, DESIGN.md section 9 "f21 tube model"): the yardstick of tests/test_tubes.py.

Every voxel against every primitive of a kept branch, numpy element-wise float64 operations in the order that vmask.h writes
(numpy rounds every operation on its own and fuses nothing); no boxes, no bricks, no lists.  The winner is the first minimum
(``argmin``) over the primitives in ascending e of f where f <= 0, +inf elsewhere: the lexicographically least (f, e)."""
import numpy as np

BLOCK = 16          # primitives evaluated at a time (a BLOCK x V float64 matrix)


def power(x, A, B, rA, rB):
    """f of vmask.h at the points x (3 arrays of one shape) for the primitives A, B (K x 3), rA, rB (K): K x shape."""
    ex = (slice(None),) + (None,) * np.ndim(x[0])
    A0, A1, A2 = (np.asarray(A, np.float64)[:, k][ex] for k in range(3))
    B0, B1, B2 = (np.asarray(B, np.float64)[:, k][ex] for k in range(3))
    rA, rB = np.asarray(rA, np.float64)[ex], np.asarray(rB, np.float64)[ex]
    x0, x1, x2 = (np.asarray(v, np.float64)[None] for v in x)
    d0, d1, d2 = B0 - A0, B1 - A1, B2 - A2
    dd = (d0 * d0 + d1 * d1) + d2 * d2
    w0, w1, w2 = x0 - A0, x1 - A1, x2 - A2
    wd = (w0 * d0 + w1 * d1) + w2 * d2
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        t = np.where(dd == 0.0, 0.0, wd / np.where(dd == 0.0, 1.0, dd))
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t > 1.0, 1.0, t)
        c0, c1, c2 = A0 + t * d0, A1 + t * d1, A2 + t * d2
        q0, q1, q2 = x0 - c0, x1 - c1, x2 - c2
        qq = (q0 * q0 + q1 * q1) + q2 * q2
        rho = rA + t * (rB - rA)
        return qq - rho * rho


def primitives(offsets, keep=None):
    """The entries e that start a primitive of a kept branch, ascending, and the branch of each."""
    offsets = np.asarray(offsets, np.int64)
    e, b = [], []
    for k in range(len(offsets) - 1):
        if keep is None or keep[k]:
            e.append(np.arange(offsets[k], offsets[k + 1] - 1))
            b.append(np.full(offsets[k + 1] - 1 - offsets[k], k))
    if not e:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(e).astype(np.int64), np.concatenate(b).astype(np.int64)


def tubes(shape, offsets, positions, radius, spacing=None, keep=None, labels=None, mask=None):
    """A dict with label (int32), field (float64), nearest (int64), sizes and overlap (int64, per branch) and missed (int)."""
    h = np.ones(3) if spacing is None else np.asarray(spacing, np.float64)
    P, r = np.asarray(positions, np.float64).reshape(-1, 3), np.asarray(radius, np.float64).reshape(-1)
    B = len(offsets) - 1
    idx = np.indices(shape).reshape(3, -1)
    x = [idx[a].astype(np.float64) * h[a] for a in range(3)]
    V = idx.shape[1]
    best, who = np.full(V, np.inf), np.full(V, -1, np.int64)
    es, bs = primitives(offsets, keep)
    for k in range(0, len(es), BLOCK):
        e = es[k:k + BLOCK]
        f = power(x, P[e], P[e + 1], r[e], r[e + 1])
        f = np.where(f <= 0.0, f, np.inf)
        first = np.argmin(f, axis=0)                                    # the first of equal minima: the smallest e of the block
        fmin = f[first, np.arange(V)]
        better = fmin < best                                            # (an earlier block keeps a tie: its e is smaller)
        best = np.where(better, fmin, best)
        who = np.where(better, e[first], who)
    branch_of = np.full(len(r) + 1, -1, np.int64)
    branch_of[es] = bs
    won = who >= 0
    lab = np.arange(1, B + 1, dtype=np.int64) if labels is None else np.asarray(labels, np.int64)
    label = np.zeros(V, np.int32)
    label[won] = lab[branch_of[who[won]]]
    m = np.zeros(V, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    sizes = np.bincount(branch_of[who[won]], minlength=B).astype(np.int64)
    overlap = np.bincount(branch_of[who[won & m]], minlength=B).astype(np.int64)
    return {'label': label.reshape(shape), 'field': best.reshape(shape), 'nearest': who.reshape(shape), 'sizes': sizes, 'overlap': overlap,
            'missed': int((m & ~won).sum())}


def capsule_volume(R, L):
    return np.pi * R * R * L + 4.0 / 3.0 * np.pi * R ** 3


def cone_volume(r1, r2, L):
    """The set f <= 0 of one primitive: the frustum whose section at the foot point t has radius r1 + t (r2 - r1), and a half ball
    at each end."""
    return np.pi * L / 3.0 * (r1 * r1 + r1 * r2 + r2 * r2) + 2.0 / 3.0 * np.pi * (r1 ** 3 + r2 ** 3)
