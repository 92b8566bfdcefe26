"""The oracles of vmask_diffuse and vmask_median (include/vmask.h, DESIGN.md section 9 entry f14).

``diffuse`` restates the diffusion in numpy: float64 arrays, one elementwise numpy operation per IEEE operation of the
definition, in its association; neighbours by ``np.take`` with clamped indices; 1.0 / h and 1.0 / K formed once.  With the
rational conductance every operation is correctly rounded on any IEEE machine, so the GPU must return the same bits; the
exponential one goes through the platform's exp.  ``median_explicit`` gathers the clamped window and sorts it - it pins the
clamping against scipy's mode='nearest'."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.ndimage as ndi

FUNCTIONS = {'rational': 0, 'exponential': 1}


def bound(spacing=None):
    """B = 1 / (2 sum ih_a^2) in the library's operations."""
    ih = 1.0 / (np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64))
    return 1.0 / (2.0 * ((ih[0] * ih[0] + ih[1] * ih[1]) + ih[2] * ih[2]))


def step(u, ih, iK, dt, function):
    acc = np.zeros(u.shape, np.float64)
    for axis in range(3):
        n = u.shape[axis]
        for shift in (-1, 1):
            q = np.take(u, np.clip(np.arange(n) + shift, 0, n - 1), axis=axis)
            d = q - u
            g = d * ih[axis]
            t = g * iK
            tt = t * t
            c = 1.0 / (1.0 + tt) if function == 0 else np.exp(-tt)
            acc = acc + (c * g) * ih[axis]
    return u + dt * acc


def diffuse(volume, K, iterations=5, time_step=None, spacing=None, function='rational', slab=None):
    """u after `iterations` steps.  `slab`: compute every step in pieces of that many planes of axis 0, each with its two
    neighbouring planes, eight pieces at a time - the same per-voxel arithmetic on arrays that fit a cache, for the large case."""
    u = np.asarray(volume).astype(np.float64)
    ih = 1.0 / (np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64))
    iK = 1.0 / np.float64(K)
    dt = np.float64(time_step) if time_step is not None and time_step > 0 else 0.5 * bound(spacing)
    n0 = u.shape[0]
    for _ in range(iterations):
        if slab is None:
            u = step(u, ih, iK, dt, FUNCTIONS[function])
            continue
        new = np.empty_like(u)

        def piece(a, u=u, new=new):
            b, lo, hi = min(a + slab, n0), max(a - 1, 0), min(a + slab + 1, n0)
            new[a:b] = step(u[lo:hi], ih, iK, dt, FUNCTIONS[function])[a - lo:b - lo]
        with ThreadPoolExecutor(8) as pool:              # (numpy releases the interpreter lock inside its loops)
            list(pool.map(piece, range(0, n0, slab)))
        u = new
    return u


def median_explicit(volume, radius):
    """The median of the clamped (2 r0 + 1) x (2 r1 + 1) x (2 r2 + 1) window: gather, sort, take the middle."""
    v = np.asarray(volume)
    idx = [np.arange(n) for n in v.shape]
    window = []
    for a in range(-radius[0], radius[0] + 1):
        for b in range(-radius[1], radius[1] + 1):
            for c in range(-radius[2], radius[2] + 1):
                i0, i1, i2 = (np.clip(i + s, 0, n - 1) for i, s, n in zip(idx, (a, b, c), v.shape))
                window.append(v[np.ix_(i0, i1, i2)])
    window = np.sort(np.stack(window), axis=0)
    return window[len(window) // 2]


def median_scipy(volume, radius):
    return ndi.median_filter(np.asarray(volume), size=tuple(2 * r + 1 for r in radius), mode='nearest')


def step_phantom(shape=(16, 20, 18), seed=7, sigma=5.0):
    """(clean, noisy): the planes [:, 10:, :] at 100, Gaussian noise on every voxel."""
    clean = np.zeros(shape)
    clean[:, 10:, :] = 100.0
    return clean, clean + np.random.default_rng(seed).normal(0.0, sigma, shape)
