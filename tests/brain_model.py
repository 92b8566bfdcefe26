"""The oracle of the skull stripping (include/vmask.h ``vmask_brain_*``, DESIGN.md section 9 entry f17): the definition's steps
1-7 in numpy / scipy, and the head phantom that the definition was measured on.

The Laplacian of Gaussian comes twice: ``log_scipy`` as sums of ``scipy.ndimage.gaussian_filter(order=..., mode='nearest',
truncate=4.0)``, and ``log_restated`` as the device's arithmetic, one elementwise numpy operation per IEEE operation in its
association - the taps through ``math.exp``, the C library's exp that the host code calls, and summed in sequence.  The GPU must
return the bits of the second.  Steps 5-7 are scipy.ndimage's binary_erosion / binary_dilation / label / binary_fill_holes.

What the definition needs, measured on the phantom below (tests/test_brain.py asserts it): with the edge term the Dice against
the true brain is 0.992 .. 1.000 over both shapes, csf 15 and 55, noise 0, 3, 6, seeds 0-2, with
diffusion=dict(conductance=20, iterations=3); with the edge term off the csf = 55 cases fall to 0.52 / 0.56, scalp and brain
merging; and WITHOUT THE DIFFUSION the noisy cases of the second shape fail (Dice 0.515): the edge term needs the diffusion on
noisy data."""
import math

import numpy as np
import scipy.ndimage as ndi

import denoise_model

CROSS = ndi.generate_binary_structure(3, 1)
STAGES = ('candidate', 'eroded', 'main', 'closed', 'final')


# ------------------------------------------------------------------ steps 1 and 2
def histogram(J):
    """(lo, hi, 256 counts): b = min(255, floor((v - lo) * (256 / (hi - lo)))) in float64."""
    v = np.asarray(J).astype(np.float64)
    lo, hi = v.min(), v.max()
    if not hi > lo:
        raise ValueError('constant volume')
    s = 256.0 / (hi - lo)
    b = np.minimum(255.0, np.floor((v - lo) * s)).astype(np.int64)
    return float(lo), float(hi), np.bincount(b.ravel(), minlength=256).astype(np.uint64)


def otsu_table(counts):
    """(between-class variance, mu1 - mu0) at t = 0..254, float64; 0 where a class is empty."""
    c = np.asarray(counts).astype(np.float64)
    W0 = np.cumsum(c)[:255]
    m = np.cumsum(np.arange(256, dtype=np.float64) * c)
    M, m = m[255], m[:255]
    W1 = c.sum() - W0
    ok = (W0 > 0) & (W1 > 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        num = m * W1 - (M - m) * W0
        return np.where(ok, num * num / (W0 * W1), 0.0), np.where(ok, (M - m) / W1 - m / W0, 0.0)


def floor_contrast(counts, lo, hi, floor=None):
    """(floor, contrast, t): Otsu's t* and floor = lo + (t* + 1) w; a given floor is kept and t is the largest one with
    lo + (t + 1) w <= floor, clamped to 0..254; contrast = (mu1 - mu0) w at that t."""
    w = (hi - lo) / 256.0
    between, gap = otsu_table(counts)
    if floor is None:
        t = int(np.argmax(between))
        floor = lo + (t + 1) * w
    else:
        t = 0
        for k in range(255):
            if lo + (k + 1.0) * w <= floor:
                t = k
    return float(floor), float(gap[t] * w), t


def otsu_brute(counts):
    """t* by a loop over the thresholds with exact integers: the first t that maximises
    (m W1 - (M - m) W0)^2 / (W0 W1), compared as fractions."""
    c = [int(x) for x in counts]
    N, M = sum(c), sum(k * x for k, x in enumerate(c))
    best, best_t = (0, 1), 0
    W0 = m = 0
    for t in range(255):
        W0 += c[t]
        m += t * c[t]
        W1 = N - W0
        if W0 == 0 or W1 == 0:
            continue
        num, den = (m * W1 - (M - m) * W0) ** 2, W0 * W1
        if num * best[1] > best[0] * den:
            best, best_t = (num, den), t
    return best_t


# ------------------------------------------------------------------ step 3
def taps(s):
    """(r, phi, phi'') for a sigma of s voxels, as the host code forms them."""
    r = int(4.0 * s + 0.5)
    e = [math.exp(-0.5 * float(x) * x / (s * s)) for x in range(-r, r + 1)]
    total = 0.0
    for v in e:
        total += v
    phi = [v / total for v in e]
    phi2 = [(float(x) * x / (s * s * s * s) - 1.0 / (s * s)) * p for x, p in zip(range(-r, r + 1), phi)]
    return r, np.array(phi), np.array(phi2)


def axis_pass(I, w, axis):
    """out[i] = sum over k = -r..r ascending, from +0.0, of w[k] * I[clamp(i - k)] along `axis`."""
    r = (len(w) - 1) // 2
    n = I.shape[axis]
    out = np.zeros(I.shape, np.float64)
    for k in range(-r, r + 1):
        out = out + w[k + r] * np.take(I, np.clip(np.arange(n) - k, 0, n - 1), axis=axis)
    return out


def log_restated(I, sigma=1.0, spacing=None):
    J = np.asarray(I).astype(np.float64)
    h = [1.0, 1.0, 1.0] if spacing is None else [float(x) for x in spacing]
    sigma = float(sigma)
    (_, p0, q0), (_, p1, q1), (_, p2, q2) = (taps(sigma / h[a]) for a in range(3))
    A0, A2 = axis_pass(J, p2, 2), axis_pass(J, q2, 2)
    B00, B20, B02 = axis_pass(A0, p1, 1), axis_pass(A0, q1, 1), axis_pass(A2, p1, 1)
    T0, T1, T2 = axis_pass(B00, q0, 0), axis_pass(B20, p0, 0), axis_pass(B02, p0, 0)
    s2 = sigma * sigma
    c0, c1, c2 = s2 / (h[0] * h[0]), s2 / (h[1] * h[1]), s2 / (h[2] * h[2])
    return (c0 * T0 + c1 * T1) + c2 * T2


def log_scipy(I, sigma=1.0, spacing=None):
    J = np.asarray(I).astype(np.float64)
    h = [1.0, 1.0, 1.0] if spacing is None else [float(x) for x in spacing]
    E = np.zeros(J.shape)
    for a in range(3):
        order = [0, 0, 0]
        order[a] = 2
        E += (sigma * sigma / (h[a] * h[a])) * ndi.gaussian_filter(J, [sigma / x for x in h], order=order, mode='nearest', truncate=4.0)
    return E


# ------------------------------------------------------------------ steps 4-7
def erode(mask, steps, border=0):
    return ndi.binary_erosion(mask, CROSS, iterations=steps, border_value=border) if steps > 0 else np.asarray(mask, bool).copy()


def dilate(mask, steps):
    return ndi.binary_dilation(mask, CROSS, iterations=steps) if steps > 0 else np.asarray(mask, bool).copy()


def largest(mask, structure=CROSS, seed=None):
    """(the largest component - among equals the smallest label -, or the one that holds `seed`; its size; the number of components)"""
    lab, n = ndi.label(mask, structure)
    if n == 0:
        if seed is not None:
            raise ValueError('the seed voxel is not in the set')
        return np.zeros(lab.shape, bool), 0, 0
    sizes = np.bincount(lab.ravel())[1:]
    if seed is not None:
        win = int(lab[tuple(seed)])
        if win == 0:
            raise ValueError('the seed voxel is not in the set')
    else:
        win = int(np.argmax(sizes)) + 1
    return lab == win, int(sizes[win - 1]), n


def morphology(J, E, floor, threshold, erosion=1, closing=1, seed=None):
    """Steps 4-7 from J and an edge response E: the five stages as bool volumes, and the number of components after the erosion."""
    st = {}
    st['candidate'] = (np.asarray(J).astype(np.float64) > floor) & (E <= threshold)
    st['eroded'] = erode(st['candidate'], erosion, 0)
    st['main'], _, ncomp = largest(st['eroded'], seed=seed)
    opened = dilate(st['main'], erosion)
    st['closed'] = erode(dilate(opened, closing), closing, 1)
    st['final'] = ndi.binary_fill_holes(st['closed'])
    return st, ncomp


def extract(I, sigma=1.0, edge=0.05, floor=None, erosion=1, closing=1, diffusion=None, spacing=None, seed=None, restated=True):
    """The whole definition: (final mask as bool, info dict with the stages, floor, contrast, threshold, components)."""
    J = np.asarray(I)
    if diffusion is not None:
        J = denoise_model.diffuse(J, diffusion['conductance'], diffusion.get('iterations', 5), spacing=spacing)
    lo, hi, counts = histogram(J)
    fl, contrast, _ = floor_contrast(counts, lo, hi, floor)
    E = (log_restated if restated else log_scipy)(J, sigma, spacing)
    st, ncomp = morphology(J, E, fl, edge * contrast, erosion, closing, seed)
    return st['final'], dict(stages=st, floor=fl, contrast=contrast, threshold=edge * contrast, components=ncomp, lo=lo, hi=hi, E=E, J=J)


def dice(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return 2.0 * (a & b).sum() / (a.sum() + b.sum())


# ------------------------------------------------------------------ the phantom
def head_phantom(shape, csf=15.0, noise=0.0, seed=0):
    """(volume, true brain).  Centred grid x_a = i - (n_a - 1) / 2.  Brain: q = sum (x_a / R_a)^2 <= 1 with R_a = n_a / 2 - 8.5,
    intensity 90, 110 where q <= 0.5.  With d the Euclidean distance to the brain: 0 < d <= 2.5 a gap of intensity `csf`,
    2.5 < d <= 6.5 scalp at 85, air at 0 beyond.  A one-voxel bridge of intensity 90 along [n0 // 2, n1 // 2, n2 // 2:] wherever
    d <= 6.5.  Gaussian noise default_rng(seed).normal(0, noise) on every voxel."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape], indexing='ij')
    q = sum((g / (n / 2.0 - 8.5)) ** 2 for g, n in zip(grids, shape))
    brain = q <= 1.0
    d = ndi.distance_transform_edt(~brain)
    I = np.zeros(shape)
    I[brain] = 90.0
    I[q <= 0.5] = 110.0
    I[(d > 0) & (d <= 2.5)] = csf
    I[(d > 2.5) & (d <= 6.5)] = 85.0
    line = np.zeros(shape, bool)
    line[shape[0] // 2, shape[1] // 2, shape[2] // 2:] = True
    I[line & (d <= 6.5)] = 90.0
    if noise > 0:
        I = I + np.random.default_rng(seed).normal(0.0, noise, shape)
    return I, brain


PHANTOM_SHAPES = ((48, 56, 52), (40, 44, 70))
DIFFUSION = dict(conductance=20.0, iterations=3)
