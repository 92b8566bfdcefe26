"""The oracle of vmask_vesselness (include/vmask.h, DESIGN.md section 9 entry f7): the definition written down in float64
with scipy.ndimage.gaussian_filter and numpy.linalg.eigvalsh."""
import numpy as np
from scipy import ndimage

TIE_REL = 1e-6


def taps(sigma_vox):
    """(radius, phi, phi', phi'') on x = -r .. r for a sigma in voxels."""
    r = int(4.0 * sigma_vox + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 * x * x / (sigma_vox * sigma_vox))
    phi /= phi.sum()
    return r, phi, -x / sigma_vox ** 2 * phi, (x * x / sigma_vox ** 4 - 1.0 / sigma_vox ** 2) * phi


def convolve_axis(I, w, axis):
    """Convolution (not correlation) of float64 `I` with the taps `w` on -r .. r along `axis`, indices clamped at the faces."""
    r = (len(w) - 1) // 2
    n = I.shape[axis]
    out = np.zeros_like(I)
    for k in range(-r, r + 1):
        idx = np.clip(np.arange(n) - k, 0, n - 1)
        out += w[k + r] * np.take(I, idx, axis=axis)
    return out


def derivative_explicit(I, sigma, spacing, order):
    """d^order[0..2] of the Gaussian-smoothed volume by explicit taps: what derivative_scipy computes."""
    out = np.asarray(I, dtype=np.float64)
    for a in range(3):
        out = convolve_axis(out, taps(sigma / spacing[a])[1 + order[a]], a)
    return out


def derivative_scipy(I, sigma, spacing, order):
    return ndimage.gaussian_filter(np.asarray(I, dtype=np.float64), [sigma / h for h in spacing], order=order, mode='nearest', truncate=4.0)


ORDERS = {(0, 0): (2, 0, 0), (1, 1): (0, 2, 0), (2, 2): (0, 0, 2), (0, 1): (1, 1, 0), (0, 2): (1, 0, 1), (1, 2): (0, 1, 1)}


def hessian(I, sigma, spacing=(1.0, 1.0, 1.0)):
    """H[..., a, b] = sigma^2 (d_a d_b G_sigma * I) / (h_a h_b)."""
    H = np.empty(I.shape + (3, 3), np.float64)
    for (a, b), order in ORDERS.items():
        H[..., a, b] = H[..., b, a] = (sigma * sigma / (spacing[a] * spacing[b])) * derivative_scipy(I, sigma, spacing, order)
    return H


def sorted_eigenvalues(H):
    """Eigenvalues ordered by magnitude, |l1| <= |l2| <= |l3| (last axis)."""
    e = np.linalg.eigvalsh(H)
    return np.take_along_axis(e, np.argsort(np.abs(e), axis=-1, kind='stable'), axis=-1)


def measure(lam, alpha, beta, gamma, bright=True):
    l1, l2, l3 = (lam[..., 0], lam[..., 1], lam[..., 2]) if bright else (-lam[..., 0], -lam[..., 1], -lam[..., 2])
    ok = (l2 < 0) & (l3 < 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ra = np.abs(l2) / np.abs(l3)
        rb2 = l1 * l1 / np.abs(l2 * l3)
        s2 = l1 * l1 + l2 * l2 + l3 * l3
        v = (1.0 - np.exp(-ra * ra / (2 * alpha * alpha))) * np.exp(-rb2 / (2 * beta * beta)) * (1.0 - np.exp(-s2 / (2 * gamma * gamma)))
    return np.where(ok, v, 0.0)


def vesselness(I, sigmas, alpha=0.5, beta=0.5, gamma=None, mask=None, spacing=None, bright=True):
    """Returns a dict: V (the maximum over the scales), scale (index of the first scale that attains it, 0 where V is 0),
    per_scale (V_sigma, nsig x shape), gammas, ties (bool: voxels where at some scale l1 l2 < 0 and
    | |l1| - |l2| | <= 1e-6 |l3| - the measure's only discontinuity)."""
    I = np.asarray(I, dtype=np.float64)
    spacing = (1.0, 1.0, 1.0) if spacing is None else tuple(float(h) for h in spacing)
    inside = np.ones(I.shape, bool) if mask is None else (np.asarray(mask) != 0)
    per, gammas = [], []
    ties = np.zeros(I.shape, bool)
    for s in sigmas:
        H = hessian(I, float(s), spacing)
        if gamma is not None and gamma > 0:
            g = float(gamma)
        else:
            f2 = (H * H).sum(axis=(-1, -2))
            g = 0.5 * np.sqrt(f2[inside].max()) if inside.any() else 0.0
        gammas.append(g)
        lam = sorted_eigenvalues(H)
        ties |= (lam[..., 0] * lam[..., 1] < 0) & (np.abs(np.abs(lam[..., 0]) - np.abs(lam[..., 1])) <= TIE_REL * np.abs(lam[..., 2]))
        v = measure(lam, alpha, beta, g, bright) if g > 0 else np.zeros(I.shape)
        per.append(np.where(inside, v, 0.0))
    per = np.stack(per)
    V = per.max(axis=0)
    return {'V': V, 'scale': np.where(V > 0, per.argmax(axis=0), 0).astype(np.uint8), 'per_scale': per,
            'gammas': np.array(gammas), 'ties': ties}


def gaussian_line(shape, axis, s, amplitude=100.0):
    """A straight bright line along `axis` through the centre with a Gaussian cross-section of width s."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape], indexing='ij')
    d2 = sum(g * g for a, g in enumerate(grids) if a != axis)
    return amplitude * np.exp(-0.5 * d2 / (s * s))
