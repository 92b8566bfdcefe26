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


def sorted_eigenvalues(H, solver=None):
    """Eigenvalues ordered by magnitude, |l1| <= |l2| <= |l3| (last axis); `solver` (H -> ascending eigenvalues) in eigvalsh's place."""
    e = np.linalg.eigvalsh(H) if solver is None else solver(H)
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


def vesselness(I, sigmas, alpha=0.5, beta=0.5, gamma=None, mask=None, spacing=None, bright=True, solver=None):
    """Returns a dict: V (the maximum over the scales), scale (index of the first scale that attains it, 0 where V is 0),
    per_scale (V_sigma, nsig x shape), gammas, ties (bool: voxels where at some scale l1 l2 < 0 and
    | |l1| - |l2| | <= 1e-6 |l3| - the measure's only discontinuity).  `solver`: one of the restated eigen-solves below
    in eigvalsh's place."""
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
        lam = sorted_eigenvalues(H, solver)
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


# ------------------------------------------------------------------ noise-free phantoms
# Where the volume is piecewise constant, smooth or symmetric, two eigenvalues of the Hessian coincide (or nearly do) on whole
# regions: the inputs on which an eigen-solve shows its conditioning.  Centred grids x_a = i - (n_a - 1) / 2; every value but
# the blob's is exact in float32.
def _grids(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape], indexing='ij')


def cube(shape, half=4.0, amplitude=100.0):
    """|x_a| < half on all three axes."""
    g = _grids(shape)
    return amplitude * ((np.abs(g[0]) < half) & (np.abs(g[1]) < half) & (np.abs(g[2]) < half)).astype(np.float64)


def blob(shape, s=3.0, amplitude=100.0):
    """An isotropic Gaussian of width s at the centre."""
    return amplitude * np.exp(-0.5 * sum(x * x for x in _grids(shape)) / (s * s))


def half_space(shape, axis, amplitude=100.0):
    """x_axis > 0: a step across the middle of the volume."""
    return amplitude * (_grids(shape)[axis] > 0).astype(np.float64)


def ball(shape, r2=36.0, amplitude=100.0):
    return amplitude * (sum(x * x for x in _grids(shape)) < r2).astype(np.float64)


def bright_voxel(shape, amplitude=100.0, background=10.0):
    """One voxel, at the index n_a // 2, on a constant background: at the voxel H is diagonal with (at an isotropic spacing)
    three equal entries, on the axes through it two are equal, far from it H = c I with c the taps' tiny sum.
    The background is not 0 for a reason: on zeros, at sigma = spacing, the twelve voxels (+-1, +-1, 0) away have the
    eigenvalues (-a, -a, +a) exactly - phi'' vanishes at x = sigma and phi'(1)^2 phi(0) = -phi''(0) phi(1)^2 - and there
    the magnitude ordering, hence the measure, is decided by the last bit: a jump that the tie set of vesselness(), which
    looks at l1 and l2 only after a stable sort, does not report.  The background shifts every eigenvalue by c and lifts it."""
    I = np.full(shape, background, np.float64)
    I[tuple(n // 2 for n in shape)] = amplitude
    return I


PHANTOMS = {'cube': cube, 'blob': blob, 'half0': lambda shape: half_space(shape, 0), 'half2': lambda shape: half_space(shape, 2),
            'ball': ball, 'voxel': bright_voxel}


def cut_mask(shape):
    """A brain mask whose face, an oblique plane next to the centre, cuts through every phantom above."""
    g = _grids(shape)
    return (g[0] + 0.5 * g[1] - g[2] > 0.25).astype(np.uint8)


# ------------------------------------------------------------------ the kernel's eigen-solves, restated
# float64, one numpy operation per operation of the device code, no FMA.  Both take the H of hessian() and return the
# eigenvalues in ascending order (last axis); sorted_eigenvalues(H, solver) and vesselness(..., solver=...) take them in
# eigvalsh's place.
def _normalised(H):
    """q, p and B = (H - q I) / p as the device code forms them (B as its six entries b00 b11 b22 b01 b02 b12), and p2 = |H - q I|_F^2."""
    a00, a11, a22, a01, a02, a12 = H[..., 0, 0], H[..., 1, 1], H[..., 2, 2], H[..., 0, 1], H[..., 0, 2], H[..., 1, 2]
    p1 = a01 * a01 + a02 * a02 + a12 * a12
    q = (a00 + a11 + a22) / 3.0
    d0, d1, d2 = a00 - q, a11 - q, a22 - q
    p2 = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1
    p = np.sqrt(p2 / 6.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ip = 1.0 / p
        b = (d0 * ip, d1 * ip, d2 * ip, a01 * ip, a02 * ip, a12 * ip)
    return q, p, b, p2


def _half_det(b):
    b00, b11, b22, b01, b02, b12 = b
    h = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02))
    return np.minimum(1.0, np.maximum(-1.0, h))


def eig3_closed_form(H):
    """The closed trigonometric form (Smith 1961) that the kernel used first.  Where two eigenvalues coincide h = +-1, one ulp
    of h is sqrt(eps) in acos(h), and the close pair carries about 1e-8 |H|: kept to show that the phantoms tell."""
    q, p, b, p2 = _normalised(H)
    with np.errstate(invalid='ignore'):
        phi = np.arccos(_half_det(b)) / 3.0
        e2 = q + 2.0 * p * np.cos(phi)
        e0 = q + 2.0 * p * np.cos(phi + 2.0943951023931954923)
        e1 = 3.0 * q - e0 - e2
    flat = ~(p2 > 0.0)
    return np.stack([np.where(flat, q, e0), np.where(flat, q, e1), np.where(flat, q, e2)], axis=-1)


def eig3_deflation(H):
    """eig3 of csrc/vves_device.hip: the isolated eigenvalue (the simple root of B's characteristic polynomial on the side of
    det B's sign, at least sqrt 3 from the other two) by Newton steps; its eigenvector from the largest cross product of two rows of B - beta I; the other two from the 2x2 block of B on the plane
    orthogonal to it (Eberly, "A robust eigensolver for 3x3 symmetric matrices"; Kopp 2008)."""
    q, p, b, _ = _normalised(H)
    with np.errstate(invalid='ignore', divide='ignore'):
        h = _half_det(b)
        sg = np.where(h < 0.0, -1.0, 1.0)                  # -B has the isolated eigenvalue on top as well
        b00, b11, b22, b01, b02, b12 = [sg * x for x in b]
        ah = np.abs(h)
        beta = 1.7320508075688772 + 0.2679491924311228 * ah  # the root of beta^3 - 3 beta - 2|h| in [sqrt 3, 2]: Newton from the chord
        for _ in range(5):
            beta = beta - (beta * (beta * beta - 3.0) - 2.0 * ah) / (3.0 * beta * beta - 3.0)
        r0, r1, r2 = (b00 - beta, b01, b02), (b01, b11 - beta, b12), (b02, b12, b22 - beta)

        def cross(u, v):
            return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])

        def dot(u, v):
            return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
        c = cross(r0, r1)
        n = dot(c, c)
        for other in (cross(r0, r2), cross(r1, r2)):
            m = dot(other, other)
            take = m > n
            c = tuple(np.where(take, o, x) for o, x in zip(other, c))
            n = np.where(take, m, n)
        inv = 1.0 / np.sqrt(n)
        v = (c[0] * inv, c[1] * inv, c[2] * inv)
        # u orthogonal to v from its two larger components, w = v x u
        first = np.abs(v[0]) > np.abs(v[1])
        k = np.where(first, v[0], v[1])
        inv = 1.0 / np.sqrt(k * k + v[2] * v[2])
        u = (np.where(first, -v[2] * inv, 0.0), np.where(first, 0.0, v[2] * inv), np.where(first, v[0] * inv, -v[1] * inv))
        w = cross(v, u)
        Bu = (b00 * u[0] + b01 * u[1] + b02 * u[2], b01 * u[0] + b11 * u[1] + b12 * u[2], b02 * u[0] + b12 * u[1] + b22 * u[2])
        Bw = (b00 * w[0] + b01 * w[1] + b02 * w[2], b01 * w[0] + b11 * w[1] + b12 * w[2], b02 * w[0] + b12 * w[1] + b22 * w[2])
        m00, m01, m11 = dot(u, Bu), dot(w, Bu), dot(w, Bw)
        mean, half = 0.5 * (m00 + m11), 0.5 * (m00 - m11)
        hyp = np.sqrt(half * half + m01 * m01)
        lo, hi = mean - hyp, mean + hyp
        pos = sg > 0.0
        e0 = q + p * np.where(pos, lo, -beta)
        e1 = q + p * np.where(pos, hi, -hi)
        e2 = q + p * np.where(pos, beta, -lo)
    flat = ~(p > 0.0)
    return np.stack([np.where(flat, q, e0), np.where(flat, q, e1), np.where(flat, q, e2)], axis=-1)
