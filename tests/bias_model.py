"""numpy restatement of the bias-field definition of include/vmask.h (vmask_bias_*): one elementwise numpy operation per IEEE
operation of the definition, loops in the stated order, so that the kernels can be held to it bit for bit.  The sharpening map
is restated twice: `sharpen_fft` with np.fft (what the library's host function is pinned to on the CPU), and through the
library's own function where a caller hands it in as `sharpen` (the loop's bit equality)."""
import numpy as np

P = 512


def axis_table(n, M):
    """(s[n] int, w[n][4], c2[n][4], c3[n][4]) of an axis of extent n with M spans."""
    i = np.arange(n, dtype=np.float64)
    u = ((i + 0.5) * float(M)) / float(n)
    s = np.minimum(np.floor(u), float(M - 1))
    t = u - s
    o = 1.0 - t
    w0 = ((o * o) * o) / 6.0
    w1 = ((((3.0 * t - 6.0) * t) * t) + 4.0) / 6.0
    w2 = (((((-3.0 * t + 3.0) * t + 3.0) * t)) + 1.0) / 6.0
    w3 = ((t * t) * t) / 6.0
    S = ((w0 * w0 + w1 * w1) + w2 * w2) + w3 * w3
    w = np.stack([w0, w1, w2, w3], axis=1)
    c2 = w * w
    c3 = ((w * w) * w) / S[:, None]
    return s.astype(np.int64), w, c2, c3


def fit(r, m, spans):
    """phi[K0][K1][K2] = fit(r, m): three contractions, each summed in ascending voxel index from +0.0."""
    r = np.asarray(r, dtype=np.float64)
    m = np.asarray(m) != 0
    n0, n1, n2 = r.shape
    K0, K1, K2 = (int(M) + 3 for M in spans)
    s, _, c2, c3 = axis_table(n0, spans[0])
    N0, D0 = np.zeros((K0, n1, n2)), np.zeros((K0, n1, n2))
    with np.errstate(invalid='ignore', over='ignore'):
        for x in range(n0):
            for j in range(4):
                k = s[x] + j
                N0[k] = np.where(m[x], N0[k] + c3[x, j] * r[x], N0[k])
                D0[k] = np.where(m[x], D0[k] + c2[x, j], D0[k])
    s, _, c2, c3 = axis_table(n1, spans[1])
    N1, D1 = np.zeros((K0, K1, n2)), np.zeros((K0, K1, n2))
    for y in range(n1):
        for j in range(4):
            k = s[y] + j
            N1[:, k] = N1[:, k] + c3[y, j] * N0[:, y]
            D1[:, k] = D1[:, k] + c2[y, j] * D0[:, y]
    s, _, c2, c3 = axis_table(n2, spans[2])
    N2, D2 = np.zeros((K0, K1, K2)), np.zeros((K0, K1, K2))
    for z in range(n2):
        for j in range(4):
            k = s[z] + j
            N2[:, :, k] = N2[:, :, k] + c3[z, j] * N1[:, :, z]
            D2[:, :, k] = D2[:, :, k] + c2[z, j] * D1[:, :, z]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(D2 > 0.0, N2 / D2, 0.0)


def evaluate(phi, spans, shape):
    """F[n0][n1][n2] = eval(phi): three expansions, each a four-term sum over j ascending from +0.0."""
    phi = np.asarray(phi, dtype=np.float64)
    n0, n1, n2 = shape
    s, w, _, _ = axis_table(n2, spans[2])
    E2 = np.zeros(phi.shape[:2] + (n2,))
    for j in range(4):
        E2 = E2 + w[:, j][None, None, :] * phi[:, :, s + j]
    s, w, _, _ = axis_table(n1, spans[1])
    E1 = np.zeros((phi.shape[0], n1, n2))
    for j in range(4):
        E1 = E1 + w[:, j][None, :, None] * E2[:, s + j, :]
    s, w, _, _ = axis_table(n0, spans[0])
    F = np.zeros((n0, n1, n2))
    for j in range(4):
        F = F + w[:, j][:, None, None] * E1[s + j]
    return F


def sharpen_fft(counts, umin, umax, fwhm=0.15, noise=0.01):
    """The sharpening map with np.fft: E[k] per bin."""
    counts = np.asarray(counts, dtype=np.float64)
    nb = counts.size
    off = (P - nb) // 2
    h = (umax - umin) / float(nb - 1)
    sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0))) / h
    k = np.arange(P)
    d = np.minimum(k, P - k) / sigma
    G = np.exp(-0.5 * (d * d))
    G = G / G.sum()
    V = np.zeros(P)
    V[off:off + nb] = counts
    centre = umin + (k - off) * h
    Gh, Vh = np.fft.fft(G), np.fft.fft(V)
    U = np.maximum(np.real(np.fft.ifft(np.conj(Gh) / (np.abs(Gh) ** 2 + noise) * Vh)), 0.0)
    num = np.real(np.fft.ifft(Gh * np.fft.fft(centre * U)))
    den = np.real(np.fft.ifft(Gh * np.fft.fft(U)))
    ok = den > 1e-12 * den.max()
    E = np.where(ok, num / np.where(ok, den, 1.0), centre)
    return E[off:off + nb]


def log_field(v, m, m0=(1, 1, 1), levels=3, iterations=20, threshold=1e-3, nb=200, fwhm=0.15, noise=0.01, sharpen=sharpen_fft):
    """(b, trace): the loop; trace is an array of rows (level, max |phi|, umin, umax), one per iteration that ran."""
    v = np.asarray(v, dtype=np.float64)
    m = np.asarray(m) != 0
    b = np.zeros(v.shape)
    trace = []
    vm = v[m]
    for level in range(levels):
        M = [int(a) * 2 ** level for a in m0]
        stop = False
        for _ in range(iterations):
            u = vm - b[m]
            umin, umax = float(u.min()), float(u.max())
            if umin == umax:
                stop = True
                break
            h = (umax - umin) / float(nb - 1)
            idx = np.clip(np.floor((u - umin) / h + 0.5), 0.0, float(nb - 1)).astype(np.int64)
            counts = np.bincount(idx, minlength=nb).astype(np.float64)
            E = np.asarray(sharpen(counts, umin, umax, fwhm, noise), dtype=np.float64)
            p = (u - umin) / h
            fl = np.clip(np.floor(p), 0.0, float(nb - 2))
            i0 = fl.astype(np.int64)
            f = p - fl
            lo, hi = E[i0], E[i0 + 1]
            r = np.zeros(v.shape)
            r[m] = u - (lo + f * (hi - lo))
            phi = fit(r, m, M)
            b = b + evaluate(phi, M, v.shape)
            top = float(np.abs(phi).max())
            trace.append((float(level), top, umin, umax))
            if top < threshold:
                break
        if stop:
            break
    return b, np.array(trace, dtype=np.float64).reshape(-1, 4)


def correct(volume, mask=None, **kw):
    """(corrected, field, trace) of the correction, with numpy's log and exp."""
    I = np.asarray(volume).astype(np.float64)
    m = I > 0.0
    if mask is not None:
        m &= np.asarray(mask) != 0
    with np.errstate(invalid='ignore', divide='ignore'):
        v = np.where(m, np.log(np.where(m, I, 1.0)), 0.0)
    b, trace = log_field(v, m, **kw)
    field = np.exp(b)
    return I / field, field, trace


# ------------------------------------------------------------------ the phantom
CLASS_VALUES = (100.0, 160.0, 220.0)


def phantom(shape, noise=0.0, seed=0):
    """(biased volume, true field, class labels 0..3): three tissue classes as nested ellipsoid shells with a wavy rim inside a
    background of 0 (class 0), times the field exp(0.3 (0.8 x - 0.5 y + 0.6 z^2 - 0.4 x y)) on coordinates in [-1, 1]."""
    ax = [(np.arange(n) + 0.5) / n * 2.0 - 1.0 for n in shape]
    x, y, z = np.meshgrid(*ax, indexing='ij')
    rho = np.sqrt(x * x + y * y + z * z) / 0.95 + 0.06 * np.sin(5.0 * x) * np.cos(4.0 * y + 3.0 * z)
    labels = np.zeros(shape, dtype=np.int64)
    labels[rho < 0.95] = 1
    labels[rho < 0.75] = 2
    labels[rho < 0.5] = 3
    clean = np.zeros(shape)
    for c, value in enumerate(CLASS_VALUES, start=1):
        clean[labels == c] = value
    if noise > 0.0:
        clean = clean * (1.0 + noise * np.random.default_rng(seed).standard_normal(shape))
    field = np.exp(0.3 * (0.8 * x - 0.5 * y + 0.6 * z * z - 0.4 * x * y))
    return clean * field, field, labels


def class_cvs(volume, labels, mask=None):
    """The coefficient of variation of `volume` within each tissue class (over `mask` where given)."""
    out = []
    for c in (1, 2, 3):
        sel = labels == c
        if mask is not None:
            sel &= np.asarray(mask) != 0
        vals = np.asarray(volume)[sel]
        out.append(float(vals.std() / vals.mean()))
    return out
