// vves_device.hip - vmask_vesselness of include/vmask.h: the multiscale Hessian vesselness filter (Frangi et al. 1998) that
// the reference pipeline gets from an external tool as vesselnessFiltered.nii.gz (entry f7).
//
// Everything is float64 from the taps to the measure; float32 appears only as an input type.  Per scale three kernels:
//   k_ves_axis2   one read of I gives G0, G1, G2: I convolved along axis 2 with the Gaussian and its first and second
//                 derivative.  A wave stages a row segment of 128 voxels plus the halo in LDS and writes 16 bytes per lane
//                 and array.
//   k_ves_axis1   G0, G1, G2 -> the six combinations (order along axis 1, order along axis 2) 00 10 20 01 11 02.
//   k_ves_axis0   the six combinations -> the six Hessian entries in registers, then either the largest squared Frobenius
//                 norm over the (masked) volume (automatic gamma: one atomic maximum per workgroup; a maximum of non-negative
//                 float64 values does not depend on the order) or the measure, folded into out / scale.  The Hessian never
//                 reaches memory.
// The two column passes walk along their axis with a sliding window in LDS: a workgroup of 1024 threads owns TX neighbouring
// columns (lanes run along the contiguous direction) and 1024 / TX rows per step; the window is a ring of 2r + S rows per input
// array, every row of which is loaded once (clamped at the faces: the ring holds the rows -r .. L-1+r by their logical
// index).  The loads of the next step are issued before the taps of this one are applied.  TX is 64 where the ring fits the
// LDS and halves as the radius grows.  The taps are computed on the host and read through uniform (scalar) loads.
// No hand-off between workgroups other than the kernel boundaries; the only atomic is that maximum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"

namespace {

constexpr int MAXR = 64;                           // largest tap radius
constexpr int TAPS = 2 * MAXR + 1;                 // pitch of one tap array; [axis][order][TAPS] per scale
constexpr int ROW_T = 256, ROW_SEG = 128;          // k_ves_axis2: 4 waves, one row segment of 128 voxels each
constexpr int COL_T = 1024;                        // the column passes: 16 waves
constexpr size_t LDS_MAX = 152 * 1024;             // of the 160 KiB of a CU

// ---------------------------------------------------------------- axis 2
template <class T>
__global__ void __launch_bounds__(ROW_T) k_ves_axis2(const T* __restrict__ in, double* __restrict__ g0, double* __restrict__ g1, double* __restrict__ g2,
                                                     const double* __restrict__ taps, int64_t rows, int n2, int r, int vec) {
    __shared__ double lds[ROW_T / 64][ROW_SEG + 2 * MAXR + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (ROW_T / 64) + wave;     // (past the last row: nothing to do)
    const int seg0 = (int)blockIdx.z * ROW_SEG;
    const bool live = row < rows;
    if (live) {
        const T* src = in + row * n2;
        for (int i = lane; i < ROW_SEG + 2 * r; i += 64) {
            const int x = min(max(seg0 - r + i, 0), n2 - 1);
            lds[wave][i] = (double)src[x];
        }
    }
    __syncthreads();
    const int x0 = seg0 + 2 * lane;
    if (!live || x0 >= n2) return;
    // out[x] = sum_m w[2r - m] * in[x - r + m]: lds[2 lane + m] for x0 and lds[2 lane + 1 + m] for x0 + 1
    const double* p = &lds[wave][2 * lane];
    double a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0;
    double v = p[0];
    for (int m = 0; m <= 2 * r; m++) {
        const double nx = p[m + 1];
        const double w0 = taps[2 * r - m], w1 = taps[TAPS + 2 * r - m], w2 = taps[2 * TAPS + 2 * r - m];
        a0 = fma(w0, v, a0); a1 = fma(w1, v, a1); a2 = fma(w2, v, a2);
        b0 = fma(w0, nx, b0); b1 = fma(w1, nx, b1); b2 = fma(w2, nx, b2);
        v = nx;
    }
    const int64_t at = row * n2 + x0;
    if (vec) {                                         // (n2 even and the arrays 16-byte aligned: x0 + 1 < n2)
        *reinterpret_cast<double2*>(g0 + at) = make_double2(a0, b0);
        *reinterpret_cast<double2*>(g1 + at) = make_double2(a1, b1);
        *reinterpret_cast<double2*>(g2 + at) = make_double2(a2, b2);
    } else {
        g0[at] = a0; g1[at] = a1; g2[at] = a2;
        if (x0 + 1 < n2) { g0[at + 1] = b0; g1[at + 1] = b1; g2[at + 1] = b2; }
    }
}

// ---------------------------------------------------------------- the column passes
// A pass along an axis of length L whose elements are `inner` apart: the volume as [outer][L][inner].
struct ColGeo {
    int64_t L, inner, ntile;                       // ntile: column tiles per outer index
    int r, C, txs;                                 // radius, rows of the ring (2r + S), log2 TX
};
template <int N> struct Ptrs { const double* p[N]; };

// the thread's place: its column, its row of a step, where its column starts in memory
struct ColThread {
    int TX, S, col, rs;
    int64_t base;
    bool live;
    __device__ __forceinline__ ColThread(const ColGeo& g) {
        TX = 1 << g.txs; S = COL_T >> g.txs;
        col = (int)threadIdx.x & (TX - 1); rs = (int)threadIdx.x >> g.txs;
        const int64_t o = blockIdx.z, ct = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;         // (tiles past ntile: no live column)
        const int64_t c = ct * TX + col;
        live = ct < g.ntile && c < g.inner;
        base = o * g.L * g.inner + c;
    }
};
// row `lr` of the ring's logical numbering (-r .. L-1+r) is the volume's row clamped to 0 .. L-1
template <int N>
__device__ __forceinline__ void col_fetch(const Ptrs<N>& in, const ColGeo& g, const ColThread& t, int64_t lr, double (&v)[N]) {
    const int64_t row = lr < 0 ? 0 : (lr > g.L - 1 ? g.L - 1 : lr);
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = t.live ? in.p[i][t.base + row * g.inner] : 0.0;
}
template <int N>
__device__ __forceinline__ void col_put(double* lds, const ColGeo& g, const ColThread& t, int slot, const double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) lds[((size_t)i * g.C + slot) * t.TX + t.col] = v[i];
}
// the whole ring: logical rows -r .. S-1+r at the slots 0 .. C-1
template <int N>
__device__ __forceinline__ void col_fill(const Ptrs<N>& in, const ColGeo& g, const ColThread& t, double* lds) {
    double v[N];
    for (int q = t.rs; q < g.C; q += t.S) { col_fetch<N>(in, g, t, (int64_t)q - g.r, v); col_put<N>(lds, g, t, q, v); }
    __syncthreads();
}

// the walk.  Step k gives the rows j = k S + rs; row j - r sits at slot j mod C, and the row that the next step needs in
// its place, j + r + S, goes to the same slot once every wave is done with this step.
template <int N, class Body>
__device__ __forceinline__ void col_walk(const Ptrs<N>& in, const ColGeo& g, const ColThread& t, double* lds, Body&& body) {
    col_fill<N>(in, g, t, lds);
    const int steps = (int)((g.L + t.S - 1) / t.S);
    int slot = t.rs;
    for (int k = 0; k < steps; k++) {
        const int64_t j = (int64_t)k * t.S + t.rs;
        const bool more = k + 1 < steps;           // (the same in every thread)
        double nx[N];
        if (more) col_fetch<N>(in, g, t, j + g.r + t.S, nx);
        if (t.live && j < g.L) body(j, slot);
        if (more) {
            __syncthreads();
            col_put<N>(lds, g, t, slot, nx);
            __syncthreads();
        }
        slot += t.S; if (slot >= g.C) slot -= g.C;
    }
}

__global__ void __launch_bounds__(COL_T) k_ves_axis1(Ptrs<3> in, double* __restrict__ t00, double* __restrict__ t10, double* __restrict__ t20,
                                                     double* __restrict__ t01, double* __restrict__ t11, double* __restrict__ t02,
                                                     const double* __restrict__ taps, ColGeo g) {
    extern __shared__ double lds[];
    const ColThread t(g);
    const int r = g.r, C = g.C;
    col_walk<3>(in, g, t, lds, [&](int64_t j, int slot) {
        double a00 = 0, a10 = 0, a20 = 0, a01 = 0, a11 = 0, a02 = 0;
        int s = slot;
        for (int m = 0; m <= 2 * r; m++) {
            const double w0 = taps[2 * r - m], w1 = taps[TAPS + 2 * r - m], w2 = taps[2 * TAPS + 2 * r - m];
            const double v0 = lds[((size_t)s) * t.TX + t.col], v1 = lds[((size_t)C + s) * t.TX + t.col], v2 = lds[((size_t)2 * C + s) * t.TX + t.col];
            a00 = fma(w0, v0, a00); a10 = fma(w1, v0, a10); a20 = fma(w2, v0, a20);
            a01 = fma(w0, v1, a01); a11 = fma(w1, v1, a11);
            a02 = fma(w0, v2, a02);
            if (++s == C) s = 0;
        }
        const int64_t at = t.base + j * g.inner;
        t00[at] = a00; t10[at] = a10; t20[at] = a20; t01[at] = a01; t11[at] = a11; t02[at] = a02;
    });
}

// eigenvalues of the symmetric 3x3 matrix: e[0] <= e[1] <= e[2].  Deflation (Eberly, "A robust eigensolver for 3x3 symmetric
// matrices"; Kopp 2008) on B = (A - q I) / p, whose eigenvalues beta sum to 0, their squares to 6: the roots of
// beta^3 - 3 beta - 2h, h = det B / 2 in [-1, 1].
//   The root on the side of h's sign lies in [sqrt 3, 2] in magnitude, at least sqrt 3 from the other two: a simple, well
//   conditioned root, taken by Newton steps from the chord (which is within 0.014 of it; the fifth step changes nothing).
//   The other two coincide at h = +-1, where the closed trigonometric form (Smith 1961: acos h, one ulp of h being sqrt(eps)
//   in the angle) leaves them 1e-8 |A| off.  They come from the 2x2 block of B on the plane orthogonal to the first one's
//   eigenvector, which is the longest cross product of two rows of B - beta I (their lengths are the two gaps' product times
//   |v_i|: never all small).
// -B takes the place of B where h < 0, so that the isolated eigenvalue is always the top one.  Selects only: no branch but
// the flat case, no indexed array, nothing transcendental.  tests/vesselness_model.py restates it operation by operation
// (eig3_deflation).
__device__ __forceinline__ void eig3(double a00, double a11, double a22, double a01, double a02, double a12, double (&e)[3]) {
    const double p1 = a01 * a01 + a02 * a02 + a12 * a12;
    const double q = (a00 + a11 + a22) / 3.0;
    const double d0 = a00 - q, d1 = a11 - q, d2 = a22 - q;
    const double p2 = d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1;
    const double p = sqrt(p2 / 6.0);
    if (!(p > 0.0)) { e[0] = e[1] = e[2] = q; return; }        // (three equal eigenvalues, or p2 underflows: 1 / p stays finite below)
    const double ip = 1.0 / p;
    double b00 = d0 * ip, b11 = d1 * ip, b22 = d2 * ip, b01 = a01 * ip, b02 = a02 * ip, b12 = a12 * ip;
    double h = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
    h = fmin(1.0, fmax(-1.0, h));
    const double sg = h < 0.0 ? -1.0 : 1.0;
    b00 *= sg; b11 *= sg; b22 *= sg; b01 *= sg; b02 *= sg; b12 *= sg;
    const double ah = fabs(h);
    double beta = 1.7320508075688772 + 0.2679491924311228 * ah;  // sqrt 3 .. 2
#pragma unroll
    for (int it = 0; it < 5; it++) beta -= (beta * (beta * beta - 3.0) - 2.0 * ah) / (3.0 * beta * beta - 3.0);
    // the eigenvector v: rows r0 r1 r2 of B - beta I, the longest of r0 x r1, r0 x r2, r1 x r2
    const double r00 = b00 - beta, r11 = b11 - beta, r22 = b22 - beta;
    double c0 = b01 * b12 - b02 * r11, c1 = b02 * b01 - r00 * b12, c2 = r00 * r11 - b01 * b01;       // r0 x r1
    double n = c0 * c0 + c1 * c1 + c2 * c2;
    {
        const double o0 = b01 * r22 - b02 * b12, o1 = b02 * b02 - r00 * r22, o2 = r00 * b12 - b01 * b02;   // r0 x r2
        const double m = o0 * o0 + o1 * o1 + o2 * o2;
        const bool take = m > n;
        c0 = take ? o0 : c0; c1 = take ? o1 : c1; c2 = take ? o2 : c2; n = take ? m : n;
    }
    {
        const double o0 = r11 * r22 - b12 * b12, o1 = b12 * b02 - b01 * r22, o2 = b01 * b12 - r11 * b02;   // r1 x r2
        const double m = o0 * o0 + o1 * o1 + o2 * o2;
        const bool take = m > n;
        c0 = take ? o0 : c0; c1 = take ? o1 : c1; c2 = take ? o2 : c2; n = take ? m : n;
    }
    double inv = 1.0 / sqrt(n);
    const double v0 = c0 * inv, v1 = c1 * inv, v2 = c2 * inv;
    // u orthogonal to v from v2 and the larger of v0, v1 (their squares sum to 1/2 at least); w = v x u
    const bool first = fabs(v0) > fabs(v1);
    const double k = first ? v0 : v1;
    inv = 1.0 / sqrt(k * k + v2 * v2);
    const double u0 = first ? -v2 * inv : 0.0, u1 = first ? 0.0 : v2 * inv, u2 = first ? v0 * inv : -v1 * inv;
    const double w0 = v1 * u2 - v2 * u1, w1 = v2 * u0 - v0 * u2, w2 = v0 * u1 - v1 * u0;
    // the block [[u.Bu, w.Bu], [w.Bu, w.Bw]]: mean -+ hypot(half the diagonal's difference, off-diagonal)
    const double x0 = b00 * u0 + b01 * u1 + b02 * u2, x1 = b01 * u0 + b11 * u1 + b12 * u2, x2 = b02 * u0 + b12 * u1 + b22 * u2;
    const double y0 = b00 * w0 + b01 * w1 + b02 * w2, y1 = b01 * w0 + b11 * w1 + b12 * w2, y2 = b02 * w0 + b12 * w1 + b22 * w2;
    const double m00 = u0 * x0 + u1 * x1 + u2 * x2, m01 = w0 * x0 + w1 * x1 + w2 * x2, m11 = w0 * y0 + w1 * y1 + w2 * y2;
    const double mean = 0.5 * (m00 + m11), half = 0.5 * (m00 - m11);
    const double hyp = sqrt(half * half + m01 * m01);             // (entries of order 1: no overflow to guard against)
    const double lo = mean - hyp, hi = mean + hyp;
    const bool pos = sg > 0.0;
    e[0] = q + p * (pos ? lo : -beta);
    e[1] = q + p * (pos ? hi : -hi);
    e[2] = q + p * (pos ? beta : -lo);
}

struct Measure {
    double hs[6];                                  // sigma^2 / (h_a h_b) for 00 11 22 01 02 12
    double ia, ib;                                 // 1 / (2 alpha^2), 1 / (2 beta^2)
    double gamma;                                  // > 0: given; otherwise 0.5 sqrt(*gmax2)
    int sign, index;                               // +1 bright / -1 dark vessels; index of the scale
};

__device__ __forceinline__ double frangi(double h00, double h11, double h22, double h01, double h02, double h12, const Measure& M, double ig) {
    double e[3];
    eig3(h00, h11, h22, h01, h02, h12, e);
    // |l1| <= |l2| <= |l3|
    double l1 = e[0], l2 = e[1], l3 = e[2], s;
    if (fabs(l1) > fabs(l2)) { s = l1; l1 = l2; l2 = s; }
    if (fabs(l2) > fabs(l3)) { s = l2; l2 = l3; l3 = s; }
    if (fabs(l1) > fabs(l2)) { s = l1; l1 = l2; l2 = s; }
    if (!(l2 < 0.0 && l3 < 0.0)) return 0.0;
    const double ra = l2 / l3, rb2 = l1 * l1 / (l2 * l3), s2 = l1 * l1 + l2 * l2 + l3 * l3;
    return (1.0 - exp(-ra * ra * M.ia)) * exp(-rb2 * M.ib) * (1.0 - exp(-s2 * ig));
}

// MODE 0: the largest squared Frobenius norm into *gmax2 (bits of a non-negative float64: they order like the values)
// MODE 1: the measure of this scale folded into out / scale
template <int MODE>
__global__ void __launch_bounds__(COL_T) k_ves_axis0(Ptrs<6> in /* 00 10 20 01 11 02 */, const uint8_t* __restrict__ mask, const double* __restrict__ taps,
                                                     ColGeo g, Measure M, unsigned long long* __restrict__ gmax2,
                                                     double* __restrict__ out, uint8_t* __restrict__ scale) {
    extern __shared__ double lds[];
    __shared__ unsigned long long wmax[COL_T / 64];
    double ig = 0.0;
    if (MODE == 1) {
        const double gm = M.gamma > 0.0 ? M.gamma : 0.5 * sqrt(__longlong_as_double((long long)*gmax2));
        if (!(gm > 0.0)) return;                   // (every thread alike) a scale without any structure contributes 0
        ig = 1.0 / (2.0 * gm * gm);
    }
    const ColThread t(g);
    const int r = g.r, C = g.C;
    double fmax2 = 0.0;
    col_walk<6>(in, g, t, lds, [&](int64_t j, int slot) {
        const int64_t at = t.base + j * g.inner;
        if (mask && !mask[at]) return;             // (out and scale are 0 there from the start)
        double h00 = 0, h11 = 0, h22 = 0, h01 = 0, h02 = 0, h12 = 0;
        int s = slot;
        for (int m = 0; m <= 2 * r; m++) {
            const double w0 = taps[2 * r - m], w1 = taps[TAPS + 2 * r - m], w2 = taps[2 * TAPS + 2 * r - m];
            const double* q = lds + (size_t)s * t.TX + t.col;
            const size_t pitch = (size_t)C * t.TX;
            h00 = fma(w2, q[0], h00);              // orders (2,0,0)
            h01 = fma(w1, q[pitch], h01);          // (1,1,0)
            h11 = fma(w0, q[2 * pitch], h11);      // (0,2,0)
            h02 = fma(w1, q[3 * pitch], h02);      // (1,0,1)
            h12 = fma(w0, q[4 * pitch], h12);      // (0,1,1)
            h22 = fma(w0, q[5 * pitch], h22);      // (0,0,2)
            if (++s == C) s = 0;
        }
        h00 *= M.hs[0]; h11 *= M.hs[1]; h22 *= M.hs[2]; h01 *= M.hs[3]; h02 *= M.hs[4]; h12 *= M.hs[5];
        if (MODE == 0) {
            fmax2 = fmax(fmax2, h00 * h00 + h11 * h11 + h22 * h22 + 2.0 * (h01 * h01 + h02 * h02 + h12 * h12));
        } else {
            const double sg = (double)M.sign;
            const double v = frangi(sg * h00, sg * h11, sg * h22, sg * h01, sg * h02, sg * h12, M, ig);
            if (v > out[at]) { out[at] = v; if (scale) scale[at] = (uint8_t)M.index; }
        }
    });
    if (MODE == 0) {
        unsigned long long b = (unsigned long long)__double_as_longlong(fmax2);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = (unsigned long long)__shfl_xor((long long)b, d, 64);
            b = o > b ? o : b;
        }
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < COL_T / 64; w++) b = wmax[w] > b ? wmax[w] : b;
            if (b) atomicMax(gmax2, b);
        }
    }
}

// ---------------------------------------------------------------- host
// phi, phi', phi'' on -r .. r for sigma in voxels
void make_taps(double s, int r, double* t /* [3][TAPS] */) {
    double sum = 0;
    for (int x = -r; x <= r; x++) { t[x + r] = std::exp(-0.5 * (double)x * x / (s * s)); sum += t[x + r]; }
    for (int x = -r; x <= r; x++) {
        const double phi = t[x + r] / sum;
        t[x + r] = phi;
        t[TAPS + x + r] = -(double)x / (s * s) * phi;
        t[2 * TAPS + x + r] = ((double)x * x / (s * s * s * s) - 1.0 / (s * s)) * phi;
    }
}

// the widest column tile whose ring of N arrays fits the LDS
bool col_geo(int64_t L, int64_t inner, int r, int N, ColGeo& g, size_t& lds) {
    for (int txs = 6; txs >= 3; txs--) {
        const int TX = 1 << txs, S = COL_T / TX, C = 2 * r + S;
        lds = (size_t)N * C * TX * sizeof(double);
        if (lds > LDS_MAX) continue;
        g.L = L; g.inner = inner; g.ntile = (inner + TX - 1) / TX; g.r = r; g.C = C; g.txs = txs;
        return true;
    }
    return false;
}

// n blocks as an x-y grid (a grid's x extent times the block size has to stay below 2^32); z as given
dim3 grid_xy(int64_t n, unsigned z) {
    const int64_t gx = std::min<int64_t>(n, 32768);
    return dim3((unsigned)gx, (unsigned)((n + gx - 1) / gx), z);
}

template <class T>
int vesselness(const T* volume, int64_t n0, int64_t n1, int64_t n2, const uint8_t* mask, const std::vector<double>& taps, const int (*radii)[3],
               const double* sigmas, int nsig, const double* h, double alpha, double beta, double gamma, int bright,
               double* out, uint8_t* scale, double* gammas_used) {
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const bool in_host = !vmask::is_device_pointer(volume), mask_host = mask && !vmask::is_device_pointer(mask);
    const bool out_host = !vmask::is_device_pointer(out), scale_host = scale && !vmask::is_device_pointer(scale);
    T* own_in = nullptr; uint8_t* own_mask = nullptr; double* own_out = nullptr; uint8_t* own_scale = nullptr;
    double* G[3] = {}; double* A[6] = {};
    double* dtaps = nullptr; unsigned long long* dmax = nullptr;
    bool oom = (in_host && mem.grab(&own_in, V, "input")) || (mask_host && mem.grab(&own_mask, V, "mask")) ||
               (out_host && mem.grab(&own_out, V, "output")) || (scale_host && mem.grab(&own_scale, V, "scale"));
    for (auto& q : G) oom = oom || mem.grab(&q, V, "derivatives");
    for (auto& q : A) oom = oom || mem.grab(&q, V, "derivatives");
    oom = oom || mem.grab(&dtaps, taps.size(), "taps") || mem.grab(&dmax, (size_t)nsig, "maxima");
    if (oom) { vmask::set_error("out of device memory (vesselness: the input, the output and nine float64 volumes; volumes are not processed in slabs)"); return VRG_E_MEM; }
    const T* din = in_host ? own_in : volume; const uint8_t* dmask = mask_host ? own_mask : mask;
    double* dout = out_host ? own_out : out; uint8_t* dscale = scale_host ? own_scale : scale;
    if (in_host) VMASK_TRY(hipMemcpy(own_in, volume, V * sizeof(T), hipMemcpyHostToDevice));
    if (mask_host) VMASK_TRY(hipMemcpy(own_mask, mask, V, hipMemcpyHostToDevice));
    VMASK_TRY(hipMemcpy(dtaps, taps.data(), taps.size() * 8, hipMemcpyHostToDevice));
    VMASK_TRY(hipMemsetAsync(dmax, 0, (size_t)nsig * 8, 0));
    VMASK_TRY(hipMemsetAsync(dout, 0, V * 8, 0));
    if (dscale) VMASK_TRY(hipMemsetAsync(dscale, 0, V, 0));
    VMASK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ves_axis1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
    VMASK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ves_axis0<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
    VMASK_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ves_axis0<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));

    const int64_t rows = n0 * n1;
    const int vec = (n2 % 2 == 0) && ((reinterpret_cast<uintptr_t>(G[0]) | reinterpret_cast<uintptr_t>(G[1]) | reinterpret_cast<uintptr_t>(G[2])) & 15u) == 0;
    const dim3 grid2 = grid_xy((rows + ROW_T / 64 - 1) / (ROW_T / 64), (unsigned)((n2 + ROW_SEG - 1) / ROW_SEG));
    for (int i = 0; i < nsig; i++) {
        const double* tp = dtaps + (size_t)i * 9 * TAPS;           // [axis][order][TAPS]
        const int* r = radii[i];
        ColGeo g1, g0; size_t lds1, lds0;
        if (!col_geo(n1, n2, r[1], 3, g1, lds1) || !col_geo(n0, n1 * n2, r[0], 6, g0, lds0)) { vmask::set_error("internal: no column tile fits"); return VRG_E_INTERNAL; }
        k_ves_axis2<T><<<grid2, ROW_T>>>(din, G[0], G[1], G[2], tp + 2 * 3 * TAPS, rows, (int)n2, r[2], vec);
        Ptrs<3> p3 = {{G[0], G[1], G[2]}};
        k_ves_axis1<<<grid_xy(g1.ntile, (unsigned)n0), COL_T, lds1>>>(p3, A[0], A[1], A[2], A[3], A[4], A[5], tp + 1 * 3 * TAPS, g1);
        Ptrs<6> p6 = {{A[0], A[1], A[2], A[3], A[4], A[5]}};
        Measure M;
        const double s2 = sigmas[i] * sigmas[i];
        M.hs[0] = s2 / (h[0] * h[0]); M.hs[1] = s2 / (h[1] * h[1]); M.hs[2] = s2 / (h[2] * h[2]);
        M.hs[3] = s2 / (h[0] * h[1]); M.hs[4] = s2 / (h[0] * h[2]); M.hs[5] = s2 / (h[1] * h[2]);
        M.ia = 1.0 / (2.0 * alpha * alpha); M.ib = 1.0 / (2.0 * beta * beta);
        M.gamma = gamma > 0.0 ? gamma : 0.0; M.sign = bright ? 1 : -1; M.index = i;
        if (!(gamma > 0.0)) k_ves_axis0<0><<<grid_xy(g0.ntile, 1), COL_T, lds0>>>(p6, dmask, tp, g0, M, dmax + i, nullptr, nullptr);
        k_ves_axis0<1><<<grid_xy(g0.ntile, 1), COL_T, lds0>>>(p6, dmask, tp, g0, M, dmax + i, dout, dscale);
    }
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if (gammas_used) {
        std::vector<double> m2(nsig);
        VMASK_TRY(hipMemcpy(m2.data(), dmax, (size_t)nsig * 8, hipMemcpyDeviceToHost));   // (the bits of float64 values)
        for (int i = 0; i < nsig; i++) gammas_used[i] = gamma > 0.0 ? gamma : 0.5 * std::sqrt(m2[i]);
    }
    if (out_host) VMASK_TRY(hipMemcpy(out, dout, V * 8, hipMemcpyDeviceToHost));
    if (scale_host) VMASK_TRY(hipMemcpy(scale, dscale, V, hipMemcpyDeviceToHost));
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_vesselness(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const uint8_t* mask,
                                const double* sigmas, int nsig, const double* spacing, double alpha, double beta, double gamma, int bright,
                                double* out, uint8_t* scale, double* gammas_used) {
    if (!volume || !out || !sigmas) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (dtype != VRG_F32 && dtype != VRG_F64) { vmask::set_error("vesselness: the volume must be float32 or float64"); return VRG_E_ARG; }
    if (nsig < 1 || nsig > 32) { vmask::set_error("vesselness: 1 to 32 scales"); return VRG_E_ARG; }
    if (!(std::isfinite(alpha) && alpha > 0.0) || !(std::isfinite(beta) && beta > 0.0)) { vmask::set_error("vesselness: alpha and beta must be finite and positive"); return VRG_E_ARG; }
    if (std::isnan(gamma) || std::isinf(gamma)) { vmask::set_error("vesselness: gamma must be finite (<= 0: automatic)"); return VRG_E_ARG; }
    double h[3] = {1.0, 1.0, 1.0};
    for (int a = 0; a < 3 && spacing; a++) {
        h[a] = spacing[a];
        if (!(std::isfinite(h[a]) && h[a] > 0.0)) { vmask::set_error("vesselness: the spacing must be finite and positive"); return VRG_E_ARG; }
    }
    std::vector<double> taps((size_t)nsig * 9 * TAPS, 0.0);
    int radii[32][3];
    for (int i = 0; i < nsig; i++) {
        if (!(std::isfinite(sigmas[i]) && sigmas[i] > 0.0)) { vmask::set_error("vesselness: every sigma must be finite and positive"); return VRG_E_ARG; }
        for (int a = 0; a < 3; a++) {
            const double s = sigmas[i] / h[a], rr = 4.0 * s + 0.5;
            if (!(rr >= 1.0) || !(rr < (double)(MAXR + 1))) { vmask::set_error("vesselness: sigma / spacing gives a tap radius int(4 sigma + 0.5) outside 1..64"); return VRG_E_ARG; }
            radii[i][a] = (int)rr;
            make_taps(s, radii[i][a], taps.data() + ((size_t)i * 9 + (size_t)a * 3) * TAPS);
        }
    }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    if (dtype == VRG_F32) return vesselness<float>((const float*)volume, n0, n1, n2, mask, taps, radii, sigmas, nsig, h, alpha, beta, gamma, bright, out, scale, gammas_used);
    return vesselness<double>((const double*)volume, n0, n1, n2, mask, taps, radii, sigmas, nsig, h, alpha, beta, gamma, bright, out, scale, gammas_used);
}
