// vbias_device.hip - vmask_bias_* of include/vmask.h: N4-style bias-field correction, the first pre-processing step the
// reference's README names and leaves to an external tool (entry f15).  Log domain, histogram sharpening
// by Wiener deconvolution on the host, an incremental cubic B-spline fit of the residual over a lattice that doubles per level.
//
//   k_bias_fit<FIRST, LAST>  one contraction of the separable scattered-data fit, [outer][n][inner] -> [outer][K][inner].  A thread
//                  owns one (outer, inner) column - 256 consecutive columns per workgroup, so lanes run along axis 2 in the
//                  dense axis-0 pass - and marches over the n voxels of the axis in ascending order, which is the order of the
//                  definition's sums.  The four control points that a voxel touches, s .. s + 3, are four (N, D) accumulator
//                  pairs in registers; when s moves on the lowest pair is retired to memory and the window shifts, so every
//                  control point is written exactly once, the ones that no voxel touches as +0.0.  FIRST reads the residual and
//                  the mask (9 B per voxel, once), the later passes read the (N, D) of the pass before; LAST writes N / D.
//   k_bias_expand  one expansion of the evaluation along axis 2 or axis 1: a thread per output value, four terms.
//   k_bias_expand0<ADD>  the last expansion, the dense write: a thread per column marches over EZ = 32 planes of axis 0 with the
//                  four E1 values of its span in registers; ADD fuses b <- b + F.
//   k_bias_log, k_bias_minmax, k_bias_hist, k_bias_residual, k_bias_exp, k_bias_count  the streaming passes of the loop, grid-stride.
// float64 throughout, nothing contracted; the only atomics are integer ones (histogram counts, the mask count).  No scratch.
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

#pragma clang fp contract(off)

namespace {

constexpr int BT = 256;                            // every kernel: 4 waves
constexpr int EZ = 32;                           // k_bias_expand0: the planes of axis 0 that a workgroup marches over
constexpr int GRID = 4096;                         // the grid-stride passes
constexpr int PADDED = 512;                        // the transform length of the sharpening map
constexpr int MAXBINS = 256;

// ---------------------------------------------------------------- axis tables (host, double)
struct AxisHost {
    int n = 0, M = 0, K = 0;
    std::vector<int32_t> s;
    std::vector<double> w, c2, c3;                 // [n][4]
};

void build_axis(int n, int M, AxisHost& t) {
    t.n = n; t.M = M; t.K = M + 3;
    t.s.resize(n); t.w.resize(4 * (size_t)n); t.c2.resize(4 * (size_t)n); t.c3.resize(4 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const double u = (((double)i + 0.5) * (double)M) / (double)n;
        double fs = std::floor(u);
        if (fs > (double)(M - 1)) fs = (double)(M - 1);
        const double tt = u - fs;
        const double o = 1.0 - tt;
        double w[4];
        w[0] = ((o * o) * o) / 6.0;
        w[1] = ((((3.0 * tt - 6.0) * tt) * tt) + 4.0) / 6.0;
        w[2] = (((((-3.0 * tt + 3.0) * tt + 3.0) * tt)) + 1.0) / 6.0;
        w[3] = ((tt * tt) * tt) / 6.0;
        const double S = ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) + w[3] * w[3];
        t.s[i] = (int32_t)fs;
        for (int j = 0; j < 4; j++) {
            t.w[4 * (size_t)i + j] = w[j];
            t.c2[4 * (size_t)i + j] = w[j] * w[j];
            t.c3[4 * (size_t)i + j] = ((w[j] * w[j]) * w[j]) / S;
        }
    }
}

struct AxisDev { const int32_t* s; const double* w; const double* c2; const double* c3; int n, K; };

// ---------------------------------------------------------------- the fit
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(BT) k_bias_fit(const double* __restrict__ An, const double* __restrict__ Ad, const uint8_t* __restrict__ mask,
                                                 int64_t cols, int64_t inner, AxisDev ax, double* __restrict__ On, double* __restrict__ Od) {
    const int64_t t = (int64_t)blockIdx.x * BT + threadIdx.x;
    if (t >= cols) return;                         // (no barrier in this kernel)
    const int64_t o = t / inner, q = t - o * inner;
    const int64_t in0 = o * ax.n * inner + q, out0 = o * ax.K * inner + q;
    double N0 = 0.0, N1 = 0.0, N2 = 0.0, N3 = 0.0, D0 = 0.0, D1 = 0.0, D2 = 0.0, D3 = 0.0;
    int base = 0;                                  // the control point of N0 / D0
    auto retire = [&]() {
        const int64_t at = out0 + (int64_t)base * inner;
        if (LAST) On[at] = D0 > 0.0 ? N0 / D0 : 0.0;
        else { On[at] = N0; Od[at] = D0; }
        N0 = N1; N1 = N2; N2 = N3; N3 = 0.0;
        D0 = D1; D1 = D2; D2 = D3; D3 = 0.0;
        base++;
    };
    for (int i = 0; i < ax.n; i++) {
        const int si = ax.s[i];
        while (base < si) retire();
        const int64_t at = in0 + (int64_t)i * inner;
        const double* c2 = ax.c2 + 4 * (int64_t)i;
        const double* c3 = ax.c3 + 4 * (int64_t)i;
        if (FIRST) {
            if (mask[at]) {                        // (outside the mask a voxel costs its mask byte)
                const double r = An[at];
                N0 = N0 + c3[0] * r; N1 = N1 + c3[1] * r; N2 = N2 + c3[2] * r; N3 = N3 + c3[3] * r;
                D0 = D0 + c2[0]; D1 = D1 + c2[1]; D2 = D2 + c2[2]; D3 = D3 + c2[3];
            }
        } else {
            const double a = An[at], d = Ad[at];
            N0 = N0 + c3[0] * a; N1 = N1 + c3[1] * a; N2 = N2 + c3[2] * a; N3 = N3 + c3[3] * a;
            D0 = D0 + c2[0] * d; D1 = D1 + c2[1] * d; D2 = D2 + c2[2] * d; D3 = D3 + c2[3] * d;
        }
    }
    while (base < ax.K) retire();
}

// ---------------------------------------------------------------- the evaluation
// [outer][K][inner] -> [outer][n][inner]
__global__ void __launch_bounds__(BT) k_bias_expand(const double* __restrict__ in, int64_t total, int64_t inner, AxisDev ax, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * BT + threadIdx.x;
    if (t >= total) return;
    const int64_t oi = t / inner, q = t - oi * inner;
    const int64_t o = oi / ax.n;
    const int i = (int)(oi - o * ax.n);
    const double* p = in + (o * ax.K + ax.s[i]) * inner + q;
    const double* w = ax.w + 4 * (int64_t)i;
    double acc = 0.0;
    acc = acc + w[0] * p[0];
    acc = acc + w[1] * p[inner];
    acc = acc + w[2] * p[2 * inner];
    acc = acc + w[3] * p[3 * inner];
    out[t] = acc;
}

template <bool ADD>
__global__ void __launch_bounds__(BT) k_bias_expand0(const double* __restrict__ E1, int64_t inner, AxisDev ax, double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * BT + threadIdx.x;
    if (q >= inner) return;                        // (no barrier in this kernel)
    const int x0 = (int)blockIdx.y * EZ, x1 = min(x0 + EZ, ax.n);
    int sb = ax.s[x0];
    const double* p = E1 + q;
    double e0 = p[(int64_t)sb * inner], e1 = p[(int64_t)(sb + 1) * inner], e2 = p[(int64_t)(sb + 2) * inner], e3 = p[(int64_t)(sb + 3) * inner];
    for (int x = x0; x < x1; x++) {
        const int sx = ax.s[x];
        while (sb < sx) { sb++; e0 = e1; e1 = e2; e2 = e3; e3 = p[(int64_t)(sb + 3) * inner]; }     // (sb + 3 <= K - 1)
        const double* w = ax.w + 4 * (int64_t)x;
        double acc = 0.0;
        acc = acc + w[0] * e0;
        acc = acc + w[1] * e1;
        acc = acc + w[2] * e2;
        acc = acc + w[3] * e3;
        const int64_t at = (int64_t)x * inner + q;
        if (ADD) out[at] = out[at] + acc;
        else out[at] = acc;
    }
}

// ---------------------------------------------------------------- the streaming passes
__device__ __forceinline__ void block_add(unsigned long long mine, unsigned long long* total) {
    __shared__ unsigned long long part[BT];
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int k = BT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(total, part[0]);
}

__global__ void __launch_bounds__(BT) k_bias_count(const uint8_t* __restrict__ mask, int64_t V, unsigned long long* total) {
    unsigned long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) mine += mask[i] ? 1u : 0u;
    block_add(mine, total);
}

// v = log((double) I) over the mask (mask_in NULL: I > 0; a mask voxel with I <= 0 leaves the mask), 0.0 elsewhere
template <class T>
__global__ void __launch_bounds__(BT) k_bias_log(const T* __restrict__ I, const uint8_t* __restrict__ mask_in, int64_t V,
                                                 double* __restrict__ v, uint8_t* __restrict__ m, unsigned long long* total) {
    unsigned long long mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) {
        const double x = (double)I[i];
        const bool in = x > 0.0 && (!mask_in || mask_in[i]);
        v[i] = in ? log(x) : 0.0;
        m[i] = in ? 1 : 0;
        mine += in ? 1u : 0u;
    }
    block_add(mine, total);
}

// per workgroup the exact min and max of u = v - b over the mask: part[2 g], part[2 g + 1] (+inf, -inf where it saw none)
__global__ void __launch_bounds__(BT) k_bias_minmax(const double* __restrict__ v, const double* __restrict__ b, const uint8_t* __restrict__ m,
                                                    int64_t V, double* __restrict__ part) {
    __shared__ double lo_s[BT], hi_s[BT];
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT)
        if (m[i]) { const double u = v[i] - b[i]; lo = fmin(lo, u); hi = fmax(hi, u); }
    lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi;
    __syncthreads();
    for (int k = BT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            lo_s[threadIdx.x] = fmin(lo_s[threadIdx.x], lo_s[threadIdx.x + k]);
            hi_s[threadIdx.x] = fmax(hi_s[threadIdx.x], hi_s[threadIdx.x + k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = lo_s[0]; part[2 * blockIdx.x + 1] = hi_s[0]; }
}

__global__ void __launch_bounds__(BT) k_bias_hist(const double* __restrict__ v, const double* __restrict__ b, const uint8_t* __restrict__ m,
                                                  int64_t V, double umin, double h, int nb, unsigned long long* __restrict__ counts) {
    __shared__ unsigned int bins[MAXBINS];         // a workgroup sees fewer than 2^32 voxels
    for (int k = threadIdx.x; k < MAXBINS; k += BT) bins[k] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT)
        if (m[i]) {
            const double u = v[i] - b[i];
            double p = floor((u - umin) / h + 0.5);
            p = !(p > 0.0) ? 0.0 : (p > (double)(nb - 1) ? (double)(nb - 1) : p);       // (a NaN lands in bin 0, never outside)
            atomicAdd(&bins[(int)p], 1u);
        }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += BT)
        if (bins[k]) atomicAdd(&counts[k], (unsigned long long)bins[k]);
}

__global__ void __launch_bounds__(BT) k_bias_residual(const double* __restrict__ v, const double* __restrict__ b, const uint8_t* __restrict__ m,
                                                      int64_t V, double umin, double h, int nb, const double* __restrict__ E, double* __restrict__ r) {
    __shared__ double map[MAXBINS];
    for (int k = threadIdx.x; k < nb; k += BT) map[k] = E[k];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) {
        double res = 0.0;
        if (m[i]) {
            const double u = v[i] - b[i];
            const double p = (u - umin) / h;
            double fl = floor(p);
            fl = !(fl > 0.0) ? 0.0 : (fl > (double)(nb - 2) ? (double)(nb - 2) : fl);
            const int i0 = (int)fl;
            const double f = p - fl;
            const double lo = map[i0], hi = map[i0 + 1];
            res = u - (lo + f * (hi - lo));
        }
        r[i] = res;
    }
}

template <class T>
__global__ void __launch_bounds__(BT) k_bias_exp(const T* __restrict__ I, const double* __restrict__ b, int64_t V,
                                                 double* __restrict__ corrected, double* __restrict__ field) {
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) {
        const double f = exp(b[i]);
        corrected[i] = (double)I[i] / f;
        if (field) field[i] = f;
    }
}

// ---------------------------------------------------------------- host
int stream_grid(int64_t V) { return (int)std::min<int64_t>((V + BT - 1) / BT, GRID); }

// the tables of one axis on the device: one allocation each
struct AxisSet {
    AxisHost host[3];
    AxisDev dev[3];
    int32_t* ds[3] = {};
    double* dw[3] = {};
    int alloc(DevMem& mem, const int64_t* n) {
        for (int a = 0; a < 3; a++) { VMASK_GRAB(ds[a], (size_t)n[a], "axis tables"); VMASK_GRAB(dw[a], 12 * (size_t)n[a], "axis tables"); }
        return VRG_OK;
    }
    int set(const int64_t* n, const int* M) {
        for (int a = 0; a < 3; a++) {
            AxisHost& t = host[a];
            build_axis((int)n[a], M[a], t);
            const size_t c = 4 * (size_t)n[a];
            VMASK_TRY(hipMemcpy(ds[a], t.s.data(), (size_t)n[a] * 4, hipMemcpyHostToDevice));
            VMASK_TRY(hipMemcpy(dw[a], t.w.data(), c * 8, hipMemcpyHostToDevice));
            VMASK_TRY(hipMemcpy(dw[a] + c, t.c2.data(), c * 8, hipMemcpyHostToDevice));
            VMASK_TRY(hipMemcpy(dw[a] + 2 * c, t.c3.data(), c * 8, hipMemcpyHostToDevice));
            dev[a] = AxisDev{ds[a], dw[a], dw[a] + c, dw[a] + 2 * c, (int)n[a], t.K};
        }
        return VRG_OK;
    }
};

// the work space of fit and eval at the largest lattice of a call: A holds [K0][n1][n2] (twice for the fit), B [K0][K1][n2]
struct Lattice {
    double *An = nullptr, *Ad = nullptr, *Bn = nullptr, *Bd = nullptr, *phi = nullptr;
    int alloc(DevMem& mem, const int64_t* n, const int* Mmax, bool fit) {
        const size_t K0 = Mmax[0] + 3, K1 = Mmax[1] + 3, K2 = Mmax[2] + 3;
        VMASK_GRAB(An, K0 * n[1] * n[2], "lattice work space");
        VMASK_GRAB(Bn, K0 * K1 * n[2], "lattice work space");
        if (fit) { VMASK_GRAB(Ad, K0 * n[1] * n[2], "lattice work space"); VMASK_GRAB(Bd, K0 * K1 * n[2], "lattice work space"); }
        VMASK_GRAB(phi, K0 * K1 * K2, "lattice");
        return VRG_OK;
    }
};

unsigned blocks_of(int64_t count) { return (unsigned)((count + BT - 1) / BT); }

// phi = fit(r, m): three launches on the null stream
void launch_fit(const double* r, const uint8_t* m, const int64_t* n, const AxisSet& ax, const Lattice& L) {
    const int64_t K0 = ax.dev[0].K, K1 = ax.dev[1].K;
    const int64_t c0 = n[1] * n[2], c1 = K0 * n[2], c2 = K0 * K1;
    k_bias_fit<true, false><<<blocks_of(c0), BT>>>(r, nullptr, m, c0, c0, ax.dev[0], L.An, L.Ad);
    k_bias_fit<false, false><<<blocks_of(c1), BT>>>(L.An, L.Ad, nullptr, c1, n[2], ax.dev[1], L.Bn, L.Bd);
    k_bias_fit<false, true><<<blocks_of(c2), BT>>>(L.Bn, L.Bd, nullptr, c2, 1, ax.dev[2], L.phi, nullptr);
}

// out = eval(phi), or out += eval(phi)
void launch_eval(const int64_t* n, const AxisSet& ax, const Lattice& L, double* out, bool add) {
    const int64_t K0 = ax.dev[0].K, K1 = ax.dev[1].K;
    const int64_t t2 = K0 * K1 * n[2], t1 = K0 * n[1] * n[2], inner = n[1] * n[2];
    k_bias_expand<<<blocks_of(t2), BT>>>(L.phi, t2, 1, ax.dev[2], L.Bn);
    k_bias_expand<<<blocks_of(t1), BT>>>(L.Bn, t1, n[2], ax.dev[1], L.An);
    const dim3 grid(blocks_of(inner), (unsigned)((n[0] + EZ - 1) / EZ));
    if (add) k_bias_expand0<true><<<grid, BT>>>(L.An, inner, ax.dev[0], out);
    else k_bias_expand0<false><<<grid, BT>>>(L.An, inner, ax.dev[0], out);
}

bool spans_ok(const int* M, int hi) { return M && M[0] >= 1 && M[0] <= hi && M[1] >= 1 && M[1] <= hi && M[2] >= 1 && M[2] <= hi; }
bool positive(double x) { return std::isfinite(x) && x > 0.0; }

struct LoopArgs { int m0[3]; int levels, iterations, nb; double threshold, fwhm, noise; };

int check_loop(const int* m0, int levels, int iterations, double threshold, int nb, double fwhm, double noise, LoopArgs& a) {
    if (!spans_ok(m0, 32)) { vmask::set_error("bias: the spans of the first level must be 1 to 32 per axis"); return VRG_E_ARG; }
    if (levels < 1 || levels > 6) { vmask::set_error("bias: 1 to 6 levels"); return VRG_E_ARG; }
    for (int k = 0; k < 3; k++)
        if ((m0[k] << (levels - 1)) > 64) { vmask::set_error("bias: the spans of the last level, m0 * 2^(levels - 1), must be at most 64"); return VRG_E_ARG; }
    if (iterations < 1 || iterations > 200) { vmask::set_error("bias: 1 to 200 iterations per level"); return VRG_E_ARG; }
    if (nb < 8 || nb > MAXBINS) { vmask::set_error("bias: 8 to 256 bins"); return VRG_E_ARG; }
    if (!positive(fwhm) || !positive(noise) || !positive(threshold)) { vmask::set_error("bias: fwhm, noise and threshold must be finite and positive"); return VRG_E_ARG; }
    a = LoopArgs{{m0[0], m0[1], m0[2]}, levels, iterations, nb, threshold, fwhm, noise};
    return VRG_OK;
}

// the loop on device-resident v, m and b (b is zeroed here); r is a float64 work volume
int run_loop(const double* v, const uint8_t* m, const int64_t* n, const LoopArgs& a, double* b, double* r, DevMem& mem, double* trace, int64_t* ntrace) {
    const int64_t V = n[0] * n[1] * n[2];
    const int g = stream_grid(V);
    int Mmax[3];
    for (int k = 0; k < 3; k++) Mmax[k] = a.m0[k] << (a.levels - 1);
    AxisSet ax;
    Lattice L;
    double* part = nullptr; unsigned long long* dcounts = nullptr; double* dE = nullptr;
    if (ax.alloc(mem, n) || L.alloc(mem, n, Mmax, true) || mem.grab(&part, 2 * (size_t)GRID, "partial extrema") ||
        mem.grab(&dcounts, MAXBINS, "histogram") || mem.grab(&dE, MAXBINS, "sharpening map")) {
        vmask::set_error("out of device memory (bias field: the log volume, the field, the residual, the mask and 2 (m0 2^(levels-1) + 3) n1 n2 doubles of the fit; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    VMASK_TRY(hipMemset(b, 0, (size_t)V * 8));
    std::vector<double> hpart(2 * (size_t)g), hist(a.nb), E(a.nb), hphi;
    std::vector<unsigned long long> hcounts(a.nb);
    int64_t records = 0;
    bool stop = false;
    for (int level = 0; level < a.levels && !stop; level++) {
        int M[3];
        for (int k = 0; k < 3; k++) M[k] = a.m0[k] << level;
        const int rc = ax.set(n, M);
        if (rc) return rc;
        const size_t nphi = (size_t)ax.dev[0].K * ax.dev[1].K * ax.dev[2].K;
        hphi.resize(nphi);
        for (int it = 0; it < a.iterations; it++) {
            k_bias_minmax<<<g, BT>>>(v, b, m, V, part);
            VMASK_TRY(hipMemcpy(hpart.data(), part, hpart.size() * 8, hipMemcpyDeviceToHost));
            double umin = INFINITY, umax = -INFINITY;
            for (int k = 0; k < g; k++) { umin = std::fmin(umin, hpart[2 * k]); umax = std::fmax(umax, hpart[2 * k + 1]); }
            if (umin == umax) { stop = true; break; }
            if (!(std::isfinite(umin) && std::isfinite(umax))) { vmask::set_error("bias: the log intensities over the mask must be finite"); return VRG_E_ARG; }
            const double h = (umax - umin) / (double)(a.nb - 1);
            VMASK_TRY(hipMemset(dcounts, 0, a.nb * sizeof(unsigned long long)));
            k_bias_hist<<<g, BT>>>(v, b, m, V, umin, h, a.nb, dcounts);
            VMASK_TRY(hipMemcpy(hcounts.data(), dcounts, a.nb * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            for (int k = 0; k < a.nb; k++) hist[k] = (double)hcounts[k];
            const int src = vmask_bias_sharpen(hist.data(), a.nb, umin, umax, a.fwhm, a.noise, E.data());
            if (src) return src;
            VMASK_TRY(hipMemcpy(dE, E.data(), a.nb * 8, hipMemcpyHostToDevice));
            k_bias_residual<<<g, BT>>>(v, b, m, V, umin, h, a.nb, dE, r);
            launch_fit(r, m, n, ax, L);
            launch_eval(n, ax, L, b, true);
            VMASK_TRY(hipGetLastError());
            VMASK_TRY(hipMemcpy(hphi.data(), L.phi, nphi * 8, hipMemcpyDeviceToHost));
            double top = 0.0;
            for (size_t k = 0; k < nphi; k++) top = std::fmax(top, std::fabs(hphi[k]));
            if (trace) { double* t = trace + 4 * records; t[0] = (double)level; t[1] = top; t[2] = umin; t[3] = umax; }
            records++;
            if (top < a.threshold) break;
        }
    }
    VMASK_TRY(hipDeviceSynchronize());
    if (ntrace) *ntrace = records;
    return VRG_OK;
}

template <class T>
int correct(const T* volume, const uint8_t* mask, const int64_t* n, const LoopArgs& a, double* corrected, double* field, double* trace, int64_t* ntrace) {
    const size_t V = (size_t)n[0] * n[1] * n[2];
    DevMem mem;
    const bool in_host = !vmask::is_device_pointer(volume), mask_host = mask && !vmask::is_device_pointer(mask);
    const bool cor_host = !vmask::is_device_pointer(corrected), field_host = field && !vmask::is_device_pointer(field);
    T* own_in = nullptr; uint8_t* own_mask = nullptr; double* own_cor = nullptr; double* own_field = nullptr;
    double* v = nullptr; double* b = nullptr; uint8_t* m = nullptr; unsigned long long* total = nullptr;
    if ((in_host && mem.grab(&own_in, V, "input")) || (mask_host && mem.grab(&own_mask, V, "mask")) || (cor_host && mem.grab(&own_cor, V, "corrected")) ||
        (field_host && mem.grab(&own_field, V, "field")) || mem.grab(&v, V, "log volume") || mem.grab(&b, V, "log field") || mem.grab(&m, V, "mask") ||
        mem.grab(&total, 1, "counter")) {
        vmask::set_error("out of device memory (bias correction: the input, the outputs, three float64 volumes and the mask; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    const T* dI = in_host ? own_in : volume; const uint8_t* dmask = mask_host ? own_mask : mask;
    double* dcor = cor_host ? own_cor : corrected; double* dfield = field_host ? own_field : field;
    if (in_host) VMASK_TRY(hipMemcpy(own_in, volume, V * sizeof(T), hipMemcpyHostToDevice));
    if (mask_host) VMASK_TRY(hipMemcpy(own_mask, mask, V, hipMemcpyHostToDevice));
    VMASK_TRY(hipMemset(total, 0, sizeof(unsigned long long)));
    const int g = stream_grid((int64_t)V);
    k_bias_log<T><<<g, BT>>>(dI, dmask, (int64_t)V, v, m, total);
    unsigned long long inside = 0;
    VMASK_TRY(hipMemcpy(&inside, total, sizeof inside, hipMemcpyDeviceToHost));
    if (!inside) { vmask::set_error("bias: the mask is empty (no voxel of it has a positive intensity)"); return VRG_E_ARG; }
    // the corrected volume is not needed until the end: it is the residual's work volume
    const int rc = run_loop(v, m, n, a, b, dcor, mem, trace, ntrace);
    if (rc) return rc;
    k_bias_exp<T><<<g, BT>>>(dI, b, (int64_t)V, dcor, dfield);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if (cor_host) VMASK_TRY(hipMemcpy(corrected, dcor, V * 8, hipMemcpyDeviceToHost));
    if (field_host) VMASK_TRY(hipMemcpy(field, dfield, V * 8, hipMemcpyDeviceToHost));
    return VRG_OK;
}

// out[k] = sum_p in[p] e^{sign 2 pi i k p / P}, the twiddles from a table of P entries
void dft(const double* re, const double* im, int sign, const double* tc, const double* ts, double* ore, double* oim) {
    for (int k = 0; k < PADDED; k++) {
        double ar = 0.0, ai = 0.0;
        for (int p = 0; p < PADDED; p++) {
            const int j = (k * p) & (PADDED - 1);
            const double c = tc[j], s = sign < 0 ? -ts[j] : ts[j];
            ar += re[p] * c - im[p] * s;
            ai += re[p] * s + im[p] * c;
        }
        ore[k] = ar; oim[k] = ai;
    }
}

}  // namespace

extern "C" int vmask_bias_axis_table(int n, int spans, int32_t* s, double* w, double* c2, double* c3) {
    if (!s || !w || !c2 || !c3) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (n < 1 || n > 32000 || spans < 1 || spans > 64) { vmask::set_error("bias: an extent of 1 to 32000 and 1 to 64 spans"); return VRG_E_ARG; }
    AxisHost t;
    build_axis(n, spans, t);
    for (int i = 0; i < n; i++) s[i] = t.s[i];
    for (size_t k = 0; k < 4 * (size_t)n; k++) { w[k] = t.w[k]; c2[k] = t.c2[k]; c3[k] = t.c3[k]; }
    return VRG_OK;
}

extern "C" int vmask_bias_sharpen(const double* counts, int nb, double umin, double umax, double fwhm, double noise, double* E) {
    if (!counts || !E) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nb < 8 || nb > MAXBINS) { vmask::set_error("bias: 8 to 256 bins"); return VRG_E_ARG; }
    if (!positive(fwhm) || !positive(noise)) { vmask::set_error("bias: fwhm and noise must be finite and positive"); return VRG_E_ARG; }
    if (!(std::isfinite(umin) && std::isfinite(umax) && umax > umin)) { vmask::set_error("bias: umin < umax, both finite"); return VRG_E_ARG; }
    constexpr int P = PADDED;
    const int off = (P - nb) / 2;
    const double h = (umax - umin) / (double)(nb - 1);
    const double sigma = fwhm / (2.0 * std::sqrt(2.0 * std::log(2.0))) / h;
    std::vector<double> buf(16 * (size_t)P, 0.0);
    double *tc = &buf[0], *ts = &buf[P], *G = &buf[2 * P], *Vp = &buf[3 * P], *zero = &buf[4 * P], *Gr = &buf[5 * P], *Gi = &buf[6 * P];
    double *Ar = &buf[7 * P], *Ai = &buf[8 * P], *Br = &buf[9 * P], *Bi = &buf[10 * P], *U = &buf[11 * P], *cU = &buf[12 * P];
    double *num = &buf[13 * P], *den = &buf[14 * P], *scratch = &buf[15 * P];
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < P; k++) { tc[k] = std::cos(two_pi * (double)k / (double)P); ts[k] = std::sin(two_pi * (double)k / (double)P); }
    double gsum = 0.0;
    for (int k = 0; k < P; k++) { const double d = (double)std::min(k, P - k) / sigma; G[k] = std::exp(-0.5 * (d * d)); gsum += G[k]; }
    for (int k = 0; k < P; k++) G[k] /= gsum;
    for (int k = 0; k < nb; k++) Vp[off + k] = counts[k];
    dft(G, zero, -1, tc, ts, Gr, Gi);
    dft(Vp, zero, -1, tc, ts, Ar, Ai);
    for (int k = 0; k < P; k++) {                  // conj(G^) / (|G^|^2 + noise) * V^
        const double q = (Gr[k] * Gr[k] + Gi[k] * Gi[k]) + noise;
        const double fr = Gr[k] / q, fi = -Gi[k] / q;
        Br[k] = fr * Ar[k] - fi * Ai[k];
        Bi[k] = fr * Ai[k] + fi * Ar[k];
    }
    dft(Br, Bi, +1, tc, ts, U, scratch);
    for (int k = 0; k < P; k++) { U[k] = std::fmax(U[k] / (double)P, 0.0); cU[k] = (umin + (double)(k - off) * h) * U[k]; }
    auto smooth = [&](const double* in, double* out) {      // Re IDFT(G^ . DFT(in))
        dft(in, zero, -1, tc, ts, Ar, Ai);
        for (int k = 0; k < P; k++) { Br[k] = Gr[k] * Ar[k] - Gi[k] * Ai[k]; Bi[k] = Gr[k] * Ai[k] + Gi[k] * Ar[k]; }
        dft(Br, Bi, +1, tc, ts, out, scratch);
        for (int k = 0; k < P; k++) out[k] /= (double)P;
    };
    smooth(cU, num);
    smooth(U, den);
    double top = 0.0;
    for (int k = 0; k < P; k++) top = std::fmax(top, den[k]);
    for (int k = 0; k < nb; k++) E[k] = den[off + k] > 1e-12 * top ? num[off + k] / den[off + k] : umin + (double)k * h;
    return VRG_OK;
}

extern "C" int vmask_bias_fit(int device, const double* r, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const int* spans, double* phi) {
    if (!r || !mask || !spans || !phi) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!spans_ok(spans, 64)) { vmask::set_error("bias: 1 to 64 spans per axis"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2};
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    AxisSet ax;
    Lattice L;
    const bool r_host = !vmask::is_device_pointer(r), m_host = !vmask::is_device_pointer(mask);
    double* own_r = nullptr; uint8_t* own_m = nullptr;
    if ((r_host && mem.grab(&own_r, V, "residual")) || (m_host && mem.grab(&own_m, V, "mask")) || ax.alloc(mem, n) || L.alloc(mem, n, spans, true)) {
        vmask::set_error("out of device memory (bias fit)");
        return VRG_E_MEM;
    }
    const double* dr = r_host ? own_r : r; const uint8_t* dm = m_host ? own_m : mask;
    if (r_host) VMASK_TRY(hipMemcpy(own_r, r, V * 8, hipMemcpyHostToDevice));
    if (m_host) VMASK_TRY(hipMemcpy(own_m, mask, V, hipMemcpyHostToDevice));
    const int src = ax.set(n, spans);
    if (src) return src;
    launch_fit(dr, dm, n, ax, L);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    VMASK_TRY(hipMemcpy(phi, L.phi, (size_t)ax.dev[0].K * ax.dev[1].K * ax.dev[2].K * 8, hipMemcpyDefault));
    return VRG_OK;
}

extern "C" int vmask_bias_eval(int device, const double* phi, const int* spans, int64_t n0, int64_t n1, int64_t n2, double* out) {
    if (!phi || !spans || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!spans_ok(spans, 64)) { vmask::set_error("bias: 1 to 64 spans per axis"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2};
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    AxisSet ax;
    Lattice L;
    const bool out_host = !vmask::is_device_pointer(out);
    double* own_out = nullptr;
    if ((out_host && mem.grab(&own_out, V, "output")) || ax.alloc(mem, n) || L.alloc(mem, n, spans, false)) {
        vmask::set_error("out of device memory (bias evaluation)");
        return VRG_E_MEM;
    }
    double* dout = out_host ? own_out : out;
    const int src = ax.set(n, spans);
    if (src) return src;
    VMASK_TRY(hipMemcpy(L.phi, phi, (size_t)ax.dev[0].K * ax.dev[1].K * ax.dev[2].K * 8, hipMemcpyDefault));
    launch_eval(n, ax, L, dout, false);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if (out_host) VMASK_TRY(hipMemcpy(out, dout, V * 8, hipMemcpyDeviceToHost));
    return VRG_OK;
}

extern "C" int vmask_bias_log_field(int device, const double* v, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const int* m0, int levels,
                                    int iterations, double threshold, int nb, double fwhm, double noise, double* b, double* trace, int64_t* ntrace) {
    if (!v || !mask || !m0 || !b) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    LoopArgs a;
    int rc = check_loop(m0, levels, iterations, threshold, nb, fwhm, noise, a);
    if (rc) return rc;
    rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2};
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const bool v_host = !vmask::is_device_pointer(v), m_host = !vmask::is_device_pointer(mask), b_host = !vmask::is_device_pointer(b);
    double* own_v = nullptr; uint8_t* own_m = nullptr; double* own_b = nullptr; double* r = nullptr; unsigned long long* total = nullptr;
    if ((v_host && mem.grab(&own_v, V, "log volume")) || (m_host && mem.grab(&own_m, V, "mask")) || (b_host && mem.grab(&own_b, V, "log field")) ||
        mem.grab(&r, V, "residual") || mem.grab(&total, 1, "counter")) {
        vmask::set_error("out of device memory (bias field: the log volume, the mask, the field and the residual; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    const double* dv = v_host ? own_v : v; const uint8_t* dm = m_host ? own_m : mask; double* db = b_host ? own_b : b;
    if (v_host) VMASK_TRY(hipMemcpy(own_v, v, V * 8, hipMemcpyHostToDevice));
    if (m_host) VMASK_TRY(hipMemcpy(own_m, mask, V, hipMemcpyHostToDevice));
    VMASK_TRY(hipMemset(total, 0, sizeof(unsigned long long)));
    k_bias_count<<<stream_grid((int64_t)V), BT>>>(dm, (int64_t)V, total);
    unsigned long long inside = 0;
    VMASK_TRY(hipMemcpy(&inside, total, sizeof inside, hipMemcpyDeviceToHost));
    if (!inside) { vmask::set_error("bias: the mask is empty"); return VRG_E_ARG; }
    rc = run_loop(dv, dm, n, a, db, r, mem, trace, ntrace);
    if (rc) return rc;
    if (b_host) VMASK_TRY(hipMemcpy(b, db, V * 8, hipMemcpyDeviceToHost));
    return VRG_OK;
}

extern "C" int vmask_bias_correct(int device, const void* volume, int dtype, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const int* m0, int levels,
                                  int iterations, double threshold, int nb, double fwhm, double noise, double* corrected, double* field,
                                  double* trace, int64_t* ntrace) {
    if (!volume || !m0 || !corrected) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (dtype != VRG_F32 && dtype != VRG_F64) { vmask::set_error("bias: the volume must be float32 or float64"); return VRG_E_ARG; }
    LoopArgs a;
    int rc = check_loop(m0, levels, iterations, threshold, nb, fwhm, noise, a);
    if (rc) return rc;
    rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2};
    if (dtype == VRG_F32) return correct<float>((const float*)volume, mask, n, a, corrected, field, trace, ntrace);
    return correct<double>((const double*)volume, mask, n, a, corrected, field, trace, ntrace);
}
