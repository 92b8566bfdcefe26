// vwarp_device.hip - vmask_warp_* of include/vmask.h: nonlinear registration by a B-spline demons warp, the part of the reference's
// "register multiple sets of images" step that its README leaves to FSL fnirt (entry f18).  A displacement u on
// the fixed grid is refined by demons forces that a multilevel B-spline fit smooths; the pyramid and the levels are host Python
// (registration.py), one level's iterations are vmask_warp_field here.
//
//   k_warp_force<TF, TM>  the force pass.  A thread owns one (i1, i2) column - 256 consecutive columns per workgroup, so lanes run
//                  along axis 2 and the reads of F, the mask and u and the writes of delta and part coalesce - and marches over
//                  axis 0 in ascending order, which is the order of the cost's innermost sum: the column's sum of r^2 and its
//                  count leave the kernel once.  The 12 doubles of the voxel map and the scales are kernel arguments.
//   k_warp_rows    the cost's sum over axis 1: a thread per i2; the n2 sums that remain are added on the host.
//   k_warp_fit<FIRST, LAST>  one contraction of the fit with three numerators and the one denominator they share: k_bias_fit's
//                  march (vbias_device.hip), a window of four control points in registers, 12 + 4 accumulators.
//   k_warp_expand, k_warp_expand0  the evaluation of the three lattices in one launch each (the component is an outer index), the
//                  last one fused with u <- u + F, as k_bias_expand0<ADD>.
//   k_warp_up      u of the next finer level: 2 x the trilinear sample of the coarse u, indices clamped.
//   k_warp_linear<T>, k_warp_nearest<T>  a volume resampled through the affine map and the warp.
// float64 throughout, nothing contracted; no float atomics, no atomics at all.  No scratch.  No barrier in the marching kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vreg_walk.h"

#pragma clang fp contract(off)

namespace {

constexpr int WT = 256;                            // every kernel: 4 waves
constexpr int WZ = 32;                             // k_warp_expand0: the planes of axis 0 that a workgroup marches over
constexpr int WGRID = 1024;                        // the grid-stride passes (k_warp_up, k_warp_linear, k_warp_nearest): at most this many workgroups

struct WarpMap { double t[12]; };                  // the first three rows of T: fixed voxel -> moving voxel
struct WarpScale { double flo, fs, mlo, ms, a2; };
struct AxisDev { const int32_t* s; const double* w; const double* c2; const double* c3; int n, K; };

__device__ __forceinline__ double coord(const WarpMap& M, int a, double q0, double q1, double q2) {
    return ((M.t[4 * a] * q0 + M.t[4 * a + 1] * q1) + M.t[4 * a + 2] * q2) + M.t[4 * a + 3];
}

__device__ __forceinline__ bool inside_of(const Ext m, double p0, double p1, double p2) {      // (a NaN fails every comparison)
    return p0 >= 0.0 && p0 <= (double)(m.n0 - 1) && p1 >= 0.0 && p1 <= (double)(m.n1 - 1) && p2 >= 0.0 && p2 <= (double)(m.n2 - 1);
}

// the 8 corners of the sample at an inside p, as doubles, and the three fractions: the floor, the clamp and the order of vmask_reg_joint_hist
template <class T> struct Corners { double v000, v001, v010, v011, v100, v101, v110, v111, t0, t1, t2; };

template <class T>
__device__ __forceinline__ void corners(const T* __restrict__ mov, const Ext m, double p0, double p1, double p2, Corners<T>& c) {
    const double f0 = floor(p0), f1 = floor(p1), f2 = floor(p2);
    c.t0 = p0 - f0; c.t1 = p1 - f1; c.t2 = p2 - f2;
    const int a0 = (int)f0, b0 = (int)f1, c0 = (int)f2;                            // 0 .. m - 1
    const int a1 = min(a0 + 1, m.n0 - 1), b1 = min(b0 + 1, m.n1 - 1), c1 = min(c0 + 1, m.n2 - 1);
    const int64_t r00 = ((int64_t)a0 * m.n1 + b0) * m.n2, r01 = ((int64_t)a0 * m.n1 + b1) * m.n2;
    const int64_t r10 = ((int64_t)a1 * m.n1 + b0) * m.n2, r11 = ((int64_t)a1 * m.n1 + b1) * m.n2;
    c.v000 = (double)mov[r00 + c0]; c.v001 = (double)mov[r00 + c1]; c.v010 = (double)mov[r01 + c0]; c.v011 = (double)mov[r01 + c1];
    c.v100 = (double)mov[r10 + c0]; c.v101 = (double)mov[r10 + c1]; c.v110 = (double)mov[r11 + c0]; c.v111 = (double)mov[r11 + c1];
}

// the trilinear sample at p: false where p is outside or the sample is not finite
template <class T>
__device__ __forceinline__ bool sample_at(const T* __restrict__ mov, const Ext m, double p0, double p1, double p2, double& value) {
    if (!inside_of(m, p0, p1, p2)) return false;
    Corners<T> c;
    corners<T>(mov, m, p0, p1, p2, c);
    const double x00 = c.v000 + c.t2 * (c.v001 - c.v000), x01 = c.v010 + c.t2 * (c.v011 - c.v010);
    const double x10 = c.v100 + c.t2 * (c.v101 - c.v100), x11 = c.v110 + c.t2 * (c.v111 - c.v110);
    const double y0 = x00 + c.t1 * (x01 - x00), y1 = x10 + c.t1 * (x11 - x10);
    value = y0 + c.t0 * (y1 - y0);
    return isfinite(value);
}

// ---------------------------------------------------------------- the force pass
template <class TF, class TM>
__global__ void __launch_bounds__(WT) k_warp_force(const TF* __restrict__ F, const uint8_t* __restrict__ mask, const double* __restrict__ u, int64_t V,
                                                   Ext n, const TM* __restrict__ mov, Ext m, WarpMap M, WarpScale sc, double* __restrict__ delta,
                                                   uint8_t* __restrict__ part, double* __restrict__ colS, unsigned int* __restrict__ colC) {
    const int64_t inner = (int64_t)n.n1 * n.n2;
    const int64_t col = (int64_t)blockIdx.x * WT + threadIdx.x;
    if (col >= inner) return;                      // (no barrier in this kernel)
    const int j = (int)(col / n.n2), k = (int)(col - (int64_t)j * n.n2);
    double S = 0.0;
    unsigned int count = 0;                        // (an axis has at most 32000 voxels)
    for (int i = 0; i < n.n0; i++) {
        const int64_t at = (int64_t)i * inner + col;
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
        uint8_t in = 0;
        const double f = (double)F[at];
        if ((!mask || mask[at]) && isfinite(f)) {
            const double q0 = (double)i + u[at], q1 = (double)j + u[V + at], q2 = (double)k + u[2 * V + at];
            const double p0 = coord(M, 0, q0, q1, q2), p1 = coord(M, 1, q0, q1, q2), p2 = coord(M, 2, q0, q1, q2);
            if (inside_of(m, p0, p1, p2)) {
                Corners<TM> c;
                corners<TM>(mov, m, p0, p1, p2, c);
                const double x00 = c.v000 + c.t2 * (c.v001 - c.v000), x01 = c.v010 + c.t2 * (c.v011 - c.v010);
                const double x10 = c.v100 + c.t2 * (c.v101 - c.v100), x11 = c.v110 + c.t2 * (c.v111 - c.v110);
                const double y0 = x00 + c.t1 * (x01 - x00), y1 = x10 + c.t1 * (x11 - x10);
                const double value = y0 + c.t0 * (y1 - y0);
                if (isfinite(value)) {
                    in = 1;
                    const double r = (f - sc.flo) * sc.fs - (value - sc.mlo) * sc.ms;
                    // the interpolant's gradient in moving voxels, from the same corners
                    const double g0 = y1 - y0;
                    const double e0 = x01 - x00, e1 = x11 - x10;
                    const double g1 = e0 + c.t0 * (e1 - e0);
                    const double d00 = c.v001 - c.v000, d01 = c.v011 - c.v010, d10 = c.v101 - c.v100, d11 = c.v111 - c.v110;
                    const double h0 = d00 + c.t1 * (d01 - d00), h1 = d10 + c.t1 * (d11 - d10);
                    const double g2 = h0 + c.t0 * (h1 - h0);
                    const double G0 = ((g0 * M.t[0] + g1 * M.t[4]) + g2 * M.t[8]) * sc.ms;
                    const double G1 = ((g0 * M.t[1] + g1 * M.t[5]) + g2 * M.t[9]) * sc.ms;
                    const double G2 = ((g0 * M.t[2] + g1 * M.t[6]) + g2 * M.t[10]) * sc.ms;
                    const double rr = r * r;
                    const double den = ((G0 * G0 + G1 * G1) + G2 * G2) + rr * sc.a2;
                    if (den > 0.0 && isfinite(den)) { d0 = (r * G0) / den; d1 = (r * G1) / den; d2 = (r * G2) / den; }
                    S = S + rr;
                    count++;
                }
            }
        }
        delta[at] = d0; delta[V + at] = d1; delta[2 * V + at] = d2;
        part[at] = in;
    }
    colS[col] = S;
    colC[col] = count;
}

// rowS[k] = sum over j, ascending from +0.0, of colS[j][k]; rowC likewise (integers)
__global__ void __launch_bounds__(WT) k_warp_rows(const double* __restrict__ colS, const unsigned int* __restrict__ colC, int n1, int n2,
                                                  double* __restrict__ rowS, unsigned long long* __restrict__ rowC) {
    const int k = (int)blockIdx.x * WT + (int)threadIdx.x;
    if (k >= n2) return;
    double S = 0.0;
    unsigned long long count = 0;
    for (int j = 0; j < n1; j++) {
        const int64_t at = (int64_t)j * n2 + k;
        S = S + colS[at];
        count += colC[at];
    }
    rowS[k] = S;
    rowC[k] = count;
}

// ---------------------------------------------------------------- the fit: three numerators, one denominator
// [outer][n][inner] -> [outer][K][inner]; component c of the numerators lies cin (cout) doubles after component c - 1
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(WT) k_warp_fit(const double* __restrict__ An, const double* __restrict__ Ad, const uint8_t* __restrict__ part,
                                                 int64_t cols, int64_t inner, int64_t cin, int64_t cout, AxisDev ax, double* __restrict__ On,
                                                 double* __restrict__ Od) {
    const int64_t t = (int64_t)blockIdx.x * WT + threadIdx.x;
    if (t >= cols) return;                         // (no barrier in this kernel)
    const int64_t o = t / inner, q = t - o * inner;
    const int64_t in0 = o * ax.n * inner + q, out0 = o * ax.K * inner + q;
    double A0 = 0.0, A1 = 0.0, A2 = 0.0, A3 = 0.0, B0 = 0.0, B1 = 0.0, B2 = 0.0, B3 = 0.0, C0 = 0.0, C1 = 0.0, C2 = 0.0, C3 = 0.0;
    double D0 = 0.0, D1 = 0.0, D2 = 0.0, D3 = 0.0;
    int base = 0;                                  // the control point of A0 / B0 / C0 / D0
    auto retire = [&]() {
        const int64_t at = out0 + (int64_t)base * inner;
        if (LAST) {
            const bool ok = D0 > 0.0;
            On[at] = ok ? A0 / D0 : 0.0; On[cout + at] = ok ? B0 / D0 : 0.0; On[2 * cout + at] = ok ? C0 / D0 : 0.0;
        } else { On[at] = A0; On[cout + at] = B0; On[2 * cout + at] = C0; Od[at] = D0; }
        A0 = A1; A1 = A2; A2 = A3; A3 = 0.0;
        B0 = B1; B1 = B2; B2 = B3; B3 = 0.0;
        C0 = C1; C1 = C2; C2 = C3; C3 = 0.0;
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
            if (part[at]) {                        // (a voxel that takes no part costs its byte)
                const double a = An[at], b = An[cin + at], c = An[2 * cin + at];
                A0 = A0 + c3[0] * a; A1 = A1 + c3[1] * a; A2 = A2 + c3[2] * a; A3 = A3 + c3[3] * a;
                B0 = B0 + c3[0] * b; B1 = B1 + c3[1] * b; B2 = B2 + c3[2] * b; B3 = B3 + c3[3] * b;
                C0 = C0 + c3[0] * c; C1 = C1 + c3[1] * c; C2 = C2 + c3[2] * c; C3 = C3 + c3[3] * c;
                D0 = D0 + c2[0]; D1 = D1 + c2[1]; D2 = D2 + c2[2]; D3 = D3 + c2[3];
            }
        } else {
            const double a = An[at], b = An[cin + at], c = An[2 * cin + at], d = Ad[at];
            A0 = A0 + c3[0] * a; A1 = A1 + c3[1] * a; A2 = A2 + c3[2] * a; A3 = A3 + c3[3] * a;
            B0 = B0 + c3[0] * b; B1 = B1 + c3[1] * b; B2 = B2 + c3[2] * b; B3 = B3 + c3[3] * b;
            C0 = C0 + c3[0] * c; C1 = C1 + c3[1] * c; C2 = C2 + c3[2] * c; C3 = C3 + c3[3] * c;
            D0 = D0 + c2[0] * d; D1 = D1 + c2[1] * d; D2 = D2 + c2[2] * d; D3 = D3 + c2[3] * d;
        }
    }
    while (base < ax.K) retire();
}

// ---------------------------------------------------------------- the evaluation, the three lattices at once
// [outer][K][inner] -> [outer][n][inner]; the component is part of `outer`
__global__ void __launch_bounds__(WT) k_warp_expand(const double* __restrict__ in, int64_t total, int64_t inner, AxisDev ax, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * WT + threadIdx.x;
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

// u[c] <- u[c] + the expansion along axis 0 of E1[c], c = blockIdx.z
__global__ void __launch_bounds__(WT) k_warp_expand0(const double* __restrict__ E1, int64_t inner, AxisDev ax, double* __restrict__ u) {
    const int64_t q = (int64_t)blockIdx.x * WT + threadIdx.x;
    if (q >= inner) return;                        // (no barrier in this kernel)
    const int x0 = (int)blockIdx.y * WZ, x1 = min(x0 + WZ, ax.n);
    int sb = ax.s[x0];
    const double* p = E1 + (int64_t)blockIdx.z * ax.K * inner + q;
    double* out = u + (int64_t)blockIdx.z * ax.n * inner;
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
        out[at] = out[at] + acc;
    }
}

// ---------------------------------------------------------------- between levels
__device__ __forceinline__ void up_axis(int i, int nc, int& lo, int& hi, double& t) {
    double c = ((double)i - 0.5) * 0.5;
    c = c < 0.0 ? 0.0 : (c > (double)(nc - 1) ? (double)(nc - 1) : c);
    const double f = floor(c);
    t = c - f;
    lo = (int)f;
    hi = min(lo + 1, nc - 1);
}

__global__ void __launch_bounds__(WT) k_warp_up(const double* __restrict__ coarse, Ext c, int64_t C, Ext n, int64_t V, double* __restrict__ fine) {
    for (int64_t v = (int64_t)blockIdx.x * WT + threadIdx.x; v < V; v += (int64_t)gridDim.x * WT) {
        int i, j, k, a0, a1, b0, b1, c0, c1;
        double t0, t1, t2;
        split(v, n, i, j, k);
        up_axis(i, c.n0, a0, a1, t0);
        up_axis(j, c.n1, b0, b1, t1);
        up_axis(k, c.n2, c0, c1, t2);
        const int64_t r00 = ((int64_t)a0 * c.n1 + b0) * c.n2, r01 = ((int64_t)a0 * c.n1 + b1) * c.n2;
        const int64_t r10 = ((int64_t)a1 * c.n1 + b0) * c.n2, r11 = ((int64_t)a1 * c.n1 + b1) * c.n2;
        for (int comp = 0; comp < 3; comp++) {
            const double* p = coarse + comp * C;
            const double v000 = p[r00 + c0], v001 = p[r00 + c1], v010 = p[r01 + c0], v011 = p[r01 + c1];
            const double v100 = p[r10 + c0], v101 = p[r10 + c1], v110 = p[r11 + c0], v111 = p[r11 + c1];
            const double x00 = v000 + t2 * (v001 - v000), x01 = v010 + t2 * (v011 - v010);
            const double x10 = v100 + t2 * (v101 - v100), x11 = v110 + t2 * (v111 - v110);
            const double y0 = x00 + t1 * (x01 - x00), y1 = x10 + t1 * (x11 - x10);
            fine[comp * V + v] = 2.0 * (y0 + t0 * (y1 - y0));
        }
    }
}

// ---------------------------------------------------------------- the resampled volume
template <class T>
__global__ void __launch_bounds__(WT) k_warp_linear(const T* __restrict__ mov, Ext m, WarpMap M, const double* __restrict__ u, double fill, Ext n,
                                                    int64_t V, double* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * WT + threadIdx.x; v < V; v += (int64_t)gridDim.x * WT) {
        int i, j, k;
        split(v, n, i, j, k);
        const double q0 = (double)i + u[v], q1 = (double)j + u[V + v], q2 = (double)k + u[2 * V + v];
        double value;
        out[v] = sample_at<T>(mov, m, coord(M, 0, q0, q1, q2), coord(M, 1, q0, q1, q2), coord(M, 2, q0, q1, q2), value) ? value : fill;
    }
}

template <class T>
__global__ void __launch_bounds__(WT) k_warp_nearest(const T* __restrict__ mov, Ext m, WarpMap M, const double* __restrict__ u, T fill, Ext n,
                                                     int64_t V, T* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * WT + threadIdx.x; v < V; v += (int64_t)gridDim.x * WT) {
        int i, j, k;
        split(v, n, i, j, k);
        const double q0 = (double)i + u[v], q1 = (double)j + u[V + v], q2 = (double)k + u[2 * V + v];
        const double r0 = floor(coord(M, 0, q0, q1, q2) + 0.5), r1 = floor(coord(M, 1, q0, q1, q2) + 0.5), r2 = floor(coord(M, 2, q0, q1, q2) + 0.5);
        out[v] = inside_of(m, r0, r1, r2) ? mov[((int64_t)(int)r0 * m.n1 + (int)r1) * m.n2 + (int)r2] : fill;
    }
}

// ---------------------------------------------------------------- host
int stream_grid(int64_t V) { return (int)std::min<int64_t>((V + WT - 1) / WT, WGRID); }
unsigned blocks_of(int64_t count) { return (unsigned)((count + WT - 1) / WT); }

size_t size_of(int dtype) {
    switch (dtype) {
        case VRG_U8: return 1;
        case VRG_I16: return 2;
        case VRG_I32: case VRG_F32: return 4;
        case VRG_F64: return 8;
        default: return 0;
    }
}

bool is_float(int dtype) { return dtype == VRG_F32 || dtype == VRG_F64; }
bool positive(double x) { return std::isfinite(x) && x > 0.0; }
bool spans_ok(const int* M) { return M[0] >= 1 && M[0] <= 64 && M[1] >= 1 && M[1] <= 64 && M[2] >= 1 && M[2] <= 64; }
Ext ext_of(const int64_t* n) { return Ext{(int)n[0], (int)n[1], (int)n[2]}; }

int check_map(const double* T, WarpMap& M) {
    for (int k = 0; k < 12; k++) {
        if (!std::isfinite(T[k])) { vmask::set_error("warp: the voxel map must be finite"); return VRG_E_ARG; }
        M.t[k] = T[k];
    }
    return VRG_OK;
}

// what the force pass takes beside its arrays
int check_force(int fdtype, int mdtype, const double* T, double flo, double fs, double mlo, double ms, double maxStep, WarpMap& M, WarpScale& sc) {
    if (!is_float(fdtype) || !is_float(mdtype)) { vmask::set_error("warp: the volumes must be float32 or float64"); return VRG_E_ARG; }
    if (!std::isfinite(flo) || !std::isfinite(fs) || !std::isfinite(mlo) || !std::isfinite(ms)) { vmask::set_error("warp: the intensity origins and scales must be finite"); return VRG_E_ARG; }
    if (!positive(maxStep)) { vmask::set_error("warp: maxStep must be finite and positive"); return VRG_E_ARG; }
    sc = WarpScale{flo, fs, mlo, ms, 1.0 / ((4.0 * maxStep) * maxStep)};
    if (!std::isfinite(sc.a2)) { vmask::set_error("warp: maxStep is too small"); return VRG_E_ARG; }
    return check_map(T, M);
}

// both shapes inside the envelope of the other passes, the device made current
int check_shapes(int device, const int64_t* n, const int64_t* m) {
    if (!vmask::shape_in_envelope(m[0], m[1], m[2])) { vmask::set_error("shape of the moving volume out of range"); return VRG_E_ARG; }
    return vmask::check_args(device, n[0], n[1], n[2]);
}

// the tables of the three axes on the device (vmask_bias_axis_table's), allocated once for a call
struct Axes {
    AxisDev dev[3];
    int32_t* ds[3] = {};
    double* dw[3] = {};
    int alloc(DevMem& mem, const int64_t* n) {
        for (int a = 0; a < 3; a++) { VMASK_GRAB(ds[a], (size_t)n[a], "axis tables"); VMASK_GRAB(dw[a], 12 * (size_t)n[a], "axis tables"); }
        return VRG_OK;
    }
    int set(const int64_t* n, const int* M) {
        for (int a = 0; a < 3; a++) {
            const size_t c = 4 * (size_t)n[a];
            std::vector<int32_t> s((size_t)n[a]);
            std::vector<double> w(3 * c);
            const int rc = vmask_bias_axis_table((int)n[a], M[a], s.data(), w.data(), w.data() + c, w.data() + 2 * c);
            if (rc) return rc;
            VMASK_TRY(hipMemcpy(ds[a], s.data(), (size_t)n[a] * 4, hipMemcpyHostToDevice));
            VMASK_TRY(hipMemcpy(dw[a], w.data(), 3 * c * 8, hipMemcpyHostToDevice));
            dev[a] = AxisDev{ds[a], dw[a], dw[a] + c, dw[a] + 2 * c, (int)n[a], M[a] + 3};
        }
        return VRG_OK;
    }
};

// the work space of fit and evaluation: A holds [3][K0][n1][n2] numerators (and [K0][n1][n2] denominators), B [3][K0][K1][n2]
struct Lattice {
    double *An = nullptr, *Ad = nullptr, *Bn = nullptr, *Bd = nullptr, *phi = nullptr;
    int alloc(DevMem& mem, const int64_t* n, const int* M) {
        const size_t K0 = M[0] + 3, K1 = M[1] + 3, K2 = M[2] + 3;
        VMASK_GRAB(An, 3 * K0 * n[1] * n[2], "lattice work space");
        VMASK_GRAB(Bn, 3 * K0 * K1 * n[2], "lattice work space");
        VMASK_GRAB(Ad, K0 * n[1] * n[2], "lattice work space");
        VMASK_GRAB(Bd, K0 * K1 * n[2], "lattice work space");
        VMASK_GRAB(phi, 3 * K0 * K1 * K2, "lattice");
        return VRG_OK;
    }
};

// phi[3] = fit(delta[3], part): three launches on the null stream
void launch_fit(const double* delta, const uint8_t* part, const int64_t* n, const Axes& ax, const Lattice& L) {
    const int64_t K0 = ax.dev[0].K, K1 = ax.dev[1].K, K2 = ax.dev[2].K;
    const int64_t c0 = n[1] * n[2], c1 = K0 * n[2], c2 = K0 * K1;
    k_warp_fit<true, false><<<blocks_of(c0), WT>>>(delta, nullptr, part, c0, c0, n[0] * c0, K0 * c0, ax.dev[0], L.An, L.Ad);
    k_warp_fit<false, false><<<blocks_of(c1), WT>>>(L.An, L.Ad, nullptr, c1, n[2], K0 * c0, c2 * n[2], ax.dev[1], L.Bn, L.Bd);
    k_warp_fit<false, true><<<blocks_of(c2), WT>>>(L.Bn, L.Bd, nullptr, c2, 1, c2 * n[2], c2 * K2, ax.dev[2], L.phi, nullptr);
}

// u[3] += eval(phi[3])
void launch_add(const int64_t* n, const Axes& ax, const Lattice& L, double* u) {
    const int64_t K0 = ax.dev[0].K, K1 = ax.dev[1].K;
    const int64_t t2 = 3 * K0 * K1 * n[2], t1 = 3 * K0 * n[1] * n[2], inner = n[1] * n[2];
    k_warp_expand<<<blocks_of(t2), WT>>>(L.phi, t2, 1, ax.dev[2], L.Bn);
    k_warp_expand<<<blocks_of(t1), WT>>>(L.Bn, t1, n[2], ax.dev[1], L.An);
    k_warp_expand0<<<dim3(blocks_of(inner), (unsigned)((n[0] + WZ - 1) / WZ), 3), WT>>>(L.An, inner, ax.dev[0], u);
}

// the buffers of the force pass's cost
struct CostMem {
    double *colS = nullptr, *rowS = nullptr;
    unsigned int* colC = nullptr;
    unsigned long long* rowC = nullptr;
    int alloc(DevMem& mem, const int64_t* n) {
        VMASK_GRAB(colS, (size_t)n[1] * n[2], "column sums"); VMASK_GRAB(colC, (size_t)n[1] * n[2], "column counts");
        VMASK_GRAB(rowS, (size_t)n[2], "row sums"); VMASK_GRAB(rowC, (size_t)n[2], "row counts");
        return VRG_OK;
    }
};

// one force pass on device arrays: delta, part, and on the host S and count
int run_force(const void* dF, int fdtype, const uint8_t* dmask, const double* du, const int64_t* n, const void* dmov, int mdtype, const int64_t* m,
              const WarpMap& M, const WarpScale& sc, double* ddelta, uint8_t* dpart, const CostMem& cm, double* S, int64_t* count) {
    const int64_t V = n[0] * n[1] * n[2], inner = n[1] * n[2];
    const Ext en = ext_of(n), em = ext_of(m);
    const unsigned g = blocks_of(inner);
    if (fdtype == VRG_F32 && mdtype == VRG_F32) k_warp_force<float, float><<<g, WT>>>((const float*)dF, dmask, du, V, en, (const float*)dmov, em, M, sc, ddelta, dpart, cm.colS, cm.colC);
    else if (fdtype == VRG_F32) k_warp_force<float, double><<<g, WT>>>((const float*)dF, dmask, du, V, en, (const double*)dmov, em, M, sc, ddelta, dpart, cm.colS, cm.colC);
    else if (mdtype == VRG_F32) k_warp_force<double, float><<<g, WT>>>((const double*)dF, dmask, du, V, en, (const float*)dmov, em, M, sc, ddelta, dpart, cm.colS, cm.colC);
    else k_warp_force<double, double><<<g, WT>>>((const double*)dF, dmask, du, V, en, (const double*)dmov, em, M, sc, ddelta, dpart, cm.colS, cm.colC);
    k_warp_rows<<<blocks_of(n[2]), WT>>>(cm.colS, cm.colC, (int)n[1], (int)n[2], cm.rowS, cm.rowC);
    VMASK_TRY(hipGetLastError());
    std::vector<double> hS((size_t)n[2]);
    std::vector<unsigned long long> hC((size_t)n[2]);
    VMASK_TRY(hipMemcpy(hS.data(), cm.rowS, hS.size() * 8, hipMemcpyDeviceToHost));
    VMASK_TRY(hipMemcpy(hC.data(), cm.rowC, hC.size() * 8, hipMemcpyDeviceToHost));
    double total = 0.0;
    unsigned long long c = 0;
    for (size_t k = 0; k < hS.size(); k++) { total = total + hS[k]; c += hC[k]; }
    *S = total; *count = (int64_t)c;
    return VRG_OK;
}

template <class T> bool fill_fits(double fill) {
    if (std::is_floating_point<T>::value) return true;
    return std::isfinite(fill) && std::floor(fill) == fill && fill >= (double)std::numeric_limits<T>::lowest() && fill <= (double)std::numeric_limits<T>::max();
}

bool fill_ok(int dtype, double fill) {
    return dtype == VRG_U8 ? fill_fits<uint8_t>(fill) : dtype == VRG_I16 ? fill_fits<int16_t>(fill) : dtype == VRG_I32 ? fill_fits<int32_t>(fill) : true;
}

template <class T> void nearest(const void* dmov, Ext m, const WarpMap& M, const double* du, double fill, Ext n, int64_t V, void* dout) {
    k_warp_nearest<T><<<stream_grid(V), WT>>>((const T*)dmov, m, M, du, (T)fill, n, V, (T*)dout);
}

}  // namespace

extern "C" int vmask_warp_force(int device, const void* fixed, int fdtype, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const double* u,
                                const void* moving, int mdtype, int64_t m0, int64_t m1, int64_t m2, const double* T, double flo, double fs, double mlo,
                                double ms, double maxStep, double* delta, uint8_t* part, double* S, int64_t* count) {
    if (!fixed || !u || !moving || !T || !delta || !part || !S || !count) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    WarpMap M; WarpScale sc;
    const int64_t n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
    int rc = check_force(fdtype, mdtype, T, flo, fs, mlo, ms, maxStep, M, sc);
    if (!rc) rc = check_shapes(device, n, m);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2, W = (size_t)m0 * m1 * m2;
    DevMem mem;
    const uint8_t* dF = nullptr; const uint8_t* dmov = nullptr; const uint8_t* dmask = nullptr; const double* du = nullptr;
    Out<double> ddelta; Out<uint8_t> dpart;
    CostMem cm;
    if ((rc = bring(mem, (const uint8_t*)fixed, V * size_of(fdtype), "fixed volume", &dF)) || (mask && (rc = bring(mem, mask, V, "mask", &dmask))) ||
        (rc = bring(mem, u, 3 * V, "warp", &du)) || (rc = bring(mem, (const uint8_t*)moving, W * size_of(mdtype), "moving volume", &dmov)) ||
        (rc = ddelta.open(mem, delta, 3 * V, "forces")) || (rc = dpart.open(mem, part, V, "participation")) || (rc = cm.alloc(mem, n))) return rc;
    double total; int64_t c;
    rc = run_force(dF, fdtype, dmask, du, n, dmov, mdtype, m, M, sc, ddelta.dev, dpart.dev, cm, &total, &c);
    if (rc) return rc;
    VMASK_TRY(hipDeviceSynchronize());
    if ((rc = ddelta.close()) || (rc = dpart.close())) return rc;
    *S = total; *count = c;
    return VRG_OK;
}

extern "C" int vmask_warp_fit(int device, const double* delta, const uint8_t* part, int64_t n0, int64_t n1, int64_t n2, const int* spans, double* phi) {
    if (!delta || !part || !spans || !phi) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!spans_ok(spans)) { vmask::set_error("warp: 1 to 64 spans per axis"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2};
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    Axes ax; Lattice L;
    const double* dd = nullptr; const uint8_t* dp = nullptr;
    if ((rc = bring(mem, delta, 3 * V, "forces", &dd)) || (rc = bring(mem, part, V, "participation", &dp)) || (rc = ax.alloc(mem, n)) ||
        (rc = L.alloc(mem, n, spans)) || (rc = ax.set(n, spans))) return rc;
    launch_fit(dd, dp, n, ax, L);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    VMASK_TRY(hipMemcpy(phi, L.phi, 3 * (size_t)ax.dev[0].K * ax.dev[1].K * ax.dev[2].K * 8, hipMemcpyDefault));
    return VRG_OK;
}

extern "C" int vmask_warp_upsample(int device, const double* coarse, int64_t c0, int64_t c1, int64_t c2, double* fine, int64_t n0, int64_t n1, int64_t n2) {
    if (!coarse || !fine) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    const int64_t n[3] = {n0, n1, n2}, c[3] = {c0, c1, c2};
    if (!vmask::shape_in_envelope(c0, c1, c2)) { vmask::set_error("shape of the coarse warp out of range"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2, C = (size_t)c0 * c1 * c2;
    DevMem mem;
    const double* dc = nullptr;
    Out<double> df;
    if ((rc = bring(mem, coarse, 3 * C, "coarse warp", &dc)) || (rc = df.open(mem, fine, 3 * V, "warp"))) return rc;
    k_warp_up<<<stream_grid((int64_t)V), WT>>>(dc, ext_of(c), (int64_t)C, ext_of(n), (int64_t)V, df.dev);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return df.close();
}

extern "C" int vmask_warp_resample(int device, const void* moving, int dtype, int64_t m0, int64_t m1, int64_t m2, const double* T, const double* u, int order,
                                   double fill, void* out, int64_t n0, int64_t n1, int64_t n2) {
    if (!moving || !T || !u || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (order != 0 && order != 1) { vmask::set_error("warp: order 0 (nearest) or 1 (trilinear)"); return VRG_E_ARG; }
    if (!size_of(dtype) || (order == 1 && !is_float(dtype))) { vmask::set_error("warp: order 1 takes float32 or float64, order 0 uint8, int16, int32, float32 or float64"); return VRG_E_ARG; }
    if (order == 0 && !fill_ok(dtype, fill)) { vmask::set_error("warp: fill is not a value of the volume's type"); return VRG_E_ARG; }
    WarpMap M;
    const int64_t n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
    int rc = check_map(T, M);
    if (!rc) rc = check_shapes(device, n, m);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2, W = (size_t)m0 * m1 * m2, width = order == 1 ? 8 : size_of(dtype);
    DevMem mem;
    const uint8_t* dmov = nullptr; const double* du = nullptr;
    Out<uint8_t> dout;
    if ((rc = bring(mem, (const uint8_t*)moving, W * size_of(dtype), "moving volume", &dmov)) || (rc = bring(mem, u, 3 * V, "warp", &du)) ||
        (rc = dout.open(mem, (uint8_t*)out, V * width, "resampled volume"))) return rc;
    const Ext en = ext_of(n), em = ext_of(m);
    if (order == 1) {
        if (dtype == VRG_F32) k_warp_linear<float><<<stream_grid((int64_t)V), WT>>>((const float*)dmov, em, M, du, fill, en, (int64_t)V, (double*)dout.dev);
        else k_warp_linear<double><<<stream_grid((int64_t)V), WT>>>((const double*)dmov, em, M, du, fill, en, (int64_t)V, (double*)dout.dev);
    } else {
        switch (dtype) {
            case VRG_U8: nearest<uint8_t>(dmov, em, M, du, fill, en, (int64_t)V, dout.dev); break;
            case VRG_I16: nearest<int16_t>(dmov, em, M, du, fill, en, (int64_t)V, dout.dev); break;
            case VRG_I32: nearest<int32_t>(dmov, em, M, du, fill, en, (int64_t)V, dout.dev); break;
            case VRG_F32: nearest<float>(dmov, em, M, du, fill, en, (int64_t)V, dout.dev); break;
            default: nearest<double>(dmov, em, M, du, fill, en, (int64_t)V, dout.dev); break;
        }
    }
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return dout.close();
}

extern "C" int vmask_warp_field(int device, const void* fixed, int fdtype, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, const void* moving,
                                int mdtype, int64_t m0, int64_t m1, int64_t m2, const double* T, double flo, double fs, double mlo, double ms,
                                const int* spans, int iterations, double maxStep, double threshold, double* u, double* trace, int64_t* ntrace) {
    if (!fixed || !moving || !T || !spans || !u) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!spans_ok(spans)) { vmask::set_error("warp: 1 to 64 spans per axis"); return VRG_E_ARG; }
    if (iterations < 1 || iterations > 200) { vmask::set_error("warp: 1 to 200 iterations"); return VRG_E_ARG; }
    if (!positive(threshold)) { vmask::set_error("warp: the threshold must be finite and positive"); return VRG_E_ARG; }
    WarpMap M; WarpScale sc;
    const int64_t n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
    int rc = check_force(fdtype, mdtype, T, flo, fs, mlo, ms, maxStep, M, sc);
    if (!rc) rc = check_shapes(device, n, m);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2, W = (size_t)m0 * m1 * m2;
    DevMem mem;
    const uint8_t* dF = nullptr; const uint8_t* dmov = nullptr; const uint8_t* dmask = nullptr;
    const bool u_host = !vmask::is_device_pointer(u);
    double* own_u = nullptr; double* ddelta = nullptr; uint8_t* dpart = nullptr;
    Axes ax; Lattice L; CostMem cm;
    if (bring(mem, (const uint8_t*)fixed, V * size_of(fdtype), "fixed volume", &dF) || (mask && bring(mem, mask, V, "mask", &dmask)) ||
        bring(mem, (const uint8_t*)moving, W * size_of(mdtype), "moving volume", &dmov) || (u_host && mem.grab(&own_u, 3 * V, "warp")) ||
        mem.grab(&ddelta, 3 * V, "forces") || mem.grab(&dpart, V, "participation") || cm.alloc(mem, n) || ax.alloc(mem, n) || L.alloc(mem, n, spans)) {
        vmask::set_error("out of device memory (warp: the two volumes, the mask and the warp where they are host arrays, three float64 force volumes, the participation bytes and 4 (spans_0 + 3) n1 n2 doubles of the fit; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    double* du = u_host ? own_u : u;
    if (u_host) VMASK_TRY(hipMemcpy(own_u, u, 3 * V * 8, hipMemcpyHostToDevice));
    if ((rc = ax.set(n, spans))) return rc;
    const size_t nphi = 3 * (size_t)ax.dev[0].K * ax.dev[1].K * ax.dev[2].K;
    std::vector<double> hphi(nphi);
    int64_t records = 0;
    for (int it = 0; it < iterations; it++) {
        double S; int64_t count;
        if ((rc = run_force(dF, fdtype, dmask, du, n, dmov, mdtype, m, M, sc, ddelta, dpart, cm, &S, &count))) return rc;
        if (it == 0 && count == 0) { vmask::set_error("warp: no voxel takes part (an empty mask, or the moving volume lies elsewhere)"); return VRG_E_ARG; }
        launch_fit(ddelta, dpart, n, ax, L);
        launch_add(n, ax, L, du);
        VMASK_TRY(hipGetLastError());
        VMASK_TRY(hipMemcpy(hphi.data(), L.phi, nphi * 8, hipMemcpyDeviceToHost));
        double top = 0.0;
        for (size_t k = 0; k < nphi; k++) top = std::fmax(top, std::fabs(hphi[k]));
        if (trace) { double* t = trace + 3 * records; t[0] = S / (double)count; t[1] = (double)count; t[2] = top; }
        records++;
        if (top < threshold) break;
    }
    VMASK_TRY(hipDeviceSynchronize());
    if (u_host) VMASK_TRY(hipMemcpy(u, du, 3 * V * 8, hipMemcpyDeviceToHost));
    if (ntrace) *ntrace = records;
    return VRG_OK;
}
