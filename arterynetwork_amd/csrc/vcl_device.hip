// vcl_device.hip - vmask_centrelines of include/vmask.h: one natural cubic smoothing spline (Reinsch) per branch of the branch
// table, the smoothing parameter found per branch by bisection on the weighted residual; position, second derivative, unit
// tangent and curvature at every entry, and the reference's three-point curvature statistic over a resampling of the curve
// ("f20 centreline splines").
//
//   k_cl_check   the table is looked at before anything is written: offsets ascending by at least 2, every voxel inside the
//                volume, no two consecutive entries of a branch the same voxel (equal neighbours in the flat table less those
//                that straddle two branches); the longest branch
//   k_cl_fit     ONE wave per branch (a block is one wave), the branches dealt to the blocks in turn.  The branch's 15 arrays of
//                n doubles - u, 1/h, the three bands of Q'W^-1 Q, the two of R, Q'y, L1, L2 and the three solutions - live in
//                LDS when n <= lds_entries, otherwise in the branch's own stretch of a global work space: the same code runs
//                over either, so every output is the same bits whichever it was.  Parallel over the entries, lane j taking j,
//                j + 64, ..: steps, bands, right-hand sides, Q c, the residual (the ordered sum of vmask.h), the evaluation at
//                the entries and at the samples.  Serial: the prefix sum of u on lane 0; the L D L' recurrence with the forward
//                substitution, then the back substitution, on lanes 0, 1, 2 - one coordinate each, every one of them running the
//                same factorisation in registers.  A trial value of lambda costs one such solve and one residual pass.
// No floating-point atomics; nothing here is contracted into an FMA; division and square root are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vseg_slots.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVE = 64;
constexpr int NARR = 15;                           // doubles of work space per entry
constexpr int64_t LDS_DEFAULT = 256, LDS_MOST = 512;      // entries of a branch kept in LDS: 30 KiB (five waves per CU), at most 60 KiB
constexpr int SEARCH_STEPS = 24;
constexpr u64 NAN_BITS = 0x7ff8000000000000ull;
enum { A_U = 0, A_R, A_A0, A_A1, A_A2, A_R0, A_R1, A_B, A_L1 = A_B + 3, A_L2, A_Z };      // A_Z .. A_Z + 2 = 14
// after the last solve: the fit g in A_B .. A_B + 2, the second derivative in A_L1, A_L2, A_A0, the first in A_A1, A_A2, A_R0
enum { EF_N = 11, BF_N = 5, BI_N = 3 };

struct Vol { uint32_t n1, n2; u64 V; };
struct Par { double h[3]; double end_w, end_v, lam_fixed, lam_lo, lam_hi, rho, step; };

__device__ __forceinline__ void unravel(int64_t idx, const Vol& s, int32_t* c) {
    const uint32_t v = (uint32_t)idx, r = v / s.n2;
    c[2] = (int32_t)(v - r * s.n2); c[0] = (int32_t)(r / s.n1); c[1] = (int32_t)(r - (uint32_t)c[0] * s.n1);
}
__device__ __forceinline__ double canonical(double x) { return x != x ? __longlong_as_double((long long)NAN_BITS) : x; }
__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt((a * a + b * b) + c * c); }

__global__ void __launch_bounds__(TPB) k_cl_check(const int64_t* __restrict__ off, u64 B, const int64_t* __restrict__ vox, u64 total, u64 V, u64* __restrict__ ctr) {
    u64 wrong = 0, same = 0, excused = 0, longest = 0;
    const u64 most = B > total ? B : total;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < most; i += (u64)gridDim.x * TPB) {
        if (i < B) {
            const int64_t a = off[i], b = off[i + 1];
            const bool bad = a < 0 || b - a < 2 || (u64)b > total || (i == 0 && a != 0);
            wrong += bad;
            if (!bad) {
                longest = longest > (u64)(b - a) ? longest : (u64)(b - a);
                if ((u64)b < total && vox[b - 1] == vox[b]) excused++;       // (the last entry of a branch and the first of the next)
            }
        }
        if (i < total) {
            wrong += (u64)vox[i] >= V;
            if (i + 1 < total) same += vox[i] == vox[i + 1];
        }
    }
    wave_add(ctr + c_at(0), wrong); wave_add(ctr + c_at(1), same); wave_add(ctr + c_at(2), excused);
    if (longest) atomicMax(ctr + c_at(3), longest);
}

// the branch as the fit sees it
struct Branch {
    const int64_t* vox;     // its entries
    int64_t n, m;
    double* w;              // NARR arrays of n doubles
    int32_t e0[3];
    __device__ __forceinline__ double* arr(int k) const { return w + (int64_t)k * n; }
};

__device__ __forceinline__ void y_of(const Branch& br, const Vol& s, const Par& p, int64_t i, double* y) {
    int32_t c[3];
    unravel(br.vox[i], s, c);
#pragma unroll
    for (int a = 0; a < 3; a++) y[a] = (double)(c[a] - br.e0[a]) * p.h[a];
}

// One solve at lambda = 1 / mu: c into A_Z; returns F in every lane.  FINAL: g and the second derivative are stored as well.
template <bool FINAL> __device__ double solve(const Branch& br, const Vol& s, const Par& p, double mu, uint32_t lane) {
    const int64_t n = br.n, m = br.m;
    double* const L1 = br.arr(A_L1); double* const L2 = br.arr(A_L2);
    if (lane < 3u) {
        const double* const a0 = br.arr(A_A0); const double* const a1 = br.arr(A_A1); const double* const a2 = br.arr(A_A2);
        const double* const R0 = br.arr(A_R0); const double* const R1 = br.arr(A_R1);
        const double* const rhs = br.arr(A_B + (int)lane);
        double* const z = br.arr(A_Z + (int)lane);
        double Dm1 = 1.0, Dm2 = 1.0, zm1 = 0.0, zm2 = 0.0, l1m1 = 0.0, d1m1 = 0.0, d2m1 = 0.0, d2m2 = 0.0;
        for (int64_t i = 0; i < m; i++) {
            const double d0 = mu * R0[i] + a0[i], d1 = mu * R1[i] + a1[i], d2 = a2[i];
            const double l2 = i >= 2 ? d2m2 / Dm2 : 0.0;
            const double l1 = i >= 1 ? (d1m1 - (l2 * Dm2) * l1m1) / Dm1 : 0.0;
            const double D = (d0 - (l1 * l1) * Dm1) - (l2 * l2) * Dm2;
            const double zz = (rhs[i] - l1 * zm1) - l2 * zm2;
            z[i] = zz / D;
            if (lane == 0u) { L1[i] = l1; L2[i] = l2; }
            Dm2 = Dm1; Dm1 = D; zm2 = zm1; zm1 = zz; l1m1 = l1; d1m1 = d1; d2m2 = d2m1; d2m1 = d2;
        }
    }
    __syncthreads();
    if (lane < 3u) {
        double* const z = br.arr(A_Z + (int)lane);
        double c1 = 0.0, c2 = 0.0;
        for (int64_t i = m - 1; i >= 0; i--) {
            const double l1 = i + 1 < m ? L1[i + 1] : 0.0, l2 = i + 2 < m ? L2[i + 2] : 0.0;
            const double c = (z[i] - l1 * c1) - l2 * c2;
            z[i] = c;
            c2 = c1; c1 = c;
        }
    }
    __syncthreads();
    const double* const r = br.arr(A_R);
    double acc = 0.0;
    for (int64_t i = lane; i < n; i += WAVE) {
        const double rm = i >= 1 ? r[i - 1] : 0.0, ri = i <= n - 2 ? r[i] : 0.0;
        const double v = (i == 0 || i == n - 1) ? p.end_v : 1.0, w = (i == 0 || i == n - 1) ? p.end_w : 1.0;
        double e[3], y[3];
        if (FINAL) y_of(br, s, p, i, y);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double* const c = br.arr(A_Z + a);
            const double cm2 = (i >= 2 && i - 2 < m) ? c[i - 2] : 0.0, cm1 = (i >= 1 && i - 1 < m) ? c[i - 1] : 0.0, ci = i < m ? c[i] : 0.0;
            const double q = rm * (cm2 - cm1) + ri * (ci - cm1);
            e[a] = v * q;
            if (FINAL) {
                br.arr(A_B + a)[i] = y[a] - e[a];
                br.arr(a == 0 ? A_L1 : a == 1 ? A_L2 : A_A0)[i] = (i >= 1 && i <= n - 2) ? mu * cm1 : 0.0;
            }
        }
        acc = acc + w * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
    acc = __shfl(acc, 0, 64);
    __syncthreads();
    return acc;
}

// the cubic at the parameter uk
__device__ __forceinline__ void point(const Branch& br, double uk, double* out) {
    const double* const u = br.arr(A_U);
    int64_t lo = 0, hi = br.n - 2;                                           // the last knot of 0 .. n - 2 with u <= uk
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (u[mid] <= uk) lo = mid; else hi = mid - 1;
    }
    const double t = uk - u[lo], hh = u[lo + 1] - u[lo];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double* const g = br.arr(A_B + a);
        const double* const gam = br.arr(a == 0 ? A_L1 : a == 1 ? A_L2 : A_A0);
        const double* const d = br.arr(a == 0 ? A_A1 : a == 1 ? A_A2 : A_R0);
        const double k3 = (gam[lo + 1] - gam[lo]) / (6.0 * hh);
        out[a] = g[lo] + t * (d[lo] + t * (0.5 * gam[lo] + t * k3));
    }
}

__global__ void __launch_bounds__(WAVE) k_cl_fit(const int64_t* __restrict__ off, u64 B, const int64_t* __restrict__ vox, Vol s, Par p, int64_t lds_n,
                                                 double* __restrict__ gws, double* __restrict__ ef, double* __restrict__ bf, int64_t* __restrict__ bi) {
    extern __shared__ double lds[];
    const uint32_t lane = threadIdx.x;
    for (u64 b = blockIdx.x; b < B; b += gridDim.x) {                        // (the same trips, and the same branches below, in every lane)
        const int64_t a = off[b], n = off[b + 1] - a, m = n - 2;
        Branch br;
        br.vox = vox + a; br.n = n; br.m = m;
        br.w = n <= lds_n ? lds : gws + a * NARR;
        unravel(vox[a], s, br.e0);
        double* const u = br.arr(A_U); double* const r = br.arr(A_R);
        // ---- the parameter
        for (int64_t i = lane; i < n - 1; i += WAVE) {
            double y0[3], y1[3];
            y_of(br, s, p, i, y0); y_of(br, s, p, i + 1, y1);
            r[i] = norm3(y1[0] - y0[0], y1[1] - y0[1], y1[2] - y0[2]);
        }
        __syncthreads();
        if (lane == 0u) {
            double at = 0.0;
            u[0] = 0.0;
            for (int64_t i = 0; i < n - 1; i++) { at = at + r[i]; u[i + 1] = at; }
        }
        __syncthreads();
        for (int64_t i = lane; i < n - 1; i += WAVE) r[i] = 1.0 / (u[i + 1] - u[i]);
        __syncthreads();
        // ---- the bands and the right-hand sides
        for (int64_t j = lane; j < m; j += WAVE) {
            const double r0 = r[j], r1 = r[j + 1], r2 = j < m - 1 ? r[j + 2] : 0.0;
            const double v0 = j == 0 ? p.end_v : 1.0, v1 = 1.0, v2 = j + 2 == n - 1 ? p.end_v : 1.0;
            const double s0 = r0 + r1, s1 = r1 + r2;
            br.arr(A_A0)[j] = ((r0 * r0) * v0 + (s0 * s0) * v1) + (r1 * r1) * v2;
            br.arr(A_A1)[j] = j < m - 1 ? -((s0 * r1) * v1 + (r1 * s1) * v2) : 0.0;
            br.arr(A_A2)[j] = j < m - 2 ? (r1 * r2) * v2 : 0.0;
            const double h0 = u[j + 1] - u[j], h1 = u[j + 2] - u[j + 1];
            br.arr(A_R0)[j] = (h0 + h1) / 3.0;
            br.arr(A_R1)[j] = h1 / 6.0;
            double y0[3], y1[3], y2[3];
            y_of(br, s, p, j, y0); y_of(br, s, p, j + 1, y1); y_of(br, s, p, j + 2, y2);
#pragma unroll
            for (int k = 0; k < 3; k++) br.arr(A_B + k)[j] = (y2[k] - y1[k]) * r1 - (y1[k] - y0[k]) * r0;
        }
        __syncthreads();
        // ---- lambda
        const bool fixed = p.lam_fixed > 0.0;
        const double target = p.rho * (double)n;
        double lam = p.lam_hi;
        int64_t solves = 1, capped = 0;
        bool moved = false;
        if (fixed) lam = p.lam_fixed;
        else if (m == 0) capped = 1;
        else if (solve<false>(br, s, p, 1.0 / p.lam_hi, lane) <= target) capped = 1;
        else {
            double lo = p.lam_lo, hi = p.lam_hi;
            for (int k = 0; k < SEARCH_STEPS; k++) {
                const double mid = sqrt(lo * hi);
                if (solve<false>(br, s, p, 1.0 / mid, lane) > target) hi = mid; else { lo = mid; moved = true; }
            }
            lam = lo; solves = SEARCH_STEPS + 1;
        }
        const double F = solve<true>(br, s, p, 1.0 / lam, lane);             // (m == 0: no unknowns, g = y)
        if (solves > 1 && !moved && F > target) capped = 2;
        // ---- at the entries
        {
            const double* const g[3] = {br.arr(A_B), br.arr(A_B + 1), br.arr(A_B + 2)};
            const double* const gam[3] = {br.arr(A_L1), br.arr(A_L2), br.arr(A_A0)};
            double* const d[3] = {br.arr(A_A1), br.arr(A_A2), br.arr(A_R0)};
            for (int64_t i = lane; i < n; i += WAVE) {
                const int64_t k = i < n - 1 ? i : n - 2;                     // the interval
                const double hh = u[k + 1] - u[k];
                double f1[3], f2[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double slope = (g[c][k + 1] - g[c][k]) / hh;
                    f1[c] = i < n - 1 ? slope - (hh * (2.0 * gam[c][k] + gam[c][k + 1])) / 6.0 : slope + (hh * (gam[c][k] + 2.0 * gam[c][k + 1])) / 6.0;
                    f2[c] = gam[c][i];
                }
                const double len = norm3(f1[0], f1[1], f1[2]);
                const double x0 = f1[1] * f2[2] - f1[2] * f2[1], x1 = f1[2] * f2[0] - f1[0] * f2[2], x2 = f1[0] * f2[1] - f1[1] * f2[0];
                double* const o = ef + (a + i) * EF_N;
                o[0] = u[i];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    o[1 + c] = (double)br.e0[c] * p.h[c] + g[c][i];
                    o[4 + c] = f2[c];
                    o[7 + c] = canonical(f1[c] / len);
                }
                o[10] = canonical(norm3(x0, x1, x2) / ((len * len) * len));
#pragma unroll
                for (int c = 0; c < 3; c++) d[c][i] = f1[c];                 // (arrays that this pass does not read)
            }
        }
        __syncthreads();
        // ---- the samples: chord t = |P_(t+1) - P_t|, triangle t = (P_t, P_(t+1), P_(t+2))
        const double U = u[n - 1];
        int64_t ms = (int64_t)ceil(U / p.step) + 1;
        if (ms < 3) ms = 3;
        double len = 0.0, sum = 0.0, most = 0.0;
        for (int64_t t = lane; t < ms - 1; t += WAVE) {
            double P[3][3];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const int64_t k = t + q;
                if (k < ms) point(br, k < ms - 1 ? ((double)k * U) / (double)(ms - 1) : U, P[q]);
                else P[q][0] = P[q][1] = P[q][2] = 0.0;
            }
            const double ab = norm3(P[0][0] - P[1][0], P[0][1] - P[1][1], P[0][2] - P[1][2]);
            len = len + norm3(P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]);
            if (t < ms - 2) {
                const double ac = norm3(P[0][0] - P[2][0], P[0][1] - P[2][1], P[0][2] - P[2][2]), bc = norm3(P[1][0] - P[2][0], P[1][1] - P[2][1], P[1][2] - P[2][2]);
                const double hi = fmax(ab, fmax(ac, bc)), lo = fmin(ab, fmin(ac, bc));
                const double mid = fmax(fmin(ab, ac), fmin(fmax(ab, ac), bc));
                const double tt = (((hi + (mid + lo)) * (lo - (hi - mid))) * (lo + (hi - mid))) * (hi + (mid - lo));
                const double kappa = (tt > 0.0 ? sqrt(tt) : 0.0) / ((hi * mid) * lo);
                sum = sum + kappa;
                most = fmax(most, kappa);
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            len = len + __shfl_xor(len, o, 64); sum = sum + __shfl_xor(sum, o, 64);
            most = fmax(most, __shfl_xor(most, o, 64));
        }
        if (lane == 0u) {
            double* const o = bf + b * BF_N;
            o[0] = lam; o[1] = F; o[2] = len; o[3] = most; o[4] = canonical(sum / (double)(ms - 2));
            int64_t* const k = bi + b * BI_N;
            k[0] = solves; k[1] = capped; k[2] = ms;
        }
        __syncthreads();                                                     // (the next branch writes the same work space)
    }
}

struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

int centrelines(const int64_t* offsets, int64_t nbranch, const int64_t* voxels, const Vol& s, const Par& p, int64_t lds_n,
                double* entry_f64, double* branch_f64, int64_t* branch_int, double* kernel_ms) {
    const u64 B = (u64)nbranch;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!B) return VRG_OK;
    DevMem mem;
    int rc;
    int64_t edge[2] = {0, 0};
    if (vmask::is_device_pointer(offsets)) {
        VMASK_TRY(hipMemcpy(&edge[0], offsets, sizeof(int64_t), hipMemcpyDeviceToHost));
        VMASK_TRY(hipMemcpy(&edge[1], offsets + B, sizeof(int64_t), hipMemcpyDeviceToHost));
    } else { edge[0] = offsets[0]; edge[1] = offsets[B]; }
    if (edge[0] != 0 || edge[1] < 2 * (int64_t)B || edge[1] > ((int64_t)1 << 40)) { vmask::set_error("offsets do not describe branches of at least two entries"); return VRG_E_ARG; }
    const u64 total = (u64)edge[1];
    const int64_t* off = nullptr; const int64_t* vox = nullptr;
    if ((rc = bring(mem, offsets, B + 1, "offsets", &off)) || (rc = bring(mem, voxels, (size_t)total, "branch voxels", &vox))) return rc;
    u64* ctr = nullptr;
    VMASK_GRAB(ctr, 4 * C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(ctr, 0, 4 * C_PITCH * sizeof(u64), 0));
    Events ev;
    float ms[2] = {0.f, 0.f};
    VMASK_TRY(hipEventCreate(&ev.e[0])); VMASK_TRY(hipEventCreate(&ev.e[1]));
    VMASK_TRY(hipEventRecord(ev.e[0], 0));
    k_cl_check<<<grid_for(total, GRID_LIST), TPB>>>(off, B, vox, total, s.V, ctr);
    VMASK_TRY(hipEventRecord(ev.e[1], 0));
    u64 seen[4 * C_PITCH];
    VMASK_TRY(hipMemcpy(seen, ctr, sizeof(seen), hipMemcpyDeviceToHost));
    VMASK_TRY(hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
    if (seen[c_at(0)]) { vmask::set_error("the branch table does not fit the volume: offsets or voxels out of range"); return VRG_E_ARG; }
    if (seen[c_at(1)] != seen[c_at(2)]) { vmask::set_error("a branch has the same voxel at two consecutive entries (a zero step)"); return VRG_E_ARG; }
    const u64 longest = seen[c_at(3)];

    double* gws = nullptr;
    if (longest > (u64)lds_n) VMASK_GRAB(gws, (size_t)total * NARR, "work space of the long branches");
    Out<double> oef, obf;
    Out<int64_t> obi;
    if ((rc = oef.open(mem, entry_f64, (size_t)total * EF_N, "entry table")) || (rc = obf.open(mem, branch_f64, B * BF_N, "branch table")) ||
        (rc = obi.open(mem, branch_int, B * BI_N, "branch integers"))) return rc;
    const int grid = (int)std::min<u64>(B, 4096);
    VMASK_TRY(hipEventRecord(ev.e[0], 0));
    k_cl_fit<<<grid, WAVE, (size_t)lds_n * NARR * sizeof(double)>>>(off, B, vox, s, p, lds_n, gws, oef.dev, obf.dev, obi.dev);
    VMASK_TRY(hipEventRecord(ev.e[1], 0));
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    VMASK_TRY(hipEventElapsedTime(&ms[1], ev.e[0], ev.e[1]));
    if ((rc = oef.close()) || (rc = obf.close()) || (rc = obi.close())) return rc;
    if (kernel_ms) *kernel_ms = (double)ms[0] + (double)ms[1];
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_centrelines(int device, int64_t n0, int64_t n1, int64_t n2, const int64_t* offsets, int64_t nbranch, const int64_t* voxels,
                                 const double* spacing, double end_weight, double smoothing, double residual_per_point, double sample_step,
                                 int64_t lds_entries, double* entry_f64, double* branch_f64, int64_t* branch_int, double* kernel_ms) {
    if (nbranch < 0 || nbranch >= ((int64_t)1 << 31)) { vmask::set_error("negative or oversized count"); return VRG_E_ARG; }
    if (nbranch && (!offsets || !voxels || !entry_f64 || !branch_f64 || !branch_int)) { vmask::set_error("null pointer (branch tables)"); return VRG_E_ARG; }
    if (lds_entries < 0 || lds_entries > LDS_MOST) { vmask::set_error("lds_entries outside [0, 512]"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Par p;
    p.h[0] = p.h[1] = p.h[2] = 1.0;
    if (spacing) {
        if (vmask::is_device_pointer(spacing)) VMASK_TRY(hipMemcpy(p.h, spacing, sizeof(p.h), hipMemcpyDeviceToHost));
        else std::copy(spacing, spacing + 3, p.h);
    }
    for (double x : p.h)
        if (!std::isfinite(x) || !(x > 0.0)) { vmask::set_error("spacing not finite and positive"); return VRG_E_ARG; }
    if (std::max({p.h[0], p.h[1], p.h[2]}) / std::min({p.h[0], p.h[1], p.h[2]}) > 1000.0) { vmask::set_error("spacing ratio above 1000"); return VRG_E_ARG; }
    const double l2 = ((p.h[0] * p.h[0] + p.h[1] * p.h[1]) + p.h[2] * p.h[2]) / 3.0, l = std::sqrt(l2), l3 = l2 * l;
    p.lam_lo = l3 * 0x1p-24; p.lam_hi = l3 * 0x1p24;
    if (!std::isfinite(end_weight) || !(end_weight > 0.0)) { vmask::set_error("end_weight not finite and positive"); return VRG_E_ARG; }
    if (smoothing != smoothing || (smoothing > 0.0 && (smoothing < p.lam_lo || smoothing > p.lam_hi))) { vmask::set_error("smoothing (lambda) outside [2^-24, 2^24] l^3"); return VRG_E_ARG; }
    if (!(smoothing > 0.0) && (!std::isfinite(residual_per_point) || !(residual_per_point > 0.0))) { vmask::set_error("residual_per_point not finite and positive"); return VRG_E_ARG; }
    if (!std::isfinite(sample_step) || !(sample_step >= l * 0x1p-10)) { vmask::set_error("sample_step not finite or below 2^-10 l"); return VRG_E_ARG; }
    p.end_w = end_weight; p.end_v = 1.0 / end_weight;
    p.lam_fixed = smoothing > 0.0 ? smoothing : 0.0;
    p.rho = residual_per_point; p.step = sample_step;
    const Vol s{(uint32_t)n1, (uint32_t)n2, (u64)n0 * (u64)n1 * (u64)n2};
    return centrelines(offsets, nbranch, voxels, s, p, lds_entries ? lds_entries : LDS_DEFAULT, entry_f64, branch_f64, branch_int, kernel_ms);
}
