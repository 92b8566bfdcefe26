// vreg_device.hip - vmask_reg_* of include/vmask.h: what a rigid / affine registration of two volumes evaluates on the device
// (entry f16).  The search itself is host Python (registration.py); one cost evaluation is one launch here.
//
//   k_reg_hist<T>  the joint histogram.  A workgroup takes RG = 256 consecutive voxels of the flattened fixed grid per trip, so
//                  lanes run along axis 2: the 1-byte bin reads coalesce and neighbouring lanes' eight gathers share cache lines;
//                  grid-stride over at most RGRID workgroups, the voxel's (i, j, k) advanced by the split stride.  The 12 doubles of
//                  the voxel map, mlo and ms are kernel arguments (scalar registers).  Counts are 32-bit in LDS (4 B^2 bytes,
//                  dynamic), one atomic per counted voxel, and are added once per workgroup to the 64-bit counts in memory.
//                  Integer counts: the result does not depend on the order.  (One LDS atomic per wave for the lanes that share
//                  a slot was measured against this and gave nothing: the kernel is bound by its arithmetic)
//   k_reg_minmax<T>, k_reg_quantise<T>  per-workgroup extrema (reduced on the host) and the fixed volume's bin image.
//   k_reg_shrink<T>  one level of the pyramid: the block mean in float64, or the block "any" of a uint8 mask.
//   k_reg_linear<T>, k_reg_nearest<T>  the resampled volume on the fixed grid.
// float64 throughout, nothing contracted; the only atomics are integer ones.  No scratch.
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

constexpr int RT = 256;                            // every kernel: 4 waves
constexpr int RG = 256;                            // k_reg_hist: the fixed voxels that a workgroup takes per grid-stride trip
constexpr int RGRID = 1024;                        // the grid-stride passes: at most this many workgroups
constexpr int MINB = 8, MAXB = 128;
static_assert(RG == RT, "a thread takes one voxel per trip");

struct RegMap { double t[12]; };                   // the first three rows of T: fixed voxel -> moving voxel
__device__ __forceinline__ double coord(const RegMap& M, int a, int i, int j, int k) {
    return ((M.t[4 * a] * (double)i + M.t[4 * a + 1] * (double)j) + M.t[4 * a + 2] * (double)k) + M.t[4 * a + 3];
}

// the trilinear sample at fixed voxel (i, j, k): false where the voxel is outside or the sample is not finite
template <class T>
__device__ __forceinline__ bool sample(const T* __restrict__ mov, const Ext m, const RegMap& M, int i, int j, int k, double& value) {
    const double p0 = coord(M, 0, i, j, k), p1 = coord(M, 1, i, j, k), p2 = coord(M, 2, i, j, k);
    const bool inside = p0 >= 0.0 && p0 <= (double)(m.n0 - 1) && p1 >= 0.0 && p1 <= (double)(m.n1 - 1) && p2 >= 0.0 && p2 <= (double)(m.n2 - 1);
    if (!inside) return false;                     // (a NaN fails every comparison)
    const double f0 = floor(p0), f1 = floor(p1), f2 = floor(p2);
    const double t0 = p0 - f0, t1 = p1 - f1, t2 = p2 - f2;
    const int a0 = (int)f0, b0 = (int)f1, c0 = (int)f2;                            // 0 .. m - 1
    const int a1 = min(a0 + 1, m.n0 - 1), b1 = min(b0 + 1, m.n1 - 1), c1 = min(c0 + 1, m.n2 - 1);
    const int64_t r00 = ((int64_t)a0 * m.n1 + b0) * m.n2, r01 = ((int64_t)a0 * m.n1 + b1) * m.n2;
    const int64_t r10 = ((int64_t)a1 * m.n1 + b0) * m.n2, r11 = ((int64_t)a1 * m.n1 + b1) * m.n2;
    const double v000 = (double)mov[r00 + c0], v001 = (double)mov[r00 + c1], v010 = (double)mov[r01 + c0], v011 = (double)mov[r01 + c1];
    const double v100 = (double)mov[r10 + c0], v101 = (double)mov[r10 + c1], v110 = (double)mov[r11 + c0], v111 = (double)mov[r11 + c1];
    const double x00 = v000 + t2 * (v001 - v000), x01 = v010 + t2 * (v011 - v010);
    const double x10 = v100 + t2 * (v101 - v100), x11 = v110 + t2 * (v111 - v110);
    const double y0 = x00 + t1 * (x01 - x00), y1 = x10 + t1 * (x11 - x10);
    value = y0 + t0 * (y1 - y0);
    return isfinite(value);
}

// clamp(floor((v - lo) * s), 0, B - 1), clamped as a double (a NaN lands in bin 0)
__device__ __forceinline__ int bin_of(double v, double lo, double s, int B) {
    double q = floor((v - lo) * s);
    q = !(q > 0.0) ? 0.0 : (q > (double)(B - 1) ? (double)(B - 1) : q);
    return (int)q;
}

template <class T>
__global__ void __launch_bounds__(RT) k_reg_hist(const uint8_t* __restrict__ fb, Ext n, int64_t V, const T* __restrict__ mov, Ext m, RegMap M,
                                                 int B, double mlo, double ms, unsigned long long* __restrict__ H) {
    extern __shared__ unsigned int counts[];       // [B][B]; a workgroup sees fewer than 2^32 voxels
    const int slots = B * B;
    for (int s = threadIdx.x; s < slots; s += RT) counts[s] = 0;
    __syncthreads();
    // the voxel's index is split once and then advanced by the split stride: no division per voxel
    const int64_t stride = (int64_t)gridDim.x * RG;
    int i, j, k, di, dj, dk;
    split(stride, n, di, dj, dk);                  // (dj < n1, dk < n2: at most one carry per axis, vreg_walk.h)
    int64_t v = (int64_t)blockIdx.x * RG + threadIdx.x;
    split(v, n, i, j, k);
    for (; v < V; v += stride) {
        const int bf = fb[v];
        if (bf < B) {                              // (255, and any other value that is no bin, does not count)
            double value;
            if (sample<T>(mov, m, M, i, j, k, value)) atomicAdd(&counts[bf * B + bin_of(value, mlo, ms, B)], 1u);
        }
        advance_split(n, di, dj, dk, i, j, k);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < slots; s += RT)
        if (counts[s]) atomicAdd(&H[s], (unsigned long long)counts[s]);
}

// per workgroup the exact min and max of the finite voxels (of the mask, where one is given): part[2 g], part[2 g + 1]
template <class T>
__global__ void __launch_bounds__(RT) k_reg_minmax(const T* __restrict__ I, const uint8_t* __restrict__ mask, int64_t V, double* __restrict__ part) {
    __shared__ double lo_s[RT], hi_s[RT];
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < V; i += (int64_t)gridDim.x * RT) {
        const double x = (double)I[i];
        if (isfinite(x) && (!mask || mask[i])) { lo = fmin(lo, x); hi = fmax(hi, x); }
    }
    lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi;
    __syncthreads();
    for (int k = RT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            lo_s[threadIdx.x] = fmin(lo_s[threadIdx.x], lo_s[threadIdx.x + k]);
            hi_s[threadIdx.x] = fmax(hi_s[threadIdx.x], hi_s[threadIdx.x + k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = lo_s[0]; part[2 * blockIdx.x + 1] = hi_s[0]; }
}

template <class T>
__global__ void __launch_bounds__(RT) k_reg_quantise(const T* __restrict__ I, const uint8_t* __restrict__ mask, int64_t V, int B, double lo, double s,
                                                     uint8_t* __restrict__ bins, unsigned long long* total) {
    __shared__ unsigned int part[RT];
    unsigned int mine = 0;                         // (a thread sees fewer than 2^32 voxels)
    for (int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x; i < V; i += (int64_t)gridDim.x * RT) {
        const double x = (double)I[i];
        const bool in = isfinite(x) && (!mask || mask[i]);
        bins[i] = in ? (uint8_t)bin_of(x, lo, s, B) : (uint8_t)255;
        mine += in ? 1u : 0u;
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int k = RT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) part[threadIdx.x] += part[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(total, (unsigned long long)part[0]);
}

// out[i] = 0.125 * sum over the 2 x 2 x 2 block at 2 i, indices clamped, d2 fastest, from +0.0; a uint8 mask: any non-zero
template <class T>
__global__ void __launch_bounds__(RT) k_reg_shrink(const T* __restrict__ in, Ext n, Ext o, int64_t total, void* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x; v < total; v += (int64_t)gridDim.x * RT) {
        int i, j, k;
        split(v, o, i, j, k);
        double acc = 0.0;
        unsigned any = 0;
        for (int d0 = 0; d0 < 2; d0++)
            for (int d1 = 0; d1 < 2; d1++)
                for (int d2 = 0; d2 < 2; d2++) {
                    const int a = min(2 * i + d0, n.n0 - 1), b = min(2 * j + d1, n.n1 - 1), c = min(2 * k + d2, n.n2 - 1);
                    const T x = in[((int64_t)a * n.n1 + b) * n.n2 + c];
                    if constexpr (sizeof(T) == 1) any |= (unsigned)x;
                    else acc = acc + (double)x;
                }
        if constexpr (sizeof(T) == 1) ((uint8_t*)out)[v] = any ? 1 : 0;
        else ((double*)out)[v] = 0.125 * acc;
    }
}

template <class T>
__global__ void __launch_bounds__(RT) k_reg_linear(const T* __restrict__ mov, Ext m, RegMap M, double fill, Ext n, int64_t V, double* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x; v < V; v += (int64_t)gridDim.x * RT) {
        int i, j, k;
        split(v, n, i, j, k);
        double value;
        out[v] = sample<T>(mov, m, M, i, j, k, value) ? value : fill;
    }
}

template <class T>
__global__ void __launch_bounds__(RT) k_reg_nearest(const T* __restrict__ mov, Ext m, RegMap M, T fill, Ext n, int64_t V, T* __restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * RT + threadIdx.x; v < V; v += (int64_t)gridDim.x * RT) {
        int i, j, k;
        split(v, n, i, j, k);
        const double q0 = floor(coord(M, 0, i, j, k) + 0.5), q1 = floor(coord(M, 1, i, j, k) + 0.5), q2 = floor(coord(M, 2, i, j, k) + 0.5);
        const bool inside = q0 >= 0.0 && q0 <= (double)(m.n0 - 1) && q1 >= 0.0 && q1 <= (double)(m.n1 - 1) && q2 >= 0.0 && q2 <= (double)(m.n2 - 1);
        out[v] = inside ? mov[((int64_t)(int)q0 * m.n1 + (int)q1) * m.n2 + (int)q2] : fill;
    }
}

// ---------------------------------------------------------------- host
int stream_grid(int64_t V, int per) { return (int)std::min<int64_t>((V + per - 1) / per, RGRID); }

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

int check_map(const double* T, RegMap& M) {
    for (int k = 0; k < 12; k++) {
        if (!std::isfinite(T[k])) { vmask::set_error("registration: the voxel map must be finite"); return VRG_E_ARG; }
        M.t[k] = T[k];
    }
    return VRG_OK;
}

int check_bins(int B) {
    if (B < MINB || B > MAXB) { vmask::set_error("registration: 8 to 128 bins"); return VRG_E_ARG; }
    return VRG_OK;
}

// both shapes inside the envelope of the other passes, the device made current
int check_shapes(int device, const int64_t* n, const int64_t* m) {
    if (!vmask::shape_in_envelope(m[0], m[1], m[2])) { vmask::set_error("shape of the moving volume out of range"); return VRG_E_ARG; }
    return vmask::check_args(device, n[0], n[1], n[2]);
}

Ext ext_of(const int64_t* n) { return Ext{(int)n[0], (int)n[1], (int)n[2]}; }

int joint_hist(int device, const uint8_t* fixedBins, const int64_t* n, const void* moving, int dtype, const int64_t* m, const double* T, int B,
               double mlo, double ms, uint64_t* H) {
    if (!fixedBins || !moving || !T || !H) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!is_float(dtype)) { vmask::set_error("registration: the moving volume must be float32 or float64"); return VRG_E_ARG; }
    if (!std::isfinite(mlo) || !std::isfinite(ms)) { vmask::set_error("registration: the moving volume's bin origin and scale must be finite"); return VRG_E_ARG; }
    RegMap M;
    int rc = check_bins(B);
    if (!rc) rc = check_map(T, M);
    if (!rc) rc = check_shapes(device, n, m);
    if (rc) return rc;
    const size_t V = (size_t)n[0] * n[1] * n[2], W = (size_t)m[0] * m[1] * m[2];
    DevMem mem;
    const uint8_t* dfb = nullptr; const uint8_t* dmov = nullptr;
    Out<unsigned long long> dH;
    if ((rc = bring(mem, fixedBins, V, "fixed bins", &dfb)) || (rc = bring(mem, (const uint8_t*)moving, W * size_of(dtype), "moving volume", &dmov)) ||
        (rc = dH.open(mem, (unsigned long long*)H, (size_t)B * B, "joint histogram"))) return rc;
    VMASK_TRY(hipMemset(dH.dev, 0, (size_t)B * B * sizeof(unsigned long long)));
    const int g = stream_grid((int64_t)V, RG);
    const size_t lds = (size_t)B * B * sizeof(unsigned int);
    if (dtype == VRG_F32) k_reg_hist<float><<<g, RT, lds>>>(dfb, ext_of(n), (int64_t)V, (const float*)dmov, ext_of(m), M, B, mlo, ms, dH.dev);
    else k_reg_hist<double><<<g, RT, lds>>>(dfb, ext_of(n), (int64_t)V, (const double*)dmov, ext_of(m), M, B, mlo, ms, dH.dev);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return dH.close();
}

template <class T> int extrema(const T* dI, const uint8_t* dmask, int64_t V, DevMem& mem, double* lohi) {
    const int g = stream_grid(V, RT);
    double* part = nullptr;
    VMASK_GRAB(part, 2 * (size_t)g, "partial extrema");
    k_reg_minmax<T><<<g, RT>>>(dI, dmask, V, part);
    VMASK_TRY(hipGetLastError());
    std::vector<double> h(2 * (size_t)g);
    VMASK_TRY(hipMemcpy(h.data(), part, h.size() * 8, hipMemcpyDeviceToHost));
    double lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < g; k++) { lo = std::fmin(lo, h[2 * k]); hi = std::fmax(hi, h[2 * k + 1]); }
    lohi[0] = lo; lohi[1] = hi;
    return VRG_OK;
}

template <class T> bool fill_fits(double fill) {
    if (std::is_floating_point<T>::value) return true;
    return std::isfinite(fill) && std::floor(fill) == fill && fill >= (double)std::numeric_limits<T>::lowest() && fill <= (double)std::numeric_limits<T>::max();
}

bool fill_ok(int dtype, double fill) {
    return dtype == VRG_U8 ? fill_fits<uint8_t>(fill) : dtype == VRG_I16 ? fill_fits<int16_t>(fill) : dtype == VRG_I32 ? fill_fits<int32_t>(fill) : true;
}

template <class T> int nearest(const void* dmov, Ext m, const RegMap& M, double fill, Ext n, int64_t V, void* dout) {
    k_reg_nearest<T><<<stream_grid(V, RT), RT>>>((const T*)dmov, m, M, (T)fill, n, V, (T*)dout);
    return VRG_OK;
}

double entropy(const std::vector<uint64_t>& c, double N) {
    double e = 0.0;
    for (uint64_t x : c)
        if (x) { const double p = (double)x / N; e = e + p * std::log(p); }
    return -e;
}

}  // namespace

extern "C" int vmask_reg_minmax(int device, const void* volume, int dtype, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, double* lohi) {
    if (!volume || !lohi) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!is_float(dtype)) { vmask::set_error("registration: the volume must be float32 or float64"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const uint8_t* dI = nullptr; const uint8_t* dmask = nullptr;
    if ((rc = bring(mem, (const uint8_t*)volume, V * size_of(dtype), "volume", &dI)) || (mask && (rc = bring(mem, mask, V, "mask", &dmask)))) return rc;
    double out[2];
    rc = dtype == VRG_F32 ? extrema<float>((const float*)dI, dmask, (int64_t)V, mem, out) : extrema<double>((const double*)dI, dmask, (int64_t)V, mem, out);
    if (rc) return rc;
    lohi[0] = out[0]; lohi[1] = out[1];
    return VRG_OK;
}

extern "C" int vmask_reg_quantise(int device, const void* volume, int dtype, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, int B, double lo,
                                  double s, uint8_t* bins, int64_t* inside) {
    if (!volume || !bins) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!is_float(dtype)) { vmask::set_error("registration: the volume must be float32 or float64"); return VRG_E_ARG; }
    if (!std::isfinite(lo) || !std::isfinite(s) || s < 0.0) { vmask::set_error("registration: the bin origin must be finite, the scale finite and not negative"); return VRG_E_ARG; }
    int rc = check_bins(B);
    if (!rc) rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const uint8_t* dI = nullptr; const uint8_t* dmask = nullptr;
    Out<uint8_t> dbins;
    unsigned long long* total = nullptr;
    if ((rc = bring(mem, (const uint8_t*)volume, V * size_of(dtype), "volume", &dI)) || (mask && (rc = bring(mem, mask, V, "mask", &dmask))) ||
        (rc = dbins.open(mem, bins, V, "bin image")) || (rc = mem.grab(&total, 1, "counter"))) return rc;
    VMASK_TRY(hipMemset(total, 0, sizeof(unsigned long long)));
    const int g = stream_grid((int64_t)V, RT);
    if (dtype == VRG_F32) k_reg_quantise<float><<<g, RT>>>((const float*)dI, dmask, (int64_t)V, B, lo, s, dbins.dev, total);
    else k_reg_quantise<double><<<g, RT>>>((const double*)dI, dmask, (int64_t)V, B, lo, s, dbins.dev, total);
    VMASK_TRY(hipGetLastError());
    unsigned long long count = 0;
    VMASK_TRY(hipMemcpy(&count, total, sizeof count, hipMemcpyDeviceToHost));
    if (inside) *inside = (int64_t)count;
    return dbins.close();
}

extern "C" int vmask_reg_joint_hist(int device, const uint8_t* fixedBins, int64_t n0, int64_t n1, int64_t n2, const void* moving, int dtype,
                                    int64_t m0, int64_t m1, int64_t m2, const double* T, int B, double mlo, double ms, uint64_t* H) {
    const int64_t n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
    return joint_hist(device, fixedBins, n, moving, dtype, m, T, B, mlo, ms, H);
}

extern "C" int vmask_reg_cost(const uint64_t* H, int B, int kind, double minOverlap, int64_t nmask, double* cost) {
    if (!H || !cost) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (check_bins(B)) return VRG_E_ARG;
    if (kind < 0 || kind > 2) { vmask::set_error("registration: cost 0 (corratio), 1 (mi) or 2 (nmi)"); return VRG_E_ARG; }
    if (!(minOverlap >= 0.0 && minOverlap <= 1.0) || nmask < 0) { vmask::set_error("registration: minOverlap in [0, 1] and a mask count that is not negative"); return VRG_E_ARG; }
    std::vector<uint64_t> rows(B, 0), cols(B, 0), all((size_t)B * B);
    uint64_t N = 0;
    for (int r = 0; r < B; r++)
        for (int c = 0; c < B; c++) { const uint64_t x = H[(size_t)r * B + c]; all[(size_t)r * B + c] = x; rows[r] += x; cols[c] += x; N += x; }
    if (N == 0 || (double)N < minOverlap * (double)nmask) { *cost = INFINITY; return VRG_OK; }
    if (kind == 0) {
        int64_t n = 0, S = 0, Q = 0;
        double within = 0.0;
        for (int r = 0; r < B; r++) {
            int64_t nr = 0, Sr = 0, Qr = 0;
            for (int y = 0; y < B; y++) { const int64_t x = (int64_t)H[(size_t)r * B + y]; nr += x; Sr += (int64_t)y * x; Qr += (int64_t)y * y * x; }
            n += nr; S += Sr; Q += Qr;
            if (nr) { const double a = (double)Sr; within = within + ((double)Qr - (a * a) / (double)nr); }
        }
        const double a = (double)S;
        const double total = (double)Q - (a * a) / (double)n;
        *cost = total > 0.0 ? within / total : 0.0;
        return VRG_OK;
    }
    const double HF = entropy(rows, (double)N), HM = entropy(cols, (double)N), HFM = entropy(all, (double)N);
    if (kind == 1) *cost = -((HF + HM) - HFM);
    else *cost = HFM > 0.0 ? -((HF + HM) / HFM) : 0.0;
    return VRG_OK;
}

extern "C" int vmask_reg_shrink(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, void* out) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!is_float(dtype) && dtype != VRG_U8) { vmask::set_error("registration: a float32 or float64 volume, or a uint8 mask"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const int64_t n[3] = {n0, n1, n2}, o[3] = {(n0 + 1) / 2, (n1 + 1) / 2, (n2 + 1) / 2};
    const size_t V = (size_t)n0 * n1 * n2, O = (size_t)o[0] * o[1] * o[2];
    DevMem mem;
    const uint8_t* dI = nullptr;
    Out<uint8_t> dout;
    if ((rc = bring(mem, (const uint8_t*)volume, V * size_of(dtype), "volume", &dI)) || (rc = dout.open(mem, (uint8_t*)out, O * (dtype == VRG_U8 ? 1 : 8), "shrunk volume"))) return rc;
    const int g = stream_grid((int64_t)O, RT);
    if (dtype == VRG_U8) k_reg_shrink<uint8_t><<<g, RT>>>(dI, ext_of(n), ext_of(o), (int64_t)O, dout.dev);
    else if (dtype == VRG_F32) k_reg_shrink<float><<<g, RT>>>((const float*)dI, ext_of(n), ext_of(o), (int64_t)O, dout.dev);
    else k_reg_shrink<double><<<g, RT>>>((const double*)dI, ext_of(n), ext_of(o), (int64_t)O, dout.dev);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return dout.close();
}

extern "C" int vmask_reg_resample(int device, const void* moving, int dtype, int64_t m0, int64_t m1, int64_t m2, const double* T, int order, double fill,
                                  void* out, int64_t n0, int64_t n1, int64_t n2) {
    if (!moving || !T || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (order != 0 && order != 1) { vmask::set_error("registration: order 0 (nearest) or 1 (trilinear)"); return VRG_E_ARG; }
    if (!size_of(dtype) || (order == 1 && !is_float(dtype))) { vmask::set_error("registration: order 1 takes float32 or float64, order 0 uint8, int16, int32, float32 or float64"); return VRG_E_ARG; }
    if (order == 0 && !fill_ok(dtype, fill)) { vmask::set_error("registration: fill is not a value of the volume's type"); return VRG_E_ARG; }
    RegMap M;
    const int64_t n[3] = {n0, n1, n2}, m[3] = {m0, m1, m2};
    int rc = check_map(T, M);
    if (!rc) rc = check_shapes(device, n, m);
    if (rc) return rc;
    const size_t V = (size_t)n0 * n1 * n2, W = (size_t)m0 * m1 * m2, width = order == 1 ? 8 : size_of(dtype);
    DevMem mem;
    const uint8_t* dmov = nullptr;
    Out<uint8_t> dout;
    if ((rc = bring(mem, (const uint8_t*)moving, W * size_of(dtype), "moving volume", &dmov)) || (rc = dout.open(mem, (uint8_t*)out, V * width, "resampled volume"))) return rc;
    const Ext en = ext_of(n), em = ext_of(m);
    const int g = stream_grid((int64_t)V, RT);
    if (order == 1) {
        if (dtype == VRG_F32) k_reg_linear<float><<<g, RT>>>((const float*)dmov, em, M, fill, en, (int64_t)V, (double*)dout.dev);
        else k_reg_linear<double><<<g, RT>>>((const double*)dmov, em, M, fill, en, (int64_t)V, (double*)dout.dev);
    } else {
        switch (dtype) {
            case VRG_U8: rc = nearest<uint8_t>(dmov, em, M, fill, en, (int64_t)V, dout.dev); break;
            case VRG_I16: rc = nearest<int16_t>(dmov, em, M, fill, en, (int64_t)V, dout.dev); break;
            case VRG_I32: rc = nearest<int32_t>(dmov, em, M, fill, en, (int64_t)V, dout.dev); break;
            case VRG_F32: rc = nearest<float>(dmov, em, M, fill, en, (int64_t)V, dout.dev); break;
            default: rc = nearest<double>(dmov, em, M, fill, en, (int64_t)V, dout.dev); break;
        }
        if (rc) return rc;
    }
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return dout.close();
}

extern "C" int vmask_reg_hold(int device, const void* host, int64_t bytes, void** held) {
    if (!held) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (bytes < 1) { vmask::set_error("registration: a held array has at least one byte"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, 1, 1, 1);
    if (rc) return rc;
    DevMem mem;
    uint8_t* p = nullptr;
    VMASK_GRAB(p, (size_t)bytes, "held array");
    if (host) VMASK_TRY(hipMemcpy(p, host, (size_t)bytes, hipMemcpyHostToDevice));
    mem.owned.clear();                             // handed to the caller, who gives it back to vmask_reg_release
    *held = p;
    return VRG_OK;
}

extern "C" int vmask_reg_fetch(const void* held, void* host, int64_t bytes) {
    if (!held || !host) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (bytes < 1) { vmask::set_error("registration: a held array has at least one byte"); return VRG_E_ARG; }
    VMASK_TRY(hipMemcpy(host, held, (size_t)bytes, hipMemcpyDeviceToHost));
    return VRG_OK;
}

extern "C" void vmask_reg_release(void* held) {
    DevMem mem;
    if (held) mem.owned.push_back(held);           // freed as the owner leaves scope
}
