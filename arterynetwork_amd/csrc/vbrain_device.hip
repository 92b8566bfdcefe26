// vbrain_device.hip - vmask_brain_* / vmask_binary_morph / vmask_largest_component / vmask_fill_holes of include/vmask.h: the
// skull stripping in front of every voxel stage, which the reference pipeline leaves to an external GUI tool (DESIGN.md
// section 9, entry f17).  A definition of our own: histogram floor, Laplacian-of-Gaussian edges, opening around the main
// component, closing, hole filling.
//
//   k_brain_minmax<T>, k_brain_hist<T>   per-workgroup extrema and a count of non-finite voxels (reduced on the host), then the 256
//                  counts: 32-bit integer atomics on LDS counters, added once per workgroup to the 64-bit counts in memory.
//   k_brain_axis2<T>   phi and phi'' along axis 2.  A workgroup owns BX2 = 256 consecutive voxels of one row; the segment and its
//                  halo sit in LDS as float64, indices clamped when loaded.
//   k_brain_axis1      phi.phi, phi''.phi and phi.phi'' along axis 1.  Lanes run along axis 2 (BLX = 64); a thread owns BY = 8
//                  consecutive rows of one column, walks the BY + 2 r input rows once and adds each to the outputs it belongs to.
//   k_brain_axis0<T, MODE>   the same along axis 0 (BZ = 8 planes per thread, 4 rows per workgroup), then
//                  E = (c0 T0 + c1 T1) + c2 T2.  MODE 0 writes E; MODE 1 writes only the candidate bits, one __ballot word per
//                  64 consecutive voxels of a row.
//                  In all three the sum of an output runs over the taps k = -r .. r ascending, from +0.0, one multiplication
//                  and one addition per tap, the sample at clamp(i - k): tests/brain_model.py restates it.
//   k_bits_pack, k_bits_unpack, k_bits_count   bytes <-> bits (64 voxels of a row along axis 2 per word, rows padded to whole
//                  words, padding bits always 0), and the number of set bits.
//   k_bits_morph<ERODE>   one step of the 6-neighbour cross on the packed volume, one word per thread: the word, its two
//                  shifted selves with carries from the neighbouring words of the row, the same word of rows i1 +- 1 and of
//                  planes i0 +- 1.  The border rule is applied here, never stored.
//   k_brain_sizes  component sizes, wave-aggregated: the lanes of a wave that share a component add their number once, and a wave
//                  carries the counts of the last two components it met from trip to trip.  (One component holds nearly every
//                  voxel here: one atomic per voxel on one counter would execute one after another at the memory side.)
//   k_brain_winner, k_brain_select   the largest component - one 64-bit atomicMax of size << 32 | (2^32 - 1 - rank) per wave -
//                  and its voxels as bits.
//   k_fill_faces, k_fill_apply   hole filling: the components of the complement that own a voxel on a face are flagged (plain
//                  stores of 1), every other complement voxel is added.
// float64 throughout, nothing contracted; the only atomics are integer ones.  No scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_cc.h"
#include "vmask_common.h"
#include "vmask_host.h"

#pragma clang fp contract(off)

namespace {

using vmask::CcRank;
using vmask::cc_rank;
typedef unsigned long long u64;

constexpr int BT = 256;                            // every kernel: 4 waves
constexpr int BGRID = 1024;                        // the grid-stride passes over the float volumes: at most this many workgroups
constexpr int BMAXR = 64, BTAPS = 2 * BMAXR + 1;   // tap radius 1 .. 64, as vmask_vesselness
constexpr int BX2 = 256;                           // k_brain_axis2: the voxels of a row that a workgroup owns
constexpr int BLX = 64;                            // k_brain_axis1 / axis0: a wave's voxels along axis 2 (one word of the bit volume)
constexpr int BY = 8;                              // k_brain_axis1: consecutive rows of a thread (a workgroup: 4 * BY rows)
constexpr int BZ = 8;                              // k_brain_axis0: consecutive planes of a thread (a workgroup: 4 rows)
constexpr int NBIN = 256;

struct Geo {
    int n0, n1, n2, W;                             // W: words per row
    __host__ __device__ size_t V() const { return (size_t)n0 * n1 * n2; }
    __host__ __device__ size_t rows() const { return (size_t)n0 * n1; }
    __host__ __device__ size_t words() const { return (size_t)n0 * n1 * W; }
};
Geo geo(int64_t n0, int64_t n1, int64_t n2) { return Geo{(int)n0, (int)n1, (int)n2, (int)((n2 + 63) / 64)}; }

int grid_for(uint64_t n) { return (int)std::max<uint64_t>(1, std::min<uint64_t>(65535u * 16u, (n + BT - 1) / BT)); }
// n workgroups as an x-y grid
dim3 grid_xy(uint64_t n, unsigned z = 1) {
    const uint64_t gx = std::max<uint64_t>(1, std::min<uint64_t>(n, 32768));
    return dim3((unsigned)gx, (unsigned)std::max<uint64_t>(1, (n + gx - 1) / gx), z);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------- histogram
// part[3 g], part[3 g + 1]: the exact min and max of the workgroup's finite voxels; part[3 g + 2]: its number of non-finite ones
template <class T>
__global__ void __launch_bounds__(BT) k_brain_minmax(const T* __restrict__ I, int64_t V, double* __restrict__ part) {
    __shared__ double lo_s[BT], hi_s[BT], bad_s[BT];
    double lo = INFINITY, hi = -INFINITY, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) {
        const double x = (double)I[i];
        if (isfinite(x)) { lo = fmin(lo, x); hi = fmax(hi, x); }
        else bad = bad + 1.0;                      // (a count below 2^31: exact)
    }
    lo_s[threadIdx.x] = lo; hi_s[threadIdx.x] = hi; bad_s[threadIdx.x] = bad;
    __syncthreads();
    for (int k = BT / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            lo_s[threadIdx.x] = fmin(lo_s[threadIdx.x], lo_s[threadIdx.x + k]);
            hi_s[threadIdx.x] = fmax(hi_s[threadIdx.x], hi_s[threadIdx.x + k]);
            bad_s[threadIdx.x] = bad_s[threadIdx.x] + bad_s[threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = lo_s[0]; part[3 * blockIdx.x + 1] = hi_s[0]; part[3 * blockIdx.x + 2] = bad_s[0]; }
}

// b = min(255, floor((v - lo) * s)), s = 256.0 / (hi - lo) formed on the host
template <class T>
__global__ void __launch_bounds__(BT) k_brain_hist(const T* __restrict__ I, int64_t V, double lo, double s, u64* __restrict__ H) {
    __shared__ unsigned int counts[NBIN];          // a workgroup sees fewer than 2^32 voxels
    for (int b = threadIdx.x; b < NBIN; b += BT) counts[b] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < V; i += (int64_t)gridDim.x * BT) {
        double q = floor(((double)I[i] - lo) * s);
        q = !(q > 0.0) ? 0.0 : (q > 255.0 ? 255.0 : q);
        atomicAdd(&counts[(int)q], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < NBIN; b += BT)
        if (counts[b]) atomicAdd(&H[b], (u64)counts[b]);
}

// ---------------------------------------------------------------- Laplacian of Gaussian
// taps of one axis: phi at t[0 .. 2 r], phi'' at t[BTAPS .. BTAPS + 2 r]
template <class T>
__global__ void __launch_bounds__(BT) k_brain_axis2(const T* __restrict__ in, double* __restrict__ A0, double* __restrict__ A2,
                                                    const double* __restrict__ t, int64_t rows, int n2, int r) {
    __shared__ double seg[BX2 + 2 * BMAXR];
    const int64_t row = (int64_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (row >= rows) return;                       // (the whole workgroup)
    const int x0 = (int)blockIdx.x * BX2, tid = (int)threadIdx.x;
    const T* __restrict__ src = in + row * n2;
    for (int s = tid; s < BX2 + 2 * r; s += BT) seg[s] = (double)src[clampi(x0 - r + s, n2 - 1)];
    __syncthreads();
    const int x = x0 + tid;
    if (x >= n2) return;
    double a0 = 0.0, a2 = 0.0;
    for (int k = -r; k <= r; k++) {
        const double v = seg[tid + r - k];         // the sample at clamp(x - k)
        a0 = a0 + t[k + r] * v;
        a2 = a2 + t[BTAPS + k + r] * v;
    }
    A0[row * n2 + x] = a0; A2[row * n2 + x] = a2;
}

// B00 = phi * A0, B20 = phi'' * A0, B02 = phi * A2 along axis 1.  Output row y takes the input row p' = y - k with the tap
// k + r = y - p' + r: walking p' downwards is walking k upwards, the order of the definition.
__global__ void __launch_bounds__(BT) k_brain_axis1(const double* __restrict__ A0, const double* __restrict__ A2, double* __restrict__ B00,
                                                    double* __restrict__ B20, double* __restrict__ B02, const double* __restrict__ t, Geo g, int r) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = (int)blockIdx.x * BLX + lane, xg = min(x, g.n2 - 1);
    const int y0 = ((int)blockIdx.y * 4 + wave) * BY, z = (int)blockIdx.z;
    if (y0 >= g.n1) return;                        // (a whole wave; no barrier in this kernel)
    const size_t plane = (size_t)z * g.n1 * g.n2;
    double s00[BY], s20[BY], s02[BY];
#pragma unroll
    for (int j = 0; j < BY; j++) { s00[j] = 0.0; s20[j] = 0.0; s02[j] = 0.0; }
    for (int pp = y0 + BY - 1 + r; pp >= y0 - r; pp--) {
        const size_t at = plane + (size_t)clampi(pp, g.n1 - 1) * g.n2 + xg;
        const double a0 = A0[at], a2 = A2[at];
#pragma unroll
        for (int j = 0; j < BY; j++) {
            const int kk = y0 + j - pp + r;        // (the same in every lane)
            if (kk >= 0 && kk <= 2 * r) {
                const double w0 = t[kk], w2 = t[BTAPS + kk];
                s00[j] = s00[j] + w0 * a0;
                s20[j] = s20[j] + w2 * a0;
                s02[j] = s02[j] + w0 * a2;
            }
        }
    }
    if (x < g.n2) {
#pragma unroll
        for (int j = 0; j < BY; j++) {
            const int y = y0 + j;
            if (y < g.n1) { const size_t o = plane + (size_t)y * g.n2 + x; B00[o] = s00[j]; B20[o] = s20[j]; B02[o] = s02[j]; }
        }
    }
}

// T0 = phi'' * B00, T1 = phi * B20, T2 = phi * B02 along axis 0; E = (c0 T0 + c1 T1) + c2 T2, c_a = sigma^2 / h_a^2.
// MODE 0: E is written.  MODE 1: only the candidate (J > floor) & (E <= thr), one ballot word per wave and plane - every lane of
// a wave stays active to the end, the lanes past the row's end with clamped loads and a 0 bit.
struct LogEnd { double c0, c1, c2, floor, thr; };
template <class T, int MODE>
__global__ void __launch_bounds__(BT) k_brain_axis0(const double* __restrict__ B00, const double* __restrict__ B20, const double* __restrict__ B02,
                                                    const T* __restrict__ J, const double* __restrict__ t, Geo g, int r, LogEnd e,
                                                    double* __restrict__ E, u64* __restrict__ bits) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = (int)blockIdx.x * BLX + lane, xg = min(x, g.n2 - 1);
    const int y = (int)blockIdx.y * 4 + wave, z0 = (int)blockIdx.z * BZ;
    if (y >= g.n1) return;                         // (a whole wave; no barrier in this kernel)
    const size_t plane = (size_t)g.n1 * g.n2, inrow = (size_t)y * g.n2 + xg;
    double s0[BZ], s1[BZ], s2[BZ];
#pragma unroll
    for (int j = 0; j < BZ; j++) { s0[j] = 0.0; s1[j] = 0.0; s2[j] = 0.0; }
    for (int pp = z0 + BZ - 1 + r; pp >= z0 - r; pp--) {
        const size_t at = (size_t)clampi(pp, g.n0 - 1) * plane + inrow;
        const double b00 = B00[at], b20 = B20[at], b02 = B02[at];
#pragma unroll
        for (int j = 0; j < BZ; j++) {
            const int kk = z0 + j - pp + r;
            if (kk >= 0 && kk <= 2 * r) {
                const double w0 = t[kk], w2 = t[BTAPS + kk];
                s0[j] = s0[j] + w2 * b00;
                s1[j] = s1[j] + w0 * b20;
                s2[j] = s2[j] + w0 * b02;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < BZ; j++) {
        const int z = z0 + j;
        if (z < g.n0) {                            // (the same in every lane)
            const double v = (e.c0 * s0[j] + e.c1 * s1[j]) + e.c2 * s2[j];
            if constexpr (MODE == 0) {
                if (x < g.n2) E[(size_t)z * plane + inrow] = v;
            } else {
                const double jv = (double)J[(size_t)z * plane + inrow];
                const u64 word = __ballot(x < g.n2 && jv > e.floor && v <= e.thr);
                if (lane == 0) bits[((size_t)z * g.n1 + y) * g.W + blockIdx.x] = word;
            }
        }
    }
}

// ---------------------------------------------------------------- packed bit volumes
// one wave per word: the word index is the same in every lane of a wave (workgroups of 256 threads, strides of whole workgroups)
#define FOR_EACH_WORD(w, nwords) \
    for (size_t w = (size_t)blockIdx.x * (BT / 64) + (threadIdx.x >> 6); w < (nwords); w += (size_t)gridDim.x * (BT / 64))

__global__ void __launch_bounds__(BT) k_bits_pack(const uint8_t* __restrict__ bytes, u64* __restrict__ bits, Geo g) {
    const int lane = (int)threadIdx.x & 63;
    const size_t nwords = g.words();
    FOR_EACH_WORD(w, nwords) {
        const size_t row = w / g.W;
        const int x = (int)(w - row * g.W) * 64 + lane;
        const u64 word = __ballot(x < g.n2 && bytes[row * g.n2 + min(x, g.n2 - 1)] != 0);
        if (lane == 0) bits[w] = word;
    }
}
__global__ void __launch_bounds__(BT) k_bits_unpack(const u64* __restrict__ bits, uint8_t* __restrict__ bytes, Geo g, int complement) {
    const int lane = (int)threadIdx.x & 63;
    const size_t nwords = g.words();
    FOR_EACH_WORD(w, nwords) {
        const size_t row = w / g.W;
        const int x = (int)(w - row * g.W) * 64 + lane;
        if (x < g.n2) bytes[row * g.n2 + x] = (uint8_t)(((bits[w] >> lane) & 1ull) ^ (u64)complement);
    }
}
__global__ void __launch_bounds__(BT) k_bits_count(const u64* __restrict__ bits, size_t nwords, u64* total) {
    unsigned int mine = 0;                         // (a thread sees fewer than 2^32 voxels)
    for (size_t w = (size_t)blockIdx.x * BT + threadIdx.x; w < nwords; w += (size_t)gridDim.x * BT) mine += (unsigned)__popcll(bits[w]);
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(total, (u64)mine);
}

// One step of the cross.  Outside the volume a voxel counts as `border` (0 or 1; dilation: 0).  The padding bits of a row's
// last word are 0 in memory: they take the border's value for the shifts and are cleared again in the result.
template <bool ERODE>
__global__ void __launch_bounds__(BT) k_bits_morph(const u64* __restrict__ in, u64* __restrict__ out, Geo g, int border) {
    const size_t nwords = g.words();
    const u64 fill = border ? ~0ull : 0ull;
    for (size_t w = (size_t)blockIdx.x * BT + threadIdx.x; w < nwords; w += (size_t)gridDim.x * BT) {
        const size_t row = w / g.W;
        const int wi = (int)(w - row * g.W), i0 = (int)(row / g.n1), i1 = (int)(row - (size_t)i0 * g.n1);
        const int live = min(64, g.n2 - wi * 64);                                  // voxels of this word
        const u64 valid = live == 64 ? ~0ull : ((1ull << live) - 1ull);
        const u64 c = in[w] | (fill & ~valid);
        const u64 prev = wi > 0 ? in[w - 1] : fill, next = wi + 1 < g.W ? in[w + 1] : fill;
        const u64 lo = (c << 1) | (prev >> 63);                                    // the voxel at i2 - 1
        const u64 hi = (c >> 1) | (next << 63);                                    // the voxel at i2 + 1
        const u64 up = i1 > 0 ? in[w - g.W] : fill, dn = i1 + 1 < g.n1 ? in[w + g.W] : fill;
        const size_t pw = (size_t)g.n1 * g.W;
        const u64 fr = i0 > 0 ? in[w - pw] : fill, bk = i0 + 1 < g.n0 ? in[w + pw] : fill;
        const u64 res = ERODE ? (c & lo & hi & up & dn & fr & bk) : (c | lo | hi | up | dn | fr | bk);
        out[w] = res & valid;
    }
}

// ---------------------------------------------------------------- the main component
// Sizes by rank.  A wave owns a contiguous run of 64-voxel trips; per trip the lanes of one component add their number once
// (ballot, popcount), and the wave keeps the counts of the two components it met last in registers - every value below is the
// same in all lanes of the wave - so that a component reaches its counter in memory once per wave and change of neighbourhood,
// not once per voxel or per trip.  (Measured at 512x512x170 before the two-entry memory and the contiguous runs, with the
// lanes outside the first lane's component adding one each: 44 ms, the brain's and the scalp's counters taking millions of
// same-address atomics one after another)
constexpr int SIZES_GRID = 2048;
__global__ void __launch_bounds__(BT) k_brain_sizes(const int32_t* __restrict__ root, CcRank rk, u64* __restrict__ sizes, uint32_t V) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t trips = (V + 63u) / 64u, nwave = gridDim.x * (BT / 64), wave = blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
    const uint32_t per = (trips + nwave - 1u) / nwave;
    const uint32_t t0 = min(wave * per, trips), t1 = min(t0 + per, trips);
    uint32_t held0 = 0xffffffffu, held1 = 0xffffffffu;
    u64 n0 = 0, n1 = 0;
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t i = t * 64u + lane;
        const int32_t r = i < V ? root[i] : -1;
        const bool fg = r >= 0;
        const uint32_t rank = fg ? cc_rank(rk, (uint32_t)r) : 0xffffffffu;
        u64 rest = __ballot(fg);
        while (rest) {                             // (once per component of the trip)
            const int first = __ffsll((long long)rest) - 1;
            const uint32_t lead = (uint32_t)__shfl((int)rank, first, 64);
            const u64 same = __ballot(fg && rank == lead);
            const u64 n = (u64)__popcll(same);
            rest &= ~same;
            if (lead == held0) n0 += n;
            else if (lead == held1) n1 += n;
            else if (n0 <= n1) { if (n0 && lane == 0) atomicAdd(&sizes[held0], n0); held0 = lead; n0 = n; }
            else { if (n1 && lane == 0) atomicAdd(&sizes[held1], n1); held1 = lead; n1 = n; }
        }
    }
    if (lane == 0) { if (n0) atomicAdd(&sizes[held0], n0); if (n1) atomicAdd(&sizes[held1], n1); }
}
__global__ void __launch_bounds__(BT) k_brain_winner(const u64* __restrict__ sizes, uint32_t ncomp, u64* best) {
    u64 mine = 0;                                  // (a size is below 2^31; the largest size wins, among equals the smallest rank)
    for (uint32_t k = blockIdx.x * BT + threadIdx.x; k < ncomp; k += gridDim.x * BT) {
        const u64 key = (sizes[k] << 32) | (u64)(0xffffffffu - k);
        mine = key > mine ? key : mine;
    }
    for (int o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(mine, o, 64); mine = other > mine ? other : mine; }
    if ((threadIdx.x & 63) == 0 && mine) atomicMax(best, mine);
}
__global__ void __launch_bounds__(BT) k_brain_select(const int32_t* __restrict__ root, CcRank rk, uint32_t win, u64* __restrict__ bits, Geo g) {
    const int lane = (int)threadIdx.x & 63;
    const size_t nwords = g.words();
    FOR_EACH_WORD(w, nwords) {
        const size_t row = w / g.W;
        const int x = (int)(w - row * g.W) * 64 + lane;
        const int32_t r = x < g.n2 ? root[row * g.n2 + x] : -1;
        const u64 word = __ballot(r >= 0 && cc_rank(rk, (uint32_t)r) == win);
        if (lane == 0) bits[w] = word;
    }
}

// ---------------------------------------------------------------- hole filling
// root: the labelling of the complement.  Face voxel f of 2 (n1 n2 + n0 n2 + n0 n1): its component is open.
__global__ void __launch_bounds__(BT) k_fill_faces(const int32_t* __restrict__ root, CcRank rk, uint8_t* __restrict__ open, Geo g) {
    const size_t f0 = (size_t)g.n1 * g.n2, f1 = (size_t)g.n0 * g.n2, f2 = (size_t)g.n0 * g.n1, total = 2 * (f0 + f1 + f2);
    for (size_t f = (size_t)blockIdx.x * BT + threadIdx.x; f < total; f += (size_t)gridDim.x * BT) {
        size_t q = f;
        int i0, i1, i2;
        if (q < 2 * f0) { i0 = q < f0 ? 0 : g.n0 - 1; q = q < f0 ? q : q - f0; i1 = (int)(q / g.n2); i2 = (int)(q - (size_t)i1 * g.n2); }
        else if (q < 2 * (f0 + f1)) { q -= 2 * f0; i1 = q < f1 ? 0 : g.n1 - 1; q = q < f1 ? q : q - f1; i0 = (int)(q / g.n2); i2 = (int)(q - (size_t)i0 * g.n2); }
        else { q -= 2 * (f0 + f1); i2 = q < f2 ? 0 : g.n2 - 1; q = q < f2 ? q : q - f2; i0 = (int)(q / g.n1); i1 = (int)(q - (size_t)i0 * g.n1); }
        const int32_t r = root[((size_t)i0 * g.n1 + i1) * g.n2 + i2];
        if (r >= 0) open[cc_rank(rk, (uint32_t)r)] = 1;
    }
}
__global__ void __launch_bounds__(BT) k_fill_apply(const int32_t* __restrict__ root, CcRank rk, const uint8_t* __restrict__ open, u64* __restrict__ bits, Geo g) {
    const int lane = (int)threadIdx.x & 63;
    const size_t nwords = g.words();
    FOR_EACH_WORD(w, nwords) {
        const size_t row = w / g.W;
        const int x = (int)(w - row * g.W) * 64 + lane;
        const int32_t r = x < g.n2 ? root[row * g.n2 + x] : -1;
        const u64 word = __ballot(r >= 0 && !open[cc_rank(rk, (uint32_t)r)]);
        if (lane == 0 && word) bits[w] |= word;    // (this wave alone touches the word)
    }
}

// ---------------------------------------------------------------- host
// the bytes that a call holds on the device, and their peak
struct Meter {
    std::map<const void*, size_t> held; size_t now = 0, peak = 0;
    void add(const void* p, size_t bytes) { held[p] = bytes; now += bytes; peak = std::max(peak, now); }
    void sub(const void* p) { const auto it = held.find(p); if (it != held.end()) { now -= it->second; held.erase(it); } }
    void pass(size_t bytes) { peak = std::max(peak, now + bytes); }             // held and given back inside a callee
};
template <class T> int mgrab(DevMem& mem, Meter& mt, T** p, size_t count, const char* what) {
    const int rc = mem.grab(p, count, what);
    if (!rc) mt.add(*p, std::max<size_t>(1, count) * sizeof(T));
    return rc;
}
void mdrop(DevMem& mem, Meter& mt, const void* p) { mt.sub(p); mem.drop(p); }
#define BRAIN_GRAB(p, count, what) do { int rc_ = mgrab(mem, mt, &(p), (count), (what)); if (rc_) return rc_; } while (0)

struct Events {                                    // HIP events of one call, destroyed when the owner leaves scope
    hipEvent_t e[8]; int n = 0;
    ~Events() { for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]); }
    int make(int count) { for (; n < count; n++) VMASK_TRY(hipEventCreate(&e[n])); return VRG_OK; }
    int mark(int k) { VMASK_TRY(hipEventRecord(e[k], 0)); return VRG_OK; }
    int micros(int a, int b, int64_t* out) { float ms = 0.f; VMASK_TRY(hipEventElapsedTime(&ms, e[a], e[b])); *out = (int64_t)((double)ms * 1000.0 + 0.5); return VRG_OK; }
};
struct CcHold {                                    // a labelling, released when the holder leaves scope
    vmask::CcOut c;
    ~CcHold() { vmask::cc_release(c); }
};
// what cc_label holds at its peak: parents, roots (4 bytes per voxel each), the root bitmap and its scan (12 bytes per 64 voxels)
size_t cc_bytes(const Geo& g) { return 8 * g.V() + 12 * ((g.V() + 63) / 64) + 4096; }

int sync_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { vmask::set_error(std::string(what) + ": " + hipGetErrorString(e)); return VRG_E_INTERNAL; }
    return VRG_OK;
}

// phi and phi'' of the three axes, [axis][2][BTAPS], as vmask_vesselness forms them; false: a radius outside 1 .. BMAXR
bool brain_taps(double sigma, const double* h, int* r, std::vector<double>& t) {
    t.assign((size_t)3 * 2 * BTAPS, 0.0);
    for (int a = 0; a < 3; a++) {
        const double s = sigma / h[a], rr = 4.0 * s + 0.5;
        if (!(rr >= 1.0) || !(rr < (double)(BMAXR + 1))) return false;
        r[a] = (int)rr;
        double* p = t.data() + (size_t)a * 2 * BTAPS;
        double sum = 0.0;
        for (int x = -r[a]; x <= r[a]; x++) { p[x + r[a]] = std::exp(-0.5 * (double)x * x / (s * s)); sum += p[x + r[a]]; }
        for (int x = -r[a]; x <= r[a]; x++) {
            const double phi = p[x + r[a]] / sum;
            p[x + r[a]] = phi;
            p[BTAPS + x + r[a]] = ((double)x * x / (s * s * s * s) - 1.0 / (s * s)) * phi;
        }
    }
    return true;
}

// the three passes on a device-resident volume.  MODE 0: dE receives E; MODE 1: dbits the candidate.
template <class T>
int log_passes(DevMem& mem, Meter& mt, const T* din, const Geo& g, double sigma, const double* h, int mode, double floor, double thr, double* dE, u64* dbits) {
    int r[3];
    std::vector<double> taps;
    if (!brain_taps(sigma, h, r, taps)) { vmask::set_error("internal: taps"); return VRG_E_INTERNAL; }
    const size_t V = g.V();
    double* dt = nullptr; double *A0 = nullptr, *A2 = nullptr, *B00 = nullptr, *B20 = nullptr, *B02 = nullptr;
    BRAIN_GRAB(dt, taps.size(), "taps");
    VMASK_TRY(hipMemcpy(dt, taps.data(), taps.size() * 8, hipMemcpyHostToDevice));
    BRAIN_GRAB(A0, V, "Gaussian derivatives"); BRAIN_GRAB(A2, V, "Gaussian derivatives");
    {
        const dim3 gr = grid_xy(g.rows());
        k_brain_axis2<T><<<dim3((unsigned)((g.n2 + BX2 - 1) / BX2), gr.x, gr.y), BT>>>(din, A0, A2, dt + 2 * 2 * BTAPS, (int64_t)g.rows(), g.n2, r[2]);
    }
    BRAIN_GRAB(B00, V, "Gaussian derivatives"); BRAIN_GRAB(B20, V, "Gaussian derivatives"); BRAIN_GRAB(B02, V, "Gaussian derivatives");
    k_brain_axis1<<<dim3((unsigned)g.W, (unsigned)((g.n1 + 4 * BY - 1) / (4 * BY)), (unsigned)g.n0), BT>>>(A0, A2, B00, B20, B02, dt + 1 * 2 * BTAPS, g, r[1]);
    int rc = sync_check("edge passes");
    if (rc) return rc;
    mdrop(mem, mt, A0); mdrop(mem, mt, A2);
    LogEnd e;
    const double s2 = sigma * sigma;
    e.c0 = s2 / (h[0] * h[0]); e.c1 = s2 / (h[1] * h[1]); e.c2 = s2 / (h[2] * h[2]); e.floor = floor; e.thr = thr;
    const dim3 g0((unsigned)g.W, (unsigned)((g.n1 + 3) / 4), (unsigned)((g.n0 + BZ - 1) / BZ));
    if (mode == 0) k_brain_axis0<T, 0><<<g0, BT>>>(B00, B20, B02, din, dt, g, r[0], e, dE, nullptr);
    else k_brain_axis0<T, 1><<<g0, BT>>>(B00, B20, B02, din, dt, g, r[0], e, nullptr, dbits);
    rc = sync_check("edge passes");
    mdrop(mem, mt, B00); mdrop(mem, mt, B20); mdrop(mem, mt, B02); mdrop(mem, mt, dt);
    return rc;
}

// `steps` steps of the cross from *cur, ping-pong with *other: the result is *cur again
void morph(u64** cur, u64** other, const Geo& g, bool erode, int steps, int border) {
    for (int s = 0; s < steps; s++) {
        if (erode) k_bits_morph<true><<<grid_for(g.words()), BT>>>(*cur, *other, g, border);
        else k_bits_morph<false><<<grid_for(g.words()), BT>>>(*cur, *other, g, 0);
        std::swap(*cur, *other);
    }
}

int count_bits(const u64* bits, const Geo& g, u64* dcount, int64_t* out) {
    VMASK_TRY(hipMemset(dcount, 0, 8));
    k_bits_count<<<grid_for(g.words()), BT>>>(bits, g.words(), dcount);
    u64 n = 0;
    VMASK_TRY(hipMemcpy(&n, dcount, 8, hipMemcpyDeviceToHost));
    *out = (int64_t)n;
    return VRG_OK;
}

// the component of `bits` that is kept, as bits, into `out` (which may be `bits`): the largest under `connectivity`, ties to the
// one met first in raster order, or the one that holds voxel `seed` (>= 0).  tmp: V bytes.  An empty volume gives an empty one.
// size_us (may be NULL): the microseconds of the size pass alone.
int main_component(Meter& mt, const u64* bits, u64* out, uint8_t* tmp, const Geo& g, int connectivity, int64_t seed, int64_t* size, int64_t* ncomp,
                   int64_t* size_us = nullptr) {
    k_bits_unpack<<<grid_for(g.words() * 64), BT>>>(bits, tmp, g, 0);
    CcHold hold;
    mt.pass(cc_bytes(g));
    int rc = vmask::cc_label(tmp, g.n0, g.n1, g.n2, connectivity, false, hold.c);
    if (rc) return rc;
    const vmask::CcOut& c = hold.c;
    if (ncomp) *ncomp = c.ncomp;
    if (size) *size = 0;
    if (c.ncomp == 0) {
        if (seed >= 0) { vmask::set_error("the seed voxel is not in the set"); return VRG_E_ARG; }
        VMASK_TRY(hipMemset(out, 0, g.words() * 8));
        return VRG_OK;
    }
    DevMem mem;
    u64* sizes = nullptr; u64* best = nullptr;
    BRAIN_GRAB(sizes, (size_t)c.ncomp, "component sizes"); BRAIN_GRAB(best, 1, "winner");
    VMASK_TRY(hipMemset(sizes, 0, (size_t)c.ncomp * 8)); VMASK_TRY(hipMemset(best, 0, 8));
    const uint32_t V = (uint32_t)g.V();
    Events ev;
    if (size_us) { int r = ev.make(2); if (r || (r = ev.mark(0))) return r; }
    k_brain_sizes<<<std::min(grid_for(V), SIZES_GRID), BT>>>(c.root, c.rank(), sizes, V);
    if (size_us) { int r = ev.mark(1); if (r) return r; }
    uint32_t win = 0;
    if (seed >= 0) {
        int32_t r = -1;
        VMASK_TRY(hipMemcpy(&r, c.root + seed, 4, hipMemcpyDeviceToHost));
        if (r < 0) { vmask::set_error("the seed voxel is not in the set"); return VRG_E_ARG; }
        uint32_t off = 0; u64 word = 0;
        VMASK_TRY(hipMemcpy(&off, c.off + ((uint32_t)r >> 6), 4, hipMemcpyDeviceToHost));
        VMASK_TRY(hipMemcpy(&word, c.bits + ((uint32_t)r >> 6), 8, hipMemcpyDeviceToHost));
        win = off + (uint32_t)__builtin_popcountll(word & ((1ull << ((uint32_t)r & 63u)) - 1ull));
    } else {
        k_brain_winner<<<grid_for(c.ncomp), BT>>>(sizes, c.ncomp, best);
        u64 key = 0;
        VMASK_TRY(hipMemcpy(&key, best, 8, hipMemcpyDeviceToHost));
        win = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    }
    if (size) { u64 s = 0; VMASK_TRY(hipMemcpy(&s, sizes + win, 8, hipMemcpyDeviceToHost)); *size = (int64_t)s; }
    k_brain_select<<<grid_for(g.words() * 64), BT>>>(c.root, c.rank(), win, out, g);
    int rs = sync_check("component selection");
    mt.sub(sizes); mt.sub(best);
    if (!rs && size_us) rs = ev.micros(0, 1, size_us);
    return rs;
}

// the complement's components that touch no face are added to `bits`.  tmp: V bytes.
int fill_holes(Meter& mt, u64* bits, uint8_t* tmp, const Geo& g) {
    k_bits_unpack<<<grid_for(g.words() * 64), BT>>>(bits, tmp, g, 1);
    CcHold hold;
    mt.pass(cc_bytes(g));
    int rc = vmask::cc_label(tmp, g.n0, g.n1, g.n2, 1, false, hold.c);
    if (rc) return rc;
    const vmask::CcOut& c = hold.c;
    if (c.ncomp == 0) return VRG_OK;
    DevMem mem;
    uint8_t* open = nullptr;
    BRAIN_GRAB(open, (size_t)c.ncomp, "open components");
    VMASK_TRY(hipMemset(open, 0, (size_t)c.ncomp));
    const size_t faces = 2 * ((size_t)g.n1 * g.n2 + (size_t)g.n0 * g.n2 + (size_t)g.n0 * g.n1);
    k_fill_faces<<<grid_for(faces), BT>>>(c.root, c.rank(), open, g);
    k_fill_apply<<<grid_for(g.words() * 64), BT>>>(c.root, c.rank(), open, bits, g);
    const int rs = sync_check("hole filling");
    mt.sub(open);
    return rs;
}

bool dtype_ok(int dtype) { return dtype == VRG_F32 || dtype == VRG_F64; }
bool spacing_ok(const double* spacing, double* h) {
    h[0] = h[1] = h[2] = 1.0;
    for (int a = 0; a < 3 && spacing; a++) {
        h[a] = spacing[a];
        if (!(std::isfinite(h[a]) && h[a] > 0.0)) return false;
    }
    return true;
}
bool sigma_ok(double sigma, const double* h) {
    if (!(std::isfinite(sigma) && sigma > 0.0)) return false;
    for (int a = 0; a < 3; a++) {
        const double rr = 4.0 * (sigma / h[a]) + 0.5;
        if (!(rr >= 1.0) || !(rr < (double)(BMAXR + 1))) return false;
    }
    return true;
}

// lo, hi and the number of non-finite voxels of a device-resident volume
template <class T> int extrema(const T* dv, size_t V, double* lo, double* hi, double* bad) {
    DevMem mem;
    const int nb = (int)std::min<size_t>((V + BT - 1) / BT, BGRID);
    double* part = nullptr;
    VMASK_GRAB(part, (size_t)3 * nb, "extrema");
    k_brain_minmax<T><<<nb, BT>>>(dv, (int64_t)V, part);
    std::vector<double> hpart((size_t)3 * nb);
    VMASK_TRY(hipMemcpy(hpart.data(), part, hpart.size() * 8, hipMemcpyDeviceToHost));
    *lo = INFINITY; *hi = -INFINITY; *bad = 0.0;
    for (int b = 0; b < nb; b++) { *lo = std::fmin(*lo, hpart[3 * b]); *hi = std::fmax(*hi, hpart[3 * b + 1]); *bad += hpart[3 * b + 2]; }
    return VRG_OK;
}

template <class T> int histogram(const T* volume, const Geo& g, double* lo, double* hi, uint64_t* counts) {
    DevMem mem;
    const size_t V = g.V();
    const T* dv = nullptr;
    int rc = bring(mem, volume, V, "volume", &dv);
    if (rc) return rc;
    double l, h, bad;
    rc = extrema(dv, V, &l, &h, &bad);
    if (rc) return rc;
    if (bad > 0.0) { vmask::set_error("brain histogram: the volume holds voxels that are not finite"); return VRG_E_ARG; }
    if (!(h > l)) { vmask::set_error("brain histogram: the volume is constant"); return VRG_E_ARG; }
    u64* dH = nullptr;
    VMASK_GRAB(dH, NBIN, "histogram");
    VMASK_TRY(hipMemset(dH, 0, NBIN * 8));
    k_brain_hist<T><<<(int)std::min<size_t>((V + BT - 1) / BT, BGRID), BT>>>(dv, (int64_t)V, l, 256.0 / (h - l), dH);
    rc = sync_check("histogram");
    if (rc) return rc;
    VMASK_TRY(hipMemcpy(counts, dH, NBIN * 8, hipMemcpyDefault));
    if (vmask::is_device_pointer(lo)) VMASK_TRY(hipMemcpy(lo, &l, 8, hipMemcpyHostToDevice)); else *lo = l;
    if (vmask::is_device_pointer(hi)) VMASK_TRY(hipMemcpy(hi, &h, 8, hipMemcpyHostToDevice)); else *hi = h;
    return VRG_OK;
}

template <class T> int finite_or_refuse(const T* dv, size_t V, const char* who) {
    double l, h, bad;
    const int rc = extrema(dv, V, &l, &h, &bad);
    if (rc) return rc;
    if (bad > 0.0) { vmask::set_error(std::string(who) + ": the volume holds voxels that are not finite"); return VRG_E_ARG; }
    return VRG_OK;
}

template <class T> int log_entry(const T* volume, const Geo& g, double sigma, const double* h, double* out) {
    DevMem mem; Meter mt;
    const T* dv = nullptr;
    int rc = bring(mem, volume, g.V(), "volume", &dv);
    if (rc) return rc;
    rc = finite_or_refuse(dv, g.V(), "brain edge response");
    if (rc) return rc;
    Out<double> o;
    rc = o.open(mem, out, g.V(), "edge response");
    if (rc) return rc;
    rc = log_passes<T>(mem, mt, dv, g, sigma, h, 0, 0.0, 0.0, o.dev, nullptr);
    return rc ? rc : o.close();
}

template <class T>
int extract(const T* volume, const Geo& g, double sigma, const double* h, double thr, double floor, int erosion, int closing, int64_t seed,
            uint8_t* out, uint8_t* stages, int64_t* info) {
    DevMem mem; Meter mt;
    const size_t V = g.V(), nw = g.words();
    int64_t inf[16] = {};
    Events ev;
    int rc = ev.make(7);
    if (rc) return rc;
    const T* dv = nullptr;
    rc = bring(mem, volume, V, "volume", &dv);
    if (rc) return rc;
    if (dv != volume) mt.add(dv, V * sizeof(T));
    rc = finite_or_refuse(dv, V, "brain extraction");
    if (rc) return rc;
    u64 *a = nullptr, *b = nullptr, *dcount = nullptr;
    BRAIN_GRAB(a, nw, "bit volume"); BRAIN_GRAB(b, nw, "bit volume"); BRAIN_GRAB(dcount, 1, "count");
    uint8_t* bytes = nullptr;                      // a stage as bytes: the labellings' input, and the way to a host `stages`
    const bool stages_dev = stages && vmask::is_device_pointer(stages);
    auto stage = [&](int k, const u64* bits) -> int {
        int r = count_bits(bits, g, dcount, &inf[k]);
        if (r || !stages) return r;
        uint8_t* dst = stages_dev ? stages + (size_t)k * V : bytes;
        k_bits_unpack<<<grid_for(nw * 64), BT>>>(bits, dst, g, 0);
        if (!stages_dev) VMASK_TRY(hipMemcpy(stages + (size_t)k * V, bytes, V, hipMemcpyDeviceToHost));
        return VRG_OK;
    };
    // steps 3 and 4: the candidate; the edge passes' float64 volumes are gone before anything is labelled
    if ((rc = ev.mark(0))) return rc;
    rc = log_passes<T>(mem, mt, dv, g, sigma, h, 1, floor, thr, nullptr, a);
    if (rc) return rc;
    if (dv != volume) mdrop(mem, mt, dv);
    BRAIN_GRAB(bytes, V, "byte volume");
    if ((rc = stage(0, a)) || (rc = ev.mark(1))) return rc;
    // step 5: opening around the main component
    morph(&a, &b, g, true, erosion, 0);
    if ((rc = stage(1, a)) || (rc = ev.mark(2))) return rc;
    int64_t size = 0, ncomp = 0;
    if ((rc = main_component(mt, a, a, bytes, g, 1, seed, &size, &ncomp, &inf[14]))) return rc;
    inf[6] = ncomp; inf[7] = size;
    if ((rc = stage(2, a)) || (rc = ev.mark(3))) return rc;
    morph(&a, &b, g, false, erosion, 0);
    // step 6: closing, the outside counting as 1 for its erosion
    morph(&a, &b, g, false, closing, 0);
    morph(&a, &b, g, true, closing, 1);
    if ((rc = stage(3, a)) || (rc = ev.mark(4))) return rc;
    // step 7
    if ((rc = fill_holes(mt, a, bytes, g))) return rc;
    if ((rc = stage(4, a)) || (rc = ev.mark(5))) return rc;
    Out<uint8_t> o;
    if (vmask::is_device_pointer(out)) { o.user = out; o.dev = out; o.count = V; }
    else { o.user = out; o.dev = bytes; o.count = V; }
    k_bits_unpack<<<grid_for(nw * 64), BT>>>(a, o.dev, g, 0);
    if ((rc = ev.mark(6)) || (rc = sync_check("brain extraction"))) return rc;
    if ((rc = o.close())) return rc;
    inf[5] = (int64_t)mt.peak;
    for (int k = 0; k < 6; k++)
        if ((rc = ev.micros(k, k + 1, &inf[8 + k]))) return rc;
    return info ? put(info, inf, 16) : VRG_OK;
}

// a uint8 volume of the caller as bits on the device
int pack_in(DevMem& mem, const uint8_t* mask, const Geo& g, u64** bits) {
    const uint8_t* dm = nullptr;
    int rc = bring(mem, mask, g.V(), "mask", &dm);
    if (rc) return rc;
    VMASK_GRAB(*bits, g.words(), "bit volume");
    k_bits_pack<<<grid_for(g.words() * 64), BT>>>(dm, *bits, g);
    rc = sync_check("packing");
    if (dm != mask) mem.drop(dm);
    return rc;
}
int unpack_out(DevMem& mem, const u64* bits, const Geo& g, uint8_t* out) {
    Out<uint8_t> o;
    int rc = o.open(mem, out, g.V(), "output");
    if (rc) return rc;
    k_bits_unpack<<<grid_for(g.words() * 64), BT>>>(bits, o.dev, g, 0);
    rc = sync_check("unpacking");
    return rc ? rc : o.close();
}

}  // namespace

extern "C" int vmask_brain_histogram(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, double* lo, double* hi, uint64_t* counts) {
    if (!volume || !lo || !hi || !counts) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!dtype_ok(dtype)) { vmask::set_error("brain histogram: the volume must be float32 or float64"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    if (dtype == VRG_F32) return histogram<float>((const float*)volume, g, lo, hi, counts);
    return histogram<double>((const double*)volume, g, lo, hi, counts);
}

extern "C" int vmask_brain_log(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing, double sigma, double* out) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!dtype_ok(dtype)) { vmask::set_error("brain edge response: the volume must be float32 or float64"); return VRG_E_ARG; }
    double h[3];
    if (!spacing_ok(spacing, h)) { vmask::set_error("brain edge response: the spacing must be finite and positive"); return VRG_E_ARG; }
    if (!sigma_ok(sigma, h)) { vmask::set_error("brain edge response: sigma must be finite and positive, with a tap radius int(4 sigma / spacing + 0.5) in 1..64"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    if (dtype == VRG_F32) return log_entry<float>((const float*)volume, g, sigma, h, out);
    return log_entry<double>((const double*)volume, g, sigma, h, out);
}

extern "C" int vmask_binary_morph(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, int op, int steps, int border, uint8_t* out) {
    if (!mask || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (op != 0 && op != 1) { vmask::set_error("morphology: op 0 (erode) or 1 (dilate)"); return VRG_E_ARG; }
    if (steps < 0 || steps > 100000) { vmask::set_error("morphology: 0 to 100000 steps"); return VRG_E_ARG; }
    if ((border != 0 && border != 1) || (op == 1 && border != 0)) { vmask::set_error("morphology: border 0 or 1, 0 for a dilation"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    DevMem mem;
    u64 *a = nullptr, *b = nullptr;
    if ((rc = pack_in(mem, mask, g, &a))) return rc;
    VMASK_GRAB(b, g.words(), "bit volume");
    morph(&a, &b, g, op == 0, steps, border);
    return unpack_out(mem, a, g, out);
}

extern "C" int vmask_largest_component(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, int connectivity, int64_t seed,
                                       uint8_t* out, int64_t* size) {
    if (!mask || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (connectivity < 1 || connectivity > 3) { vmask::set_error("largest component: connectivity 1, 2 or 3"); return VRG_E_ARG; }
    if (!vmask::shape_in_envelope(n0, n1, n2)) { vmask::set_error("shape out of range"); return VRG_E_ARG; }
    if (seed < -1 || seed >= n0 * n1 * n2) { vmask::set_error("largest component: the seed is a raster index of the volume, or -1"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    DevMem mem; Meter mt;
    u64* a = nullptr; uint8_t* bytes = nullptr;
    if ((rc = pack_in(mem, mask, g, &a))) return rc;
    VMASK_GRAB(bytes, g.V(), "byte volume");
    int64_t sz = 0;
    if ((rc = main_component(mt, a, a, bytes, g, connectivity, seed, &sz, nullptr))) return rc;
    mem.drop(bytes);
    if ((rc = unpack_out(mem, a, g, out))) return rc;
    return size ? put(size, &sz, 1) : VRG_OK;
}

extern "C" int vmask_fill_holes(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2, uint8_t* out) {
    if (!mask || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    DevMem mem; Meter mt;
    u64* a = nullptr; uint8_t* bytes = nullptr;
    if ((rc = pack_in(mem, mask, g, &a))) return rc;
    VMASK_GRAB(bytes, g.V(), "byte volume");
    if ((rc = fill_holes(mt, a, bytes, g))) return rc;
    mem.drop(bytes);
    return unpack_out(mem, a, g, out);
}

extern "C" int vmask_brain_extract(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing, double sigma,
                                   double threshold, double floor, int erosion, int closing, int64_t seed, uint8_t* out, uint8_t* stages, int64_t* info) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (!dtype_ok(dtype)) { vmask::set_error("brain extraction: the volume must be float32 or float64"); return VRG_E_ARG; }
    double h[3];
    if (!spacing_ok(spacing, h)) { vmask::set_error("brain extraction: the spacing must be finite and positive"); return VRG_E_ARG; }
    if (!sigma_ok(sigma, h)) { vmask::set_error("brain extraction: sigma must be finite and positive, with a tap radius int(4 sigma / spacing + 0.5) in 1..64"); return VRG_E_ARG; }
    if (std::isnan(threshold) || !std::isfinite(floor)) { vmask::set_error("brain extraction: the threshold must be a number and the floor finite"); return VRG_E_ARG; }
    if (erosion < 0 || erosion > 1000 || closing < 0 || closing > 1000) { vmask::set_error("brain extraction: erosion and closing 0 to 1000 steps"); return VRG_E_ARG; }
    if (!vmask::shape_in_envelope(n0, n1, n2)) { vmask::set_error("shape out of range"); return VRG_E_ARG; }
    if (seed < -1 || seed >= n0 * n1 * n2) { vmask::set_error("brain extraction: the seed is a raster index of the volume, or -1"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Geo g = geo(n0, n1, n2);
    if (dtype == VRG_F32) return extract<float>((const float*)volume, g, sigma, h, threshold, floor, erosion, closing, seed, out, stages, info);
    return extract<double>((const double*)volume, g, sigma, h, threshold, floor, erosion, closing, seed, out, stages, info);
}
