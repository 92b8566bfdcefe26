// vter_device.hip - vmask_territories of include/vmask.h: every voxel of the vessel mask gets the label of the segment that
// owns its nearest skeleton voxel, every segment the count of the voxels it received ("f8 territories").
//
// Sites = the voxels with skeleton != 0.  L(s) = 1 + the smallest k with s in segment k, 0 for a site in no segment.
// N(v) = the site at the smallest squared Euclidean distance from v, the one of smallest linear index among equidistant ones.
// labels = L(N(v)) inside the mask, nearest = idx(N(v)), sizes[l] = mask voxels with label l.
//
// Passes (kernel boundaries are the only hand-off between workgroups):
//   k_ter_sites      one thread per segment entry: atomicMin of k + 1 (k: binary search of the entry's position in offsets) into
//                    the site-label volume; entries that are no skeleton voxel and offsets that descend are counted
//   k_ter_rows       axis 2: one wave per row, the row's sites as one ballot word per 64 voxels; every voxel gets the i2 of the
//                    nearest site of its own row, the left one of two at equal distance
//   k_ter_envelope<1>  axis 1: Meijster's lower envelope over g^2 = (i2 - f2)^2; every voxel gets the winning j1 and the
//                    squared distance inside its plane
//   k_ter_envelope<0>  axis 0: the lower envelope over those; the winning j0 gives (j0, j1(j0), f2(j0, j1)) = N(v), and the
//                    finish is fused: label look-up, labels / nearest stores, sizes by one atomic per label and wave
// A line without a site contributes no parabola (it is skipped, not entered with an "infinite" value), so every number in
// the envelope arithmetic is a true squared distance: below 2^29 where n0^2 + n1^2 + n2^2 < 2^29 (32-bit arithmetic, the EDT's
// rule), below 2^32 inside the envelope of the passes (extents <= 32000; 64-bit arithmetic, 32-bit storage).
// The envelope: a stack of (site | start << 16, G(site)) per line, popped while the top's value at its start is strictly
// larger than the new parabola's there, the new start = 1 + the last position where the top is <= the new one: an equal value
// goes to the smaller line index, which over the axis order 2, 1, 0 is the smallest linear index (DESIGN.md has the argument).
// Both envelope passes have the lanes of a wave on neighbouring i2 (axis 0: on neighbouring i1 * n2 + i2): every row access is
// one contiguous request, no transpose.  The stack's top sits in registers, its topmost <= RING entries in LDS ([slot][thread]),
// deeper ones in a spill area in global memory, one region per line, moved in chunks of CHUNK entries (64 bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"

namespace {

constexpr int TPB = 256;
constexpr int GRID_LIST = 1024;                    // blocks, at most, of the kernel over segment entries
constexpr int ROW_WAVES = TPB / 64;
constexpr int ROW_WORDS = 512;                     // 64-voxel words of the longest row (extents <= 32000: 500)
constexpr int RING = 16, CHUNK = 8, AHEAD = 8, ENV_TPB = 64;
constexpr uint32_t NO_COORD = 0xffffu;             // in the 16-bit coordinate volumes: no site on the line
constexpr uint32_t NO_LABEL = 0xffffffffu;         // in the site-label volume: touched by no segment entry
constexpr int CTR_PAD = 32;                        // the bad-entry counter keeps 256 bytes to itself, the sizes follow

typedef unsigned long long u64;

struct Dim { int32_t n0, n1, n2; };

// ---- site labels
__global__ void __launch_bounds__(TPB) k_ter_sites(const int64_t* __restrict__ off, int64_t nseg, const int64_t* __restrict__ vox, u64 total,
                                                   const uint8_t* __restrict__ skel, u64 V, uint32_t* __restrict__ SL, u64* __restrict__ bad) {
    u64 wrong = 0;
    const u64 step = (u64)gridDim.x * TPB, first = (u64)blockIdx.x * TPB + threadIdx.x;
    for (u64 k = first; k < (u64)nseg; k += step) wrong += off[k] < 0 || off[k] > off[k + 1];
    for (u64 e = first; e < total; e += step) {
        const int64_t v = vox[e];
        if (v < 0 || (u64)v >= V || !skel[v]) { wrong++; continue; }
        int64_t lo = 0, hi = nseg;                                      // the k with off[k] <= e < off[k + 1]
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if ((u64)off[mid] <= e) lo = mid; else hi = mid; }
        atomicMin(&SL[v], (uint32_t)lo + 1u);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) wrong += __shfl_xor(wrong, o, 64);
    if (wrong && (threadIdx.x & 63u) == 0u) atomicAdd(bad, wrong);
}

// ---- axis 2: F2[v] = i2 of the nearest site in v's own row (the left one of two at equal distance), NO_COORD without one
__global__ void __launch_bounds__(TPB) k_ter_rows(const uint8_t* __restrict__ skel, uint16_t* __restrict__ F2, uint32_t nrows, int32_t n2) {
    __shared__ u64 words[ROW_WAVES][ROW_WORDS];
    __shared__ int32_t before[ROW_WAVES][ROW_WORDS];                    // the last site in front of a word, -1: none
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int32_t nw = (n2 + 63) / 64;
    for (uint32_t row0 = blockIdx.x * ROW_WAVES; row0 < nrows; row0 += gridDim.x * ROW_WAVES) {   // (the same trips in every wave of a block)
        const uint32_t row = row0 + wave;
        const bool live = row < nrows;
        const size_t at = (size_t)(live ? row : 0u) * (size_t)n2;
        int32_t prev = -1;
        for (int32_t c = 0; c < nw; c++) {
            const int32_t i2 = c * 64 + (int32_t)lane;
            const u64 w = __ballot(live && i2 < n2 && skel[at + i2] != 0);
            if (lane == 0u) { words[wave][c] = w; before[wave][c] = prev; }
            if (w) prev = c * 64 + 63 - __clzll((long long)w);
        }
        __syncthreads();
        int32_t next = -1;                                              // the first site behind a word
        for (int32_t c = nw - 1; c >= 0; c--) {
            const u64 w = words[wave][c];
            const int32_t i2 = c * 64 + (int32_t)lane;
            const u64 ml = w & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull)), mr = w & (~0ull << lane);
            const int32_t L = ml ? c * 64 + 63 - __clzll((long long)ml) : before[wave][c];
            const int32_t R = mr ? c * 64 + __ffsll((long long)mr) - 1 : next;
            uint32_t f = NO_COORD;
            if (L >= 0 && (R < 0 || i2 - L <= R - i2)) f = (uint32_t)L;
            else if (R >= 0) f = (uint32_t)R;
            if (live && i2 < n2) F2[at + i2] = (uint16_t)f;
            if (w) next = c * 64 + __ffsll((long long)w) - 1;
        }
        __syncthreads();
    }
}

// ---- the arithmetic of the envelope: int32_t where every square and sum stays below 2^30, else long long
// floor(a / b) for b > 0: the double quotient of a non-multiple lies at least 1 / b away from an integer, more than its
// rounding error while |a| < 2^52 (here |a| < 2^34, b < 2^17)
__device__ __forceinline__ long long floordiv(long long a, long long b) { return (long long)floor((double)a / (double)b); }
// 32 bits (|a| < 2^31, 0 < b < 2^16): a float quotient from the hardware reciprocal, off by less than 2^-6 while it is below
// 2^15, so its truncation is the floor or one beside it, set right by one multiplication; a quotient of 2^15 or more only
// has to come out larger than every extent (the entry is then not pushed)
__device__ __forceinline__ int32_t floordiv(int32_t a, int32_t b) {
    const float qf = (float)a * __builtin_amdgcn_rcpf((float)b);
    const bool big = fabsf(qf) >= 32768.f;
    int32_t q = big ? 0 : (int32_t)qf;
    const int32_t r = a - __mul24(q, b);
    q += (int32_t)(r >= b) - (int32_t)(r < 0);
    return big ? (qf > 0 ? (1 << 20) : -(1 << 20)) : q;
}
__device__ __forceinline__ int32_t mul_(int32_t a, int32_t b) { return __mul24(a, b); }
__device__ __forceinline__ long long mul_(long long a, long long b) { return a * b; }

// The lines of one envelope pass: line (o, c), o < nouter, c < ninner, has its voxel u at o * outer + c + u * stride (all
// below 2^31); the lanes of a wave take 64 neighbouring c of one o.
//   AXIS 1: o = i0, c = i2, u = i1: reads F2, writes J1 (the winning j1) and D1 (the squared distance inside the plane, -1: no site)
//   AXIS 0: o = 0, c = i1 * n2 + i2, u = i0: reads D1, and for the mask's voxels J1, F2 and the site labels; writes labels,
//           nearest and adds to cnt
struct Env {
    uint32_t nouter, ninner, outer, stride;
    int32_t m, n1, n2;
    uint16_t* F2; uint16_t* J1; int32_t* D1; uint2* SP;
    const uint8_t* mask; const uint32_t* SL; int32_t* labels; int64_t* nearest; u64* cnt; uint32_t nlab;
};
__host__ __device__ inline size_t padded(size_t m) { return (m + CHUNK - 1) / CHUNK * CHUNK; }

template <typename I, int AXIS>
__global__ void __launch_bounds__(ENV_TPB) k_ter_envelope(const Env a) {
    __shared__ uint2 ring[RING][ENV_TPB];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t cpl = (a.ninner + 63u) / 64u, nitems = a.nouter * cpl;
    const int32_t m = a.m;
    const size_t mp = padded((size_t)m);
    const uint32_t stride = a.stride;
    for (uint32_t item0 = blockIdx.x * (ENV_TPB / 64) + (tid >> 6); item0 < nitems; item0 += gridDim.x * (ENV_TPB / 64)) {
        const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item0);      // (the same in every lane of the wave)
        const uint32_t o = item / cpl, c0 = (item - o * cpl) * 64u + lane;
        const bool active = c0 < a.ninner;                             // (a lane past the end of the row meets no site and stores nothing)
        const uint32_t c = active ? c0 : 0u, base = o * a.outer + c;
        uint2* __restrict__ spill = a.SP + ((size_t)o * a.ninner + c) * mp;
#define AT(u) (base + (uint32_t)(u) * stride)
#define SLOT(i) ((uint32_t)(i) % (uint32_t)RING)
        // entries [low, q] of the stack are in the ring (entry i in slot i % RING), entries [0, low) in the spill area
        // (low a multiple of CHUNK); q == -1: no site yet
        int32_t q = -1, low = 0;
        I ts = 0, tt = 0, tg = 0, tv = 0;                              // the top: site, start, G(site), its value at its start
        auto load_top = [&]() {                                        // q was decremented and is >= 0: its entry becomes the top
            if (q < low) {                                             // (q == low - 1: the chunk below the ring comes back)
                low -= CHUNK;
                uint2 e[CHUNK];
#pragma unroll
                for (int i = 0; i < CHUNK; i++) e[i] = spill[low + i];
#pragma unroll
                for (int i = 0; i < CHUNK; i++) ring[SLOT(low + i)][tid] = e[i];
            }
            const uint2 p = ring[SLOT(q)][tid];
            ts = (I)(p.x & 0xffffu); tt = (I)(p.x >> 16); tg = (I)p.y; tv = mul_(tt - ts, tt - ts) + tg;
        };
        auto value = [&](int32_t u) -> I {                             // G(u), -1: the line through u has no site
            if (!active || u >= m) return (I)-1;
            if constexpr (AXIS == 1) {
                const uint32_t f = a.F2[AT(u)];
                const I g = (I)c - (I)f;
                return f == NO_COORD ? (I)-1 : mul_(g, g);
            } else {
                return (I)a.D1[AT(u)];
            }
        };
        for (int32_t u0 = 0; u0 < m; u0 += AHEAD) {
            I gv[AHEAD];
#pragma unroll
            for (int k = 0; k < AHEAD; k++) gv[k] = value(u0 + k);
#pragma unroll
            for (int k = 0; k < AHEAD; k++) {
                const I Gu = gv[k], u = (I)(u0 + k);
                if (Gu < 0) continue;
                while (q >= 0 && tv > mul_(tt - u, tt - u) + Gu) { if (--q >= 0) load_top(); }
                I w = 0;
                if (q >= 0) w = 1 + floordiv(mul_(u + ts, u - ts) + Gu - tg, (I)2 * (u - ts));   // (>= tt + 1: the top wins at its own start)
                if (w < (I)m) {
                    q++;
                    if (q - low >= RING) {                             // the ring is full: its oldest chunk moves to the spill area
#pragma unroll
                        for (int i = 0; i < CHUNK; i++) spill[low + i] = ring[SLOT(low + i)][tid];
                        low += CHUNK;
                    }
                    ts = u; tt = w; tg = Gu; tv = mul_(w - u, w - u) + Gu;
                    ring[SLOT(q)][tid] = make_uint2((uint32_t)u | ((uint32_t)w << 16), (uint32_t)Gu);
                }
            }
        }
        uint32_t i1 = 0, i2 = 0;
        if constexpr (AXIS == 0) { i1 = c / (uint32_t)a.n2; i2 = c - i1 * (uint32_t)a.n2; }
        for (int32_t u = m - 1; u >= 0; u--) {                         // (the same trips in every lane of a wave)
            const bool have = q >= 0;
            const uint32_t at = AT(u);
            if constexpr (AXIS == 1) {
                if (active) {
                    const I dd = (I)u - ts;
                    a.J1[at] = (uint16_t)(have ? (uint32_t)ts : NO_COORD);
                    a.D1[at] = have ? (int32_t)(mul_(dd, dd) + tg) : -1;
                }
            } else {
                const bool in = active && a.mask[at] != 0;
                uint32_t lab = 0;
                int64_t near = -1;
                if (in && have) {
                    const uint32_t j0 = (uint32_t)ts, j1 = a.J1[j0 * stride + c];
                    if (j1 < (uint32_t)a.n1) {                          // (always: the plane j0 has a site, or it had entered no parabola)
                        const uint32_t row = (j0 * (uint32_t)a.n1 + j1) * (uint32_t)a.n2, j2 = a.F2[row + i2];
                        if (j2 < (uint32_t)a.n2) {
                            near = (int64_t)(row + j2);
                            const uint32_t l = a.SL[row + j2];
                            lab = l == NO_LABEL || l >= a.nlab ? 0u : l;
                        }
                    }
                }
                if (active) {
                    a.labels[at] = (int32_t)lab;
                    if (a.nearest) a.nearest[at] = near;
                }
                u64 todo = __ballot(in);                               // one atomic per label among the wave's 64 voxels
                while (todo) {
                    const int lead = __ffsll((long long)todo) - 1;
                    const uint32_t l = (uint32_t)__shfl((int)lab, lead, 64);
                    const u64 same = __ballot(in && lab == l);
                    if ((int)lane == lead) atomicAdd(&a.cnt[l], (u64)__popcll(same));
                    todo &= ~same;
                }
            }
            if (have && (I)u == tt) { if (--q >= 0) load_top(); }
        }
#undef AT
#undef SLOT
    }
}

int grid_for(u64 items, u64 cap) { return (int)std::max<u64>(1, std::min<u64>(cap, items)); }

int territories(const uint8_t* mask, const uint8_t* skeleton, Dim d, const int64_t* offsets, int64_t nseg, const int64_t* voxels,
                int32_t* labels, int64_t* nearest, int64_t* sizes) {
    const u64 V = (u64)d.n0 * d.n1 * d.n2;
    DevMem mem;
    int64_t ends[2] = {0, 0};                                           // offsets[0], offsets[nseg]
    if (offsets) {
        if (vmask::is_device_pointer(offsets)) {
            VMASK_TRY(hipMemcpy(&ends[0], offsets, sizeof(int64_t), hipMemcpyDeviceToHost));
            VMASK_TRY(hipMemcpy(&ends[1], offsets + nseg, sizeof(int64_t), hipMemcpyDeviceToHost));
        } else { ends[0] = offsets[0]; ends[1] = offsets[nseg]; }
    }
    if (ends[0] != 0 || ends[1] < 0 || (ends[1] > 0 && !voxels)) { vmask::set_error("offsets do not start at 0, or end below it, or there are no voxels"); return VRG_E_ARG; }
    const u64 total = (u64)ends[1];
    const uint8_t* dmask; const uint8_t* dskel; const int64_t* doff = nullptr; const int64_t* dvox = nullptr;
    int rc = bring(mem, mask, V, "mask", &dmask);
    if (!rc) rc = bring(mem, skeleton, V, "skeleton", &dskel);
    if (!rc && nseg) rc = bring(mem, offsets, (size_t)nseg + 1, "offsets", &doff);
    if (!rc && total) rc = bring(mem, voxels, (size_t)total, "segment voxels", &dvox);
    if (rc) return rc;
    uint32_t* SL = nullptr; u64* ctr = nullptr; uint16_t* F2 = nullptr; uint16_t* J1 = nullptr; int32_t* D1 = nullptr; uint2* SP = nullptr;
    VMASK_GRAB(SL, V, "site labels");
    VMASK_GRAB(ctr, (size_t)CTR_PAD + (size_t)nseg + 1, "sizes");
    VMASK_TRY(hipMemsetAsync(SL, 0xff, V * sizeof(uint32_t), 0));
    VMASK_TRY(hipMemsetAsync(ctr, 0, ((size_t)CTR_PAD + (size_t)nseg + 1) * sizeof(u64), 0));
    if (nseg) {
        k_ter_sites<<<grid_for((std::max<u64>(total, (u64)nseg) + TPB - 1) / TPB, GRID_LIST), TPB>>>(doff, nseg, dvox, total, dskel, V, SL, ctr);
        u64 bad = 0;
        VMASK_TRY(hipMemcpy(&bad, ctr, sizeof(u64), hipMemcpyDeviceToHost));
        if (bad) { vmask::set_error(std::to_string(bad) + " segment entries that are no skeleton voxel of the volume (or offsets that descend)"); return VRG_E_ARG; }
    }
    const size_t lines = std::max((size_t)d.n0 * d.n2 * padded((size_t)d.n1), (size_t)d.n1 * d.n2 * padded((size_t)d.n0));
    VMASK_GRAB(F2, V, "row coordinates"); VMASK_GRAB(J1, V, "plane coordinates"); VMASK_GRAB(D1, V, "plane distances");
    VMASK_GRAB(SP, lines, "envelope spill area");
    Out<int32_t> olab; Out<int64_t> onear;                              // (nearest is optional: never opened, its dev stays null)
    if ((rc = olab.open(mem, labels, V, "labels")) || (nearest && (rc = onear.open(mem, nearest, V, "nearest")))) return rc;
    u64* cnt = ctr + CTR_PAD;

    const uint32_t nrows = (uint32_t)d.n0 * (uint32_t)d.n1;
    k_ter_rows<<<grid_for(((u64)nrows + ROW_WAVES - 1) / ROW_WAVES, 65535u * 16u), TPB>>>(dskel, F2, nrows, d.n2);
    // (every squared distance, and so every square and sum of the envelope passes, below 2^29: 32-bit arithmetic)
    const bool small = (int64_t)d.n0 * d.n0 + (int64_t)d.n1 * d.n1 + (int64_t)d.n2 * d.n2 < ((int64_t)1 << 29);
    Env e;
    e.n1 = d.n1; e.n2 = d.n2; e.F2 = F2; e.J1 = J1; e.D1 = D1; e.SP = SP;
    e.mask = dmask; e.SL = SL; e.labels = olab.dev; e.nearest = onear.dev; e.cnt = cnt; e.nlab = (uint32_t)nseg + 1u;
    auto egrid = [](const Env& x) { return grid_for((u64)x.nouter * ((x.ninner + 63u) / 64u), 65535u * 16u); };
    e.nouter = (uint32_t)d.n0; e.ninner = (uint32_t)d.n2; e.outer = (uint32_t)d.n1 * (uint32_t)d.n2; e.stride = (uint32_t)d.n2; e.m = d.n1;
    if (small) k_ter_envelope<int32_t, 1><<<egrid(e), ENV_TPB>>>(e);
    else k_ter_envelope<long long, 1><<<egrid(e), ENV_TPB>>>(e);
    e.nouter = 1u; e.ninner = (uint32_t)d.n1 * (uint32_t)d.n2; e.outer = 0u; e.stride = e.ninner; e.m = d.n0;
    if (small) k_ter_envelope<int32_t, 0><<<egrid(e), ENV_TPB>>>(e);
    else k_ter_envelope<long long, 0><<<egrid(e), ENV_TPB>>>(e);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if ((rc = olab.close()) || (rc = onear.close())) return rc;
    VMASK_TRY(hipMemcpy(sizes, cnt, ((size_t)nseg + 1) * sizeof(int64_t), vmask::is_device_pointer(sizes) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_territories(int device, const uint8_t* mask, const uint8_t* skeleton, int64_t n0, int64_t n1, int64_t n2,
                                 const int64_t* offsets, int64_t nseg, const int64_t* voxels,
                                 int32_t* labels, int64_t* nearest, int64_t* sizes) {
    if (!mask || !skeleton || !labels || !sizes) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nseg < 0 || nseg >= 0x7fffffff - 1) { vmask::set_error("segment count out of range"); return VRG_E_ARG; }
    if (nseg && !offsets) { vmask::set_error("segments without offsets"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Dim d;
    d.n0 = (int32_t)n0; d.n1 = (int32_t)n1; d.n2 = (int32_t)n2;
    return territories(mask, skeleton, d, offsets, nseg, voxels, labels, nearest, sizes);
}
