// vgeo_device.hip - vmask_geodesic of include/vmask.h: shortest-path distance from seed voxels through the 26-adjacency graph of
// the mask, and the label of the seed that every voxel's shortest paths come from ("f9 geodesic").
//
// D(seed) = 0, elsewhere D(v) = min over in-mask neighbours u of fl(D(u) + w(u - v)) in IEEE double: the least fixed point, what
// Dijkstra computes with the same addition.  Lab(seed) = its (smallest) label, elsewhere the smallest Lab(u) among the tight
// predecessors, fl(D(u) + w) == D(v).  Both are unique fixed points, so the schedule below cannot show in the result.
//
// The volume is cut into 8x8x8 bricks; only bricks that hold a mask voxel get storage (a slot): 512 doubles and 512 labels.  In
// that storage a voxel outside the mask (or outside the volume) holds -1, an unreached one +inf: membership and value are one
// 8-byte word, so a halo voxel is one load.
//   k_geo_mark     the mask as a flat byte string in aligned 16-byte words: counts the mask voxels, marks their bricks
//   k_geo_slots    numbers the marked bricks (brick -> slot grid, slot -> brick list)
//   k_geo_init     one workgroup per slot: -1 / +inf and "no label"
//   k_geo_check    one thread per seed: counts seeds outside the volume or the mask and labels outside 1..max_label
//   k_geo_seed     one thread per seed: D = 0, atomicMin of the label; its brick and the bricks that hold it in their halo are flagged
//   k_geo_list     compacts the flag array of this round into the list of active bricks and clears what it read
//   k_geo_relax<0> one workgroup per active brick: brick + one-voxel halo into LDS, Jacobi sweeps in LDS until nothing changes
//                  (at most MAX_SWEEPS: a brick that is not done flags itself), changed voxels stored; where a voxel of the
//                  outer shell changed, the bricks that see it are flagged for the next round
//   k_geo_relax<1> the same machinery over the labels once D is final: integer minimum over the tight predecessors
//   k_geo_scatter  bricks -> dense dist / labels, sizes by one atomic per distinct label among a wave's voxels
// Rounds are ordered by kernel boundaries only; the host reads one counter per round.  Within a round a halo load may race with
// the owning workgroup's store: both are single aligned 8-byte (4-byte) relaxed atomic accesses, stored values only decrease and
// each is the fl-sum along a real path (>= D), and a workgroup that changed a shell voxel flags every brick that reads it, so the
// reader runs again after the kernel boundary: the terminal state satisfies every constraint (<= D).  The flags of round r + 1
// live in another array than those that round r's list kernel clears.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"

namespace {

constexpr int TPB = 256;
constexpr int BRICK = 512;                         // voxels of a brick = threads of a brick's workgroup
constexpr int HALO = 1000;                         // 10^3: the brick and its one-voxel halo
constexpr int MAX_SWEEPS = 32;                     // inner sweeps of one brick in one round
constexpr int GRID_CAP = 65535 * 16;
constexpr int32_t FREE = -1, OCCUPIED = -2;        // in the brick -> slot grid before the slots are numbered
constexpr int32_t NO_LABEL = 0x7fffffff;
constexpr int64_t MAX_ROUNDS = (int64_t)1 << 26;
constexpr int C_PITCH = 32;                        // every counter keeps 256 bytes to itself
enum { C_MASK, C_SLOTS, C_BAD, C_REACHED, C_LIST0, C_LIST1, C_N };

typedef unsigned long long u64;

struct Geo { int32_t n0, n1, n2, B0, B1, B2; };
struct Weights { double w[8]; };                   // [|d0| << 2 | |d1| << 1 | |d2|]

__device__ __forceinline__ void wave_add(u64* p, u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if (v && (threadIdx.x & 63u) == 0u) atomicAdd(p, v);
}

// brick index and position inside the brick of the voxel with linear index idx
__device__ __forceinline__ void locate(uint32_t idx, const Geo& g, uint32_t& brick, uint32_t& local) {
    const uint32_t r = idx / (uint32_t)g.n2, i2 = idx - r * (uint32_t)g.n2, i0 = r / (uint32_t)g.n1, i1 = r - i0 * (uint32_t)g.n1;
    brick = ((i0 >> 3) * (uint32_t)g.B1 + (i1 >> 3)) * (uint32_t)g.B2 + (i2 >> 3);
    local = ((i0 & 7u) << 6) | ((i1 & 7u) << 3) | (i2 & 7u);
}

// values that another workgroup may store while this one loads them: single relaxed accesses at device scope
__device__ __forceinline__ double ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the occupied bricks
// bit k of the result: byte k of the word is != 0
__device__ __forceinline__ uint32_t nz4(uint32_t w) {
    const uint32_t h = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return ((h >> 7) & 1u) | ((h >> 14) & 2u) | ((h >> 21) & 4u) | ((h >> 28) & 8u);
}

// word b of the aligned string covers voxels 16 b - lead .. + 15
__global__ void __launch_bounds__(TPB) k_geo_mark(const uint4* __restrict__ base, u64 nwords, uint32_t lead, u64 V, Geo g,
                                                  int32_t* __restrict__ grid, u64* __restrict__ ctr) {
    u64 n = 0;
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < nwords; b += (u64)gridDim.x * TPB) {
        const uint4 w = base[b];
        if (!(w.x | w.y | w.z | w.w)) continue;
        uint32_t m = nz4(w.x) | (nz4(w.y) << 4) | (nz4(w.z) << 8) | (nz4(w.w) << 12);
        const int64_t f0 = (int64_t)(16 * b) - (int64_t)lead, left = (int64_t)V - f0;    // (left >= 1)
        if (f0 < 0) m &= ~((1u << (uint32_t)(-f0)) - 1u);
        if (left < 16) m &= (1u << (uint32_t)left) - 1u;
        n += (u64)__popc(m);
        uint32_t last = 0xffffffffu;
        for (; m; m &= m - 1u) {
            uint32_t brick, local;
            locate((uint32_t)(f0 + (int64_t)(__ffs((int)m) - 1)), g, brick, local);
            if (brick != last) grid[brick] = OCCUPIED;
            last = brick;
        }
    }
    wave_add(&ctr[C_MASK * C_PITCH], n);
}

__global__ void __launch_bounds__(TPB) k_geo_slots(int32_t* __restrict__ grid, uint32_t nbricks, uint32_t cap, uint32_t* __restrict__ brick_of,
                                                   u64* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t b0 = blockIdx.x * TPB; b0 < nbricks; b0 += gridDim.x * TPB) {           // (the same trips in every lane of a wave)
        const uint32_t b = b0 + threadIdx.x;
        const bool has = b < nbricks && grid[b] == OCCUPIED;
        const u64 who = __ballot(has);
        if (!who) continue;
        u64 first = 0;
        if (lane == (uint32_t)(__ffsll((long long)who) - 1)) first = atomicAdd(&ctr[C_SLOTS * C_PITCH], (u64)__popcll(who));
        first = __shfl(first, __ffsll((long long)who) - 1, 64);
        const uint32_t slot = (uint32_t)first + (uint32_t)__popcll(who & ((1ull << lane) - 1ull));
        if (has && slot < cap) { grid[b] = (int32_t)slot; brick_of[slot] = b; }           // (slot < cap always: a brick holds a voxel)
    }
}

__global__ void __launch_bounds__(BRICK) k_geo_init(const uint8_t* __restrict__ mask, Geo g, const uint32_t* __restrict__ brick_of,
                                                    double* __restrict__ D, int32_t* __restrict__ Lab) {
    const uint32_t slot = blockIdx.x, t = threadIdx.x, b = brick_of[slot];
    const uint32_t b2 = b % (uint32_t)g.B2, r = b / (uint32_t)g.B2, b1 = r % (uint32_t)g.B1, b0 = r / (uint32_t)g.B1;
    const uint32_t i0 = b0 * 8u + (t >> 6), i1 = b1 * 8u + ((t >> 3) & 7u), i2 = b2 * 8u + (t & 7u);
    const bool in = i0 < (uint32_t)g.n0 && i1 < (uint32_t)g.n1 && i2 < (uint32_t)g.n2 && mask[((size_t)i0 * g.n1 + i1) * g.n2 + i2] != 0;
    D[(size_t)slot * BRICK + t] = in ? INFINITY : -1.0;
    if (Lab) Lab[(size_t)slot * BRICK + t] = NO_LABEL;
}

// ---- seeds
__global__ void __launch_bounds__(TPB) k_geo_check(const int64_t* __restrict__ seeds, const int32_t* __restrict__ seed_labels, u64 nseed,
                                                   const uint8_t* __restrict__ mask, u64 V, int64_t max_label, u64* __restrict__ ctr) {
    u64 wrong = 0;
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < nseed; e += (u64)gridDim.x * TPB) {
        const int64_t v = seeds[e], l = seed_labels ? (int64_t)seed_labels[e] : 1;
        wrong += v < 0 || (u64)v >= V || !mask[v] || l < 1 || l > max_label;
    }
    wave_add(&ctr[C_BAD * C_PITCH], wrong);
}

__global__ void __launch_bounds__(TPB) k_geo_seed(const int64_t* __restrict__ seeds, const int32_t* __restrict__ seed_labels, u64 nseed, Geo g,
                                                  const int32_t* __restrict__ grid, double* __restrict__ D, int32_t* __restrict__ Lab,
                                                  uint32_t* __restrict__ flag) {
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < nseed; e += (u64)gridDim.x * TPB) {
        uint32_t brick, local;
        locate((uint32_t)seeds[e], g, brick, local);
        const int32_t slot = grid[brick];
        if (slot < 0) continue;                                          // (cannot happen: the seed is a mask voxel)
        const size_t at = (size_t)slot * BRICK + local;
        D[at] = 0.0;
        if (Lab) atomicMin(&Lab[at], seed_labels ? seed_labels[e] : 1);
        // the seed's brick, and the bricks that hold the seed in their halo: no relaxation changes a seed, so nobody else flags them
        const uint32_t a = local >> 6, b = (local >> 3) & 7u, c = local & 7u;
        const int32_t b2 = (int32_t)(brick % (uint32_t)g.B2), r = (int32_t)(brick / (uint32_t)g.B2), b1 = r % g.B1, b0 = r / g.B1;
#pragma nounroll
        for (int x = -1; x <= 1; x++)
#pragma nounroll
            for (int y = -1; y <= 1; y++)
#pragma nounroll
                for (int z = -1; z <= 1; z++) {
                    if ((x < 0 && a != 0u) || (x > 0 && a != 7u) || (y < 0 && b != 0u) || (y > 0 && b != 7u) || (z < 0 && c != 0u) || (z > 0 && c != 7u)) continue;
                    const int32_t c0 = b0 + x, c1 = b1 + y, c2 = b2 + z;
                    if ((uint32_t)c0 >= (uint32_t)g.B0 || (uint32_t)c1 >= (uint32_t)g.B1 || (uint32_t)c2 >= (uint32_t)g.B2) continue;
                    const int32_t s = grid[((size_t)c0 * g.B1 + c1) * g.B2 + c2];
                    if (s >= 0) flag[s] = 1u;
                }
    }
}

// ---- one round
__global__ void __launch_bounds__(TPB) k_geo_list(uint32_t* __restrict__ flag, uint32_t nslots, uint32_t* __restrict__ list,
                                                  u64* __restrict__ cursor, u64* __restrict__ next_cursor) {
    const uint32_t lane = threadIdx.x & 63u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *next_cursor = 0;
    for (uint32_t s0 = blockIdx.x * TPB; s0 < nslots; s0 += gridDim.x * TPB) {            // (the same trips in every lane of a wave)
        const uint32_t s = s0 + threadIdx.x;
        const bool has = s < nslots && flag[s] != 0u;
        const u64 who = __ballot(has);
        if (!who) continue;
        u64 first = 0;
        if (lane == (uint32_t)(__ffsll((long long)who) - 1)) first = atomicAdd(cursor, (u64)__popcll(who));
        first = __shfl(first, __ffsll((long long)who) - 1, 64);
        if (has) { list[(uint32_t)first + (uint32_t)__popcll(who & ((1ull << lane) - 1ull))] = s; flag[s] = 0u; }
    }
}

// LABELS == 0: D, LABELS == 1: the labels over the final D.  One workgroup of BRICK threads per entry of list.
template <int LABELS>
__global__ void __launch_bounds__(BRICK) k_geo_relax(const uint32_t* __restrict__ list, const uint32_t* __restrict__ brick_of,
                                                     const int32_t* __restrict__ grid, Geo g, Weights wt, double* D, int32_t* Lab,
                                                     uint32_t* __restrict__ flag_next) {
    __shared__ double sD[HALO];
    __shared__ int32_t sL[LABELS ? HALO : 1];
    __shared__ int32_t nslot[27];                                       // the slots of the 27 bricks around (13: this one), -1: none
    __shared__ uint32_t mark[27];                                       // a voxel that the brick in that direction reads has changed
    const uint32_t t = threadIdx.x, slot = list[blockIdx.x], b = brick_of[slot];
    const int32_t b2 = (int32_t)(b % (uint32_t)g.B2), r = (int32_t)(b / (uint32_t)g.B2), b1 = r % g.B1, b0 = r / g.B1;
    if (t < 27u) {
        const int32_t c0 = b0 + (int32_t)(t / 9u) - 1, c1 = b1 + (int32_t)((t / 3u) % 3u) - 1, c2 = b2 + (int32_t)(t % 3u) - 1;
        const bool in = (uint32_t)c0 < (uint32_t)g.B0 && (uint32_t)c1 < (uint32_t)g.B1 && (uint32_t)c2 < (uint32_t)g.B2;
        nslot[t] = in ? grid[((size_t)c0 * g.B1 + c1) * g.B2 + c2] : -1;
        mark[t] = 0u;
    }
    __syncthreads();
    for (uint32_t q = t; q < (uint32_t)HALO; q += BRICK) {
        const int32_t la = (int32_t)(q / 100u), rem = (int32_t)(q - (uint32_t)la * 100u), lb = rem / 10, lc = rem - lb * 10;
        const int32_t ga = la - 1, gb = lb - 1, gc = lc - 1;            // -1 .. 8 relative to the brick
        const int32_t s = nslot[((ga < 0 ? 0 : ga > 7 ? 2 : 1) * 3 + (gb < 0 ? 0 : gb > 7 ? 2 : 1)) * 3 + (gc < 0 ? 0 : gc > 7 ? 2 : 1)];
        double v = INFINITY;
        int32_t l = NO_LABEL;
        if (s >= 0) {
            const size_t at = (size_t)s * BRICK + (size_t)(((ga & 7) << 6) | ((gb & 7) << 3) | (gc & 7));
            const double d = ld(D + at);
            if (d >= 0.0) { v = d; if (LABELS) l = ld(Lab + at); }
        }
        sD[q] = v;
        if (LABELS) sL[q] = l;
    }
    const uint32_t a = t >> 6, bb = (t >> 3) & 7u, c = t & 7u;
    const int32_t me = (int32_t)((a + 1u) * 100u + (bb + 1u) * 10u + (c + 1u));
    const size_t mine = (size_t)slot * BRICK + t;
    const double d0 = D[mine];                                          // (only this workgroup stores to its brick)
    __syncthreads();
    bool changed = false, any = false;
    if constexpr (LABELS == 0) {
        const bool in = d0 >= 0.0;
        double cur = in ? d0 : INFINITY;
        for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
            double best = cur;
            if (in) {
#pragma unroll
                for (int x = -1; x <= 1; x++)
#pragma unroll
                    for (int y = -1; y <= 1; y++)
#pragma unroll
                        for (int z = -1; z <= 1; z++) {
                            if (!x && !y && !z) continue;
                            const double cand = sD[me + x * 100 + y * 10 + z] + wt.w[((x != 0) << 2) | ((y != 0) << 1) | (z != 0)];
                            best = cand < best ? cand : best;
                        }
            }
            const bool better = best < cur;
            any = __syncthreads_or(better) != 0;                        // (every load of this sweep is behind it)
            if (better) { cur = best; sD[me] = best; }
            __syncthreads();
            if (!any) break;
        }
        changed = in && cur < d0;
        if (changed) st(D + mine, cur);
    } else {
        const bool in = d0 >= 0.0 && d0 < INFINITY;
        uint32_t tight = 0u;                                            // the neighbours u with fl(D(u) + w) == D(v)
        if (in) {
            int j = 0;
#pragma unroll
            for (int x = -1; x <= 1; x++)
#pragma unroll
                for (int y = -1; y <= 1; y++)
#pragma unroll
                    for (int z = -1; z <= 1; z++, j++) {
                        if (!x && !y && !z) continue;
                        if (sD[me + x * 100 + y * 10 + z] + wt.w[((x != 0) << 2) | ((y != 0) << 1) | (z != 0)] == d0) tight |= 1u << j;
                    }
        }
        const int32_t l0 = Lab[mine];
        int32_t cur = l0;
        for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
            int32_t best = cur;
            int j = 0;
#pragma unroll
            for (int x = -1; x <= 1; x++)
#pragma unroll
                for (int y = -1; y <= 1; y++)
#pragma unroll
                    for (int z = -1; z <= 1; z++, j++) {
                        if (!x && !y && !z) continue;
                        if (tight & (1u << j)) best = min(best, sL[me + x * 100 + y * 10 + z]);
                    }
            const bool better = best < cur;
            any = __syncthreads_or(better) != 0;
            if (better) { cur = best; sL[me] = best; }
            __syncthreads();
            if (!any) break;
        }
        changed = cur < l0;
        if (changed) st(Lab + mine, cur);
    }
    if (changed) {                                                      // the bricks that hold this voxel in their halo
#pragma unroll
        for (int x = -1; x <= 1; x++)
#pragma unroll
            for (int y = -1; y <= 1; y++)
#pragma unroll
                for (int z = -1; z <= 1; z++) {
                    if (!x && !y && !z) continue;
                    if ((x < 0 && a != 0u) || (x > 0 && a != 7u) || (y < 0 && bb != 0u) || (y > 0 && bb != 7u) || (z < 0 && c != 0u) || (z > 0 && c != 7u)) continue;
                    mark[(x + 1) * 9 + (y + 1) * 3 + (z + 1)] = 1u;
                }
    }
    __syncthreads();
    if (t < 27u && t != 13u && mark[t] && nslot[t] >= 0) flag_next[nslot[t]] = 1u;
    if (t == 13u && any) flag_next[slot] = 1u;                          // the sweeps ran out: this brick goes on in the next round
}

// ---- bricks -> dense volumes
__global__ void __launch_bounds__(TPB) k_geo_scatter(Geo g, u64 V, const int32_t* __restrict__ grid, const double* __restrict__ D,
                                                     const int32_t* __restrict__ Lab, double* __restrict__ dist, int32_t* __restrict__ labels,
                                                     u64* __restrict__ cnt, u64* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    u64 reached = 0;
    for (u64 i0 = (u64)blockIdx.x * TPB; i0 < V; i0 += (u64)gridDim.x * TPB) {            // (the same trips in every lane of a wave)
        const u64 idx = i0 + threadIdx.x;
        double d = -1.0;
        int32_t l = 0;
        if (idx < V) {
            uint32_t brick, local;
            locate((uint32_t)idx, g, brick, local);
            const int32_t slot = grid[brick];
            if (slot >= 0) {
                const size_t at = (size_t)slot * BRICK + local;
                d = D[at];
                if (Lab && d >= 0.0) { l = Lab[at]; if (l == NO_LABEL) l = 0; }
            }
            if (dist) dist[idx] = d;
            if (labels) labels[idx] = l;
        }
        const bool in = d >= 0.0;
        reached += in && d < INFINITY;
        if (!cnt) continue;
        u64 todo = __ballot(in);                                        // one atomic per label among the wave's 64 voxels
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int32_t ll = __shfl(l, lead, 64);
            const u64 same = __ballot(in && l == ll);
            if ((int)lane == lead) atomicAdd(&cnt[ll], (u64)__popcll(same));
            todo &= ~same;
        }
    }
    wave_add(&ctr[C_REACHED * C_PITCH], reached);
}

int grid_for(u64 items, u64 cap) { return (int)std::max<u64>(1, std::min<u64>(cap, items)); }

struct Bricks {                                                         // (names only: the call's DevMem owns them)
    u64* ctr = nullptr; int32_t* grid = nullptr; uint32_t* brick_of = nullptr; double* D = nullptr; int32_t* Lab = nullptr;
    uint32_t* flag = nullptr; uint32_t* list = nullptr;
};

// the fixed point of one kind: rounds until no brick is flagged; flags of the first round are in flag[0 .. nslots)
template <int LABELS>
int iterate(const Bricks& b, uint32_t nslots, const Geo& g, const Weights& wt, int64_t& rounds) {
    const int glist = grid_for(((u64)nslots + TPB - 1) / TPB, 1024);
    int cur = 0;
    for (rounds = 0;; rounds++) {
        if (rounds == MAX_ROUNDS) { vmask::set_error("the relaxation did not finish"); return VRG_E_INTERNAL; }
        u64* cursor = b.ctr + (size_t)(C_LIST0 + (int)(rounds & 1)) * C_PITCH;
        u64* other = b.ctr + (size_t)(C_LIST0 + (int)((rounds + 1) & 1)) * C_PITCH;
        k_geo_list<<<glist, TPB>>>(b.flag + (size_t)cur * nslots, nslots, b.list, cursor, other);
        u64 active = 0;
        VMASK_TRY(hipMemcpy(&active, cursor, sizeof(u64), hipMemcpyDeviceToHost));
        if (!active) break;
        k_geo_relax<LABELS><<<(uint32_t)active, BRICK>>>(b.list, b.brick_of, b.grid, g, wt, b.D, b.Lab, b.flag + (size_t)(cur ^ 1) * nslots);
        cur ^= 1;
    }
    VMASK_TRY(hipGetLastError());
    return VRG_OK;
}

int geodesic(const uint8_t* mask, Geo g, const int64_t* seeds, const int32_t* seed_labels, int64_t nseed, const Weights& wt,
             double* dist, int32_t* labels, int64_t* sizes, int64_t max_label, int64_t* counts) {
    const u64 V = (u64)g.n0 * g.n1 * g.n2;
    const uint32_t nbricks = (uint32_t)g.B0 * (uint32_t)g.B1 * (uint32_t)g.B2;
    const bool want_labels = labels || sizes;
    DevMem mem;
    Bricks b;
    const uint8_t* dmask; const int64_t* dseeds = nullptr; const int32_t* dseed_labels = nullptr;
    int rc = bring(mem, mask, V, "mask", &dmask);
    if (!rc && nseed) rc = bring(mem, seeds, (size_t)nseed, "seeds", &dseeds);
    if (!rc && nseed && seed_labels) rc = bring(mem, seed_labels, (size_t)nseed, "seed labels", &dseed_labels);
    if (rc) return rc;
    const size_t nctr = (size_t)C_N * C_PITCH + (size_t)max_label + 1;   // the counters, then sizes
    VMASK_GRAB(b.ctr, nctr, "counters");
    VMASK_TRY(hipMemsetAsync(b.ctr, 0, nctr * sizeof(u64), 0));
    u64* cnt = b.ctr + (size_t)C_N * C_PITCH;
    if (nseed) {
        k_geo_check<<<grid_for(((u64)nseed + TPB - 1) / TPB, 1024), TPB>>>(dseeds, dseed_labels, (u64)nseed, dmask, V, max_label, b.ctr);
        u64 bad = 0;
        VMASK_TRY(hipMemcpy(&bad, b.ctr + (size_t)C_BAD * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
        if (bad) { vmask::set_error(std::to_string(bad) + " seeds outside the volume or the mask, or with a label outside 1..max_label"); return VRG_E_ARG; }
    }
    // the occupied bricks
    VMASK_GRAB(b.grid, nbricks, "brick grid");
    VMASK_TRY(hipMemsetAsync(b.grid, 0xff, (size_t)nbricks * sizeof(int32_t), 0));            // FREE
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(dmask) & 15u);
    const u64 nwords = (lead + V + 15u) / 16u;
    k_geo_mark<<<grid_for((nwords + TPB - 1) / TPB, GRID_CAP), TPB>>>(reinterpret_cast<const uint4*>(dmask - lead), nwords, lead, V, g, b.grid, b.ctr);
    u64 nmask = 0;
    VMASK_TRY(hipMemcpy(&nmask, b.ctr + (size_t)C_MASK * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
    const uint32_t cap = (uint32_t)std::min<u64>(nmask, nbricks);
    VMASK_GRAB(b.brick_of, cap, "brick list");
    k_geo_slots<<<grid_for(((u64)nbricks + TPB - 1) / TPB, GRID_CAP), TPB>>>(b.grid, nbricks, cap, b.brick_of, b.ctr);
    u64 found = 0;
    VMASK_TRY(hipMemcpy(&found, b.ctr + (size_t)C_SLOTS * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
    if (found > cap) { vmask::set_error("more occupied bricks than mask voxels"); return VRG_E_INTERNAL; }
    const uint32_t nslots = (uint32_t)found;
    int64_t rounds[2] = {0, 0};
    if (nslots) {
        VMASK_GRAB(b.D, (size_t)nslots * BRICK, "brick distances");
        if (want_labels) VMASK_GRAB(b.Lab, (size_t)nslots * BRICK, "brick labels");
        VMASK_GRAB(b.flag, (size_t)2 * nslots, "brick flags");
        VMASK_GRAB(b.list, nslots, "active bricks");
        VMASK_TRY(hipMemsetAsync(b.flag, 0, (size_t)2 * nslots * sizeof(uint32_t), 0));
        k_geo_init<<<nslots, BRICK>>>(dmask, g, b.brick_of, b.D, b.Lab);
        if (nseed) {
            k_geo_seed<<<grid_for(((u64)nseed + TPB - 1) / TPB, 1024), TPB>>>(dseeds, dseed_labels, (u64)nseed, g, b.grid, b.D, b.Lab, b.flag);
            rc = iterate<0>(b, nslots, g, wt, rounds[0]);
            if (rc) return rc;
            if (want_labels) {                                          // D is final: every brick looks at its labels once, then as flagged
                VMASK_TRY(hipMemsetAsync(b.flag, 0, (size_t)2 * nslots * sizeof(uint32_t), 0));
                VMASK_TRY(hipMemsetAsync(b.flag, 1, (size_t)nslots * sizeof(uint32_t), 0));      // (0x01010101: not 0)
                rc = iterate<1>(b, nslots, g, wt, rounds[1]);
                if (rc) return rc;
            }
        }
    }
    Out<double> odist; Out<int32_t> olab;                               // (both optional: one that is never opened keeps a null dev)
    if ((dist && (rc = odist.open(mem, dist, V, "dist"))) || (labels && (rc = olab.open(mem, labels, V, "labels")))) return rc;
    k_geo_scatter<<<grid_for((V + TPB - 1) / TPB, GRID_CAP), TPB>>>(g, V, b.grid, b.D, b.Lab, odist.dev, olab.dev, sizes ? cnt : nullptr, b.ctr);
    VMASK_TRY(hipGetLastError());
    u64 reached = 0;
    VMASK_TRY(hipMemcpy(&reached, b.ctr + (size_t)C_REACHED * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
    if ((rc = odist.close()) || (rc = olab.close())) return rc;
    if (sizes) VMASK_TRY(hipMemcpy(sizes, cnt, ((size_t)max_label + 1) * sizeof(int64_t), vmask::is_device_pointer(sizes) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (counts) {
        const int64_t out[5] = {(int64_t)nmask, (int64_t)reached, (int64_t)nslots, rounds[0], rounds[1]};
        rc = put(counts, out, 5);
        if (rc) return rc;
    }
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_geodesic(int device, const uint8_t* mask, int64_t n0, int64_t n1, int64_t n2,
                              const int64_t* seeds, const int32_t* seed_labels, int64_t nseed, const double* spacing,
                              double* dist, int32_t* labels, int64_t* sizes, int64_t max_label, int64_t* counts) {
    if (!mask || (nseed && !seeds)) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nseed < 0 || max_label < 0 || max_label >= 0x7fffffff) { vmask::set_error("seed count or max_label out of range"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    double h[3] = {1.0, 1.0, 1.0};
    if (spacing) {
        if (vmask::is_device_pointer(spacing)) VMASK_TRY(hipMemcpy(h, spacing, sizeof(h), hipMemcpyDeviceToHost));
        else std::copy(spacing, spacing + 3, h);
    }
    for (double x : h)
        if (!std::isfinite(x) || !(x > 0.0)) { vmask::set_error("spacing not finite and positive"); return VRG_E_ARG; }
    if (std::max({h[0], h[1], h[2]}) / std::min({h[0], h[1], h[2]}) > 1000.0) { vmask::set_error("spacing ratio above 1000"); return VRG_E_ARG; }
    Weights wt;
    for (int k = 0; k < 8; k++) {                                       // float64, summed in the order of the axes
        const double x = (k & 4) ? h[0] : 0.0, y = (k & 2) ? h[1] : 0.0, z = (k & 1) ? h[2] : 0.0;
        volatile double xx = x * x, yy = y * y, zz = z * z;             // (each product rounded on its own: no fused multiply-add)
        volatile double s = xx + yy;
        wt.w[k] = std::sqrt(s + zz);
    }
    Geo g;
    g.n0 = (int32_t)n0; g.n1 = (int32_t)n1; g.n2 = (int32_t)n2;
    g.B0 = (g.n0 + 7) / 8; g.B1 = (g.n1 + 7) / 8; g.B2 = (g.n2 + 7) / 8;
    return geodesic(mask, g, seeds, seed_labels, nseed, wt, dist, labels, sizes, max_label, counts);
}
