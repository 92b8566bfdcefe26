// vbrick.h - the sparse brick store that the floods inside a mask share: vgeo_device.hip (geodesic distance and labels) and
// vbridge_device.hip (cost flood, roots and contacts).  Everything has internal linkage.
//
// The volume is cut into 8x8x8 bricks; only the bricks that a client marks OCCUPIED in the brick -> slot grid get storage (a
// slot): 512 doubles D and whatever else the client keeps per voxel.  In D a voxel outside the client's domain (or outside the
// volume) holds -1, an unreached one +inf: membership and value are one 8-byte word, so a halo voxel is one load.
//   k_brick_slots  numbers the occupied bricks (brick -> slot grid, slot -> brick list): ballot + one atomic per wave; the
//                  numbering is not deterministic and cannot show in a client's output
//   k_brick_list   compacts the flag array of this round into the list of active bricks and clears what it read
// A client's round kernel runs one workgroup of BRICK threads per active brick: load_halo brings the brick and its one-voxel halo
// into LDS, the client sweeps there until nothing changes (at most MAX_SWEEPS: a brick that is not done flags itself) and stores
// the changed voxels, mark_readers flags the bricks that see a changed voxel of the outer shell for the next round.  iterate
// repeats list + round kernel until no brick is flagged.
//
// THE HAND-OFF.  Rounds are ordered by kernel boundaries only; the host reads one counter per round.  Within a round a halo load
// may race with the owning workgroup's store: both are single aligned 8-byte (4-byte) relaxed atomic accesses (ld / st below),
// and only the owning workgroup stores to a brick.  A client's update has to meet two conditions:
//   (1) stored values only decrease;
//   (2) every stored value is attained along a real path (for D: the fl-sum along it), so it is never below the fixed point.
// Then a racing load sees either the old or the new value, both >= the fixed point, and a workgroup that changed a shell voxel
// flags every brick that reads it, so the reader runs again after the kernel boundary: when no flag is left, every voxel
// satisfies every constraint (<= the fixed point), and with (2) equals it.  The flags of round r + 1 live in another array than
// those that round r's list kernel clears, so a flag raised while the list kernel runs is never lost.
//
// Nothing here multiplies and adds floating-point values: the header means the same with and without fp contraction.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vmask_wave.h"

namespace {

constexpr int TPB = 256;
constexpr int BRICK = 512;                         // voxels of a brick = threads of a brick's workgroup
constexpr int HALO = 1000;                         // 10^3: the brick and its one-voxel halo
constexpr int MAX_SWEEPS = 32;                     // inner sweeps of one brick in one round
constexpr int GRID_CAP = 65535 * 16;
constexpr int32_t FREE = -1, OCCUPIED = -2;        // in the brick -> slot grid before the slots are numbered
constexpr int32_t NO_VALUE = 0x7fffffff;           // an int32 field (label, root) that no path has reached
constexpr int64_t MAX_ROUNDS = (int64_t)1 << 26;

struct Geo { int32_t n0, n1, n2, B0, B1, B2; };
inline Geo make_geo(int64_t n0, int64_t n1, int64_t n2) {
    Geo g;
    g.n0 = (int32_t)n0; g.n1 = (int32_t)n1; g.n2 = (int32_t)n2;
    g.B0 = (g.n0 + 7) / 8; g.B1 = (g.n1 + 7) / 8; g.B2 = (g.n2 + 7) / 8;
    return g;
}
struct Brick3 { int32_t b0, b1, b2; };

inline int grid_for(u64 items, u64 cap) { return (int)std::max<u64>(1, std::min<u64>(cap, items)); }

// brick index and position inside the brick of the voxel with linear index idx
__device__ __forceinline__ void locate(uint32_t idx, const Geo& g, uint32_t& brick, uint32_t& local) {
    const uint32_t r = idx / (uint32_t)g.n2, i2 = idx - r * (uint32_t)g.n2, i0 = r / (uint32_t)g.n1, i1 = r - i0 * (uint32_t)g.n1;
    brick = ((i0 >> 3) * (uint32_t)g.B1 + (i1 >> 3)) * (uint32_t)g.B2 + (i2 >> 3);
    local = ((i0 & 7u) << 6) | ((i1 & 7u) << 3) | (i2 & 7u);
}
// the place of brick b on the brick grid
__device__ __forceinline__ Brick3 brick_coords(uint32_t b, const Geo& g) {
    const uint32_t r = b / (uint32_t)g.B2;
    return {(int32_t)(r / (uint32_t)g.B1), (int32_t)(r % (uint32_t)g.B1), (int32_t)(b % (uint32_t)g.B2)};
}
// thread t's voxel in the 10^3 LDS image of its brick and halo
__device__ __forceinline__ int32_t halo_at(uint32_t t) { return (int32_t)(((t >> 6) + 1u) * 100u + (((t >> 3) & 7u) + 1u) * 10u + ((t & 7u) + 1u)); }

// values that another workgroup may store while this one loads them: single relaxed accesses at device scope
__device__ __forceinline__ double ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the bricks with storage, the bricks of one round
// cap: the entries of brick_of
__global__ void __launch_bounds__(TPB) k_brick_slots(int32_t* __restrict__ grid, uint32_t nbricks, uint32_t cap, uint32_t* __restrict__ brick_of,
                                                     u64* __restrict__ counter) {
    const uint32_t lane = lane_id();
    for (uint32_t b0 = blockIdx.x * TPB; b0 < nbricks; b0 += gridDim.x * TPB) {           // (the same trips in every lane of a wave)
        const uint32_t b = b0 + threadIdx.x;
        const bool has = b < nbricks && grid[b] == OCCUPIED;
        const u64 who = __ballot(has);
        if (!who) continue;
        u64 first = 0;
        if (lane == (uint32_t)(__ffsll((long long)who) - 1)) first = atomicAdd(counter, (u64)__popcll(who));
        first = __shfl(first, __ffsll((long long)who) - 1, 64);
        const uint32_t slot = (uint32_t)first + (uint32_t)__popcll(who & ((1ull << lane) - 1ull));
        if (has && slot < cap) { grid[b] = (int32_t)slot; brick_of[slot] = b; }           // (slot < cap always: number_bricks checks the count)
    }
}

__global__ void __launch_bounds__(TPB) k_brick_list(uint32_t* __restrict__ flag, uint32_t nslots, uint32_t* __restrict__ list,
                                                    u64* __restrict__ cursor, u64* __restrict__ next_cursor) {
    const uint32_t lane = lane_id();
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

// ---- inside a workgroup of BRICK threads that holds brick b
// What every brick kernel starts with: the slots of the 27 bricks around (13: this one, -1: none) into nslot[27], then the brick
// and its halo into LDS: D (+inf outside the domain), with COST the cost (1 there), with FIELD an int32 field (`none` there).
// What the caller stored to LDS before is visible after it; it ends behind a barrier.
template <bool COST, bool FIELD>
__device__ __forceinline__ void load_halo(uint32_t b, const Geo& g, const int32_t* __restrict__ grid, const double* D, const double* __restrict__ Cst,
                                          const int32_t* F, int32_t none, double* sD, double* sC, int32_t* sF, int32_t* nslot) {
    const uint32_t t = threadIdx.x;
    if (t < 27u) {
        const Brick3 at = brick_coords(b, g);
        const int32_t c0 = at.b0 + (int32_t)(t / 9u) - 1, c1 = at.b1 + (int32_t)((t / 3u) % 3u) - 1, c2 = at.b2 + (int32_t)(t % 3u) - 1;
        const bool in = (uint32_t)c0 < (uint32_t)g.B0 && (uint32_t)c1 < (uint32_t)g.B1 && (uint32_t)c2 < (uint32_t)g.B2;
        nslot[t] = in ? grid[((size_t)c0 * g.B1 + c1) * g.B2 + c2] : -1;
    }
    __syncthreads();
    for (uint32_t q = t; q < (uint32_t)HALO; q += BRICK) {
        const int32_t la = (int32_t)(q / 100u), rem = (int32_t)(q - (uint32_t)la * 100u), lb = rem / 10, lc = rem - lb * 10;
        const int32_t ga = la - 1, gb = lb - 1, gc = lc - 1;            // -1 .. 8 relative to the brick
        const int32_t s = nslot[((ga < 0 ? 0 : ga > 7 ? 2 : 1) * 3 + (gb < 0 ? 0 : gb > 7 ? 2 : 1)) * 3 + (gc < 0 ? 0 : gc > 7 ? 2 : 1)];
        double v = INFINITY, c = 1.0;
        int32_t f = none;
        if (s >= 0) {
            const size_t at = (size_t)s * BRICK + (size_t)(((ga & 7) << 6) | ((gb & 7) << 3) | (gc & 7));
            const double d = ld(D + at);
            if (d >= 0.0) {
                v = d;
                if constexpr (COST) c = Cst[at];
                if constexpr (FIELD) f = ld(F + at);
            }
        }
        sD[q] = v;
        if constexpr (COST) sC[q] = c;
        if constexpr (FIELD) sF[q] = f;
    }
    __syncthreads();
}

// does the brick at (x, y, z) in -1..1 from this one hold this brick's voxel (a, b, c) in its halo (or, at 0 0 0, in itself)
__device__ __forceinline__ bool reads(int x, int y, int z, uint32_t a, uint32_t b, uint32_t c) {
    return !((x < 0 && a != 0u) || (x > 0 && a != 7u) || (y < 0 && b != 0u) || (y > 0 && b != 7u) || (z < 0 && c != 0u) || (z > 0 && c != 7u));
}

// How every round kernel ends: a thread whose voxel changed marks the bricks that read it (mark[27], zeroed before load_halo);
// every marked brick with storage is flagged for the next round, and this brick too if its sweeps ran out (any).
__device__ __forceinline__ void mark_readers(bool changed, bool any, uint32_t slot, const int32_t* nslot, uint32_t* mark, uint32_t* __restrict__ flag_next) {
    const uint32_t t = threadIdx.x, a = t >> 6, b = (t >> 3) & 7u, c = t & 7u;
    if (changed) {
#pragma unroll
        for (int x = -1; x <= 1; x++)
#pragma unroll
            for (int y = -1; y <= 1; y++)
#pragma unroll
                for (int z = -1; z <= 1; z++) {
                    if (!x && !y && !z) continue;
                    if (reads(x, y, z, a, b, c)) mark[(x + 1) * 9 + (y + 1) * 3 + (z + 1)] = 1u;
                }
    }
    __syncthreads();
    if (t < 27u && t != 13u && mark[t] && nslot[t] >= 0) flag_next[nslot[t]] = 1u;
    if (t == 13u && any) flag_next[slot] = 1u;
}

// The integer-minimum fixed point inside a brick: the voxel's value = the smallest of its own and those of its tight
// predecessors, bit k of `tight` = the neighbour with code k (0..25: the lexicographic order of the offsets, the centre left
// out).  sL: the field with its halo, me: halo_at(thread).  Returns the voxel's value; any: the sweeps ran out.
__device__ __forceinline__ int32_t min_over_tight(uint32_t tight, int32_t cur, int32_t* sL, int32_t me, bool& any) {
    any = false;
    for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
        int32_t best = cur;
        int k = 0;
#pragma unroll
        for (int x = -1; x <= 1; x++)
#pragma unroll
            for (int y = -1; y <= 1; y++)
#pragma unroll
                for (int z = -1; z <= 1; z++) {
                    if (!x && !y && !z) continue;
                    if (tight & (1u << k)) best = min(best, sL[me + x * 100 + y * 10 + z]);
                    k++;
                }
        const bool better = best < cur;
        any = __syncthreads_or(better) != 0;                            // (every load of this sweep is behind it)
        if (better) { cur = best; sL[me] = best; }
        __syncthreads();
        if (!any) break;
    }
    return cur;
}

// ---- host
// numbers the OCCUPIED bricks of grid; cap: the entries of brick_of, `what`: the error if there are more
inline int number_bricks(int32_t* grid, uint32_t nbricks, uint32_t cap, uint32_t* brick_of, u64* counter, const char* what, uint32_t& nslots) {
    k_brick_slots<<<grid_for(((u64)nbricks + TPB - 1) / TPB, GRID_CAP), TPB>>>(grid, nbricks, cap, brick_of, counter);
    u64 found = 0;
    VMASK_TRY(hipMemcpy(&found, counter, sizeof(u64), hipMemcpyDeviceToHost));
    if (found > cap) { vmask::set_error(what); return VRG_E_INTERNAL; }
    nslots = (uint32_t)found;
    return VRG_OK;
}

// the fixed point of one kind: rounds until no brick is flagged.  flag: two arrays of nslots, the flags of the first round in
// the first; counters: the two list cursors, C_PITCH apart; launch(list, active, flag_next): the client's round kernel
template <class Launch>
int iterate(uint32_t* flag, uint32_t* list, u64* counters, uint32_t nslots, int64_t& rounds, Launch launch) {
    const int glist = grid_for(((u64)nslots + TPB - 1) / TPB, 1024);
    int cur = 0;
    for (rounds = 0;; rounds++) {
        if (rounds == MAX_ROUNDS) { vmask::set_error("the relaxation did not finish"); return VRG_E_INTERNAL; }
        u64* cursor = counters + c_at((int)(rounds & 1));
        u64* other = counters + c_at((int)((rounds + 1) & 1));
        k_brick_list<<<glist, TPB>>>(flag + (size_t)cur * nslots, nslots, list, cursor, other);
        u64 active = 0;
        VMASK_TRY(hipMemcpy(&active, cursor, sizeof(u64), hipMemcpyDeviceToHost));
        if (!active) break;
        launch(list, (uint32_t)active, flag + (size_t)(cur ^ 1) * nslots);
        cur ^= 1;
    }
    VMASK_TRY(hipGetLastError());
    return VRG_OK;
}

}  // namespace
