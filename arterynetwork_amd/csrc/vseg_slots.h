// vseg_slots.h - what the passes over the compacted object voxels ("slots") share: vseg_device.hip (segment tracing) and
// vbr_device.hip (branch graph).  The volume is read as a flat byte string in aligned 16-byte words, its object voxels are
// counted, listed (one atomic per wave) and entered idx -> slot into an open-addressing hash table; the 27-bit neighbourhood
// numbering of those translation units (wave helpers and the word read: vmask_wave.h, host-side helpers: vmask_host.h).
// Everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vmask_wave.h"

namespace {

constexpr int TPB = 256;
constexpr int GRID_VOLUME = 2048;                  // blocks, at most, of the two kernels that read the volume (16 bytes per thread and turn)
constexpr int GRID_LIST = 256;                     // blocks, at most, of the kernels over slots, darts and segment heads

struct Dim { int32_t n0, n1, n2; };

constexpr uint32_t NONE = 0xffffffffu;

// ---- idx -> slot: open addressing, linear probing, at most half full; entry = idx << 32 | slot
struct Hash { u64* tab; uint32_t mask, shift; };
constexpr u64 H_EMPTY = ~0ull;
__device__ __forceinline__ uint32_t h_home(const Hash& h, uint32_t key) { return (key * 2654435761u) >> h.shift; }
__device__ __forceinline__ void h_insert(const Hash& h, uint32_t key, uint32_t slot) {
    uint32_t p = h_home(h, key);
    for (uint32_t tries = 0; tries <= h.mask; tries++, p = (p + 1u) & h.mask)
        if (atomicCAS(&h.tab[p], H_EMPTY, ((u64)key << 32) | slot) == H_EMPTY) return;
}
__device__ __forceinline__ uint32_t h_find(const Hash& h, uint32_t key) {
    uint32_t p = h_home(h, key);
    for (uint32_t tries = 0; tries <= h.mask; tries++, p = (p + 1u) & h.mask) {
        const u64 e = h.tab[p];
        if ((uint32_t)(e >> 32) == key) return (uint32_t)e;
        if (e == H_EMPTY) break;
    }
    return NONE;
}
// the table's geometry for n object voxels (n >= 1): 2^bits entries, at least 2 n
inline int hash_bits(uint32_t n) {
    int bits = 4;
    while ((1ull << bits) < 2ull * n) bits++;
    return bits;
}

// ---- the object voxels, counted and listed
__global__ void __launch_bounds__(TPB) k_seg_count(const uint4* __restrict__ base, u64 nwords, uint32_t lead, u64 V, u64* __restrict__ c_obj) {
    u64 n = 0;
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < nwords; b += (u64)gridDim.x * TPB) n += (u64)__popc(word_mask(base, b, lead, V));
    wave_add(c_obj, n);
}

__global__ void __launch_bounds__(TPB) k_seg_compact(const uint4* __restrict__ base, u64 nwords, uint32_t lead, u64 V, uint32_t nobj,
                                                     uint32_t* __restrict__ list, Hash h, u64* __restrict__ cursor) {
    for (u64 b0 = (u64)blockIdx.x * TPB; b0 < nwords; b0 += (u64)gridDim.x * TPB) {      // (the same trips in every lane of a wave)
        const u64 b = b0 + threadIdx.x;
        uint32_t m = b < nwords ? word_mask(base, b, lead, V) : 0u;
        if (!__ballot(m != 0u)) continue;
        uint32_t total;
        const uint32_t off = wave_scan((uint32_t)__popc(m), total);
        u64 slot = wave_reserve(cursor, total) + off;
        const uint32_t first = (uint32_t)(16 * b - lead);                                  // (used only where a bit of m is set)
        for (; m; m &= m - 1u, slot++) {
            if (slot >= nobj) break;                                                       // (cannot happen: the volume did not change since the count)
            const uint32_t idx = first + (uint32_t)(__ffs((int)m) - 1);
            list[slot] = idx;
            h_insert(h, idx, (uint32_t)slot);
        }
    }
}

// ---- the 3x3x3 neighbourhood as a 27-bit word, bit t = a*9 + b*3 + c for the offset (a-1, b-1, c-1); bits ascend with the linear index
__device__ __forceinline__ int32_t bit_offset(int t, const Dim& d) {
    const int a = t / 9, b = (t / 3) % 3, c = t % 3;
    return ((a - 1) * d.n1 + (b - 1)) * d.n2 + (c - 1);
}
// the word of the object voxel idx
__device__ __forceinline__ uint32_t gather_word(const uint8_t* __restrict__ vol, const Dim& d, uint32_t idx) {
    const int32_t r = (int32_t)(idx / (uint32_t)d.n2), i2 = (int32_t)(idx - (uint32_t)r * (uint32_t)d.n2), i0 = r / d.n1, i1 = r - i0 * d.n1;
    uint32_t w = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int t = a * 9 + b * 3 + c;
                if (t == 13) continue;
                const bool in = (uint32_t)(i0 + a - 1) < (uint32_t)d.n0 && (uint32_t)(i1 + b - 1) < (uint32_t)d.n1 && (uint32_t)(i2 + c - 1) < (uint32_t)d.n2;
                if (in && vol[(int64_t)idx + bit_offset(t, d)]) w |= 1u << t;
            }
    return w;
}

inline int grid_for(u64 items, int cap) { return (int)std::max<u64>(1, std::min<u64>((u64)cap, (items + TPB - 1) / TPB)); }

}  // namespace
