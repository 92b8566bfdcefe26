// vmask_wave.h - the device helpers that the passes over a mask share whatever their storage is (vseg_slots.h: compacted voxels,
// vbrick.h: sparse bricks): padded counters, the sums, scans and reservations of one wave, and the mask read as a flat byte
// string in aligned 16-byte words.  Everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef unsigned long long u64;

// counters on the device sit 256 bytes apart: each is added to by every wave that has something to add
constexpr int C_PITCH = 32;
__host__ __device__ inline int c_at(int k) { return k * C_PITCH; }

// ---- wave helpers (every lane of the wave must call them)
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ void wave_add(u64* ctr, u64 x) {
    x = wave_sum(x);
    if (x && lane_id() == 0u) atomicAdd(ctr, x);
}
// exclusive prefix sum of x over the wave's lanes; total = the wave's sum
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, uint32_t& total) {
    uint32_t v = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(v, o, 64); if (lane_id() >= (uint32_t)o) v += y; }
    total = __shfl(v, 63, 64);
    return v - x;
}
// room for `total` entries behind the cursor, the wave's first entry returned to every lane
__device__ __forceinline__ u64 wave_reserve(u64* cursor, uint32_t total) {
    u64 at = 0;
    if (lane_id() == 0u) at = atomicAdd(cursor, (u64)total);
    return __shfl(at, 0, 64);
}

// ---- the volume as a flat byte string read in aligned 16-byte words
// bit k of the result: byte k of the word is != 0
__device__ __forceinline__ uint32_t nz4(uint32_t w) {
    const uint32_t h = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
    return ((h >> 7) & 1u) | ((h >> 14) & 2u) | ((h >> 21) & 4u) | ((h >> 28) & 8u);
}
// word b of the aligned string covers voxels 16 b - lead .. + 15: the 16-bit mask of its object voxels, those outside [0, V) dropped
__device__ __forceinline__ uint32_t word_mask(const uint4* __restrict__ base, u64 b, uint32_t lead, u64 V) {
    const uint4 w = base[b];
    if (!(w.x | w.y | w.z | w.w)) return 0u;
    uint32_t m = nz4(w.x) | (nz4(w.y) << 4) | (nz4(w.z) << 8) | (nz4(w.w) << 12);
    const int64_t f0 = (int64_t)(16 * b) - (int64_t)lead, left = (int64_t)V - f0;    // (left >= 1)
    if (f0 < 0) m &= ~((1u << (uint32_t)(-f0)) - 1u);
    if (left < 16) m &= (1u << (uint32_t)left) - 1u;
    return m;
}

}  // namespace
