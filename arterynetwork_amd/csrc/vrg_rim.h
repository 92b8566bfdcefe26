// vrg_rim.h - the arithmetic of the rim groups' count (dense pass, option dense_memo = 2; rim_groups in vrg_device.hip), kept apart
// from the wave's cross-lane steps so that a host program can run it: tests/test_dense_rim_memo.py compiles this header alone and
// compares it with plain population counts.  Nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VRG_RIM_HD __host__ __device__ inline
#else
#define VRG_RIM_HD inline
#endif

// A lane's class word holds four groups of four voxels, two bits per voxel (bit 1 of a pair: outer).  Returns the lane's outer voxels
// of each group, one count (0..4) per byte.  The wave adds these words with plain 32-bit additions: over 32 lanes a byte reaches at
// most 128 and never carries into the next.
VRG_RIM_HD uint32_t vrg_rim_pack(uint32_t w) {
    uint32_t x = (w >> 1) & 0x55555555u;
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0f0f0f0fu;
}
// a, b: the 32-bit sums of the packed words of lanes 0..31 and 32..63 (each byte <= 128; their sum, up to 256, is formed here in 32
// bits); inner: the groups in which a lane holds an inner voxel; ic01, ic23: the four counts of init, 16 bits each.  Returns the groups
// that take their sum from the table: no inner voxel, as many outer voxels as init counted included ones, not 0.  ne: the groups that
// hold an included voxel; nouter: the unit's outer voxels.
VRG_RIM_HD uint32_t vrg_rim_decide(uint32_t a, uint32_t b, uint32_t inner, uint32_t ic01, uint32_t ic23, uint32_t& ne, uint32_t& nouter) {
    uint32_t m = 0u, some = 0u;
    nouter = 0u;
    for (int j = 0; j < 4; j++) {
        const uint32_t n = ((a >> (8 * j)) & 0xffu) + ((b >> (8 * j)) & 0xffu);
        const uint32_t ic = ((j < 2 ? ic01 : ic23) >> (16 * (j & 1))) & 0xffffu;
        if (n == ic && n != 0u) m |= 1u << j;
        if (n != 0u) some |= 1u << j;
        nouter += n;
    }
    ne = some | inner;
    return m & ~inner;
}
