// vskel_simple.h - the thinning predicate of k_skel_step (vskel_device.hip): "may the centre of this 3x3x3 neighbourhood be deleted",
// kept apart from the kernel so that a host program can run it: tests/test_skeleton.py compiles this header alone and compares
// `deletable` with a plain restatement of the definition on all 2^26 neighbourhoods.  Nothing but <stdint.h>.
//
// For an object voxel P with 3x3x3 neighbourhood N26* (P removed), P is
//   an end point  when N26* holds exactly one object voxel,
//   simple        (Malandain-Bertrand) when the object voxels of N26* form one 26-connected component and the background
//                 voxels of N18* that are 6-connected inside N18* to a background face neighbour form one 6-connected component
//                 (there is at least one background face neighbour).
// P may be deleted when it is simple and not an end point.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VSKEL_HD __host__ __device__ __forceinline__
#else
#define VSKEL_HD inline
#endif

// ---- the 3x3x3 neighbourhood as a 27-bit word: bit a*9 + b*3 + c for the offset (a-1, b-1, c-1)
constexpr uint32_t N_ALL = (1u << 27) - 1u, N_CENTRE = 1u << 13;
constexpr uint32_t C0 = 0x1249249u, C2 = C0 << 2;                       // c == 0 / c == 2
constexpr uint32_t B0 = 0x7u | (0x7u << 9) | (0x7u << 18), B2 = B0 << 6;   // b == 0 / b == 2
constexpr uint32_t N_FACE = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);
constexpr uint32_t N_CORNER = (1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26);
constexpr uint32_t N_18 = N_ALL & ~N_CORNER & ~N_CENTRE;

VSKEL_HD int vskel_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

// the neighbours of x (bits 0..26 only) one step along c, along b, along a: what a shift carries into the next row, plane or
// past bit 26 is masked off
VSKEL_HD uint32_t step_c(uint32_t x) { return ((x << 1) & (N_ALL & ~C0)) | ((x >> 1) & ~C2); }
VSKEL_HD uint32_t step_b(uint32_t x) { return ((x << 3) & (N_ALL & ~B0)) | ((x >> 3) & ~B2); }
VSKEL_HD uint32_t step_a(uint32_t x) { return ((x << 9) & N_ALL) | (x >> 9); }
// the part of `set` that is 26-connected (a box dilation: the three axes one after the other) / 6-connected to `seed`
VSKEL_HD uint32_t fill26(uint32_t seed, uint32_t set) {
    uint32_t x = seed, y;
    do { y = x; x |= step_c(x); x |= step_b(x); x |= step_a(x); x &= set; } while (x != y);
    return x;
}
VSKEL_HD uint32_t fill6(uint32_t seed, uint32_t set) {
    uint32_t x = seed, y;
    do { y = x; x = (x | step_c(x) | step_b(x) | step_a(x)) & set; } while (x != y);
    return x;
}
// object bits of N26* -> may the centre be deleted (not an end point, simple)
VSKEL_HD bool deletable(uint32_t obj) {
    if (vskel_popcount(obj) < 2) return false;                          // end point; an isolated voxel is not simple
    if (fill26(obj & (0u - obj), obj) != obj) return false;             // more than one 26-component of the object
    const uint32_t bg = ~obj & N_18, face = bg & N_FACE;
    if (!face) return false;
    return (fill6(face & (0u - face), bg) & face) == face;             // every background face neighbour reached inside N18*
}
