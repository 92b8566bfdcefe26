// vreg_walk.h - how k_reg_hist (vreg_device.hip) walks the fixed grid: a voxel's flat index is split once into (i, j, k) and then
// advanced by the split stride with one carry per axis, no division per voxel.  Kept apart from the kernel so that a host program
// can run it: tests/test_registration.py compiles this header alone and compares every step of the walk with split().
// Nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VREG_WALK_HD __host__ __device__ __forceinline__
#else
#define VREG_WALK_HD inline
#endif

struct Ext { int n0, n1, n2; };

VREG_WALK_HD void split(int64_t v, const Ext n, int& i, int& j, int& k) {
    const unsigned u = (unsigned)v, plane = (unsigned)n.n1 * (unsigned)n.n2;       // (fewer than 2^31 voxels)
    const unsigned a = u / plane, r = u - a * plane, b = r / (unsigned)n.n2;
    i = (int)a; j = (int)b; k = (int)(r - b * (unsigned)n.n2);
}

// (i, j, k) = split(v)  ->  split(v + stride), with (di, dj, dk) = split(stride): dj < n1 and dk < n2, so at most one carry per axis
VREG_WALK_HD void advance_split(const Ext n, int di, int dj, int dk, int& i, int& j, int& k) {
    k += dk;
    if (k >= n.n2) { k -= n.n2; j++; }
    j += dj;
    if (j >= n.n1) { j -= n.n1; i++; }
    i += di;
}
