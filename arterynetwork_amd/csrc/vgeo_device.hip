// vgeo_device.hip - vmask_geodesic of include/vmask.h: shortest-path distance from seed voxels through the 26-adjacency graph of
// the mask, and the label of the seed that every voxel's shortest paths come from ("f9 geodesic").
//
// D(seed) = 0, elsewhere D(v) = min over in-mask neighbours u of fl(D(u) + w(u - v)) in IEEE double: the least fixed point, what
// Dijkstra computes with the same addition.  Lab(seed) = its (smallest) label, elsewhere the smallest Lab(u) among the tight
// predecessors, fl(D(u) + w) == D(v).  Both are unique fixed points, so the schedule below cannot show in the result.
//
// The volume is cut into 8x8x8 bricks; only bricks that hold a mask voxel get storage (vbrick.h: the store, its round driver
// and the hand-off argument that makes racing halo loads safe): 512 doubles and 512 labels.
//   k_geo_mark     the mask as a flat byte string in aligned 16-byte words: counts the mask voxels, marks their bricks
//   k_brick_slots  (vbrick.h) numbers the marked bricks (brick -> slot grid, slot -> brick list)
//   k_geo_init     one workgroup per slot: -1 / +inf and "no label"
//   k_geo_check    one thread per seed: counts seeds outside the volume or the mask and labels outside 1..max_label
//   k_geo_seed     one thread per seed: D = 0, atomicMin of the label; its brick and the bricks that hold it in their halo are flagged
//   k_brick_list   (vbrick.h) compacts the flag array of this round into the list of active bricks and clears what it read
//   k_geo_relax<0> one workgroup per active brick: brick + one-voxel halo into LDS, Jacobi sweeps in LDS until nothing changes
//                  (at most MAX_SWEEPS: a brick that is not done flags itself), changed voxels stored; where a voxel of the
//                  outer shell changed, the bricks that see it are flagged for the next round
//   k_geo_relax<1> the same machinery over the labels once D is final: integer minimum over the tight predecessors
//   k_geo_scatter  bricks -> dense dist / labels, sizes by one atomic per distinct label among a wave's voxels
// Both updates meet the two conditions of vbrick.h's hand-off: stored values only decrease, and each is attained along a real
// path (D: the fl-sum along it, >= D; a label: that of a seed at the far end of a chain of tight predecessors).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vbrick.h"

namespace {

enum { C_MASK, C_SLOTS, C_BAD, C_REACHED, C_LIST0, C_LIST1, C_N };

struct Weights { double w[8]; };                   // [|d0| << 2 | |d1| << 1 | |d2|]

// ---- the occupied bricks
__global__ void __launch_bounds__(TPB) k_geo_mark(const uint4* __restrict__ base, u64 nwords, uint32_t lead, u64 V, Geo g,
                                                  int32_t* __restrict__ grid, u64* __restrict__ ctr) {
    u64 n = 0;
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < nwords; b += (u64)gridDim.x * TPB) {
        uint32_t m = word_mask(base, b, lead, V);
        n += (u64)__popc(m);
        const uint32_t first = (uint32_t)(16 * b - lead);                                  // (used only where a bit of m is set)
        uint32_t last = 0xffffffffu;
        for (; m; m &= m - 1u) {
            uint32_t brick, local;
            locate(first + (uint32_t)(__ffs((int)m) - 1), g, brick, local);
            if (brick != last) grid[brick] = OCCUPIED;
            last = brick;
        }
    }
    wave_add(&ctr[c_at(C_MASK)], n);
}

__global__ void __launch_bounds__(BRICK) k_geo_init(const uint8_t* __restrict__ mask, Geo g, const uint32_t* __restrict__ brick_of,
                                                    double* __restrict__ D, int32_t* __restrict__ Lab) {
    const uint32_t slot = blockIdx.x, t = threadIdx.x;
    const Brick3 at = brick_coords(brick_of[slot], g);
    const uint32_t i0 = (uint32_t)at.b0 * 8u + (t >> 6), i1 = (uint32_t)at.b1 * 8u + ((t >> 3) & 7u), i2 = (uint32_t)at.b2 * 8u + (t & 7u);
    const bool in = i0 < (uint32_t)g.n0 && i1 < (uint32_t)g.n1 && i2 < (uint32_t)g.n2 && mask[((size_t)i0 * g.n1 + i1) * g.n2 + i2] != 0;
    D[(size_t)slot * BRICK + t] = in ? INFINITY : -1.0;
    if (Lab) Lab[(size_t)slot * BRICK + t] = NO_VALUE;
}

// ---- seeds
__global__ void __launch_bounds__(TPB) k_geo_check(const int64_t* __restrict__ seeds, const int32_t* __restrict__ seed_labels, u64 nseed,
                                                   const uint8_t* __restrict__ mask, u64 V, int64_t max_label, u64* __restrict__ ctr) {
    u64 wrong = 0;
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < nseed; e += (u64)gridDim.x * TPB) {
        const int64_t v = seeds[e], l = seed_labels ? (int64_t)seed_labels[e] : 1;
        wrong += v < 0 || (u64)v >= V || !mask[v] || l < 1 || l > max_label;
    }
    wave_add(&ctr[c_at(C_BAD)], wrong);
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
        const Brick3 here = brick_coords(brick, g);
#pragma nounroll
        for (int x = -1; x <= 1; x++)
#pragma nounroll
            for (int y = -1; y <= 1; y++)
#pragma nounroll
                for (int z = -1; z <= 1; z++) {
                    if (!reads(x, y, z, local >> 6, (local >> 3) & 7u, local & 7u)) continue;
                    const int32_t c0 = here.b0 + x, c1 = here.b1 + y, c2 = here.b2 + z;
                    if ((uint32_t)c0 >= (uint32_t)g.B0 || (uint32_t)c1 >= (uint32_t)g.B1 || (uint32_t)c2 >= (uint32_t)g.B2) continue;
                    const int32_t s = grid[((size_t)c0 * g.B1 + c1) * g.B2 + c2];
                    if (s >= 0) flag[s] = 1u;
                }
    }
}

// ---- one round
// LABELS == 0: D, LABELS == 1: the labels over the final D.  One workgroup of BRICK threads per entry of list.
template <int LABELS>
__global__ void __launch_bounds__(BRICK) k_geo_relax(const uint32_t* __restrict__ list, const uint32_t* __restrict__ brick_of,
                                                     const int32_t* __restrict__ grid, Geo g, Weights wt, double* D, int32_t* Lab,
                                                     uint32_t* __restrict__ flag_next) {
    __shared__ double sD[HALO];
    __shared__ int32_t sL[LABELS ? HALO : 1];
    __shared__ int32_t nslot[27];
    __shared__ uint32_t mark[27];
    const uint32_t t = threadIdx.x, slot = list[blockIdx.x];
    if (t < 27u) mark[t] = 0u;
    load_halo<false, LABELS != 0>(brick_of[slot], g, grid, D, nullptr, Lab, NO_VALUE, sD, nullptr, sL, nslot);
    const int32_t me = halo_at(t);
    const size_t mine = (size_t)slot * BRICK + t;
    const double d0 = D[mine];                                          // (only this workgroup stores to its brick)
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
        // bit k: the neighbour with code k (vbrick.h's min_over_tight) is a tight predecessor, fl(D(u) + w) == D(v).  (Written out
        // here: as a function of its own it compiles to all 13 LDS reads in flight at once, 64 VGPRs where this takes 24)
        uint32_t tight = 0u;
        if (d0 >= 0.0 && d0 < INFINITY) {
            int k = 0;
#pragma unroll
            for (int x = -1; x <= 1; x++)
#pragma unroll
                for (int y = -1; y <= 1; y++)
#pragma unroll
                    for (int z = -1; z <= 1; z++) {
                        if (!x && !y && !z) continue;
                        if (sD[me + x * 100 + y * 10 + z] + wt.w[((x != 0) << 2) | ((y != 0) << 1) | (z != 0)] == d0) tight |= 1u << k;
                        k++;
                    }
        }
        const int32_t l0 = Lab[mine], cur = min_over_tight(tight, l0, sL, me, any);
        changed = cur < l0;
        if (changed) st(Lab + mine, cur);
    }
    mark_readers(changed, any, slot, nslot, mark, flag_next);
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
                if (Lab && d >= 0.0) { l = Lab[at]; if (l == NO_VALUE) l = 0; }
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
    wave_add(&ctr[c_at(C_REACHED)], reached);
}

struct Bricks {                                                         // (names only: the call's DevMem owns them)
    u64* ctr = nullptr; int32_t* grid = nullptr; uint32_t* brick_of = nullptr; double* D = nullptr; int32_t* Lab = nullptr;
    uint32_t* flag = nullptr; uint32_t* list = nullptr;
};

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
        VMASK_TRY(hipMemcpy(&bad, b.ctr + c_at(C_BAD), sizeof(u64), hipMemcpyDeviceToHost));
        if (bad) { vmask::set_error(std::to_string(bad) + " seeds outside the volume or the mask, or with a label outside 1..max_label"); return VRG_E_ARG; }
    }
    // the occupied bricks
    VMASK_GRAB(b.grid, nbricks, "brick grid");
    VMASK_TRY(hipMemsetAsync(b.grid, 0xff, (size_t)nbricks * sizeof(int32_t), 0));            // FREE
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(dmask) & 15u);
    const u64 nwords = (lead + V + 15u) / 16u;
    k_geo_mark<<<grid_for((nwords + TPB - 1) / TPB, GRID_CAP), TPB>>>(reinterpret_cast<const uint4*>(dmask - lead), nwords, lead, V, g, b.grid, b.ctr);
    u64 nmask = 0;
    VMASK_TRY(hipMemcpy(&nmask, b.ctr + c_at(C_MASK), sizeof(u64), hipMemcpyDeviceToHost));
    const uint32_t cap = (uint32_t)std::min<u64>(nmask, nbricks);
    VMASK_GRAB(b.brick_of, cap, "brick list");
    uint32_t nslots = 0;
    if ((rc = number_bricks(b.grid, nbricks, cap, b.brick_of, b.ctr + c_at(C_SLOTS), "more occupied bricks than mask voxels", nslots))) return rc;
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
            rc = iterate(b.flag, b.list, b.ctr + c_at(C_LIST0), nslots, rounds[0], [&](const uint32_t* list, uint32_t active, uint32_t* flag_next) {
                k_geo_relax<0><<<active, BRICK>>>(list, b.brick_of, b.grid, g, wt, b.D, b.Lab, flag_next);
            });
            if (rc) return rc;
            if (want_labels) {                                          // D is final: every brick looks at its labels once, then as flagged
                VMASK_TRY(hipMemsetAsync(b.flag, 0, (size_t)2 * nslots * sizeof(uint32_t), 0));
                VMASK_TRY(hipMemsetAsync(b.flag, 1, (size_t)nslots * sizeof(uint32_t), 0));      // (0x01010101: not 0)
                rc = iterate(b.flag, b.list, b.ctr + c_at(C_LIST0), nslots, rounds[1], [&](const uint32_t* list, uint32_t active, uint32_t* flag_next) {
                    k_geo_relax<1><<<active, BRICK>>>(list, b.brick_of, b.grid, g, wt, b.D, b.Lab, flag_next);
                });
                if (rc) return rc;
            }
        }
    }
    Out<double> odist; Out<int32_t> olab;                               // (both optional: one that is never opened keeps a null dev)
    if ((dist && (rc = odist.open(mem, dist, V, "dist"))) || (labels && (rc = olab.open(mem, labels, V, "labels")))) return rc;
    k_geo_scatter<<<grid_for((V + TPB - 1) / TPB, GRID_CAP), TPB>>>(g, V, b.grid, b.D, b.Lab, odist.dev, olab.dev, sizes ? cnt : nullptr, b.ctr);
    VMASK_TRY(hipGetLastError());
    u64 reached = 0;
    VMASK_TRY(hipMemcpy(&reached, b.ctr + c_at(C_REACHED), sizeof(u64), hipMemcpyDeviceToHost));
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
    return geodesic(mask, make_geo(n0, n1, n2), seeds, seed_labels, nseed, wt, dist, labels, sizes, max_label, counts);
}
