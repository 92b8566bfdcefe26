// vbridge_device.hip - vmask_bridge of include/vmask.h: the cheapest path through a cost volume between every two components of
// the vessel mask that come within reach of each other ("f19 bridges"): the headless stand-in for the
// "Reconnect" operation of the reference's manual-correction GUI.
//
// Every mask voxel is a source (D = 0, Root = its own index).  A domain voxel outside the mask has D(v) = min over its domain
// neighbours u of fl(D(u) + w(u, v)) where that is <= R = max_cost / 2, else +inf, with w(u, v) = fl(fl(c(u) + c(v)) * hw[k]):
// the least fixed point, what Dijkstra computes with the same two roundings.  Root(v) = the smallest Root(u) among the tight
// predecessors (fl(D(u) + w) == D(v)), Pred(v) = the tight predecessor of the same Root with the smallest offset code.  All three
// are unique fixed points, so the schedule below cannot show in the result.
//
// NO FUSED MULTIPLY-ADD: hipcc contracts a * b + c on the device by default, which would round D + (c(u) + c(v)) * hw once and
// not twice.  Contraction is switched off for this whole file by the pragma below (hipcc's default mode honours it); every
// product and every sum here is its own IEEE operation, on the device and on the host.
//
// The volume is cut into 8x8x8 bricks (vbrick.h: the store, its round driver and the hand-off argument).  Storage (a slot: 512 x
// D, cost, Root, Pred, component word) goes to the bricks that hold a domain voxel and lie within ceil(steps / 8) bricks
// (Chebyshev) of a brick with a mask voxel, steps = the most edges a path of length <= R can have: R / w_min, w_min the lightest
// edge the cost volume allows.
//   k_br_check     every voxel once: counts the domain, the costs that are not finite and positive, the smallest cost; marks
//                  the bricks that hold a mask voxel and those that hold a domain voxel
//   k_br_dilate    one axis of the box dilation of the mask's bricks on the brick grid;  k_br_want: dilated and domain
//   k_brick_slots  (vbrick.h) numbers the wanted bricks;  k_br_init: D, cost, Root of a slot
//   k_brick_list   (vbrick.h) compacts this round's flags into the list of active bricks
//   k_br_flood     one workgroup per active brick: D and cost of the brick + halo in LDS, Jacobi sweeps there, candidates above
//                  R dropped at once; shell changes flag the bricks that read them - the two conditions of vbrick.h's hand-off
//                  hold (stored values only decrease, each is the fl-sum along a real path)
//   k_br_root      the same rounds over Root once D is final: integer minimum over the tight predecessors
//   k_br_pred      once: Pred, and per voxel the word (component of Root << 1 | Root is a tip) that the contact pass reads
//   k_br_contact   every voxel looks at its 26 neighbours; the ordered pair (u, v) with comp(Root(u)) < comp(Root(v)) is a
//                  contact.  <0> counts them; <1> enters (a, b) in an open-addressing table and takes the minimum of the bits of
//                  K (positive doubles order as integers); <2> among the contacts that attain K the minimum of idx(u) << 5 | k.
//                  A contact first LOADS the table word and goes to the atomic only when it would lower it, so that once a
//                  pair's minimum has settled a contact stops at the load.  This stands in for aggregating within a wave and is
//                  a choice made for its simplicity: what it costs against same-address atomics is in DESIGN.md's f19 record
//                  where measured, and otherwise unmeasured
//   k_br_collect   table -> the list of pairs with K <= max_cost (the host sorts it by (a, b))
//   k_br_path      one thread per bridge: <0> the lengths of the two Pred chains, <1> pairs, costs and the path
//   k_br_scatter   bricks -> the dense dist / root / pred / comp volumes
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vbrick.h"
#include "vmask_cc.h"

namespace {

using vmask::CcRank;
using vmask::cc_rank;

enum { C_DOMAIN, C_BAD, C_CMIN, C_SLOTS, C_REACHED, C_CONTACTS, C_PAIRS, C_KEPT, C_LIST0, C_LIST1, C_N };

constexpr u64 EMPTY = ~0ull;

// the offset with code k = 0..25: the lexicographic order of (d0, d1, d2) in -1..1 with the centre left out
__device__ __forceinline__ void offset_of(int k, int& x, int& y, int& z) {
    const int j = k < 13 ? k : k + 1;
    x = j / 9 - 1; y = (j / 3) % 3 - 1; z = j % 3 - 1;
}
__device__ __forceinline__ double edge(double cu, double cv, double hw) { const double s = cu + cv; return s * hw; }

// ---- the inputs, and the bricks that get storage
template <class T>
__global__ void __launch_bounds__(TPB) k_br_check(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ domain, const T* __restrict__ cost,
                                                  u64 V, Geo g, uint8_t* __restrict__ mmark, uint8_t* __restrict__ dmark, u64* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    u64 ndom = 0, nbad = 0, cmin = 0x7ff0000000000000ull;               // (the bits of +inf)
    for (u64 i0 = (u64)blockIdx.x * TPB; i0 < V; i0 += (u64)gridDim.x * TPB) {            // (the same trips in every lane of a wave)
        const u64 idx = i0 + threadIdx.x;
        bool m = false, d = false;
        uint32_t brick = 0xffffffffu, local;
        if (idx < V) {
            m = mask[idx] != 0;
            d = m || !domain || domain[idx] != 0;
            if (d) {
                locate((uint32_t)idx, g, brick, local);
                const double c = (double)cost[idx];
                if (c > 0.0 && c < INFINITY) cmin = min(cmin, (u64)__double_as_longlong(c));
                else nbad++;
                ndom++;
            }
        }
        const uint32_t mb = m ? brick : 0xffffffffu;
        const uint32_t pd = __shfl_up(brick, 1, 64), pm = __shfl_up(mb, 1, 64);          // one store per run of a brick in the wave
        if (d && (lane == 0u || pd != brick)) dmark[brick] = 1;
        if (m && (lane == 0u || pm != mb)) mmark[brick] = 1;
    }
    wave_add(&ctr[C_DOMAIN * C_PITCH], ndom);
    wave_add(&ctr[C_BAD * C_PITCH], nbad);
#pragma unroll
    for (int o = 32; o; o >>= 1) cmin = min(cmin, (u64)__shfl_xor(cmin, o, 64));
    if (lane == 0u && cmin != 0x7ff0000000000000ull) atomicMin(&ctr[C_CMIN * C_PITCH], cmin);
}

// out[b] = any in[] within r bricks of b along one axis
__global__ void __launch_bounds__(TPB) k_br_dilate(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, Geo g, int axis, int32_t r) {
    const uint32_t nbricks = (uint32_t)g.B0 * (uint32_t)g.B1 * (uint32_t)g.B2;
    for (uint32_t b = blockIdx.x * TPB + threadIdx.x; b < nbricks; b += gridDim.x * TPB) {
        const Brick3 at = brick_coords(b, g);
        const int32_t c = axis == 0 ? at.b0 : axis == 1 ? at.b1 : at.b2, n = axis == 0 ? g.B0 : axis == 1 ? g.B1 : g.B2;
        const int64_t stride = axis == 0 ? (int64_t)g.B1 * g.B2 : axis == 1 ? g.B2 : 1;
        const int32_t lo = max(0, c - r), hi = min(n - 1, c + r);
        uint8_t any = 0;
        for (int32_t e = lo; e <= hi && !any; e++) any = in[(int64_t)b + (int64_t)(e - c) * stride];
        out[b] = any;
    }
}

__global__ void __launch_bounds__(TPB) k_br_want(const uint8_t* __restrict__ close_by, const uint8_t* __restrict__ dmark, uint32_t nbricks, int32_t* __restrict__ grid) {
    for (uint32_t b = blockIdx.x * TPB + threadIdx.x; b < nbricks; b += gridDim.x * TPB) grid[b] = (close_by[b] && dmark[b]) ? OCCUPIED : FREE;
}

template <class T>
__global__ void __launch_bounds__(BRICK) k_br_init(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ domain, const T* __restrict__ cost, Geo g,
                                                   const uint32_t* __restrict__ brick_of, double* __restrict__ D, double* __restrict__ Cst,
                                                   int32_t* __restrict__ Root) {
    const uint32_t slot = blockIdx.x, t = threadIdx.x;
    const Brick3 here = brick_coords(brick_of[slot], g);
    const uint32_t i0 = (uint32_t)here.b0 * 8u + (t >> 6), i1 = (uint32_t)here.b1 * 8u + ((t >> 3) & 7u), i2 = (uint32_t)here.b2 * 8u + (t & 7u);
    double d = -1.0, c = 1.0;
    int32_t root = NO_VALUE;
    if (i0 < (uint32_t)g.n0 && i1 < (uint32_t)g.n1 && i2 < (uint32_t)g.n2) {
        const size_t idx = ((size_t)i0 * g.n1 + i1) * g.n2 + i2;
        const bool m = mask[idx] != 0;
        if (m || !domain || domain[idx] != 0) { d = m ? 0.0 : INFINITY; c = (double)cost[idx]; if (m) root = (int32_t)idx; }
    }
    const size_t at = (size_t)slot * BRICK + t;
    D[at] = d; Cst[at] = c; Root[at] = root;
}

// ---- one round
// the 26 edge weights into LDS (the first barrier of load_halo covers them)
__device__ __forceinline__ void load_weights(const double* __restrict__ hw, double* sH) {
    const uint32_t t = threadIdx.x;
    if (t >= 32u && t < 58u) sH[t - 32u] = hw[t - 32u];
}

__global__ void __launch_bounds__(BRICK) k_br_flood(const uint32_t* __restrict__ list, const uint32_t* __restrict__ brick_of, const int32_t* __restrict__ grid,
                                                    Geo g, const double* __restrict__ hw, double R, double* D, const double* __restrict__ Cst,
                                                    uint32_t* __restrict__ flag_next) {
    __shared__ double sD[HALO], sC[HALO], sH[26];
    __shared__ int32_t nslot[27];
    __shared__ uint32_t mark[27];
    const uint32_t t = threadIdx.x, slot = list[blockIdx.x];
    if (t < 27u) mark[t] = 0u;
    load_weights(hw, sH);
    load_halo<true, false>(brick_of[slot], g, grid, D, Cst, nullptr, 0, sD, sC, nullptr, nslot);
    const int32_t me = halo_at(t);
    const size_t mine = (size_t)slot * BRICK + t;
    const double d0 = D[mine], cme = sC[me];                            // (only this workgroup stores to its brick)
    const bool in = d0 > 0.0;                                           // in the domain and no source
    double cur = in ? d0 : INFINITY;
    bool any = false;
    for (int sweep = 0; sweep < MAX_SWEEPS; sweep++) {
        double best = cur;
        if (in) {
            int k = 0;
#pragma unroll
            for (int x = -1; x <= 1; x++)
#pragma unroll
                for (int y = -1; y <= 1; y++)
#pragma unroll
                    for (int z = -1; z <= 1; z++) {
                        if (!x && !y && !z) continue;
                        const int n = me + x * 100 + y * 10 + z;
                        const double cand = sD[n] + edge(cme, sC[n], sH[k]);
                        k++;
                        best = (cand <= R && cand < best) ? cand : best;
                    }
        }
        const bool better = best < cur;
        any = __syncthreads_or(better) != 0;                            // (every load of this sweep is behind it)
        if (better) { cur = best; sD[me] = best; }
        __syncthreads();
        if (!any) break;
    }
    const bool changed = in && cur < d0;
    if (changed) st(D + mine, cur);
    mark_readers(changed, any, slot, nslot, mark, flag_next);
}

// bit k: the neighbour with code k is a tight predecessor of the voxel at `me`
__device__ __forceinline__ uint32_t tight_bits(const double* sD, const double* sC, const double* sH, int32_t me, double d0) {
    uint32_t tight = 0u;
    const double cme = sC[me];
    int k = 0;
#pragma unroll
    for (int x = -1; x <= 1; x++)
#pragma unroll
        for (int y = -1; y <= 1; y++)
#pragma unroll
            for (int z = -1; z <= 1; z++) {
                if (!x && !y && !z) continue;
                const int n = me + x * 100 + y * 10 + z;
                if (sD[n] + edge(cme, sC[n], sH[k]) == d0) tight |= 1u << k;
                k++;
            }
    return tight;
}

__global__ void __launch_bounds__(BRICK) k_br_root(const uint32_t* __restrict__ list, const uint32_t* __restrict__ brick_of, const int32_t* __restrict__ grid,
                                                   Geo g, const double* __restrict__ hw, const double* __restrict__ D, const double* __restrict__ Cst,
                                                   int32_t* Root, uint32_t* __restrict__ flag_next) {
    __shared__ double sD[HALO], sC[HALO], sH[26];
    __shared__ int32_t sL[HALO];
    __shared__ int32_t nslot[27];
    __shared__ uint32_t mark[27];
    const uint32_t t = threadIdx.x, slot = list[blockIdx.x];
    if (t < 27u) mark[t] = 0u;
    load_weights(hw, sH);
    load_halo<true, true>(brick_of[slot], g, grid, D, Cst, Root, NO_VALUE, sD, sC, sL, nslot);
    const int32_t me = halo_at(t);
    const size_t mine = (size_t)slot * BRICK + t;
    const double d0 = D[mine];
    const uint32_t tight = (d0 > 0.0 && d0 < INFINITY) ? tight_bits(sD, sC, sH, me, d0) : 0u;
    bool any;
    const int32_t l0 = Root[mine], cur = min_over_tight(tight, l0, sL, me, any);
    const bool changed = cur < l0;
    if (changed) st(Root + mine, cur);
    mark_readers(changed, any, slot, nslot, mark, flag_next);
}

// one workgroup per slot, once D and Root are final
__global__ void __launch_bounds__(BRICK) k_br_pred(const uint32_t* __restrict__ brick_of, const int32_t* __restrict__ grid, Geo g, const double* __restrict__ hw,
                                                   const double* __restrict__ D, const double* __restrict__ Cst, const int32_t* __restrict__ Root,
                                                   const int32_t* __restrict__ ccroot, CcRank rk, const uint8_t* __restrict__ tips,
                                                   uint8_t* __restrict__ Pred, int32_t* __restrict__ Cid, u64* __restrict__ ctr) {
    __shared__ double sD[HALO], sC[HALO], sH[26];
    __shared__ int32_t sL[HALO];
    __shared__ int32_t nslot[27];
    const uint32_t t = threadIdx.x, slot = blockIdx.x;
    load_weights(hw, sH);
    load_halo<true, true>(brick_of[slot], g, grid, D, Cst, Root, NO_VALUE, sD, sC, sL, nslot);
    const int32_t me = halo_at(t);
    const size_t mine = (size_t)slot * BRICK + t;
    const double d0 = D[mine];
    const int32_t root = sL[me];
    const bool reached = d0 > 0.0 && d0 < INFINITY;
    uint32_t code = 255u;
    if (reached) {
        const uint32_t tight = tight_bits(sD, sC, sH, me, d0);
        int k = 0;
#pragma unroll
        for (int x = -1; x <= 1; x++)
#pragma unroll
            for (int y = -1; y <= 1; y++)
#pragma unroll
                for (int z = -1; z <= 1; z++) {
                    if (!x && !y && !z) continue;
                    if (code == 255u && (tight & (1u << k)) && sL[me + x * 100 + y * 10 + z] == root) code = (uint32_t)k;
                    k++;
                }
    }
    Pred[mine] = (uint8_t)code;
    int32_t cid = 0;
    if (d0 >= 0.0 && root != NO_VALUE) cid = (int32_t)(((cc_rank(rk, (uint32_t)ccroot[root]) + 1u) << 1) | ((!tips || tips[root]) ? 1u : 0u));
    Cid[mine] = cid;
    wave_add(&ctr[C_REACHED * C_PITCH], reached ? 1ull : 0ull);
}

// ---- contacts
__device__ __forceinline__ uint32_t hash_of(u64 key, uint32_t bits) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - bits)); }

// PHASE 0: count; 1: enter the pair, minimum of the bits of K; 2: among the contacts that attain it, minimum of idx(u) << 5 | k
template <int PHASE>
__global__ void __launch_bounds__(BRICK) k_br_contact(const uint32_t* __restrict__ brick_of, const int32_t* __restrict__ grid, Geo g, const double* __restrict__ hw,
                                                      const double* __restrict__ D, const double* __restrict__ Cst, const int32_t* __restrict__ Cid,
                                                      int tip_rule, u64* tkey, u64* tK, u64* ttie, uint32_t tbits, u64* __restrict__ ctr) {
    __shared__ double sD[HALO], sC[HALO], sH[26];
    __shared__ int32_t sI[HALO];
    __shared__ int32_t nslot[27];
    const uint32_t t = threadIdx.x, slot = blockIdx.x, b = brick_of[slot];
    load_weights(hw, sH);
    load_halo<true, true>(b, g, grid, D, Cst, Cid, 0, sD, sC, sI, nslot);
    const int32_t me = halo_at(t);
    const int32_t ime = sI[me];
    const double dme = sD[me], cme = sC[me];
    const Brick3 here = brick_coords(b, g);
    const u64 idx = ((u64)((uint32_t)here.b0 * 8u + (t >> 6)) * (u64)g.n1 + ((uint32_t)here.b1 * 8u + ((t >> 3) & 7u))) * (u64)g.n2 + ((uint32_t)here.b2 * 8u + (t & 7u));
    u64 found = 0;
    if (ime != 0) {                                                     // (then D is finite: Root exists)
        const uint32_t ca = (uint32_t)ime >> 1, tipa = (uint32_t)ime & 1u;
#pragma nounroll
        for (int k = 0; k < 26; k++) {
            int x, y, z;
            offset_of(k, x, y, z);
            const int n = me + x * 100 + y * 10 + z;
            const int32_t iv = sI[n];
            if (iv == 0) continue;
            const uint32_t cb = (uint32_t)iv >> 1;
            if (!(ca < cb) || (int)(tipa + ((uint32_t)iv & 1u)) < tip_rule) continue;
            found++;
            if (PHASE == 0) continue;
            const double s = dme + sD[n];
            const double K = s + edge(cme, sC[n], sH[k]);
            const u64 kb = (u64)__double_as_longlong(K), key = ((u64)ca << 32) | (u64)cb;
            uint32_t h = hash_of(key, tbits);
            const uint32_t tmask = (1u << tbits) - 1u;
            bool hit = false;
            for (uint32_t probe = 0; probe <= tmask && !hit; probe++) {  // (the table has more entries than there are pairs)
                u64 at = ld(tkey + h);
                if (PHASE == 1 && at == EMPTY) { at = atomicCAS(tkey + h, EMPTY, key); if (at == EMPTY) at = key; }
                if (at == key) hit = true;
                else if (at == EMPTY) break;                            // (phase 2 only, and not then: phase 1 entered every pair)
                else h = (h + 1u) & tmask;
            }
            if (!hit) continue;
            if (PHASE == 1) { if (kb < ld(tK + h)) atomicMin(tK + h, kb); }
            else if (kb == tK[h]) { const u64 tie = (idx << 5) | (u64)k; if (tie < ld(ttie + h)) atomicMin(ttie + h, tie); }
        }
    }
    if (PHASE == 0) wave_add(&ctr[C_CONTACTS * C_PITCH], found);
}

__global__ void __launch_bounds__(TPB) k_br_collect(const u64* __restrict__ tkey, const u64* __restrict__ tK, const u64* __restrict__ ttie, u64 entries,
                                                    double max_cost, u64* __restrict__ kept, u64 cap, u64* __restrict__ ctr) {
    u64 npair = 0;
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < entries; e += (u64)gridDim.x * TPB) {
        const u64 key = tkey[e];
        if (key == EMPTY) continue;
        npair++;
        if (!(__longlong_as_double((long long)tK[e]) <= max_cost)) continue;
        const u64 at = atomicAdd(&ctr[C_KEPT * C_PITCH], 1ull);
        if (at < cap) { kept[3 * at] = key; kept[3 * at + 1] = tK[e]; kept[3 * at + 2] = ttie[e]; }
    }
    wave_add(&ctr[C_PAIRS * C_PITCH], npair);
}

// ---- paths
struct Store { const int32_t* grid; const uint8_t* Pred; const int32_t* Root; };
// the voxel that Pred names at idx, -1 at a source (or where there is none)
__device__ __forceinline__ int64_t pred_of(int64_t idx, const Geo& g, const Store& s) {
    uint32_t brick, local;
    locate((uint32_t)idx, g, brick, local);
    const int32_t slot = s.grid[brick];
    if (slot < 0) return -1;
    const uint32_t code = s.Pred[(size_t)slot * BRICK + local];
    if (code > 25u) return -1;
    int x, y, z;
    offset_of((int)code, x, y, z);
    return idx + ((int64_t)x * g.n1 + y) * g.n2 + z;
}
__device__ __forceinline__ int64_t root_of(int64_t idx, const Geo& g, const Store& s) {
    uint32_t brick, local;
    locate((uint32_t)idx, g, brick, local);
    return s.Root[(size_t)s.grid[brick] * BRICK + local];
}

// kept: (a << 32 | b, bits of K, idx(u) << 5 | k) per bridge, sorted.  WRITE 0: lens[2 i], lens[2 i + 1] = the entries of the two chains
template <int WRITE>
__global__ void __launch_bounds__(TPB) k_br_path(const u64* __restrict__ kept, uint32_t n, Geo g, Store s, int64_t limit, int32_t* __restrict__ lens,
                                                 const int64_t* __restrict__ offsets, int64_t* __restrict__ pairs, double* __restrict__ costs,
                                                 int64_t* __restrict__ voxels) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const u64 key = kept[3 * (size_t)i], tie = kept[3 * (size_t)i + 2];
    const int64_t u = (int64_t)(tie >> 5);
    int x, y, z;
    offset_of((int)(tie & 31u), x, y, z);
    const int64_t v = u + ((int64_t)x * g.n1 + y) * g.n2 + z;
    if (WRITE == 0) {
        int32_t lu = 0, lv = 0;
        for (int64_t p = u; p >= 0 && lu < limit; p = pred_of(p, g, s)) lu++;
        for (int64_t p = v; p >= 0 && lv < limit; p = pred_of(p, g, s)) lv++;
        lens[2 * (size_t)i] = lu; lens[2 * (size_t)i + 1] = lv;
    } else {
        const int64_t off = offsets[i];
        const int32_t lu = lens[2 * (size_t)i], lv = lens[2 * (size_t)i + 1];
        int64_t p = u;
        for (int32_t j = 0; j < lu; j++, p = pred_of(p, g, s)) voxels[off + lu - 1 - j] = p;
        p = v;
        for (int32_t j = 0; j < lv; j++, p = pred_of(p, g, s)) voxels[off + lu + j] = p;
        int64_t* row = pairs + 6 * (size_t)i;
        row[0] = (int64_t)(key >> 32); row[1] = (int64_t)(key & 0xffffffffull); row[2] = u; row[3] = v;
        row[4] = root_of(u, g, s); row[5] = root_of(v, g, s);
        costs[i] = __longlong_as_double((long long)kept[3 * (size_t)i + 1]);
    }
}

// ---- bricks -> dense volumes
__global__ void __launch_bounds__(TPB) k_br_scatter(Geo g, u64 V, const int32_t* __restrict__ grid, const double* __restrict__ D, const int32_t* __restrict__ Root,
                                                    const uint8_t* __restrict__ Pred, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ domain,
                                                    const int32_t* __restrict__ ccroot, CcRank rk,
                                                    double* __restrict__ dist, int32_t* __restrict__ root, uint8_t* __restrict__ pred, int32_t* __restrict__ comp) {
    for (u64 idx = (u64)blockIdx.x * TPB + threadIdx.x; idx < V; idx += (u64)gridDim.x * TPB) {
        const bool m = mask[idx] != 0, dom = m || !domain || domain[idx] != 0;
        double d = dom ? (m ? 0.0 : INFINITY) : -1.0;                   // (a domain voxel without storage is out of reach)
        int32_t r = m ? (int32_t)idx : -1;
        uint8_t p = 255;
        uint32_t brick, local;
        locate((uint32_t)idx, g, brick, local);
        const int32_t slot = grid[brick];
        if (slot >= 0 && dom && !m) {
            const size_t at = (size_t)slot * BRICK + local;
            d = D[at];
            if (d < INFINITY) { r = Root[at]; p = Pred[at]; }
        }
        if (dist) dist[idx] = d;
        if (root) root[idx] = r;
        if (pred) pred[idx] = p;
        if (comp) comp[idx] = m ? (int32_t)cc_rank(rk, (uint32_t)ccroot[idx]) + 1 : 0;
    }
}

struct CcHold {                                                         // (the labelling's arrays are freed on every return)
    vmask::CcOut c;
    ~CcHold() { vmask::cc_release(c); }
};

struct Bricks {                                                         // (names only: the call's DevMem owns them)
    u64* ctr = nullptr; int32_t* grid = nullptr; uint32_t* brick_of = nullptr; double* D = nullptr; double* Cst = nullptr;
    int32_t* Root = nullptr; uint8_t* Pred = nullptr; int32_t* Cid = nullptr; uint32_t* flag = nullptr; uint32_t* list = nullptr;
    const double* hw = nullptr;
};

struct Args {
    const uint8_t* mask; const uint8_t* domain; const void* cost; int dtype; const uint8_t* tips;
    double max_cost; int tip_rule;
    int64_t* counts; int64_t* pairs; double* costs; int64_t cap_pair; int64_t* offsets; int64_t* voxels; int64_t cap_vox;
    double* dist; int32_t* root; uint8_t* pred; int32_t* comp;
};

template <class T>
int bridge(const Args& a, Geo g, const double* hw_host) {
    const u64 V = (u64)g.n0 * g.n1 * g.n2;
    const uint32_t nbricks = (uint32_t)g.B0 * (uint32_t)g.B1 * (uint32_t)g.B2;
    const double R = 0.5 * a.max_cost;
    DevMem mem;
    Bricks b;
    const uint8_t* dmask; const uint8_t* ddomain = nullptr; const uint8_t* dtips = nullptr; const T* dcost;
    int rc = bring(mem, a.mask, V, "mask", &dmask);
    if (!rc && a.domain) rc = bring(mem, a.domain, V, "domain", &ddomain);
    if (!rc && a.tips) rc = bring(mem, a.tips, V, "tips", &dtips);
    if (!rc) rc = bring(mem, (const T*)a.cost, V, "cost", &dcost);
    if (rc) return rc;
    VMASK_GRAB(b.ctr, (size_t)C_N * C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(b.ctr, 0, (size_t)C_N * C_PITCH * sizeof(u64), 0));
    VMASK_TRY(hipMemsetAsync(b.ctr + (size_t)C_CMIN * C_PITCH, 0xff, sizeof(u64), 0));
    { double* d = nullptr; VMASK_GRAB(d, 26, "weights"); VMASK_TRY(hipMemcpy(d, hw_host, 26 * sizeof(double), hipMemcpyHostToDevice)); b.hw = d; }
    uint8_t* marks = nullptr;                                           // mask bricks, domain bricks, two work arrays of the dilation
    VMASK_GRAB(marks, (size_t)4 * nbricks, "brick marks");
    VMASK_TRY(hipMemsetAsync(marks, 0, (size_t)4 * nbricks, 0));
    uint8_t* mmark = marks; uint8_t* dmark = marks + nbricks; uint8_t* w0 = marks + (size_t)2 * nbricks; uint8_t* w1 = marks + (size_t)3 * nbricks;
    k_br_check<T><<<grid_for((V + TPB - 1) / TPB, GRID_CAP), TPB>>>(dmask, ddomain, dcost, V, g, mmark, dmark, b.ctr);
    u64 head[3 * C_PITCH];
    VMASK_TRY(hipMemcpy(head, b.ctr, sizeof(head), hipMemcpyDeviceToHost));
    const u64 ndomain = head[C_DOMAIN * C_PITCH], nbad = head[C_BAD * C_PITCH], cbits = head[C_CMIN * C_PITCH];
    if (nbad) { vmask::set_error(std::to_string(nbad) + " costs inside the domain that are not finite and positive"); return VRG_E_ARG; }
    double hmin = hw_host[0];
    for (int k = 1; k < 26; k++) hmin = std::min(hmin, hw_host[k]);
    int32_t reach = 0;                                                  // bricks
    if (cbits != EMPTY) {
        double cmin;
        std::memcpy(&cmin, &cbits, sizeof(double));
        const double c2 = cmin + cmin, wmin = c2 * hmin;
        if (!(wmin > 0.0) || R / wmin > 1099511627776.0) { vmask::set_error("max_cost above 2^41 times the lightest edge the cost volume allows"); return VRG_E_ARG; }
        // a path of n edges is at least n wmin (1 - 2^-12) long: the bound above keeps every rounding below 2^-12 wmin
        const double steps = std::floor(R / wmin * 1.001) + 1.0;
        reach = (int32_t)std::min<double>((double)std::max({g.B0, g.B1, g.B2}), std::ceil(steps / 8.0));
    }
    // the components
    CcHold hold;
    rc = vmask::cc_label(dmask, g.n0, g.n1, g.n2, 3, false, hold.c);
    if (rc) return rc;
    const uint32_t ncomp = hold.c.ncomp;
    // the bricks with storage
    VMASK_GRAB(b.grid, nbricks, "brick grid");
    const int gb = grid_for(((u64)nbricks + TPB - 1) / TPB, GRID_CAP);
    k_br_dilate<<<gb, TPB>>>(mmark, w0, g, 0, reach);
    k_br_dilate<<<gb, TPB>>>(w0, w1, g, 1, reach);
    k_br_dilate<<<gb, TPB>>>(w1, w0, g, 2, reach);
    k_br_want<<<gb, TPB>>>(w0, dmark, nbricks, b.grid);
    VMASK_GRAB(b.brick_of, nbricks, "brick list");
    uint32_t nslots = 0;                                                // (brick_of holds one entry per brick)
    if ((rc = number_bricks(b.grid, nbricks, nbricks, b.brick_of, b.ctr + c_at(C_SLOTS), "more slots than bricks", nslots))) return rc;
    mem.drop(marks);
    int64_t rounds[2] = {0, 0};
    u64 reached = 0, contacts = 0, npairs = 0, nkept = 0;
    std::vector<u64> kept;
    u64* dkept = nullptr;
    int32_t* dlens = nullptr;
    std::vector<int64_t> offs(1, 0);
    if (nslots) {
        VMASK_GRAB(b.D, (size_t)nslots * BRICK, "brick distances");
        VMASK_GRAB(b.Cst, (size_t)nslots * BRICK, "brick costs");
        VMASK_GRAB(b.Root, (size_t)nslots * BRICK, "brick roots");
        VMASK_GRAB(b.Pred, (size_t)nslots * BRICK, "brick predecessors");
        VMASK_GRAB(b.Cid, (size_t)nslots * BRICK, "brick components");
        VMASK_GRAB(b.flag, (size_t)2 * nslots, "brick flags");
        VMASK_GRAB(b.list, nslots, "active bricks");
        k_br_init<T><<<nslots, BRICK>>>(dmask, ddomain, dcost, g, b.brick_of, b.D, b.Cst, b.Root);
        for (int pass = 0; pass < 2; pass++) {                          // every brick looks once, then as flagged
            VMASK_TRY(hipMemsetAsync(b.flag, 0, (size_t)2 * nslots * sizeof(uint32_t), 0));
            VMASK_TRY(hipMemsetAsync(b.flag, 1, (size_t)nslots * sizeof(uint32_t), 0));          // (0x01010101: not 0)
            rc = iterate(b.flag, b.list, b.ctr + c_at(C_LIST0), nslots, rounds[pass], [&](const uint32_t* list, uint32_t active, uint32_t* flag_next) {
                if (pass) k_br_root<<<active, BRICK>>>(list, b.brick_of, b.grid, g, b.hw, b.D, b.Cst, b.Root, flag_next);
                else k_br_flood<<<active, BRICK>>>(list, b.brick_of, b.grid, g, b.hw, R, b.D, b.Cst, flag_next);
            });
            if (rc) return rc;
        }
        k_br_pred<<<nslots, BRICK>>>(b.brick_of, b.grid, g, b.hw, b.D, b.Cst, b.Root, hold.c.root, hold.c.rank(), dtips, b.Pred, b.Cid, b.ctr);
        k_br_contact<0><<<nslots, BRICK>>>(b.brick_of, b.grid, g, b.hw, b.D, b.Cst, b.Cid, a.tip_rule, nullptr, nullptr, nullptr, 0, b.ctr);
        VMASK_TRY(hipGetLastError());
        VMASK_TRY(hipMemcpy(&reached, b.ctr + (size_t)C_REACHED * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
        VMASK_TRY(hipMemcpy(&contacts, b.ctr + (size_t)C_CONTACTS * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
    }
    if (contacts) {
        // at most one pair per contact and per two components; the table keeps at least half of its entries empty
        const u64 most = std::min<u64>(contacts, (u64)ncomp * (ncomp - 1) / 2);
        uint32_t tbits = 6;
        while (((u64)1 << tbits) < 2 * most) tbits++;
        const u64 entries = (u64)1 << tbits;
        u64* table = nullptr;
        VMASK_GRAB(table, (size_t)3 * entries, "pair table");
        VMASK_TRY(hipMemsetAsync(table, 0xff, (size_t)3 * entries * sizeof(u64), 0));
        u64* tkey = table; u64* tK = table + entries; u64* ttie = table + 2 * entries;
        k_br_contact<1><<<nslots, BRICK>>>(b.brick_of, b.grid, g, b.hw, b.D, b.Cst, b.Cid, a.tip_rule, tkey, tK, ttie, tbits, b.ctr);
        k_br_contact<2><<<nslots, BRICK>>>(b.brick_of, b.grid, g, b.hw, b.D, b.Cst, b.Cid, a.tip_rule, tkey, tK, ttie, tbits, b.ctr);
        VMASK_GRAB(dkept, (size_t)3 * most, "kept pairs");
        k_br_collect<<<grid_for((entries + TPB - 1) / TPB, 4096), TPB>>>(tkey, tK, ttie, entries, a.max_cost, dkept, most, b.ctr);
        VMASK_TRY(hipGetLastError());
        VMASK_TRY(hipMemcpy(&npairs, b.ctr + (size_t)C_PAIRS * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
        VMASK_TRY(hipMemcpy(&nkept, b.ctr + (size_t)C_KEPT * C_PITCH, sizeof(u64), hipMemcpyDeviceToHost));
        if (nkept > most) { vmask::set_error("more bridges than pairs"); return VRG_E_INTERNAL; }
        mem.drop(table);
    }
    const Store store{b.grid, b.Pred, b.Root};
    if (nkept) {                                                        // ascending by (a, b): the keys are distinct
        kept.resize((size_t)3 * nkept);
        VMASK_TRY(hipMemcpy(kept.data(), dkept, kept.size() * sizeof(u64), hipMemcpyDeviceToHost));
        std::vector<uint32_t> order((size_t)nkept);
        for (uint32_t i = 0; i < nkept; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return kept[3 * (size_t)x] < kept[3 * (size_t)y]; });
        std::vector<u64> sorted(kept.size());
        for (size_t i = 0; i < nkept; i++) std::copy(kept.begin() + 3 * (size_t)order[i], kept.begin() + 3 * (size_t)order[i] + 3, sorted.begin() + 3 * i);
        VMASK_TRY(hipMemcpy(dkept, sorted.data(), sorted.size() * sizeof(u64), hipMemcpyHostToDevice));
        VMASK_GRAB(dlens, (size_t)2 * nkept, "path lengths");
        k_br_path<0><<<(uint32_t)((nkept + TPB - 1) / TPB), TPB>>>(dkept, (uint32_t)nkept, g, store, (int64_t)std::min<u64>(V, 0x7fffffff), dlens, nullptr, nullptr, nullptr, nullptr);
        VMASK_TRY(hipGetLastError());
        std::vector<int32_t> lens((size_t)2 * nkept);
        VMASK_TRY(hipMemcpy(lens.data(), dlens, lens.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        offs.resize((size_t)nkept + 1);
        for (size_t i = 0; i < nkept; i++) offs[i + 1] = offs[i] + lens[2 * i] + lens[2 * i + 1];
    }
    const int64_t nvox = offs.back();
    const int64_t out[10] = {(int64_t)ncomp, (int64_t)ndomain, (int64_t)reached, (int64_t)contacts, (int64_t)npairs, (int64_t)nkept, nvox,
                             (int64_t)nslots, rounds[0], rounds[1]};
    const bool lists = a.pairs || a.costs || a.offsets || a.voxels;
    if (lists && ((int64_t)nkept > a.cap_pair || nvox > a.cap_vox)) {
        if (a.counts && (rc = put(a.counts, out, 10))) return rc;
        vmask::set_error("capacity too small: " + std::to_string(nkept) + " bridges, " + std::to_string(nvox) + " path entries");
        return VRG_E_ARG;
    }
    if (lists) {
        if ((rc = put(a.offsets, offs.data(), offs.size()))) return rc;
        if (nkept) {
            Out<int64_t> opairs, ovox; Out<double> ocosts; const int64_t* doffs = nullptr;
            if ((rc = opairs.open(mem, a.pairs, (size_t)6 * nkept, "pairs")) || (rc = ocosts.open(mem, a.costs, (size_t)nkept, "costs")) ||
                (rc = ovox.open(mem, a.voxels, (size_t)nvox, "path voxels")) || (rc = send(mem, offs, "offsets", &doffs))) return rc;
            k_br_path<1><<<(uint32_t)((nkept + TPB - 1) / TPB), TPB>>>(dkept, (uint32_t)nkept, g, store, 0, dlens, doffs, opairs.dev, ocosts.dev, ovox.dev);
            VMASK_TRY(hipGetLastError());
            if ((rc = opairs.close()) || (rc = ocosts.close()) || (rc = ovox.close())) return rc;
        }
    }
    if (a.dist || a.root || a.pred || a.comp) {
        Out<double> odist; Out<int32_t> oroot, ocomp; Out<uint8_t> opred;
        if ((a.dist && (rc = odist.open(mem, a.dist, V, "dist"))) || (a.root && (rc = oroot.open(mem, a.root, V, "root"))) ||
            (a.pred && (rc = opred.open(mem, a.pred, V, "pred"))) || (a.comp && (rc = ocomp.open(mem, a.comp, V, "comp")))) return rc;
        k_br_scatter<<<grid_for((V + TPB - 1) / TPB, GRID_CAP), TPB>>>(g, V, b.grid, b.D, b.Root, b.Pred, dmask, ddomain, hold.c.root, hold.c.rank(),
                                                                        odist.dev, oroot.dev, opred.dev, ocomp.dev);
        VMASK_TRY(hipGetLastError());
        if ((rc = odist.close()) || (rc = oroot.close()) || (rc = opred.close()) || (rc = ocomp.close())) return rc;
    }
    VMASK_TRY(hipDeviceSynchronize());
    if (a.counts && (rc = put(a.counts, out, 10))) return rc;
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_bridge(int device, const uint8_t* mask, const uint8_t* domain, const void* cost, int dtype, const uint8_t* tips,
                            int64_t n0, int64_t n1, int64_t n2, const double* spacing, double max_cost, int tip_rule,
                            int64_t* counts, int64_t* pairs, double* costs, int64_t cap_pair, int64_t* offsets, int64_t* voxels, int64_t cap_vox,
                            double* dist, int32_t* root, uint8_t* pred, int32_t* comp) {
    if (!mask || !cost) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (dtype != VRG_F32 && dtype != VRG_F64) { vmask::set_error("cost: VRG_F32 or VRG_F64"); return VRG_E_ARG; }
    if (!std::isfinite(max_cost) || !(max_cost > 0.0)) { vmask::set_error("max_cost not finite and positive"); return VRG_E_ARG; }
    if (tip_rule < 0 || tip_rule > 2) { vmask::set_error("tip_rule outside 0..2"); return VRG_E_ARG; }
    const bool lists = pairs || costs || offsets || voxels;
    if (lists && (!pairs || !costs || !offsets || !voxels || cap_pair < 0 || cap_vox < 0)) { vmask::set_error("pairs, costs, offsets and voxels: all or none, capacities >= 0"); return VRG_E_ARG; }
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
    double hw[26];
    for (int k = 0; k < 26; k++) {                                      // float64, summed in the order of the axes; the halving is exact
        const int j = k < 13 ? k : k + 1;
        const double x = (j / 9 - 1) * h[0], y = ((j / 3) % 3 - 1) * h[1], z = (j % 3 - 1) * h[2];
        volatile double xx = x * x, yy = y * y, zz = z * z;
        volatile double s = xx + yy;
        hw[k] = 0.5 * std::sqrt(s + zz);
    }
    const Args a{mask, domain, cost, dtype, tips, max_cost, tip_rule, counts, pairs, costs, cap_pair, offsets, voxels, cap_vox, dist, root, pred, comp};
    const Geo g = make_geo(n0, n1, n2);
    return dtype == VRG_F32 ? bridge<float>(a, g, hw) : bridge<double>(a, g, hw);
}
