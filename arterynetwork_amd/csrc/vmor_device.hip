// vmor_device.hip - vmask_morphometry of include/vmask.h: what can be said about a branch of the branch graph - step counts,
// the radius sample's sums, end directions, the chord -, about a node - radius, the three incident branches - and, from
// roots, the path distance and depth of every node ("f11 branch morphometry").
//
//   k_mor_check      the tables are looked at before anything is written: offsets ascending by at least 2, every voxel inside the
//                    volume, every end and root a node id; one counter of what is wrong
//   k_mor_branch     ONE launch over the entries.  A wave takes four consecutive branches per trip: a branch of at most 17
//                    entries is done by the 16 lanes of its quarter (four such branches share the wave), a longer one by the
//                    whole wave, lane j taking the entries j, j + 64, ..  The float sums follow the order stated in vmask.h: a
//                    lane's values in sequence, then the xor tree - in a quarter the tree's first two steps add 0.0, which they
//                    would in the full wave as well.  The integer counts are ballots.
//   k_mor_gather     dist at every entry (asked for by the file writers: the radius of every voxel of a branch)
//   k_mor_incident   one thread per branch end: the node's end count, and the smallest, the largest and the sum of the packed
//                    (branch, end) words at the node - with three ends the middle one is the sum less the other two
//   k_mor_node       one thread per node: its radius and the three incident branches
//   k_mor_relax      one thread per branch: D(v) <- min(D(v), fl(D(u) + w)) both ways by atomicMin on the bits; the host reads
//                    one counter per round (as k_br_hook's rounds do)
//   k_mor_parent     one thread per branch: the smallest tight branch of either end by atomicMin
//   k_mor_level      one round of depthLevel / depthVoxel down the parent tree: a node takes its values from a parent that got
//                    its own in an EARLIER launch (a stamp says in which), so kernel boundaries are the only ordering
//   k_mor_finish     the unreached nodes' -1, branchLevel
// No floating-point atomics; nothing here is contracted into an FMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vseg_slots.h"

#pragma clang fp contract(off)

namespace {

constexpr int SHORT_MAX = 17;                      // entries of a branch that a quarter wave takes: 16 pairs, at most 15 sample values
constexpr u64 INF_BITS = 0x7ff0000000000000ull, NAN_BITS = 0x7ff8000000000000ull;
enum { BI_STEP = 0, BI_JUMPS = 7, BI_JUMP_OFFSET = 8, BI_RADIUS_COUNT = 14, BI_END_DIR = 15, BI_CHORD = 21, BI_N = 24 };
enum { BF_SUM = 0, BF_DEVSQ, BF_MIN, BF_MAX, BF_PATH, BF_N };

struct Vol { uint32_t n1, n2; u64 V; };

__device__ __forceinline__ void unravel(int64_t idx, const Vol& s, int32_t& i0, int32_t& i1, int32_t& i2) {
    const uint32_t v = (uint32_t)idx, r = v / s.n2;
    i2 = (int32_t)(v - r * s.n2); i0 = (int32_t)(r / s.n1); i1 = (int32_t)(r - (uint32_t)i0 * s.n1);
}
// b - a as an integer offset; the class 4|d0| + 2|d1| + |d2| - 1 of a 26-adjacent pair, 7 for any other pair
__device__ __forceinline__ int pair_class(int64_t a, int64_t b, const Vol& s, int32_t& d0, int32_t& d1, int32_t& d2) {
    int32_t a0, a1, a2, b0, b1, b2;
    unravel(a, s, a0, a1, a2); unravel(b, s, b0, b1, b2);
    d0 = b0 - a0; d1 = b1 - a1; d2 = b2 - a2;
    const int32_t e0 = abs(d0), e1 = abs(d1), e2 = abs(d2);
    if ((e0 | e1 | e2) > 1 || !(e0 | e1 | e2)) return 7;
    return 4 * e0 + 2 * e1 + e2 - 1;
}
__device__ __forceinline__ double canonical(double x) { return x != x ? __longlong_as_double((long long)NAN_BITS) : x; }

__global__ void __launch_bounds__(TPB) k_mor_check(const int64_t* __restrict__ off, u64 B, const int64_t* __restrict__ vox, u64 total, u64 V,
                                                   const int64_t* __restrict__ ends, const int64_t* __restrict__ nodevox, u64 N,
                                                   const int64_t* __restrict__ roots, u64 nroots, u64* __restrict__ bad) {
    u64 wrong = 0;
    const u64 m0 = B > total ? B : total, m1 = N > nroots ? N : nroots, most = m0 > m1 ? m0 : m1;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < most; i += (u64)gridDim.x * TPB) {
        if (i < B) {
            const int64_t a = off[i], b = off[i + 1], ea = ends[2 * i], eb = ends[2 * i + 1];
            wrong += a < 0 || b - a < 2 || (u64)b > total || (i == 0 && a != 0);
            wrong += ea < -1 || eb < -1 || ea >= (int64_t)N || eb >= (int64_t)N || ((ea < 0) != (eb < 0));
        }
        if (i < total) wrong += (u64)vox[i] >= V;
        if (i < N) wrong += (u64)nodevox[i] >= V;
        if (i < nroots) wrong += (u64)roots[i] >= N;
    }
    wave_add(bad, wrong);
}

__global__ void __launch_bounds__(TPB) k_mor_branch(const int64_t* __restrict__ off, u64 B, const int64_t* __restrict__ vox, const double* __restrict__ dist,
                                                    Vol s, int64_t local_steps, int64_t* __restrict__ bi, double* __restrict__ bf) {
    const uint32_t lane = lane_id(), q = lane >> 4, l = lane & 15u;
    const u64 waves = (u64)gridDim.x * (TPB / 64), wave = ((u64)blockIdx.x * TPB + threadIdx.x) >> 6;
    const double inf = __longlong_as_double((long long)INF_BITS);
    for (u64 b0 = 4 * wave; b0 < B; b0 += 4 * waves) {                     // (the same trips in every lane of a wave)
        const u64 b = b0 + q;
        const bool valid = b < B;
        const int64_t a = valid ? off[b] : 0, n = valid ? off[b + 1] - a : 0;
        const int64_t first = n >= 3 ? 1 : 0, m = n >= 3 ? n - 2 : n;     // the radius sample: the interior entries, both of a pair
        const bool small = valid && n <= SHORT_MAX;
        int32_t d0, d1, d2;
        // ---- a quarter wave per branch
        int cls = -1;
        double x = 0.0;
        bool has = false;
        if (small) {
            if ((int64_t)l < n - 1) cls = pair_class(vox[a + l], vox[a + l + 1], s, d0, d1, d2);
            if ((int64_t)l < m) { x = dist[vox[a + first + l]]; has = true; }
        }
        u64 mine = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const u64 hit = __ballot(cls == c);
            if (l == (uint32_t)c) mine = (u64)__popcll((hit >> (16u * q)) & 0xffffull);
        }
        double sum = x, mn = has ? x : inf, mx = has ? x : -inf;
#pragma unroll
        for (int o = 8; o; o >>= 1) {
            sum = sum + __shfl_xor(sum, o, 64);
            mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64));
        }
        const double mean = sum / (double)m;                              // (m >= 1 wherever the result is used)
        const double dev = has ? x - mean : 0.0;
        double sq = dev * dev;
#pragma unroll
        for (int o = 8; o; o >>= 1) sq = sq + __shfl_xor(sq, o, 64);
        if (small) {
            if (l < 8u) bi[b * BI_N + BI_STEP + l] = (int64_t)mine;
            if (l == 0u) { bf[b * BF_N + BF_SUM] = sum; bf[b * BF_N + BF_DEVSQ] = canonical(sq); bf[b * BF_N + BF_MIN] = mn; bf[b * BF_N + BF_MAX] = mx; }
        }
        // ---- the whole wave per longer branch, one after the other
        for (u64 todo = __ballot(valid && !small && l == 0u); todo; todo &= todo - 1ull) {
            const int src = __ffsll((long long)todo) - 1;
            const u64 bb = b0 + ((uint32_t)src >> 4);
            const int64_t aa = __shfl(a, src, 64), nn = __shfl(n, src, 64), mm = nn - 2;
            u64 cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            double acc = 0.0, lo = inf, hi = -inf;
            for (int64_t k = 0; k < nn - 1; k += 64) {
                const int64_t i = k + lane;
                int c = -1;
                if (i < nn - 1) c = pair_class(vox[aa + i], vox[aa + i + 1], s, d0, d1, d2);
#pragma unroll
                for (int t = 0; t < 8; t++) cnt[t] += (u64)__popcll(__ballot(c == t));
                if (i < mm) { const double y = dist[vox[aa + 1 + i]]; acc = acc + y; lo = fmin(lo, y); hi = fmax(hi, y); }
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                acc = acc + __shfl_xor(acc, o, 64);
                lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64));
            }
            const double mu = acc / (double)mm;
            double acc2 = 0.0;
            for (int64_t k = 0; k < mm; k += 64) {
                const int64_t i = k + lane;
                if (i < mm) { const double e = dist[vox[aa + 1 + i]] - mu; acc2 = acc2 + e * e; }
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) acc2 = acc2 + __shfl_xor(acc2, o, 64);
            u64 own = 0;
#pragma unroll
            for (int t = 0; t < 8; t++) if (lane == (uint32_t)t) own = cnt[t];
            if (lane < 8u) bi[bb * BI_N + BI_STEP + lane] = (int64_t)own;
            if (lane == 0u) { bf[bb * BF_N + BF_SUM] = acc; bf[bb * BF_N + BF_DEVSQ] = canonical(acc2); bf[bb * BF_N + BF_MIN] = lo; bf[bb * BF_N + BF_MAX] = hi; }
        }
        // ---- per branch, one lane: the jump offsets, the sample's size, the end directions and the chord
        if (valid && l == 0u) {
            int64_t* o = bi + b * BI_N;
            const int64_t v0 = vox[a], v1 = vox[a + n - 1];
            const bool front = pair_class(v0, vox[a + 1], s, d0, d1, d2) == 7;
            o[BI_JUMP_OFFSET] = front ? d0 : 0; o[BI_JUMP_OFFSET + 1] = front ? d1 : 0; o[BI_JUMP_OFFSET + 2] = front ? d2 : 0;
            const bool back = n > 2 && pair_class(vox[a + n - 2], v1, s, d0, d1, d2) == 7;
            o[BI_JUMP_OFFSET + 3] = back ? d0 : 0; o[BI_JUMP_OFFSET + 4] = back ? d1 : 0; o[BI_JUMP_OFFSET + 5] = back ? d2 : 0;
            o[BI_RADIUS_COUNT] = m;
            const int64_t in = local_steps < n - 1 ? local_steps : n - 1;
            (void)pair_class(v0, vox[a + in], s, d0, d1, d2);
            o[BI_END_DIR] = d0; o[BI_END_DIR + 1] = d1; o[BI_END_DIR + 2] = d2;
            (void)pair_class(v1, vox[a + n - 1 - in], s, d0, d1, d2);
            o[BI_END_DIR + 3] = d0; o[BI_END_DIR + 4] = d1; o[BI_END_DIR + 5] = d2;
            (void)pair_class(v0, v1, s, d0, d1, d2);
            o[BI_CHORD] = d0; o[BI_CHORD + 1] = d1; o[BI_CHORD + 2] = d2;
        }
    }
}

__global__ void __launch_bounds__(TPB) k_mor_gather(const int64_t* __restrict__ vox, u64 total, const double* __restrict__ dist, double* __restrict__ out) {
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < total; e += (u64)gridDim.x * TPB) out[e] = dist[vox[e]];
}

struct Incident { uint32_t* deg; u64* lo; u64* hi; u64* sum; };

__global__ void __launch_bounds__(TPB) k_mor_incident(const int64_t* __restrict__ ends, u64 B, u64 N, Incident t) {
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < 2 * B; e += (u64)gridDim.x * TPB) {
        const int64_t v = ends[e];
        if (v < 0 || (u64)v >= N) continue;
        atomicAdd(&t.deg[v], 1u); atomicMin(&t.lo[v], e); atomicMax(&t.hi[v], e); atomicAdd(&t.sum[v], e);      // e = 2 branch + end
    }
}

__global__ void __launch_bounds__(TPB) k_mor_node(const int64_t* __restrict__ nodevox, u64 N, const double* __restrict__ dist, Incident t,
                                                  double* __restrict__ radius, int64_t* __restrict__ incident) {
    for (u64 v = (u64)blockIdx.x * TPB + threadIdx.x; v < N; v += (u64)gridDim.x * TPB) {
        radius[v] = dist[nodevox[v]];
        int64_t i0 = -1, i1 = -1, i2 = -1;
        if (t.deg[v] == 3u) {
            const u64 lo = t.lo[v], hi = t.hi[v], mid = t.sum[v] - lo - hi;
            if ((lo >> 1) != (mid >> 1) && (mid >> 1) != (hi >> 1)) { i0 = (int64_t)lo; i1 = (int64_t)mid; i2 = (int64_t)hi; }
        }
        incident[3 * v] = i0; incident[3 * v + 1] = i1; incident[3 * v + 2] = i2;
    }
}

__global__ void __launch_bounds__(TPB) k_mor_roots(const int64_t* __restrict__ roots, u64 nroots, u64 N, u64* __restrict__ D, int64_t* __restrict__ depth,
                                                   int32_t* __restrict__ stamp) {
    for (u64 k = (u64)blockIdx.x * TPB + threadIdx.x; k < nroots; k += (u64)gridDim.x * TPB) {
        const u64 v = (u64)roots[k];
        if (v >= N) continue;
        D[v] = 0ull; depth[3 * v + 1] = 0; depth[3 * v + 2] = 0; stamp[v] = 0;      // (several entries may name one node: the same values)
    }
}

__global__ void __launch_bounds__(TPB) k_mor_fill(u64* __restrict__ D, u64 N) {
    for (u64 v = (u64)blockIdx.x * TPB + threadIdx.x; v < N; v += (u64)gridDim.x * TPB) D[v] = INF_BITS;
}

// D is read and lowered in the same launch: a stale read only delays, the round that lowers nothing has read the final state
__global__ void __launch_bounds__(TPB) k_mor_relax(const int64_t* __restrict__ ends, const double* __restrict__ bf, u64 B, u64 N, u64* D, u64* __restrict__ c_lowered) {
    u64 lowered = 0;
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < B; b += (u64)gridDim.x * TPB) {
        const int64_t u = ends[2 * b], v = ends[2 * b + 1];
        if (u < 0 || v < 0 || u == v || (u64)u >= N || (u64)v >= N) continue;
        const double w = bf[b * BF_N + BF_PATH];
        const u64 du = D[u], dv = D[v];
        const u64 to_v = (u64)__double_as_longlong(__longlong_as_double((long long)du) + w), to_u = (u64)__double_as_longlong(__longlong_as_double((long long)dv) + w);
        if (to_v < dv && atomicMin(&D[v], to_v) > to_v) lowered++;        // (non-negative doubles order as their bits; inf + w == inf lowers nothing)
        if (to_u < du && atomicMin(&D[u], to_u) > to_u) lowered++;
    }
    wave_add(c_lowered, lowered);
}

// depth[3 v]: parentBranch as an unsigned word, all ones (-1) where there is none
__global__ void __launch_bounds__(TPB) k_mor_parent(const int64_t* __restrict__ ends, const double* __restrict__ bf, u64 B, u64 N, const u64* __restrict__ D, int64_t* depth) {
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < B; b += (u64)gridDim.x * TPB) {
        const int64_t u = ends[2 * b], v = ends[2 * b + 1];
        if (u < 0 || v < 0 || u == v || (u64)u >= N || (u64)v >= N) continue;
        const double w = bf[b * BF_N + BF_PATH];
        const u64 du = D[u], dv = D[v];
        if (du < dv && dv != INF_BITS && (u64)__double_as_longlong(__longlong_as_double((long long)du) + w) == dv) atomicMin((u64*)&depth[3 * v], b);
        if (dv < du && du != INF_BITS && (u64)__double_as_longlong(__longlong_as_double((long long)dv) + w) == du) atomicMin((u64*)&depth[3 * u], b);
    }
}

__global__ void __launch_bounds__(TPB) k_mor_level(const int64_t* __restrict__ ends, const int64_t* __restrict__ off, u64 B, u64 N, int32_t round,
                                                   int64_t* depth, int32_t* stamp, u64* __restrict__ c_set) {
    u64 set = 0;
    for (u64 v = (u64)blockIdx.x * TPB + threadIdx.x; v < N; v += (u64)gridDim.x * TPB) {
        const int64_t b = depth[3 * v];
        if (b < 0 || (u64)b >= B || stamp[v] <= round) continue;          // no parent, or done
        const int64_t ea = ends[2 * b], u = ea == (int64_t)v ? ends[2 * b + 1] : ea;
        if (u < 0 || (u64)u >= N || stamp[u] >= round) continue;          // the parent's values must come from an earlier launch
        depth[3 * v + 1] = depth[3 * u + 1] + 1;
        depth[3 * v + 2] = depth[3 * u + 2] + (off[b + 1] - off[b] - 1);
        stamp[v] = round;
        set++;
    }
    wave_add(c_set, set);
}

__global__ void __launch_bounds__(TPB) k_mor_finish(const int64_t* __restrict__ ends, u64 B, u64 N, const int64_t* __restrict__ depth, int64_t* __restrict__ level) {
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < B; b += (u64)gridDim.x * TPB) {
        const int64_t u = ends[2 * b], v = ends[2 * b + 1];
        int64_t lv = -1;
        if (u >= 0 && v >= 0 && (u64)u < N && (u64)v < N) {
            const int64_t lu = depth[3 * u + 1], lw = depth[3 * v + 1];
            if (lu >= 0 && lw >= 0) lv = lu > lw ? lu : lw;
        }
        level[b] = lv;
    }
}

struct Args {
    const double* dist; const int64_t* offsets; int64_t B; const int64_t* voxels; const int64_t* ends; const int64_t* nodevox; int64_t N;
    const int64_t* roots; int64_t nroots; int64_t local_steps;
    int64_t* bi; double* bf; double* radius; int64_t* incident; double* entry_radius; double* distance; int64_t* depth; int64_t* level; int64_t* counts;
};

// the length of the offset o in the spacing h: the squares summed in the order of the axes
inline double length_of(const int64_t* o, const double* h) {
    const double t0 = (double)o[0] * h[0], t1 = (double)o[1] * h[1], t2 = (double)o[2] * h[2];
    return std::sqrt((t0 * t0 + t1 * t1) + t2 * t2);
}

int morphometry(const Args& g, const Vol& s, const double* h) {
    const u64 B = (u64)g.B, N = (u64)g.N, R = (u64)g.nroots;
    DevMem mem;
    int rc;
    int64_t total = 0;
    if (B) {
        int64_t edge[2] = {0, 0};
        if (vmask::is_device_pointer(g.offsets)) {
            VMASK_TRY(hipMemcpy(&edge[0], g.offsets, sizeof(int64_t), hipMemcpyDeviceToHost));
            VMASK_TRY(hipMemcpy(&edge[1], g.offsets + B, sizeof(int64_t), hipMemcpyDeviceToHost));
        } else { edge[0] = g.offsets[0]; edge[1] = g.offsets[B]; }
        if (edge[0] != 0 || edge[1] < 2 * (int64_t)B || edge[1] > ((int64_t)1 << 40)) { vmask::set_error("offsets do not describe branches of at least two entries"); return VRG_E_ARG; }
        total = edge[1];
    }
    const int64_t* off = nullptr; const int64_t* vox = nullptr; const int64_t* ends = nullptr; const int64_t* nodevox = nullptr; const int64_t* roots = nullptr;
    const double* dist = nullptr;
    if ((rc = bring(mem, g.offsets, B ? B + 1 : 0, "offsets", &off)) || (rc = bring(mem, g.voxels, (size_t)total, "branch voxels", &vox)) ||
        (rc = bring(mem, g.ends, 2 * B, "branch ends", &ends)) || (rc = bring(mem, g.nodevox, N, "node voxels", &nodevox)) ||
        (rc = bring(mem, g.roots, R, "roots", &roots)) || (rc = bring(mem, g.dist, (size_t)s.V, "distance volume", &dist))) return rc;
    u64* ctr = nullptr;
    VMASK_GRAB(ctr, 2 * C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(ctr, 0, 2 * C_PITCH * sizeof(u64), 0));
    const u64 most = std::max(std::max(B, (u64)total), std::max(N, R));
    u64 bad = 0;
    if (most) {
        k_mor_check<<<grid_for(most, GRID_LIST), TPB>>>(off, B, vox, (u64)total, s.V, ends, nodevox, N, roots, R, ctr);
        VMASK_TRY(hipMemcpy(&bad, ctr, sizeof(u64), hipMemcpyDeviceToHost));
    }
    if (bad) { vmask::set_error("the branch table does not fit the volume: offsets, voxels, ends, node voxels or roots out of range"); return VRG_E_ARG; }

    Out<int64_t> obi, oinc, odepth, olevel;
    Out<double> obf, orad, odist, oentry;
    if ((rc = obi.open(mem, g.bi, B * BI_N, "branch integers")) || (rc = obf.open(mem, g.bf, B * BF_N, "branch sums")) ||
        (rc = orad.open(mem, g.radius, N, "node radii")) || (rc = oinc.open(mem, g.incident, 3 * N, "incident branches"))) return rc;
    if (B) k_mor_branch<<<grid_for(16 * B, 4 * GRID_LIST), TPB>>>(off, B, vox, dist, s, g.local_steps, obi.dev, obf.dev);
    if (g.entry_radius && total) {
        if ((rc = oentry.open(mem, g.entry_radius, (size_t)total, "entry radii"))) return rc;
        k_mor_gather<<<grid_for((u64)total, 4 * GRID_LIST), TPB>>>(vox, (u64)total, dist, oentry.dev);
    }
    if (N) {
        Incident t{nullptr, nullptr, nullptr, nullptr};
        VMASK_GRAB(t.deg, N, "end counts"); VMASK_GRAB(t.lo, N, "incident ends"); VMASK_GRAB(t.hi, N, "incident ends"); VMASK_GRAB(t.sum, N, "incident ends");
        VMASK_TRY(hipMemsetAsync(t.deg, 0, N * sizeof(uint32_t), 0)); VMASK_TRY(hipMemsetAsync(t.lo, 0xff, N * sizeof(u64), 0));
        VMASK_TRY(hipMemsetAsync(t.hi, 0, N * sizeof(u64), 0)); VMASK_TRY(hipMemsetAsync(t.sum, 0, N * sizeof(u64), 0));
        if (B) k_mor_incident<<<grid_for(2 * B, GRID_LIST), TPB>>>(ends, B, N, t);
        k_mor_node<<<grid_for(N, GRID_LIST), TPB>>>(nodevox, N, dist, t, orad.dev, oinc.dev);
    }
    VMASK_TRY(hipGetLastError());
    // the path lengths: on the host from the integer counts, in the stated order, and back for the depth
    if (B) try {
        std::vector<int64_t> hbi(B * BI_N);
        std::vector<double> hbf(B * BF_N);
        VMASK_TRY(hipMemcpy(hbi.data(), obi.dev, hbi.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        VMASK_TRY(hipMemcpy(hbf.data(), obf.dev, hbf.size() * sizeof(double), hipMemcpyDeviceToHost));
        double wc[7];
        for (int c = 0; c < 7; c++) {
            const int64_t o[3] = {((c + 1) >> 2) & 1, ((c + 1) >> 1) & 1, (c + 1) & 1};
            wc[c] = length_of(o, h);
        }
        for (u64 b = 0; b < B; b++) {
            const int64_t* o = &hbi[b * BI_N];
            double len = 0.0;
            for (int c = 0; c < 7; c++) len = len + (double)o[BI_STEP + c] * wc[c];
            len = len + length_of(o + BI_JUMP_OFFSET, h);
            len = len + length_of(o + BI_JUMP_OFFSET + 3, h);
            hbf[b * BF_N + BF_PATH] = len;
        }
        if (obf.dev == obf.user || R) VMASK_TRY(hipMemcpy(obf.dev, hbf.data(), hbf.size() * sizeof(double), hipMemcpyHostToDevice));
        if (obi.dev != obi.user) std::copy(hbi.begin(), hbi.end(), obi.user);
        if (obf.dev != obf.user) std::copy(hbf.begin(), hbf.end(), obf.user);
    } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (branch tables)"); return VRG_E_MEM; }
    if ((rc = orad.close()) || (rc = oinc.close()) || (rc = oentry.close())) return rc;

    int64_t rounds[2] = {0, 0};
    if (R) {
        if ((rc = odist.open(mem, g.distance, N, "path distances")) || (rc = odepth.open(mem, g.depth, 3 * N, "node depths")) ||
            (rc = olevel.open(mem, g.level, B, "branch levels"))) return rc;
        u64* D = reinterpret_cast<u64*>(odist.dev);
        int32_t* stamp = nullptr;
        VMASK_GRAB(stamp, N, "level stamps");
        const int gn = grid_for(N, GRID_LIST), gb = grid_for(B, GRID_LIST);
        k_mor_fill<<<gn, TPB>>>(D, N);
        VMASK_TRY(hipMemsetAsync(odepth.dev, 0xff, 3 * N * sizeof(int64_t), 0));
        VMASK_TRY(hipMemsetAsync(stamp, 0x7f, N * sizeof(int32_t), 0));
        k_mor_roots<<<grid_for(R, GRID_LIST), TPB>>>(roots, R, N, D, odepth.dev, stamp);
        const int64_t limit = std::max<int64_t>((int64_t)N, 1);
        for (u64 lowered = 1; B && lowered;) {
            if (rounds[0] == limit) { vmask::set_error("the path distances did not settle within one round per node"); return VRG_E_INTERNAL; }
            VMASK_TRY(hipMemsetAsync(ctr, 0, sizeof(u64), 0));
            k_mor_relax<<<gb, TPB>>>(ends, obf.dev, B, N, D, ctr);
            VMASK_TRY(hipMemcpy(&lowered, ctr, sizeof(u64), hipMemcpyDeviceToHost));
            rounds[0]++;
        }
        if (B) k_mor_parent<<<gb, TPB>>>(ends, obf.dev, B, N, D, odepth.dev);
        for (u64 set = 1; B && set;) {
            if (rounds[1] == limit) { vmask::set_error("the depth levels did not settle within one round per node"); return VRG_E_INTERNAL; }
            VMASK_TRY(hipMemsetAsync(ctr, 0, sizeof(u64), 0));
            k_mor_level<<<gn, TPB>>>(ends, off, B, N, (int32_t)(rounds[1] + 1), odepth.dev, stamp, ctr);
            VMASK_TRY(hipMemcpy(&set, ctr, sizeof(u64), hipMemcpyDeviceToHost));
            rounds[1]++;
        }
        if (B) k_mor_finish<<<gb, TPB>>>(ends, B, N, odepth.dev, olevel.dev);
        VMASK_TRY(hipGetLastError());
        if ((rc = odist.close()) || (rc = odepth.close()) || (rc = olevel.close())) return rc;
    }
    if (g.counts && (rc = put(g.counts, rounds, 2))) return rc;
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_morphometry(int device, int64_t n0, int64_t n1, int64_t n2, const double* dist,
                                 const int64_t* offsets, int64_t nbranch, const int64_t* voxels, const int64_t* branch_ends,
                                 const int64_t* node_voxel, int64_t nnode, const double* spacing,
                                 const int64_t* roots, int64_t nroots, int64_t local_steps,
                                 int64_t* branch_int, double* branch_f64, double* node_radius, int64_t* incident, double* entry_radius,
                                 double* path_distance, int64_t* node_depth, int64_t* branch_level, int64_t* counts) {
    if (!dist) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nbranch < 0 || nnode < 0 || nroots < 0 || nbranch >= ((int64_t)1 << 31) || nnode >= ((int64_t)1 << 31)) { vmask::set_error("negative or oversized count"); return VRG_E_ARG; }
    if (local_steps < 1) { vmask::set_error("local_steps must be at least 1"); return VRG_E_ARG; }
    if (nbranch && (!offsets || !voxels || !branch_ends || !branch_int || !branch_f64)) { vmask::set_error("null pointer (branch tables)"); return VRG_E_ARG; }
    if (nnode && (!node_voxel || !node_radius || !incident)) { vmask::set_error("null pointer (node tables)"); return VRG_E_ARG; }
    if (nroots && (!roots || (nnode && (!path_distance || !node_depth)) || (nbranch && !branch_level))) { vmask::set_error("null pointer (depth tables)"); return VRG_E_ARG; }
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
    const Vol s{(uint32_t)n1, (uint32_t)n2, (u64)n0 * (u64)n1 * (u64)n2};
    const Args g{dist, offsets, nbranch, voxels, branch_ends, node_voxel, nnode, roots, nroots, local_steps,
                 branch_int, branch_f64, node_radius, incident, entry_radius, path_distance, node_depth, branch_level, counts};
    return morphometry(g, s, h);
}
