// vtube_device.hip - vmask_tubes of include/vmask.h: the branch table with sub-voxel centre points and radii rasterised to a
// volume - per voxel the label of the primitive (a segment swept by a ball of linearly changing radius) it lies deepest in by
// the power distance f, per branch the voxels won and how many of them the mask has ("f21 tube model").
//
//   k_tube_check   the tables are looked at before anything is written: offsets, labels, every coordinate and radius
//   k_tube_owner   per entry e the branch that primitive e (entries e, e + 1) belongs to, -1 where e is the last entry of its
//                  branch or the branch is dropped
//   k_tube_bin     ONE wave per primitive: its conservative index box (prim_box), the 8x8x8 bricks of vbrick.h's geometry that
//                  the box meets dealt to the lanes; <false> counts per brick (one integer atomic per pair), <true> fills the
//                  brick lists behind the scan, taking the places of a list from its end.  The order inside a list is whatever
//                  the atomics make it; the winner rule does not see it
//   k_tube_stats   the number of pairs, of occupied bricks and the longest list: what the host reads before it allocates the lists;
//                  the exclusive scan of the counts over the bricks is rocprim's
//   k_tube_occupied   the list of the occupied bricks
//   k_tube_eval    one workgroup of 512 threads per occupied brick, one voxel per thread, a wave per 8x8 slice.  The list goes
//                  through LDS in chunks of 256 records (A, d, dd, rA, rB - rA: 72 bytes, beside them the entry and the box along
//                  axis 0); every lane reads the same record (an LDS broadcast) and keeps (f, e) in registers; a wave skips a
//                  record whose box misses its slice.  label, field, nearest are stored once; sizes and overlap take one atomic
//                  per distinct branch of a wave
//   k_tube_fill    the voxels of the bricks with an empty list: 0, +inf, -1, and the mask voxels there counted as missed; four voxels
//                  and one 16-byte store per thread where n2 is a multiple of 4 and the arrays are aligned, else one voxel
// Everything that reaches an output is a minimum over a set or an integer sum: repeats are bit-identical.  Nothing here is
// contracted into an FMA; the division is the correctly rounded one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>                               // (rocprim.hpp calls memset without it)
#include <rocprim/rocprim.hpp>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vbrick.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vmask_wave.h"

#pragma clang fp contract(off)

namespace {

constexpr int CHUNK = 256;                         // records of a brick list in LDS at a time
constexpr int REC = 9;                             // doubles of a record: A, d, dd, rA, rB - rA
constexpr int64_t MAX_PAIRS = 0x7fffffffll;
enum { C_TABLE = 0, C_FINITE, C_NEGATIVE, C_RANGE, C_LABEL, C_PRIMS, C_PAIRS, C_OCCUPIED, C_LONGEST, C_CURSOR, C_MISSED, C_N };
enum { T_CHECK = 0, T_COUNT, T_SCAN, T_LISTS, T_EVAL, T_FILL, T_N };

struct Par { double h[3]; };

// The index box of the primitive (A, rA) - (B, rB): per axis from min(A - rA, B - rB) to max(A + rA, B + rB) in voxels, one voxel
// wider, clipped to the volume.  false: it misses the volume.  (The arguments are finite and at most 2^20 max(h): k_tube_check.)
__device__ __forceinline__ bool prim_box(const double* A, const double* B, double rA, double rB, const Par& p, const Geo& g, int32_t* lo, int32_t* hi) {
    const int32_t n[3] = {g.n0, g.n1, g.n2};
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double l = floor(fmin(A[a] - rA, B[a] - rB) / p.h[a]) - 1.0, u = ceil(fmax(A[a] + rA, B[a] + rB) / p.h[a]) + 1.0;
        const double last = (double)(n[a] - 1);
        if (u < 0.0 || l > last) any = false;
        lo[a] = (int32_t)fmin(fmax(l, 0.0), last);
        hi[a] = (int32_t)fmin(fmax(u, 0.0), last);
    }
    return any;
}

__global__ void __launch_bounds__(TPB) k_tube_check(const int64_t* __restrict__ off, u64 B, u64 E, const double* __restrict__ P, const double* __restrict__ r,
                                                    const int32_t* __restrict__ blabel, double most, u64* __restrict__ ctr) {
    u64 table = 0, finite = 0, negative = 0, range = 0, label = 0;
    const u64 items = B > E ? B : E;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < items; i += (u64)gridDim.x * TPB) {
        if (i < B) {
            const int64_t a = off[i], b = off[i + 1];
            table += a < 0 || b - a < 2 || (u64)b > E || (i == 0 && a != 0);
            if (blabel) label += blabel[i] <= 0;
        }
        if (i < E) {
            const double v[4] = {P[3 * i], P[3 * i + 1], P[3 * i + 2], r[i]};
            bool f = false, q = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool fin = fabs(v[k]) <= 1.7976931348623157e308;          // (false for a NaN)
                f |= !fin;
                q |= fin && fabs(v[k]) > most;
            }
            finite += f; range += q;
            negative += v[3] < 0.0;
        }
    }
    wave_add(ctr + c_at(C_TABLE), table); wave_add(ctr + c_at(C_FINITE), finite); wave_add(ctr + c_at(C_NEGATIVE), negative);
    wave_add(ctr + c_at(C_RANGE), range); wave_add(ctr + c_at(C_LABEL), label);
}

__global__ void __launch_bounds__(TPB) k_tube_owner(const int64_t* __restrict__ off, u64 B, u64 E, const uint8_t* __restrict__ keep, int32_t* __restrict__ owner,
                                                    u64* __restrict__ ctr) {
    u64 prims = 0;
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < E; e += (u64)gridDim.x * TPB) {
        u64 lo = 0, hi = B - 1;                                                   // the last branch with off <= e
        while (lo < hi) {
            const u64 mid = (lo + hi + 1) >> 1;
            if ((u64)off[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const bool is = e + 1 < (u64)off[lo + 1] && (!keep || keep[lo]);
        owner[e] = is ? (int32_t)lo : -1;
        prims += is;
    }
    wave_add(ctr + c_at(C_PRIMS), prims);
}

template <bool FILL>
__global__ void __launch_bounds__(TPB) k_tube_bin(u64 E, const int32_t* __restrict__ owner, const double* __restrict__ P, const double* __restrict__ r, Par p, Geo g,
                                                  uint32_t* __restrict__ cnt, const uint32_t* __restrict__ start, uint32_t* __restrict__ list) {
    const uint32_t lane = lane_id();
    const u64 waves = (u64)gridDim.x * (TPB / 64);
    for (u64 e = (u64)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); e < E; e += waves) {        // (the same trips in every lane of a wave)
        if (owner[e] < 0) continue;
        const double A[3] = {P[3 * e], P[3 * e + 1], P[3 * e + 2]}, Bp[3] = {P[3 * e + 3], P[3 * e + 4], P[3 * e + 5]};
        int32_t lo[3], hi[3];
        if (!prim_box(A, Bp, r[e], r[e + 1], p, g, lo, hi)) continue;
        const uint32_t b0 = (uint32_t)lo[0] >> 3, b1 = (uint32_t)lo[1] >> 3, b2 = (uint32_t)lo[2] >> 3;
        const uint32_t m1 = ((uint32_t)hi[1] >> 3) - b1 + 1u, m2 = ((uint32_t)hi[2] >> 3) - b2 + 1u;
        const uint32_t cells = (((uint32_t)hi[0] >> 3) - b0 + 1u) * m1 * m2;      // (at most the bricks of the volume: < 2^23)
        for (uint32_t c = lane; c < cells; c += 64u) {
            const uint32_t q = c / m2, c2 = c - q * m2, c0 = q / m1, c1 = q - c0 * m1;
            const uint32_t brick = ((b0 + c0) * (uint32_t)g.B1 + (b1 + c1)) * (uint32_t)g.B2 + (b2 + c2);
            if (FILL) list[start[brick] + atomicSub(&cnt[brick], 1u) - 1u] = (uint32_t)e;
            else atomicAdd(&cnt[brick], 1u);
        }
    }
}

// ---- what the host needs before it allocates the lists: the pairs, the occupied bricks, the longest list
__global__ void __launch_bounds__(TPB) k_tube_stats(const uint32_t* __restrict__ cnt, uint32_t nbricks, u64* __restrict__ ctr) {
    u64 pairs = 0, occupied = 0, longest = 0;
    for (uint32_t b = blockIdx.x * TPB + threadIdx.x; b < nbricks; b += gridDim.x * TPB) {
        const uint32_t c = cnt[b];
        pairs += c; occupied += c != 0u; longest = longest > c ? longest : c;
    }
    wave_add(ctr + c_at(C_PAIRS), pairs); wave_add(ctr + c_at(C_OCCUPIED), occupied);
    if (longest) atomicMax(ctr + c_at(C_LONGEST), longest);
}
// the occupied bricks, compacted: one atomic per wave; the order is not deterministic and cannot show in an output
__global__ void __launch_bounds__(TPB) k_tube_occupied(const uint32_t* __restrict__ cnt, uint32_t nbricks, uint32_t* __restrict__ occ, u64* __restrict__ ctr) {
    for (uint32_t b0 = blockIdx.x * TPB; b0 < nbricks; b0 += gridDim.x * TPB) {             // (the same trips in every lane of a wave)
        const uint32_t b = b0 + threadIdx.x;
        const bool has = b < nbricks && cnt[b] != 0u;
        uint32_t total;
        const uint32_t at = wave_scan(has ? 1u : 0u, total);
        if (!total) continue;
        const u64 first = wave_reserve(ctr + c_at(C_CURSOR), total);
        if (has) occ[first + at] = b;                                                     // (as many as k_tube_stats counted)
    }
}

// ---- the voxels
__global__ void __launch_bounds__(BRICK) k_tube_eval(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                     const double* __restrict__ P, const double* __restrict__ r, const int32_t* __restrict__ owner,
                                                     const int32_t* __restrict__ blabel, const uint8_t* __restrict__ mask, Par p, Geo g,
                                                     int32_t* __restrict__ label, double* __restrict__ field, int64_t* __restrict__ nearest,
                                                     u64* __restrict__ sizes, u64* __restrict__ overlap, u64* __restrict__ ctr) {
    __shared__ double sR[CHUNK * REC];
    __shared__ int32_t sE[CHUNK], sLo[CHUNK], sHi[CHUNK];
    const uint32_t t = threadIdx.x, b = occ[blockIdx.x];
    const Brick3 at = brick_coords(b, g);
    const int32_t slice = at.b0 * 8 + (int32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));      // the wave's i0
    const int32_t i1 = at.b1 * 8 + (int32_t)((t >> 3) & 7u), i2 = at.b2 * 8 + (int32_t)(t & 7u);
    const bool in = slice < g.n0 && i1 < g.n1 && i2 < g.n2;
    const double x0 = (double)slice * p.h[0], x1 = (double)i1 * p.h[1], x2 = (double)i2 * p.h[2];
    const uint32_t first = start[b], n = start[b + 1] - first;
    double best = INFINITY;
    int32_t who = -1;
    for (uint32_t base = 0; base < n; base += CHUNK) {
        const uint32_t m = n - base < (uint32_t)CHUNK ? n - base : (uint32_t)CHUNK;
        __syncthreads();                                                          // (the chunk before is read)
        if (t < m) {
            const uint32_t e = list[first + base + t];
            const double A[3] = {P[3 * (size_t)e], P[3 * (size_t)e + 1], P[3 * (size_t)e + 2]};
            const double Bp[3] = {P[3 * (size_t)e + 3], P[3 * (size_t)e + 4], P[3 * (size_t)e + 5]};
            const double rA = r[e], rB = r[e + 1];
            const double d0 = Bp[0] - A[0], d1 = Bp[1] - A[1], d2 = Bp[2] - A[2];
            double* const rec = sR + t * REC;
            rec[0] = A[0]; rec[1] = A[1]; rec[2] = A[2]; rec[3] = d0; rec[4] = d1; rec[5] = d2;
            rec[6] = (d0 * d0 + d1 * d1) + d2 * d2; rec[7] = rA; rec[8] = rB - rA;
            int32_t lo[3], hi[3];
            (void)prim_box(A, Bp, rA, rB, p, g, lo, hi);                          // (it met this brick: not empty)
            sE[t] = (int32_t)e; sLo[t] = lo[0]; sHi[t] = hi[0];
        }
        __syncthreads();
        for (uint32_t k = 0; k < m; k++) {
            if (slice < sLo[k] || slice > sHi[k]) continue;                       // (the same in every lane of the wave)
            const double* const rec = sR + k * REC;
            const double A0 = rec[0], A1 = rec[1], A2 = rec[2], d0 = rec[3], d1 = rec[4], d2 = rec[5], dd = rec[6];
            const double w0 = x0 - A0, w1 = x1 - A1, w2 = x2 - A2;
            const double wd = (w0 * d0 + w1 * d1) + w2 * d2;
            double tt = dd == 0.0 ? 0.0 : wd / dd;
            tt = tt > 0.0 ? tt : 0.0;
            tt = tt > 1.0 ? 1.0 : tt;
            const double c0 = A0 + tt * d0, c1 = A1 + tt * d1, c2 = A2 + tt * d2;
            const double q0 = x0 - c0, q1 = x1 - c1, q2 = x2 - c2;
            const double qq = (q0 * q0 + q1 * q1) + q2 * q2;
            const double rho = rec[7] + tt * rec[8];
            const double f = qq - rho * rho;
            const int32_t e = sE[k];
            if (f <= 0.0 && (f < best || (f == best && e < who))) { best = f; who = e; }
        }
    }
    // ---- the voxel's outputs; the counts: one atomic per distinct branch of the wave
    const size_t idx = ((size_t)slice * (size_t)g.n1 + (size_t)i1) * (size_t)g.n2 + (size_t)i2;
    const bool won = in && who >= 0;
    const int32_t br = won ? owner[who] : -1;
    const bool masked = in && mask && mask[idx] != 0;
    if (in) {
        label[idx] = won ? (blabel ? blabel[br] : br + 1) : 0;
        if (field) field[idx] = best;
        if (nearest) nearest[idx] = (int64_t)who;
    }
    wave_add(ctr + c_at(C_MISSED), (u64)(masked && !won));
    u64 left = __ballot(won);
    while (left) {                                                                // (the same trips in every lane of the wave)
        const int32_t lead = __shfl(br, __ffsll((long long)left) - 1, 64);
        const bool mine = won && br == lead;
        const u64 same = __ballot(mine), inside = __ballot(mine && masked);
        if (lane_id() == (uint32_t)(__ffsll((long long)left) - 1)) {
            atomicAdd(sizes + lead, (u64)__popcll(same));
            if (inside) atomicAdd(overlap + lead, (u64)__popcll(inside));
        }
        left &= ~same;
    }
}

// start == nullptr: no brick has a list.  VEC = 4: n2 is a multiple of 4 and the arrays are aligned, so four consecutive voxels lie in
// one row and one brick and take one 16-byte store per output
template <int VEC>
__global__ void __launch_bounds__(TPB) k_tube_fill(const uint32_t* __restrict__ start, Geo g, uint32_t V, const uint8_t* __restrict__ mask,
                                                   int32_t* __restrict__ label, double* __restrict__ field, int64_t* __restrict__ nearest, u64* __restrict__ ctr) {
    u64 missed = 0;
    const u64 items = V / VEC;
    for (u64 k = (u64)blockIdx.x * TPB + threadIdx.x; k < items; k += (u64)gridDim.x * TPB) {
        const u64 i = k * VEC;
        if (start) {
            uint32_t brick, local;
            locate((uint32_t)i, g, brick, local);
            if (start[brick + 1] != start[brick]) continue;
        }
        if (VEC == 4) {
            *reinterpret_cast<int4*>(label + i) = make_int4(0, 0, 0, 0);
            if (field) {
                const double2 none = make_double2(INFINITY, INFINITY);
                reinterpret_cast<double2*>(field + i)[0] = none; reinterpret_cast<double2*>(field + i)[1] = none;
            }
            if (nearest) {
                const longlong2 none = make_longlong2(-1, -1);
                reinterpret_cast<longlong2*>(nearest + i)[0] = none; reinterpret_cast<longlong2*>(nearest + i)[1] = none;
            }
            if (mask) missed += (u64)__popc(nz4(*reinterpret_cast<const uint32_t*>(mask + i)));
        } else {
            label[i] = 0;
            if (field) field[i] = INFINITY;
            if (nearest) nearest[i] = -1;
            if (mask) missed += mask[i] != 0;
        }
    }
    wave_add(ctr + c_at(C_MISSED), missed);
}
inline bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

struct Events {
    hipEvent_t e[8] = {};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

int tubes(const Geo& g, const Par& p, const int64_t* offsets, int64_t nbranch, const double* positions, const double* radius, const uint8_t* keep,
          const int32_t* branch_label, const uint8_t* mask, int32_t* label, double* field, int64_t* nearest, int64_t* sizes, int64_t* overlap,
          int64_t* missed, int64_t* counts, double* step_ms) {
    const u64 B = (u64)nbranch, V = (u64)g.n0 * (u64)g.n1 * (u64)g.n2;
    const uint32_t nbricks = (uint32_t)g.B0 * (uint32_t)g.B1 * (uint32_t)g.B2;
    DevMem mem;
    int rc;
    u64 E = 0;
    if (B) {
        int64_t edge[2] = {0, 0};
        if (vmask::is_device_pointer(offsets)) {
            VMASK_TRY(hipMemcpy(&edge[0], offsets, sizeof(int64_t), hipMemcpyDeviceToHost));
            VMASK_TRY(hipMemcpy(&edge[1], offsets + B, sizeof(int64_t), hipMemcpyDeviceToHost));
        } else { edge[0] = offsets[0]; edge[1] = offsets[B]; }
        if (edge[0] != 0 || edge[1] < 2 * (int64_t)B || edge[1] > MAX_PAIRS) { vmask::set_error("offsets do not describe branches of at least two entries (fewer than 2^31 in all)"); return VRG_E_ARG; }
        E = (u64)edge[1];
    }
    const int64_t* off = nullptr; const double* P = nullptr; const double* r = nullptr;
    const uint8_t* kp = nullptr; const int32_t* bl = nullptr; const uint8_t* mk = nullptr;
    if ((rc = bring(mem, offsets, B ? B + 1 : 0, "offsets", &off)) || (rc = bring(mem, positions, (size_t)E * 3, "centre points", &P)) ||
        (rc = bring(mem, radius, (size_t)E, "radii", &r)) || (rc = bring(mem, keep, keep ? B : 0, "keep", &kp)) ||
        (rc = bring(mem, branch_label, branch_label ? B : 0, "branch labels", &bl)) || (rc = bring(mem, mask, mask ? (size_t)V : 0, "mask", &mk))) return rc;
    if (!B) { kp = nullptr; bl = nullptr; }
    u64* ctr = nullptr;
    VMASK_GRAB(ctr, C_N * C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(ctr, 0, C_N * C_PITCH * sizeof(u64), 0));
    Events ev;
    for (hipEvent_t& x : ev.e) VMASK_TRY(hipEventCreate(&x));
    float ms[T_N] = {};
    u64 seen[C_N * C_PITCH];
    // ---- the tables
    if (B) {
        const double most = 0x1p20 * std::max({p.h[0], p.h[1], p.h[2]});
        VMASK_TRY(hipEventRecord(ev.e[0], 0));
        k_tube_check<<<grid_for((std::max(B, E) + TPB - 1) / TPB, 1024), TPB>>>(off, B, E, P, r, bl, most, ctr);
        VMASK_TRY(hipEventRecord(ev.e[1], 0));
        VMASK_TRY(hipMemcpy(seen, ctr, sizeof(seen), hipMemcpyDeviceToHost));
        VMASK_TRY(hipEventElapsedTime(&ms[T_CHECK], ev.e[0], ev.e[1]));
        if (seen[c_at(C_TABLE)]) { vmask::set_error("the branch table is malformed: offsets must start at 0 and give every branch at least two entries"); return VRG_E_ARG; }
        if (seen[c_at(C_FINITE)]) { vmask::set_error("a coordinate or radius is not finite"); return VRG_E_ARG; }
        if (seen[c_at(C_NEGATIVE)]) { vmask::set_error("a radius is negative"); return VRG_E_ARG; }
        if (seen[c_at(C_RANGE)]) { vmask::set_error("a coordinate or radius is above 2^20 times the largest spacing"); return VRG_E_ARG; }
        if (seen[c_at(C_LABEL)]) { vmask::set_error("a branch label is not positive"); return VRG_E_ARG; }
    }
    // ---- the outputs
    Out<int32_t> olabel;
    Out<double> ofield;
    Out<int64_t> onearest, osizes, ooverlap;
    if ((rc = olabel.open(mem, label, (size_t)V, "labels")) || (field && (rc = ofield.open(mem, field, (size_t)V, "field"))) ||
        (nearest && (rc = onearest.open(mem, nearest, (size_t)V, "nearest"))) || (B && (rc = osizes.open(mem, sizes, B, "sizes"))) ||
        (B && (rc = ooverlap.open(mem, overlap, B, "overlap")))) return rc;
    // ---- the bricks of every primitive
    uint32_t* start = nullptr;
    u64 prims = 0, pairs = 0, nocc = 0, longest = 0;
    if (B) {
        int32_t* owner = nullptr;
        uint32_t* cnt = nullptr; uint32_t* occ = nullptr; uint32_t* list = nullptr;
        VMASK_GRAB(owner, (size_t)E, "owners");
        VMASK_GRAB(cnt, (size_t)nbricks + 1, "brick counts");                             // (one more, 0: the scan's last entry is the total)
        VMASK_GRAB(start, (size_t)nbricks + 1, "brick lists' starts");
        VMASK_TRY(hipMemsetAsync(cnt, 0, ((size_t)nbricks + 1) * sizeof(uint32_t), 0));
        const int gbin = grid_for((E + TPB / 64 - 1) / (TPB / 64), GRID_CAP), gbricks = grid_for(((u64)nbricks + TPB - 1) / TPB, 1024);
        VMASK_TRY(hipEventRecord(ev.e[0], 0));
        k_tube_owner<<<grid_for((E + TPB - 1) / TPB, 1024), TPB>>>(off, B, E, kp, owner, ctr);
        k_tube_bin<false><<<gbin, TPB>>>(E, owner, P, r, p, g, cnt, nullptr, nullptr);
        VMASK_TRY(hipEventRecord(ev.e[1], 0));
        k_tube_stats<<<gbricks, TPB>>>(cnt, nbricks, ctr);
        VMASK_TRY(hipMemcpy(seen, ctr, sizeof(seen), hipMemcpyDeviceToHost));
        prims = seen[c_at(C_PRIMS)]; pairs = seen[c_at(C_PAIRS)]; nocc = seen[c_at(C_OCCUPIED)]; longest = seen[c_at(C_LONGEST)];
        if (pairs > (u64)MAX_PAIRS) { vmask::set_error("more than 2^31 - 1 (brick, primitive) pairs: the tubes are too many or too wide for one call"); return VRG_E_ARG; }
        VMASK_TRY(hipEventElapsedTime(&ms[T_COUNT], ev.e[0], ev.e[1]));
        VMASK_TRY(hipMemsetAsync(osizes.dev, 0, B * sizeof(int64_t), 0));                 // (nothing of the caller's is written before this line)
        VMASK_TRY(hipMemsetAsync(ooverlap.dev, 0, B * sizeof(int64_t), 0));
        if (nocc) {
            uint8_t* tmp = nullptr;
            size_t tb = 0;
            VMASK_TRY(rocprim::exclusive_scan(nullptr, tb, cnt, start, 0u, (size_t)nbricks + 1, rocprim::plus<uint32_t>()));
            VMASK_GRAB(tmp, tb, "scan space");
            VMASK_GRAB(list, (size_t)pairs, "brick lists");
            VMASK_GRAB(occ, (size_t)nocc, "occupied bricks");
            VMASK_TRY(hipEventRecord(ev.e[2], 0));
            VMASK_TRY(rocprim::exclusive_scan(tmp, tb, cnt, start, 0u, (size_t)nbricks + 1, rocprim::plus<uint32_t>()));
            k_tube_occupied<<<gbricks, TPB>>>(cnt, nbricks, occ, ctr);
            VMASK_TRY(hipEventRecord(ev.e[3], 0));
            k_tube_bin<true><<<gbin, TPB>>>(E, owner, P, r, p, g, cnt, start, list);
            VMASK_TRY(hipEventRecord(ev.e[4], 0));
            k_tube_eval<<<(int)nocc, BRICK>>>(occ, start, list, P, r, owner, bl, mk, p, g, olabel.dev, field ? ofield.dev : nullptr,
                                              nearest ? onearest.dev : nullptr, (u64*)osizes.dev, (u64*)ooverlap.dev, ctr);
            VMASK_TRY(hipEventRecord(ev.e[5], 0));
        } else start = nullptr;
    }
    VMASK_TRY(hipEventRecord(ev.e[6], 0));
    double* const dfield = field ? ofield.dev : nullptr;
    int64_t* const dnearest = nearest ? onearest.dev : nullptr;
    if (g.n2 % 4 == 0 && aligned(olabel.dev, 16) && aligned(dfield, 16) && aligned(dnearest, 16) && aligned(mk, 4))
        k_tube_fill<4><<<grid_for((V / 4 + TPB - 1) / TPB, GRID_CAP), TPB>>>(start, g, (uint32_t)V, mk, olabel.dev, dfield, dnearest, ctr);
    else
        k_tube_fill<1><<<grid_for((V + TPB - 1) / TPB, GRID_CAP), TPB>>>(start, g, (uint32_t)V, mk, olabel.dev, dfield, dnearest, ctr);
    VMASK_TRY(hipEventRecord(ev.e[7], 0));
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipMemcpy(seen, ctr, sizeof(seen), hipMemcpyDeviceToHost));
    if (nocc) {
        VMASK_TRY(hipEventElapsedTime(&ms[T_SCAN], ev.e[2], ev.e[3]));
        VMASK_TRY(hipEventElapsedTime(&ms[T_LISTS], ev.e[3], ev.e[4]));
        VMASK_TRY(hipEventElapsedTime(&ms[T_EVAL], ev.e[4], ev.e[5]));
    }
    VMASK_TRY(hipEventElapsedTime(&ms[T_FILL], ev.e[6], ev.e[7]));
    if ((rc = olabel.close()) || (field && (rc = ofield.close())) || (nearest && (rc = onearest.close())) || (B && (rc = osizes.close())) ||
        (B && (rc = ooverlap.close()))) return rc;
    const int64_t m = (int64_t)seen[c_at(C_MISSED)];
    if ((rc = put(missed, &m, 1))) return rc;
    if (counts) {
        const int64_t c[4] = {(int64_t)prims, (int64_t)nocc, (int64_t)pairs, (int64_t)longest};
        if ((rc = put(counts, c, 4))) return rc;
    }
    if (step_ms) for (int k = 0; k < T_N; k++) step_ms[k] = (double)ms[k];
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_tubes(int device, int64_t n0, int64_t n1, int64_t n2, const double* spacing, const int64_t* offsets, int64_t nbranch,
                           const double* positions, const double* radius, const uint8_t* keep, const int32_t* branch_label, const uint8_t* mask,
                           int32_t* label, double* field, int64_t* nearest, int64_t* sizes, int64_t* overlap, int64_t* missed, int64_t* counts,
                           double* step_ms) {
    if (nbranch < 0 || nbranch >= ((int64_t)1 << 30)) { vmask::set_error("negative or oversized count"); return VRG_E_ARG; }
    if (!label || !missed) { vmask::set_error("null pointer (label, missed)"); return VRG_E_ARG; }
    if (nbranch && (!offsets || !positions || !radius || !sizes || !overlap)) { vmask::set_error("null pointer (branch tables)"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Par p;
    p.h[0] = p.h[1] = p.h[2] = 1.0;
    if (spacing) {
        if (vmask::is_device_pointer(spacing)) VMASK_TRY(hipMemcpy(p.h, spacing, sizeof(p.h), hipMemcpyDeviceToHost));
        else std::copy(spacing, spacing + 3, p.h);
    }
    for (double x : p.h)
        if (!std::isfinite(x) || !(x > 0.0)) { vmask::set_error("spacing not finite and positive"); return VRG_E_ARG; }
    if (std::max({p.h[0], p.h[1], p.h[2]}) / std::min({p.h[0], p.h[1], p.h[2]}) > 1000.0) { vmask::set_error("spacing ratio above 1000"); return VRG_E_ARG; }
    return tubes(make_geo(n0, n1, n2), p, offsets, nbranch, positions, radius, keep, branch_label, mask, label, field, nearest, sizes, overlap,
                 missed, counts, step_ms);
}
