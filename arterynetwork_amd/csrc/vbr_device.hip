// vbr_device.hip - vmask_branches of include/vmask.h: the branch graph of a voxel set - junction clusters merged into single
// nodes, short spurs pruned ("f10 branch graph").
//
// One graph build works on the compacted object voxels ("slots", vseg_slots.h) and on the segments that vmask_segments
// returns for the same volume (called with device pointers):
//   k_seg_count / k_seg_compact  list the object voxels, idx -> slot into the hash table (vseg_slots.h)
//   k_br_gather                  the 27-bit neighbourhood word of every slot; a junction voxel (deg >= 3) starts as its own
//                                parent: P = idx << 32 | slot, so that the order of the packed words is the order of idx
//   k_br_adjacent                the bits of a junction's word whose neighbour is a junction too (looked up once)
//   k_br_hook                    one labelling round, in place: the parent of v takes the smallest grandparent found among v's
//                                junction neighbours (hooking by atomicMin), v itself takes the smallest of those and of its own
//                                grandparent (shortcut).  Parents only descend and always name a member of the same cluster; a
//                                round that lowers nothing has every P equal to the cluster's smallest (idx, slot).  The host
//                                reads one counter per round.  No thread walks a chain of parents.
//   k_br_members                 per cluster (at the slot of its label): member count, representative = atomicMax of
//                                (deg << 32 | ~idx)
//   k_br_classify                one thread per segment: the end nodes through the hash table, the intra-cluster flag, the
//                                branch ends counted at the nodes, the emitted length, the spur test and the packed
//                                atomicMin (L << 32 | segment) per cluster
//   k_br_clear                   one thread per segment entry: the voxels of the selected spurs leave the volume
//   k_br_nodes                   end points and cluster labels compacted into node records (sorted by representative on the
//                                host: the records alone travel), k_br_nodeid scatters the node ids back to the slots
//   k_br_emit                    one thread per segment entry writes the branch voxels behind two prefix sums over the segments
//                                (rocPRIM), the entry at position 0 also the representatives, the offset and the two node ids
// Between two builds of a pruning round the volume is thinned by vmask_skeleton in place.
#include <hip/hip_runtime.h>
#include <cstring>                               // (rocprim.hpp calls memset without it)
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vseg_slots.h"

namespace {

constexpr int MAX_LABEL_ROUNDS = 96;
constexpr uint32_t KEEP_LAST = 1u << 31;           // in a spur's cluster word: the cluster is at the segment's last voxel
enum { SF_PRE = 1u, SF_POST = 2u, SF_RING = 4u };  // per segment: representative in front / behind, closed curve without a node

enum { C_OBJ = 0, C_CURSOR, C_ISO, C_NODES, C_CLUSTERS, C_ENDPTS, C_PASS, C_BRANCH, C_ENTRIES, C_DROPPED, C_SPURS, C_VOXELS,
       C_LABEL /* [MAX_LABEL_ROUNDS]: parents lowered */, C_N = C_LABEL + MAX_LABEL_ROUNDS };

__host__ __device__ inline u64 pack(uint32_t hi, uint32_t lo) { return ((u64)hi << 32) | lo; }

__global__ void __launch_bounds__(TPB) k_br_binary(const uint8_t* in, uint8_t* out, u64 V) {
    for (u64 v = (u64)blockIdx.x * TPB + threadIdx.x; v < V; v += (u64)gridDim.x * TPB) out[v] = in[v] ? 1 : 0;
}

__global__ void __launch_bounds__(TPB) k_br_gather(const uint8_t* __restrict__ vol, Dim d, const uint32_t* __restrict__ list, uint32_t n,
                                                   uint32_t* __restrict__ word, u64* __restrict__ P, u64* __restrict__ ctr) {
    u64 iso = 0;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i], w = gather_word(vol, d, idx);
        word[i] = w;
        P[i] = __popc(w) >= 3 ? pack(idx, i) : ~0ull;
        iso += w == 0u;
    }
    wave_add(&ctr[c_at(C_ISO)], iso);
}

__global__ void __launch_bounds__(TPB) k_br_adjacent(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, Dim d, Hash h,
                                                     uint32_t* __restrict__ jmask) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i], w = word[i];
        uint32_t jm = 0;
        if (__popc(w) >= 3)
            for (uint32_t m = w; m; m &= m - 1u) {
                const int t = __ffs((int)m) - 1;
                const uint32_t j = h_find(h, idx + (uint32_t)bit_offset(t, d));
                if (j < n && __popc(word[j]) >= 3) jm |= 1u << t;
            }
        jmask[i] = jm;
    }
}

// P is read and lowered in the same launch: a stale read only delays, the round that lowers nothing has read the final state
__global__ void __launch_bounds__(TPB) k_br_hook(const uint32_t* __restrict__ list, const uint32_t* __restrict__ jmask, uint32_t n, Dim d, Hash h,
                                                 u64* P, u64* __restrict__ c_lowered) {
    u64 lowered = 0;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t jm = jmask[i];
        if (!jm) continue;
        const uint32_t idx = list[i];
        const u64 pi = P[i];
        const uint32_t sp = (uint32_t)pi;
        if (sp >= n) continue;                                          // (cannot happen: a junction's parent is a junction's slot)
        const u64 gi = P[sp];
        u64 best = gi;
        for (uint32_t m = jm; m; m &= m - 1u) {
            const uint32_t j = h_find(h, idx + (uint32_t)bit_offset(__ffs((int)m) - 1, d));
            if (j >= n) continue;
            const uint32_t sj = (uint32_t)P[j];
            if (sj >= n) continue;
            const u64 gj = P[sj];
            if (gj < gi && atomicMin(&P[sp], gj) > gj) lowered++;
            best = gj < best ? gj : best;
        }
        if (best < pi && atomicMin(&P[i], best) > best) lowered++;
    }
    wave_add(c_lowered, lowered);
}

__global__ void __launch_bounds__(TPB) k_br_members(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, const u64* __restrict__ P,
                                                    u64* __restrict__ rep, uint32_t* __restrict__ members) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const int deg = __popc(word[i]);
        if (deg < 3) continue;
        const uint32_t r = (uint32_t)P[i];
        if (r >= n) continue;
        atomicMax(&rep[r], pack((uint32_t)deg, ~list[i]));
        atomicAdd(&members[r], 1u);
    }
}

// the node of a voxel that ends a segment: an end point is its own, a junction voxel's is the slot of its cluster's label
__device__ __forceinline__ uint32_t node_slot(uint32_t s, int deg, const u64* __restrict__ P) { return deg >= 3 ? (uint32_t)P[s] : s; }
__device__ __forceinline__ uint32_t rep_idx(uint32_t key, const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, const u64* __restrict__ rep) {
    return __popc(word[key]) >= 3 ? ~(uint32_t)rep[key] : list[key];
}

struct Prune { int64_t min_len; double factor; const double* dist; u64 V; int on; };

__global__ void __launch_bounds__(TPB) k_br_classify(const int64_t* __restrict__ off, const int64_t* __restrict__ vox, uint32_t nseg,
                                                     const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, Hash h,
                                                     const u64* __restrict__ P, const u64* __restrict__ rep, Prune pr,
                                                     uint32_t* __restrict__ ends, u64* __restrict__ best,
                                                     uint32_t* __restrict__ elen, uint32_t* __restrict__ sflag, uint32_t* __restrict__ ska, uint32_t* __restrict__ skb,
                                                     uint32_t* __restrict__ scl, u64* __restrict__ ctr) {
    u64 branches = 0, entries = 0, dropped = 0;
    for (uint32_t k = blockIdx.x * TPB + threadIdx.x; k < nseg; k += gridDim.x * TPB) {
        const int64_t a = off[k];
        const uint32_t len = (uint32_t)(off[k + 1] - a), first = (uint32_t)vox[a], last = (uint32_t)vox[a + len - 1];
        const uint32_t sa = h_find(h, first), sb = h_find(h, last);
        uint32_t el = 0, fl = 0, ka = NONE, kb = NONE, cl = NONE;
        if (sa < n && sb < n && len >= 2u) {
            const int da = __popc(word[sa]), db = __popc(word[sb]);
            ka = node_slot(sa, da, P); kb = node_slot(sb, db, P);
            if (ka >= n || kb >= n) { ka = kb = NONE; }                 // (cannot happen)
            else if (len == 2u && da >= 3 && db >= 3 && ka == kb) dropped++;
            else {
                if (first == last && da == 2) fl = SF_RING;
                else {
                    atomicAdd(&ends[ka], 1u); atomicAdd(&ends[kb], 1u);
                    if (rep_idx(ka, list, word, rep) != first) fl |= SF_PRE;
                    if (rep_idx(kb, list, word, rep) != last) fl |= SF_POST;
                }
                el = len + (fl & SF_PRE ? 1u : 0u) + (fl & SF_POST ? 1u : 0u);
                branches++; entries += el;
                const uint32_t L = len - 1u;
                uint32_t c = NONE;
                if (da == 1 && db >= 3) c = kb | KEEP_LAST;
                else if (db == 1 && da >= 3) c = ka;
                if (pr.on && c != NONE) {
                    const uint32_t key = c & ~KEEP_LAST;
                    bool spur = (int64_t)L <= pr.min_len;
                    if (!spur && pr.dist) {
                        const uint32_t r = rep_idx(key, list, word, rep);
                        spur = r < pr.V && (double)L <= pr.factor * pr.dist[r];
                    }
                    if (spur) { cl = c; atomicMin(&best[key], pack(L, k)); }
                }
            }
        }
        elen[k] = el; sflag[k] = fl; ska[k] = ka; skb[k] = kb; scl[k] = cl;
    }
    wave_add(&ctr[c_at(C_BRANCH)], branches);
    wave_add(&ctr[c_at(C_ENTRIES)], entries);
    wave_add(&ctr[c_at(C_DROPPED)], dropped);
}

// the segment of entry e: the last k with off[k] <= e
__device__ __forceinline__ uint32_t find_segment(const int64_t* __restrict__ off, uint32_t nseg, int64_t e) {
    uint32_t lo = 0, hi = nseg;                                         // off[lo] <= e < off[hi]
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(TPB) k_br_clear(const int64_t* __restrict__ off, const int64_t* __restrict__ vox, uint32_t nseg, u64 total, u64 V,
                                                  const uint32_t* __restrict__ scl, const u64* __restrict__ best, uint32_t n,
                                                  uint8_t* __restrict__ vol, u64* __restrict__ ctr) {
    u64 spurs = 0, voxels = 0;
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < total; e += (u64)gridDim.x * TPB) {
        const uint32_t k = find_segment(off, nseg, (int64_t)e), c = scl[k];
        if (c == NONE) continue;
        const uint32_t key = c & ~KEEP_LAST;
        const int64_t a = off[k];
        const uint32_t len = (uint32_t)(off[k + 1] - a), p = (uint32_t)((int64_t)e - a);
        if (key >= n || best[key] != pack(len - 1u, k)) continue;       // not the one spur of its cluster in this round
        const uint32_t keep = (c & KEEP_LAST) ? len - 1u : 0u;
        if (p == keep) continue;
        const u64 v = (u64)vox[e];
        if (v >= V) continue;                                           // (cannot happen)
        vol[v] = 0;
        voxels++;
        spurs += p == (keep ? 0u : len - 1u);                           // counted at its end point
    }
    wave_add(&ctr[c_at(C_SPURS)], spurs);
    wave_add(&ctr[c_at(C_VOXELS)], voxels);
}

// a node record: x representative idx, y the node's slot, z members (1 for an end point) | cluster bit, w branch ends
__global__ void __launch_bounds__(TPB) k_br_nodes(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, const u64* __restrict__ P,
                                                  const u64* __restrict__ rep, const uint32_t* __restrict__ members, const uint32_t* __restrict__ ends,
                                                  uint4* __restrict__ rec, u64 cap, u64* __restrict__ ctr) {
    u64 clusters = 0, endpts = 0, pass = 0;
    for (uint32_t i0 = blockIdx.x * TPB; i0 < n; i0 += gridDim.x * TPB) {                 // (the same trips in every lane of a wave)
        const uint32_t i = i0 + threadIdx.x;
        int deg = 0;
        bool mine = false;
        if (i < n) { deg = __popc(word[i]); mine = deg == 1 || (deg >= 3 && (uint32_t)P[i] == i); }
        if (!__ballot(mine)) continue;
        uint32_t total;
        const uint32_t o = wave_scan(mine ? 1u : 0u, total);
        const u64 at = wave_reserve(&ctr[c_at(C_NODES)], total) + o;
        if (!mine) continue;
        const uint32_t e = ends[i];
        if (deg == 1) endpts++; else { clusters++; pass += e == 2u; }
        if (rec && at < cap) rec[at] = make_uint4(deg == 1 ? list[i] : ~(uint32_t)rep[i], i, deg == 1 ? 1u : (members[i] | (1u << 31)), e);
    }
    wave_add(&ctr[c_at(C_CLUSTERS)], clusters);
    wave_add(&ctr[c_at(C_ENDPTS)], endpts);
    wave_add(&ctr[c_at(C_PASS)], pass);
}

__global__ void __launch_bounds__(TPB) k_br_nodeid(const uint32_t* __restrict__ slots, uint32_t nn, uint32_t n, uint32_t* __restrict__ nodeid) {
    for (uint32_t k = blockIdx.x * TPB + threadIdx.x; k < nn; k += gridDim.x * TPB) if (slots[k] < n) nodeid[slots[k]] = k;
}

struct Positive { __host__ __device__ u64 operator()(uint32_t x) const { return x ? 1ull : 0ull; } };
struct Widen { __host__ __device__ u64 operator()(uint32_t x) const { return (u64)x; } };

__global__ void __launch_bounds__(TPB) k_br_emit(const int64_t* __restrict__ off, const int64_t* __restrict__ vox, uint32_t nseg, u64 total,
                                                 const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, const u64* __restrict__ rep,
                                                 const uint32_t* __restrict__ elen, const uint32_t* __restrict__ sflag, const uint32_t* __restrict__ ska,
                                                 const uint32_t* __restrict__ skb, const u64* __restrict__ bidx, const u64* __restrict__ voff,
                                                 const uint32_t* __restrict__ nodeid, u64 nbranch, u64 nentries,
                                                 int64_t* __restrict__ o_ends, int64_t* __restrict__ o_off, int64_t* __restrict__ o_vox) {
    for (u64 e = (u64)blockIdx.x * TPB + threadIdx.x; e < total; e += (u64)gridDim.x * TPB) {
        const uint32_t k = find_segment(off, nseg, (int64_t)e), el = elen[k];
        if (!el) continue;
        const uint32_t fl = sflag[k], p = (uint32_t)((int64_t)e - off[k]);
        const u64 b = bidx[k], o = voff[k];
        if (b >= nbranch || o + el > nentries) continue;                // (cannot happen)
        o_vox[o + (fl & SF_PRE ? 1u : 0u) + p] = vox[e];
        if (p) continue;
        const uint32_t ka = ska[k], kb = skb[k];
        o_off[b] = (int64_t)o;
        o_ends[2 * b] = (fl & SF_RING) ? -1 : (int64_t)nodeid[ka];
        o_ends[2 * b + 1] = (fl & SF_RING) ? -1 : (int64_t)nodeid[kb];
        if (fl & SF_PRE) o_vox[o] = (int64_t)rep_idx(ka, list, word, rep);
        if (fl & SF_POST) o_vox[o + el - 1u] = (int64_t)rep_idx(kb, list, word, rep);
    }
}

struct Graph {                                                          // one build: what the kernels after it need
    uint32_t n = 0, nseg = 0; u64 total = 0; int label_rounds = 0;
    u64 nodes = 0, clusters = 0, endpts = 0, pass = 0, branches = 0, entries = 0, iso = 0, dropped = 0;
};

struct Buffers {
    u64* ctr = nullptr; uint32_t* list = nullptr; u64* tab = nullptr; uint32_t* word = nullptr; uint32_t* jmask = nullptr; u64* P = nullptr;
    u64* rep = nullptr; uint32_t* members = nullptr; uint32_t* ends = nullptr; u64* best = nullptr; uint32_t* nodeid = nullptr;
    size_t cap_n = 0; int bits = 0;
    int64_t* soff = nullptr; int64_t* svox = nullptr; size_t cap_seg = 0, cap_vox = 0;
    uint32_t* elen = nullptr; uint32_t* sflag = nullptr; uint32_t* ska = nullptr; uint32_t* skb = nullptr; uint32_t* scl = nullptr; size_t cap_k = 0;
};

// the graph of the 0/1 volume vol (device); pr.on: run the spur test as well
int build_graph(int device, DevMem& mem, Buffers& b, const uint8_t* vol, Dim d, const Prune& pr, Graph& g) {
    const u64 V = (u64)d.n0 * d.n1 * d.n2;
    g = Graph();
    VMASK_TRY(hipMemsetAsync(b.ctr, 0, (size_t)C_N * C_PITCH * sizeof(u64), 0));
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(vol) & 15u);
    const uint4* base = reinterpret_cast<const uint4*>(vol - lead);
    const u64 nwords = (lead + V + 15u) / 16u;
    const int gvol = grid_for(nwords, GRID_VOLUME);
    k_seg_count<<<gvol, TPB>>>(base, nwords, lead, V, b.ctr + c_at(C_OBJ));
    u64 nobj = 0;
    VMASK_TRY(hipMemcpy(&nobj, b.ctr + c_at(C_OBJ), sizeof(u64), hipMemcpyDeviceToHost));
    if (nobj >= (1ull << 30)) { vmask::set_error("more than 2^30 object voxels"); return VRG_E_ARG; }
    const uint32_t n = g.n = (uint32_t)nobj;
    if (!n) return VRG_OK;
    if (n > b.cap_n) {                                                  // (the first build: pruning only removes voxels)
        b.bits = hash_bits(n);
        VMASK_GRAB(b.tab, (size_t)1 << b.bits, "index table");
        VMASK_GRAB(b.list, n, "voxel list"); VMASK_GRAB(b.word, n, "neighbourhoods"); VMASK_GRAB(b.jmask, n, "junction neighbours");
        VMASK_GRAB(b.P, n, "cluster labels"); VMASK_GRAB(b.rep, n, "representatives"); VMASK_GRAB(b.members, n, "member counts");
        VMASK_GRAB(b.ends, n, "branch ends"); VMASK_GRAB(b.best, n, "spur choice"); VMASK_GRAB(b.nodeid, n, "node ids");
        b.cap_n = n;
    }
    // the segments: the capacities of a curve skeleton first, the stated ones where that is too little
    int64_t sc[5] = {0, 0, 0, 0, 0};
    if (!b.cap_seg) {
        b.cap_seg = (size_t)n + 16; b.cap_vox = 2 * (size_t)n + 16;
        VMASK_GRAB(b.soff, b.cap_seg + 1, "segment offsets"); VMASK_GRAB(b.svox, b.cap_vox, "segment voxels");
    }
    int rc = vmask_segments(device, vol, d.n0, d.n1, d.n2, sc, b.soff, (int64_t)b.cap_seg, b.svox, (int64_t)b.cap_vox);
    if (rc == VRG_E_ARG && ((u64)sc[0] > b.cap_seg || (u64)sc[1] > b.cap_vox)) {
        b.cap_seg = std::max<size_t>(b.cap_seg, (size_t)sc[0]); b.cap_vox = std::max<size_t>(b.cap_vox, (size_t)sc[1]);
        VMASK_GRAB(b.soff, b.cap_seg + 1, "segment offsets"); VMASK_GRAB(b.svox, b.cap_vox, "segment voxels");
        rc = vmask_segments(device, vol, d.n0, d.n1, d.n2, sc, b.soff, (int64_t)b.cap_seg, b.svox, (int64_t)b.cap_vox);
    }
    if (rc) return rc;
    if ((u64)sc[0] >= (1ull << 31)) { vmask::set_error("more than 2^31 segments"); return VRG_E_ARG; }
    const uint32_t nseg = g.nseg = (uint32_t)sc[0];
    g.total = (u64)sc[1];
    if (nseg > b.cap_k) {
        VMASK_GRAB(b.elen, nseg, "branch lengths"); VMASK_GRAB(b.sflag, nseg, "branch flags"); VMASK_GRAB(b.ska, nseg, "branch ends");
        VMASK_GRAB(b.skb, nseg, "branch ends"); VMASK_GRAB(b.scl, nseg, "spur clusters");
        b.cap_k = nseg;
    }
    Hash h{b.tab, (uint32_t)((1ull << b.bits) - 1ull), 32u - (uint32_t)b.bits};
    VMASK_TRY(hipMemsetAsync(b.tab, 0xff, ((size_t)1 << b.bits) * sizeof(u64), 0));
    VMASK_TRY(hipMemsetAsync(b.rep, 0, (size_t)n * sizeof(u64), 0));
    VMASK_TRY(hipMemsetAsync(b.members, 0, (size_t)n * sizeof(uint32_t), 0));
    VMASK_TRY(hipMemsetAsync(b.ends, 0, (size_t)n * sizeof(uint32_t), 0));
    VMASK_TRY(hipMemsetAsync(b.best, 0xff, (size_t)n * sizeof(u64), 0));
    const int gslot = grid_for(n, GRID_LIST);
    k_seg_compact<<<gvol, TPB>>>(base, nwords, lead, V, n, b.list, h, b.ctr + c_at(C_CURSOR));
    k_br_gather<<<gslot, TPB>>>(vol, d, b.list, n, b.word, b.P, b.ctr);
    k_br_adjacent<<<gslot, TPB>>>(b.list, b.word, n, d, h, b.jmask);
    for (;;) {                                                          // until a round lowers no parent
        if (g.label_rounds == MAX_LABEL_ROUNDS) { vmask::set_error("cluster labelling did not finish"); return VRG_E_INTERNAL; }
        u64* c = b.ctr + c_at(C_LABEL + g.label_rounds);
        k_br_hook<<<gslot, TPB>>>(b.list, b.jmask, n, d, h, b.P, c);
        u64 lowered = 0;
        VMASK_TRY(hipMemcpy(&lowered, c, sizeof(u64), hipMemcpyDeviceToHost));
        g.label_rounds++;
        if (!lowered) break;
    }
    k_br_members<<<gslot, TPB>>>(b.list, b.word, n, b.P, b.rep, b.members);
    if (nseg)
        k_br_classify<<<grid_for(nseg, GRID_LIST), TPB>>>(b.soff, b.svox, nseg, b.list, b.word, n, h, b.P, b.rep, pr, b.ends, b.best,
                                                          b.elen, b.sflag, b.ska, b.skb, b.scl, b.ctr);
    return VRG_OK;
}

int branches(int device, const uint8_t* volume, Dim d, int64_t min_len, double factor, const double* dist, int64_t max_rounds,
             uint8_t* skeleton, int64_t* counts, int64_t* nodes, int64_t cap_node, int64_t* ends, int64_t* offsets, int64_t cap_branch,
             int64_t* voxels, int64_t cap_vox) {
    const u64 V = (u64)d.n0 * d.n1 * d.n2;
    const bool want = nodes != nullptr;
    DevMem mem;
    Buffers b;
    uint8_t* vol = nullptr;
    VMASK_GRAB(vol, V, "volume");
    const int gbyte = grid_for(V, 4 * GRID_VOLUME);
    if (vmask::is_device_pointer(volume)) k_br_binary<<<gbyte, TPB>>>(volume, vol, V);
    else {
        VMASK_TRY(hipMemcpy(vol, volume, V, hipMemcpyHostToDevice));
        k_br_binary<<<gbyte, TPB>>>(vol, vol, V);
    }
    Prune pr{min_len, factor, dist, V, 0};
    if (dist && !vmask::is_device_pointer(dist)) {
        double* dd = nullptr;
        VMASK_GRAB(dd, V, "distance volume");
        VMASK_TRY(hipMemcpy(dd, dist, V * sizeof(double), hipMemcpyHostToDevice));
        pr.dist = dd;
    }
    VMASK_GRAB(b.ctr, (size_t)C_N * C_PITCH, "counters");
    Graph g;
    int64_t rounds = 0;
    u64 spurs = 0, removed = 0;
    for (;;) {
        pr.on = rounds < max_rounds && (min_len > 0 || (dist && factor > 0.0));
        int rc = build_graph(device, mem, b, vol, d, pr, g);
        if (rc) return rc;
        if (!pr.on || !g.nseg) break;
        k_br_clear<<<grid_for(g.total, GRID_LIST), TPB>>>(b.soff, b.svox, g.nseg, g.total, V, b.scl, b.best, g.n, vol, b.ctr);
        u64 hc[C_PITCH + 1];
        VMASK_TRY(hipMemcpy(hc, b.ctr + c_at(C_SPURS), sizeof(hc), hipMemcpyDeviceToHost));
        if (!hc[0]) break;                                              // the graph just built is the final one
        rounds++; spurs += hc[0]; removed += hc[C_PITCH];
        rc = vmask_skeleton(device, vol, d.n0, d.n1, d.n2, vol, nullptr, nullptr);     // (reads all of its input before it writes)
        if (rc) return rc;
    }
    // the nodes are counted with the branch ends of the final graph in place
    uint4* rec = nullptr;
    const u64 cap_rec = want ? std::min<u64>((u64)cap_node, g.n) : 0;
    if (g.n) {
        if (cap_rec) VMASK_GRAB(rec, cap_rec, "node records");
        k_br_nodes<<<grid_for(g.n, GRID_LIST), TPB>>>(b.list, b.word, g.n, b.P, b.rep, b.members, b.ends, rec, cap_rec, b.ctr);
        u64 hc[(C_DROPPED - C_ISO) * C_PITCH + 1];
        VMASK_TRY(hipMemcpy(hc, b.ctr + c_at(C_ISO), sizeof(hc), hipMemcpyDeviceToHost));
        g.iso = hc[0]; g.nodes = hc[c_at(C_NODES - C_ISO)]; g.clusters = hc[c_at(C_CLUSTERS - C_ISO)]; g.endpts = hc[c_at(C_ENDPTS - C_ISO)];
        g.pass = hc[c_at(C_PASS - C_ISO)]; g.branches = hc[c_at(C_BRANCH - C_ISO)]; g.entries = hc[c_at(C_ENTRIES - C_ISO)];
        g.dropped = hc[c_at(C_DROPPED - C_ISO)];
    }
    const int64_t out[12] = {(int64_t)g.nodes, (int64_t)g.clusters, (int64_t)g.endpts, (int64_t)g.pass, (int64_t)g.branches, (int64_t)g.entries,
                             (int64_t)g.iso, (int64_t)g.dropped, rounds, (int64_t)spurs, (int64_t)removed, g.label_rounds};
    int rc = put(counts, out, 12);
    if (rc) return rc;
    if (want) {
        if ((u64)cap_node < g.nodes || (u64)cap_branch < g.branches || (u64)cap_vox < g.entries) {
            vmask::set_error("capacity too small (the needed sizes are in counts)");
            return VRG_E_ARG;
        }
        const int64_t zero = 0;
        if (!g.branches) { rc = put(offsets, &zero, 1); if (rc) return rc; }
        if (g.nodes) try {                                              // the records alone go to the host: sorted by representative there
            std::vector<uint4> hrec(g.nodes);
            VMASK_TRY(hipMemcpy(hrec.data(), rec, g.nodes * sizeof(uint4), hipMemcpyDeviceToHost));
            std::sort(hrec.begin(), hrec.end(), [](const uint4& x, const uint4& y) { return x.x < y.x; });
            std::vector<int64_t> table(4 * g.nodes);
            std::vector<uint32_t> slots(g.nodes);
            for (size_t k = 0; k < g.nodes; k++) {
                table[4 * k] = hrec[k].x; table[4 * k + 1] = hrec[k].z >> 31; table[4 * k + 2] = hrec[k].z & 0x7fffffffu; table[4 * k + 3] = hrec[k].w;
                slots[k] = hrec[k].y;
            }
            rc = put(nodes, table.data(), table.size());
            if (rc) return rc;
            uint32_t* dslots = nullptr;
            VMASK_GRAB(dslots, g.nodes, "node slots");
            VMASK_TRY(hipMemcpy(dslots, slots.data(), g.nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
            k_br_nodeid<<<grid_for(g.nodes, GRID_LIST), TPB>>>(dslots, (uint32_t)g.nodes, g.n, b.nodeid);
        } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (node records)"); return VRG_E_MEM; }
        if (g.branches) {
            u64* bidx = nullptr; u64* voff = nullptr; void* tmp = nullptr;
            VMASK_GRAB(bidx, g.nseg, "branch indices"); VMASK_GRAB(voff, g.nseg, "branch offsets");
            auto kept = rocprim::make_transform_iterator(b.elen, Positive());
            auto lens = rocprim::make_transform_iterator(b.elen, Widen());
            size_t tb = 0, tb2 = 0;
            VMASK_TRY(rocprim::exclusive_scan(nullptr, tb, kept, bidx, 0ull, (size_t)g.nseg, rocprim::plus<u64>()));
            VMASK_TRY(rocprim::exclusive_scan(nullptr, tb2, lens, voff, 0ull, (size_t)g.nseg, rocprim::plus<u64>()));
            tb = std::max(tb, tb2);
            uint8_t* tmpb = nullptr;
            VMASK_GRAB(tmpb, tb, "scan space");
            tmp = tmpb;
            VMASK_TRY(rocprim::exclusive_scan(tmp, tb, kept, bidx, 0ull, (size_t)g.nseg, rocprim::plus<u64>()));
            VMASK_TRY(rocprim::exclusive_scan(tmp, tb, lens, voff, 0ull, (size_t)g.nseg, rocprim::plus<u64>()));
            Out<int64_t> oe, oo, ov;
            if ((rc = oe.open(mem, ends, 2 * g.branches, "branch ends")) || (rc = oo.open(mem, offsets, g.branches + 1, "offsets")) ||
                (rc = ov.open(mem, voxels, g.entries, "branch voxels"))) return rc;
            k_br_emit<<<grid_for(g.total, GRID_LIST), TPB>>>(b.soff, b.svox, g.nseg, g.total, b.list, b.word, b.rep, b.elen, b.sflag, b.ska, b.skb,
                                                            bidx, voff, b.nodeid, g.branches, g.entries, oe.dev, oo.dev, ov.dev);
            const int64_t last = (int64_t)g.entries;
            VMASK_TRY(hipMemcpy(oo.dev + g.branches, &last, sizeof(int64_t), hipMemcpyHostToDevice));
            VMASK_TRY(hipGetLastError());
            if ((rc = oe.close()) || (rc = oo.close()) || (rc = ov.close())) return rc;
        }
    }
    if (skeleton) VMASK_TRY(hipMemcpy(skeleton, vol, V, vmask::is_device_pointer(skeleton) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_branches(int device, const uint8_t* volume, int64_t n0, int64_t n1, int64_t n2,
                              int64_t min_len, double radius_factor, const double* dist, int64_t max_rounds,
                              uint8_t* skeleton, int64_t* counts, int64_t* nodes, int64_t cap_node,
                              int64_t* branch_ends, int64_t* offsets, int64_t cap_branch, int64_t* voxels, int64_t cap_vox) {
    if (!volume || !counts) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    const int given = (nodes != nullptr) + (branch_ends != nullptr) + (offsets != nullptr) + (voxels != nullptr);
    if (given != 0 && given != 4) { vmask::set_error("nodes, branch_ends, offsets and voxels: all or none"); return VRG_E_ARG; }
    if (given && (cap_node < 0 || cap_branch < 0 || cap_vox < 0)) { vmask::set_error("negative capacity"); return VRG_E_ARG; }
    if (min_len < 0 || max_rounds < 0) { vmask::set_error("min_len and max_rounds must not be negative"); return VRG_E_ARG; }
    if (!std::isfinite(radius_factor) || radius_factor < 0.0) { vmask::set_error("radius_factor must be finite and not negative"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Dim d;
    d.n0 = (int32_t)n0; d.n1 = (int32_t)n1; d.n2 = (int32_t)n2;
    return branches(device, volume, d, min_len, radius_factor, dist, max_rounds, skeleton, counts, nodes, cap_node, branch_ends, offsets, cap_branch,
                    voxels, cap_vox);
}
