// vcomp_device.hip - vmask_compartments of include/vmask.h: the bounded traversal of the branch graph from the initial voxels of
// every compartment, never onto one of its boundary voxels ("f12 compartments").  A pair is one
// (compartment, branch), numbered compartment * B + branch; all pairs are handled together.
//
//   k_comp_check     the tables and the lists are looked at before anything is written: what k_mor_check refuses, the end entries
//                    against the nodes' voxels, every listed index inside the volume, no voxel in both lists of a compartment;
//                    every entry and node marks its voxel in the sorted list of all listed voxels
//   k_comp_unhit     the listed voxels that no entry and no node marked; one counter of what is wrong
//   k_comp_nodes     one thread per (compartment, node): blocked / initial by binary search in the compartment's sorted lists,
//                    depth and level 0 at the initial nodes
//   k_comp_pairs     one thread per pair, ONE pass over the branch's interior entries: has it a blocked entry, an initial one; the
//                    hops from the first initial entry in front of every blocked one to the first end, from the last initial
//                    entry behind every blocked one to the last end - the ends' depths are lowered to them (atomicMin).  A closed
//                    branch keeps the depth of its private vertex instead.
//   k_comp_relax     one thread per pair: a branch free of blocked entries between two unblocked nodes lowers either end's depth to
//                    the other's + (n - 1) by 64-bit atomicMin; the host reads one counter per round (as k_mor_relax does)
//   k_comp_level     the same rounds for the levels over the tight predecessors: level(u) + 1 through a tight branch, 1 from a
//                    tight initial entry inside the branch
//   k_comp_walk      one thread per pair walks the branch between its sources (the ends, the initial entries; a blocked entry
//                    cuts): launch one lowers the entry's key depth << 8 | label, launch two - the keys are final - stores the
//                    level where the pair's key is the entry's, and marks the entry as reached twice where it is not
//   k_comp_merge     one thread per node: the smallest (depth, label) over the compartments, the counts
//   k_comp_finish    one thread per branch: the entries' outputs (the end entries take their node's), branch_comp, branch_level,
//                    the counts
// Kernel boundaries are the only ordering between the steps.  Integers only.
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr u64 NONE64 = ~0ull;
constexpr int MAX_COMP = 255;
enum : uint8_t { F_BLOCKED = 1, F_INIT = 2 };
enum { CC_OWNED = 0, CC_REACHED = 1, CC_BRANCHES = 2, CC_N = 3 };

// the lists of all compartments, each compartment's slice sorted ascending
struct Lists { const int64_t* ioff; const int64_t* ivox; const int64_t* boff; const int64_t* bvox; };
struct Table { const int64_t* off; const int64_t* vox; const int64_t* ends; const int64_t* nodevox; u64 B, N; };
// per pair: f flags, a / b hops of an initial entry to the first / last end (-1: none; a closed branch: a = its private vertex' depth)
struct Pairs { uint8_t* f; int64_t* a; int64_t* b; };
// per (compartment, node): f flags, d depth, l level (NONE64: unreached)
struct Nodes { uint8_t* f; u64* d; u64* l; };

// the position of x in the ascending v[lo, hi), or -1
__device__ __forceinline__ int64_t find(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t x) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && v[lo] == x ? lo : -1;
}
// a voxel in compartment c: F_BLOCKED, F_INIT or 0 (no voxel is in both lists)
__device__ __forceinline__ uint8_t flags_of(const Lists& L, u64 c, int64_t x) {
    if (find(L.bvox, L.boff[c], L.boff[c + 1], x) >= 0) return F_BLOCKED;
    if (find(L.ivox, L.ioff[c], L.ioff[c + 1], x) >= 0) return F_INIT;
    return 0;
}
__device__ __forceinline__ bool lower(u64* p, u64 x) { return x < *p && atomicMin(p, x) > x; }

__global__ void __launch_bounds__(TPB) k_comp_check(Table t, u64 total, u64 V, Lists L, u64 K, u64 ni, u64 nb, const int64_t* __restrict__ all, u64 M,
                                                    uint8_t* __restrict__ hit, u64* __restrict__ bad) {
    u64 wrong = 0;
    const u64 m0 = t.B > total ? t.B : total, m1 = t.N > ni ? t.N : ni, m2 = m0 > m1 ? m0 : m1, most = m2 > nb ? m2 : nb;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < most; i += (u64)gridDim.x * TPB) {
        if (i < t.B) {
            const int64_t a = t.off[i], b = t.off[i + 1], ea = t.ends[2 * i], eb = t.ends[2 * i + 1];
            const bool range = !(a < 0 || b - a < 2 || (u64)b > total || (i == 0 && a != 0));
            const bool nodes = !(ea < -1 || eb < -1 || ea >= (int64_t)t.N || eb >= (int64_t)t.N || ((ea < 0) != (eb < 0)));
            wrong += !range; wrong += !nodes;
            if (range && nodes) {                                         // (only now are these indices safe)
                const int64_t first = t.vox[a], last = t.vox[b - 1];
                wrong += ea < 0 ? first != last : (first != t.nodevox[ea] || last != t.nodevox[eb]);
            }
        }
        if (i < total) {
            const int64_t x = t.vox[i];
            wrong += (u64)x >= V;
            const int64_t at = find(all, 0, (int64_t)M, x);
            if (at >= 0) hit[at] = 1;
        }
        if (i < t.N) {
            const int64_t x = t.nodevox[i];
            wrong += (u64)x >= V;
            const int64_t at = find(all, 0, (int64_t)M, x);
            if (at >= 0) hit[at] = 1;
        }
        if (i < ni) {
            const int64_t x = L.ivox[i];
            wrong += (u64)x >= V;
            u64 lo = 0, hi = K;                                           // the compartment of item i: the last c with ioff[c] <= i
            while (hi - lo > 1) { const u64 mid = (lo + hi) >> 1; if ((u64)L.ioff[mid] <= i) lo = mid; else hi = mid; }
            wrong += find(L.bvox, L.boff[lo], L.boff[lo + 1], x) >= 0;
        }
        if (i < nb) wrong += (u64)L.bvox[i] >= V;
    }
    wave_add(bad, wrong);
}

__global__ void __launch_bounds__(TPB) k_comp_unhit(const uint8_t* __restrict__ hit, u64 M, u64* __restrict__ bad) {
    u64 wrong = 0;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < M; i += (u64)gridDim.x * TPB) wrong += !hit[i];
    wave_add(bad, wrong);
}

__global__ void __launch_bounds__(TPB) k_comp_nodes(Table t, Lists L, u64 K, Nodes nd) {
    for (u64 p = (u64)blockIdx.x * TPB + threadIdx.x; p < K * t.N; p += (u64)gridDim.x * TPB) {
        const u64 c = p / t.N, v = p - c * t.N;
        const uint8_t f = flags_of(L, c, t.nodevox[v]);
        nd.f[p] = f;
        nd.d[p] = nd.l[p] = (f & F_INIT) ? 0ull : NONE64;
    }
}

__global__ void __launch_bounds__(TPB) k_comp_pairs(Table t, Lists L, u64 K, Nodes nd, Pairs pr) {
    for (u64 p = (u64)blockIdx.x * TPB + threadIdx.x; p < K * t.B; p += (u64)gridDim.x * TPB) {
        const u64 c = p / t.B, b = p - c * t.B;
        const int64_t a = t.off[b], n = t.off[b + 1] - a;
        uint8_t f = 0;
        int64_t front = -1, back = -1;                                    // the first initial entry in front of every blocked one; the last behind
        if (L.ioff[c + 1] > L.ioff[c] || L.boff[c + 1] > L.boff[c])
            for (int64_t i = 1; i < n - 1; i++) {
                const uint8_t g = flags_of(L, c, t.vox[a + i]);
                if (g & F_BLOCKED) back = -1;
                else if (g & F_INIT) { if (!f) front = i; back = i; }
                f |= g;
            }
        int64_t to_first = front, to_last = back < 0 ? -1 : n - 1 - back;
        const int64_t u = t.ends[2 * b], w = t.ends[2 * b + 1];
        if (u < 0) {                                                      // a closed branch: its private vertex
            const uint8_t g = flags_of(L, c, t.vox[a]);
            int64_t d = to_first < 0 ? to_last : (to_last < 0 || to_first < to_last ? to_first : to_last);
            if (g & F_INIT) d = 0;
            if (g & F_BLOCKED) d = -1;
            to_first = d; to_last = -1;
        } else {
            if (to_first >= 0 && !(nd.f[c * t.N + u] & F_BLOCKED)) atomicMin(&nd.d[c * t.N + u], (u64)to_first);
            if (to_last >= 0 && !(nd.f[c * t.N + w] & F_BLOCKED)) atomicMin(&nd.d[c * t.N + w], (u64)to_last);
        }
        pr.f[p] = f; pr.a[p] = to_first; pr.b[p] = to_last;
    }
}

// the depths are read and lowered in the same launch: a stale read only delays, the round that lowers nothing has read the final state
__global__ void __launch_bounds__(TPB) k_comp_relax(Table t, u64 K, Nodes nd, Pairs pr, u64* __restrict__ c_lowered) {
    u64 lowered = 0;
    for (u64 p = (u64)blockIdx.x * TPB + threadIdx.x; p < K * t.B; p += (u64)gridDim.x * TPB) {
        const u64 c = p / t.B, b = p - c * t.B;
        const int64_t u = t.ends[2 * b], w = t.ends[2 * b + 1];
        if (u < 0 || u == w || (pr.f[p] & F_BLOCKED)) continue;
        const u64 pu = c * t.N + (u64)u, pw = c * t.N + (u64)w;
        if ((nd.f[pu] | nd.f[pw]) & F_BLOCKED) continue;
        const u64 len = (u64)(t.off[b + 1] - t.off[b] - 1), du = nd.d[pu], dw = nd.d[pw];
        if (du != NONE64 && lower(&nd.d[pw], du + len)) lowered++;
        if (dw != NONE64 && lower(&nd.d[pu], dw + len)) lowered++;
    }
    wave_add(c_lowered, lowered);
}

__global__ void __launch_bounds__(TPB) k_comp_level(Table t, u64 K, Nodes nd, Pairs pr, u64* __restrict__ c_lowered) {
    u64 lowered = 0;
    for (u64 p = (u64)blockIdx.x * TPB + threadIdx.x; p < K * t.B; p += (u64)gridDim.x * TPB) {
        const u64 c = p / t.B, b = p - c * t.B;
        const int64_t u = t.ends[2 * b], w = t.ends[2 * b + 1];
        if (u < 0) continue;
        const u64 pu = c * t.N + (u64)u, pw = c * t.N + (u64)w;
        const bool open_u = !(nd.f[pu] & F_BLOCKED), open_w = !(nd.f[pw] & F_BLOCKED);
        const u64 du = nd.d[pu], dw = nd.d[pw];
        if (open_u && pr.a[p] >= 0 && du == (u64)pr.a[p] && lower(&nd.l[pu], 1ull)) lowered++;
        if (open_w && pr.b[p] >= 0 && dw == (u64)pr.b[p] && lower(&nd.l[pw], 1ull)) lowered++;
        if (u == w || (pr.f[p] & F_BLOCKED) || !open_u || !open_w || du == NONE64 || dw == NONE64) continue;
        const u64 len = (u64)(t.off[b + 1] - t.off[b] - 1);
        if (du + len == dw) { const u64 l = nd.l[pu]; if (l != NONE64 && lower(&nd.l[pw], l + 1ull)) lowered++; }
        if (dw + len == du) { const u64 l = nd.l[pw]; if (l != NONE64 && lower(&nd.l[pu], l + 1ull)) lowered++; }
    }
    wave_add(c_lowered, lowered);
}

struct Source { u64 d, l; };                                              // d == NONE64: no source
__device__ __forceinline__ u64 plus(u64 d, int64_t hops) { return d == NONE64 ? NONE64 : d + (u64)hops; }

template <bool SECOND>
__global__ void __launch_bounds__(TPB) k_comp_walk(Table t, Lists L, u64 K, Nodes nd, Pairs pr, u64* key, int64_t* __restrict__ level, uint8_t* __restrict__ twice,
                                                   u64* __restrict__ cc) {
    for (u64 p = (u64)blockIdx.x * TPB + threadIdx.x; p < K * t.B; p += (u64)gridDim.x * TPB) {
        const u64 c = p / t.B, b = p - c * t.B, label = c + 1;
        const int64_t a = t.off[b], n = t.off[b + 1] - a, u = t.ends[2 * b], w = t.ends[2 * b + 1];
        const uint8_t f = pr.f[p];
        Source left{NONE64, 0}, right{NONE64, 0};
        if (u < 0) {
            if (pr.a[p] >= 0) left.d = right.d = (u64)pr.a[p];
        } else {
            const u64 pu = c * t.N + (u64)u, pw = c * t.N + (u64)w;
            if (!(nd.f[pu] & F_BLOCKED)) { left.d = nd.d[pu]; left.l = nd.l[pu]; }
            if (!(nd.f[pw] & F_BLOCKED)) { right.d = nd.d[pw]; right.l = nd.l[pw]; }
        }
        if (left.d == NONE64 && right.d == NONE64 && !(f & F_INIT)) continue;
        u64 reached = 0;
        auto emit = [&](int64_t i, u64 d, u64 l) {
            const u64 mine = (d << 8) | label;
            if (!SECOND) { atomicMin(&key[a + i], mine); reached++; }
            else if (key[a + i] == mine) level[a + i] = (int64_t)l;
            else twice[a + i] = 1;
        };
        if (u < 0 && left.d != NONE64) emit(0, left.d, 0);               // the private vertex, kept at the first entry
        int64_t at = 0;                                                   // the source to the left of the run being walked, `left`
        for (int64_t i = 1; i <= n - 1;) {
            int64_t q = n - 1;                                            // the next initial or blocked entry, or the last entry
            uint8_t g = 0;
            if (f)
                for (q = i; q < n - 1; q++)
                    if ((g = flags_of(L, c, t.vox[a + q]))) break;
            const Source next = q == n - 1 ? right : (g & F_INIT) ? Source{0, 0} : Source{NONE64, 0};
            if (left.d != NONE64 || next.d != NONE64)
                for (int64_t k = at + 1; k < q; k++) {
                    const u64 dl = plus(left.d, k - at), dr = plus(next.d, q - k);
                    emit(k, dl < dr ? dl : dr, dl < dr ? left.l : dr < dl ? next.l : (left.l < next.l ? left.l : next.l));
                }
            if (q < n - 1 && (g & F_INIT)) emit(q, 0, 0);
            left = next; at = q; i = q + 1;
        }
        if (!SECOND && reached) atomicAdd(&cc[label * CC_N + CC_REACHED], reached);
    }
}

// a block's counts per label, added to the table at the block's end
__device__ __forceinline__ void flush(const u64* h, u64 K, u64* __restrict__ cc) {
    __syncthreads();
    for (u64 k = threadIdx.x; k < CC_N * (K + 1); k += TPB)
        if (h[k]) atomicAdd(&cc[k], h[k]);
}

__global__ void __launch_bounds__(TPB) k_comp_merge(u64 N, u64 K, Nodes nd, uint8_t* __restrict__ comp, int64_t* __restrict__ depth, int64_t* __restrict__ level,
                                                    u64* __restrict__ cc) {
    __shared__ u64 h[CC_N * (MAX_COMP + 1)];
    for (int k = threadIdx.x; k < CC_N * (MAX_COMP + 1); k += TPB) h[k] = 0;
    __syncthreads();
    for (u64 v = (u64)blockIdx.x * TPB + threadIdx.x; v < N; v += (u64)gridDim.x * TPB) {
        u64 best = NONE64, owner = 0, lv = NONE64, reach = 0;
        for (u64 c = 0; c < K; c++) {
            const u64 d = nd.d[c * N + v];
            if (d == NONE64) continue;
            reach++;
            atomicAdd(&h[(c + 1) * CC_N + CC_REACHED], 1ull);
            if (d < best) { best = d; owner = c + 1; lv = nd.l[c * N + v]; }
        }
        comp[v] = (uint8_t)owner; depth[v] = (int64_t)best; level[v] = (int64_t)lv;      // (NONE64 is -1)
        atomicAdd(&h[owner * CC_N + CC_OWNED], 1ull);
        if (reach > 1) atomicAdd(&h[CC_REACHED], 1ull);
    }
    flush(h, K, cc);
}

__global__ void __launch_bounds__(TPB) k_comp_finish(Table t, u64 K, const uint8_t* __restrict__ ncomp, const int64_t* __restrict__ ndepth, const int64_t* __restrict__ nlevel,
                                                     const uint8_t* __restrict__ twice, uint8_t* __restrict__ ecomp, int64_t* edepth, int64_t* elevel,
                                                     uint8_t* __restrict__ bcomp, int64_t* __restrict__ blevel, u64* __restrict__ cc) {
    __shared__ u64 h[CC_N * (MAX_COMP + 1)];
    for (int k = threadIdx.x; k < CC_N * (MAX_COMP + 1); k += TPB) h[k] = 0;
    __syncthreads();
    for (u64 b = (u64)blockIdx.x * TPB + threadIdx.x; b < t.B; b += (u64)gridDim.x * TPB) {
        const int64_t a = t.off[b], n = t.off[b + 1] - a, u = t.ends[2 * b], w = t.ends[2 * b + 1];
        uint8_t first = 0;
        bool same = true;
        int64_t d0 = -1, l0 = -1, low = INT64_MAX;
        for (int64_t i = 0; i < n; i++) {
            uint8_t oc; int64_t od, ol;
            if (u >= 0 && (i == 0 || i == n - 1)) { const int64_t v = i == 0 ? u : w; oc = ncomp[v]; od = ndepth[v]; ol = nlevel[v]; }
            else if (u < 0 && i == n - 1) { oc = first; od = d0; ol = l0; }
            else {
                const u64 k = ((const u64*)edepth)[a + i];
                oc = k == NONE64 ? 0 : (uint8_t)(k & 255ull); od = k == NONE64 ? -1 : (int64_t)(k >> 8); ol = k == NONE64 ? -1 : elevel[a + i];
                atomicAdd(&h[oc * CC_N + CC_OWNED], 1ull);
                if (twice[a + i]) atomicAdd(&h[CC_REACHED], 1ull);
            }
            if (i == 0) { first = oc; d0 = od; l0 = ol; }
            same = same && oc == first;
            if (ol < low) low = ol;
            ecomp[a + i] = oc; edepth[a + i] = od; elevel[a + i] = ol;
        }
        const uint8_t mine = same ? first : 0;
        bcomp[b] = mine; blevel[b] = mine ? low : -1;
        atomicAdd(&h[mine * CC_N + CC_BRANCHES], 1ull);
    }
    flush(h, K, cc);
}

bool ascends_from_zero(const std::vector<int64_t>& off) {
    if (off.empty() || off[0] != 0) return false;
    for (size_t k = 1; k < off.size(); k++)
        if (off[k] < off[k - 1]) return false;
    return off.back() < ((int64_t)1 << 31);
}
// one compartment's slice sorted; every listed voxel once, ascending, in `all`
void sort_lists(const std::vector<int64_t>& off, std::vector<int64_t>& vox, std::vector<int64_t>& all) {
    for (size_t c = 0; c + 1 < off.size(); c++) std::sort(vox.begin() + off[c], vox.begin() + off[c + 1]);
    all.insert(all.end(), vox.begin(), vox.end());
}

struct Args {
    const int64_t* offsets; int64_t B; const int64_t* voxels; const int64_t* ends; const int64_t* nodevox; int64_t N;
    int64_t K; const int64_t* init_off; const int64_t* init_vox; const int64_t* bound_off; const int64_t* bound_vox;
    uint8_t* entry_comp; int64_t* entry_depth; int64_t* entry_level; uint8_t* node_comp; int64_t* node_depth; int64_t* node_level;
    uint8_t* branch_comp; int64_t* branch_level; int64_t* comp_counts; int64_t* counts;
};

int compartments(const Args& g, u64 V) {
    const u64 B = (u64)g.B, N = (u64)g.N, K = (u64)g.K;
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
    // ---- the lists: the two offset tables decide how much is read, so the host looks at them; each compartment's slice is sorted
    std::vector<int64_t> ioff, boff, ivox, bvox, all;
    try {
        if ((rc = fetch(g.init_off, K + 1, ioff)) || (rc = fetch(g.bound_off, K + 1, boff))) return rc;
        if (!ascends_from_zero(ioff) || !ascends_from_zero(boff)) { vmask::set_error("a list offset table does not ascend from 0"); return VRG_E_ARG; }
        if ((ioff.back() && !g.init_vox) || (boff.back() && !g.bound_vox)) { vmask::set_error("null pointer (compartment lists)"); return VRG_E_ARG; }
        if ((rc = fetch(g.init_vox, (size_t)ioff.back(), ivox)) || (rc = fetch(g.bound_vox, (size_t)boff.back(), bvox))) return rc;
        sort_lists(ioff, ivox, all); sort_lists(boff, bvox, all);
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
    } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (compartment lists)"); return VRG_E_MEM; }
    const u64 ni = ivox.size(), nb = bvox.size(), M = all.size();
    Table t{nullptr, nullptr, nullptr, nullptr, B, N};
    if ((rc = bring(mem, g.offsets, B ? B + 1 : 0, "offsets", &t.off)) || (rc = bring(mem, g.voxels, (size_t)total, "branch voxels", &t.vox)) ||
        (rc = bring(mem, g.ends, 2 * B, "branch ends", &t.ends)) || (rc = bring(mem, g.nodevox, N, "node voxels", &t.nodevox))) return rc;
    int64_t* lists = nullptr;
    uint8_t* hit = nullptr;
    u64* ctr = nullptr;
    const size_t words = 2 * (K + 1) + ni + nb + M;
    VMASK_GRAB(lists, words, "compartment lists"); VMASK_GRAB(hit, M, "list marks"); VMASK_GRAB(ctr, 2 * C_PITCH, "counters");
    try {
        std::vector<int64_t> pack;
        pack.reserve(words);
        for (const std::vector<int64_t>* v : {&ioff, &boff, &ivox, &bvox, &all}) pack.insert(pack.end(), v->begin(), v->end());
        VMASK_TRY(hipMemcpy(lists, pack.data(), words * sizeof(int64_t), hipMemcpyHostToDevice));
    } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (compartment lists)"); return VRG_E_MEM; }
    const Lists L{lists, lists + 2 * (K + 1), lists + (K + 1), lists + 2 * (K + 1) + ni};
    const int64_t* dall = lists + 2 * (K + 1) + ni + nb;
    VMASK_TRY(hipMemsetAsync(ctr, 0, 2 * C_PITCH * sizeof(u64), 0));
    if (M) VMASK_TRY(hipMemsetAsync(hit, 0, M, 0));
    const u64 most = std::max(std::max(B, (u64)total), std::max(N, std::max(ni, nb)));
    u64 bad = 0;
    if (most) {
        k_comp_check<<<grid_for(most, GRID_LIST), TPB>>>(t, (u64)total, V, L, K, ni, nb, dall, M, hit, ctr);
        if (M) k_comp_unhit<<<grid_for(M, GRID_LIST), TPB>>>(hit, M, ctr);
        VMASK_TRY(hipMemcpy(&bad, ctr, sizeof(u64), hipMemcpyDeviceToHost));
    }
    if (bad) {
        vmask::set_error("the branch table or the compartment lists do not fit: offsets, voxels, ends, node voxels or end entries out of range, "
                         "a listed voxel outside the volume, the voxel of no vertex or in both lists of a compartment");
        return VRG_E_ARG;
    }

    Out<uint8_t> oec, onc, obc;
    Out<int64_t> oed, oel, ond, onl, obl;
    if ((rc = oec.open(mem, g.entry_comp, (size_t)total, "entry compartments")) || (rc = oed.open(mem, g.entry_depth, (size_t)total, "entry depths")) ||
        (rc = oel.open(mem, g.entry_level, (size_t)total, "entry levels")) || (rc = onc.open(mem, g.node_comp, N, "node compartments")) ||
        (rc = ond.open(mem, g.node_depth, N, "node depths")) || (rc = onl.open(mem, g.node_level, N, "node levels")) ||
        (rc = obc.open(mem, g.branch_comp, B, "branch compartments")) || (rc = obl.open(mem, g.branch_level, B, "branch levels"))) return rc;
    Nodes nd{nullptr, nullptr, nullptr};
    Pairs pr{nullptr, nullptr, nullptr};
    uint8_t* twice = nullptr;
    u64* cc = nullptr;
    VMASK_GRAB(nd.f, K * N, "node flags"); VMASK_GRAB(nd.d, K * N, "node depths per compartment"); VMASK_GRAB(nd.l, K * N, "node levels per compartment");
    VMASK_GRAB(pr.f, K * B, "pair flags"); VMASK_GRAB(pr.a, K * B, "pair hops"); VMASK_GRAB(pr.b, K * B, "pair hops");
    VMASK_GRAB(twice, (size_t)total, "entry marks"); VMASK_GRAB(cc, CC_N * (K + 1), "compartment counts");
    VMASK_TRY(hipMemsetAsync(cc, 0, CC_N * (K + 1) * sizeof(u64), 0));
    if (total) {
        VMASK_TRY(hipMemsetAsync(twice, 0, (size_t)total, 0));
        VMASK_TRY(hipMemsetAsync(oed.dev, 0xff, (size_t)total * sizeof(int64_t), 0));                        // the keys: NONE64
        VMASK_TRY(hipMemsetAsync(oel.dev, 0xff, (size_t)total * sizeof(int64_t), 0));
    }
    const int gp = grid_for(K * B, GRID_LIST);
    int64_t rounds[2] = {0, 0};
    if (N) k_comp_nodes<<<grid_for(K * N, GRID_LIST), TPB>>>(t, L, K, nd);
    if (B) k_comp_pairs<<<gp, TPB>>>(t, L, K, nd, pr);
    const int64_t limit = std::max<int64_t>((int64_t)N, 1) + 1;
    for (int phase = 0; phase < 2; phase++)
        for (u64 lowered = 1; B && N && lowered;) {
            if (rounds[phase] == limit) { vmask::set_error(phase ? "the levels did not settle within one round per node" : "the depths did not settle within one round per node"); return VRG_E_INTERNAL; }
            VMASK_TRY(hipMemsetAsync(ctr, 0, sizeof(u64), 0));
            if (phase) k_comp_level<<<gp, TPB>>>(t, K, nd, pr, ctr);
            else k_comp_relax<<<gp, TPB>>>(t, K, nd, pr, ctr);
            VMASK_TRY(hipMemcpy(&lowered, ctr, sizeof(u64), hipMemcpyDeviceToHost));
            rounds[phase]++;
        }
    if (B) {
        k_comp_walk<false><<<gp, TPB>>>(t, L, K, nd, pr, reinterpret_cast<u64*>(oed.dev), oel.dev, twice, cc);
        k_comp_walk<true><<<gp, TPB>>>(t, L, K, nd, pr, reinterpret_cast<u64*>(oed.dev), oel.dev, twice, cc);
    }
    if (N) k_comp_merge<<<grid_for(N, GRID_LIST), TPB>>>(N, K, nd, onc.dev, ond.dev, onl.dev, cc);
    if (B) k_comp_finish<<<grid_for(B, GRID_LIST), TPB>>>(t, K, onc.dev, ond.dev, onl.dev, twice, oec.dev, oed.dev, oel.dev, obc.dev, obl.dev, cc);
    VMASK_TRY(hipGetLastError());
    if ((rc = oec.close()) || (rc = oed.close()) || (rc = oel.close()) || (rc = onc.close()) || (rc = ond.close()) || (rc = onl.close()) ||
        (rc = obc.close()) || (rc = obl.close())) return rc;
    try {
        std::vector<int64_t> hcc(CC_N * (K + 1));
        VMASK_TRY(hipMemcpy(hcc.data(), cc, hcc.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        if ((rc = put(g.comp_counts, hcc.data(), hcc.size()))) return rc;
    } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (compartment counts)"); return VRG_E_MEM; }
    if (g.counts && (rc = put(g.counts, rounds, 2))) return rc;
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_compartments(int device, int64_t n0, int64_t n1, int64_t n2,
                                  const int64_t* offsets, int64_t nbranch, const int64_t* voxels, const int64_t* branch_ends,
                                  const int64_t* node_voxel, int64_t nnode,
                                  int64_t ncomp, const int64_t* init_off, const int64_t* init_vox, const int64_t* bound_off, const int64_t* bound_vox,
                                  uint8_t* entry_comp, int64_t* entry_depth, int64_t* entry_level,
                                  uint8_t* node_comp, int64_t* node_depth, int64_t* node_level,
                                  uint8_t* branch_comp, int64_t* branch_level, int64_t* comp_counts, int64_t* counts) {
    if (ncomp < 1 || ncomp > MAX_COMP) { vmask::set_error("the number of compartments must be 1 .. 255"); return VRG_E_ARG; }
    if (nbranch < 0 || nnode < 0 || nbranch >= ((int64_t)1 << 31) || nnode >= ((int64_t)1 << 31)) { vmask::set_error("negative or oversized count"); return VRG_E_ARG; }
    if (!init_off || !bound_off || !comp_counts) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nbranch && (!offsets || !voxels || !branch_ends || !entry_comp || !entry_depth || !entry_level || !branch_comp || !branch_level)) { vmask::set_error("null pointer (branch tables)"); return VRG_E_ARG; }
    if (nnode && (!node_voxel || !node_comp || !node_depth || !node_level)) { vmask::set_error("null pointer (node tables)"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    const Args g{offsets, nbranch, voxels, branch_ends, node_voxel, nnode, ncomp, init_off, init_vox, bound_off, bound_vox,
                 entry_comp, entry_depth, entry_level, node_comp, node_depth, node_level, branch_comp, branch_level, comp_counts, counts};
    return compartments(g, (u64)n0 * (u64)n1 * (u64)n2);
}
