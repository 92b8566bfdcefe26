// vseg_device.hip - vmask_segments of include/vmask.h: the 26-adjacency graph of a voxel set traced into segments
// ("f6 segment tracing").
//
// S = the voxels != 0, deg(v) = voxels of S among v's 26 neighbours; node: deg != 2, path voxel: deg == 2.  Segments: every
// pair of adjacent nodes [a, b]; every maximal run of path voxels with the nodes at its two ends [a, p1 .. pk, b]; every
// component of path voxels only (a free ring) closed through its voxel m of smallest linear index [m, .., m].  Canonical
// form: idx(first) < idx(last), or idx(second) < idx(second-to-last) when first == last; segments ascending by (first, second).
//
// Passes.  Only the first two read the volume, everything after works on the compacted object voxels ("slots"):
//   k_seg_count / k_seg_compact  the volume as a flat byte string in aligned 16-byte words: count, then list the linear
//                                indices of the object voxels (one atomic per wave) and enter idx -> slot into a hash table
//                                (vseg_slots.h, shared with vbr_device.hip)
//   k_seg_gather                 the 27-bit neighbourhood word of every slot (bit a*9 + b*3 + c, as vskel_device.hip), the two
//                                neighbours of a path voxel
//   k_seg_link                   a dart (v, s) is "at path voxel v, heading to its neighbour s"; its successor is the dart at
//                                that neighbour heading away from v, or the dart is terminal when the neighbour is a node
//   k_seg_jump                   Wyllie pointer jumping over all darts, double-buffered, one launch per round (the kernel
//                                boundary orders the rounds).  A dart carries (successor, hops to it, smallest idx in the
//                                window behind the hops, hops to that voxel and the dart's own direction bit there): chains
//                                end at terminal darts, and on free rings the minimum, the distance to it and the direction
//                                come out of the same doubling, so a ring is never cut and ranked a second time.
//                                The host reads two counters per round: darts not yet at a terminal, and of those the ones
//                                whose window minimum still differs from their successor's.  No thread ever walks a chain.
//   k_seg_resolve                every path voxel derives its segment's key (first, second), its position and the length
//                                from its two darts alone; every node finds its adjacent nodes of larger index; counts
//   k_seg_heads                  one record (key, length) per segment; the host sorts the records by key and sums the lengths (the
//                                heads alone travel: one read and one write, whatever their number)
//   k_seg_scatter                every path voxel writes itself at offset[segment] + position (segment: binary search of its
//                                key), the voxel at position 1 also writes both ends; nodes write their two-voxel edges
// Launches and device-to-host reads grow with log2 of the longest chain, never with the number of segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vseg_slots.h"

namespace {

constexpr int MAX_ROUNDS = 72;                     // (2 * 32 + a few: more cannot be needed inside the 32-bit envelope)

enum { C_OBJ = 0, C_CURSOR, C_NODE, C_ISO, C_PATH, C_OPEN, C_SEG, C_TOTAL, C_HEAD, C_ROUND /* [MAX_ROUNDS][2]: open darts, unsettled minima */,
       C_N = C_ROUND + 2 * MAX_ROUNDS };

constexpr uint32_t F_TERM = 1u << 31;              // in a dart's successor word: the successor is a terminal dart

__global__ void __launch_bounds__(TPB) k_seg_gather(const uint8_t* __restrict__ vol, Dim d, const uint32_t* __restrict__ list, uint32_t n,
                                                    uint32_t* __restrict__ word, uint32_t* __restrict__ nbr, u64* __restrict__ ctr) {
    u64 nodes = 0, iso = 0, path = 0;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i];
        const uint32_t w = gather_word(vol, d, idx);
        word[i] = w;
        const int deg = __popc(w);
        if (deg == 2) {
            path++;
            nbr[2u * i] = idx + (uint32_t)bit_offset(__ffs((int)w) - 1, d);
            nbr[2u * i + 1u] = idx + (uint32_t)bit_offset(31 - __clz((int)w), d);
        } else { nodes++; iso += deg == 0; }
    }
    wave_add(&ctr[c_at(C_NODE)], nodes);
    wave_add(&ctr[c_at(C_ISO)], iso);
    wave_add(&ctr[c_at(C_PATH)], path);
}

// a dart's state: x successor dart | F_TERM, y hops to it, z smallest idx among the y voxels from the dart's own on,
// w (hops to that voxel) * 2 + (direction bit s of the dart met there)
__global__ void __launch_bounds__(TPB) k_seg_link(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, const uint32_t* __restrict__ nbr,
                                                  uint32_t n, Hash h, uint4* __restrict__ st, u64* __restrict__ ctr) {
    u64 open = 0;
    const uint32_t nd = 2u * n;
    for (uint32_t dt = blockIdx.x * TPB + threadIdx.x; dt < nd; dt += gridDim.x * TPB) {
        const uint32_t i = dt >> 1, s = dt & 1u, idx = list[i];
        uint4 a = make_uint4(dt | F_TERM, 0u, idx, s);                 // terminal, and what a node's two unused darts hold
        if (__popc(word[i]) == 2) {
            const uint32_t j = h_find(h, nbr[dt]);
            if (j < n && __popc(word[j]) == 2) {
                a.x = 2u * j + (nbr[2u * j] == idx ? 1u : 0u);        // at the neighbour, heading away from here
                a.y = 1u;
                open++;
            }
        }
        st[dt] = a;
    }
    wave_add(&ctr[c_at(C_OPEN)], open);
}

__global__ void __launch_bounds__(TPB) k_seg_jump(const uint4* __restrict__ in, uint4* __restrict__ out, uint32_t nd, u64* __restrict__ c_open, u64* __restrict__ c_min) {
    u64 open = 0, unsettled = 0;
    for (uint32_t dt = blockIdx.x * TPB + threadIdx.x; dt < nd; dt += gridDim.x * TPB) {
        uint4 a = in[dt];
        if (!(a.x & F_TERM) && a.x < nd) {
            const uint4 b = in[a.x];                                    // a terminal dart is its own successor with 0 hops
            const bool differ = b.z != a.z;
            if (b.z < a.z) { a.w = 2u * a.y + b.w; a.z = b.z; }
            a.x = b.x; a.y += b.y;
            // two windows one behind the other share their minimum only once they lap the ring: it is then the ring's
            if (!(a.x & F_TERM)) { open++; unsettled += differ; }
        }
        out[dt] = a;
    }
    wave_add(c_open, open);
    wave_add(c_min, unsettled);
}

// per slot: x first, y second (the segment's key), z position in the segment (NONE: writes nothing), w length; tail: the last voxel.
// A node keeps in x the bits of its neighbours that are nodes of larger index.
__global__ void __launch_bounds__(TPB) k_seg_resolve(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, const uint32_t* __restrict__ nbr,
                                                     uint32_t n, Dim d, Hash h, const uint4* __restrict__ st, uint4* __restrict__ info,
                                                     uint32_t* __restrict__ tail, u64* __restrict__ ctr) {
    u64 nseg = 0, total = 0;
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i], w = word[i];
        uint4 o = make_uint4(0u, 0u, NONE, 0u);
        uint32_t last = 0;
        if (__popc(w) == 2) {
            const uint4 A = st[2u * i], B = st[2u * i + 1u];
            if ((A.x & F_TERM) && (B.x & F_TERM)) {                    // on a chain between two nodes
                const uint32_t ta = A.x & ~F_TERM, tb = B.x & ~F_TERM;
                if (ta < 2u * n && tb < 2u * n) {
                    const uint32_t enda = nbr[ta], lasta = list[ta >> 1], endb = nbr[tb], lastb = list[tb >> 1];
                    const bool froma = enda < endb || (enda == endb && lasta < lastb);
                    o.x = froma ? enda : endb; o.y = froma ? lasta : lastb;
                    o.z = 1u + (froma ? A.y : B.y); o.w = A.y + B.y + 3u;
                    last = froma ? endb : enda;
                }
            } else if (idx != A.z) {                                    // on a free ring [m, its smaller neighbour, .., m]; m itself is written by the voxel behind it
                const uint32_t m = A.z, sm = h_find(h, m);
                if (sm < n) {
                    o.x = m; o.y = nbr[2u * sm];
                    o.z = (A.w & 1u) ? A.w >> 1 : B.w >> 1;            // hops to m against the ring's direction
                    o.w = (A.w >> 1) + (B.w >> 1) + 1u;
                    last = m;
                }
            }
            if (o.z == 1u) { nseg++; total += o.w; }
        } else {
            for (uint32_t hi = w >> 14; hi; hi &= hi - 1u) {            // neighbours of larger index
                const int t = 14 + __ffs((int)hi) - 1;
                const uint32_t j = h_find(h, idx + (uint32_t)bit_offset(t, d));
                if (j < n && __popc(word[j]) != 2) o.x |= 1u << t;
            }
            nseg += (u64)__popc(o.x); total += 2u * (u64)__popc(o.x);
        }
        info[i] = o; tail[i] = last;
    }
    wave_add(&ctr[c_at(C_SEG)], nseg);
    wave_add(&ctr[c_at(C_TOTAL)], total);
}

__global__ void __launch_bounds__(TPB) k_seg_heads(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, Dim d,
                                                   const uint4* __restrict__ info, u64 nseg, u64* __restrict__ keys, uint32_t* __restrict__ lens, u64* __restrict__ ctr) {
    for (uint32_t i0 = blockIdx.x * TPB; i0 < n; i0 += gridDim.x * TPB) {                 // (the same trips in every lane of a wave)
        const uint32_t i = i0 + threadIdx.x;
        uint4 o = make_uint4(0u, 0u, NONE, 0u);
        bool path = false;
        if (i < n) { o = info[i]; path = __popc(word[i]) == 2; }
        const uint32_t mine = path ? (o.z == 1u ? 1u : 0u) : (i < n ? (uint32_t)__popc(o.x) : 0u);
        if (!__ballot(mine != 0u)) continue;
        uint32_t total;
        const uint32_t off = wave_scan(mine, total);
        u64 at = wave_reserve(&ctr[c_at(C_HEAD)], total) + off;
        if (!mine) continue;
        if (path) { if (at < nseg) { keys[at] = ((u64)o.x << 32) | o.y; lens[at] = o.w; } continue; }
        const uint32_t idx = list[i];
        for (uint32_t e = o.x; e; e &= e - 1u, at++)
            if (at < nseg) { keys[at] = ((u64)idx << 32) | (idx + (uint32_t)bit_offset(__ffs((int)e) - 1, d)); lens[at] = 2u; }
    }
}

__device__ __forceinline__ u64 find_key(const u64* __restrict__ keys, u64 nseg, u64 key) {
    u64 lo = 0, hi = nseg;                                              // first position whose key is >= key
    while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < nseg && keys[lo] == key ? lo : nseg;
}

__global__ void __launch_bounds__(TPB) k_seg_scatter(const uint32_t* __restrict__ list, const uint32_t* __restrict__ word, uint32_t n, Dim d,
                                                     const uint4* __restrict__ info, const uint32_t* __restrict__ tail, const u64* __restrict__ keys,
                                                     const int64_t* __restrict__ off, u64 nseg, u64 total, int64_t* __restrict__ vox) {
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i];
        const uint4 o = info[i];
        if (__popc(word[i]) == 2) {
            if (o.z == NONE) continue;
            const u64 k = find_key(keys, nseg, ((u64)o.x << 32) | o.y);
            if (k == nseg) continue;
            const u64 at = (u64)off[k];
            if (at + o.w > total || o.z >= o.w) continue;              // (cannot happen)
            vox[at + o.z] = (int64_t)idx;
            if (o.z == 1u) { vox[at] = (int64_t)o.x; vox[at + o.w - 1u] = (int64_t)tail[i]; }
        } else {
            for (uint32_t e = o.x; e; e &= e - 1u) {
                const uint32_t other = idx + (uint32_t)bit_offset(__ffs((int)e) - 1, d);
                const u64 k = find_key(keys, nseg, ((u64)idx << 32) | other);
                if (k == nseg) continue;
                const u64 at = (u64)off[k];
                if (at + 2u > total) continue;
                vox[at] = (int64_t)idx; vox[at + 1u] = (int64_t)other;
            }
        }
    }
}

struct Buffers {                                                        // (names only: the call's DevMem owns them)
    u64* ctr = nullptr; uint32_t* list = nullptr; u64* tab = nullptr; uint32_t* word = nullptr; uint32_t* nbr = nullptr;
    uint4* st[2] = {nullptr, nullptr}; uint4* info = nullptr; uint32_t* tail = nullptr;
    u64* keys[2] = {nullptr, nullptr}; uint32_t* lens = nullptr; int64_t* off = nullptr; int64_t* vox = nullptr;
};

int segments(const uint8_t* skeleton, Dim d, int64_t* counts, int64_t* offsets, int64_t cap_seg, int64_t* voxels, int64_t cap_vox) {
    const u64 V = (u64)d.n0 * d.n1 * d.n2;
    const bool want = offsets != nullptr;
    DevMem mem;
    Buffers b;
    const uint8_t* vol = nullptr;
    int rc = bring(mem, skeleton, V, "volume", &vol);
    if (rc) return rc;
    VMASK_GRAB(b.ctr, (size_t)C_N * C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(b.ctr, 0, (size_t)C_N * C_PITCH * sizeof(u64), 0));
    const uint32_t lead = (uint32_t)(reinterpret_cast<uintptr_t>(vol) & 15u);
    const uint4* base = reinterpret_cast<const uint4*>(vol - lead);
    const u64 nwords = (lead + V + 15u) / 16u;
    const int gvol = grid_for(nwords, GRID_VOLUME);
    k_seg_count<<<gvol, TPB>>>(base, nwords, lead, V, b.ctr + c_at(C_OBJ));
    u64 nobj = 0;
    VMASK_TRY(hipMemcpy(&nobj, b.ctr + c_at(C_OBJ), sizeof(u64), hipMemcpyDeviceToHost));
    int64_t out[5] = {0, 0, 0, 0, 0};
    if (nobj >= (1ull << 30)) { vmask::set_error("more than 2^30 object voxels"); return VRG_E_ARG; }
    const uint32_t n = (uint32_t)nobj, nd = 2u * n;
    u64 nseg = 0, total = 0;
    int rounds = 0, cur = 0;
    Hash h{nullptr, 0u, 0u};
    if (n) {
        const int bits = hash_bits(n);
        h.mask = (uint32_t)((1ull << bits) - 1ull); h.shift = 32u - (uint32_t)bits;
        VMASK_GRAB(b.tab, (size_t)1 << bits, "index table");
        h.tab = b.tab;
        VMASK_GRAB(b.list, n, "voxel list"); VMASK_GRAB(b.word, n, "neighbourhoods"); VMASK_GRAB(b.nbr, nd, "neighbours");
        VMASK_GRAB(b.st[0], nd, "darts"); VMASK_GRAB(b.st[1], nd, "darts"); VMASK_GRAB(b.info, n, "segment keys"); VMASK_GRAB(b.tail, n, "segment ends");
        VMASK_TRY(hipMemsetAsync(b.tab, 0xff, ((size_t)1 << bits) * sizeof(u64), 0));
        VMASK_TRY(hipMemsetAsync(b.nbr, 0xff, (size_t)nd * sizeof(uint32_t), 0));
        const int gslot = grid_for(n, GRID_LIST), gdart = grid_for(nd, GRID_LIST);
        k_seg_compact<<<gvol, TPB>>>(base, nwords, lead, V, n, b.list, h, b.ctr + c_at(C_CURSOR));
        k_seg_gather<<<gslot, TPB>>>(vol, d, b.list, n, b.word, b.nbr, b.ctr);
        k_seg_link<<<gdart, TPB>>>(b.list, b.word, b.nbr, n, h, b.st[0], b.ctr);
        u64 open = 0;
        VMASK_TRY(hipMemcpy(&open, b.ctr + c_at(C_OPEN), sizeof(u64), hipMemcpyDeviceToHost));
        while (open) {                                                  // until every dart is at a terminal or on a ring that knows its minimum
            if (rounds == MAX_ROUNDS) { vmask::set_error("pointer jumping did not finish"); return VRG_E_INTERNAL; }
            u64* c = b.ctr + c_at(C_ROUND + 2 * rounds);
            k_seg_jump<<<gdart, TPB>>>(b.st[cur], b.st[cur ^ 1], nd, c, c + C_PITCH);
            u64 hc[C_PITCH + 1];
            VMASK_TRY(hipMemcpy(hc, c, sizeof(hc), hipMemcpyDeviceToHost));
            cur ^= 1; rounds++;
            open = hc[0];
            if (!hc[C_PITCH]) break;
        }
        k_seg_resolve<<<gslot, TPB>>>(b.list, b.word, b.nbr, n, d, h, b.st[cur], b.info, b.tail, b.ctr);
        u64 hc[(C_TOTAL - C_NODE) * C_PITCH + 1];
        VMASK_TRY(hipMemcpy(hc, b.ctr + c_at(C_NODE), sizeof(hc), hipMemcpyDeviceToHost));
        nseg = hc[c_at(C_SEG - C_NODE)]; total = hc[c_at(C_TOTAL - C_NODE)];
        out[2] = (int64_t)hc[0]; out[3] = (int64_t)hc[c_at(C_ISO - C_NODE)];
    }
    out[0] = (int64_t)nseg; out[1] = (int64_t)total; out[4] = rounds;
    rc = put(counts, out, 5);
    if (rc || !want) return rc;
    if ((u64)cap_seg < nseg || (u64)cap_vox < total) { vmask::set_error("capacity too small (the needed sizes are in counts)"); return VRG_E_ARG; }
    if (!nseg) { const int64_t zero = 0; return put(offsets, &zero, 1); }
    if (nseg >= (1ull << 31)) { vmask::set_error("more than 2^31 segments"); return VRG_E_ARG; }
    VMASK_GRAB(b.keys[0], nseg, "segment heads"); VMASK_GRAB(b.keys[1], nseg, "segment heads");
    VMASK_GRAB(b.lens, nseg, "segment heads");
    int64_t* doff = offsets; int64_t* dvox = voxels;
    if (!vmask::is_device_pointer(offsets)) { VMASK_GRAB(b.off, nseg + 1, "offsets"); doff = b.off; }
    if (!vmask::is_device_pointer(voxels)) { VMASK_GRAB(b.vox, total, "segment voxels"); dvox = b.vox; }
    const int gslot = grid_for(n, GRID_LIST);
    k_seg_heads<<<gslot, TPB>>>(b.list, b.word, n, d, b.info, nseg, b.keys[0], b.lens, b.ctr);
    // the heads alone go to the host: sorted by key there, their lengths summed into the offsets
    std::vector<u64> hkeys(nseg);
    std::vector<uint32_t> hlens(nseg);
    VMASK_TRY(hipMemcpy(hkeys.data(), b.keys[0], nseg * sizeof(u64), hipMemcpyDeviceToHost));
    VMASK_TRY(hipMemcpy(hlens.data(), b.lens, nseg * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<std::pair<u64, uint32_t>> heads(nseg);
    for (size_t k = 0; k < nseg; k++) heads[k] = {hkeys[k], hlens[k]};
    std::sort(heads.begin(), heads.end());
    std::vector<int64_t> hoff(nseg + 1);
    hoff[0] = 0;
    for (size_t k = 0; k < nseg; k++) { hkeys[k] = heads[k].first; hoff[k + 1] = hoff[k] + heads[k].second; }
    if ((u64)hoff[nseg] != total) { vmask::set_error("segment lengths do not add up"); return VRG_E_INTERNAL; }
    VMASK_TRY(hipMemcpy(b.keys[1], hkeys.data(), nseg * sizeof(u64), hipMemcpyHostToDevice));
    VMASK_TRY(hipMemcpy(doff, hoff.data(), (nseg + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    k_seg_scatter<<<gslot, TPB>>>(b.list, b.word, n, d, b.info, b.tail, b.keys[1], doff, nseg, total, dvox);
    VMASK_TRY(hipGetLastError());
    if (b.off) std::copy(hoff.begin(), hoff.end(), offsets);
    if (b.vox) VMASK_TRY(hipMemcpy(voxels, dvox, total * sizeof(int64_t), hipMemcpyDeviceToHost));
    VMASK_TRY(hipDeviceSynchronize());
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_segments(int device, const uint8_t* skeleton, int64_t n0, int64_t n1, int64_t n2,
                              int64_t* counts, int64_t* offsets, int64_t cap_seg, int64_t* voxels, int64_t cap_vox) {
    if (!skeleton || !counts) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if ((offsets == nullptr) != (voxels == nullptr)) { vmask::set_error("offsets and voxels: both or neither"); return VRG_E_ARG; }
    if (offsets && (cap_seg < 0 || cap_vox < 0)) { vmask::set_error("negative capacity"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Dim d;
    d.n0 = (int32_t)n0; d.n1 = (int32_t)n1; d.n2 = (int32_t)n2;
    return segments(skeleton, d, counts, offsets, cap_seg, voxels, cap_vox);
}
