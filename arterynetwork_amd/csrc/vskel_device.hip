// vskel_device.hip - vmask_skeleton of include/vmask.h: curve skeleton of a binary volume by subfield-sequential
// thinning with border marking.
//
// A voxel P of the object with 3x3x3 neighbourhood N26* (P removed) is
//   border     when one of its 6 face neighbours is background,
//   end point  when N26* holds exactly one object voxel,
//   simple     (Malandain-Bertrand) when the object voxels of N26* form one 26-connected component and the background
//              voxels of N18* that are 6-connected inside N18* to a background face neighbour form one 6-connected component.
// Its subfield is (i0&1)*4 + (i1&1)*2 + (i2&1): two voxels of one subfield are never 26-neighbours.  A cycle marks every
// border voxel, then for s = 0..7 deletes at once every marked voxel of subfield s that is neither an end point nor
// non-simple on the image as it is at the start of step s; cycles repeat until one deletes nothing.
//
// Layout: the thinning runs on a zero-padded uint8 copy (0/1) of the volume, [n0+2][n1+2][R], voxel (i0,i1,i2) at
// ((i0+1)*(n1+2) + i1+1)*R + 4 + i2 with R = 4*ceil(n2/4) + 8: no neighbourhood read tests bounds, and a row's voxels
// start at a 4-byte boundary (the whole-volume passes take four voxels per load).  Everything outside the volume is background.
// Kernels per cycle: k_skel_mark scans the padded copy and compacts the border voxels into eight lists, one per subfield
// (a wave works inside one row, so the subfield of its k-th voxels is the same in every lane: two ballots and one atomic
// per wave and subfield); then eight launches of k_skel_step, launch s over list s: the 26 neighbours gathered into one
// register word (bit a*9 + b*3 + c for the offset (a-1, b-1, c-1)), the end-point test a popcount, both component counts
// flood fills by shifts and masks of that word - no table (vskel_simple.h, which a host program enumerates).  Launch s stores only to voxels of subfield s and loads only
// voxels of other subfields: no race, no fence; the kernel boundary orders the steps.  The host reads one deletion counter
// per cycle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vskel_simple.h"

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / 64;                      // waves per block

struct Geo {
    int32_t n0, n1, n2;
    uint32_t W;                                    // 4-voxel words per row that hold voxels of the volume
    uint32_t cpr;                                  // 64-word chunks per row: one wave and turn each
    size_t R, plane;                               // bytes per padded row / per padded i0 plane
    __host__ __device__ size_t row_base(uint32_t i0, uint32_t i1) const { return ((size_t)(i0 + 1) * (size_t)(n1 + 2) + (i1 + 1)) * R + 4; }
    __host__ __device__ uint64_t items() const { return (uint64_t)n0 * n1 * cpr; }
    size_t bytes() const { return (size_t)(n0 + 2) * plane; }
};
struct Starts { uint32_t at[8]; };                 // where each subfield's list starts in the list array

// counters on the device.  The eight list lengths are 256 bytes apart: every wave of k_skel_mark that finds a border voxel adds to
// one of them, and adds to one cache line queue up behind each other
enum { C_OBJ = 0 /* [8] object voxels per subfield */, C_DEL = 8 /* deletions of the cycle */, C_LIST = 64 /* [8], one per C_PITCH */, C_PITCH = 64, C_N = C_LIST + 8 * C_PITCH };
__host__ __device__ inline int c_list(int s) { return C_LIST + s * C_PITCH; }

// the wave's turn -> its row and its lane's word in it (the same row in every lane)
struct Turn { uint32_t i0, i1, w; bool valid; };
__device__ __forceinline__ Turn turn_of(const Geo& g, uint64_t item) {
    const uint32_t row = (uint32_t)(item / g.cpr), chunk = (uint32_t)(item - (uint64_t)row * g.cpr);
    Turn t;
    t.i0 = row / (uint32_t)g.n1; t.i1 = row - t.i0 * (uint32_t)g.n1;
    t.w = chunk * 64u + (threadIdx.x & 63u);
    t.valid = t.w < g.W;
    return t;
}
__device__ __forceinline__ uint64_t first_item() {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WPB + (threadIdx.x >> 6)));
}
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) { return (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull)); }

// padded 0/1 copy of in != 0 (P is zeroed before) and the object's voxel count per subfield
__global__ void __launch_bounds__(TPB) k_skel_pad(const uint8_t* __restrict__ in, uint8_t* __restrict__ P, Geo g, unsigned int* __restrict__ ctr) {
    for (uint64_t item = first_item(); item < g.items(); item += (uint64_t)gridDim.x * WPB) {
        const Turn t = turn_of(g, item);
        uint32_t word = 0;
        if (t.valid) {
            const uint8_t* src = in + ((size_t)t.i0 * g.n1 + t.i1) * (size_t)g.n2 + 4u * t.w;
            const uint32_t left = (uint32_t)g.n2 - 4u * t.w;          // (>= 1)
#pragma unroll
            for (int k = 0; k < 4; k++) if ((uint32_t)k < left && src[k]) word |= 1u << (8 * k);
            *reinterpret_cast<uint32_t*>(P + g.row_base(t.i0, t.i1) + 4u * t.w) = word;
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {                                  // voxels q and q + 2 of a word are of one subfield
            const unsigned int n = (unsigned int)(__popcll(__ballot((word >> (8 * q)) & 1u)) + __popcll(__ballot((word >> (8 * q + 16)) & 1u)));
            if (n && (threadIdx.x & 63u) == 0u) atomicAdd(&ctr[C_OBJ + (t.i0 & 1u) * 4u + (t.i1 & 1u) * 2u + q], n);
        }
    }
}

__global__ void __launch_bounds__(TPB) k_skel_unpad(const uint8_t* __restrict__ P, uint8_t* __restrict__ out, Geo g) {
    for (uint64_t item = first_item(); item < g.items(); item += (uint64_t)gridDim.x * WPB) {
        const Turn t = turn_of(g, item);
        if (!t.valid) continue;
        const uint32_t word = *reinterpret_cast<const uint32_t*>(P + g.row_base(t.i0, t.i1) + 4u * t.w);
        uint8_t* dst = out + ((size_t)t.i0 * g.n1 + t.i1) * (size_t)g.n2 + 4u * t.w;
        const uint32_t left = (uint32_t)g.n2 - 4u * t.w;
#pragma unroll
        for (int k = 0; k < 4; k++) if ((uint32_t)k < left) dst[k] = (uint8_t)((word >> (8 * k)) & 1u);
    }
}

// the border voxels (object, a face neighbour background) into the eight lists, as linear indices of the volume
__global__ void __launch_bounds__(TPB) k_skel_mark(const uint8_t* __restrict__ P, Geo g, Starts st, uint32_t* __restrict__ list, unsigned int* __restrict__ ctr) {
    for (uint64_t item = first_item(); item < g.items(); item += (uint64_t)gridDim.x * WPB) {
        const Turn t = turn_of(g, item);
        uint32_t border = 0;                                           // bit 8k: voxel k of the word is a border voxel
        if (t.valid) {
            const uint8_t* p = P + g.row_base(t.i0, t.i1) + 4u * t.w;
            const uint32_t word = *reinterpret_cast<const uint32_t*>(p);
            if (word) {                                                // (nearly every word of a vessel mask is empty)
                const uint32_t up = *reinterpret_cast<const uint32_t*>(p - g.R), down = *reinterpret_cast<const uint32_t*>(p + g.R);
                const uint32_t back = *reinterpret_cast<const uint32_t*>(p - g.plane), front = *reinterpret_cast<const uint32_t*>(p + g.plane);
                const uint32_t lo = (word << 8) | p[-1], hi = (word >> 8) | ((uint32_t)p[4] << 24);
                border = word & ~(up & down & back & front & lo & hi);
            }
        }
        if (!__ballot(border != 0u)) continue;
        const uint32_t first = (t.i0 * (uint32_t)g.n1 + t.i1) * (uint32_t)g.n2 + 4u * t.w;
#pragma unroll
        for (int q = 0; q < 2; q++) {                                  // voxels q and q + 2 of a word are of one subfield
            const bool a = (border >> (8 * q)) & 1u, b = (border >> (8 * q + 16)) & 1u;
            const unsigned long long ma = __ballot(a), mb = __ballot(b);
            if (!(ma | mb)) continue;
            const uint32_t s = (t.i0 & 1u) * 4u + (t.i1 & 1u) * 2u + q, na = (uint32_t)__popcll(ma);
            unsigned int at = 0;
            if ((threadIdx.x & 63u) == 0u) at = atomicAdd(&ctr[c_list(s)], na + (unsigned int)__popcll(mb));
            at = (unsigned int)__shfl((int)at, 0, 64) + st.at[s];
            if (a) list[at + lanes_below(ma)] = first + q;
            if (b) list[at + na + lanes_below(mb)] = first + q + 2;
        }
    }
}

// step s of a cycle: one thread per listed voxel of subfield s
__global__ void __launch_bounds__(TPB) k_skel_step(uint8_t* __restrict__ P, Geo g, const uint32_t* __restrict__ list, unsigned int* __restrict__ ctr, int s) {
    const uint32_t n = ctr[c_list(s)];
    for (uint32_t i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
        const uint32_t idx = list[i];
        const uint32_t r = idx / (uint32_t)g.n2, i2 = idx - r * (uint32_t)g.n2, i0 = r / (uint32_t)g.n1, i1 = r - i0 * (uint32_t)g.n1;
        uint8_t* p = P + g.row_base(i0, i1) + i2;
        uint32_t obj = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                const uint8_t* q = p + (ptrdiff_t)(a - 1) * (ptrdiff_t)g.plane + (ptrdiff_t)(b - 1) * (ptrdiff_t)g.R;
#pragma unroll
                for (int c = 0; c < 3; c++) if (a * 9 + b * 3 + c != 13) obj |= (uint32_t)q[c - 1] << (a * 9 + b * 3 + c);
            }
        if (deletable(obj)) { *p = 0; atomicAdd(&ctr[C_DEL], 1u); }
    }
}

int grid_items(uint64_t items) { return (int)std::max<uint64_t>(1, std::min<uint64_t>(16384, (items + WPB - 1) / WPB)); }

int skeleton(const uint8_t* volume, Geo g, uint8_t* out, int64_t* kept, int64_t* cycles) {
    const size_t V = (size_t)g.n0 * g.n1 * g.n2;
    DevMem mem;
    const uint8_t* din = nullptr;
    Out<uint8_t> o;
    int rc;
    if ((rc = bring(mem, volume, V, "volume", &din)) || (rc = o.open(mem, out, V, "skeleton"))) return rc;
    uint8_t* P = nullptr; uint32_t* list = nullptr; unsigned int* ctr = nullptr;
    VMASK_GRAB(P, g.bytes(), "padded volume");
    VMASK_GRAB(ctr, C_N, "counters");
    VMASK_TRY(hipMemsetAsync(P, 0, g.bytes(), 0));
    VMASK_TRY(hipMemsetAsync(ctr, 0, C_N * sizeof(unsigned int), 0));
    const int grid = grid_items(g.items());
    k_skel_pad<<<grid, TPB>>>(din, P, g, ctr);
    unsigned int h[8];
    VMASK_TRY(hipMemcpy(h, ctr + C_OBJ, sizeof(h), hipMemcpyDeviceToHost));
    Starts st; uint64_t nobj = 0; int sgrid[8];
    for (int s = 0; s < 8; s++) {
        st.at[s] = (uint32_t)nobj; nobj += h[C_OBJ + s];                 // (a list never holds more than its subfield's object voxels)
        sgrid[s] = (int)std::max<uint32_t>(1u, std::min<uint32_t>(8192u, (h[C_OBJ + s] + TPB - 1) / TPB));
    }
    int64_t ncycles = 0; uint64_t left = nobj;
    if (nobj) {
        VMASK_GRAB(list, nobj, "border lists");
        for (;;) {
            VMASK_TRY(hipMemsetAsync(ctr + C_DEL, 0, (C_N - C_DEL) * sizeof(unsigned int), 0));
            k_skel_mark<<<grid, TPB>>>(P, g, st, list, ctr);
            for (int s = 0; s < 8; s++) k_skel_step<<<sgrid[s], TPB>>>(P, g, list + st.at[s], ctr, s);
            unsigned int deleted = 0;
            VMASK_TRY(hipMemcpy(&deleted, ctr + C_DEL, sizeof(deleted), hipMemcpyDeviceToHost));
            ncycles++;
            left -= deleted;
            if (!deleted) break;
        }
    } else ncycles = 1;                                                  // (the one cycle of an empty volume deletes nothing)
    k_skel_unpad<<<grid, TPB>>>(P, o.dev, g);
    VMASK_TRY(hipGetLastError());
    if (o.dev == out) VMASK_TRY(hipDeviceSynchronize());
    else if ((rc = o.close())) return rc;
    if (kept) *kept = (int64_t)left;
    if (cycles) *cycles = ncycles;
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_skeleton(int device, const uint8_t* volume, int64_t n0, int64_t n1, int64_t n2, uint8_t* out, int64_t* kept, int64_t* cycles) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    Geo g;
    g.n0 = (int32_t)n0; g.n1 = (int32_t)n1; g.n2 = (int32_t)n2;
    g.W = ((uint32_t)n2 + 3u) / 4u; g.cpr = (g.W + 63u) / 64u;
    g.R = 4 * (size_t)g.W + 8; g.plane = (size_t)(n1 + 2) * g.R;
    return skeleton(volume, g, out, kept, cycles);
}
