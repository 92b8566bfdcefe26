// vmask_cc.h - the connected-component labelling of vmask_device.hip for the other translation units behind include/vmask.h
// (vbrain_device.hip).  Declarations only: the kernels and cc_run stay in vmask_device.hip.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vmask {

// Component number - 1 of the root at voxel r = the roots before it in raster order: the roots before its 64-voxel word (off)
// + the roots below it inside the word (bits).
struct CcRank { const unsigned long long* bits; const uint32_t* off; };
__device__ __forceinline__ uint32_t cc_rank(CcRank k, uint32_t r) {
    return k.off[r >> 6] + (uint32_t)__popcll(k.bits[r >> 6] & ((1ull << (r & 63u)) - 1ull));
}

// What a labelling leaves on the device: root[v] = the smallest raster index of v's component (-1: background), the root
// bitmap and its exclusive popcount scan (rank()), ncomp, and - with_sizes only - sizes[rank].  The arrays belong to the
// holder until cc_release.
struct CcOut {
    int32_t* root = nullptr; unsigned long long* bits = nullptr; uint32_t* off = nullptr; unsigned long long* sizes = nullptr;
    uint32_t ncomp = 0;
    void* owned[8] = {}; int nowned = 0;
    CcRank rank() const { return CcRank{bits, off}; }
};
// cc_run on a device-resident uint8 volume (connectivity 1, 2, 3 as vmask_label).  A VRG_* code; on failure nothing is held.
int cc_label(const uint8_t* dvol, int32_t n0, int32_t n1, int32_t n2, int connectivity, bool with_sizes, CcOut& out);
void cc_release(CcOut& out);

}  // namespace vmask
