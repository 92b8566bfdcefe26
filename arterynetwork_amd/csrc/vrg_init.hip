// vrg_init.hip - the backend object, init and the volume of the product backend (vrg_device.h: the overview): streams, options, memory,
// packing of caller arrays, level tables, bins, histograms, the init-mode kernels.
#include "vrg_device.h"

#include <rocprim/rocprim.hpp>

namespace {

// ---- dense helpers over the real voxels -------------------------------------------------------------
__device__ __forceinline__ uint32_t real_idx(const VrgCtx& c, uint64_t t, int& x, int& y, int& z) {
    x = (int)(t % (uint64_t)c.nx); uint64_t r = t / (uint64_t)c.nx;
    y = (int)(r % (uint64_t)c.ny); z = (int)(r / (uint64_t)c.ny);
    return vrg_idx(c, x, y, z);
}
#define VOXEL_LOOP(c) \
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nV_ = (uint64_t)(c).nx * (c).ny * (c).nz; \
         t < nV_; t += (uint64_t)gridDim.x * blockDim.x)

__global__ void k_init_voxel(VrgCtx c) {
    VOXEL_LOOP(c) { int x, y, z; vrg_item_init_voxel(c, real_idx(c, t, x, y, z)); }
}
__global__ void k_hist_voxel(VrgCtx c) {
    VOXEL_LOOP(c) { int x, y, z; vrg_item_hist_voxel(c, real_idx(c, t, x, y, z)); }
}
// same, for level tables that fit LDS (fp32 storage): per-workgroup private histograms (the level values too),
// streamed over the padded interior 16 bytes per lane, flushed with one global atomic per non-zero bin.
constexpr uint32_t HIST_LDS_LEVELS = 4096;
__global__ void __launch_bounds__(TPB) k_hist_lds(VrgCtx c) {
    __shared__ float s_lev[HIST_LDS_LEVELS];
    __shared__ uint32_t s_h[2][HIST_LDS_LEVELS];
    const uint32_t L = c.L;
    for (uint32_t i = threadIdx.x; i < L; i += TPB) { s_lev[i] = (float)c.lev[i]; s_h[0][i] = 0; s_h[1][i] = 0; }
    __syncthreads();
    const uint8_t* __restrict__ in = c.lab[0];
    const uint32_t plane = (uint32_t)c.PY * (uint32_t)c.PX, first = 2u * plane;
    const uint32_t ndw = (uint32_t)(((uint64_t)c.nz * plane) >> 2);
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < ndw; d += gridDim.x * blockDim.x) {
        const uint32_t base = first + (d << 2);
        uint32_t v = *reinterpret_cast<const uint32_t*>(in + base);
        if ((v & 0x24242424u) == 0x24242424u) continue;          // all four excluded or padding
        const float4 f = *reinterpret_cast<const float4*>(c.I + base);
        const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
            uint8_t cb = (uint8_t)(v >> (8 * bb));
            if (cb & (VB_OOB | VB_X)) continue;
            uint32_t lo = 0, hi = L - 1;
            if (c.lev16) lo = c.lev16[base + bb];
            else while (lo < hi) { uint32_t m = (lo + hi) >> 1; if (s_lev[m] < fv[bb]) lo = m + 1; else hi = m; }
            atomicAdd(&s_h[(cb & VB_S) ? 0 : 1][lo], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < L; i += TPB) {
        if (s_h[0][i]) atomicAdd(&c.hin[i], (int32_t)s_h[0][i]);
        if (s_h[1][i]) atomicAdd(&c.hout[i], (int32_t)s_h[1][i]);
    }
}
__global__ void k_init_entry(VrgCtx c) {
    ITEM_LOOP(c.st->ni + c.st->no) vrg_item_init_entry(c, i);
}
__global__ void k_fin_init(VrgCtx c) {
    VrgState& s = *c.st;
    s.np = s.ni + s.no; s.nfree = 0; s.nfresh = 0; s.nfx = 0; s.nf = 0; s.last_nf = 0; s.npend = 0; s.nmk = 0; s.nnz = 0;
    s.nalloc = 0; s.ndead = 0; s.d_ni = 0; s.d_no = 0; s.corr = 0; s.use_tab = 0; s.bail = 0;
    vrg_init_counts(c);
    const VrgDense& d = *c.dn;
    VrgTrace& t = c.trace[0];
    t.nflip = 0; t.nseg = (int64_t)d.n_in; t.n_in = (int64_t)d.n_in; t.n_out = (int64_t)d.n_out; t.ni = s.ni; t.no = s.no;
    t.sum_in = d.sum_in; t.sum_out = d.sum_out; t.ties = 0; t.near_ties = 0;
    s.ties = 0; s.near_ties = 0; s.ties_filed = 0; s.near_filed = 0;
}
__global__ void k_recount_hist(VrgCtx c, int32_t* rin, int32_t* rout) {
    VOXEL_LOOP(c) {
        int x, y, z; uint32_t idx = real_idx(c, t, x, y, z);
        uint8_t bb = c.lab[0][idx];
        if (bb & VB_X) continue;
        uint32_t lev = vrg_level_of(c, vrg_voxel_value(c, idx));
        atomicAdd((bb & VB_S) ? &rin[lev] : &rout[lev], 1);
    }
}
__global__ void k_collect_seg(VrgCtx c, uint64_t* stamps, uint32_t* idxs, uint32_t cap, uint32_t* count) {
    VOXEL_LOOP(c) {
        int x, y, z; uint32_t idx = real_idx(c, t, x, y, z);
        if (c.lab[0][idx] & VB_S) {
            uint32_t p = atomicAdd(count, 1u);
            if (p < cap) { stamps[p] = c.stamp[idx]; idxs[p] = idx; }
        }
    }
}
template <class T> __global__ void k_gather_I(VrgCtx c, T* dst) {
    VOXEL_LOOP(c) { int x, y, z; uint32_t idx = real_idx(c, t, x, y, z); dst[t] = c.I ? (T)c.I[idx] : (T)c.I64[idx]; }
}
__global__ void k_f2d(const float* a, double* b, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) b[i] = (double)a[i];
}

// ---- repacking caller arrays ------------------------------------------------------------------------
__device__ __forceinline__ double load_as_double(const void* p, int dtype, int64_t i) {
    switch (dtype) {
        case 0: return ((const uint8_t*)p)[i];
        case 1: return ((const int16_t*)p)[i];
        case 2: return ((const uint16_t*)p)[i];
        case 3: return ((const int32_t*)p)[i];
        case 4: return (double)((const int64_t*)p)[i];
        case 5: return ((const float*)p)[i];
        default: return ((const double*)p)[i];
    }
}
__device__ __forceinline__ void store_int(void* p, int dtype, int64_t i, int v) {
    switch (dtype) {
        case 0: ((uint8_t*)p)[i] = (uint8_t)v; break;
        case 1: ((int16_t*)p)[i] = (int16_t)v; break;
        case 2: ((uint16_t*)p)[i] = (uint16_t)v; break;
        case 3: ((int32_t*)p)[i] = v; break;
        case 4: ((int64_t*)p)[i] = v; break;
        case 5: ((float*)p)[i] = (float)v; break;
        default: ((double*)p)[i] = v; break;
    }
}
// (nz: the number of non-zero values - np.count_nonzero(dataArray) of the reference's closing message, :95 - counted on the way)
__global__ void k_pack_volume(VrgCtx c, float* dst, double* dst64, const void* src, int dtype, int64_t s0, int64_t s1, int64_t s2, int* flag, unsigned long long* nz) {
    unsigned long long mine = 0;
    VOXEL_LOOP(c) {
        int x, y, z; uint32_t idx = real_idx(c, t, x, y, z);
        double v = load_as_double(src, dtype, x * s0 + y * s1 + z * s2);
        mine += v != 0.0;
        if (dst64) { dst64[idx] = v; continue; }
        float f = (float)v;
        if ((double)f != v) *flag = 1;
        dst[idx] = f;
    }
    mine = (unsigned long long)wave_sum((long long)mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(nz, mine);
}
__global__ void k_pack_labels(VrgCtx c, uint8_t* dst, const void* src, int dtype, int64_t s0, int64_t s1, int64_t s2, int* flag) {
    VOXEL_LOOP(c) {
        int x, y, z; uint32_t idx = real_idx(c, t, x, y, z);
        double v = load_as_double(src, dtype, x * s0 + y * s1 + z * s2);
        uint8_t bb = 0;
        if (v == 0) bb = VB_S; else if (v == 3) bb = 0; else if (v == 4) bb = VB_X; else *flag = 1;
        dst[idx] = bb;
    }
}
__global__ void k_unpack_labels(VrgCtx c, const uint8_t* lab, void* dst, int dtype, int64_t s0, int64_t s1, int64_t s2, int what) {
    VOXEL_LOOP(c) {
        int x, y, z; uint32_t idx = real_idx(c, t, x, y, z);
        const int v = vrg_dec(lab[idx]);
        store_int(dst, dtype, x * s0 + y * s1 + z * s2, what ? (v <= 1 ? 1 : 0) : v);
    }
}
__global__ void k_build_lev16(VrgCtx c, uint16_t* dst) {
    VOXEL_LOOP(c) { int x, y, z; uint32_t idx = real_idx(c, t, x, y, z); dst[idx] = (uint16_t)vrg_level_of(c, vrg_voxel_value(c, idx)); }
}

// 16-bit storage, the dense pass's memo (option dense_memo): gsum[g] = the sum of the values the pass would add for the 256 voxels
// of group g (unit g >> 2, class byte g & 3: voxels 256 g + 4 lane + 0..3).  One wave per group; the order of the additions
// is fixed and does not depend on the grid: every lane adds its four values in voxel order, then the butterfly of wave_sum.
__global__ void __launch_bounds__(TPB) k_build_gsum(const uint16_t* lev16, const double* lev, uint32_t ngroups, double* gsum) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t g = wave; g < ngroups; g += nwaves) {
        const uint16_t* p = lev16 + ((size_t)g << 8) + (lane << 2);
        double s = (double)(float)lev[p[0]];
        s += (double)(float)lev[p[1]]; s += (double)(float)lev[p[2]]; s += (double)(float)lev[p[3]];
        s = wave_sum(s);
        if (lane == 0) gsum[g] = s;
    }
}

// ... and the memo of the rim groups (dense_memo = 2): isum[g] = the same sum over the voxels of group g that are included (class
// not 0) in the class bits as init has just built them, an excluded voxel adding +0.0 - the same additions in the same order, so a
// group without excluded voxels gets gsum[g] bit for bit -, and icnt[g] = how many they are (0..256).
__global__ void __launch_bounds__(TPB) k_build_rim(const uint32_t* cls, const uint16_t* lev16, const double* lev, uint32_t ngroups, double* isum, uint16_t* icnt) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t g = wave; g < ngroups; g += nwaves) {
        const uint32_t wj = (cls[((size_t)(g >> 2) << 6) + lane] >> (8u * (g & 3u))) & 0xffu;
        const uint16_t* p = lev16 + ((size_t)g << 8) + (lane << 2);
        double s = (wj & 0x03u) ? (double)(float)lev[p[0]] : 0.0;
        s += (wj & 0x0cu) ? (double)(float)lev[p[1]] : 0.0; s += (wj & 0x30u) ? (double)(float)lev[p[2]] : 0.0; s += (wj & 0xc0u) ? (double)(float)lev[p[3]] : 0.0;
        s = wave_sum(s);
        const long long n = wave_sum((long long)__popc((wj | (wj >> 1)) & 0x55u));
        if (lane == 0) { isum[g] = s; icnt[g] = (uint16_t)n; }
    }
}

const size_t kElem[7] = {1, 2, 2, 4, 8, 4, 8};

// strides must describe a dense permutation of the three axes (numpy C or F order)
bool dense_strides(const VrgCtx& c, const int64_t st[3]) {
    int64_t dim[3] = {c.nx, c.ny, c.nz};
    int o[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++) for (int j = i + 1; j < 3; j++) if (st[o[j]] < st[o[i]]) { int t = o[i]; o[i] = o[j]; o[j] = t; }
    int64_t expect = 1;
    for (int i = 0; i < 3; i++) {
        if (dim[o[i]] == 1) continue;                 // stride of a length-1 axis is irrelevant
        if (st[o[i]] != expect) return false;
        expect *= dim[o[i]];
    }
    return true;
}
bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}
int voxel_blocks(const VrgCtx& c) {
    uint64_t V = (uint64_t)c.nx * c.ny * c.nz;
    return (int)std::min<uint64_t>(4096, (V + TPB - 1) / TPB);
}


void make_streams(VrgBackend* b) {
    int lo = 0, hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));      // hi = numerically lowest = highest priority
    if (b->sa) { HIP_CHECK(hipStreamSynchronize(b->sa)); HIP_CHECK(hipStreamDestroy(b->sa)); }
    if (b->sb) { HIP_CHECK(hipStreamSynchronize(b->sb)); HIP_CHECK(hipStreamDestroy(b->sb)); }
    // prio_mode 0: equal; 1: band stream A high; 2: dense stream B high
    // (keeping the dense pass off 1-8 CUs of every XCD with a CU-masked stream - free places for the band chain - was measured in
    // round 4: the chain beside a pass stays at 37 us, the pass gets 3-20 % slower: what the chain waits for is memory, not a place)
    HIP_CHECK(hipStreamCreateWithPriority(&b->sa, hipStreamNonBlocking, b->prio_mode == 1 ? hi : (b->prio_mode == 2 ? lo : 0)));
    HIP_CHECK(hipStreamCreateWithPriority(&b->sb, hipStreamNonBlocking, b->prio_mode == 2 ? hi : (b->prio_mode == 1 ? lo : 0)));
}

}  // namespace

void use_device(VrgBackend* b) { HIP_CHECK(hipSetDevice(b->device)); }

// ---- backend interface ---------------------------------------------------------------------------------
VrgBackend* be_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    VrgBackend* b = new VrgBackend();
    b->device = device;
    make_streams(b);
    if (b->err[0]) { be_destroy(b); return nullptr; }
    return b;
}
void be_destroy(VrgBackend* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->rsv) (void)hipFree(b->rsv);
    if (b->gsum) (void)hipFree(b->gsum);
    if (b->isum) (void)hipFree(b->isum);
    if (b->sa) (void)hipStreamSynchronize(b->sa);
    if (b->sb) (void)hipStreamSynchronize(b->sb);
    if (b->comm) { ncclCommDestroy(b->comm); b->comm = nullptr; }
    for (auto& p : b->ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (int j = 0; j < 4; j++) if (b->mark[j]) (void)hipEventDestroy(b->mark[j]);
    if (b->tmp) (void)hipFree(b->tmp);
    for (int j = 0; j < 2; j++) if (b->xfer[j]) (void)hipHostFree(b->xfer[j]);
    if (b->keys2) (void)hipFree(b->keys2);
    if (b->sa) (void)hipStreamDestroy(b->sa);
    if (b->sb) (void)hipStreamDestroy(b->sb);
    if (b->sc) { (void)hipStreamSynchronize(b->sc); (void)hipStreamDestroy(b->sc); }
    if (b->sd) { (void)hipStreamSynchronize(b->sd); (void)hipStreamDestroy(b->sd); }
    delete b;
}
void be_set_tuning(VrgBackend* b, const char* name, long long v) {
    use_device(b);
    if (std::strcmp(name, "sweep_blocks") == 0 && v >= 0 && v <= 4096) b->sweep_blocks = (int)v;
    if (std::strcmp(name, "serial_streams") == 0) b->serial = v != 0;
    if (std::strcmp(name, "repl") == 0) b->repl = v != 0;
    if (std::strcmp(name, "skip_excluded") == 0) b->skip = v != 0;
    if (std::strcmp(name, "nt_loads") == 0) b->nt_loads = v < 0 ? -1 : (v != 0);
    if (std::strcmp(name, "iter_hint") == 0) b->iter_hint = (int)v;
    if (std::strcmp(name, "open_sweeps") == 0) b->open_sweeps = v != 0;
    if (std::strcmp(name, "mark_compact") == 0) b->mark_compact = v != 0;
    if (std::strcmp(name, "band_blocks_max") == 0 && v >= 32 && v <= BAND_BLOCKS) b->band_blocks_max = (uint32_t)v;
    if (std::strcmp(name, "band_hint") == 0) b->band_hint = (uint32_t)std::min<long long>(std::max<long long>(v, 0), 0x7fffffff);
    if (std::strcmp(name, "direct_hint") == 0) b->direct_hint = v != 0;
    if (std::strcmp(name, "dense_pipe") == 0) b->dense_pipe = (int)v;
    if (std::strcmp(name, "dense_close") == 0) { dense_close_open(b); b->dense_close = v != 0; }
    if (std::strcmp(name, "dense_memo") == 0) b->dense_memo = v < 0 ? -1 : (v == 2 ? 2 : (v != 0));
    if (std::strcmp(name, "memo_above") == 0 && v >= 0) b->memo_above = (uint32_t)std::min<long long>(v, 0x7fffffff);
    if (std::strcmp(name, "verify_every") == 0 && v >= 0) b->verify_every = (int)std::min<long long>(v, 1 << 20);
    if (std::strcmp(name, "small_flips") == 0 && v >= 0) b->small_flips = (uint32_t)std::min<long long>(v, NF_WIDE);
    if (std::strcmp(name, "flip_hint") == 0) {           // (a sweep as large as the one that came back has been applied: the floor has done its job)
        const uint32_t f = (uint32_t)std::min<long long>(std::max<long long>(v, 0), 0x7fffffff);
        if (f >= b->flip_hint_min) b->flip_hint_min = 0;
        b->flip_hint = std::max(f, b->flip_hint_min);
    }
    if (std::strcmp(name, "flip_hint_min") == 0) { b->flip_hint_min = (uint32_t)std::min<long long>(std::max<long long>(v, 0), 0x7fffffff); b->flip_hint = std::max(b->flip_hint, b->flip_hint_min); }
    if (std::strcmp(name, "prio_mode") == 0 && v >= 0 && v <= 2 && v != b->prio_mode) { b->prio_mode = (int)v; make_streams(b); }
}
void* be_alloc(VrgBackend* b, size_t bytes) { use_device(b); void* p = nullptr; if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
static void drop_gsum(VrgBackend* b) { if (b->gsum) HIP_CHECK(hipFree(b->gsum)); b->gsum = nullptr; b->gsum_bytes = 0; b->gsum_for = nullptr; }
static void drop_rim(VrgBackend* b) { if (b->isum) HIP_CHECK(hipFree(b->isum)); b->isum = nullptr; b->rim_bytes = 0; b->rim_for = nullptr; }
void be_free(VrgBackend* b, void* p) {
    use_device(b);
    if (p && p == (const void*)b->gsum_for) drop_gsum(b);        // (the engine drops the 16-bit level indices: their group sums go with them)
    if (p && p == (const void*)b->rim_for) drop_rim(b);
    HIP_CHECK(hipFree(p));
}
void be_fill(VrgBackend* b, void* p, int byte, size_t bytes) { use_device(b); HIP_CHECK(hipMemsetAsync(p, byte, bytes, b->sa)); }
void be_upload(VrgBackend* b, void* dst, const void* src, size_t bytes) { use_device(b); HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, b->sa)); HIP_CHECK(hipStreamSynchronize(b->sa)); }
void be_download(VrgBackend* b, void* dst, const void* src, size_t bytes) { use_device(b); HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, b->sa)); HIP_CHECK(hipStreamSynchronize(b->sa)); }
void be_copy(VrgBackend* b, void* dst, const void* src, size_t bytes) { use_device(b); HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, b->sa)); }
const char* be_last_error(VrgBackend* b) {
    if (!b->err[0]) { (void)hipSetDevice(b->device); hipError_t e = hipGetLastError(); if (e != hipSuccess) std::snprintf(b->err, sizeof(b->err), "HIP error '%s' (asynchronous)", hipGetErrorString(e)); }
    return b->err[0] ? b->err : nullptr;
}
void be_clear_error(VrgBackend* b) { b->err[0] = 0; }
// (the engine synchronises when a run ends or a trip was handed back: no fused sweep is waiting for its dense pass then)
bool be_band_busy(VrgBackend* b) { use_device(b); const hipError_t e = hipStreamQuery(b->sa); if (e == hipErrorNotReady) { (void)hipGetLastError(); return true; } return false; }
void be_sync(VrgBackend* b) { use_device(b); dense_close_open(b); HIP_CHECK(hipStreamSynchronize(b->sa)); HIP_CHECK(hipStreamSynchronize(b->sb)); if (b->sd) HIP_CHECK(hipStreamSynchronize(b->sd)); b->fused_prev = false; b->prev_open = false; }

// A device-resident input is read on the library's own stream: the caller's producer must have finished (vrg.h).
// ---- host arrays in and out --------------------------------------------------------------------------------------------------------
// The reference's own calling convention is int64 valueMap and int / float64 dataArray (variationalRegionGrowing.py:44-46, :288): 8 bytes per
// voxel each way over PCIe from pageable memory.  A HOST array wider than what the device keeps is therefore narrowed on the host first -
// labels to one byte, intensities to fp32 when every value survives that (else the raw array travels: the volume is kept as float64) - by a
// few threads, a chunk at a time through two page-locked buffers, so that the narrowing of one chunk overlaps the copy of the chunk before;
// results go the other way: one byte per voxel comes back and is widened into the caller's array on the host.
constexpr size_t XFER_CHUNK = 32u << 20;              // elements per chunk
static int host_threads() { const unsigned n = std::thread::hardware_concurrency(); return (int)std::min<unsigned>(16u, std::max<unsigned>(1u, n)); }
template <class F> static void parallel_chunks(size_t n, F f) {                  // f(begin, end) on a few threads
    const int nt = n < (1u << 20) ? 1 : host_threads();
    if (nt == 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (int t = 0; t < nt; t++) { const size_t a = std::min(n, t * per), e = std::min(n, a + per); if (a < e) th.emplace_back([=] { f(a, e); }); }
    for (auto& x : th) x.join();
}
static bool xfer_buffers(VrgBackend* b, size_t bytes) {
    if (b->xfer_bytes >= bytes) return true;
    for (int j = 0; j < 2; j++) { if (b->xfer[j]) (void)hipHostFree(b->xfer[j]); b->xfer[j] = nullptr; }
    b->xfer_bytes = 0;
    for (int j = 0; j < 2; j++) if (hipHostMalloc(&b->xfer[j], bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
    b->xfer_bytes = bytes;
    return true;
}
template <class T> static double host_load(const void* p, size_t i) { return (double)((const T*)p)[i]; }
static double host_load_as_double(const void* p, int dtype, size_t i) {
    switch (dtype) { case 0: return host_load<uint8_t>(p, i); case 1: return host_load<int16_t>(p, i); case 2: return host_load<uint16_t>(p, i); case 3: return host_load<int32_t>(p, i);
                     case 4: return host_load<int64_t>(p, i); case 5: return host_load<float>(p, i); default: return host_load<double>(p, i); }
}
// a host array of V elements narrowed to `out_elem`-byte elements (1: label bytes, 255 for a value that is no label; 4: fp32) and copied to
// device memory `dev`, chunk by chunk; *flag: a value did not survive (labels: not 0 / 3 / 4; intensities: not exact in fp32 - the copy stops)
static bool narrow_to_device(VrgBackend* b, void* dev, const void* src, int dtype, size_t V, int out_elem, int* flag) {
    if (!xfer_buffers(b, XFER_CHUNK * 4)) return false;
    *flag = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int j = 0; j < 2; j++) HIP_CHECK(hipEventCreateWithFlags(&ev[j], hipEventDisableTiming));
    int k = 0;
    for (size_t i0 = 0; i0 < V; i0 += XFER_CHUNK, k ^= 1) {
        const size_t n = std::min(XFER_CHUNK, V - i0);
        HIP_CHECK(hipEventSynchronize(ev[k]));           // (the copy that last used this buffer is done)
        std::atomic<int> bad{0};
        void* buf = b->xfer[k];
        parallel_chunks(n, [&](size_t a, size_t e) {
            int mine = 0;
            if (out_elem == 1) { uint8_t* o = (uint8_t*)buf; for (size_t i = a; i < e; i++) { const double v = host_load_as_double(src, dtype, i0 + i); const bool ok = v == 0 || v == 3 || v == 4; o[i] = ok ? (uint8_t)v : 255; mine |= !ok; } }
            else { float* o = (float*)buf; for (size_t i = a; i < e; i++) { const double v = host_load_as_double(src, dtype, i0 + i); const float f = (float)v; o[i] = f; mine |= ((double)f != v); } }
            if (mine) bad.store(1);
        });
        if (bad.load()) { *flag = 1; if (out_elem == 4) break; }
        HIP_CHECK(hipMemcpyAsync((uint8_t*)dev + i0 * out_elem, buf, n * out_elem, hipMemcpyHostToDevice, b->sa));
        HIP_CHECK(hipEventRecord(ev[k], b->sa));
    }
    HIP_CHECK(hipStreamSynchronize(b->sa));
    for (int j = 0; j < 2; j++) (void)hipEventDestroy(ev[j]);
    return true;
}
// A device-resident input is read on the library's own stream: the caller's producer must have finished (vrg.h).
// *dtype_dev: the element type of what is on the device (a narrowed host array: VRG_U8 / VRG_F32); *early: the narrowing already
// answered the question the kernel would have answered (an intensity that fp32 cannot hold: nothing was copied)
static const void* stage_in(VrgBackend* b, const VrgCtx& c, const void* src, int dtype, void** tmp, int* dtype_dev, int narrow_to, int* early) {
    *tmp = nullptr; *dtype_dev = dtype; *early = 0;
    if (is_device_ptr(src)) return src;
    const size_t V = (size_t)c.nx * c.ny * c.nz;
    if (narrow_to && (int)kElem[dtype] > narrow_to) {
        if (hipMalloc(tmp, V * narrow_to) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        int flag = 0;
        if (!narrow_to_device(b, *tmp, src, dtype, V, narrow_to, &flag)) { HIP_CHECK(hipFree(*tmp)); *tmp = nullptr; return nullptr; }
        if (flag && narrow_to == 4) { *early = 1; return *tmp; }           // (the volume is kept as float64: the caller comes again for the raw array)
        *dtype_dev = narrow_to == 1 ? VRG_U8 : VRG_F32;
        return *tmp;
    }
    size_t bytes = V * kElem[dtype];
    if (hipMalloc(tmp, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    HIP_CHECK(hipMemcpyAsync(*tmp, src, bytes, hipMemcpyHostToDevice, b->sa));
    return *tmp;
}

int be_pack_volume(VrgBackend* b, const VrgCtx& c, float* dst, double* dst64, const void* src, int dtype, const int64_t st[3], int* inexact, long long* nonzero) {
    use_device(b);
    if (!dense_strides(c, st)) return -1;
    void* tmp; int dt = dtype, early = 0;
    const void* d = stage_in(b, c, src, dtype, &tmp, &dt, dst64 ? 0 : 4, &early);     // (the fp32 attempt narrows a wide host array; the float64 pass takes it raw)
    if (!d) return -1;
    if (early) { *inexact = 1; HIP_CHECK(hipFree(tmp)); return 0; }
    struct { int flag; int pad; unsigned long long nz; } host = {0, 0, 0}, *dev = nullptr;
    HIP_CHECK(hipMalloc(&dev, sizeof(host))); HIP_CHECK(hipMemsetAsync(dev, 0, sizeof(host), b->sa));
    k_pack_volume<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, dst, dst64, d, dt, st[0], st[1], st[2], &dev->flag, &dev->nz);
    HIP_CHECK(hipMemcpyAsync(&host, dev, sizeof(host), hipMemcpyDeviceToHost, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    *inexact = host.flag; if (nonzero) *nonzero = (long long)host.nz;
    HIP_CHECK(hipFree(dev)); if (tmp) HIP_CHECK(hipFree(tmp));
    return 0;
}
int be_pack_labels(VrgBackend* b, const VrgCtx& c, uint8_t* dst, const void* src, int dtype, const int64_t st[3], int* bad) {
    use_device(b);
    if (!dense_strides(c, st)) return -1;
    void* tmp; int dt = dtype, early = 0;
    const void* d = stage_in(b, c, src, dtype, &tmp, &dt, 1, &early);
    if (!d) return -1;
    int* flag; HIP_CHECK(hipMalloc(&flag, sizeof(int))); HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), b->sa));
    k_pack_labels<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, dst, d, dt, st[0], st[1], st[2], flag);
    HIP_CHECK(hipMemcpyAsync(bad, flag, sizeof(int), hipMemcpyDeviceToHost, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    HIP_CHECK(hipFree(flag)); if (tmp) HIP_CHECK(hipFree(tmp));
    return 0;
}
template <class T> static void host_widen(void* dst, const uint8_t* src, size_t a, size_t e) { T* o = (T*)dst; for (size_t i = a; i < e; i++) o[i] = (T)src[i]; }
// what: 0 = the labels 0..4 (valueMap on return, :33-36), 1 = segmentedMap (labels <= 1 -> 1, else 0: :31-32)
int be_unpack_labels(VrgBackend* b, const VrgCtx& c, const uint8_t* lab, void* dst, int dtype, const int64_t st[3], int what) {
    use_device(b);
    if (!dense_strides(c, st)) return -1;
    bool dev = is_device_ptr(dst);
    const size_t V = (size_t)c.nx * c.ny * c.nz;
    if (dev) {
        k_unpack_labels<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, lab, dst, dtype, st[0], st[1], st[2], what);
        HIP_CHECK(hipStreamSynchronize(b->sa));
        return 0;
    }
    // a host array: one byte per voxel in the caller's layout comes back, widened on the host chunk by chunk
    void* d = nullptr;
    if (hipMalloc(&d, V) != hipSuccess) { (void)hipGetLastError(); return -1; }
    k_unpack_labels<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, lab, d, VRG_U8, st[0], st[1], st[2], what);
    if (kElem[dtype] == 1) { HIP_CHECK(hipMemcpyAsync(dst, d, V, hipMemcpyDeviceToHost, b->sa)); HIP_CHECK(hipStreamSynchronize(b->sa)); HIP_CHECK(hipFree(d)); return 0; }
    if (!xfer_buffers(b, XFER_CHUNK * 4)) { HIP_CHECK(hipFree(d)); return -1; }
    int k = 0;
    size_t prev0 = 0, prevn = 0; int prevk = -1;
    auto widen = [&](size_t i0, size_t n, int kk) {
        const uint8_t* srcb = (const uint8_t*)b->xfer[kk];
        uint8_t* base = (uint8_t*)dst + i0 * kElem[dtype];
        parallel_chunks(n, [&](size_t a, size_t e) {
            switch (dtype) { case 1: host_widen<int16_t>(base, srcb, a, e); break; case 2: host_widen<uint16_t>(base, srcb, a, e); break; case 3: host_widen<int32_t>(base, srcb, a, e); break;
                             case 4: host_widen<int64_t>(base, srcb, a, e); break; case 5: host_widen<float>(base, srcb, a, e); break; default: host_widen<double>(base, srcb, a, e); break; }
        });
    };
    for (size_t i0 = 0; i0 < V; i0 += XFER_CHUNK, k ^= 1) {
        const size_t n = std::min(XFER_CHUNK, V - i0);
        HIP_CHECK(hipMemcpyAsync(b->xfer[k], (const uint8_t*)d + i0, n, hipMemcpyDeviceToHost, b->sa));
        if (prevk >= 0) widen(prev0, prevn, prevk);        // (the chunk before, while this one travels)
        HIP_CHECK(hipStreamSynchronize(b->sa));
        prev0 = i0; prevn = n; prevk = k;
    }
    if (prevk >= 0) widen(prev0, prevn, prevk);
    HIP_CHECK(hipFree(d));
    return 0;
}

// sorted distinct intensity values (rocPRIM radix sort + unique), as float64
template <class T> static int build_levels_t(VrgBackend* b, const VrgCtx& c, double** lev, uint32_t* L) {
    size_t V = (size_t)c.nx * c.ny * c.nz;
    T *a = nullptr, *bb = nullptr; uint32_t* cnt = nullptr; void* tmp = nullptr; size_t tb = 0, tb2 = 0;
    int rc = -1;
    double* out = nullptr;
    if (hipMalloc(&a, V * sizeof(T)) == hipSuccess && hipMalloc(&bb, V * sizeof(T)) == hipSuccess && hipMalloc(&cnt, 4) == hipSuccess) {
        k_gather_I<T><<<voxel_blocks(c), TPB, 0, b->sa>>>(c, a);
        HIP_CHECK(rocprim::radix_sort_keys(nullptr, tb, a, bb, V, 0, 8 * sizeof(T), b->sa));
        HIP_CHECK(rocprim::unique(nullptr, tb2, bb, a, cnt, V, rocprim::equal_to<T>(), b->sa));
        tb = std::max(tb, tb2);
        if (hipMalloc(&tmp, tb) == hipSuccess) {
            HIP_CHECK(rocprim::radix_sort_keys(tmp, tb, a, bb, V, 0, 8 * sizeof(T), b->sa));
            HIP_CHECK(rocprim::unique(tmp, tb, bb, a, cnt, V, rocprim::equal_to<T>(), b->sa));
            uint32_t n = 0;
            HIP_CHECK(hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, b->sa));
            HIP_CHECK(hipStreamSynchronize(b->sa));
            if (n && hipMalloc(&out, (size_t)n * 8) == hipSuccess) {
                if (sizeof(T) == 4) k_f2d<<<256, TPB, 0, b->sa>>>((const float*)a, out, n);
                else HIP_CHECK(hipMemcpyAsync(out, a, (size_t)n * 8, hipMemcpyDeviceToDevice, b->sa));
                HIP_CHECK(hipStreamSynchronize(b->sa));
                *lev = out; *L = n; rc = 0;
            }
        }
    }
    (void)hipGetLastError();
    if (a) HIP_CHECK(hipFree(a)); if (bb) HIP_CHECK(hipFree(bb)); if (cnt) HIP_CHECK(hipFree(cnt)); if (tmp) HIP_CHECK(hipFree(tmp));
    return rc;
}
int be_build_levels(VrgBackend* b, const VrgCtx& c, double** lev, uint32_t* L) {
    use_device(b);
    return c.I ? build_levels_t<float>(b, c, lev, L) : build_levels_t<double>(b, c, lev, L);
}

__global__ void k_lev_map(VrgCtx c, uint16_t* map, int* bad) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < c.L; k += gridDim.x * blockDim.x) {
        const double v = c.lev[k];
        if (v != floor(v)) *bad = 1; else map[(uint32_t)(v - c.lev[0])] = (uint16_t)k;
    }
}
bool be_build_lev_map(VrgBackend* b, const VrgCtx& c, uint16_t* map, uint32_t span) {
    use_device(b);
    int* bad = nullptr; int hbad = 1;
    if (hipMalloc(&bad, sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return false; }
    HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), b->sa));
    HIP_CHECK(hipMemsetAsync(map, 0xff, (size_t)span * 2, b->sa));
    k_lev_map<<<(c.L + TPB - 1) / TPB, TPB, 0, b->sa>>>(c, map, bad);
    HIP_CHECK(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    HIP_CHECK(hipFree(bad));
    return hbad == 0;
}

__global__ void k_ktab(VrgCtx c, double* ktab) {
    const uint64_t n = (uint64_t)c.L * c.L;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = (uint32_t)(i / c.L), b = (uint32_t)(i - (uint64_t)a * c.L);
        ktab[i] = vrg_kern(c, c.lev[b] - c.lev[a]);
    }
}
void be_build_ktab(VrgBackend* b, const VrgCtx& c, double* ktab) { use_device(b); k_ktab<<<1024, TPB, 0, b->sa>>>(c, ktab); }

// the bins' moments from the per-level class histograms (init; fixed-point integer adds: any order gives the same bits)
__global__ void k_bins_build(VrgCtx c) {
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < c.L; l += gridDim.x * blockDim.x) {
        const int32_t a = c.hin[l], b = c.hout[l];
        if (a | b) vrg_bin_add(c, c.lev[l], a, b);
    }
}
// ... and how many of them differ from `ref_in` / `ref_out` built the same way from other histograms (verification aid)
__global__ void k_bins_diff(VrgCtx c, const int64_t* ref_in, const int64_t* ref_out, unsigned long long* out) {
    const uint64_t n = (uint64_t)c.nb * (VRG_BIN_K + 1);
    unsigned long long bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) bad += (c.bm_in[i] != ref_in[i]) + (c.bm_out[i] != ref_out[i]);
    if (bad) atomicAdd(out, bad);
}
void be_build_bins(VrgBackend* b, const VrgCtx& c) {
    use_device(b);
    HIP_CHECK(hipMemsetAsync(c.bm_in, 0, (size_t)c.nb * (VRG_BIN_K + 1) * 8, b->sa)); HIP_CHECK(hipMemsetAsync(c.bm_out, 0, (size_t)c.nb * (VRG_BIN_K + 1) * 8, b->sa));
    k_bins_build<<<2048, TPB, 0, b->sa>>>(c);
}
long long be_check_bins(VrgBackend* b, const VrgCtx& c, const int32_t* rin, const int32_t* rout) {
    use_device(b);
    if (!c.nb) return 0;
    const size_t bytes = (size_t)c.nb * (VRG_BIN_K + 1) * 8;
    int64_t *ri = nullptr, *ro = nullptr; unsigned long long* d = nullptr; unsigned long long bad = ~0ull;
    if (hipMalloc(&ri, bytes) == hipSuccess && hipMalloc(&ro, bytes) == hipSuccess && hipMalloc(&d, 8) == hipSuccess) {
        VrgCtx r = c;
        r.bm_in = ri; r.bm_out = ro; r.hin = const_cast<int32_t*>(rin); r.hout = const_cast<int32_t*>(rout);
        HIP_CHECK(hipMemsetAsync(ri, 0, bytes, b->sa)); HIP_CHECK(hipMemsetAsync(ro, 0, bytes, b->sa)); HIP_CHECK(hipMemsetAsync(d, 0, 8, b->sa));
        k_bins_build<<<2048, TPB, 0, b->sa>>>(r);
        k_bins_diff<<<256, TPB, 0, b->sa>>>(c, ri, ro, d);
        HIP_CHECK(hipMemcpyAsync(&bad, d, 8, hipMemcpyDeviceToHost, b->sa));
        HIP_CHECK(hipStreamSynchronize(b->sa));
    }
    (void)hipGetLastError();
    if (ri) HIP_CHECK(hipFree(ri)); if (ro) HIP_CHECK(hipFree(ro)); if (d) HIP_CHECK(hipFree(d));
    return (long long)bad;
}

__global__ void k_build_lidx(VrgCtx c, uint32_t* dst) {
    VOXEL_LOOP(c) { int x, y, z; uint32_t idx = real_idx(c, t, x, y, z); dst[idx] = vrg_level_of(c, vrg_voxel_value(c, idx)); }
}
void be_build_lidx(VrgBackend* b, const VrgCtx& c, uint32_t* dst) {
    use_device(b);
    HIP_CHECK(hipMemsetAsync(dst, 0, ((size_t)c.PV + 1023) / 1024 * 1024 * 4, b->sa));
    k_build_lidx<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, dst);
}
void be_build_lev16(VrgBackend* b, const VrgCtx& c, uint16_t* dst) {
    use_device(b);
    HIP_CHECK(hipMemsetAsync(dst, 0, ((size_t)c.PV + 1023) / 1024 * 1024 * 2, b->sa));
    k_build_lev16<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, dst);
    // ... and the sums of their 256-voxel groups (the dense pass's memo): rebuilt whenever the indices are.  Without the memory for
    // them (8 B per 256 voxels) the pass counts every group voxel by voxel.
    drop_rim(b);                               // (the rim groups' tables belong to the old indices: the next init builds them anew, build_rim)
    const size_t ngroups = ((size_t)c.PV + 1023) / 1024 * 4;
    if (b->gsum_bytes != ngroups * sizeof(double)) {
        drop_gsum(b);
        if (hipMalloc((void**)&b->gsum, ngroups * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); b->gsum = nullptr; return; }
        b->gsum_bytes = ngroups * sizeof(double);
    }
    b->gsum_for = dst;
    k_build_gsum<<<4096, TPB, 0, b->sa>>>(dst, c.lev, (uint32_t)ngroups, b->gsum);
}

// The rim groups' tables (dense_memo = 2; k_build_rim), from the class bits init_dense has just built: at EVERY init - the labels may
// be new - and only with 16-bit storage.  One allocation of 10 B per group, the sums in front.  Without the memory for it the pass
// runs without them (dense_memo in vrg_device.hip).
void build_rim(VrgBackend* b, const VrgCtx& c) {
    // ... and only where the option can select them: not with dense_memo = 0 or 1, nor by default on a volume of up to 100 000 units
    if (!c.lev16 || !b->skip || b->dense_memo == 0 || b->dense_memo == 1 || (b->dense_memo < 0 && ((uint64_t)c.PV >> 10) <= 100000)) { drop_rim(b); return; }
    const size_t ngroups = ((size_t)c.PV + 1023) / 1024 * 4;
    if (b->rim_bytes != ngroups * 10) {
        drop_rim(b);
        if (hipMalloc((void**)&b->isum, ngroups * 10) != hipSuccess) { (void)hipGetLastError(); b->isum = nullptr; return; }
        b->rim_bytes = ngroups * 10;
    }
    b->rim_for = c.lev16;
    k_build_rim<<<4096, TPB, 0, b->sa>>>(c.clsb[0], c.lev16, c.lev, (uint32_t)ngroups, b->isum, reinterpret_cast<uint16_t*>(b->isum + ngroups));
}

void be_init_band(VrgBackend* b, const VrgCtx& c) {
    use_device(b);
    k_init_voxel<<<voxel_blocks(c), TPB, 0, b->sa>>>(c);
}

void be_init_sort(VrgBackend* b, const VrgCtx& c, uint32_t n_in, uint32_t n_out) {
    use_device(b);
    uint32_t nmax = std::max(n_in, n_out);
    if (nmax == 0) return;
    uint64_t* kout = nullptr; void* tmp = nullptr; size_t tb = 0;
    HIP_CHECK(hipMalloc(&kout, (size_t)nmax * 8));
    HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tb, c.init_key, kout, c.init_idx, c.p_idx, nmax, 0, 64, b->sa));
    HIP_CHECK(hipMalloc(&tmp, tb));
    if (n_in) HIP_CHECK(rocprim::radix_sort_pairs(tmp, tb, c.init_key, kout, c.init_idx, c.p_idx, n_in, 0, 64, b->sa));
    if (n_out) HIP_CHECK(rocprim::radix_sort_pairs(tmp, tb, c.init_key + (c.bcap - n_out), kout, c.init_idx + (c.bcap - n_out),
                                                   c.p_idx + n_in, n_out, 0, 64, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    HIP_CHECK(hipFree(kout)); HIP_CHECK(hipFree(tmp));
}

void be_init_finish(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user) {
    use_device(b);
    b->dense_pending = 0;
    dense_close_open(b);
    HIP_CHECK(hipStreamSynchronize(b->sb));     // both class copies are rebuilt: no dense pass may be in flight
    k_init_entry<<<ITEM_BLOCKS, TPB, 0, b->sa>>>(c);
    if (c.I && c.L <= HIST_LDS_LEVELS) k_hist_lds<<<1024, TPB, 0, b->sa>>>(c);
    else k_hist_voxel<<<voxel_blocks(c), TPB, 0, b->sa>>>(c);
    if (c.nb) be_build_bins(b, c);              // (large level table: the histograms also as bin moments, before the first exact densities)
    init_exact(b, c);
    b->rim_auto = 1;                            // (the first count may use the rim groups' tables: its sums are the same either way)
    init_dense(b, c, cb, user);
    k_fin_init<<<1, 1, 0, b->sa>>>(c);
    b->pass_bytes = be_dense_bytes(b, c);       // (decides between ordinary and non-temporal loads for the sweeps' passes)
    // the default keeps the rim groups' memo only where there are rim groups to speak of (dense_memo in vrg_device.hip): counted just now
    if (b->dense_memo < 0 && b->rim_groups * 2 < b->memo_groups) { b->rim_auto = 0; b->pass_bytes = be_dense_bytes(b, c); }
}

void be_events_collect(VrgBackend* b, VrgEvents* ev, long long n_valid) {
    if (!ev) return;
    use_device(b);
    if (b->ev_used) { HIP_CHECK(hipStreamSynchronize(b->sb)); HIP_CHECK(hipStreamSynchronize(b->sa)); }   // the dense stream may trail the band stream by one pass
    for (size_t i = 0; i < b->ev_used; i++) {
        if (b->ev_pool[i].trip < n_valid) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, b->ev_pool[i].a, b->ev_pool[i].b) == hipSuccess) {
                if (b->ev_pool[i].kind == 0) { ev->ms_total += ms; ev->launches++; } else { ev->chain_ms_total += ms; ev->chain_launches += b->ev_pool[i].ntrips; }
            }
            else (void)hipGetLastError();
        }
    }
    b->ev_used = 0; b->ev_trip = 0;
}

void be_recount_hist(VrgBackend* b, const VrgCtx& c, int32_t* rin, int32_t* rout) {
    use_device(b);
    k_recount_hist<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, rin, rout);
    HIP_CHECK(hipStreamSynchronize(b->sa));
}
long long be_slow_flips(VrgBackend* b, const VrgCtx& c) { use_device(b); uint32_t v = 0; HIP_CHECK(hipMemcpyAsync(&v, c.counters + 49, 4, hipMemcpyDeviceToHost, b->sa)); HIP_CHECK(hipStreamSynchronize(b->sa)); return (long long)v; }
long long be_memo_trips(VrgBackend* b) { return b->memo_trips; }
uint32_t be_collect_segmented(VrgBackend* b, const VrgCtx& c, uint64_t* stamps, uint32_t* idxs, uint32_t cap) {
    use_device(b);
    uint64_t* ds = nullptr; uint32_t* di = nullptr; uint32_t* dc = nullptr;
    HIP_CHECK(hipMalloc(&ds, (size_t)(cap + 1) * 8)); HIP_CHECK(hipMalloc(&di, (size_t)(cap + 1) * 4)); HIP_CHECK(hipMalloc(&dc, 4));
    if (!ds || !di || !dc) { if (ds) (void)hipFree(ds); if (di) (void)hipFree(di); if (dc) (void)hipFree(dc); return 0xffffffffu; }
    HIP_CHECK(hipMemsetAsync(dc, 0, 4, b->sa));
    k_collect_seg<<<voxel_blocks(c), TPB, 0, b->sa>>>(c, ds, di, cap, dc);
    uint32_t n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, dc, 4, hipMemcpyDeviceToHost, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    uint32_t m = std::min(n, cap);
    HIP_CHECK(hipMemcpy(stamps, ds, (size_t)m * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(idxs, di, (size_t)m * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipFree(ds)); HIP_CHECK(hipFree(di)); HIP_CHECK(hipFree(dc));
    return n;
}
