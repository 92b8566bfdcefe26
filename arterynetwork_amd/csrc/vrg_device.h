// vrg_device.h - the product backend: HIP kernels for MI355X (gfx950, wave64).  Private to the backend: what its files share.
//
// One while-loop trip of variationalRegionGrowing.py:58-117 (be_sweep_once) is k_band + update() on stream A, plus the dense
// pass on stream B.  update() (:156-259) comes in three kinds, all running the item functions of vrg_items.h on the same data:
//   k_band  (many workgroups, one thread - or 16 / 8 / 4 lanes - per band-pool slot): adds the density corrections of the
//           sweep before (:236-247) to the surviving entries, decides every entry (:79-88) and appends the flips to an
//           unordered list; extra workgroups compute the exact densities (:252-255) of the entries the sweep before added
//           and decide those; behind a fused sweep 32 more write its label bytes, class bits and free list.
//   FUSED   k_sweep: ONE launch, one flip per workgroup, for sweeps with at most 128 flips (65 on a large level table) -
//           every workgroup ranks the flips and resolves the skip rule itself; nothing is applied inside the sweep
//           (-> k_memo on large bands).  A sweep with more flips hands itself back untouched (VBAIL_FUSE).
//   CHAIN   k_order (-> k_rank_wide -> k_list_wide -> k_prepass_wide -> k_fix_wide above 512 flips) -> k_mark_relabel<1> (up to 256 flips) or
//           k_mark_compact (a flip per half-wave) -> k_mark_relabel<4> over the flips it left -> k_close: up to 65 536 flips without a host
//           synchronisation; the relabel kernels' workgroups reserve their stretches of the sweep's lists through VrgCtx::rsv (cache lines of their
//           own: same-address atomics execute one after the other).  A sweep with more flips (or one that needs larger arrays) is handed back
//           untouched (VrgState::bail) and
//   HOST-DRIVEN (be_sweep_once with VRG_SWEEP_SYNC): the host reads the flip count - above 65 536 flips a radix sort ranks them and the chain's
//           chip-wide kernels do the rest; the full-stencil check variant (and a lowered "small_flips") runs the item functions as device-wide kernels.
//   stream B, the dense pass (enqueued behind the kernel that raises its request: k_close, or the k_band after a fused sweep):
//     k_recount_pipe / k_recount_bits : the dense kernel (every listed 1024-voxel unit, HBM-bound, read-only: 4 B intensity - or a 2-B
//        level index - of included voxels + 2 class bits per voxel): region sizes and intensity sums (:113-116, :249-250), one slot per
//        workgroup, added up in slot order by the next kernel on the stream (the next sweep's k_gate, or k_dense_close where the host looks
//        first; option dense_close = 0 and the passes without a gate: by the pass's last workgroup), checked against the sizes the band side keeps by increments.  k_recount_pipe (fp32 storage) walks the list two
//        trips deep; 16-bit storage stays one trip deep in k_recount_bits (two deep measured slower: profiles/depth16_ab_880.json) and, on
//        large volumes (option dense_memo), takes the intensity sum of a 256-voxel group whose voxels are all outer from a table built
//        once per volume (VrgBackend::gsum) instead of fetching the group.  With the rim groups' tables (dense_memo = 2: isum, icnt) the
//        walk decides per trip of three units - no inner voxel, as many outer voxels per unit as init counted included ones (vrg_rim.h) -
//        and a trip that passes takes all twelve sums from isum: two trips per turn of a loop that fetches entries, class words, sums
//        and counts with vector loads a turn ahead; any other trip goes group by group (rim_groups) as before
//     -> on several GPUs: slab all-reduce -> k_dense_fin (the same check on the totals, trace sums).
//   Stream A does not join: it runs up to two sweeps ahead of the dense pass (two copies of the class bits).
// Labels are updated IN PLACE: measured on MI355X, streaming I + labels read-only runs at 5.8-6.0 TB/s
// while the same stream with a 1 B/voxel label write-back drops to 4.8 TB/s, so unchanged labels are
// never rewritten.  (The full-stencil check variant relabels every voxel through lab[1].)
// Every kernel starts by reading the device-resident VrgState and returns at once when the stop
// flag is set, so the host can enqueue batches of sweeps without synchronising.
// All state of the backend (device, streams, events, communicator, first error) lives in VrgBackend: one per handle.
//
// The backend's translation units (each launches only the kernels it defines; they meet in the host functions declared at the end):
//   vrg_chain.hip   the band chain (k_band, k_order and the *_wide kernels, k_mark_relabel / k_mark_compact, k_close, the fused sweep,
//                   the item kernels of host-driven trips) and the host side of a trip (be_sweep_once)
//   vrg_device.hip  the dense pass (k_gate, k_recount_pipe / k_recount_bits, the unit list, the slab close and all-reduce)
//   vrg_init.hip    the backend object, init and the volume (packing of caller arrays, level tables, bins, histograms)
//   vrg_follow.hip  leader / follower replication: the follower's side, the RCCL communicator and the transports
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include <rccl/rccl.h>

#include "vrg_backend.h"
#include "vrg_items.h"

struct EvPair { hipEvent_t a, b; long long trip; int kind; int ntrips; };   // kind 0: a dense launch, 1: the band chain of ntrips trips (the last of them: trip)

struct VrgBackend {
    int device = 0;
    hipStream_t sa = nullptr;            // stream A: the band kernels of every trip in program order, copies
    hipStream_t sb = nullptr;            // stream B: the dense pass (recount, slab all-reduce, k_dense_fin); trails stream A by up to one sweep
    hipStream_t sc = nullptr;            // stream C: the change log's transport (leader / follower replication: RCCL broadcasts), created on first use
    int repl = 0;                        // this handle is a rank of a leader / follower group: the communicator carries the log, not slab sums
    hipStream_t sd = nullptr;            // stream D: a follower's label bytes and stamps (beside its dense passes, which read the class bits only)
    hipEvent_t mark[4] = {nullptr, nullptr, nullptr, nullptr};   // a follower's staging buffers: the kernels that read buffer j have been enqueued up to here (per stream)
    int sweep_blocks = 0;                // 0 = auto (dense_blocks)
    int prio_mode = 2;                   // the dense stream gets the higher priority (measured: -1..2 % step time)
    uint32_t small_flips = 65536;        // flips per sweep the device-resident four-launch chain takes on (option "small_flips", at most NF_WIDE); a sweep with more is driven from the host
    ncclComm_t comm = nullptr;           // per-sweep all-reduce of the slab statistics (multi-GPU)
    char err[256] = "";                  // first HIP / RCCL failure; the engine turns it into VRG_E_INTERNAL
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    long long ev_trip = 0;               // trips enqueued since the last be_events_collect
    void* tmp = nullptr; size_t tmp_bytes = 0;        // scratch of the host-driven sorts
    uint64_t* keys2 = nullptr; size_t keys2_n = 0;
    int dense_pending = 0;                            // Z-slabs: recounts enqueued since the last staged all-reduce
    int serial = 0;                                   // option "serial_streams": see be_sweep_once
    int skip = 1;                                     // option "skip_excluded": the dense pass does not fetch the intensities of excluded voxels
    int nt_loads = -1;                                // option "nt_loads": -1 = by the size of the pass, 0 / 1 = ordinary / non-temporal loads
    int verify_every = 1;                             // option "verify_every": the dense pass on every n-th sweep only (0: never)
    int dense_pipe = 1;                               // option "dense_pipe": fp32 storage + skip_excluded run the two-trips-deep recount (k_recount_pipe)
    int dense_close = 1;                              // option "dense_close": a gated pass is closed by the next kernel on the dense stream (0: by its own last workgroup, ticket and all)
    bool dense_open = false; int open_fin = 2;        // ... such a pass has been enqueued with no k_dense_close behind it (dense_close_open) ...
    VrgCtx open_c;                                    // ... and the context / kind of close that kernel is launched with
    int dense_memo = -1;                              // option "dense_memo": 16-bit storage + skip_excluded take the sums of all-outer 256-voxel groups from gsum (-1: large volumes only, 1: always, 0: never; 2: the rim groups' sums too, from isum / icnt)
    double* gsum = nullptr; size_t gsum_bytes = 0;    // sum of the values of every 256-voxel group of the padded volume (k_build_gsum), built with the level indices ...
    const uint16_t* gsum_for = nullptr;               // ... at this address (be_build_lev16); freed with them (be_free) or with the backend
    long long memo_groups = 0;                        // full groups be_dense_bytes counted last (stats: dense_memo_groups)
    double* isum = nullptr; size_t rim_bytes = 0;     // dense_memo = 2: per 256-voxel group the sum of the values of its voxels included at init (f64) and, behind the sums, their
    const uint16_t* rim_for = nullptr;                // number (u16) - one allocation, built behind the class bits at every init (build_rim) for the level indices at this address; freed with them
    int rim_auto = 1;                                 // the default (dense_memo = -1) takes the rim groups' memo: decided by what init finds (be_init_finish)
    long long rim_groups = 0;                         // memoised groups of fewer than 256 voxels be_dense_bytes counted last (stats: dense_rim_groups)
    uint64_t pass_bytes = 0;                          // bytes a dense pass fetches, counted at the end of init (0: not known yet)
    uint32_t memo_above = 32768;                      // option "memo_above": band entries above which a fused trip keeps the per-level memo (k_memo)
    long long memo_trips = 0;                         // fused trips that did
    bool fused_memo = false;                          // ... and it kept the per-level memo (k_memo)
    bool fused_prev = false;                          // the trip enqueued last was a fused one: the dense pass of the sweep it applied is not enqueued yet
                                                      // (its request comes from THIS trip's k_band; if that trip stopped or handed itself back, the stop word makes the gate leave)
    bool prev_open = false;                           // ... and its sweep was open-ended: this trip's k_band derives the closed state (and lists the touched levels itself)
    int open_par = 0;                                 // ... the set of per-level counters it filled
    long long follow_counts = 0;                      // a follower's dense passes so far (which of them are timed: option "events")
    uint32_t band_blocks_max = 2048;                  // option "band_blocks_max": most workgroups k_band uses for the pool (BAND_BLOCKS)
    uint64_t* rsv = nullptr;                          // VrgCtx::rsv of this handle's four-launch trips (64 words, zero between sweeps)
    int mark_compact = 1;                             // option "mark_compact": four-launch trips of thousands of flips relabel with k_mark_compact (+ k_mark_relabel for what it leaves)
    int open_sweeps = 1;                              // option "open_sweeps": fused sweeps inside a batch end at their commit, without a closing workgroup
    int iter_hint = 0;                                // sweeps applied when the engine last read the state + trips enqueued since
    uint32_t band_hint = 0;                           // pool slots in use when the engine last read the state (0: unknown)
    void* xfer[2] = {nullptr, nullptr}; size_t xfer_bytes = 0;      // two page-locked buffers for host arrays on their way in / out
    uint32_t flip_hint_min = 0;                       // (a trip came back with this many flips: the launches are sized for at least that until the engine reads a state again)
    uint32_t flip_hint = 0;                           // ... and the flips of the sweep applied last (sizes the chip-wide launches of a four-launch trip)
    int direct_hint = 1;                              // ... and whether corrections are then evaluated entry by entry (8 lanes per slot)
};

#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess && !b->err[0]) { \
    std::snprintf(b->err, sizeof(b->err), "HIP error '%s' in %s (%s:%d)", hipGetErrorString(e_), #x, __FILE__, __LINE__); \
    std::fprintf(stderr, "%s\n", b->err); } } while (0)

namespace {

constexpr int TPB = 256;            // 4 waves of 64
constexpr int ITEM_BLOCKS = 256;    // item kernels: 64 Ki threads, grid-stride
constexpr int EXACT_BLOCKS = 512;   // k_band: workgroups for the exact densities (one pending slot per workgroup at a time)
constexpr int SWEEP_BLOCKS = 256;   // 1 workgroup (4 waves) per CU, each wave with 3 KiB of labels + 12 KiB of intensities in
                                    // flight: measured best for the HBM-bound recount while stream B's band kernels run beside
                                    // it (880x880x640: 256 -> 0.38 ms, 192/384 -> 0.42-0.43, 320 -> 0.49, 512 -> 0.40, 1024 -> 0.44)
constexpr uint32_t NF_SMALL = 4096; // flips one workgroup sorts in LDS
constexpr uint32_t NF_WIDE = 65536; // flips the device-resident chain can take (option small_flips); more: host-driven trips
constexpr uint32_t NF_ORDER = 512;  // ... above this many the ordering step runs chip-wide (k_rank_wide, k_prepass_wide, k_fix_wide) instead of in k_order's one workgroup (86 us at 1600 flips)
constexpr uint32_t NZ_LDS = 1024;   // touched levels k_band keeps in LDS
constexpr int KS_THREADS = 1024;    // k_fix (host-driven trips): one big workgroup
constexpr int KC_THREADS = 256;     // k_close: one wave per SIMD, so that its workgroups fit on a CU beside the three recount waves
                                    // per SIMD (16-wave workgroups had to wait for the recount to end: 0.1 ms per sweep)

// ---- wave / block primitives (wave = 64 lanes) -------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // fixed butterfly: deterministic
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { uint32_t t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    return v;
}
// exclusive scan of one value per thread over a 256-thread block; returns the block total in `total`
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t& total, uint32_t* sh /*4+*/) {
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < w; i++) base += sh[i];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + inc - v;
}


// in-kernel time stamps of the band chain (diagnostic build -DVRG_STAMPS only; in the product build no stamp executes)
#if defined(VRG_STAMPS)
#define VRG_STAMP(c, k) do { c.dbg[k] = wall_clock64(); } while (0)
#define VRG_STAMP_NOW() wall_clock64()
#define VRG_STAMP_PUT(c, k, v) do { c.dbg[k] = (v); } while (0)
#define VRG_STAMP_MAX(c, k) do { atomicMax(&c.dbg[k], (unsigned long long)wall_clock64()); } while (0)   // the last workgroup's exit
// per-workgroup stamps (thread 0 of every workgroup; word k of the workgroup's VRG_DBG_PER)
#define VRG_STAMP_WG(c, k) do { if (threadIdx.x == 0 && blockIdx.x < (uint32_t)VRG_DBG_WG && (k) < (uint32_t)VRG_DBG_PER) c.dbg[64 + blockIdx.x * VRG_DBG_PER + (k)] = wall_clock64(); } while (0)
#define VRG_STAMP_WG_PUT(c, k, v) do { if (threadIdx.x == 0 && blockIdx.x < (uint32_t)VRG_DBG_WG) c.dbg[64 + blockIdx.x * VRG_DBG_PER + (k)] = (v); } while (0)
#else
#define VRG_STAMP_WG(c, k) do { } while (0)
#define VRG_STAMP_WG_PUT(c, k, v) do { (void)(v); } while (0)
#define VRG_STAMP(c, k) do { } while (0)
#define VRG_STAMP_NOW() 0ull
#define VRG_STAMP_PUT(c, k, v) do { (void)(v); } while (0)
#define VRG_STAMP_MAX(c, k) do { } while (0)
#endif
// random delays at the entry of every concurrent kernel and in front of every hand-off (diagnostic build -DVRG_CHAOS only,
// tools/build_chaos.sh; in the product build nothing executes): one wave in four sleeps for up to ~110 us, so workgroups,
// kernels and the two streams meet in orders a quiet machine never produces - the results must not change
// (tools/gpu.sh <tag> chaos)
#if defined(VRG_CHAOS)
__device__ __forceinline__ void vrg_chaos_delay(uint32_t salt) {
    uint32_t h = ((uint32_t)wall_clock64() * 2654435761u) ^ (blockIdx.x * 40503u + (threadIdx.x >> 6) * 9973u + salt * 7919u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    h = (uint32_t)__builtin_amdgcn_readfirstlane((int)h);
    if ((h & 3u) == 0u) { const uint32_t n = (h >> 2) & 63u; for (uint32_t i = 0; i < n; i++) __builtin_amdgcn_s_sleep(64); }
}
#define VRG_CHAOS_POINT(salt) vrg_chaos_delay(salt)
#else
#define VRG_CHAOS_POINT(salt) do { } while (0)
#endif
#define ITEM_LOOP(n) for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n_ = (n); i < n_; i += gridDim.x * blockDim.x)
// same with a 64-bit item index: (listed flips) x (positions) can exceed 2^32 on adversarial volumes
#define ITEM_LOOP64(n) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n_ = (n); i < n_; i += (uint64_t)gridDim.x * blockDim.x)
constexpr unsigned long long SPIN_LIMIT = 300000000ull;    // bounded spins (wait_dense_read_for, gate_dense_due): wall_clock64 ticks (100 MHz): 3 s
constexpr int BAND_BLOCKS = 2048;     // most workgroups k_band uses for the pool (above 2048 x 256 slots a thread takes several turns: every workgroup files its flips with one bump of the
                                      // flip counter, and those bumps run one after the other); fewer when the engine knows the pool is small (band_blocks())

// The unit list from the bitmap, by one workgroup of 1024 threads (a few microseconds): thread t counts the set bits of
// its stretch of bitmap words, a block scan gives its place, it writes its units.  Bitmap words are read past L1 / a
// stale L2 line (sc1): band kernels of the other stream set bits with device-scope atomics.
constexpr int GATE_THREADS = 1024;
// (p = parity of the pass being prepared: the units its sweep listed for the first time are merged into the bitmap first -
// VrgCtx::unew; the sweep's labels are in place, and no other sweep of that parity can be writing)
__device__ void ulist_refresh(const VrgCtx& c, bool force, int p) {
    __shared__ uint32_t s_part[GATE_THREADS / 64];
    __shared__ uint32_t s_gen;
    const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) s_gen = vrg_load_u32(&c.uctl[UC_GEN + p * UC_GEN_STRIDE]);
    __syncthreads();
    if (!force && s_gen == 0u) return;                         // (uniform)
    const uint32_t plane = (uint32_t)c.PY * (uint32_t)c.PX, lo = (2u + (uint32_t)c.z0) * plane, hi = (2u + (uint32_t)c.z1) * plane;
    uint32_t f_lo = (uint32_t)(((uint64_t)lo + 1023u) >> 10), f_hi = hi >> 10;
    if (f_hi < f_lo) f_hi = f_lo;
    const uint32_t w0 = f_lo >> 5, w1 = (f_hi + 31u) >> 5, nwords = w1 - w0;
    const uint32_t per = (nwords + GATE_THREADS - 1) / GATE_THREADS;
    const uint32_t a = w0 + t * per, b = min(a + per, w1);
    for (uint32_t wi = a; wi < b; wi++) {                      // merge this sweep's new units (whole words; the slab's range is cut out below)
        const uint32_t nw = vrg_load_u32(&c.unew[p][wi]);
        if (nw) { c.ubits[wi] = c.ubits[wi] | nw; c.unew[p][wi] = 0u; }
    }
    auto word = [&](uint32_t wi) -> uint32_t {
        uint32_t bits = c.ubits[wi];
        const uint32_t u0 = wi << 5;
        if (u0 < f_lo) bits &= 0xffffffffu << (f_lo - u0);
        if (f_hi - u0 < 32u) bits &= (1u << (f_hi - u0)) - 1u;
        return bits;
    };
    uint32_t cnt = 0;
    for (uint32_t wi = a; wi < b; wi++) cnt += __popc(word(wi));
    const uint32_t incl = wave_incl_scan(cnt);
    if (lane == 63) s_part[wv] = incl;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (int k = 0; k < GATE_THREADS / 64; k++) { if (k < (int)wv) base += s_part[k]; total += s_part[k]; }
    uint32_t q = base + incl - cnt;
    for (uint32_t wi = a; wi < b; wi++) {
        uint32_t bits = word(wi);
        while (bits) { c.ulist[q++] = (wi << 5) + vrg_ctz(bits); bits &= bits - 1u; }
    }
    if (t == 0) { c.uctl[UC_N] = total; c.uctl[UC_GEN + p * UC_GEN_STRIDE] = 0u; }
}

}  // namespace

// ---- host functions the backend's files share (hidden: not part of the library's interface) ---------------------------------------
#pragma GCC visibility push(hidden)
void use_device(VrgBackend* b);                                                                          // vrg_init.hip
void init_exact(VrgBackend* b, const VrgCtx& c);                                                         // vrg_chain.hip
void init_dense(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user);                            // vrg_device.hip
void dense_close_open(VrgBackend* b);                                                                    // vrg_device.hip
void build_rim(VrgBackend* b, const VrgCtx& c);                                                          // vrg_init.hip
void enqueue_dense(VrgBackend* b, const VrgCtx& c, hipEvent_t e_start, hipEvent_t e_stop, be_reduce_fn cb, void* user);   // vrg_device.hip
#pragma GCC visibility pop
