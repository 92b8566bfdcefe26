// vrg_device.hip - the dense pass of the product backend (vrg_device.h: the overview): k_gate, the recount (k_recount_pipe /
// k_recount_bits), the class bits and the unit list, the slab close and all-reduce, and their host side - launch sizing included.
// The dense stream runs k_gate -> pass -> k_gate -> pass ...: a pass behind a gate ends with its workgroups' slots stored (plain stores,
// dctl[VD_OPEN] = their number) and the NEXT kernel on the stream - the kernel boundary makes the slots visible - adds them up in the fixed
// slot order and closes the pass: the next gate, first thing and before it waits for its own request, or k_dense_close wherever the host
// looks before another gate runs (dense_close_open: be_sync, the staged all-reduce, verify-last, the byte count, serial_streams).  The
// passes without a gate (init, verify-last, a follower's count) and option dense_close = 0 close in the pass's last workgroup, by ticket.
#include "vrg_device.h"
#include "vrg_rim.h"

namespace {

// dense side, in front of every recount: a sweep has been applied since the last recount - or the run has stopped and
// there is nothing to count.  True at once whenever the dense pass is what bounds the step (the band side runs a sweep
// ahead).  A kernel of its own (one thread), not the first thing in the recount: the recount's duration - what the HIP
// events and rocprofv3 report for the roofline - must be streaming time only, and workgroups that wait while holding
// LDS (the 16-bit variant: 64 KiB each) could leave no CU for k_close, which produces what they wait for.
// rseq: the recounts done (only this stream changes the word); req, stop: the caller's first look at the two gate words, fetched with
// everything else the gate reads first - the wait looks again only while the request is really missing.
__device__ __forceinline__ bool gate_dense_due(const VrgCtx& c, int64_t rseq, int64_t req, int64_t stop) {
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        if (req > rseq) return true;
        if (stop) return vrg_load_i64(&c.gate[VG_REQ]) > rseq;   // (the last applied sweep's request is older than the stop flag)
        __builtin_amdgcn_s_sleep(4);                          // (~0.1 us per look: one thread polls, two words of one cache line)
        if (wall_clock64() - t0 > SPIN_LIMIT) { c.dctl[VD_ERR] = 10; return false; }
        req = vrg_load_i64(&c.gate[VG_REQ]); stop = vrg_load_i64(&c.gate[VG_STOP]);
    }
}

// ---- the dense pass ----------------------------------------------------------------------------------
// Region recount (:113-116 innerSize/outerSize, :249-250 dataArray[mask]) over every voxel, every sweep.
// Streams the interior planes of the padded volume in units of 1024 voxels (k_recount_bits below).  Sums are
// reduced lane -> wave butterfly -> LDS -> one slot per workgroup, added in fixed slot order by the last workgroup
// to finish: bit-reproducible.
typedef float f4v __attribute__((ext_vector_type(4)));
typedef double d2v __attribute__((ext_vector_type(2)));
typedef uint32_t u2v __attribute__((ext_vector_type(2)));

struct SweepAcc { long long nin, nout; double sin_, sout; };

// per-workgroup slot, then the LAST workgroup to arrive adds all slots in slot order and publishes the totals.
// Hand-off without fences (cdna guide, Guideline 16 / "Valid forms", first row of the measured table): one lane stores its
// workgroup's four values write-through (sc1), drains them (vmcnt(0)), takes a ticket with an agent-scope atomic add;
// the workgroup whose add came last reads every slot with sc1 loads behind a workgroup barrier.  (An agent-scope release
// + acquire pair costs ~1.7 us each - a tenth of a slab's recount.)
__device__ __forceinline__ void st_sc1(long long* p, long long v) { __hip_atomic_store(p, v, VRG_MO_STORE, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(double* p, double v) { __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), VRG_MO_STORE, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long ld_sc1(const long long* p) { return __hip_atomic_load(p, VRG_MO_LOAD, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_sc1(const double* p) { return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), VRG_MO_LOAD, __HIP_MEMORY_SCOPE_AGENT)); }
// The sum over the slots of a pass of `n` workgroups, by the first TPB threads of the calling workgroup (every thread of it calls): thread t adds
// slots t, t + TPB, ..., then the wave butterfly, then the four wave values left to right - one fixed order whoever runs it (the pass's last
// workgroup, the next gate, k_dense_close).  stg: the first `staged` slots as the caller has fetched them into LDS already (the gate: with
// everything else it reads first), the four arrays one behind the other; the other slots are loaded here.  The totals are valid in thread 0.
__device__ __forceinline__ VrgDense slots_total(const VrgCtx& c, uint32_t n, long long (*sh_n)[4], double (*sh_s)[4], uint32_t staged = 0, const long long* stg = nullptr) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long x = 0, y = 0; double sx = 0, sy = 0;
    if (threadIdx.x < TPB) {
        for (uint32_t i = threadIdx.x; i < n; i += TPB) {
            if (i < staged) {
                x += stg[i]; y += stg[staged + i];
                sx += __builtin_bit_cast(double, stg[2 * staged + i]); sy += __builtin_bit_cast(double, stg[3 * staged + i]);
            } else {
                x += ld_sc1((const long long*)&c.st_nin[i]); y += ld_sc1((const long long*)&c.st_nout[i]); sx += ld_sc1(&c.st_sin[i]); sy += ld_sc1(&c.st_sout[i]);
            }
        }
    }
    x = wave_sum(x); y = wave_sum(y); sx = wave_sum(sx); sy = wave_sum(sy);
    __syncthreads();
    if (lane == 0 && wv < 4) { sh_n[0][wv] = x; sh_n[1][wv] = y; sh_s[0][wv] = sx; sh_s[1][wv] = sy; }
    __syncthreads();
    VrgDense d;
    d.n_in = (double)(sh_n[0][0] + sh_n[0][1] + sh_n[0][2] + sh_n[0][3]);
    d.n_out = (double)(sh_n[1][0] + sh_n[1][1] + sh_n[1][2] + sh_n[1][3]);
    d.sum_in = ((sh_s[0][0] + sh_s[0][1]) + sh_s[0][2]) + sh_s[0][3];
    d.sum_out = ((sh_s[1][0] + sh_s[1][1]) + sh_s[1][2]) + sh_s[1][3];
    return d;
}
// ONE thread closes the recount of a sweep with this device's slab sums `d` (fin 2: one GPU, the pass is closed with it; 1: Z-slabs, the
// staged all-reduce closes it).
// (expect: the two sizes the pass has to reproduce, where the caller has fetched them from exp_ring already)
__device__ __forceinline__ void recount_close(const VrgCtx& c, const VrgDense& d, int fin, const int64_t* expect = nullptr) {
    vrg_recount_done(c, d);                          // this device's slab sums of the recount
    if (fin == 2) vrg_dense_fin_one(c, d, expect);   // nothing to sum over ranks: close the pass here
}
// ... for a pass that left its slots open, by ONE thread of the next kernel on the dense stream: the same close, nothing open any more, and
// the pass counters written through and drained - the caller may go on running (a gate waits for its own request next) while the band
// side waits for VD_RSEQ.  (The counter tells the band side one thing only: the pass has read its class copy - it ended a kernel ago.  What
// the close files beside it - the ring entry, the trace record - is read by later kernels of this stream and by the host behind a
// synchronisation: plain stores.)
__device__ __forceinline__ void close_publish(const VrgCtx& c, const VrgDense& d, int fin, const int64_t* expect = nullptr) {
    recount_close(c, d, fin, expect);
    c.dctl[VD_OPEN] = 0;
    const int64_t rseq = c.dctl[VD_RSEQ], seq = c.dctl[VD_SEQ];
    vrg_store_i64(&c.dctl[VD_RSEQ], rseq); vrg_store_i64(&c.dctl[VD_SEQ], seq);
    vrg_drain();
}
// defer (option dense_close, the passes behind a gate): the workgroup leaves its slot with plain stores and the kernel ends - no drain, no
// ticket, no closing workgroup.  The kernel boundary behind the pass makes the slots visible, and the next kernel on the dense stream sums
// them (close_publish): the gate of the next pass, or k_dense_close where the host is about to look.  dctl[VD_OPEN] = the number of slots.
__device__ __forceinline__ void sweep_finish(const VrgCtx& c, SweepAcc a, int fin, bool defer = false) {
    __shared__ long long sh_n[2][4];
    __shared__ double sh_s[2][4];
    __shared__ int is_last;
    a.nin = wave_sum(a.nin); a.nout = wave_sum(a.nout); a.sin_ = wave_sum(a.sin_); a.sout = wave_sum(a.sout);
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sh_n[0][wv] = a.nin; sh_n[1][wv] = a.nout; sh_s[0][wv] = a.sin_; sh_s[1][wv] = a.sout; }
    __syncthreads();
    if (defer) {
        if (threadIdx.x == 0) {
            c.st_nin[blockIdx.x] = sh_n[0][0] + sh_n[0][1] + sh_n[0][2] + sh_n[0][3];
            c.st_nout[blockIdx.x] = sh_n[1][0] + sh_n[1][1] + sh_n[1][2] + sh_n[1][3];
            c.st_sin[blockIdx.x] = ((sh_s[0][0] + sh_s[0][1]) + sh_s[0][2]) + sh_s[0][3];
            c.st_sout[blockIdx.x] = ((sh_s[1][0] + sh_s[1][1]) + sh_s[1][2]) + sh_s[1][3];
            if (blockIdx.x == 0) c.dctl[VD_OPEN] = (int64_t)gridDim.x;
        }
        return;
    }
    if (threadIdx.x == 0) {
        st_sc1((long long*)&c.st_nin[blockIdx.x], sh_n[0][0] + sh_n[0][1] + sh_n[0][2] + sh_n[0][3]);
        st_sc1((long long*)&c.st_nout[blockIdx.x], sh_n[1][0] + sh_n[1][1] + sh_n[1][2] + sh_n[1][3]);
        st_sc1(&c.st_sin[blockIdx.x], ((sh_s[0][0] + sh_s[0][1]) + sh_s[0][2]) + sh_s[0][3]);
        st_sc1(&c.st_sout[blockIdx.x], ((sh_s[1][0] + sh_s[1][1]) + sh_s[1][2]) + sh_s[1][3]);
        vrg_drain();
        VRG_CHAOS_POINT(13);
        uint32_t t = __hip_atomic_fetch_add(&c.counters[0], 1u, VRG_MO_TICKET, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (t == gridDim.x - 1);
        if (is_last) c.counters[0] = 0;              // every workgroup has arrived: reset for the next launch
    }
    __syncthreads();
    if (!is_last) return;
    const VrgDense d = slots_total(c, gridDim.x, sh_n, sh_s);
    if (threadIdx.x == 0) {
        if (fin == 0) { *c.dn_part = d; if (c.world == 1) *c.dn = d; }   // init: the sizes found the incremental counts
        else if (fin == 4) vrg_follow_check(c, d, (uint32_t)c.fexp[0], c.fexp[1], c.fexp[2]);   // a follower's count of the sweep its apply step announced
        else recount_close(c, d, fin);
    }
}

constexpr uint32_t LEV16_MAX = 16384;   // 16-bit storage: the level values sit in LDS (<= 16384 x f32)

// The recount needs two facts per voxel - inner / outer - so it streams the
// 2-bit class volume (VrgCtx::clsb, 0.25 B/voxel) instead of the label bytes: 4.25 B (fp32 storage), 2.25 B
// (16-bit storage) or 8.25 B (float64 storage) per voxel.  Units are 1024-voxel aligned in the absolute voxel
// index; lane l owns class dword l of a unit and the 4 x 4 intensities at 256*j + 4*l, i.e. one 256-B + four 1-KiB
// (or 512-B / 2-KiB) requests per wave and unit.  A slab edge that cuts a unit is handled by masking (first / last
// wave); padding planes are class 0.
// UNITS = units a wave loads per trip (bytes in flight); NT = non-temporal loads: the volume is read once per
// sweep and is far larger than the 256-MiB Infinity Cache, so nothing is worth keeping.
// MODE 0: fp32 intensities, 1: 16-bit level indices + LDS value table (floats), 2: float64 intensities, 3: as 1 with the table
// held as doubles (up to TAB64_LEVELS levels): the pass is then bound by its arithmetic, not by memory - SQ counters, 16-bit
// storage at 880x880x640: VALU busy 0.6-0.8 of all issue slots, a quarter of it the float -> double conversion of every value
// (half rate on this chip) - and the doubles come out of the table ready to be added.
// Dense pass number seq (= passes closed + 1) reads copy seq & 1 of the class bits.
template <int MODE> struct UnitVals { f4v f[4]; };
template <> struct UnitVals<1> { u2v q[4]; };           // raw level indices: the LDS look-ups wait until the sums are formed
template <> struct UnitVals<3> { u2v q[4]; };
constexpr uint32_t TAB64_LEVELS = 4096;                 // 32 KiB of LDS per workgroup
template <int MODE> __device__ __forceinline__ void lookup4(const UnitVals<MODE>& u, int j, const float* s_val, float lv[4], double dv[4]) {
    if constexpr (MODE == 1) {
        lv[0] = s_val[u.q[j].x & 0xffffu]; lv[1] = s_val[u.q[j].x >> 16];
        lv[2] = s_val[u.q[j].y & 0xffffu]; lv[3] = s_val[u.q[j].y >> 16];
    } else if constexpr (MODE == 3) {
        const double* s_dv = reinterpret_cast<const double*>(s_val);
        dv[0] = s_dv[u.q[j].x & 0xffffu]; dv[1] = s_dv[u.q[j].x >> 16];
        dv[2] = s_dv[u.q[j].y & 0xffffu]; dv[3] = s_dv[u.q[j].y >> 16];
    }
}
template <> struct UnitVals<2> { d2v f[4][2]; };
template <int MODE>
__device__ __forceinline__ void stats_group(SweepAcc& a, uint32_t wj, const UnitVals<MODE>& u, int j, const float* s_val) {
    float lv[4]; double dv[4];
    lookup4<MODE>(u, j, s_val, lv, dv);
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
        if constexpr (MODE == 2 || MODE == 3) {
            const uint32_t t = wj >> (2 * bb);
            double x;
            if constexpr (MODE == 2) x = u.f[j][bb >> 1][bb & 1]; else x = dv[bb];
            a.sin_ += (t & 1u) ? x : 0.0;
            a.sout += (t & 2u) ? x : 0.0;
        } else {
            // class bit -> all-ones / all-zeros mask over the float's bits: a masked-out voxel adds +0.0
            uint32_t xi;
            if constexpr (MODE == 1) xi = __float_as_uint(lv[bb]); else xi = __float_as_uint(u.f[j][bb]);
            const uint32_t m_in = (uint32_t)((int32_t)(wj << (31 - 2 * bb)) >> 31);
            const uint32_t m_out = (uint32_t)((int32_t)(wj << (30 - 2 * bb)) >> 31);
            a.sin_ += (double)__uint_as_float(xi & m_in);
            a.sout += (double)__uint_as_float(xi & m_out);
        }
    }
}
// the same for a group in which no lane holds an inner voxel: only the outer sum moves (same additions, same order)
template <int MODE>
__device__ __forceinline__ void stats_group_outer(SweepAcc& a, uint32_t wj, const UnitVals<MODE>& u, int j, const float* s_val) {
    float lv[4]; double dv[4];
    lookup4<MODE>(u, j, s_val, lv, dv);
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
        if constexpr (MODE == 2 || MODE == 3) {
            double x;
            if constexpr (MODE == 2) x = u.f[j][bb >> 1][bb & 1]; else x = dv[bb];
            a.sout += ((wj >> (2 * bb)) & 2u) ? x : 0.0;
        } else {
            uint32_t xi;
            if constexpr (MODE == 1) xi = __float_as_uint(lv[bb]); else xi = __float_as_uint(u.f[j][bb]);
            const uint32_t m_out = (uint32_t)((int32_t)(wj << (30 - 2 * bb)) >> 31);
            a.sout += (double)__uint_as_float(xi & m_out);
        }
    }
}
// ... and for the table of doubles with one entry more, s_dv[lz] = +0.0 (the memoising pass, MODE 3): the INDEX is selected before the
// look-up - a voxel that is not outer reads entry lz - instead of the 64-bit value after it: one v_cndmask_b32 per voxel instead of
// two; the same +0.0 is added in the same place, so the sums are bit-identical.  (Measured at 880x880x640, three rounds in turn,
// 1024 workgroups: dense 0.1076-0.1079 -> 0.1027-0.1029 ms; profiles/dense_memo_ab_880.json.)
__device__ __forceinline__ void stats_group_outer_idx(SweepAcc& a, uint32_t wj, const UnitVals<3>& u, int j, const float* s_val, uint32_t lz) {
    const double* s_dv = reinterpret_cast<const double*>(s_val);
    a.sout += s_dv[(wj & 2u) ? (u.q[j].x & 0xffffu) : lz];
    a.sout += s_dv[(wj & 8u) ? (u.q[j].x >> 16) : lz];
    a.sout += s_dv[(wj & 32u) ? (u.q[j].y & 0xffffu) : lz];
    a.sout += s_dv[(wj & 128u) ? (u.q[j].y >> 16) : lz];
}
// SKIP: a group of four voxels per lane whose 256 voxels are all excluded costs the wave nothing (the branch is
// wave-uniform there); partly excluded groups run with the excluded lanes masked off.  Adding +0.0 or not adding at
// all gives the same sums (the accumulators never hold -0.0: they start at +0.0).
template <int MODE>
__device__ __forceinline__ double unit_value(const UnitVals<MODE>& u, int j, int bb, const float* lv, const double* dv) {
    if constexpr (MODE == 2) return u.f[j][bb >> 1][bb & 1];
    else if constexpr (MODE == 3) return dv[bb];
    else if constexpr (MODE == 1) return (double)lv[bb];
    else return (double)u.f[j][bb];
}
// Most groups inside the brain mask hold four outer voxels (class byte 0xAA): when every lane that takes part has
// such a group, the four values go straight into the outer sum - the same additions in the same order as the general
// path makes (which also adds +0.0 to the inner sum four times: no change).
// MEMO (option dense_memo, 16-bit storage): a group whose 256 voxels are all outer - class byte 0xAA in every lane, bit j of the
// wave-uniform mask fm - adds the sum of its values, built once per volume (k_build_gsum, vrg_init.hip: its intensities never
// change), to the wave's accumulator of such sums instead: no index load, no look-up.  Every other group goes the paths below.
struct UnitSums { double g[4]; };
template <int MODE, bool SKIP, bool MEMO = false>
__device__ __forceinline__ void stats_bits(SweepAcc& a, uint32_t w, const UnitVals<MODE>& u, const float* s_val, uint32_t fm = 0u, const UnitSums* gs = nullptr, double* gacc = nullptr, uint32_t lz = 0u) {
    a.nin += __popc(w & 0x55555555u); a.nout += __popc(w & 0xAAAAAAAAu);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t wj = (w >> (8 * j)) & 0xffu;
        if constexpr (MEMO) { if ((fm >> j) & 1u) { *gacc += gs->g[j]; continue; } }
        if (!SKIP || wj != 0u) {
            if (SKIP && __builtin_amdgcn_ballot_w64(wj != 0xAAu) == 0ull) {
                float lv[4]; double dv[4];
                lookup4<MODE>(u, j, s_val, lv, dv);
#pragma unroll
                for (int bb = 0; bb < 4; bb++) a.sout += unit_value<MODE>(u, j, bb, lv, dv);
            } else if (SKIP && __builtin_amdgcn_ballot_w64((wj & 0x55u) != 0u) == 0ull) {
                // no lane holds an inner voxel here (the rim of the brain mask: outer and excluded voxels mixed): the outer
                // sum alone, masked - the general path would add +0.0 to the inner sum sixteen times for nothing
                if constexpr (MEMO && MODE == 3) stats_group_outer_idx(a, wj, u, j, s_val, lz);
                else stats_group_outer<MODE>(a, wj, u, j, s_val);
            } else {
                stats_group<MODE>(a, wj, u, j, s_val);
            }
        }
    }
}
// the full groups of a unit's class word (all 64 lanes take part: the walk's loop is wave-uniform)
__device__ __forceinline__ uint32_t full_groups(uint32_t w) {
    const uint32_t x = w ^ 0xAAAAAAAAu;
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) if (__builtin_amdgcn_ballot_w64((x & (0xffu << (8 * j))) != 0u) == 0ull) m |= 1u << j;
    return m;
}
// RIM (dense_memo = 2): the groups of a unit's class word whose outer voxels are exactly the voxels that were included at init - no
// lane holds an inner voxel, and the wave counts as many outer voxels as init counted included ones (ic01, ic23: the unit's four
// counts, 16 bits each; not 0).  Inclusion is monotone - a voxel never becomes excluded and an excluded one is never included
// (VB_X is set by init alone) - so the sets are then equal, and the group's outer sum is the sum init formed (k_build_rim).  A full
// group is the case of 256.  The count is exact: every lane packs its four counts (0..4) into the bytes of one word; five DPP steps
// add them over each half of the wave (at most 128 per byte), and the two halves meet in scalar registers, where 256 fits.
// (All 64 lanes take part: the walk's loop is wave-uniform.)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x) {
    return x + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, false);      // (a lane without a source adds 0)
}
// ne: the groups that hold an included voxel; nouter: the unit's outer voxels.
__device__ __forceinline__ uint32_t rim_groups(uint32_t w, uint32_t ic01, uint32_t ic23, uint32_t& ne, uint32_t& nouter) {
    uint32_t x = vrg_rim_pack(w);                                // byte j: this lane's outer voxels of group j (vrg_rim.h)
    x = dpp_add<0x111, 0xf>(x); x = dpp_add<0x112, 0xf>(x); x = dpp_add<0x114, 0xf>(x); x = dpp_add<0x118, 0xf>(x);    // row_shr 1, 2, 4, 8: lane 15 of a row holds the row's counts
    x = dpp_add<0x142, 0xa>(x);                                  // row_bcast 15 into rows 1 and 3: lanes 31 and 63 hold a half-wave's
    const uint32_t a = __builtin_amdgcn_readlane(x, 31), b = __builtin_amdgcn_readlane(x, 63);
    uint32_t inner = 0u;
    if (__builtin_amdgcn_ballot_w64((w & 0x55555555u) != 0u) != 0ull) {         // (rare: the region's voxels are few)
#pragma unroll
        for (int j = 0; j < 4; j++) if (__builtin_amdgcn_ballot_w64((w & (0x55u << (8 * j))) != 0u) != 0ull) inner |= 1u << j;
    }
    return vrg_rim_decide(a, b, inner, ic01, ic23, ne, nouter);
}
// the four group sums of unit u, as scalar loads like the list entries (written by an earlier kernel only: constant address space)
__device__ __forceinline__ void load_gsum(const double* gsum, uint32_t u, UnitSums& o) {
    typedef const double __attribute__((address_space(4))) cf64;
    const cf64* p = (cf64*)gsum + ((size_t)u << 2);
#pragma unroll
    for (int j = 0; j < 4; j++) o.g[j] = p[j];
}
// An entry of the unit list as a scalar load: through a pointer into the constant address space, which tells the compiler that
// nothing in this kernel writes the list (k_gate, the kernel before it on the stream, does) - behind the workgroup barrier that
// follows the LDS table it would otherwise fetch each entry with a vector load, wait for it alone and broadcast it.
__device__ __forceinline__ uint32_t ulist_entry(const uint32_t* ulist, uint32_t k) {
    typedef const uint32_t __attribute__((address_space(4))) cu32;
    return ((cu32*)ulist)[k];
}
template <bool NT>
__device__ __forceinline__ uint32_t load_cls(const uint32_t* cls, uint32_t u, uint32_t lane) {
    const uint32_t* pc = cls + ((size_t)u << 6) + lane;
    return NT ? __builtin_nontemporal_load(pc) : *pc;
}
// The walk of dense_memo = 2 decides per TRIP, not per group, whether it needs rim_groups at all (vrg_rim.h, "the unit-level decision":
// no inner voxel and as many outer voxels per unit as init counted included ones - the argument stands there).  A lane's counts of two
// units share a word; six DPP steps leave the wave's sums in lane 63.
__device__ __forceinline__ uint32_t wave_total63(uint32_t x) {
    x = dpp_add<0x111, 0xf>(x); x = dpp_add<0x112, 0xf>(x); x = dpp_add<0x114, 0xf>(x); x = dpp_add<0x118, 0xf>(x);    // row_shr 1, 2, 4, 8
    x = dpp_add<0x142, 0xa>(x);                                  // row_bcast 15 into rows 1 and 3
    return dpp_add<0x143, 0xc>(x);                               // row_bcast 31 into rows 2 and 3: lane 63 holds all 64 lanes'
}
__device__ __forceinline__ double readlane_f64(double x, int l) {
    const u2v b = __builtin_bit_cast(u2v, x);
    return __builtin_bit_cast(double, u2v{(uint32_t)__builtin_amdgcn_readlane((int)b.x, l), (uint32_t)__builtin_amdgcn_readlane((int)b.y, l)});
}
// What the walk holds of one trip, all of it fetched with VECTOR loads of lane-distributed addresses: they return in order and their
// number is static, so the compiler counts its waits.  Lanes 4 q .. 4 q + 3 belong to slot q of the trip (the lanes above UNITS * 4
// repeat the last slot).  ent: the slot's list entry (its unit).  w: the class words (all 64 lanes, per slot).  gs: lane 4 q + j
// holds sum j of slot q's unit.  ic: lanes 4 q and 4 q + 1 hold the two words of its counts.
template <int UNITS> struct RimStage { uint32_t ent; uint32_t w[UNITS]; double gs; uint32_t ic; };
// The trips of a turn of the short way: the walk's window, seven VGPRs per trip and one for the entry behind it.  Measured at 2, 3 and
// 4 (bench.py 880x880x640, 768 workgroups, three rounds each in turn: pass 0.0335 / 0.0322-0.0326 / 0.0342-0.0343 ms; four trips take
// all 128 VGPRs).  (-DVRG_RIM_TRIPS=n builds another width for an A/B: python -m arterynetwork_amd.build --define VRG_RIM_TRIPS=2 --out ...)
#ifndef VRG_RIM_TRIPS
#define VRG_RIM_TRIPS 3
#endif
constexpr int RIM_TRIPS = VRG_RIM_TRIPS;
template <int UNITS>
__device__ __forceinline__ uint32_t rim_entries(const uint32_t* __restrict__ ulist, uint32_t k, uint32_t last, uint32_t lane) {
    return ulist[min(k + min(lane >> 2, (uint32_t)(UNITS - 1)), last)];       // (clamped: a slot past the list's end reads the last entry and is zeroed where it is used)
}
// the class words, sums and counts of the units of ent (isum, icnt: the tables of k_build_rim)
template <int UNITS, bool NT>
__device__ __forceinline__ void rim_request(RimStage<UNITS>& s, uint32_t ent, const uint32_t* __restrict__ cls, const double* __restrict__ isum, const uint32_t* __restrict__ icnt, uint32_t lane) {
    s.ent = ent;
#pragma unroll
    for (int q = 0; q < UNITS; q++) s.w[q] = load_cls<NT>(cls, (uint32_t)__builtin_amdgcn_readlane((int)ent, 4 * q), lane);
    s.gs = isum[((size_t)ent << 2) + (lane & 3u)];
    s.ic = icnt[((size_t)ent << 1) + (lane & 1u)];
}
// the intensities of the lane's 4 x 4 voxels of unit u.  SKIP: a group of four voxels that are all excluded (class 0:
// label 4 or padding) is not fetched - the reference's dataArray[mask] gathers (:249-250) do not touch excluded voxels
// either; a 128-byte line is then not transferred when all eight lanes that share it skip it, i.e. wherever 32
// consecutive voxels are excluded (the brain mask leaves long runs).  The sums are bit-identical: a class-0 voxel
// contributes +0.0 either way.
template <int MODE, bool NT, bool SKIP>
__device__ __forceinline__ void load_vals(const VrgCtx& c, uint32_t u, uint32_t lane, uint32_t w, UnitVals<MODE>& o, uint32_t fm = 0u) {
    const uint32_t base = (u << 10) + (lane << 2);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool need = (!SKIP || ((w >> (8 * j)) & 0xffu) != 0u) && !((fm >> j) & 1u);     // (fm: the full groups of a memoising pass - none otherwise)
        if constexpr (MODE == 1 || MODE == 3) {
            o.q[j] = u2v{0u, 0u};
            if (need) { const u2v* pq = reinterpret_cast<const u2v*>(c.lev16 + base + (j << 8)); o.q[j] = NT ? __builtin_nontemporal_load(pq) : *pq; }
        } else if constexpr (MODE == 2) {
            o.f[j][0] = d2v{0.0, 0.0}; o.f[j][1] = d2v{0.0, 0.0};
            if (need) {
                const d2v* pd = reinterpret_cast<const d2v*>(c.I64 + base + (j << 8));
                o.f[j][0] = NT ? __builtin_nontemporal_load(pd) : pd[0];
                o.f[j][1] = NT ? __builtin_nontemporal_load(pd + 1) : pd[1];
            }
        } else {
            o.f[j] = f4v{0.f, 0.f, 0.f, 0.f};
            if (need) { const f4v* pi = reinterpret_cast<const f4v*>(c.I + base + (j << 8)); o.f[j] = NT ? __builtin_nontemporal_load(pi) : *pi; }
        }
    }
}
// The pass walks the LIST of units that hold an included voxel (VrgCtx::ulist, ascending; the 28 % of the bench volume's
// units that lie wholly outside the brain mask are never visited), all waves in formation: trip t of wave w takes
// entries (t * nwaves + w) * UNITS ..., so neighbouring waves read neighbouring units at about the same time and memory
// sees one dense sweep through the volume.  (Measured at 880x880x640: each wave streaming a contiguous range of its own
// - same bytes, every trip useful - took 0.20-0.37 ms by how the ranges were cut; in formation 0.177; the all-units walk
// of round 2, which fetched the class words of the empty units too, 0.19.)
// SKIP = false (option skip_excluded = 0): the listed units are walked the same way with unpredicated loads - each lane
// makes the same additions in the same order, a class-0 voxel adding +0.0: bit-identical sums - and the units that are
// not listed are streamed afterwards for their bytes only.
// The list entries are read through the scalar cache (ulist_entry).
// MEMO (16-bit storage with SKIP, option dense_memo): gsum holds the sum of every 256-voxel group's values (four per unit); a
// unit's four sums arrive through the scalar cache with its class words, one trip ahead, and the groups that are full this
// sweep take theirs (stats_bits).  The wave adds them in the order it meets them, into an accumulator of their own that
// joins lane 0's outer sum behind the walk: a fixed order for a given grid, like every other sum of the pass.  The units
// the slab's faces cut are counted voxel by voxel as ever.
// RIM (with MEMO; dense_memo = 2): gsum is the table of the sums and counts of the voxels included at init (k_build_rim), and the
// groups that take their sum from it are those of rim_groups - the full ones among them.  Such a pass walks the list in a loop of
// its own (the RIM block below): entries, class words, sums and counts come through VECTOR loads a turn of RIM_TRIPS trips ahead, one
// count per turn decides whether its trips need rim_groups at all (vrg_rim.h), and nearly every turn does not.  (With scalar loads and
// a decision per group the kernel spilled 73 SGPRs and stood still four times per trip, one wait behind the other: 0.087 ms per pass
// at 880x880x640; 0.038 with one count per unit - profiles/dense_unit_ab_880.json -, 0.033 with one per turn, the sums added
// lane-parallel and three workgroups per CU - profiles/dense_turn_ab_880.json.)
template <int UNITS, bool NT, int MODE, bool SKIP, bool MEMO = false, bool RIM = false>
__global__ void __launch_bounds__(TPB) k_recount_bits(VrgCtx c, int check_done, const double* gsum, int defer) {
    VRG_CHAOS_POINT(7);
    // (the three words a pass starts from, requested together: all written by kernels of this stream that have ended - or, for the checks
    // that run on the band stream, behind a host synchronisation)
    const int64_t go = c.dctl[VD_GO], rseq = c.dctl[VD_RSEQ];
    const uint32_t n = c.uctl[UC_N];
    if (check_done && check_done < 3 && !go) return;     // the gate says: no sweep to count (the run has stopped) or this sweep's pass is left out
    extern __shared__ __attribute__((aligned(16))) float s_val[];   // 16-bit storage: the level values (c.L floats - MODE 3: doubles -, sized at launch)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t* __restrict__ ulist = c.ulist;
    const uint32_t last = n ? n - 1u : 0u;
    uint32_t i = __builtin_amdgcn_readfirstlane(wave * UNITS);     // (wave-uniform.  The list entries come through the scalar cache, ulist_entry; a RIM pass fetches them with vector loads, rim_entries)
    // (the first trip's units travel with everything else a wave reads first)
    uint32_t uu[UNITS];
    constexpr int T = RIM_TRIPS;                       // (RIM: the trips of a turn of the short way)
    RimStage<UNITS> D[T];                              // (RIM: the walk's window, below)
    uint32_t E[T], en[T];
    const uint32_t step = nwaves * UNITS;
    if constexpr (RIM) {
        static_assert(!RIM || UNITS == 3, "the short way packs the counts of three units into two words");
        static_assert(T >= 2 && T * UNITS <= VRG_TURN_MAX_UNITS, "one word decides a turn of at most 63 units (vrg_rim.h)");
#pragma unroll
        for (int k = 0; k < T; k++) { en[k] = 0u; E[k] = 0u; }
        if (i < n) {                                   // (a wave with nothing to walk reads nothing: an empty list has no readable entry)
#pragma unroll
            for (int k = 0; k < T; k++) en[k] = rim_entries<UNITS>(ulist, i + (uint32_t)k * step, last, lane);
#pragma unroll
            for (int k = 0; k < T; k++) E[k] = rim_entries<UNITS>(ulist, i + (uint32_t)(T + k) * step, last, lane);
        }
    } else {
#pragma unroll
        for (int q = 0; q < UNITS; q++) uu[q] = i < n ? ulist_entry(ulist, min(i + q, last)) : 0u;     // (an empty list has no readable entry)
    }
    if (MODE == 1) {
        for (uint32_t k = threadIdx.x; k < c.L; k += TPB) s_val[k] = (float)c.lev[k];
        __syncthreads();
    }
    if (MODE == 3) {                                 // (the stored value is the float: the same doubles as MODE 1 adds)
        double* s_dv = reinterpret_cast<double*>(s_val);
        for (uint32_t k = threadIdx.x; k < c.L; k += TPB) s_dv[k] = (double)(float)c.lev[k];
        if (MEMO && threadIdx.x == 0) s_dv[c.L] = 0.0;             // (stats_group_outer_idx)
        __syncthreads();
    }
    const uint32_t* __restrict__ cls = c.clsb[(rseq + (check_done >= 3 ? 0 : 1)) & 1];   // (3: the run's last sweep, counted after all)
    const uint32_t plane = (uint32_t)c.PY * (uint32_t)c.PX;
    const uint32_t lo = (2u + (uint32_t)c.z0) * plane;         // this device's Z-slab [z0, z1) as a voxel range
    const uint32_t hi = (2u + (uint32_t)c.z1) * plane;
    uint32_t f_lo = (uint32_t)(((uint64_t)lo + 1023u) >> 10), f_hi = hi >> 10;       // units wholly inside it
    if (f_hi < f_lo) f_hi = f_lo;
    SweepAcc acc = {0, 0, 0.0, 0.0};
    double gacc = 0.0;
    [[maybe_unused]] UnitSums gs[UNITS];           // (the walk of a pass without the rim tables; a RIM pass keeps its sums in its window)
    if constexpr (MEMO && !RIM) {
#pragma unroll
        for (int q = 0; q < UNITS; q++) load_gsum(gsum, uu[q], gs[q]);
    }
    // the class words of a trip are fetched one trip ahead (the intensity loads depend on them), before this trip's
    // intensities: loads return in order, so they cost no wait of their own
    [[maybe_unused]] uint32_t w[UNITS];            // (likewise)
    if constexpr (!RIM) {
#pragma unroll
        for (int q = 0; q < UNITS; q++) { uu[q] = __builtin_amdgcn_readfirstlane(uu[q]); w[q] = i < n ? load_cls<NT>(cls, uu[q], lane) : 0u; }
#pragma unroll
        for (int q = 0; q < UNITS; q++) { asm volatile("" : "+v"(w[q])); if (i + q >= n) w[q] = 0u; }   // settle the first trip's class words here: no waits in mid-loop
    }
    if constexpr (RIM) {
        // RIM: a memoising trip issues hardly an intensity load and forms hardly a sum, so what it would wait for is what it asks for itself:
        // the list entries and then the class words, sums and counts that depend on them.  All of these are vector loads with clamped
        // indices, issued unconditionally.  The wave keeps a window of T trips' class words, sums and counts (D) and the entries of the
        // T trips behind them (E).  The short way takes T trips per turn of its loop: it waits for the window - requested a whole
        // turn ago -, decides the turn with ONE packed word per lane added over the wave and looked at in lane 63 (vrg_rim.h, "one count
        // per TURN"), adds the turn's sums and requests the next window from E and the entries behind it.  The sums are added where the
        // loads left them, one per lane and trip: lane 4 q + j holds sum j of slot q, so the turn costs T additions in every lane, in
        // walk order, into the lane's own accumulator (lsum), and lanes 0..11 join the outer sum behind the walk - a fixed order for a
        // given grid and list.  A group that is empty now was empty at init and its sum is +0.0, which changes nothing (no accumulator
        // ever holds -0.0), so these are the additions rim_groups' masks select.
        // A turn that fails stays a turn (below); only a wave's last trips, fewer than T, move the window on by one trip with copies.
        // Alone, a whole trip is tested by itself (vrg_unit_short) and, if it passes, still adds its twelve sums from the table; only a
        // trip that fails, and the list's last trip if the list ends inside it, goes the per-group way as ever: rim_groups, load_vals,
        // stats_bits (a few dozen trips per pass on the bench volume).
        const double* __restrict__ isum = gsum;
        const uint32_t ngroups = (uint32_t)((((uint64_t)c.PV + 1023u) >> 10) << 2);
        const uint32_t* __restrict__ icnt = reinterpret_cast<const uint32_t*>(gsum + ngroups);
        if (i < n) {
#pragma unroll
            for (int k = 0; k < T; k++) rim_request<UNITS, NT>(D[k], en[k], cls, isum, icnt, lane);
        }
        uint32_t nmemo = 0u;                       // this lane's outer voxels of the trips that went the short way
        double lsum = 0.0;                         // lane 4 q + j: sum j of slot q of those trips, added trip by trip in walk order
        const int32_t role01 = vrg_unit_role01(lane), role2i = vrg_unit_role2i(lane);
        const uint32_t tmask = vrg_turn_mask(lane);
        auto totals = [&](const RimStage<UNITS>& t) -> uint32_t {                          // (lane 63: 0 iff the trip takes the short way, vrg_unit_short)
            const uint32_t share = vrg_unit_share(t.ic);
            return wave_total63(vrg_unit_word01(t.w[0], t.w[1], share, role01)) | wave_total63(vrg_unit_word2i(t.w[0], t.w[1], t.w[2], share, role2i));
        };
        // one trip alone, the window's first, at list position pos: a trip of a turn that failed, or one of a wave's last trips.  A whole
        // trip that passes the test still takes its twelve sums from the table - the same addition as in a turn; only a trip that fails,
        // and the list's last trip if the list ends inside it, goes the per-group way
        auto alone = [&](uint32_t pos) __attribute__((always_inline)) {
            if (pos + UNITS <= n && __builtin_amdgcn_readlane((int)totals(D[0]), 63) == 0) {
                lsum += D[0].gs;
                nmemo += vrg_unit_outer(D[0].w[0]) + vrg_unit_outer(D[0].w[1]) + vrg_unit_outer(D[0].w[2]);
            } else {
                uint32_t wq[UNITS], fm[UNITS];
                UnitVals<MODE> f[UNITS];
#pragma unroll
                for (int q = 0; q < UNITS; q++) {
                    uint32_t ne, no;
                    wq[q] = pos + q < n ? D[0].w[q] : 0u;                                  // (uniform: slots past the list's end hold nothing)
                    uu[q] = (uint32_t)__builtin_amdgcn_readlane((int)D[0].ent, 4 * q);
                    fm[q] = rim_groups(wq[q], (uint32_t)__builtin_amdgcn_readlane((int)D[0].ic, 4 * q), (uint32_t)__builtin_amdgcn_readlane((int)D[0].ic, 4 * q + 1), ne, no);
                }
#pragma unroll
                for (int q = 0; q < UNITS; q++) load_vals<MODE, NT, SKIP>(c, uu[q], lane, wq[q], f[q], fm[q]);
#pragma unroll
                for (int q = 0; q < UNITS; q++) {
                    UnitSums gq;
#pragma unroll
                    for (int j = 0; j < 4; j++) gq.g[j] = readlane_f64(D[0].gs, 4 * q + j);
                    stats_bits<MODE, SKIP, true>(acc, wq[q], f[q], s_val, fm[q], &gq, &gacc, c.L);
                }
            }
        };
        while (i < n) {
            while (i + (uint32_t)(T - 1) * step + UNITS <= n) {            // (T whole trips)
                uint32_t outer = 0u, orw = 0u, shares = 0u;
#pragma unroll
                for (int k = 0; k < T; k++) {
#pragma unroll
                    for (int q = 0; q < UNITS; q++) { outer += vrg_unit_outer(D[k].w[q]); orw |= D[k].w[q]; }
                    shares += vrg_unit_share(D[k].ic);
                }
                if (vrg_turn_short((uint32_t)__builtin_amdgcn_readlane((int)wave_total63(vrg_turn_word(outer, orw, shares, tmask)), 63))) {
                    nmemo += outer;
#pragma unroll
                    for (int k = 0; k < T; k++) lsum += D[k].gs;
                } else {
                    // a turn that fails stays a turn: its trips go alone one after the other, in walk order, each as the window's first - the
                    // window is rotated by one trip with copies, T times, and stands as it stood -, and the next window is requested as ever.
                    // (Leaving the loop here and moving the window on trip by trip cost a wave a memory round trip per trip: with the
                    // region's units in a few waves those waves finished 12 us behind the others, a third of the pass.)
#pragma nounroll
                    for (int r = 0; r < T; r++) {
                        alone(i + (uint32_t)r * step);
                        const RimStage<UNITS> t0 = D[0];
#pragma unroll
                        for (int k = 0; k + 1 < T; k++) D[k] = D[k + 1];
                        D[T - 1] = t0;
                    }
                }
#pragma unroll
                for (int k = 0; k < T; k++) rim_request<UNITS, NT>(D[k], E[k], cls, isum, icnt, lane);
#pragma unroll
                for (int k = 0; k < T; k++) E[k] = rim_entries<UNITS>(ulist, i + (uint32_t)(2 * T + k) * step, last, lane);
                i += (uint32_t)T * step;
            }
            if (i >= n) break;
            alone(i);                                  // (fewer than T whole trips are left: the window moves on by one trip)
#pragma unroll
            for (int k = 0; k + 1 < T; k++) D[k] = D[k + 1];
            rim_request<UNITS, NT>(D[T - 1], E[0], cls, isum, icnt, lane);
#pragma unroll
            for (int k = 0; k + 1 < T; k++) E[k] = E[k + 1];
            E[T - 1] = rim_entries<UNITS>(ulist, i + (uint32_t)(2 * T) * step, last, lane);
            i += step;
        }
        acc.nout += nmemo;
        if (lane < 4u * UNITS) acc.sout += lsum;   // (the lanes above repeat the last slot's sums)
    }
    if constexpr (!RIM) while (i < n) {              // (a RIM instantiation has walked its list above: it holds no second walk)
        const uint32_t in = i + nwaves * UNITS;
        uint32_t un[UNITS], wn[UNITS];
#pragma unroll
        for (int q = 0; q < UNITS; q++) { un[q] = ulist_entry(ulist, min(in + q, last)); wn[q] = load_cls<NT>(cls, un[q], lane); }
#pragma unroll
        for (int q = 0; q < UNITS; q++) if (in + q >= n) wn[q] = 0u;          // (uniform: slots past the list's end hold nothing)
        UnitVals<MODE> f[UNITS];
        if constexpr (MEMO) {
            UnitSums gn[UNITS];
            uint32_t fm[UNITS];
#pragma unroll
            for (int q = 0; q < UNITS; q++) { load_gsum(gsum, un[q], gn[q]); fm[q] = full_groups(w[q]); }
#pragma unroll
            for (int q = 0; q < UNITS; q++) load_vals<MODE, NT, SKIP>(c, uu[q], lane, w[q], f[q], fm[q]);
#pragma unroll
            for (int q = 0; q < UNITS; q++) stats_bits<MODE, SKIP, true>(acc, w[q], f[q], s_val, fm[q], &gs[q], &gacc, c.L);
#pragma unroll
            for (int q = 0; q < UNITS; q++) gs[q] = gn[q];
        } else {
#pragma unroll
            for (int q = 0; q < UNITS; q++) load_vals<MODE, NT, SKIP>(c, uu[q], lane, w[q], f[q]);
#pragma unroll
            for (int q = 0; q < UNITS; q++) stats_bits<MODE, SKIP>(acc, w[q], f[q], s_val);
        }
#pragma unroll
        for (int q = 0; q < UNITS; q++) { w[q] = wn[q]; uu[q] = un[q]; }
        i = in;
    }
    if constexpr (MEMO) { if (lane == 0u) acc.sout += gacc; }
    if (!SKIP) {                                               // the bytes of the units that are not listed (they add nothing)
        for (uint32_t u = f_lo + wave; u < f_hi; u += nwaves) {
            if ((c.ubits[u >> 5] >> (u & 31u)) & 1u) continue;
            UnitVals<MODE> f;
            const uint32_t w1 = load_cls<NT>(cls, u, lane);
            load_vals<MODE, NT, false>(c, u, lane, w1, f);
            if constexpr (MODE == 1 || MODE == 3) { asm volatile("" :: "v"(f.q[0]), "v"(f.q[1]), "v"(f.q[2]), "v"(f.q[3]), "v"(w1)); }
            else if constexpr (MODE == 2) { asm volatile("" :: "v"(f.f[0][0]), "v"(f.f[1][1]), "v"(f.f[2][0]), "v"(f.f[3][1]), "v"(f.f[0][1]), "v"(f.f[1][0]), "v"(f.f[2][1]), "v"(f.f[3][0]), "v"(w1)); }
            else { asm volatile("" :: "v"(f.f[0]), "v"(f.f[1]), "v"(f.f[2]), "v"(f.f[3]), "v"(w1)); }
        }
    }
    // units the slab edges cut: the first and the last unit touching [lo, hi), masked to the slab
    const uint32_t e0 = lo >> 10, e1 = (hi - 1u) >> 10;
    const uint32_t edge = wave == 0 ? e0 : (wave == nwaves - 1 && e1 != e0 ? e1 : 0xffffffffu);
    if (edge != 0xffffffffu && !(edge >= f_lo && edge < f_hi)) {
        UnitVals<MODE> f;
        uint32_t w1 = load_cls<false>(cls, edge, lane);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t v = (edge << 10) + (j << 8) + (lane << 2);        // groups of 4 voxels never straddle a plane
            if (v < lo || v >= hi) w1 &= ~(0xffu << (8 * j));
        }
        load_vals<MODE, false, SKIP>(c, edge, lane, w1, f);
        stats_bits<MODE, SKIP>(acc, w1, f, s_val);
    }
    sweep_finish(c, acc, check_done == 3 ? 0 : check_done, defer != 0);
}
// fp32 storage + skip_excluded (the default; option dense_pipe = 0 switches it off): the same walk, software-pipelined two
// trips deep.  Every intensity load is issued unconditionally - a lane whose group is excluded reads one fixed dummy line
// (the first 16 bytes of the padded volume) instead of being predicated off - so the number of loads in flight is static,
// the compiler's wait counts are exact, and the NEXT trip's intensities are requested before this trip's sums are formed
// (with predicated loads the compiler waits for everything before it forms a sum).  Same additions in the same order:
// bit-identical to k_recount_bits.  Measured (one process, alternating): 880x880x640 0.173 vs 0.178-0.183 ms; 512x512x170
// 0.031 vs 0.036 ms; without a brain mask 0.340 vs 0.335 (nothing to hide there).
template <int UNITS, bool NT>
__device__ __forceinline__ void load_vals_uncond(const VrgCtx& c, uint32_t u, uint32_t lane, uint32_t w, UnitVals<0>& o) {
    const uint32_t base = (u << 10) + (lane << 2);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool need = ((w >> (8 * j)) & 0xffu) != 0u;
        const f4v* pi = reinterpret_cast<const f4v*>(need ? c.I + base + (j << 8) : c.I);
        o.f[j] = NT ? __builtin_nontemporal_load(pi) : *pi;
    }
}
template <int UNITS, bool NT>
__global__ void __launch_bounds__(TPB) k_recount_pipe(VrgCtx c, int check_done, int defer) {
    VRG_CHAOS_POINT(8);
    const int64_t go = c.dctl[VD_GO], rseq = c.dctl[VD_RSEQ];      // (requested together with the list's length, as in k_recount_bits)
    const uint32_t n = c.uctl[UC_N];
    if (check_done && check_done < 3 && !go) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t* __restrict__ ulist = c.ulist;
    const uint32_t last = n ? n - 1u : 0u, stride = nwaves * UNITS;
    uint32_t i = __builtin_amdgcn_readfirstlane(wave * UNITS);     // (wave-uniform: the list is read through the scalar cache)
    const uint32_t* __restrict__ cls = c.clsb[(rseq + (check_done >= 3 ? 0 : 1)) & 1];   // (3: the run's last sweep, counted after all)
    const uint32_t plane = (uint32_t)c.PY * (uint32_t)c.PX;
    const uint32_t lo = (2u + (uint32_t)c.z0) * plane, hi = (2u + (uint32_t)c.z1) * plane;
    uint32_t f_lo = (uint32_t)(((uint64_t)lo + 1023u) >> 10), f_hi = hi >> 10;
    if (f_hi < f_lo) f_hi = f_lo;
    SweepAcc acc = {0, 0, 0.0, 0.0};
    if (i < n) {
        uint32_t u0[UNITS], u1[UNITS], w0[UNITS], w1[UNITS];
        UnitVals<0> fa[UNITS];
#pragma unroll
        for (int q = 0; q < UNITS; q++) { u0[q] = __builtin_amdgcn_readfirstlane(ulist[min(i + q, last)]); w0[q] = load_cls<NT>(cls, u0[q], lane); }
#pragma unroll
        for (int q = 0; q < UNITS; q++) { u1[q] = __builtin_amdgcn_readfirstlane(ulist[min(i + stride + q, last)]); w1[q] = load_cls<NT>(cls, u1[q], lane); }
#pragma unroll
        for (int q = 0; q < UNITS; q++) { if (i + q >= n) w0[q] = 0u; if (i + stride + q >= n) w1[q] = 0u; }
#pragma unroll
        for (int q = 0; q < UNITS; q++) load_vals_uncond<UNITS, NT>(c, u0[q], lane, w0[q], fa[q]);
        while (i < n) {
            uint32_t u2[UNITS], w2[UNITS];
            UnitVals<0> fb[UNITS];
#pragma unroll
            for (int q = 0; q < UNITS; q++) { u2[q] = __builtin_amdgcn_readfirstlane(ulist[min(i + 2u * stride + q, last)]); w2[q] = load_cls<NT>(cls, u2[q], lane); }
#pragma unroll
            for (int q = 0; q < UNITS; q++) load_vals_uncond<UNITS, NT>(c, u1[q], lane, w1[q], fb[q]);      // the next trip's intensities first ...
#pragma unroll
            for (int q = 0; q < UNITS; q++) stats_bits<0, true>(acc, w0[q], fa[q], nullptr);                 // ... then this trip's sums
#pragma unroll
            for (int q = 0; q < UNITS; q++) { if (i + 2u * stride + q >= n) w2[q] = 0u; w0[q] = w1[q]; u0[q] = u1[q]; fa[q] = fb[q]; w1[q] = w2[q]; u1[q] = u2[q]; }
            i += stride;
        }
    }
    const uint32_t e0 = lo >> 10, e1 = (hi - 1u) >> 10;
    const uint32_t edge = wave == 0 ? e0 : (wave == nwaves - 1 && e1 != e0 ? e1 : 0xffffffffu);
    if (edge != 0xffffffffu && !(edge >= f_lo && edge < f_hi)) {
        UnitVals<0> f;
        uint32_t w1e = load_cls<false>(cls, edge, lane);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t v = (edge << 10) + (j << 8) + (lane << 2);
            if (v < lo || v >= hi) w1e &= ~(0xffu << (8 * j));
        }
        load_vals<0, false, true>(c, edge, lane, w1e, f);
        stats_bits<0, true>(acc, w1e, f, nullptr);
    }
    sweep_finish(c, acc, check_done == 3 ? 0 : check_done, defer != 0);
}

// init: the whole unit list from the bitmap (ulist_refresh, vrg_device.h)
__global__ void __launch_bounds__(GATE_THREADS) k_ulist_init(VrgCtx c) { ulist_refresh(c, true, 0); }
// in front of every recount (dense stream): wait for the sweep's labels, then bring the unit list up to date if that sweep
// (or an earlier one) listed a new unit - rare: label 4 turns into 3 only next to the band
// ... or, with option verify_every, close the sweep's pass without a count (fin = 2: one GPU, the pass is closed here; 1: the
// marker travels through the staged all-reduce like a slab's sums).  VD_GO tells the recount behind the gate what to do.
// Option dense_close: FIRST the gate closes the pass before it, if that one left its slots open (close_publish) - and publishes the
// pass counters before it starts to wait, so that the band side (wait_dense_read_for) never waits for the gate's end.  Everything the gate
// decides from is requested in one batch, ahead of any decision: the pass counters, the request and the stop word, VD_OPEN and one slot
// per thread (a pass of up to GATE_THREADS workgroups: all of them).  What depends on those words - the sizes the open pass has to
// reproduce, the list's generation word - is requested by thread 0 as soon as they are there and arrives while the slots are added.
// (The generation word cannot join the first batch: the band side writes it BEFORE it raises the request, so only a load issued after
// the request has been seen is sure to see it.)
__global__ void __launch_bounds__(GATE_THREADS) k_gate(VrgCtx c, int every, int fin) {
    VRG_CHAOS_POINT(9);
    __shared__ int s_due, s_par;
    __shared__ uint32_t s_gen;
    __shared__ long long sh_n[2][4];
    __shared__ double sh_s[2][4];
    __shared__ long long s_slot[4 * GATE_THREADS];
    const uint32_t t = threadIdx.x;
    int64_t rseq = 0, seqc = 0, req = 0, stop = 0;
    if (t == 0) { rseq = vrg_load_i64(&c.dctl[VD_RSEQ]); seqc = vrg_load_i64(&c.dctl[VD_SEQ]); req = vrg_load_i64(&c.gate[VG_REQ]); stop = vrg_load_i64(&c.gate[VG_STOP]); }
    const uint32_t open = (uint32_t)vrg_load_i64(&c.dctl[VD_OPEN]);        // (uniform: only kernels of this stream write it, and they have ended)
    {   // (nstat >= GATE_THREADS slots exist; those past the pass's grid are not added)
        const long long x = ld_sc1((const long long*)&c.st_nin[t]), y = ld_sc1((const long long*)&c.st_nout[t]);
        const double sx = ld_sc1(&c.st_sin[t]), sy = ld_sc1(&c.st_sout[t]);
        s_slot[t] = x; s_slot[GATE_THREADS + t] = y;
        s_slot[2 * GATE_THREADS + t] = __builtin_bit_cast(long long, sx); s_slot[3 * GATE_THREADS + t] = __builtin_bit_cast(long long, sy);
    }
    int64_t expect[2] = {0, 0};
    uint32_t gen = 0;
    bool early = false;
    if (t == 0) {
        if (open && fin == 2) { expect[0] = vrg_load_i64(&c.exp_ring[2 * ((seqc + 1) % VRG_RING)]); expect[1] = vrg_load_i64(&c.exp_ring[2 * ((seqc + 1) % VRG_RING) + 1]); }
        const int64_t after = rseq + (open ? 1 : 0);
        early = req > after;                                   // (the request is there already: its sweep's generation word is in place)
        if (early) gen = vrg_load_u32(&c.uctl[UC_GEN + (int)((after + 1) & 1) * UC_GEN_STRIDE]);
    }
    __syncthreads();
    if (open) {
        const VrgDense d = slots_total(c, open, sh_n, sh_s, GATE_THREADS, s_slot);
        if (t == 0) { close_publish(c, d, fin, fin == 2 ? expect : nullptr); rseq++; }
    }
    if (t == 0) {
        const int due = gate_dense_due(c, rseq, req, stop) ? 1 : 0;
        const int64_t seq = rseq + 1;                          // the pass this gate stands in front of
        if (due && !early) gen = vrg_load_u32(&c.uctl[UC_GEN + (int)(seq & 1) * UC_GEN_STRIDE]);
        int go = due;
        if (due && vrg_dense_skipped(seq, every, c.ver_n, c.ver_me)) {
            vrg_recount_done(c, vrg_dense_skip_marker());
            if (fin == 2) vrg_dense_fin_one(c, vrg_dense_skip_marker());
            go = 0;
        }
        c.dctl[VD_GO] = go;
        s_due = due; s_par = (int)(seq & 1); s_gen = gen;
    }
    __syncthreads();
    if (s_due && s_gen) ulist_refresh(c, false, s_par);        // (also for a pass that is left out: its sweep's new units join the bitmap at THEIR gate.  It looks at the word again)
}
// ... and where no gate will follow before somebody looks at the pass counters, the trace or the ring (the host, the staged all-reduce,
// a kernel of the other stream behind a host synchronisation): one workgroup that closes the pass before it, if that one is open
__global__ void __launch_bounds__(TPB) k_dense_close(VrgCtx c, int fin) {
    __shared__ long long sh_n[2][4];
    __shared__ double sh_s[2][4];
    const uint32_t open = (uint32_t)vrg_load_i64(&c.dctl[VD_OPEN]);
    if (!open) return;                                         // (uniform)
    const VrgDense d = slots_total(c, open, sh_n, sh_s);
    if (threadIdx.x == 0) close_publish(c, d, fin);
}
__global__ void k_verify_last(VrgCtx c) { vrg_dense_verify_last(c, c.world == 1 ? *c.dn_part : *c.dn); }
__global__ void k_cls_build(VrgCtx c) {
    const uint32_t nd = (uint32_t)((((uint64_t)c.PV + 1023u) >> 10) << 6);
    // (a wave = the 64 class words of ONE 1024-voxel unit: one atomic per listed unit instead of one per non-empty word - 14 M
    // atomics on 15 K bitmap words made this 3 ms of vrg_init at 880x880x640)
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < nd; d += gridDim.x * blockDim.x) {
        const uint32_t w = vrg_cls_word_build(c, d);
        if (__ballot(w != 0u) && (threadIdx.x & 63u) == 0u) vrg_atomic_or(&c.ubits[d >> 11], 1u << ((d >> 6) & 31u));
    }
}

// Bytes one dense pass requests from memory for the class copy the last pass read: per listed unit its list entry (4 B)
// and its class words (256 B; the units the slab's faces cut: always) + every 128-byte intensity line that holds an
// included voxel (what k_recount_bits<.., SKIP> fetches).  memo (a memoising pass, option dense_memo): a whole unit costs the 32 B
// of its four group sums more, and a full group of a whole unit - 256 outer voxels - no intensity lines; out[1] counts those groups.
// memo = 2 (dense_memo = 2, the tables of k_build_rim at isum): a whole unit costs 8 B of counts more still, and a group of a whole unit
// without an inner voxel whose outer voxels number what init counted (not 0) no intensity lines; out[1] counts those of 256 voxels,
// out[2] the others.
__global__ void __launch_bounds__(TPB) k_dense_bytes(VrgCtx c, unsigned long long* out, int memo, const double* isum = nullptr) {
    const uint16_t* icnt = memo == 2 ? reinterpret_cast<const uint16_t*>(isum + ((((uint64_t)c.PV + 1023u) >> 10) << 2)) : nullptr;
    const uint32_t* __restrict__ cls = c.clsb[vrg_load_i64(&c.dctl[VD_RSEQ]) & 1];
    const uint32_t plane = (uint32_t)c.PY * (uint32_t)c.PX;
    const uint32_t lo = (2u + (uint32_t)c.z0) * plane, hi = (2u + (uint32_t)c.z1) * plane;
    const uint32_t e0 = lo >> 10, e1 = (hi - 1u) >> 10;
    uint32_t f_lo = (uint32_t)(((uint64_t)lo + 1023u) >> 10), f_hi = hi >> 10;
    if (f_hi < f_lo) f_hi = f_lo;
    const uint32_t lpl = c.lev16 ? 16u : (c.I ? 8u : 4u);          // lanes (of 4 voxels each) per 128-byte line
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    unsigned long long bytes = 0, full = 0, rim = 0;
    for (uint32_t u = e0 + wave; u <= e1; u += nwaves) {
        const bool whole = u >= f_lo && u < f_hi;
        if (whole && !((c.ubits[u >> 5] >> (u & 31u)) & 1u)) continue;
        uint32_t w = cls[((size_t)u << 6) + lane];
        bytes += whole ? (memo == 2 ? 300u : (memo ? 292u : 260u)) : 256u;      // class words (+ the unit's list entry, + its group sums, + its counts)
        for (int j = 0; j < 4; j++) {
            const uint32_t v = (u << 10) + (j << 8) + (lane << 2);
            const uint32_t wj = (w >> (8 * j)) & 0xffu;
            if (memo == 2 && whole) {                                // (wave-uniform)
                const uint32_t nout = (uint32_t)wave_sum((long long)__popc(wj & 0xAAu));
                if (__ballot((wj & 0x55u) != 0u) == 0ull && nout != 0u && nout == icnt[4u * u + j]) { if (nout == 256u) full++; else rim++; continue; }
            } else if (memo && whole && __ballot(wj != 0xAAu) == 0ull) { full++; continue; }    // (wave-uniform)
            const bool need = v >= lo && v < hi && wj != 0u;
            const uint64_t m = __ballot(need);
            for (uint32_t g = 0; g < 64u; g += lpl) bytes += ((m >> g) & ((1ull << lpl) - 1ull)) ? 128u : 0u;
        }
    }
    if (lane == 0 && bytes) atomicAdd(out, bytes);
    if (lane == 0 && full) atomicAdd(out + 1, full);
    if (lane == 0 && rim) atomicAdd(out + 2, rim);
}

__global__ void k_dense_pack(VrgCtx c) { vrg_dense_pack(c); }
__global__ void k_dense_fin(VrgCtx c) { vrg_dense_fin_staged(c); }

// Non-temporal loads for the dense pass?  By the bytes a pass fetches (counted when init has built the class bits): up
// to a little more than the 256-MiB Infinity Cache, ordinary loads keep most of the slab there from sweep to sweep
// (512x512x170, 102 MB: 0.0345 -> 0.0306 ms per pass, and less HBM traffic for the band kernels to queue behind; 274 MB:
// 0.0582 -> 0.0545); a larger pass would only thrash the cache (342 MB: even; 548 MB: 0.102 -> 0.112; 1.1 GB: 0.19 -> 0.204).
// (The memoising 16-bit pass at 880x880x640 requests 362 MB: ordinary loads 0.0969, 0.0984 ms, step 0.104, 0.107; non-temporal
// 0.0943, 0.0947, step 0.097 - the line stays where it is.)
constexpr uint64_t NT_ABOVE_BYTES = 300ull << 20;
bool dense_nt(const VrgBackend* b, const VrgCtx&) {
    if (b->nt_loads >= 0) return b->nt_loads != 0;
    return b->pass_bytes == 0 || b->pass_bytes > NT_ABOVE_BYTES;
}

// Memoised group sums (option dense_memo): 16-bit storage with skip_excluded, and the sums on hand are those of the level indices
// this pass reads (be_build_lev16 builds both; the pair is dropped together).  By default (-1) only a volume of more than 100 000
// units memoises: the pass of a small one comes out of the Infinity Cache and is not what bounds the step, so the bytes it saves buy
// nothing, and it measured slower (512x512x170, 46 000 units, one run each: pass 0.0261 -> 0.0280 ms, step 0.0332 -> 0.0347;
// 880x880x640: 0.117 -> 0.095, 1024^3: 0.224 -> 0.170).  The whole volume decides, not the slab, so that the ranks of a group
// decide alike (as for the automatic 16-bit storage itself); the slab passes of a large volume have not been timed with it.
// 1: every 16-bit pass; 0: none.
// 2: every 16-bit pass, and the rim groups take their sums from a table as well (rim_groups; the tables of this init's labels, build_rim,
// have to be on hand - the full groups' memo serves otherwise); the default picks 2 wherever it picked 1.  Returns 0, 1 or 2.
int dense_memo(const VrgBackend* b, const VrgCtx& c) {
    if (!b->dense_memo || !b->skip || !c.lev16) return 0;
    const bool large = ((uint64_t)c.PV >> 10) > 100000;
    if (b->dense_memo < 0 && !large) return 0;
    // By default only where init found the rim groups to be a fair share of what is memoised (be_init_finish: at least half as many as full
    // groups - the bench volume has 723 000 against 498 000): without a brain mask a row's end is the only rim group beside three full ones,
    // (Unlike the size rule above, this one looks at the SLAB: be_init_finish counts the groups of this rank's slab, so the ranks of a Z-slab group
    // may choose differently between 2 and 1 - and with that between grids.  Every choice counts the same voxels; only the order of the sums differs.)
    // and the pass measured slower with the tables than without (880x880x640 --no-brain-mask, one run each: 0.0959 -> 0.1115 ms, step 0.0995 -> 0.1175).
    if (b->dense_memo != 1 && (b->dense_memo == 2 || b->rim_auto) && b->isum && b->rim_for == c.lev16) return 2;
    return b->gsum && b->gsum_for == c.lev16 ? 1 : 0;
}

// workgroups of the dense recount: >= 32 one-KiB units per wave, at most 1 workgroup per CU
int dense_blocks(const VrgBackend* b, const VrgCtx& c) {
    if (b->sweep_blocks > 0) return b->sweep_blocks;
    uint64_t units = ((uint64_t)(c.z1 - c.z0) * c.PY * c.PX) >> 10;
    // skipping pass: few registers, many short trips - 3 waves per SIMD on a big volume, the 16-bit variant (LDS look-ups,
    // half the bytes per trip) 8; measured in DESIGN.md section 5.  A SMALL pass (512x512x170, an 80-plane slab) is not
    // what bounds the step - the band chain is, and every recount wave on a CU is a queue of loads the band kernels'
    // dependent loads wait behind: 200-280 workgroups there (512x512x170: step 0.0447 ms with 192-256, 0.0456 with 353,
    // 0.0481 with 512; 880x880x80: 0.0466 with 256, 0.0493 with 483, 0.0505 with 512).
    // Streaming pass (skip_excluded = 0): 1 resp. 2 workgroups per CU.
    if (!b->skip) return (int)std::min<uint64_t>(c.lev16 ? 2 * SWEEP_BLOCKS : SWEEP_BLOCKS, std::max<uint64_t>(64, units / 128));
    // 16-bit storage: four workgroups per CU.  With the list entries coming through the scalar cache a wave no longer stands still
    // three times per trip, and fewer waves keep the pass fed (one session, 880x880x640 / 1024^3: 768 -> 0.123 / -, 1024 -> 0.115 / 0.224,
    // 1280 -> 0.116 / 0.224, 1536 -> 0.126 / 0.245, 1792 -> 0.117 / - ms; with vector loads of the entries 1536 was best: 0.122 / 0.240)
    // (small passes, where the band chain bounds the step: 512x512x170 942 -> 0.0428 ms/step, 384-512 -> 0.0381; 80-plane slab
    // 1289 -> 0.0516, 512 -> 0.0394; 160 planes 1536 -> 0.0633, 1024 -> 0.0499 - measured with vector loads of the entries)
    // The memoising pass (dense_memo) does half the work per trip - the full groups cost it neither loads nor look-ups - and wants more waves
    // to cover what a trip still waits for: six workgroups per CU (tools/sweep_recount.py --storage16, 60 sweeps per point, one process per shape,
    // 880x880x640 / 1024^3: 768 -> 0.120 / 0.237, 1024 -> 0.107, 0.107 / 0.204, 0.204, 1280 -> 0.098, 0.099 / 0.188, 1536 -> 0.097, 0.100 / 0.180, 0.181,
    // 1792 -> 0.107, 0.108 / 0.199, 0.206, 2048 -> 0.104 / - ms; before the rim path of stats_group_outer_idx).  Small passes keep their grid.
    // With the rim groups' memo (dense_memo = 2) a trip is short and waits for nothing it asked for itself, and the pass is flat from 1024 to
    // 2048 workgroups (tools/sweep_recount.py 880x880x640 --storage16, 60 sweeps per point, one process: 256 -> 0.166, 512 -> 0.105, 0.106,
    // 768 -> 0.090, 1024 -> 0.085, 0.085, 1280 -> 0.090, 1536 -> 0.089, 2048 -> 0.084 ms; profiles/dense_rim_ab_880.json): four per CU again.
    // With the walk by units (vector loads of the per-unit data, one count per unit) more waves no longer help: bench.py 880x880x640, three rounds
    // each in turn, pass 1024 -> 0.0379-0.0380 ms, 1536 -> 0.0417-0.0421, 2048 -> 0.0439-0.0442 (profiles/dense_unit_ab_880.json): four per CU stay.
    // With one count per turn and the sums added lane-parallel (a turn of three trips) the pass wants FEWER waves: what is left of it is a fixed
    // part - start, the tickets of sweep_finish, which queue at one address, the last workgroup's sum over the slots - and the stream itself,
    // and the short turn lets three workgroups per CU keep the stream fed.  bench.py 880x880x640, three rounds each in turn, pass / step:
    // 640 -> 0.0332-0.0334 / 0.0389-0.0392 ms, 768 -> 0.0322-0.0326 / 0.0382-0.0388, 1024 -> 0.0359-0.0367 / 0.0429-0.0440; the parent's walk
    // gained nothing below 1024 (768 -> 0.0380-0.0385 / 0.0429-0.0430, 640 -> 0.0417-0.0421 / 0.0470-0.0476); profiles/dense_turn_ab_880.json.
    if (c.lev16) {
        const int memo = dense_memo(b, c);
        return (int)std::min<uint64_t>(units <= 100000 ? 2 * SWEEP_BLOCKS : (memo == 1 ? 6 * SWEEP_BLOCKS : memo == 2 ? 3 * SWEEP_BLOCKS : 4 * SWEEP_BLOCKS), std::max<uint64_t>(64, units / 48));
    }
    // fp32: whole or half multiples of the CU count only - 552 or 640 workgroups leave some CUs with a wave more than others for
    // the whole pass (880x880x160: 552 -> 0.058 ms, 384 -> 0.050; 880x880x320: 640 -> 0.103, 512 -> 0.094, 768 -> 0.091 but a
    // slower step, 0.1035 vs 0.1003, the band chain queueing behind three waves per SIMD); one session, tools/gpu_slabsweep.sh
    // (round 4, with the fused band chain beside the pass - fewer dependent round trips for the pass's loads to delay: 80-plane
    // slab 256 -> 0.0419 ms/step, 384 -> 0.0382, 512 -> 0.0392; 160 planes 384 -> 0.0577, 512 -> 0.0552, 768 -> 0.0582; 512x512x170
    // 256 -> 0.0343, 384 -> 0.0347, 512 -> 0.0509: the band kernels then wait for a place on the chip)
    // (round 6, the chain at 0.031 ms: 512x512x170 - 45 000 units - 256 -> 0.0342-0.0345 ms per step, 320-448 -> 0.0322-0.0331, three repeats each, 512 -> 0.0333, 768 -> 0.035)
    const uint64_t pick = units <= 100000 ? 384 : units <= 350000 ? 512 : 768;
    return (int)std::min<uint64_t>(pick, std::max<uint64_t>(64, units / 110));      // (512x512x170: 45 000 units -> 384, a whole multiple of half the CUs; not 282)
}

}  // namespace

// sum the slab statistics over the ranks: RCCL on the stream, or the host callback (synchronises)
static void reduce_dense(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user, hipStream_t st) {
    if (b->repl) return;                             // (every rank of a leader / follower group counts whole volumes: nothing to sum)
    if (b->comm) {
        ncclResult_t r = ncclAllReduce(c.dn_part, c.dn, 4, ncclDouble, ncclSum, b->comm, st);
        if (r != ncclSuccess && !b->err[0]) {        // sticky: the engine turns it into VRG_E_INTERNAL at its next synchronisation point
            std::snprintf(b->err, sizeof(b->err), "RCCL all-reduce of the slab statistics failed: %s", ncclGetErrorString(r));
            std::fprintf(stderr, "%s\n", b->err);
        }
    } else if (cb) {
        double v[4];
        HIP_CHECK(hipMemcpyAsync(v, c.dn_part, sizeof(v), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        cb(v, user);
        HIP_CHECK(hipMemcpyAsync(c.dn, v, sizeof(v), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
}

// Z-slabs: pack the slab sums of the recounts not yet closed, sum them over the ranks (RCCL on the dense stream, or the
// host callback once per entry), close those passes
constexpr int DENSE_GROUP = 8;
static_assert(DENSE_GROUP <= VRG_STAGE, "staging buffer");
static void reduce_staged(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user) {
    b->dense_pending = 0;
    dense_close_open(b);                             // (the last recount's slab sums join the ring first)
    k_dense_pack<<<1, 1, 0, b->sb>>>(c);
    if (b->comm) {
        ncclResult_t r = ncclAllReduce(c.stage_in, c.stage_out, 4 * VRG_STAGE, ncclDouble, ncclSum, b->comm, b->sb);
        if (r != ncclSuccess && !b->err[0]) {        // sticky: the engine turns it into VRG_E_INTERNAL at its next synchronisation point
            std::snprintf(b->err, sizeof(b->err), "RCCL all-reduce of the slab statistics failed: %s", ncclGetErrorString(r));
            std::fprintf(stderr, "%s\n", b->err);
        }
    } else if (cb) {
        double v[4 * VRG_STAGE]; int64_t n = 0;
        HIP_CHECK(hipMemcpyAsync(v, c.stage_in, sizeof(v), hipMemcpyDeviceToHost, b->sb));
        HIP_CHECK(hipMemcpyAsync(&n, c.dctl + VD_NST, sizeof(n), hipMemcpyDeviceToHost, b->sb));
        HIP_CHECK(hipStreamSynchronize(b->sb));
        for (int64_t j = 0; j < n && j < VRG_STAGE; j++) cb(v + 4 * j, user);
        HIP_CHECK(hipMemcpyAsync(c.stage_out, v, sizeof(v), hipMemcpyHostToDevice, b->sb));
        HIP_CHECK(hipStreamSynchronize(b->sb));
    } else {
        HIP_CHECK(hipMemcpyAsync(c.stage_out, c.stage_in, VRG_STAGE * sizeof(VrgDense), hipMemcpyDeviceToDevice, b->sb));
    }
    k_dense_fin<<<1, 1, 0, b->sb>>>(c);
}


// The two-trips-deep walk of the listed units (option dense_pipe, default 1): fp32 storage with skip_excluded, k_recount_pipe.
static bool dense_deep(const VrgBackend* b, const VrgCtx& c) { return b->dense_pipe && b->skip && c.I && !c.lev16; }

// The start / stop events ride on the dispatch itself (hipExtLaunchKernel): no separate event packets in the stream,
// which cost ~4 us each between two back-to-back recounts.
template <bool NT, bool SKIP>
static void launch_recount_as(const VrgCtx& c, int blocks, int check, int defer, bool deep, const double* gsum, bool rim, hipStream_t st, hipEvent_t e_start, hipEvent_t e_stop) {
    const double* const none = nullptr;
    if constexpr (SKIP) {
        if (deep) { hipExtLaunchKernelGGL((k_recount_pipe<3, NT>), dim3(blocks), dim3(TPB), 0, st, e_start, e_stop, 0, c, check, defer); return; }
        if (gsum && rim) {     // (dense_memo = 2: gsum is the table of build_rim)
            if (c.L <= TAB64_LEVELS) hipExtLaunchKernelGGL((k_recount_bits<3, NT, 3, true, true, true>), dim3(blocks), dim3(TPB), (c.L + 1) * sizeof(double), st, e_start, e_stop, 0, c, check, gsum, defer);
            else hipExtLaunchKernelGGL((k_recount_bits<3, NT, 1, true, true, true>), dim3(blocks), dim3(TPB), c.L * sizeof(float), st, e_start, e_stop, 0, c, check, gsum, defer);
            return;
        }
        if (gsum) {            // (dense_memo: 16-bit storage)
            if (c.L <= TAB64_LEVELS) hipExtLaunchKernelGGL((k_recount_bits<3, NT, 3, true, true>), dim3(blocks), dim3(TPB), (c.L + 1) * sizeof(double), st, e_start, e_stop, 0, c, check, gsum, defer);
            else hipExtLaunchKernelGGL((k_recount_bits<3, NT, 1, true, true>), dim3(blocks), dim3(TPB), c.L * sizeof(float), st, e_start, e_stop, 0, c, check, gsum, defer);
            return;
        }
    }
    if (c.lev16 && c.L <= TAB64_LEVELS) hipExtLaunchKernelGGL((k_recount_bits<3, NT, 3, SKIP>), dim3(blocks), dim3(TPB), c.L * sizeof(double), st, e_start, e_stop, 0, c, check, none, defer);
    else if (c.lev16) hipExtLaunchKernelGGL((k_recount_bits<3, NT, 1, SKIP>), dim3(blocks), dim3(TPB), c.L * sizeof(float), st, e_start, e_stop, 0, c, check, none, defer);
    else if (c.I) hipExtLaunchKernelGGL((k_recount_bits<3, NT, 0, SKIP>), dim3(blocks), dim3(TPB), 0, st, e_start, e_stop, 0, c, check, none, defer);
    else hipExtLaunchKernelGGL((k_recount_bits<2, NT, 2, SKIP>), dim3(blocks), dim3(TPB), 0, st, e_start, e_stop, 0, c, check, none, defer);
}
// One dense pass of this handle on stream st: the gate in front of a sweep's pass (checks 1 and 2: it waits, on the device, until the
// sweep's labels are in place, and keeps the unit list current; also when every pass is counted - with several verifiers this handle
// counts its share), then the recount.  The passes of the sweeps (checks 1, 2) and a follower's counts of them (4) walk the list two
// trips deep where there is such a kernel (dense_deep: fp32 storage); the init count (0) and the verify-last count (3) run once: one trip deep.
// Non-temporal loads (dense_nt): for a pass that is larger than the 256-MiB Infinity Cache, where nothing is worth keeping; a smaller
// slab is read with ordinary loads and then comes out of that cache sweep after sweep.
// Option dense_close (default 1): a pass behind a gate leaves its slots open, and the next kernel on the dense stream closes it - the next
// gate, or k_dense_close wherever the host (or a kernel it orders behind the stream) looks first: dense_close_open.  dense_open: such a pass
// has been enqueued and no k_dense_close behind it yet (the pass may have returned at its gate's word, or a later gate may have closed it:
// k_dense_close then finds nothing open); open_c / open_fin: what that kernel is launched with.
static void launch_recount(VrgBackend* b, const VrgCtx& c, int check, hipStream_t st, hipEvent_t e_start = nullptr, hipEvent_t e_stop = nullptr) {
    const int blocks = dense_blocks(b, c);
    const bool nt = dense_nt(b, c), deep = dense_deep(b, c) && check != 0 && check != 3;
    const int defer = (check == 1 || check == 2) && b->dense_close ? 1 : 0;
    if (check == 1 || check == 2) k_gate<<<1, GATE_THREADS, 0, st>>>(c, b->verify_every, check);
    const int memo = dense_memo(b, c);
    const double* const gsum = memo == 2 ? b->isum : (memo ? b->gsum : nullptr);
    if (b->skip) { if (nt) launch_recount_as<true, true>(c, blocks, check, defer, deep, gsum, memo == 2, st, e_start, e_stop); else launch_recount_as<false, true>(c, blocks, check, defer, deep, gsum, memo == 2, st, e_start, e_stop); }
    else { if (nt) launch_recount_as<true, false>(c, blocks, check, defer, deep, nullptr, false, st, e_start, e_stop); else launch_recount_as<false, false>(c, blocks, check, defer, deep, nullptr, false, st, e_start, e_stop); }
    if (defer) { b->dense_open = true; b->open_c = c; b->open_fin = check; }
}
void dense_close_open(VrgBackend* b) {
    if (!b->dense_open) return;
    b->dense_open = false;
    k_dense_close<<<1, TPB, 0, b->sb>>>(b->open_c, b->open_fin);
}

// init: the class bits and the unit list from the labels, then the first count (the sizes the sweeps keep by increments start from it)
void init_dense(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user) {
    k_cls_build<<<2048, TPB, 0, b->sa>>>(c);
    build_rim(b, c);                     // (dense_memo = 2: what each 256-voxel group includes at init, behind the class bits; the first count may use it)
    k_ulist_init<<<1, GATE_THREADS, 0, b->sa>>>(c);
    launch_recount(b, c, 0, b->sa);
    reduce_dense(b, c, cb, user, b->sa);
}

// dense stream: every voxel once, read-only; k_gate in front of the recount waits until the sweep's labels are in place.
// (Option "serial_streams", for tools that run one kernel at a time - rocprofv3 --pmc does: a kernel that waits on the
// device for another one could then wait for ever, so the host orders the two streams instead.)
void enqueue_dense(VrgBackend* b, const VrgCtx& c, hipEvent_t e_start, hipEvent_t e_stop, be_reduce_fn cb, void* user) {
    if (b->serial) HIP_CHECK(hipStreamSynchronize(b->sa));
    const bool ranks = !b->repl && (c.world > 1 || b->comm || cb);
    launch_recount(b, c, ranks ? 1 : 2, b->sb, e_start, e_stop);
    if (b->serial) { dense_close_open(b); HIP_CHECK(hipStreamSynchronize(b->sb)); }      // (the band kernels the host enqueues next wait for this pass's counter)
    // one GPU: the next kernel on the stream closes the pass (option dense_close = 0: the recount's last workgroup does).  Z-slabs: the slab sums of DENSE_GROUP recounts
    // are summed over the ranks by ONE all-reduce (nothing on the band side waits for it: the decisions use the
    // incremental sizes; the totals are only cross-checked against them and filed in the trace)
    if (ranks && ++b->dense_pending >= DENSE_GROUP) reduce_staged(b, c, cb, user);
}

// option verify_every != 1, at the end of a run (both streams idle, every pass closed): the labels of the last sweep counted
// after all and compared with the sizes kept by increments (collective on several ranks)
void be_verify_last(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user) {
    use_device(b);
    if (b->dense_open) { dense_close_open(b); HIP_CHECK(hipStreamSynchronize(b->sb)); }   // (the count below reads the pass counter on the band stream)
    launch_recount(b, c, 3, b->sa);      // (check 3: no gate - launch_recount puts one in front of checks 1 and 2 only)
    reduce_dense(b, c, cb, user, b->sa);
    k_verify_last<<<1, 1, 0, b->sa>>>(c);
    HIP_CHECK(hipStreamSynchronize(b->sa));
}

void be_dense_flush(VrgBackend* b, const VrgCtx& c, be_reduce_fn cb, void* user) {
    use_device(b);
    const bool ranks = !b->repl && (c.world > 1 || b->comm || cb);
    if (ranks && b->dense_pending) reduce_staged(b, c, cb, user);
    dense_close_open(b);
}

void be_follow_count(VrgBackend* b, const VrgCtx& c, VrgEvents* ev) {
    use_device(b);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ev && ev->enabled > 0 && (b->follow_counts++ % ev->enabled) == 0) {     // (every enabled-th count, as on one GPU: an event pair costs the stream a few us)
        if (b->ev_used == b->ev_pool.size())
            for (int k = 0; k < 32; k++) { EvPair n; HIP_CHECK(hipEventCreate(&n.a)); HIP_CHECK(hipEventCreate(&n.b)); n.trip = 0; n.kind = 0; n.ntrips = 1; b->ev_pool.push_back(n); }
        EvPair& p = b->ev_pool[b->ev_used++];
        p.trip = 0; p.kind = 0; p.ntrips = 1; e0 = p.a; e1 = p.b;
    }
    // the very pass a single GPU runs for this sweep (same kernel, same workgroups, same unit list: the same sums bit for bit); its closing
    // workgroup compares the totals with what the leader filed (check 4)
    launch_recount(b, c, 4, b->sa, e0, e1);
}

// what the dense pass of this handle is launched as: {non-temporal loads, storage mode (0 fp32, 1 u16 level index, 2 f64),
// workgroups, skip_excluded, k_recount_pipe instead of k_recount_bits}
void be_dense_info(VrgBackend* b, const VrgCtx& c, int64_t out[5]) {
    out[0] = dense_nt(b, c) ? 1 : 0; out[1] = c.lev16 ? (c.L <= TAB64_LEVELS ? 3 : 1) : (c.I ? 0 : 2); out[2] = dense_blocks(b, c); out[3] = b->skip ? 1 : 0;
    out[4] = dense_deep(b, c) ? 1 : 0;
}
uint64_t be_dense_bytes(VrgBackend* b, const VrgCtx& c) {
    use_device(b);
    b->memo_groups = 0; b->rim_groups = 0;
    if (!b->skip) {           // every voxel of the slab's units is streamed
        const uint64_t plane = (uint64_t)c.PY * c.PX, lo = (2u + (uint64_t)c.z0) * plane, hi = (2u + (uint64_t)c.z1) * plane;
        const uint64_t bpv4 = c.lev16 ? 9 : (c.I ? 17 : 33);      // 4 x (intensity bytes + 0.25)
        return (hi - lo) * bpv4 / 4;
    }
    dense_close_open(b);                 // (k_dense_bytes reads the pass counter: which class copy the last pass read)
    HIP_CHECK(hipStreamSynchronize(b->sb));
    unsigned long long* d = nullptr; unsigned long long v[3] = {0, 0, 0};
    HIP_CHECK(hipMalloc(&d, 24));
    if (!d) return 0;
    HIP_CHECK(hipMemsetAsync(d, 0, 24, b->sa));
    const int memo = dense_memo(b, c);
    k_dense_bytes<<<ITEM_BLOCKS, TPB, 0, b->sa>>>(c, d, memo, memo == 2 ? b->isum : nullptr);
    HIP_CHECK(hipMemcpyAsync(v, d, 24, hipMemcpyDeviceToHost, b->sa));
    HIP_CHECK(hipStreamSynchronize(b->sa));
    HIP_CHECK(hipFree(d));
    b->memo_groups = (long long)v[1]; b->rim_groups = (long long)v[2];
    return v[0];
}
// the rim groups' tables of this handle (dense_memo = 2): {bytes held, memoised groups of fewer than 256 voxels be_dense_bytes last counted}
void be_dense_rim_info(VrgBackend* b, const VrgCtx&, int64_t out[2]) { out[0] = b->isum ? (int64_t)b->rim_bytes : 0; out[1] = b->rim_groups; }
// the memoised group sums of this handle: {bytes held, full groups be_dense_bytes last counted}
void be_dense_memo_info(VrgBackend* b, const VrgCtx&, int64_t out[2]) { out[0] = b->gsum ? (int64_t)b->gsum_bytes : 0; out[1] = b->memo_groups; }
