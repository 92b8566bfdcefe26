// vrg_follow.hip - leader / follower replication in the product backend (vrg_device.h: the overview): the follower's side (its
// label bytes, class bits and trace records from the leader's change log), the RCCL communicator, the transports, IPC and page-locked
// host memory.
#include "vrg_device.h"

int be_comm_unique_id(void* id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "id size");
    return ncclGetUniqueId((ncclUniqueId*)id128) == ncclSuccess ? 0 : -1;
}
int be_comm_init(VrgBackend* b, int nranks, int rank, const void* id128) {
    use_device(b);
    if (b->comm) { ncclCommDestroy(b->comm); b->comm = nullptr; }
    ncclUniqueId id; std::memcpy(&id, id128, sizeof(id));
    ncclResult_t r = ncclCommInitRank(&b->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        b->comm = nullptr;
        if (!b->err[0]) std::snprintf(b->err, sizeof(b->err), "ncclCommInitRank(%d ranks, rank %d) failed: %s", nranks, rank, ncclGetErrorString(r));
        return -1;
    }
    return 0;
}

// ---- leader / follower replication: the follower's side, and the transports -----------------------------------------------------
struct FollowGroup { VrgLogSweep h[8]; int n; int count_last; };
// label bytes and stamps: ONE workgroup, the sweeps in order (a voxel may change in consecutive sweeps) with a barrier between them.
// Runs beside a dense pass, where every dependent load takes 2-3 us: a thread's records of a sweep are fetched together, then the label
// bytes they name, then the stores go out - two round trips per sweep whatever its length (up to FQ x 1024 records; more: another turn).
constexpr int FQ = 8;
typedef uint32_t fu4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ VrgLogRec follow_rec(const VrgLogRec* p) {
    const fu4 v = *reinterpret_cast<const fu4*>(p);
    VrgLogRec r; r.idx = v.x; r.rank = v.y; r.old = (uint8_t)v.z; r.nw = (uint8_t)(v.z >> 8); r.pad = 0; r.pad2 = 0;
    return r;
}
__global__ void __launch_bounds__(GATE_THREADS) k_follow_labels(VrgCtx c, const VrgLogRec* __restrict__ recs, FollowGroup g) {
    const uint32_t t = threadIdx.x;
    const uint32_t safe = vrg_idx(c, 0, 0, 0);
    for (int s = 0; s < g.n; s++) {
        const VrgLogRec* r = recs + g.h[s].rec0;
        const uint32_t n = g.h[s].nrec, k = g.h[s].sweep;
        for (uint32_t i0 = 0; i0 < n; i0 += FQ * GATE_THREADS) {
            VrgLogRec q[FQ]; uint8_t have[FQ];
#pragma unroll
            for (int j = 0; j < FQ; j++) { const uint32_t i = i0 + j * GATE_THREADS + t; q[j] = follow_rec(r + (i < n ? i : n - 1u)); if (i >= n) q[j].idx = VRG_NONE; }
#pragma unroll
            for (int j = 0; j < FQ; j++) have[j] = vrg_load_coherent(c.lab[0] + (q[j].idx != VRG_NONE ? q[j].idx : safe));      // (unconditional: a load under a branch would wait for the ones before it; past L1: another wave of this workgroup may have written the byte a sweep ago)
#pragma unroll
            for (int j = 0; j < FQ; j++) {
                if (q[j].idx == VRG_NONE) continue;
                if ((uint8_t)(have[j] & (VB_LABEL | VB_OOB)) != q[j].old) {      // this rank's labels have drifted from the leader's
                    if (c.dctl[VD_ERR] == 0) { c.dctl[VD_ERR] = 12; c.fexp[3] = (int64_t)k; c.fexp[4] = (int64_t)q[j].idx; c.fexp[5] = (int64_t)have[j]; c.fexp[6] = (int64_t)q[j].old; c.fexp[7] = (int64_t)q[j].nw; }
                    continue;
                }
                c.lab[0][q[j].idx] = q[j].nw;
                if ((q[j].nw & VB_S) && !(q[j].old & VB_S)) c.stamp[q[j].idx] = ((uint64_t)k << 32) | q[j].rank;
            }
        }
        __syncthreads();
    }
}
// class bits (their changes commute: no order between the sweeps - the group's records are one stretch of the batch), trace records;
// then - when the last sweep of the group is counted next - the unit list and what the count has to reproduce
__global__ void __launch_bounds__(GATE_THREADS) k_follow_classes(VrgCtx c, const VrgLogRec* __restrict__ recs, FollowGroup g) {
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)g.n) vrg_follow_trace(c, g.h[t]);
    const uint32_t first = g.h[0].rec0, n = g.h[g.n - 1].rec0 + g.h[g.n - 1].nrec - first;
    const VrgLogRec* r = recs + first;
    for (uint32_t i0 = 0; i0 < n; i0 += FQ * GATE_THREADS) {
        VrgLogRec q[FQ];
#pragma unroll
        for (int j = 0; j < FQ; j++) { const uint32_t i = i0 + j * GATE_THREADS + t; q[j] = follow_rec(r + (i < n ? i : n - 1u)); if (i >= n) q[j].idx = VRG_NONE; }
#pragma unroll
        for (int j = 0; j < FQ; j++) vrg_follow_class_rec(c, q[j]);
    }
    if (!g.count_last) return;
    if (t == 0) vrg_follow_expect(c, g.h[g.n - 1]);
    vrg_drain();
    __syncthreads();
    ulist_refresh(c, false, 0);
}

static hipStream_t label_stream(VrgBackend* b) {
    if (!b->sd) HIP_CHECK(hipStreamCreateWithFlags(&b->sd, hipStreamNonBlocking));
    return b->sd;
}
void be_follow_apply(VrgBackend* b, const VrgCtx& c, const VrgLogRec* recs, const VrgLogSweep* hdr, int n, int count_last) {
    use_device(b);
    for (int i0 = 0; i0 < n; i0 += 8) {
        FollowGroup g; g.n = std::min(8, n - i0); g.count_last = (count_last && i0 + g.n == n) ? 1 : 0;
        for (int i = 0; i < g.n; i++) g.h[i] = hdr[i0 + i];
        k_follow_labels<<<1, GATE_THREADS, 0, label_stream(b)>>>(c, recs, g);
        k_follow_classes<<<1, GATE_THREADS, 0, b->sa>>>(c, recs, g);
    }
}
void be_follow_mark(VrgBackend* b, int slot) {
    use_device(b);
    for (int q = 0; q < 2; q++) {                      // (both streams read the staging buffer: the class bits' and the label bytes')
        hipEvent_t& e = b->mark[2 * slot + q];
        if (q == 1 && !b->sd) continue;
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(e, q ? b->sd : b->sa));
    }
}
void be_follow_wait(VrgBackend* b, int slot) { use_device(b); for (int q = 0; q < 2; q++) if (b->mark[2 * slot + q]) HIP_CHECK(hipEventSynchronize(b->mark[2 * slot + q])); }
static hipStream_t repl_stream(VrgBackend* b) {
    if (!b->sc) HIP_CHECK(hipStreamCreateWithFlags(&b->sc, hipStreamNonBlocking));
    return b->sc;
}
int be_repl_bcast(VrgBackend* b, void* dev_buf, size_t bytes, int root) {
    use_device(b);
    if (!b->comm) return -1;
    const ncclResult_t r = ncclBroadcast(dev_buf, dev_buf, bytes, ncclChar, root, b->comm, repl_stream(b));
    if (r != ncclSuccess) { if (!b->err[0]) std::snprintf(b->err, sizeof(b->err), "RCCL broadcast of the change log failed: %s", ncclGetErrorString(r)); return -1; }
    return 0;
}
int be_repl_allsum(VrgBackend* b, double* dev_buf, size_t n) {
    use_device(b);
    if (!b->comm) return -1;
    const ncclResult_t r = ncclAllReduce(dev_buf, dev_buf, n, ncclDouble, ncclSum, b->comm, repl_stream(b));
    if (r != ncclSuccess) { if (!b->err[0]) std::snprintf(b->err, sizeof(b->err), "RCCL all-reduce of the trace sums failed: %s", ncclGetErrorString(r)); return -1; }
    return 0;
}
void be_repl_wait(VrgBackend* b) { use_device(b); if (b->sc) HIP_CHECK(hipStreamSynchronize(b->sc)); }
void be_repl_copy(VrgBackend* b, void* dst, const void* src, size_t bytes) {
    use_device(b);
    HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, repl_stream(b)));
    HIP_CHECK(hipStreamSynchronize(b->sc));
}
void* be_host_alloc(VrgBackend* b, size_t bytes) { use_device(b); void* p = nullptr; if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
void be_host_free(VrgBackend* b, void* p) { use_device(b); if (p) (void)hipHostFree(p); }
int be_ipc_export(VrgBackend* b, void* dev_ptr, void* handle64) {
    use_device(b);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "ipc handle size");
    if (hipIpcGetMemHandle((hipIpcMemHandle_t*)handle64, dev_ptr) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return 0;
}
void* be_ipc_open(VrgBackend* b, const void* handle64) {
    use_device(b);
    hipIpcMemHandle_t h; std::memcpy(&h, handle64, sizeof(h));
    void* p = nullptr;
    if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void be_ipc_close(VrgBackend* b, void* mapped) { use_device(b); if (mapped && hipIpcCloseMemHandle(mapped) != hipSuccess) (void)hipGetLastError(); }
