// vflow_device.hip - vmask_flow of include/vmask.h: the pressures at the free nodes of the branch graph and the flow in every
// branch under the law P_u - P_v = R |Q|^(k-1) Q, for S scenarios of one topology in one launch (DESIGN.md section 9,
// "f13 flow").
//
//   k_flow_check     the tables are looked at before anything is written: every end a node id or -1 -1, every resistance of a
//                    participating branch finite and positive, every fixed pressure finite; one counter of what is wrong
//   k_flow           ONE workgroup of 256 threads per scenario, the grid being the scenarios.  Todini's global gradient
//                    iteration; every linear system by Jacobi-preconditioned conjugate gradients, matrix-free over the node-major
//                    incidence list that the host builds (a node sums its own row: no atomics).  Nothing passes between
//                    workgroups, nothing is ordered by anything but __syncthreads(); the sums follow the orders stated in vmask.h.
// The host derives the topology once per call: which branches take part, the components without a fixed node, the free nodes,
// their anchors, the incidence list.  No floating-point atomics; nothing here is contracted into an FMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"
#include "vseg_slots.h"

#pragma clang fp contract(off)

namespace {

constexpr double EPS_INNER = 1e-8;                 // the inner rule: sqrt(r.z) down by this factor from the solve's start
constexpr double FLOOR_FACTOR = 0.01;              // the floor of |Q| in g: FLOOR_FACTOR tol max |Q|
constexpr u64 NAN_BITS = 0x7ff8000000000000ull;
enum : uint8_t { K_FREE = 0, K_FIXED = 1, K_FLOATING = 2 };

// the topology, the same for every scenario: kind / anchor per node, part per branch, the free nodes ascending, per node the
// entries [inc_off[v], inc_off[v + 1]) of its participating branches in ascending branch index: inc_eb = 2 branch + end, inc_other
// the node at the branch's other end
struct Graph {
    const int64_t* ends; const uint8_t* kind; const uint32_t* anchor; const uint8_t* part; const uint32_t* free;
    const uint32_t* inc_off; const uint32_t* inc_eb; const uint32_t* inc_other; u64 N, B, F;
};
struct Scen { const double* R; u64 rs; const double* pf; u64 ps; double k, tol; int64_t max_iter; };
struct Space { double* node; double* branch; };    // per scenario 4 N and 2 B doubles
struct Res { double* P; double* flow; int64_t* status; double* residual; };

__device__ __forceinline__ bool finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000ll); }

__global__ void __launch_bounds__(TPB) k_flow_check(const int64_t* __restrict__ ends, u64 B, u64 N, const uint8_t* __restrict__ fixed,
                                                    const double* __restrict__ R, u64 nR, const double* __restrict__ pf, u64 nP, u64* __restrict__ bad) {
    u64 wrong = 0;
    const u64 m0 = B > nR ? B : nR, most = m0 > nP ? m0 : nP;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < most; i += (u64)gridDim.x * TPB) {
        if (i < B) {
            const int64_t ea = ends[2 * i], eb = ends[2 * i + 1];
            wrong += ea < -1 || eb < -1 || ea >= (int64_t)N || eb >= (int64_t)N || ((ea < 0) != (eb < 0));
        }
        if (i < nR) {
            const u64 b = i % B;
            const int64_t ea = ends[2 * b], eb = ends[2 * b + 1];
            if (ea >= 0 && eb >= 0 && ea < (int64_t)N && eb < (int64_t)N && ea != eb) { const double x = R[i]; wrong += !(x > 0.0) || !finite(x); }
        }
        if (i < nP && fixed[i % N]) wrong += !finite(pf[i]);
    }
    wave_add(bad, wrong);
}

// the workgroup's sum in the order of vmask.h: a thread's own values in sequence (the caller), the xor tree of every wave, then
// ((w0 + w1) + w2) + w3.  The barrier inside also orders the global writes before it against the reads after it.
__device__ __forceinline__ double block_sum(double v, double (*lds)[TPB / 64], int& slot) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = v + __shfl_xor(v, o, 64);
    if (lane_id() == 0u) lds[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((lds[slot][0] + lds[slot][1]) + lds[slot][2]) + lds[slot][3];
    slot ^= 1;
    return t;
}
__device__ __forceinline__ void block_max2(double& a, double& b, double (*lds)[TPB / 64], int& slot) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { a = fmax(a, __shfl_xor(a, o, 64)); b = fmax(b, __shfl_xor(b, o, 64)); }
    const int sa = slot, sb = slot + 2;
    if (lane_id() == 0u) { lds[sa][threadIdx.x >> 6] = a; lds[sb][threadIdx.x >> 6] = b; }
    __syncthreads();
    a = fmax(fmax(lds[sa][0], lds[sa][1]), fmax(lds[sa][2], lds[sa][3]));
    b = fmax(fmax(lds[sb][0], lds[sb][1]), fmax(lds[sb][2], lds[sb][3]));
    slot ^= 1;
}

__global__ void __launch_bounds__(TPB) k_flow(Graph G, Scen sc, Space ws, Res out) {
    __shared__ double lds[4][TPB / 64];                                   // two slots in turn for the sums, four for the maxima
    int slot = 0;
    const u64 s = blockIdx.x, N = G.N, B = G.B, F = G.F;
    const uint32_t tid = threadIdx.x;
    const double* R = sc.R + s * sc.rs;
    const double* pf = sc.pf + s * sc.ps;
    double* P = out.P + s * N;
    double* flow = out.flow + s * B;
    double* r = ws.node + s * 4 * N; double* p = r + N; double* ap = p + N; double* diag = ap + N;
    double* Q = ws.branch + s * 2 * B; double* g = Q + B;
    const double k = sc.k, tol = sc.tol;
    const bool unit = k == 1.0;                                           // nothing transcendental runs
    const double c = 1.0 - 1.0 / k, inv_k = 1.0 / k, km1 = k - 1.0;
    const u64 cap = 2 * F + 64;

    for (u64 i = tid; i < N; i += TPB) {
        const uint8_t kind = G.kind[i];
        P[i] = kind == K_FIXED ? pf[i] : kind == K_FREE ? pf[G.anchor[i]] : __longlong_as_double((long long)NAN_BITS);
        p[i] = 0.0;
    }
    for (u64 b = tid; b < B; b += TPB) { Q[b] = 0.0; flow[b] = 0.0; }
    __syncthreads();

    int64_t outer = 0, inner = 0, converged = 0;
    double rel = __longlong_as_double(0x7ff0000000000000ll), qm = 0.0;
    while (outer < sc.max_iter) {
        const bool linear = unit || outer == 0;
        const double qfloor = (FLOOR_FACTOR * tol) * qm;
        for (u64 b = tid; b < B; b += TPB) {
            if (!G.part[b]) continue;
            double gb = 1.0 / R[b];
            if (!linear) {
                const double a = fmax(fabs(Q[b]), qfloor);
                if (a > 0.0) gb = 1.0 / ((k * R[b]) * pow(a, km1));
            }
            g[b] = gb;
        }
        __syncthreads();
        double acc = 0.0;
        for (u64 j = tid; j < F; j += TPB) {
            const u64 i = G.free[j];
            const double pi = P[i];
            double sg = 0.0, sd = 0.0, sq = 0.0;
            for (uint32_t e = G.inc_off[i]; e < G.inc_off[i + 1]; e++) {
                const uint32_t eb = G.inc_eb[e], b = eb >> 1;
                const double gb = g[b];
                sg = sg + gb;
                sd = sd + gb * (pi - P[G.inc_other[e]]);
                if (!linear) sq = sq + ((eb & 1u) ? -Q[b] : Q[b]);
            }
            const double ri = linear ? 0.0 - sd : (0.0 - c * sq) - sd;
            const double z = ri / sg;
            r[i] = ri; diag[i] = sg; p[i] = z;
            acc = acc + ri * z;
        }
        double rz = block_sum(acc, lds, slot);
        const double thresh = (EPS_INNER * EPS_INNER) * rz;
        u64 it = 0;
        while (it < cap && rz > thresh) {
            acc = 0.0;
            for (u64 j = tid; j < F; j += TPB) {
                const u64 i = G.free[j];
                const double pi = p[i];
                double a = 0.0;
                for (uint32_t e = G.inc_off[i]; e < G.inc_off[i + 1]; e++) a = a + g[G.inc_eb[e] >> 1] * (pi - p[G.inc_other[e]]);
                ap[i] = a;
                acc = acc + pi * a;
            }
            const double pAp = block_sum(acc, lds, slot);
            if (!(pAp > 0.0)) break;                                      // (the same value in every thread)
            const double alpha = rz / pAp;
            acc = 0.0;
            for (u64 j = tid; j < F; j += TPB) {
                const u64 i = G.free[j];
                P[i] = P[i] + alpha * p[i];
                const double ri = r[i] - alpha * ap[i], z = ri / diag[i];
                r[i] = ri; ap[i] = z;
                acc = acc + ri * z;
            }
            const double rz_new = block_sum(acc, lds, slot);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (u64 j = tid; j < F; j += TPB) { const u64 i = G.free[j]; p[i] = ap[i] + beta * p[i]; }
            it++;
            __syncthreads();
        }
        inner += (int64_t)it;
        __syncthreads();
        double qmax = 0.0, qnew = 0.0;
        for (u64 b = tid; b < B; b += TPB) {
            if (!G.part[b]) continue;
            const double d = P[G.ends[2 * b]] - P[G.ends[2 * b + 1]];
            const double ql = unit ? d / R[b] : copysign(pow(fabs(d) / R[b], inv_k), d);
            flow[b] = ql;
            qmax = fmax(qmax, fabs(ql));
            if (!unit) {
                const double qn = outer == 0 ? ql : c * Q[b] + g[b] * d;
                Q[b] = qn;
                qnew = fmax(qnew, fabs(qn));
            }
        }
        block_max2(qmax, qnew, lds, slot);
        qm = qnew;
        double res = 0.0, unused = 0.0;
        for (u64 j = tid; j < F; j += TPB) {
            const u64 i = G.free[j];
            double sum = 0.0;
            for (uint32_t e = G.inc_off[i]; e < G.inc_off[i + 1]; e++) { const uint32_t eb = G.inc_eb[e]; const double q = flow[eb >> 1]; sum = sum + ((eb & 1u) ? -q : q); }
            res = fmax(res, fabs(sum));
        }
        block_max2(res, unused, lds, slot);
        outer++;
        rel = qmax > 0.0 ? res / qmax : (res == 0.0 ? 0.0 : __longlong_as_double(0x7ff0000000000000ll));
        if (res <= tol * qmax) { converged = 1; break; }
    }
    if (tid == 0u) {
        out.status[3 * s] = converged; out.status[3 * s + 1] = outer; out.status[3 * s + 2] = inner;
        out.residual[s] = rel;
    }
}

struct Args {
    int64_t N, B; const int64_t* ends; const uint8_t* fixed; int64_t S; const double* R; int64_t rs; const double* pf; int64_t ps;
    double k, tol; int64_t max_iter; double* P; double* flow; int64_t* status; double* residual; int64_t* counts;
};

// what the host derives from the (checked) ends and flags
struct Topology {
    std::vector<uint8_t> kind, part;
    std::vector<uint32_t> anchor, free, inc_off, inc_eb, inc_other;
    int64_t floating_components = 0, floating_nodes = 0;
};

void derive(const int64_t* ends, const uint8_t* fixed, u64 N, u64 B, Topology& t) {
    std::vector<uint32_t> parent(N);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    t.part.assign(B, 0);
    for (u64 b = 0; b < B; b++) {
        const int64_t u = ends[2 * b], v = ends[2 * b + 1];
        if (u < 0 || u == v) continue;
        t.part[b] = 1;
        const uint32_t a = find((uint32_t)u), c = find((uint32_t)v);
        if (a != c) parent[std::max(a, c)] = std::min(a, c);
    }
    constexpr uint32_t NOBODY = 0xffffffffu;
    std::vector<uint32_t> anchor_of(N, NOBODY);
    for (u64 v = N; v-- > 0;)
        if (fixed[v]) anchor_of[find((uint32_t)v)] = (uint32_t)v;     // (descending: the smallest fixed node stays)
    t.kind.assign(N, K_FREE); t.anchor.assign(N, 0);
    for (u64 v = 0; v < N; v++) {
        const uint32_t root = find((uint32_t)v), a = anchor_of[root];
        if (a == NOBODY) { t.kind[v] = K_FLOATING; t.floating_nodes++; if (root == v) t.floating_components++; }
        else if (fixed[v]) t.kind[v] = K_FIXED;
        else { t.anchor[v] = a; t.free.push_back((uint32_t)v); }
    }
    t.inc_off.assign(N + 1, 0);
    for (u64 b = 0; b < B; b++) {
        if (t.part[b] && t.kind[ends[2 * b]] == K_FLOATING) t.part[b] = 0;
        if (t.part[b]) { t.inc_off[ends[2 * b] + 1]++; t.inc_off[ends[2 * b + 1] + 1]++; }
    }
    for (u64 v = 0; v < N; v++) t.inc_off[v + 1] += t.inc_off[v];
    t.inc_eb.assign(t.inc_off[N], 0); t.inc_other.assign(t.inc_off[N], 0);
    std::vector<uint32_t> at(t.inc_off.begin(), t.inc_off.end() - 1);
    for (u64 b = 0; b < B; b++) {                                         // ascending branch index at every node, the first end first
        if (!t.part[b]) continue;
        for (uint32_t e = 0; e < 2; e++) {
            const uint32_t v = (uint32_t)ends[2 * b + e], o = (uint32_t)ends[2 * b + 1 - e], slot = at[v]++;
            t.inc_eb[slot] = (uint32_t)(2 * b + e); t.inc_other[slot] = o;
        }
    }
}

int flow(const Args& a) {
    const u64 N = (u64)a.N, B = (u64)a.B, S = (u64)a.S;
    DevMem mem;
    int rc;
    const u64 nR = B * (a.rs ? S : 1), nP = N * (a.ps ? S : 1);
    const int64_t* ends = nullptr; const uint8_t* fixed = nullptr; const double* R = nullptr; const double* pf = nullptr;
    if ((rc = bring(mem, a.ends, 2 * B, "branch ends", &ends)) || (rc = bring(mem, a.fixed, N, "fixed flags", &fixed)) ||
        (rc = bring(mem, a.R, nR, "resistances", &R)) || (rc = bring(mem, a.pf, nP, "fixed pressures", &pf))) return rc;
    u64* ctr = nullptr;
    VMASK_GRAB(ctr, C_PITCH, "counters");
    VMASK_TRY(hipMemsetAsync(ctr, 0, C_PITCH * sizeof(u64), 0));
    const u64 most = std::max(std::max(B, nR), nP);
    u64 bad = 0;
    if (most) {
        k_flow_check<<<grid_for(most, GRID_LIST), TPB>>>(ends, B, N, fixed, R, nR, pf, nP, ctr);
        VMASK_TRY(hipMemcpy(&bad, ctr, sizeof(u64), hipMemcpyDeviceToHost));
    }
    if (bad) { vmask::set_error("the network does not fit: an end that is no node id or -1 -1, a resistance that is not finite and positive, a fixed pressure that is not finite"); return VRG_E_ARG; }

    Topology t;
    Graph G{ends, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, B, 0};
    try {
        std::vector<int64_t> hends;                                       // (host tables are read where they are: only device tables are copied back)
        std::vector<uint8_t> hfixed;
        const int64_t* he = a.ends; const uint8_t* hf = a.fixed;
        if (B && vmask::is_device_pointer(a.ends)) { if ((rc = fetch(a.ends, 2 * B, hends))) return rc; he = hends.data(); }
        if (N && vmask::is_device_pointer(a.fixed)) { if ((rc = fetch(a.fixed, N, hfixed))) return rc; hf = hfixed.data(); }
        derive(he, hf, N, B, t);
    } catch (const std::bad_alloc&) { vmask::set_error("out of host memory (flow topology)"); return VRG_E_MEM; }
    G.F = t.free.size();
    if ((rc = send(mem, t.kind, "node kinds", &G.kind)) || (rc = send(mem, t.anchor, "anchors", &G.anchor)) || (rc = send(mem, t.part, "branch flags", &G.part)) ||
        (rc = send(mem, t.free, "free nodes", &G.free)) || (rc = send(mem, t.inc_off, "incidence offsets", &G.inc_off)) ||
        (rc = send(mem, t.inc_eb, "incidence list", &G.inc_eb)) || (rc = send(mem, t.inc_other, "incidence list", &G.inc_other))) return rc;

    Out<double> oP, oflow, ores;
    Out<int64_t> ostatus;
    if ((rc = oP.open(mem, a.P, S * N, "node pressures")) || (rc = oflow.open(mem, a.flow, S * B, "branch flows")) ||
        (rc = ostatus.open(mem, a.status, 3 * S, "scenario status")) || (rc = ores.open(mem, a.residual, S, "residuals"))) return rc;
    Space ws{nullptr, nullptr};
    VMASK_GRAB(ws.node, S * 4 * N, "work space (nodes)"); VMASK_GRAB(ws.branch, S * 2 * B, "work space (branches)");
    const Scen sc{R, a.rs ? B : 0, pf, a.ps ? N : 0, a.k, a.tol, a.max_iter};
    const Res out{oP.dev, oflow.dev, ostatus.dev, ores.dev};
    k_flow<<<(unsigned)S, TPB>>>(G, sc, ws, out);
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if ((rc = oP.close()) || (rc = oflow.close()) || (rc = ostatus.close()) || (rc = ores.close())) return rc;
    const int64_t counts[2] = {t.floating_components, t.floating_nodes};
    if (a.counts && (rc = put(a.counts, counts, 2))) return rc;
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_flow(int device, int64_t nnode, int64_t nbranch, const int64_t* branch_ends, const uint8_t* fixed,
                          int64_t nscen, const double* resistance, int64_t r_stride, const double* fixed_pressure, int64_t p_stride,
                          double k, double tol, int64_t max_iter,
                          double* node_pressure, double* branch_flow, int64_t* status, double* residual, int64_t* counts) {
    if (nscen < 1 || nscen >= ((int64_t)1 << 31)) { vmask::set_error("the number of scenarios must be 1 .. 2^31 - 1"); return VRG_E_ARG; }
    if (!(k >= 1.0 && k <= 3.0)) { vmask::set_error("the exponent k must be in [1, 3]"); return VRG_E_ARG; }
    if (!(tol > 0.0 && tol < 1.0)) { vmask::set_error("tol must be in (0, 1)"); return VRG_E_ARG; }
    if (max_iter < 1) { vmask::set_error("max_iter must be at least 1"); return VRG_E_ARG; }
    if (nbranch < 0 || nnode < 0 || nbranch >= ((int64_t)1 << 30) || nnode >= ((int64_t)1 << 31)) { vmask::set_error("negative or oversized count"); return VRG_E_ARG; }
    if ((r_stride != 0 && r_stride != nbranch) || (p_stride != 0 && p_stride != nnode)) { vmask::set_error("a stride is 0 (shared) or the row length"); return VRG_E_ARG; }
    if (!status || !residual) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (nbranch && (!branch_ends || !resistance || !branch_flow)) { vmask::set_error("null pointer (branch tables)"); return VRG_E_ARG; }
    if (nnode && (!fixed || !fixed_pressure || !node_pressure)) { vmask::set_error("null pointer (node tables)"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, 1, 1, 1);
    if (rc) return rc;
    const Args a{nnode, nbranch, branch_ends, fixed, nscen, resistance, r_stride, fixed_pressure, p_stride, k, tol, max_iter,
                 node_pressure, branch_flow, status, residual, counts};
    return flow(a);
}
