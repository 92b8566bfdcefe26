// vden_device.hip - vmask_diffuse and vmask_median of include/vmask.h: the edge-preserving denoising step in front of
// vmask_vesselness, which the reference pipeline leaves to an external GUI tool (entry f14).
//
//   k_den_diffuse  one explicit Perona-Malik step, 6 neighbours, float64 (float32 only as the input type of the first step).
//                  A workgroup of 256 threads owns a tile of DY x DX = 16 x 64 voxels of the (axis 1, axis 2) plane - lanes run
//                  along axis 2, a thread holds DR = 4 consecutive rows of one column - and marches over DZ = 32 planes of
//                  axis 0 with the planes z - 1, z, z + 1 of its voxels in registers (and z + 2 on its way), so the +-1-plane
//                  reuse never goes through a cache: per step a voxel is read once, apart from the one-voxel rim of a tile
//                  (the in-plane halo, which the neighbouring tile reads at about the same time) and the two planes that the
//                  chunks before and after re-read (2 of 32).  The plane z of the tile sits in LDS with its halo for the
//                  axis-1 and axis-2 neighbours; two LDS images alternate, one barrier per plane.  Indices are clamped at the
//                  faces when a voxel is loaded, so a missing neighbour is the voxel itself and d = 0.
//   k_den_median   the median over a window of 1, 3, 9 or 27 values by a fixed min / max exchange network in registers
//                  (Batcher's merge exchange, pruned to the comparators the middle output depends on; the halves of a
//                  comparator that nothing reads are never computed).  A workgroup owns MY x MX = 4 x 64 columns and marches
//                  over MZ = 32 planes of axis 0; a thread keeps the in-plane patches of the planes z - 1, z, z + 1 of its
//                  voxel in registers, so it loads 9 values per voxel, not 27.  Reads are clamped by index arithmetic.
// No scratch, no atomics, nothing passes between workgroups; launches are ordered by the stream, one synchronisation at the end.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>

#include "../../include/vmask.h"
#include "../../include/vrg.h"
#include "vmask_common.h"
#include "vmask_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int DEN_T = 256;                         // both kernels: 4 waves, lanes along axis 2
constexpr int DX = 64, DY = 16, DZ = 32;           // k_den_diffuse: the tile along axis 2, axis 1, and the planes of a chunk
constexpr int DR = DY / (DEN_T / DX);              // rows of a thread
constexpr int DHALO = 2 * DX + 2 * DY;             // rim of a tile without the corners: the first 160 threads load one voxel each
constexpr int MX = 64, MY = DEN_T / MX, MZ = 32;   // k_den_median

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------- diffusion
struct DiffGeo {
    int n0, n1, n2;
    double ih0, ih1, ih2, iK, dt;
};

// what the neighbour q adds to acc at p: every operation one IEEE double operation, in the association of vmask.h.
// den_term(p, q) is the exact negative of den_term(q, p) - a difference, products and a conductance that sees only t * t - and
// acc, which starts at +0.0, is never -0.0, so "acc - den_term(p, q)" has the bits of "acc + den_term(q, p)": the kernel
// computes the term of a pair of voxels once where one thread holds both - along axis 0 (kept from the plane before) and
// between the DR rows of a thread - 4.25 divisions per voxel for the definition's 6.
template <int FN>
__device__ __forceinline__ double den_term(double uq, double up, double ih, double iK) {
    const double d = uq - up;
    const double g = d * ih;
    const double t = g * iK;
    const double tt = t * t;
    const double c = FN == 0 ? 1.0 / (1.0 + tt) : exp(-tt);
    return (c * g) * ih;
}

template <class T, int FN>
__global__ void __launch_bounds__(DEN_T) k_den_diffuse(const T* __restrict__ in, double* __restrict__ out, DiffGeo g) {
    __shared__ double tile[2][DY + 2][DX + 2];
    const int t = (int)threadIdx.x, lx = t & (DX - 1), ly = t / DX;
    const int x0 = (int)blockIdx.x * DX, y0 = (int)blockIdx.y * DY, z0 = (int)blockIdx.z * DZ;
    const int z1 = min(z0 + DZ, g.n0);
    const int x = x0 + lx;
    const int64_t plane = (int64_t)g.n1 * g.n2;
    int64_t off[DR];                               // the thread's voxels inside a plane, clamped
#pragma unroll
    for (int k = 0; k < DR; k++) off[k] = (int64_t)clampi(y0 + ly * DR + k, g.n1 - 1) * g.n2 + clampi(x, g.n2 - 1);
    // the thread's voxel of the rim: the row above, the row below, the column left, the column right of the tile
    const bool rim = t < DHALO;                    // (no barrier sits under it)
    int hy, hx;                                    // its place in the LDS image
    if (t < DX) { hy = 0; hx = t + 1; }
    else if (t < 2 * DX) { hy = DY + 1; hx = t - DX + 1; }
    else if (t < 2 * DX + DY) { hy = t - 2 * DX + 1; hx = 0; }
    else { hy = t - 2 * DX - DY + 1; hx = DX + 1; }     // (t >= DHALO: not used)
    const int64_t hoff = (int64_t)clampi(y0 + hy - 1, g.n1 - 1) * g.n2 + clampi(x0 + hx - 1, g.n2 - 1);
    auto at = [&](int z) { return in + (int64_t)clampi(z, g.n0 - 1) * plane; };

    double prv[DR], cur[DR], nxt[DR], far[DR], hnxt = 0.0, hfar = 0.0;
    double f0[DR];                                 // what this plane added at the plane before
    {
        const T* pm = at(z0 - 1); const T* pc = at(z0); const T* pn = at(z0 + 1);
#pragma unroll
        for (int k = 0; k < DR; k++) { prv[k] = (double)pm[off[k]]; cur[k] = (double)pc[off[k]]; nxt[k] = (double)pn[off[k]]; far[k] = nxt[k]; }
        if (rim) { tile[0][hy][hx] = (double)pc[hoff]; hnxt = (double)pn[hoff]; }
#pragma unroll
        for (int k = 0; k < DR; k++) { tile[0][ly * DR + k + 1][lx + 1] = cur[k]; f0[k] = den_term<FN>(cur[k], prv[k], g.ih0, g.iK); }
    }
    __syncthreads();
    const bool col_live = x < g.n2;
    for (int z = z0; z < z1; z++) {
        const int b = (z - z0) & 1;
        if (z + 2 <= z1) {                         // plane z + 2 is the upper neighbour of the next plane but one
            const T* pf = at(z + 2);
#pragma unroll
            for (int k = 0; k < DR; k++) far[k] = (double)pf[off[k]];
            if (rim) hfar = (double)pf[hoff];
        }
        if (z + 1 < z1) {                          // the other image: every wave left it at the last barrier
#pragma unroll
            for (int k = 0; k < DR; k++) tile[b ^ 1][ly * DR + k + 1][lx + 1] = nxt[k];
            if (rim) tile[b ^ 1][hy][hx] = hnxt;
        }
        // what row j of the thread's column adds at row j - 1, j = 0 .. DR (row -1 and row DR: the neighbours' rows, from the
        // image): row j - 1 adds the negative of it at row j
        double e1[DR + 1];
#pragma unroll
        for (int j = 0; j <= DR; j++) {
            const double lo = j > 0 ? cur[j - 1] : tile[b][ly * DR][lx + 1];
            const double hi = j < DR ? cur[j] : tile[b][ly * DR + DR + 1][lx + 1];
            e1[j] = den_term<FN>(hi, lo, g.ih1, g.iK);
        }
#pragma unroll
        for (int k = 0; k < DR; k++) {
            const int r = ly * DR + k + 1;         // the voxel's row in the image
            const double p = cur[k];
            const double up0 = den_term<FN>(nxt[k], p, g.ih0, g.iK);
            double acc = 0.0;
            acc = acc - f0[k];
            acc = acc + up0;
            acc = acc - e1[k];
            acc = acc + e1[k + 1];
            acc = acc + den_term<FN>(tile[b][r][lx], p, g.ih2, g.iK);
            acc = acc + den_term<FN>(tile[b][r][lx + 2], p, g.ih2, g.iK);
            f0[k] = up0;
            const int y = y0 + ly * DR + k;
            if (col_live && y < g.n1) out[(int64_t)z * plane + (int64_t)y * g.n2 + x] = p + g.dt * acc;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DR; k++) { prv[k] = cur[k]; cur[k] = nxt[k]; nxt[k] = far[k]; }
        hnxt = hfar;
    }
}

// ---------------------------------------------------------------- median
// Batcher's merge exchange for n = 3, 9, 27 without the comparators that the middle output does not depend on.
struct CE { unsigned char a, b; };
constexpr CE NET3[] = {{0, 1}, {0, 2}, {1, 2}};
constexpr CE NET9[] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {1, 2}, {5, 6}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {2, 4}, {3, 5},
                       {1, 2}, {3, 4}, {5, 6}, {0, 8}, {4, 8}, {2, 4}, {3, 5}, {3, 4}};
constexpr CE NET27[] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {8, 9}, {10, 11}, {12, 13}, {14, 15}, {16, 17}, {18, 19}, {20, 21}, {22, 23}, {24, 25},
                        {0, 2}, {1, 3}, {4, 6}, {5, 7}, {8, 10}, {9, 11}, {12, 14}, {13, 15}, {16, 18}, {17, 19}, {20, 22}, {21, 23}, {24, 26},
                        {1, 2}, {5, 6}, {9, 10}, {13, 14}, {17, 18}, {21, 22}, {25, 26},
                        {0, 4}, {1, 5}, {2, 6}, {3, 7}, {8, 12}, {9, 13}, {10, 14}, {11, 15}, {16, 20}, {17, 21}, {18, 22}, {19, 23},
                        {2, 4}, {3, 5}, {10, 12}, {11, 13}, {18, 20}, {19, 21},
                        {1, 2}, {3, 4}, {5, 6}, {9, 10}, {11, 12}, {13, 14}, {17, 18}, {19, 20}, {21, 22}, {25, 26},
                        {0, 8}, {1, 9}, {2, 10}, {3, 11}, {4, 12}, {5, 13}, {6, 14}, {7, 15}, {16, 24}, {17, 25}, {18, 26},
                        {4, 8}, {5, 9}, {6, 10}, {7, 11}, {20, 24}, {21, 25}, {22, 26},
                        {2, 4}, {3, 5}, {6, 8}, {7, 9}, {10, 12}, {11, 13}, {18, 20}, {19, 21}, {22, 24}, {23, 25},
                        {1, 2}, {3, 4}, {5, 6}, {7, 8}, {9, 10}, {11, 12}, {13, 14}, {17, 18}, {19, 20}, {21, 22}, {23, 24}, {25, 26},
                        {0, 16}, {1, 17}, {2, 18}, {3, 19}, {4, 20}, {5, 21}, {6, 22}, {7, 23}, {8, 24}, {9, 25}, {10, 26},
                        {8, 16}, {9, 17}, {10, 18}, {11, 19}, {12, 20}, {13, 21}, {14, 22},
                        {7, 11}, {12, 16}, {13, 17}, {14, 18}, {11, 13}, {14, 16}, {13, 14}};

template <int N> struct Net;
template <> struct Net<3> { static constexpr const CE* net = NET3; static constexpr int len = sizeof(NET3) / sizeof(CE); };
template <> struct Net<9> { static constexpr const CE* net = NET9; static constexpr int len = sizeof(NET9) / sizeof(CE); };
template <> struct Net<27> { static constexpr const CE* net = NET27; static constexpr int len = sizeof(NET27) / sizeof(CE); };

__device__ __forceinline__ void exchange(float& a, float& b) { const float lo = fminf(a, b), hi = fmaxf(a, b); a = lo; b = hi; }
__device__ __forceinline__ void exchange(double& a, double& b) { const double lo = fmin(a, b), hi = fmax(a, b); a = lo; b = hi; }

template <int N, class T, size_t... I>
__device__ __forceinline__ void run_net(T (&v)[N], std::index_sequence<I...>) {
    (exchange(v[Net<N>::net[I].a], v[Net<N>::net[I].b]), ...);    // (every index a constant: v stays in registers)
}
template <int N, class T>
__device__ __forceinline__ T median_of(T (&v)[N]) {
    if constexpr (N > 1) run_net<N>(v, std::make_index_sequence<Net<N>::len>());
    return v[N / 2];
}

template <class T, int R0, int R1, int R2>
__global__ void __launch_bounds__(DEN_T) k_den_median(const T* __restrict__ in, T* __restrict__ out, int n0, int n1, int n2) {
    constexpr int P = (2 * R1 + 1) * (2 * R2 + 1), W0 = 2 * R0 + 1, N = P * W0;
    const int x = (int)blockIdx.x * MX + ((int)threadIdx.x & (MX - 1)), y = (int)blockIdx.y * MY + (int)threadIdx.x / MX;
    const int z0 = (int)blockIdx.z * MZ, z1 = min(z0 + MZ, n0);
    if (x >= n2 || y >= n1) return;                // (no barrier in this kernel)
    const int64_t plane = (int64_t)n1 * n2;
    int64_t off[P];                                // the in-plane patch, clamped
#pragma unroll
    for (int a = 0; a <= 2 * R1; a++)
#pragma unroll
        for (int b = 0; b <= 2 * R2; b++) off[a * (2 * R2 + 1) + b] = (int64_t)clampi(y + a - R1, n1 - 1) * n2 + clampi(x + b - R2, n2 - 1);
    T w[W0][P];                                    // the patches of the planes z - R0 .. z + R0
#pragma unroll
    for (int i = 0; i < W0 - 1; i++) {
        const T* p = in + (int64_t)clampi(z0 - R0 + i, n0 - 1) * plane;
#pragma unroll
        for (int j = 0; j < P; j++) w[i][j] = p[off[j]];
    }
    for (int z = z0; z < z1; z++) {
        const T* p = in + (int64_t)clampi(z + R0, n0 - 1) * plane;
#pragma unroll
        for (int j = 0; j < P; j++) w[W0 - 1][j] = p[off[j]];
        T v[N];
#pragma unroll
        for (int i = 0; i < W0; i++)
#pragma unroll
            for (int j = 0; j < P; j++) v[i * P + j] = w[i][j];
        out[(int64_t)z * plane + (int64_t)y * n2 + x] = median_of<N>(v);
#pragma unroll
        for (int i = 0; i < W0 - 1; i++)
#pragma unroll
            for (int j = 0; j < P; j++) w[i][j] = w[i + 1][j];
    }
}

// ---------------------------------------------------------------- host
template <class T>
int diffuse(const T* volume, int64_t n0, int64_t n1, int64_t n2, const DiffGeo& g, int iterations, int function, double* out) {
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const bool in_host = !vmask::is_device_pointer(volume), out_host = !vmask::is_device_pointer(out);
    T* own_in = nullptr; double* own_out = nullptr; double* work = nullptr;
    if ((in_host && mem.grab(&own_in, V, "input")) || (out_host && mem.grab(&own_out, V, "output")) || mem.grab(&work, V, "work volume")) {
        vmask::set_error("out of device memory (diffusion: the input, the output and one float64 volume; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    const T* din = in_host ? own_in : volume; double* dout = out_host ? own_out : out;
    if (in_host) VMASK_TRY(hipMemcpy(own_in, volume, V * sizeof(T), hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n2 + DX - 1) / DX), (unsigned)((n1 + DY - 1) / DY), (unsigned)((n0 + DZ - 1) / DZ));
    for (int i = 0; i < iterations; i++) {
        double* dst = (iterations - 1 - i) % 2 == 0 ? dout : work;     // the last step lands in out
        const double* src = dst == dout ? work : dout;
        if (i == 0) {
            if (function == 0) k_den_diffuse<T, 0><<<grid, DEN_T>>>(din, dst, g);
            else k_den_diffuse<T, 1><<<grid, DEN_T>>>(din, dst, g);
        } else {
            if (function == 0) k_den_diffuse<double, 0><<<grid, DEN_T>>>(src, dst, g);
            else k_den_diffuse<double, 1><<<grid, DEN_T>>>(src, dst, g);
        }
    }
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if (out_host) VMASK_TRY(hipMemcpy(out, dout, V * 8, hipMemcpyDeviceToHost));
    return VRG_OK;
}

template <class T, int R0, int R1, int R2>
void median_launch(const T* in, T* out, int64_t n0, int64_t n1, int64_t n2) {
    const dim3 grid((unsigned)((n2 + MX - 1) / MX), (unsigned)((n1 + MY - 1) / MY), (unsigned)((n0 + MZ - 1) / MZ));
    k_den_median<T, R0, R1, R2><<<grid, DEN_T>>>(in, out, (int)n0, (int)n1, (int)n2);
}

template <class T>
int median(const T* volume, int64_t n0, int64_t n1, int64_t n2, int r0, int r1, int r2, T* out) {
    const size_t V = (size_t)n0 * n1 * n2;
    DevMem mem;
    const bool in_host = !vmask::is_device_pointer(volume), out_host = !vmask::is_device_pointer(out);
    T* own_in = nullptr; T* own_out = nullptr;
    if ((in_host && mem.grab(&own_in, V, "input")) || (out_host && mem.grab(&own_out, V, "output"))) {
        vmask::set_error("out of device memory (median: the input and the output; volumes are not processed in slabs)");
        return VRG_E_MEM;
    }
    const T* din = in_host ? own_in : volume; T* dout = out_host ? own_out : out;
    if (in_host) VMASK_TRY(hipMemcpy(own_in, volume, V * sizeof(T), hipMemcpyHostToDevice));
    switch (r0 * 4 + r1 * 2 + r2) {
        case 0: median_launch<T, 0, 0, 0>(din, dout, n0, n1, n2); break;
        case 1: median_launch<T, 0, 0, 1>(din, dout, n0, n1, n2); break;
        case 2: median_launch<T, 0, 1, 0>(din, dout, n0, n1, n2); break;
        case 3: median_launch<T, 0, 1, 1>(din, dout, n0, n1, n2); break;
        case 4: median_launch<T, 1, 0, 0>(din, dout, n0, n1, n2); break;
        case 5: median_launch<T, 1, 0, 1>(din, dout, n0, n1, n2); break;
        case 6: median_launch<T, 1, 1, 0>(din, dout, n0, n1, n2); break;
        default: median_launch<T, 1, 1, 1>(din, dout, n0, n1, n2); break;
    }
    VMASK_TRY(hipGetLastError());
    VMASK_TRY(hipDeviceSynchronize());
    if (out_host) VMASK_TRY(hipMemcpy(out, dout, V * sizeof(T), hipMemcpyDeviceToHost));
    return VRG_OK;
}

}  // namespace

extern "C" int vmask_diffuse(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, const double* spacing,
                             double K, int iterations, double time_step, int function, double* out) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (dtype != VRG_F32 && dtype != VRG_F64) { vmask::set_error("diffusion: the volume must be float32 or float64"); return VRG_E_ARG; }
    if (iterations < 1 || iterations > 1000) { vmask::set_error("diffusion: 1 to 1000 iterations"); return VRG_E_ARG; }
    if (!(std::isfinite(K) && K > 0.0)) { vmask::set_error("diffusion: K must be finite and positive"); return VRG_E_ARG; }
    if (function != 0 && function != 1) { vmask::set_error("diffusion: function 0 (rational) or 1 (exponential)"); return VRG_E_ARG; }
    double ih[3] = {1.0, 1.0, 1.0};
    for (int a = 0; a < 3 && spacing; a++) {
        if (!(std::isfinite(spacing[a]) && spacing[a] > 0.0)) { vmask::set_error("diffusion: the spacing must be finite and positive"); return VRG_E_ARG; }
        ih[a] = 1.0 / spacing[a];
    }
    const double bound = 1.0 / (2.0 * ((ih[0] * ih[0] + ih[1] * ih[1]) + ih[2] * ih[2]));
    if (!std::isfinite(time_step) || time_step > bound) { vmask::set_error("diffusion: the time step must be finite and at most 1 / (2 sum 1 / h_a^2) (<= 0: half of that)"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    DiffGeo g;
    g.n0 = (int)n0; g.n1 = (int)n1; g.n2 = (int)n2;
    g.ih0 = ih[0]; g.ih1 = ih[1]; g.ih2 = ih[2];
    g.iK = 1.0 / K;
    g.dt = time_step > 0.0 ? time_step : 0.5 * bound;
    if (dtype == VRG_F32) return diffuse<float>((const float*)volume, n0, n1, n2, g, iterations, function, out);
    return diffuse<double>((const double*)volume, n0, n1, n2, g, iterations, function, out);
}

extern "C" int vmask_median(int device, const void* volume, int dtype, int64_t n0, int64_t n1, int64_t n2, int r0, int r1, int r2, void* out) {
    if (!volume || !out) { vmask::set_error("null pointer"); return VRG_E_ARG; }
    if (dtype != VRG_F32 && dtype != VRG_F64) { vmask::set_error("median: the volume must be float32 or float64"); return VRG_E_ARG; }
    if (r0 < 0 || r0 > 1 || r1 < 0 || r1 > 1 || r2 < 0 || r2 > 1) { vmask::set_error("median: every radius 0 or 1"); return VRG_E_ARG; }
    const int rc = vmask::check_args(device, n0, n1, n2);
    if (rc) return rc;
    if (dtype == VRG_F32) return median<float>((const float*)volume, n0, n1, n2, r0, r1, r2, (float*)out);
    return median<double>((const double*)volume, n0, n1, n2, r0, r1, r2, (double*)out);
}
