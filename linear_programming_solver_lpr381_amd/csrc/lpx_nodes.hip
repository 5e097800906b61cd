// lpx_nodes.hip -- branch-and-bound node assembly on the device (K9): node and child builders, the batched
// solution gather, parent parking and the group's state records, each with its launcher.
#include "lpx_internal.h"

namespace lpx {

// ------------------------------------------------------------------------------------------------
// Branch-and-bound node assembly on the device.  A node LP is the root model plus `d` unit rows
// (Models/Branch&Bound.cs:233-248); its tableau (BuildTableau, Models/PrimalSimplex.cs:179-203) is the
// root tableau with d more rows and d more slack columns.  The root tableau stays resident; a node is
// built by one streaming kernel from it and d cut descriptors instead of 8 MB of host work + H2D.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpx_build_node(const double* __restrict__ T0, int ld0, int R0, int C0,
                                                      double* __restrict__ T, int ld, int R, int C,
                                                      const int32_t* __restrict__ cvar, const double* __restrict__ ccoef,
                                                      const double* __restrict__ czero, const double* __restrict__ crhs,
                                                      int32_t* __restrict__ basis)
{
    const int m0 = R0 - 1, m = R - 1, n = C0 - R0, d = R - R0;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j == 0 && i < m) basis[i] = n + i;                               // :197
    if (j >= ld) return;
    double v = 0.0;
    if (j < C) {
        if (i < m0 || i == m) {                                          // root constraint rows / objective row
            const int i0 = (i == m) ? m0 : i;
            if (j < n + m0) v = T0[(size_t)i0 * ld0 + j];
            else if (j == C - 1) v = T0[(size_t)i0 * ld0 + (C0 - 1)];
        } else {                                                         // branching row k
            const int k = i - m0;
            if (j < n) v = (j == cvar[k]) ? ccoef[k] : czero[k];
            else if (j == n + m0 + k) v = 1.0;                           // its slack, :191
            else if (j == C - 1) v = crhs[k];                            // :192
        }
    }
    (void)d;
    T[(size_t)i * ld + j] = v;
}

// The same for a whole group of nodes in ONE launch (blockIdx.z = node): small node LPs are solved hundreds at a time, and
// a launch + two small copies per node were the largest host phase left.  The kernel also writes each node's live-shape
// record and clears its state record.
__global__ __launch_bounds__(256) void lpx_build_nodes(const double* __restrict__ T0, int ld0, int R0, int C0,
                                                       const BuildDesc* __restrict__ descs,
                                                       const int32_t* __restrict__ cvar, const double* __restrict__ ccoef,
                                                       const double* __restrict__ czero, const double* __restrict__ crhs)
{
    const BuildDesc D = descs[blockIdx.z];
    const int R = D.R, C = D.C, ld = D.ld;
    const int m0 = R0 - 1, m = R - 1, n = C0 - R0;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (i >= R) return;
    if (i == 0 && blockIdx.x == 0) {
        if (threadIdx.x == 0) { D.shape[0] = R; D.shape[1] = C; }
        int32_t* stw = reinterpret_cast<int32_t*>(D.st);
        for (int k = threadIdx.x; k < (int)(sizeof(DevState) / sizeof(int32_t)); k += 256) stw[k] = 0;
    }
    if (j == 0 && i < m) D.basis[i] = n + i;                             // :197
    if (j >= ld) return;
    double v = 0.0;
    if (j < C) {
        if (i < m0 || i == m) {                                          // root constraint rows / objective row
            const int i0 = (i == m) ? m0 : i;
            if (j < n + m0) v = T0[(size_t)i0 * ld0 + j];
            else if (j == C - 1) v = T0[(size_t)i0 * ld0 + (C0 - 1)];
        } else {                                                         // branching row k
            const int k = D.cut0 + (i - m0);
            if (j < n) v = (j == cvar[k]) ? ccoef[k] : czero[k];
            else if (j == n + m0 + (i - m0)) v = 1.0;                    // its slack, :191
            else if (j == C - 1) v = crhs[k];                            // :192
        }
    }
    D.T[(size_t)i * ld + j] = v;
}

hipError_t launch_build_nodes(const double* T0, int ld0, int R0, int C0, const BuildDesc* descs, int count, int maxld, int maxR,
                              const int32_t* cvar, const double* ccoef, const double* czero, const double* crhs, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_build_nodes, dim3((maxld + 255) / 256, maxR, count), dim3(256), 0, s, T0, ld0, R0, C0, descs, cvar, ccoef, czero, crhs);
    return hipGetLastError();
}

// Warm start: the child of a solved node is the parent's FINAL tableau plus one branching
// row expressed in the parent's basis.  With x_k basic in row ik:  `x_k <= f`  becomes  e_k - T[ik,:]  (rhs
// f - x_k* < 0) and  `x_k >= c`  becomes  -e_k + T[ik,:]  (rhs -c + x_k* < 0); the new slack is basic in the new
// row.  The objective row is unchanged, so the tableau stays dual feasible and only the dual loop has to run.
__global__ __launch_bounds__(256) void lpx_build_child(const double* __restrict__ Tp, int ldp, int Rp, int Cp,
                                                       const int32_t* __restrict__ basis_p,
                                                       double* __restrict__ T, int ld, int var, int ik, int is_ge,
                                                       double bound, int32_t* __restrict__ basis)
{
    const int mp = Rp - 1, R = Rp + 1, C = Cp + 1;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j == 0 && i < mp) basis[i] = basis_p[i];
    if (j == 0 && i == mp) basis[mp] = Cp - 1;                      // the new slack column
    if (j >= ld || i >= R) return;
    double v = 0.0;
    if (j < C) {
        const int js = (j < Cp - 1) ? j : ((j == C - 1) ? Cp - 1 : -1);   // source column in the parent (-1: new slack)
        if (i == mp) {                                              // the branching row
            if (js < 0) v = 1.0;
            else {
                const double t = Tp[(size_t)ik * ldp + js];
                const double e = (js == var) ? 1.0 : 0.0;
                const double rhs = (js == Cp - 1) ? bound : 0.0;
                v = is_ge ? ((-e - rhs) + t) : ((e + rhs) - t);     // GE: -e_k + row, rhs -c + x_k ; LE: e_k - row, rhs f - x_k
            }
        } else {
            const int is = (i < mp) ? i : mp;                       // i == mp + 1 is the parent's objective row
            v = (js < 0) ? 0.0 : Tp[(size_t)is * ldp + js];
        }
    }
    T[(size_t)i * ld + j] = v;
}

// lpx_build_child for a group of children in one launch (blockIdx.z = child); shape and state records written here too
__global__ __launch_bounds__(256) void lpx_build_children(const ChildDesc* __restrict__ descs)
{
    const ChildDesc D = descs[blockIdx.z];
    const double* __restrict__ Tp = D.Tp; double* __restrict__ T = D.T;
    const int ldp = D.ldp, Rp = D.Rp, Cp = D.Cp, ld = D.ld, var = D.var, ik = D.ik, is_ge = D.is_ge;
    const double bound = D.bound;
    const int mp = Rp - 1, R = Rp + 1, C = Cp + 1;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (i >= R) return;
    if (i == 0 && blockIdx.x == 0) {
        if (threadIdx.x == 0) { D.shape[0] = R; D.shape[1] = C; }
        int32_t* stw = reinterpret_cast<int32_t*>(D.st);
        for (int k = threadIdx.x; k < (int)(sizeof(DevState) / sizeof(int32_t)); k += 256) stw[k] = 0;
    }
    if (j == 0 && i < mp) D.basis[i] = D.basis_p[i];
    if (j == 0 && i == mp) D.basis[mp] = Cp - 1;                    // the new slack column
    if (j >= ld) return;
    double v = 0.0;
    if (j < C) {
        const int js = (j < Cp - 1) ? j : ((j == C - 1) ? Cp - 1 : -1);   // source column in the parent (-1: new slack)
        if (i == mp) {                                              // the branching row
            if (js < 0) v = 1.0;
            else {
                const double t = Tp[(size_t)ik * ldp + js];
                const double e = (js == var) ? 1.0 : 0.0;
                const double rhs = (js == Cp - 1) ? bound : 0.0;
                v = is_ge ? ((-e - rhs) + t) : ((e + rhs) - t);     // GE: -e_k + row, rhs -c + x_k ; LE: e_k - row, rhs f - x_k
            }
        } else {
            const int is = (i < mp) ? i : mp;                       // i == mp + 1 is the parent's objective row
            v = (js < 0) ? 0.0 : Tp[(size_t)is * ldp + js];
        }
    }
    T[(size_t)i * ld + j] = v;
}

hipError_t launch_build_children(const ChildDesc* descs, int count, int maxld, int maxR, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_build_children, dim3((maxld + 255) / 256, maxR, count), dim3(256), 0, s, descs);
    return hipGetLastError();
}

hipError_t launch_build_child(const double* Tp, int ldp, int Rp, int Cp, const int32_t* basis_p, double* T, int ld,
                              int var, int ik, int is_ge, double bound, int32_t* basis, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_build_child, dim3((ld + 255) / 256, Rp + 1), dim3(256), 0, s, Tp, ldp, Rp, Cp, basis_p, T, ld,
                       var, ik, is_ge, bound, basis);
    return hipGetLastError();
}

// Final solution of a whole batch of nodes in one launch (FinalizeReport's reads, Models/PrimalSimplex.cs:135-138, for
// every node of a B&B group): block b copies node b's RHS column and basis into one contiguous record of the output,
// which is pinned host memory the kernel writes directly -- one launch + one wait per batch instead of two strided
// copies + one wait per node.
__global__ __launch_bounds__(256) void lpx_gather_solution(const GatherDesc* __restrict__ descs, double* __restrict__ out_rhs,
                                                           int32_t* __restrict__ out_basis)
{
    const GatherDesc D = descs[blockIdx.x];
    for (int i = threadIdx.x; i < D.R; i += 256) {
        out_rhs[D.off + i] = D.T[(size_t)i * D.ld + (D.C - 1)];
        if (i < D.R - 1) out_basis[D.off + i] = D.basis[i];
    }
}

hipError_t launch_gather_solution(const GatherDesc* descs, int count, double* out_rhs, int32_t* out_basis, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_gather_solution, dim3(count), dim3(256), 0, s, descs, out_rhs, out_basis);
    return hipGetLastError();
}

hipError_t launch_build_node(const double* T0, int ld0, int R0, int C0, double* T, int ld, int R, int C,
                             const int32_t* cvar, const double* ccoef, const double* czero, const double* crhs,
                             int32_t* basis, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_build_node, dim3((ld + 255) / 256, R), dim3(256), 0, s, T0, ld0, R0, C0, T, ld, R, C,
                       cvar, ccoef, czero, crhs, basis);
    return hipGetLastError();
}

// parent parking for a whole group: every finished node's tableau and basis into its store slot, one launch
__global__ __launch_bounds__(256) void lpx_park_many(const ParkDesc* __restrict__ descs)
{
    const ParkDesc D = descs[blockIdx.y];
    const size_t n2 = D.doubles / 2;                                  // leading dimensions are multiples of 16: whole double2s
    const double2* __restrict__ src = reinterpret_cast<const double2*>(D.srcT);
    double2* __restrict__ dst = reinterpret_cast<double2*>(D.dstT);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < D.m; i += 256) D.dstB[i] = D.srcB[i];
}
hipError_t launch_park_many(const ParkDesc* descs, int count, int blocks_per_node, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_park_many, dim3(blocks_per_node, count), dim3(256), 0, s, descs);
    return hipGetLastError();
}

// state records of a whole group in one launch each way (pinned host array <-> every node's device record): a group of 64
// nodes paid 64 small copies per begin and per poll
__global__ __launch_bounds__(64) void lpx_states_scatter(const SelParams* __restrict__ arr, const DevState* __restrict__ src)
{
    const int32_t* s = reinterpret_cast<const int32_t*>(src + blockIdx.x);
    int32_t* d = reinterpret_cast<int32_t*>(arr[blockIdx.x].st);
    for (int k = threadIdx.x; k < (int)(sizeof(DevState) / sizeof(int32_t)); k += 64) d[k] = s[k];
}
__global__ __launch_bounds__(64) void lpx_states_gather(const SelParams* __restrict__ arr, DevState* __restrict__ dst)
{
    const int32_t* s = reinterpret_cast<const int32_t*>(arr[blockIdx.x].st);
    int32_t* d = reinterpret_cast<int32_t*>(dst + blockIdx.x);
    for (int k = threadIdx.x; k < (int)(sizeof(DevState) / sizeof(int32_t)); k += 64) d[k] = s[k];
}
hipError_t launch_states_scatter(const SelParams* arr, const DevState* src_pinned, int count, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_states_scatter, dim3(count), dim3(64), 0, s, arr, src_pinned);
    return hipGetLastError();
}
hipError_t launch_states_gather(const SelParams* arr, DevState* dst_pinned, int count, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_states_gather, dim3(count), dim3(64), 0, s, arr, dst_pinned);
    return hipGetLastError();
}

}  // namespace lpx
