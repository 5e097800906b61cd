// lpx_bounded.h -- what the select kernels of the bounded-variable family share (private to lpx_bounded.hip, lpx_bounded_dual.hip
// and lpx_bounded_long.hip): the view of the live tableau, the final-status exit, the leaving row of the dual loops, the
// complement of a row, the bound flip of a column and the pivot prep.  Each arithmetic step of the contracts in include/lpx.h
// ("bounded-variable primal simplex", "bounded dual simplex", "long-step ratio test ...") is written here once.  Every piece is
// called by the whole workgroup (1 x SEL_NT lanes); a piece has a barrier inside only where its comment says so, and the
// barriers around it are the caller's.  Built with -ffp-contract=off like the rest of the library.
#pragma once
#include "lpx_resident.h"      // rs_hysteresis (also pulls in lpx_block.h)

namespace lpx {

// w and the ratios live in LDS up to this many doubles; a longer array goes to the handle's global scratch `ws` (it stays in L2)
static constexpr int BND_LDS_DOUBLES = 4096;
__device__ __forceinline__ double* bnd_buf(int n, double* lds, double* ws) { return n <= BND_LDS_DOUBLES ? lds : ws; }

// The record as a kernel reads it, built once: lane, live shape, and the two homes of the RHS column.
struct BndView {
    int t, R, C, m, rhs;
    size_t ld;
    double* T;
    double* rhsb;        // contiguous copy of the RHS column: every write of T[:,rhs] goes here too
    __device__ __forceinline__ explicit BndView(const SelParams& P)
        : t(threadIdx.x), R(P.shape ? P.shape[0] : P.R), C(P.shape ? P.shape[1] : P.C), m(R - 1), rhs(C - 1), ld((size_t)P.ld),
          T(P.T), rhsb(P.rhsbuf) {}
    __device__ __forceinline__ double* row(int i) const { return T + (size_t)i * ld; }
};

// a launch that ends the loop: lpx_update reads st->r = -1 first and returns on it
__device__ __forceinline__ void bnd_exit(DevState* st, int t, int status)
{
    if (t == 0) { st->status = status; st->r = -1; st->q = -1; }
}

// Leaving row of the dual loops: the infeasibility of every row, below zero (kind 0) or above the basic variable's bound
// (kind 1), into wbuf; first strict minimum below -eps, or -1.  One barrier inside; every lane is past its reads of wbuf on return.
__device__ __forceinline__ int bnd_leaving_row(const BndView& V, const BndParams& B, double* wbuf, double* s_v, int* s_i)
{
    const SelParams& P = B.P;
    const double inf = __builtin_inf();
    for (int i = V.t; i < V.m; i += SEL_NT) {
        const double b = V.rhsb[i];
        const int pb = P.basis[i];
        const double u = (unsigned)pb < (unsigned)V.rhs ? B.ub[pb] : inf;   // gather from a small array: L2
        double w = inf;                                                    // the row does not take part
        if (b < -P.eps) w = b;
        else if (u < inf) w = u - b;
        wbuf[i] = w;
    }
    __syncthreads();
    return block_first_min_below(wbuf, 1, V.m, P.eps, s_v, s_i);
}

// Entry j of the complement of a row whose basic variable p (bound up) leaves at its upper bound: every entry but the basic
// column's 1.0 negated, RHS = up - RHS.  Negation is exact, so complementing on the fly in front of a division gives the bits
// of complementing the row and then dividing it.
__device__ __forceinline__ double bnd_complement(double v, int j, int p, int rhs, double up)
{
    return j == rhs ? up - v : (j == p ? v : -v);
}

// The complement of row r materialised, rhsbuf[r] kept current; lane 0 toggles flip[p].  No barrier.
__device__ __forceinline__ void bnd_complement_row(const BndView& V, const BndParams& B, int r, int p, double up)
{
    double* trow = V.row(r);
    for (int j = V.t; j < V.C; j += SEL_NT) {
        const double n = bnd_complement(trow[j], j, p, V.rhs, up);
        trow[j] = n;
        if (j == V.rhs) V.rhsb[r] = n;
    }
    if (V.t == 0) B.flip[p] ^= 1;
}

// Bound flip of column q (bound uq), event `iter`: x_q runs to its other bound and no other column moves -- RHS column and
// column q, R elements each; lane 0 toggles flip[q] and records (-1, q).  No barrier: what reads the result waits in the caller.
__device__ __forceinline__ void bnd_flip_column(const BndView& V, const BndParams& B, int q, double uq, int iter)
{
    const SelParams& P = B.P;
    for (int i = V.t; i < V.R; i += SEL_NT) {
        const double a = V.T[(size_t)i * V.ld + q];
        const double nb = V.rhsb[i] - uq * a;           // mul, then sub: contraction is off
        V.T[(size_t)i * V.ld + V.rhs] = nb;
        V.rhsb[i] = nb;
        V.T[(size_t)i * V.ld + q] = -a;
    }
    if (V.t == 0) {
        B.flip[q] ^= 1;
        if (iter < P.trace_cap) { P.trace[2 * iter] = -1; P.trace[2 * iter + 1] = q; }
    }
}

// Pivot prep on (r, q), event `iter`, and lane 0's record of it: column snapshot -> pcol, barrier, row r normalised -> prow and
// T[r,:] (rhsbuf[r] too: lpx_update leaves row r alone); the rank-1 update is the lpx_update launch that follows.  p = basis[r].
// kind is what the trace (-2 - r for kind 1) and the per-kind counts of lpx_bounded_counts record.  complement: row r still
// stands uncomplemented and its complement is applied on the fly in front of the division; false when kind is 0 or the caller
// has complemented the row in place.
__device__ __forceinline__ void bnd_pivot_prep(const BndView& V, const BndParams& B, int r, int q, int p, int iter, int kind, bool complement)
{
    const SelParams& P = B.P;
    DevState* st = P.st;
    double* trow = V.row(r);
    const double a = trow[q];                           // one address for the whole workgroup: a broadcast load
    const double up = complement ? B.ub[p] : 0.0;
    const double piv = complement ? -a : a;
    for (int i = V.t; i < V.R; i += SEL_NT)
        P.pcol[i] = (i == r) ? 0.0 : V.T[(size_t)i * V.ld + q];
    __syncthreads();                                    // pivot, basis[r] and column read before anything is rewritten
    for (int j = V.t; j < V.C; j += SEL_NT) {
        double v = trow[j];
        if (complement) v = bnd_complement(v, j, p, V.rhs, up);
        const double n = v / piv;
        trow[j] = n;
        P.prow[j] = n;
        if (j == V.rhs) V.rhsb[r] = n;
    }
    if (V.t == 0) {
        if (complement) B.flip[p] ^= 1;
        P.basis[r] = q;
        if (iter < P.trace_cap) { P.trace[2 * iter] = kind ? -2 - r : r; P.trace[2 * iter + 1] = q; }
        st->iter = iter + 1; st->primal_count = iter + 1;
        st->r = r; st->q = q; st->qn = -1;
        if (kind) st->dual_iter += 1; else st->fdf_count += 1;
    }
}

// Defined in lpx_bounded_dual.hip, launched from lpx_bounded_long.hip beside the long-step forms
template <bool SKIP_FIXED>
__global__ void lpx_bounded_dual_select(BndParams B);

}  // namespace lpx
