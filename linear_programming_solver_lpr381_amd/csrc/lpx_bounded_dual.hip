// lpx_bounded_dual.hip -- the dual side of the bounded-variable simplex, gfx950 (CDNA4, wave64): the select kernel of
// lpx_bounded_dual_run / _run2 and the two kernels of lpx_tableau_change_bounds.
//
// The representation is the one of lpx_bounded.hip: ub[j] in [0, +inf] and flip[j] beside the tableau, plus the lower shift
// lo[j] (internal column j stands for x_j - lo[j], or ub[j] - (x_j - lo[j]) when flipped).  The arithmetic contract is in
// include/lpx.h ("bounded dual simplex"); DESIGN.md section 4.14 has the launch shape.  Built with -ffp-contract=off.
//
// One launch of lpx_bounded_dual_select (1 workgroup x 1024 lanes) decides ONE event; the steps it shares with the other two
// select kernels are the pieces of lpx_bounded.h:
//   w_i of every row into `buf` (LDS, or global scratch)       -> r  (bnd_leaving_row)
//   kind 1 (the basic variable of row r is above its bound): row r is complemented, on the fly
//   column ratios of the (complemented) row r into `buf`        -> q  (rs_hysteresis: the exact chain of lpx_select's dual loop)
//   no q: LPX_INFEASIBLE, with the complement of a kind-1 row applied in place (bnd_complement_row)
//   pivot prep (bnd_pivot_prep, complement on the fly); the rank-1 update is the lpx_update launch that follows.
// w and the ratios are never alive together, so they share one array: 4096 doubles of LDS, and the handle's scratch `ws` for
// whichever of them is longer than that.  The kernel is launched from lpx_bounded_long.hip (launch_bounded_dual_select).
#include "lpx_bounded.h"       // the pieces shared with the other two kernels: view, exit, leaving row, complement, pivot prep

namespace lpx {

// SKIP_FIXED (LPX_BDUAL_SKIP_FIXED): a column with ub[j] == 0 does not enter.
template <bool SKIP_FIXED>
__global__ __launch_bounds__(SEL_NT) void lpx_bounded_dual_select(BndParams B)
{
    __shared__ double s_buf[BND_LDS_DOUBLES];
    __shared__ int s_out;
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];

    const SelParams& P = B.P;
    DevState* st = P.st;
    if (st->status != LPX_RUNNING) return;              // uniform: loop already finished

    const BndView V(P);
    const int t = V.t, m = V.m, rhs = V.rhs;
    double* ratios = bnd_buf(rhs, s_buf, P.ws);
    const double inf = __builtin_inf();

    const int iter = st->iter;                          // events so far
    if (iter >= P.max_iter) { bnd_exit(st, t, LPX_ITER_LIMIT); return; }

    const int r = bnd_leaving_row(V, B, bnd_buf(m, s_buf, P.ws), s_v, s_i);
    if (r < 0) { bnd_exit(st, t, LPX_OPTIMAL); return; }
    const int kind = V.rhsb[r] < -P.eps ? 0 : 1;        // one address for the whole workgroup: a broadcast load
    const int p = P.basis[r];

    // ---- entering column over row r.  kind 1: the row is complemented first, on the fly (see bnd_complement)
    {
        const double* trow = V.row(r);
        const double* zrow = V.row(m);
        for (int j = t; j < rhs; j += SEL_NT) {
            double a = trow[j];
            if (kind && j != p) a = -a;
            bool part = a < -P.eps;
            if constexpr (SKIP_FIXED) part = part && B.ub[j] > 0.0;
            ratios[j] = part ? zrow[j] / (-a) : inf;
        }
    }
    __syncthreads();
    const int q = rs_hysteresis(rhs, P.tol_dual, ratios, s_v, s_i, &s_out);
    if (q < 0) {
        // no entering column: the LP is infeasible.  The complement of a kind-1 row stays applied (a valid representation).
        if (kind) bnd_complement_row(V, B, r, p, B.ub[p]);
        bnd_exit(st, t, LPX_INFEASIBLE);
        return;
    }
    bnd_pivot_prep(V, B, r, q, p, iter, kind, kind);
}

template __global__ void lpx_bounded_dual_select<false>(BndParams);     // launched by launch_bounded_dual_select in
template __global__ void lpx_bounded_dual_select<true>(BndParams);      // lpx_bounded_long.hip, which sees all eight forms

// ---- lpx_tableau_change_bounds: two launches, neither reads what it writes ------------------------------------------------------
// Launch 1: the shift of every changed column from the OLD lo / ub / flip, then the new ub and lo.  The columns are distinct
// (checked on the host), so no lane reads an entry another lane writes.
static constexpr int CHG_NT = 256;

__global__ __launch_bounds__(CHG_NT) void lpx_bounds_shift(int K, const int32_t* __restrict__ cols, const double* __restrict__ lower,
                                                           const double* __restrict__ upper, double* __restrict__ ub,
                                                           double* __restrict__ lo, const uint8_t* __restrict__ flip,
                                                           double* __restrict__ shift)
{
    const int k = blockIdx.x * CHG_NT + threadIdx.x;
    if (k >= K) return;
    const int j = cols[k];
    const double lj = lo[j];
    const double l1 = lower[k] - lj;
    const double u1 = upper[k] - lj;                    // +inf stays +inf
    shift[k] = flip[j] ? ub[j] - u1 : l1;
    ub[j] = upper[k] - lower[k];
    lo[j] = lower[k];
}

// Launch 2: one lane per row walks the K shifts in order: T[i,Cm] = T[i,Cm] - s*T[i,j], one multiply and one subtract each
// (contraction is off).  It reads columns j < Cm and writes only the RHS column and its contiguous copy.
__global__ __launch_bounds__(CHG_NT) void lpx_bounds_apply(double* __restrict__ T, int ld, int R, int Cm, int K,
                                                           const int32_t* __restrict__ cols, const double* __restrict__ shift,
                                                           double* __restrict__ rhsbuf)
{
    const int i = blockIdx.x * CHG_NT + threadIdx.x;
    if (i >= R) return;
    double* row = T + (size_t)i * ld;
    double b = row[Cm];
    for (int k = 0; k < K; ++k) {
        const double s = shift[k];                      // uniform: a scalar load
        if (s == 0.0) continue;
        const double prod = s * row[cols[k]];
        b = b - prod;
    }
    row[Cm] = b;
    rhsbuf[i] = b;
}

hipError_t launch_bounds_shift(int K, const int32_t* cols, const double* lower, const double* upper, double* ub, double* lo,
                               const uint8_t* flip, double* shift, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_bounds_shift, dim3((K + CHG_NT - 1) / CHG_NT), dim3(CHG_NT), 0, s, K, cols, lower, upper, ub, lo, flip, shift);
    return hipGetLastError();
}

hipError_t launch_bounds_apply(double* T, int ld, int R, int Cm, int K, const int32_t* cols, const double* shift, double* rhsbuf,
                               hipStream_t s)
{
    hipLaunchKernelGGL(lpx_bounds_apply, dim3((R + CHG_NT - 1) / CHG_NT), dim3(CHG_NT), 0, s, T, ld, R, Cm, K, cols, shift, rhsbuf);
    return hipGetLastError();
}

}  // namespace lpx
