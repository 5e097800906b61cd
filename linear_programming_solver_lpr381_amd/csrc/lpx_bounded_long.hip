// lpx_bounded_long.hip -- select kernel of lpx_bounded_dual_run3, gfx950 (CDNA4, wave64): the bounded dual simplex with a
// long-step (bound-flipping) ratio test and an objective cutoff -- and the launcher of every form of the dual loop.
//
// The representation and the launch shape are those of lpx_bounded_dual.hip (ub, flip, lo beside the tableau; 1 workgroup x 1024
// lanes; w and the ratios share 4096 doubles of LDS, or the handle's scratch `ws` beyond that); the steps shared with the other
// two select kernels are the pieces of lpx_bounded.h.  The arithmetic contract is in
// include/lpx.h ("long-step ratio test, objective cutoff and dual start"); DESIGN.md section 4.16 has the launch shape.  Built
// with -ffp-contract=off.
//
// One launch decides ONE pivot and every pass in front of it:
//   CUTOFF: T[m,Cm] <= *B.cutoff (a device double on the handle: a driver moves it without a new parameter record) -> LPX_CUTOFF
//   w_i of every row into `buf`                                -> r  (bnd_leaving_row)
//   kind 1: row r is complemented IN PLACE (bnd_complement_row), before anything else reads it: a pass subtracts from
//           T[r,Cm], and ub[p] - (b - x) and (ub[p] - b) + x round differently
//   column ratios of row r into `buf`, once                    -> q  (rs_hysteresis)
//   LONG_STEP: while ub[q] is finite and T[r,Cm] - ub[q] * T[r,q] is still below -eps, column q PASSES -- the bound flip of
//           lpx_bounded_select (bnd_flip_column), its ratio set to +inf, and the pick is repeated over the same ratio array.
//           A column passes at most once: at most Cm trips.
//   pivot prep after the last pass (bnd_pivot_prep on the row as it stands); the rank-1 update is the lpx_update launch that
//   follows.
// There is no wait on another workgroup anywhere; every loop is bounded by R or Cm.
#include "lpx_bounded.h"       // the pieces shared with the other two kernels, and the declaration of lpx_bounded_dual_select

namespace lpx {

template <bool SKIP_FIXED, bool LONG_STEP, bool CUTOFF>
__global__ __launch_bounds__(SEL_NT) void lpx_bounded_long_select(BndParams B)
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

    int iter = st->iter;                                // events so far (passes and pivots alike)
    if (iter >= P.max_iter) { bnd_exit(st, t, LPX_ITER_LIMIT); return; }
    if constexpr (CUTOFF) {
        // two broadcast loads; nothing is touched, no event
        if (V.row(m)[rhs] <= *B.cutoff) { bnd_exit(st, t, LPX_CUTOFF); return; }
    }

    const int r = bnd_leaving_row(V, B, bnd_buf(m, s_buf, P.ws), s_v, s_i);
    if (r < 0) { bnd_exit(st, t, LPX_OPTIMAL); return; }
    const int kind = V.rhsb[r] < -P.eps ? 0 : 1;        // one address for the whole workgroup: a broadcast load
    const int p = P.basis[r];
    double* trow = V.row(r);

    // ---- kind 1: the complement of row r, materialised in every form
    if (kind) {
        const double up = B.ub[p];
        __syncthreads();                                // uniform: every lane read the same rhsb[r] for `kind`, and has read it before it is rewritten
        bnd_complement_row(V, B, r, p, up);
    }

    // ---- the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
    {
        const double* zrow = V.row(m);
        for (int j = t; j < rhs; j += SEL_NT) {
            const double a = trow[j];
            bool part = a < -P.eps;
            if constexpr (SKIP_FIXED) part = part && B.ub[j] > 0.0;
            ratios[j] = part ? zrow[j] / (-a) : inf;
        }
    }
    __syncthreads();

    // ---- entering column; with LONG_STEP the boxed candidates that leave row r infeasible pass first
    int q = rs_hysteresis(rhs, P.tol_dual, ratios, s_v, s_i, &s_out);
    if constexpr (LONG_STEP) {
        for (int pass = 0; pass < rhs && q >= 0; ++pass) {            // a column passes at most once: its ratio becomes +inf
            const double uq = B.ub[q];
            if (!(uq < inf)) break;
            const double prod = uq * trow[q];           // mul, then sub: contraction is off
            const double nb = V.rhsb[r] - prod;
            if (!(nb < -P.eps)) break;
            __syncthreads();                            // trow[q] and rhsb[r] read by every lane before the rewrite
            bnd_flip_column(V, B, q, uq, iter);
            if (t == 0) ratios[q] = inf;
            ++iter;
            __syncthreads();                            // the next pick reads what this pass wrote
            q = rs_hysteresis(rhs, P.tol_dual, ratios, s_v, s_i, &s_out);
        }
    }
    if (q < 0) {
        // no entering column: the LP is infeasible.  The complement and the passes stay applied (a valid representation).
        if (t == 0) { st->iter = iter; st->primal_count = iter; }
        bnd_exit(st, t, LPX_INFEASIBLE);
        return;
    }
    bnd_pivot_prep(V, B, r, q, p, iter, kind, false);  // on the row as it stands; passes = events - both per-kind counts
}

// The one launcher of the dual loop: b.dual = 1 + flags (lpx_internal.h).  Without LONG_STEP and CUTOFF the kernel is
// lpx_bounded_dual_select (lpx_bounded_dual.hip), with either of them the form of lpx_bounded_long_select above.
hipError_t launch_bounded_dual_select(const BndParams& b, hipStream_t s)
{
    constexpr int SF = LPX_BDUAL_SKIP_FIXED, LS = LPX_BDUAL_LONG_STEP, CO = LPX_BDUAL_CUTOFF;
    void (*k)(BndParams) = nullptr;
    switch (b.dual - 1) {
    case 0:            k = lpx_bounded_dual_select<false>; break;
    case SF:           k = lpx_bounded_dual_select<true>; break;
    case LS:           k = lpx_bounded_long_select<false, true, false>; break;
    case LS | SF:      k = lpx_bounded_long_select<true, true, false>; break;
    case CO:           k = lpx_bounded_long_select<false, false, true>; break;
    case CO | SF:      k = lpx_bounded_long_select<true, false, true>; break;
    case CO | LS:      k = lpx_bounded_long_select<false, true, true>; break;
    case CO | LS | SF: k = lpx_bounded_long_select<true, true, true>; break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3(1), dim3(SEL_NT), 0, s, b);
    return hipGetLastError();
}

}  // namespace lpx
