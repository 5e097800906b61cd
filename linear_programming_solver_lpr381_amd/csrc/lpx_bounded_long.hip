// lpx_bounded_long.hip -- select kernel of lpx_bounded_dual_run3, gfx950 (CDNA4, wave64): the bounded dual simplex with a
// long-step (bound-flipping) ratio test and an objective cutoff.
//
// The representation and the mould are those of lpx_bounded_dual.hip (ub, flip, lo beside the tableau; 1 workgroup x 1024 lanes;
// w and the ratios share 4096 doubles of LDS, or the handle's scratch `ws` beyond that).  The arithmetic contract is in
// include/lpx.h ("long-step ratio test, objective cutoff and dual start"); DESIGN.md section 4.16 has the launch shape.  Built
// with -ffp-contract=off.
//
// One launch decides ONE pivot and every pass in front of it:
//   CUTOFF: T[m,Cm] <= *B.cutoff (a device double on the handle: a driver moves it without a new parameter record) -> LPX_CUTOFF
//   w_i of every row into `buf`                                -> r  (block_first_min_below)
//   kind 1: row r is complemented IN PLACE, before anything else reads it: a pass subtracts from T[r,Cm], and
//           ub[p] - (b - x) and (ub[p] - b) + x round differently
//   column ratios of row r into `buf`, once                    -> q  (rs_hysteresis)
//   LONG_STEP: while ub[q] is finite and T[r,Cm] - ub[q] * T[r,q] is still below -eps, column q PASSES -- the in-kernel bound
//           flip of lpx_bounded_select (RHS column and column q, R elements each, rhsbuf kept current), its ratio set to +inf,
//           and the pick is repeated over the same ratio array.  A column passes at most once: at most Cm trips.
//   pivot prep after the last pass (column snapshot -> pcol, row r normalised -> prow and T[r,:]); the rank-1 update is the
//   lpx_update launch that follows.
// There is no wait on another workgroup anywhere; every loop is bounded by R or Cm.
#include "lpx_resident.h"      // rs_hysteresis (also pulls in lpx_block.h)

namespace lpx {

static constexpr int BDL_LDS_DOUBLES = 4096;

template <bool SKIP_FIXED, bool LONG_STEP, bool CUTOFF>
__global__ __launch_bounds__(SEL_NT) void lpx_bounded_long_select(BndParams B)
{
    __shared__ double s_buf[BDL_LDS_DOUBLES];
    __shared__ int s_out;
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];

    const SelParams& P = B.P;
    DevState* st = P.st;
    if (st->status != LPX_RUNNING) return;              // uniform: loop already finished

    const int t = threadIdx.x;
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    const int m = R - 1;
    const int rhs = C - 1;
    const size_t ld = (size_t)P.ld;
    double* T = P.T;
    double* rhsb = P.rhsbuf;                            // contiguous copy of the RHS column: every write of T[:,rhs] goes here too
    double* wbuf = (m <= BDL_LDS_DOUBLES) ? s_buf : P.ws;
    double* ratios = (rhs <= BDL_LDS_DOUBLES) ? s_buf : P.ws;
    const double inf = __builtin_inf();

    int iter = st->iter;                                // events so far (passes and pivots alike)
    if (iter >= P.max_iter) {
        if (t == 0) { st->status = LPX_ITER_LIMIT; st->r = -1; st->q = -1; }
        return;
    }
    if constexpr (CUTOFF) {
        if (T[(size_t)m * ld + rhs] <= *B.cutoff) {     // two broadcast loads; nothing is touched, no event
            if (t == 0) { st->status = LPX_CUTOFF; st->r = -1; st->q = -1; }
            return;
        }
    }

    // ---- leaving row, as lpx_bounded_dual_select
    for (int i = t; i < m; i += SEL_NT) {
        const double b = rhsb[i];
        const int pb = P.basis[i];
        const double u = (unsigned)pb < (unsigned)rhs ? B.ub[pb] : inf;
        double w = inf;
        if (b < -P.eps) w = b;
        else if (u < inf) w = u - b;
        wbuf[i] = w;
    }
    __syncthreads();
    const int r = block_first_min_below(wbuf, 1, m, P.eps, s_v, s_i);    // every lane is past its reads of wbuf on return
    if (r < 0) {
        if (t == 0) { st->status = LPX_OPTIMAL; st->r = -1; st->q = -1; }
        return;
    }
    const int kind = rhsb[r] < -P.eps ? 0 : 1;          // one address for the whole workgroup: a broadcast load
    const int p = P.basis[r];
    double* trow = T + (size_t)r * ld;

    // ---- kind 1: the complement of row r, materialised (every entry but the basic column's 1.0 negated, RHS = ub[p] - RHS)
    if (kind) {
        const double up = B.ub[p];
        __syncthreads();                                // uniform: every lane read the same rhsb[r] for `kind`, and has read it before it is rewritten
        for (int j = t; j < C; j += SEL_NT) {
            const double v = trow[j];
            const double n = (j == rhs) ? up - v : (j == p ? v : -v);
            trow[j] = n;
            if (j == rhs) rhsb[r] = n;
        }
        if (t == 0) B.flip[p] ^= 1;
    }

    // ---- the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
    {
        const double* zrow = T + (size_t)m * ld;
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
            const double nb = rhsb[r] - prod;
            if (!(nb < -P.eps)) break;
            __syncthreads();                            // trow[q] and rhsb[r] read by every lane before the rewrite
            for (int i = t; i < R; i += SEL_NT) {
                const double a = T[(size_t)i * ld + q];
                const double ni = rhsb[i] - uq * a;
                T[(size_t)i * ld + rhs] = ni;
                rhsb[i] = ni;
                T[(size_t)i * ld + q] = -a;
            }
            if (t == 0) {
                B.flip[q] ^= 1;
                if (iter < P.trace_cap) { P.trace[2 * iter] = -1; P.trace[2 * iter + 1] = q; }
                ratios[q] = inf;
            }
            ++iter;
            __syncthreads();                            // the next pick reads what this pass wrote
            q = rs_hysteresis(rhs, P.tol_dual, ratios, s_v, s_i, &s_out);
        }
    }
    if (q < 0) {
        // no entering column: the LP is infeasible.  The complement and the passes stay applied (a valid representation).
        if (t == 0) { st->status = LPX_INFEASIBLE; st->iter = iter; st->primal_count = iter; st->r = -1; st->q = -1; }
        return;
    }

    // ---- pivot prep on the row as it stands
    const double piv = trow[q];                         // broadcast load
    for (int i = t; i < R; i += SEL_NT)
        P.pcol[i] = (i == r) ? 0.0 : T[(size_t)i * ld + q];
    __syncthreads();                                   // pivot, basis[r] and column read before anything is rewritten
    for (int j = t; j < C; j += SEL_NT) {
        const double n = trow[j] / piv;
        trow[j] = n;
        P.prow[j] = n;
        if (j == rhs) rhsb[r] = n;                     // lpx_update leaves row r alone
    }
    if (t == 0) {
        P.basis[r] = q;
        if (iter < P.trace_cap) { P.trace[2 * iter] = kind ? -2 - r : r; P.trace[2 * iter + 1] = q; }
        st->iter = iter + 1; st->primal_count = iter + 1;
        st->r = r; st->q = q; st->qn = -1;
        if (kind) st->dual_iter += 1; else st->fdf_count += 1;      // per-kind pivot counts; passes = events - both
    }
}

// b.dual = LPX_BDUAL_FORM_BASE + flags, at least one of LONG_STEP (2) and CUTOFF (4) set
hipError_t launch_bounded_long_select(const BndParams& b, hipStream_t s)
{
    switch (b.dual - BDUAL_FORM_BASE) {
    case 2: hipLaunchKernelGGL((lpx_bounded_long_select<false, true, false>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    case 3: hipLaunchKernelGGL((lpx_bounded_long_select<true, true, false>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    case 4: hipLaunchKernelGGL((lpx_bounded_long_select<false, false, true>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    case 5: hipLaunchKernelGGL((lpx_bounded_long_select<true, false, true>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    case 6: hipLaunchKernelGGL((lpx_bounded_long_select<false, true, true>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    case 7: hipLaunchKernelGGL((lpx_bounded_long_select<true, true, true>), dim3(1), dim3(SEL_NT), 0, s, b); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace lpx
