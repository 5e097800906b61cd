// lpx_bounded_dual.hip -- the dual side of the bounded-variable simplex, gfx950 (CDNA4, wave64): the select kernel of
// lpx_bounded_dual_run and the two kernels of lpx_tableau_change_bounds.
//
// The representation is the one of lpx_bounded.hip: ub[j] in [0, +inf] and flip[j] beside the tableau, plus the lower shift
// lo[j] (internal column j stands for x_j - lo[j], or ub[j] - (x_j - lo[j]) when flipped).  The arithmetic contract is in
// include/lpx.h ("bounded dual simplex"); DESIGN.md section 4.14 has the launch shape.  Built with -ffp-contract=off.
//
// One launch of lpx_bounded_dual_select (1 workgroup x 1024 lanes, the mould of lpx_bounded_select) decides ONE event:
//   w_i of every row into `buf` (LDS, or global scratch)       -> r  (block_first_min_below: first strict minimum below -eps)
//   kind 1 (the basic variable of row r is above its bound): row r is complemented, on the fly
//   column ratios of the (complemented) row r into `buf`        -> q  (rs_hysteresis: the exact chain of lpx_select's dual loop)
//   pivot prep (column snapshot -> pcol, row r complemented and normalised -> prow and T[r,:]); the rank-1 update is the
//   lpx_update launch that follows.
// w and the ratios are never alive together, so they share one array: 4096 doubles of LDS, and the handle's scratch `ws` for
// whichever of them is longer than that.
#include "lpx_resident.h"      // rs_hysteresis (also pulls in lpx_block.h)

namespace lpx {

static constexpr int BDD_LDS_DOUBLES = 4096;

// SKIP_FIXED (lpx_bounded_dual_run2 with LPX_BDUAL_SKIP_FIXED): a column with ub[j] == 0 does not enter.  The unflagged
// instantiation is the kernel of lpx_bounded_dual_run, unchanged.
template <bool SKIP_FIXED>
__global__ __launch_bounds__(SEL_NT) void lpx_bounded_dual_select(BndParams B)
{
    __shared__ double s_buf[BDD_LDS_DOUBLES];
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
    double* rhsb = P.rhsbuf;                            // contiguous copy of the RHS column, kept current by lpx_update
    double* wbuf = (m <= BDD_LDS_DOUBLES) ? s_buf : P.ws;
    double* ratios = (rhs <= BDD_LDS_DOUBLES) ? s_buf : P.ws;
    const double inf = __builtin_inf();

    const int iter = st->iter;                          // events so far
    if (iter >= P.max_iter) {
        if (t == 0) { st->status = LPX_ITER_LIMIT; st->r = -1; st->q = -1; }
        return;
    }

    // ---- leaving row: infeasibility of every row, below zero (kind 0) or above the basic variable's bound (kind 1)
    for (int i = t; i < m; i += SEL_NT) {
        const double b = rhsb[i];
        const int pb = P.basis[i];
        const double u = (unsigned)pb < (unsigned)rhs ? B.ub[pb] : inf;   // gather from a small array: L2
        double w = inf;                                                  // the row does not take part
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

    // ---- entering column over row r.  kind 1: the row is complemented first -- every entry but the basic column's 1.0
    // negated, RHS = ub[p] - RHS.  Negation is exact, so it is applied on the fly in front of the division.
    {
        const double* zrow = T + (size_t)m * ld;
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
    const double up = kind ? B.ub[p] : 0.0;
    if (q < 0) {
        // no entering column: the LP is infeasible.  The complement of a kind-1 row stays applied (a valid representation).
        if (kind) {
            for (int j = t; j < C; j += SEL_NT) {
                const double v = trow[j];
                const double n = (j == rhs) ? up - v : (j == p ? v : -v);
                trow[j] = n;
                if (j == rhs) rhsb[r] = n;
            }
        }
        if (t == 0) {
            if (kind) B.flip[p] ^= 1;
            st->status = LPX_INFEASIBLE; st->r = -1; st->q = -1;
        }
        return;
    }

    // ---- pivot prep, as lpx_bounded_select: the complement in front of the division
    const double a = trow[q];                           // broadcast load
    const double piv = kind ? -a : a;
    for (int i = t; i < R; i += SEL_NT)
        P.pcol[i] = (i == r) ? 0.0 : T[(size_t)i * ld + q];
    __syncthreads();                                   // pivot, basis[r] and column read before anything is rewritten
    for (int j = t; j < C; j += SEL_NT) {
        double v = trow[j];
        if (kind) v = (j == rhs) ? up - v : (j == p ? v : -v);
        const double n = v / piv;
        trow[j] = n;
        P.prow[j] = n;
        if (j == rhs) rhsb[r] = n;                     // lpx_update leaves row r alone
    }
    if (t == 0) {
        if (kind) B.flip[p] ^= 1;
        P.basis[r] = q;
        if (iter < P.trace_cap) { P.trace[2 * iter] = kind ? -2 - r : r; P.trace[2 * iter + 1] = q; }
        st->iter = iter + 1; st->primal_count = iter + 1;
        st->r = r; st->q = q; st->qn = -1;
        if (kind) st->dual_iter += 1; else st->fdf_count += 1;      // per-kind event counts (lpx_bounded_counts)
    }
}

hipError_t launch_bounded_dual_select(const BndParams& b, hipStream_t s)
{
    if (b.dual == 2) hipLaunchKernelGGL(lpx_bounded_dual_select<true>, dim3(1), dim3(SEL_NT), 0, s, b);
    else hipLaunchKernelGGL(lpx_bounded_dual_select<false>, dim3(1), dim3(SEL_NT), 0, s, b);
    return hipGetLastError();
}

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
