// lpx_bounded.hip -- select kernel of the bounded-variable (upper-bounding) primal simplex, gfx950 (CDNA4, wave64).  It decides
// the entering column, the three-way ratio of every row, and between a bound flip and a pivot; the flip, the complement and
// the pivot prep themselves are the shared pieces of lpx_bounded.h.
//
// Every column j < C-1 has an upper bound ub[j] in [0, +inf] kept BESIDE the tableau and a one-byte state flip[j]: flip[j] = 1
// means that column j currently stands for u_j - x_j.  The arithmetic contract is in include/lpx.h ("bounded-variable primal
// simplex"); DESIGN.md section 4.13 has the launch shape.  Built with -ffp-contract=off like the rest of the library.
//
// One launch of lpx_bounded_select (1 workgroup x 1024 lanes, like lpx_select in lpx_kernels.hip) runs events until one of them
// is a pivot or the loop ends:
//   ChooseEntering over the objective row                                   -> q
//   three-way ratio of every row into `ratios` (LDS, or global scratch)     -> r, best      (rs_hysteresis: the exact chain)
//   ub[q] <= best: bound flip (bnd_flip_column), then the NEXT event in the same launch
//   else: pivot prep (bnd_pivot_prep; row r complemented on the fly when its basic variable leaves at its upper bound), and
//         the launch ends; the rank-1 update is the lpx_update launch that follows.
// A launch that ends on a flip (iteration cap, optimum, unbounded column) leaves st->r = -1 or a final status, which lpx_update
// reads first and returns on.
#include "lpx_bounded.h"       // the pieces shared with the dual kernels: view, exit, bound flip, pivot prep

namespace lpx {

__global__ __launch_bounds__(SEL_NT) void lpx_bounded_select(BndParams B)
{
    __shared__ double s_ratio[BND_LDS_DOUBLES];
    __shared__ int s_out;
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];

    const SelParams& P = B.P;
    DevState* st = P.st;
    if (st->status != LPX_RUNNING) return;              // uniform: loop already finished

    const BndView V(P);
    const int t = V.t, m = V.m, rhs = V.rhs;
    double* ratios = bnd_buf(m, s_ratio, P.ws);
    const double inf = __builtin_inf();

    int iter = st->iter;                                // events so far (flips and pivots alike)
    int r = -1, q = -1;
    int final_status = LPX_RUNNING;

    for (;;) {
        if (iter >= P.max_iter) { final_status = LPX_ITER_LIMIT; break; }
        // a flip of this launch rewrote T[m,q]: its barrier (below) ordered that store before these loads
        q = block_first_min_below(V.row(m), 1, rhs, P.eps, s_v, s_i);
        if (q < 0) { final_status = LPX_OPTIMAL; break; }
        for (int i = t; i < m; i += SEL_NT) {
            const double a = V.T[(size_t)i * V.ld + q];
            const double b = V.rhsb[i];
            const int pb = P.basis[i];
            const double u = (unsigned)pb < (unsigned)rhs ? B.ub[pb] : inf;   // gather from a small array: L2
            double rho = inf;
            if (a > P.eps) rho = b / a;                                  // basic variable goes to zero
            else if (a < -P.eps && u < inf) rho = (u - b) / (-a);        // basic variable goes to its upper bound
            ratios[i] = rho;
        }
        __syncthreads();
        r = rs_hysteresis(m, P.tol_primal, ratios, s_v, s_i, &s_out);
        const double best = r >= 0 ? ratios[r] : inf;
        const double uq = B.ub[q];
        if (uq < inf && uq <= best) {
            bnd_flip_column(V, B, q, uq, iter);         // ties go to the flip
            ++iter;
            r = -1;
            __syncthreads();                            // the next event reads what this one wrote (objective row, RHS, ratios reuse)
            continue;
        }
        if (r < 0) { q = -1; final_status = LPX_UNBOUNDED; }
        break;
    }

    if (final_status != LPX_RUNNING) {
        if (t == 0) { st->iter = iter; st->primal_count = iter; }
        bnd_exit(st, t, final_status);
        return;
    }

    // kind 1 (T[r,q] < -eps): the basic variable p of row r leaves at its upper bound, as u_p - x_p = 0
    const int kind = V.row(r)[q] > P.eps ? 0 : 1;       // one address for the whole workgroup: a broadcast load
    bnd_pivot_prep(V, B, r, q, P.basis[r], iter, kind, kind);
}

hipError_t launch_bounded_select(const BndParams& b, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_bounded_select, dim3(1), dim3(SEL_NT), 0, s, b);
    return hipGetLastError();
}

}  // namespace lpx
