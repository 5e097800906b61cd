// lpx_bounded.hip -- select kernel of the bounded-variable (upper-bounding) primal simplex, gfx950 (CDNA4, wave64).
//
// Every column j < C-1 has an upper bound ub[j] in [0, +inf] kept BESIDE the tableau and a one-byte state flip[j]: flip[j] = 1
// means that column j currently stands for u_j - x_j.  The arithmetic contract is in include/lpx.h ("bounded-variable primal
// simplex"); DESIGN.md section 4.13 has the launch shape.  Built with -ffp-contract=off like the rest of the library.
//
// One launch of lpx_bounded_select (1 workgroup x 1024 lanes, the mould of lpx_select in lpx_kernels.hip) runs events until one
// of them is a pivot or the loop ends:
//   ChooseEntering over the objective row                                   -> q
//   three-way ratio of every row into `ratios` (LDS, or global scratch)     -> r, best      (rs_hysteresis: the exact chain)
//   ub[q] <= best: bound flip -- RHS column and column q, R elements each, then the NEXT event in the same launch
//   else: pivot prep (column snapshot -> pcol, row r complemented when its basic variable leaves at its upper bound,
//         normalised -> prow and T[r,:]), and the launch ends; the rank-1 update is the lpx_update launch that follows.
// A launch that ends on a flip (iteration cap, optimum, unbounded column) leaves st->r = -1 or a final status, which lpx_update
// reads first and returns on.
#include "lpx_resident.h"      // rs_hysteresis (also pulls in lpx_block.h)

namespace lpx {

// ratios held in LDS up to this many rows; longer tableaux keep them in the handle's global scratch `ws` (they stay in L2)
static constexpr int BND_LDS_DOUBLES = 4096;

__global__ __launch_bounds__(SEL_NT) void lpx_bounded_select(BndParams B)
{
    __shared__ double s_ratio[BND_LDS_DOUBLES];
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
    double* ratios = (m <= BND_LDS_DOUBLES) ? s_ratio : P.ws;
    const double inf = __builtin_inf();

    int iter = st->iter;                                // events so far (flips and pivots alike)
    int r = -1, q = -1;
    int final_status = LPX_RUNNING;

    for (;;) {
        if (iter >= P.max_iter) { final_status = LPX_ITER_LIMIT; break; }
        // a flip of this launch rewrote T[m,q]: its barrier (below) ordered that store before these loads
        q = block_first_min_below(T + (size_t)m * ld, 1, rhs, P.eps, s_v, s_i);
        if (q < 0) { final_status = LPX_OPTIMAL; break; }
        for (int i = t; i < m; i += SEL_NT) {
            const double a = T[(size_t)i * ld + q];
            const double b = rhsb[i];
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
            // bound flip (ties go to it): x_q runs to its other bound, no other column moves
            for (int i = t; i < R; i += SEL_NT) {
                const double a = T[(size_t)i * ld + q];
                const double nb = rhsb[i] - uq * a;     // mul, then sub: contraction is off
                T[(size_t)i * ld + rhs] = nb;
                rhsb[i] = nb;
                T[(size_t)i * ld + q] = -a;
            }
            if (t == 0) {
                B.flip[q] ^= 1;
                if (iter < P.trace_cap) { P.trace[2 * iter] = -1; P.trace[2 * iter + 1] = q; }
            }
            ++iter;
            r = -1;
            __syncthreads();                            // the next event reads what this one wrote (objective row, RHS, ratios reuse)
            continue;
        }
        if (r < 0) { q = -1; final_status = LPX_UNBOUNDED; }
        break;
    }

    if (final_status != LPX_RUNNING) {
        if (t == 0) { st->status = final_status; st->iter = iter; st->primal_count = iter; st->r = -1; st->q = -1; }
        return;
    }

    // ---- pivot prep.  kind 1 (T[r,q] < -eps): row r is complemented first -- every entry but the basic column's 1.0 negated,
    // RHS = ub[p] - RHS -- so that its basic variable p leaves at its upper bound as u_p - x_p = 0.  Negation is exact, so the
    // complement is applied on the fly in front of the division: same bits as complementing the row and then normalising it.
    const double a = T[(size_t)r * ld + q];            // one address for the whole workgroup: a broadcast load
    const int kind = a > P.eps ? 0 : 1;
    const int p = P.basis[r];
    const double up = kind ? B.ub[p] : 0.0;
    const double piv = kind ? -a : a;
    for (int i = t; i < R; i += SEL_NT)
        P.pcol[i] = (i == r) ? 0.0 : T[(size_t)i * ld + q];
    __syncthreads();                                   // pivot, basis[r] and column read before anything is rewritten
    double* trow = T + (size_t)r * ld;
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
        if (kind) st->dual_iter += 1; else st->fdf_count += 1;      // per-kind pivot counts (lpx_bounded_counts)
    }
}

hipError_t launch_bounded_select(const BndParams& b, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_bounded_select, dim3(1), dim3(SEL_NT), 0, s, b);
    return hipGetLastError();
}

}  // namespace lpx
