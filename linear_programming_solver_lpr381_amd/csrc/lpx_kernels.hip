// lpx_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the dense-tableau simplex loop: the two-launch paths.
// (One launch per pivot: lpx_pivot_fused.hip; the group step: lpx_group_fused.hip; node assembly: lpx_nodes.hip.)
//
// Built with -ffp-contract=off: `t - f*p` must round twice (v_mul_f64 + v_add_f64), exactly as the
// reference's scalar C# does (Models/PrimalSimplex.cs:255); pivot-row normalisation uses true IEEE
// division (Models/PrimalSimplex.cs:250), never a reciprocal multiply.
//
// Two launches per pivot on one stream:
//   lpx_select  (1 workgroup x 1024 lanes)  ChooseEntering + ChooseLeaving + pivot prep
//   lpx_update  (>> 256 workgroups)         rank-1 update of the whole tableau, HBM-bound
#include "lpx_resident.h"      // rs_hysteresis: the hysteresis scan over ratios held in LDS (also pulls in lpx_block.h)
#include "lpx_scan.h"
#include "lpx_tile.h"

namespace lpx {

// ------------------------------------------------------------------------------------------------
// lpx_select: one workgroup decides the next pivot and prepares the update's operands.
// ------------------------------------------------------------------------------------------------
// The two ratio scans of the dual path as real calls: inlined three times (one per phase) their 16-ratio register blocks pushed
// the 1024-lane kernel (128 VGPRs per lane) into scratch spills -- 13 in lpx_select, 22 in lpx_select_b (code-object metadata).
__device__ __attribute__((noinline)) int sel_row_scan(int m, double tol, const double* col, size_t cs, const double* rhsb, double eps, int* s_out)
{
    return block_hysteresis_auto<SEL_NW>(m, tol, RowRatio{col, cs, rhsb, 1, eps}, s_out);
}
__device__ __attribute__((noinline)) int sel_col_scan(int L, double tol, const double* lrow, const double* zrow, double eps, int* s_out)
{
    return block_hysteresis_auto<SEL_NW>(L, tol, DualColRatio{lrow, zrow, eps}, s_out);
}

// `ratios`: dynamic LDS for max(m, C-1) doubles, or nullptr when the tableau is too long for it (then the scans read their
// operands from global memory on one wave, as in round 1).  With it, ALL 1024 lanes gather the operands and divide in
// parallel (one round trip, ~1 division per lane), and the chain runs over LDS: minimum + band count on four waves, exact
// replay on wave 0 only when rows tie (rs_hysteresis, lpx_resident.h -- the scan the resident kernels use, bit-identical).
__device__ __forceinline__ void lpx_select_body(const SelParams& P, double* ratios)
{
    __shared__ int s_out;
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];

    DevState* st = P.st;
    if (st->status != LPX_RUNNING) return;              // uniform: loop already finished

    const int t = threadIdx.x;
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    const int m = R - 1;
    const int rhs = C - 1;
    const size_t ld = (size_t)P.ld;
    double* T = P.T;
    // contiguous copy of the RHS column: filled once per run by lpx_rhs_init, kept current by lpx_update (rows i != r)
    // and by this kernel (row r) -- the dual loop's leaving-row scan and every ratio test read it instead of a strided column
    const double* rhsb = P.rhsbuf;

    int phase = st->phase;
    const int fdf_count = st->fdf_count, dual_iter = st->dual_iter, primal_count = st->primal_count;
    const int iter = st->iter;
    int r = -1, q = -1;
    int final_status = LPX_RUNNING;

    {
        // state machine: ForceDualFeasibility -> dual loop -> (repaired mode) primal clean-up
        for (int hop = 0; hop < 3 && final_status == LPX_RUNNING && r < 0; ++hop) {
            if (phase == 0) {
                // ForceDualFeasibility, Models/DualSimplex.cs:195-228
                if (fdf_count >= P.fdf_guard) { phase = 1; continue; }
                q = block_first_min_below(T + (size_t)m * ld, 1, rhs, P.eps, s_v, s_i);
                if (q < 0) { phase = 1; continue; }
                if (ratios) {
                    for (int i = t; i < m; i += SEL_NT) { const double a = T[(size_t)i * ld + q]; ratios[i] = a > P.eps ? rhsb[i] / a : __builtin_inf(); }
                    __syncthreads();
                    r = rs_hysteresis(m, P.tol_fdf, ratios, s_v, s_i, &s_out);
                } else
                r = sel_row_scan(m, P.tol_fdf, T + q, ld, rhsb, P.eps, &s_out);
                if (r < 0) { q = -1; phase = 1; continue; }
            } else if (phase == 1) {
                // dual loop, Models/DualSimplex.cs:36-113
                if (dual_iter >= P.max_iter) { final_status = LPX_ITER_LIMIT; break; }
                r = block_first_min_below(rhsb, 1, m, P.eps, s_v, s_i);
                if (r < 0) {
                    if (P.cleanup) {
                        int qe = block_first_min_below(T + (size_t)m * ld, 1, rhs, P.eps, s_v, s_i);
                        if (qe >= 0) { phase = 2; continue; }
                    }
                    final_status = LPX_OPTIMAL; break;
                }
                if (ratios) {
                    const double* lrow = T + (size_t)r * ld; const double* zrow = T + (size_t)m * ld;
                    for (int j = t; j < rhs; j += SEL_NT) { const double a = lrow[j]; ratios[j] = a < -P.eps ? zrow[j] / (-a) : __builtin_inf(); }
                    __syncthreads();
                    q = rs_hysteresis(rhs, P.tol_dual, ratios, s_v, s_i, &s_out);
                } else
                q = sel_col_scan(rhs, P.tol_dual, T + (size_t)r * ld, T + (size_t)m * ld, P.eps, &s_out);
                if (q < 0) { r = -1; final_status = LPX_INFEASIBLE; break; }
            } else {
                // primal loop, Models/PrimalSimplex.cs:92-124
                if (primal_count >= P.max_iter - dual_iter) { final_status = LPX_ITER_LIMIT; break; }
                q = block_first_min_below(T + (size_t)m * ld, 1, rhs, P.eps, s_v, s_i);
                if (q < 0) { final_status = LPX_OPTIMAL; break; }
                if (ratios) {
                    for (int i = t; i < m; i += SEL_NT) { const double a = T[(size_t)i * ld + q]; ratios[i] = a > P.eps ? rhsb[i] / a : __builtin_inf(); }
                    __syncthreads();
                    r = rs_hysteresis(m, P.tol_primal, ratios, s_v, s_i, &s_out);
                } else
                r = sel_row_scan(m, P.tol_primal, T + q, ld, rhsb, P.eps, &s_out);
                if (r < 0) { q = -1; final_status = LPX_UNBOUNDED; break; }
            }
        }
    }

    if (final_status != LPX_RUNNING || r < 0) {
        if (t == 0) {
            st->status = (final_status == LPX_RUNNING) ? LPX_OPTIMAL : final_status;
            st->phase = phase; st->r = -1; st->q = -1;
        }
        return;
    }

    // ---- pivot prep (Models/PrimalSimplex.cs:249-250, :254): snapshot the pivot column, normalise
    // the pivot row in place and into `prow` so the update kernel never reads what it overwrites.
    const double piv = T[(size_t)r * ld + q];          // one address for the whole workgroup: a broadcast load
    for (int i = t; i < R; i += SEL_NT)
        P.pcol[i] = (i == r) ? 0.0 : T[(size_t)i * ld + q];
    __syncthreads();                                   // pivot and column read before the row is rewritten
    double* trow = T + (size_t)r * ld;
    for (int j = t; j < C; j += SEL_NT) {
        double p = trow[j] / piv;
        trow[j] = p;
        P.prow[j] = p;
        if (j == rhs) P.rhsbuf[r] = p;                 // lpx_update leaves row r alone
    }
    if (t == 0) {
        P.basis[r] = q;                                // basis[leaving] = entering, :110
        if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = q; }
        st->iter = iter + 1;
        st->r = r; st->q = q; st->phase = phase; st->qn = -1;
        if (phase == 0) st->fdf_count = fdf_count + 1;
        else if (phase == 1) st->dual_iter = dual_iter + 1;
        else st->primal_count = primal_count + 1;
    }
}

// contiguous copy of the RHS column, once at the start of a dual run (single and batched)
__device__ __forceinline__ void lpx_rhs_init_body(const SelParams& P)
{
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    for (int i = threadIdx.x; i < R; i += SEL_NT) P.rhsbuf[i] = P.T[(size_t)i * P.ld + (C - 1)];
}

// ------------------------------------------------------------------------------------------------
// Lookahead select (primal and forced-pivot paths).
//
// The gather-based select above spends most of its time in 64-cache-lines-per-instruction strided
// column reads on ONE CU.  Here the update kernel of pivot k writes, as by-products of the stream it
// already does, the column that pivot k+1 will enter on (`coln`) and the RHS column (`rhsbuf`), both
// contiguous.  That is possible because the entering column of pivot k+1 depends only on the
// objective row AFTER pivot k, which select(k) can compute itself (obj - f_m * prow, the very
// arithmetic the update kernel will repeat bit for bit).  So select(k):
//   ratio test on contiguous colc/rhsbuf  ->  r
//   normalise row r (contiguous)          ->  prow, T[r,:]
//   updated scan row u = T[s,:] - colc[s]*prow  ->  next entering column qn   (s = objective row;
//   forced mode: s = next forced row, rule = first |u| >= thresh from the next forced column)
// Column buffers ping-pong on pivot parity: update(k) reads colc as factors while writing coln.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lpx_la_init_body(const SelParams& P)
{
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];
    DevState* st = P.st;
    if (st->status != LPX_RUNNING) return;
    const int iter = st->iter;
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    double* colc = (iter & 1) ? P.col1 : P.col0;
    ScanRule rule; rule.forced = (P.mode == MODE_FORCED); rule.eps = P.eps; rule.thresh = P.fthresh;
    rule.C = C; rule.c0 = 0;
    int scanrow = R - 1;
    if (rule.forced) {
        const int k = st->forced_k;
        scanrow = k < P.fcount ? P.frows[k] : -1;
        rule.c0 = k < P.fcount ? P.fcols[k] : 0;
    }
    int qn = la_prepare_from_T(P, R, C, colc, scanrow, rule, s_v, s_i);
    if (threadIdx.x == 0) {
        st->qn = qn;
        if (P.us) { *P.us = *st; P.us->qn = qn; P.part_i[MB_CNT] = 0; }
    }
}

__global__ __launch_bounds__(SEL_NT) void lpx_select_la(SelParams P)
{
    __shared__ int s_out;
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];

    DevState* st = P.st;
    LPX_STAMP_BEGIN
    if (st->status != LPX_RUNNING) return;
    LPX_STAMP(0);

    const int t = threadIdx.x;
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    const int m = R - 1;
    const size_t ld = (size_t)P.ld;
    double* T = P.T;
    const int iter = st->iter;
    const int primal_count = st->primal_count;
    double* colc = (iter & 1) ? P.col1 : P.col0;     // column q of the current tableau
    double* coln = (iter & 1) ? P.col0 : P.col1;     // receives column qn of the next one
    const int q = st->qn;
    int r = -1, scanrow = -1;
    int final_status = LPX_RUNNING;
    ScanRule rule; rule.forced = (P.mode == MODE_FORCED); rule.eps = P.eps; rule.thresh = P.fthresh;
    rule.C = C; rule.c0 = 0;

    if (rule.forced) {
        const int k = st->forced_k;
        if (k >= P.fcount) {
            final_status = LPX_OPTIMAL;
        } else {
            r = P.frows[k];
            scanrow = (k + 1 < P.fcount) ? P.frows[k + 1] : -1;
            rule.c0 = (k + 1 < P.fcount) ? P.fcols[k + 1] : 0;
            if (t == 0) { P.fchosen[k] = q; st->forced_k = k + 1; }
            if (q < 0) {                                  // no eligible column: skip this pivot
                int qn = la_prepare_from_T(P, R, C, colc, scanrow, rule, s_v, s_i);
                if (t == 0) { st->r = -1; st->q = -1; st->qn = qn; }
                return;
            }
        }
    } else {
        // primal loop head, Models/PrimalSimplex.cs:95-106
        if (primal_count >= P.max_iter) final_status = LPX_ITER_LIMIT;
        else if (q < 0) final_status = LPX_OPTIMAL;
        else {
            r = block_hysteresis_argmin(m, P.tol_primal, RowRatio{colc, 1, P.rhsbuf, 1, P.eps}, &s_out);
            if (r < 0) final_status = LPX_UNBOUNDED;
            scanrow = m;
        }
    }
    LPX_STAMP(1);
    if (final_status != LPX_RUNNING) {
        if (t == 0) { st->status = final_status; st->r = -1; st->q = -1; }
        return;
    }

    // Pivot prep (Models/PrimalSimplex.cs:249-250) fused with the lookahead scan of the updated row.
    const double piv = colc[r];
    const bool same = (scanrow == r);
    const double fs = (scanrow >= 0 && !same) ? colc[scanrow] : 0.0;
    double* trow = T + (size_t)r * ld;
    const double* srow = T + (size_t)(scanrow >= 0 ? scanrow : 0) * ld;
    MinIdx best; rule_init(rule, best);
    for (int j = t; j < C; j += SEL_NT) {
        const double p = trow[j] / piv;
        trow[j] = p;
        P.prow[j] = p;
        if (scanrow >= 0) {
            const double u = same ? p : srow[j] - fs * p;     // what lpx_update will store at T[s,j]
            rule_feed(rule, best, j, u);
        }
    }
    LPX_STAMP(2);
    best = block_min_idx(best, s_v, s_i);                     // barrier inside: prow is complete
    LPX_STAMP(3);
    const int qn = (scanrow >= 0) ? rule_decode(rule, best) : -1;
    if (t == 0) {
        if (qn >= 0) coln[r] = P.prow[qn];                    // row r is not touched by lpx_update
        P.rhsbuf[r] = P.prow[C - 1];
        if (!rule.forced) P.basis[r] = q;                     // basis[leaving] = entering, :110
        if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = q; }
        st->iter = iter + 1;
        st->r = r; st->q = q; st->qn = qn;
        if (!rule.forced) st->primal_count = primal_count + 1;
    }
    LPX_STAMP(4);
    LPX_STAMP_END;
}

// ------------------------------------------------------------------------------------------------
// lpx_update: T[i, :] -= pcol[i] * prow[:] for every row i != r  (Models/PrimalSimplex.cs:251-256,
// Models/DualSimplex.cs:240-245).  HBM-bound: 16 bytes of traffic per element, 2 flop.
//
// Work unit = one wave x (128 columns x UPD_ROWS rows): each lane owns two adjacent doubles
// (one 16-byte global_load_dwordx4 / global_store_dwordx4 per row, 1 KiB contiguous per wave per
// row), keeps its slice of the normalised pivot row in registers, takes the row factor from a
// scalar load, and has UPD_ROWS independent loads in flight.  Units are flattened over
// (row block, column chunk) so ragged widths waste at most part of one wave per row block.
// ------------------------------------------------------------------------------------------------
// The in-place walker behind lpx_update* and lpx_update_mb*: unit -> tile, the straight-line tile for almost every wave,
// row by row for the rest.  MB: the multi-workgroup protocol captures row r too (it already holds the normalised pivot row, so
// nxt[r] and rhsbuf[r] are written); without it row r is skipped ENTIRELY (lpx_bounded.hip, the dual select and the revised
// path's exact inverse rely on that) and rhsbuf may be null (the exact inverse has no RHS column to capture).
// `lane` comes from the header: lpx_update_mb_body has it for its reduction, and taking it from there keeps that kernel's code.
// POLICY: 0 = default cache policy (tableau at home in the Infinity Cache), 1 = nontemporal loads and stores, 2 =
// nontemporal loads, the wave's LAST row stored with the default policy and the others nontemporal (see UPDM in lpx_tile.h).
template <int ROWS, int NTH, int POLICY, bool MB>
__device__ __forceinline__ void upd_inplace_tiles(double* T, int ld, int R, int C, const double* prow, const double* fac, double* nxt,
                                                  double* rhsbuf, int r, int qn, int lane, int ncw, int nunits, int mixmod)
{
    constexpr bool NT = POLICY != 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.x * (NTH / 64) + wave;
    if (unit >= nunits) return;
    const int cw = unit % ncw;
    const int rb = unit / ncw;
    const int col = cw * 128 + lane * 2;
    if (col >= ld) return;                      // ld is a multiple of 16, so col+1 < ld too
    const int row0 = rb * ROWS;
    if (row0 >= R) return;                      // capacity-sized grid: rows beyond the live shape
    const double2 p = *reinterpret_cast<const double2*>(prow + col);
    double* base = T + (size_t)row0 * ld + col;
    const int c0 = cw * 128;
    const bool plain_wave = row0 + ROWS <= R && (r < row0 || r >= row0 + ROWS) &&
                            !(qn >= c0 && qn < c0 + 128) && !((MB || rhsbuf != nullptr) && C - 1 >= c0 && C - 1 < c0 + 128);
    if (NT && plain_wave) {
        upd_plain_tile<ROWS, NT, POLICY == 2 ? MIX_INPLACE : MIX_NONE>(base, base, (size_t)ld, p, fac, row0, rb, mixmod);
        return;
    }
    // every other wave -- and every wave of the cache-resident form (8 rows x 256 lanes, default policy), which measured
    // FASTER with the per-row branches (lpx_update_b 53 vs 74 us, config 2's update 9.1 vs 16.4 us): all loads, then per row
    const bool wq = (qn >= 0) && ((qn & ~1) == col);              // this lane owns column qn
    const bool wr = (MB || rhsbuf != nullptr) && (((C - 1) & ~1) == col);   // this lane owns the RHS column
    double2 v[ROWS];
    double f[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int i = row0 + k;
        if (i < R) {
            v[k] = upd_load<NT>(base + (size_t)k * ld);
            f[k] = fac[i];
        }
    }
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int i = row0 + k;
        if (i < R && (MB || i != r)) {
            double2 o;
            if (!MB || i != r) {
                o.x = v[k].x - f[k] * p.x;      // mul, then sub: contraction is off
                o.y = v[k].y - f[k] * p.y;
                upd_store<NT>(base + (size_t)k * ld, o);
            } else {
                o = p;                          // row r already holds the normalised pivot row
            }
            if (wq) nxt[i] = (qn & 1) ? o.y : o.x;
            if (wr) rhsbuf[i] = ((C - 1) & 1) ? o.y : o.x;
        }
    }
}

template <int ROWS = UPD_ROWS, int NTH = UPD_NT, int POLICY = 0>
__device__ __forceinline__ void lpx_update_body(double* __restrict__ T, int ld, int Rcap, int Ccap,
                                                const int32_t* __restrict__ shape,
                                                const double* __restrict__ prow,
                                                double* fac0, double* fac1,
                                                double* __restrict__ rhsbuf,
                                                const DevState* __restrict__ st,
                                                int ncw, int nunits, int mixmod = 1)
{
    if (st->status != LPX_RUNNING) return;
    const int r = st->r;
    if (r < 0) return;
    const int R = shape ? shape[0] : Rcap, C = shape ? shape[1] : Ccap;
    const int par = (st->iter - 1) & 1;                   // parity of the pivot being applied
    // fac: pivot column snapshot (factors); the other one takes the by-product, the next pivot's column
    upd_inplace_tiles<ROWS, NTH, POLICY, false>(T, ld, R, C, prow, par ? fac1 : fac0, par ? fac0 : fac1, rhsbuf, r, st->qn,
                                                threadIdx.x & 63, ncw, nunits, mixmod);
}

// ------------------------------------------------------------------------------------------------
// Multi-workgroup select (primal and forced paths).
//
// lpx_select_la above is one 1024-lane workgroup: ~9.5 us per pivot at 1025x3073, of which the
// barrier-heavy ratio scan is 4 us and the 3073 divisions plus the wait for the slowest wave another
// 4.6 us (in-kernel stamps, tools/diag_select_stamps.py).  Here `nblk` 256-lane workgroups run the
// same step: every workgroup repeats the ratio test (contiguous 8 B x 2 x m, L2-resident, identical
// result everywhere), then normalises ONE column slice of the pivot row, scans the same slice of the
// updated objective row and publishes a partial argmin; the workgroup that arrives last reduces the <= 128
// partials to the next entering column (one word the update kernel reads).
//
// Two state records break what would otherwise be intra-kernel races:
//   st  written by select workgroup 0, read by every update workgroup and by the host;
//   us  written by update workgroup 0, read by every select workgroup.
// Apart from the partials (agent-scope stores and loads around one agent-scope counter, see below) nothing is read
// and written by workgroups of the same launch; the kernel boundary orders the rest (cdna_hip_programming.md G16).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lpx_select_mb_body(const SelParams& P)
{
    __shared__ double s_v[MB_NT / 64];
    __shared__ int s_i[MB_NT / 64];

    const DevState* us = P.us;
    DevState* st = P.st;
    const int t = threadIdx.x, b = blockIdx.x;
    LPX_STAMP_BEGIN
    const int status_in = us->status;
    if (status_in != LPX_RUNNING) { if (b == 0 && t == 0) st->status = status_in; return; }

    LPX_STAMP_MB(0);
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    const int m = R - 1;
    const size_t ld = (size_t)P.ld;
    double* T = P.T;
    const int iter = us->iter;
    const int primal_count = us->primal_count;
    double* colc = (iter & 1) ? P.col1 : P.col0;     // column q of the current tableau
    const int q = us->qn;
    int r = -1, scanrow = -1;
    int final_status = LPX_RUNNING;
    ScanRule rule; rule.forced = (P.mode == MODE_FORCED); rule.eps = P.eps; rule.thresh = P.fthresh;
    rule.C = C; rule.c0 = 0;
    const int k = us->forced_k;

    if (rule.forced) {
        if (k >= P.fcount) {
            final_status = LPX_OPTIMAL;
        } else {
            r = P.frows[k];
            scanrow = (k + 1 < P.fcount) ? P.frows[k + 1] : -1;
            rule.c0 = (k + 1 < P.fcount) ? P.fcols[k + 1] : 0;
            if (q < 0) {                                  // no eligible column: skip this pivot
                if (b != 0) return;
                int qn = la_prepare_from_T<MB_NT>(P, R, C, colc, scanrow, rule, s_v, s_i);
                if (t == 0) {
                    P.fchosen[k] = -1;
                    st->status = LPX_RUNNING; st->iter = iter; st->r = -1; st->q = -1;
                    st->forced_k = k + 1; st->primal_count = primal_count;
                    st->qn = qn; st->qn_valid = 1; st->c0n = rule.c0;
                }
                return;
            }
        }
    } else {
        // primal loop head, Models/PrimalSimplex.cs:95-106
        if (primal_count >= P.max_iter) final_status = LPX_ITER_LIMIT;
        else if (q < 0) final_status = LPX_OPTIMAL;
        else {
            // every wave of every workgroup gets the same row: one wave each for m <= 1024 (no barrier), the segments of a
            // longer column spread over the workgroup's waves
            r = block_hysteresis_segments<MB_NT / 64>(m, P.tol_primal, RowRatio{colc, 1, P.rhsbuf, 1, P.eps});
            if (r < 0) final_status = LPX_UNBOUNDED;
            scanrow = m;
        }
    }
    LPX_STAMP_MB(1);
    if (final_status != LPX_RUNNING) {
        if (b == 0 && t == 0) { st->status = final_status; st->iter = iter; st->r = -1; st->q = -1; }
        return;
    }

    // this workgroup's column slice
    const int per = (C + P.nblk - 1) / P.nblk;
    const int j0 = b * per, j1 = min(C, j0 + per);
    const double piv = colc[r];
    const bool same = (scanrow == r);
    const double fs = (scanrow >= 0 && !same) ? colc[scanrow] : 0.0;
    double* trow = T + (size_t)r * ld;
    const double* srow = T + (size_t)(scanrow >= 0 ? scanrow : 0) * ld;
    MinIdx best; rule_init(rule, best);
    for (int j = j0 + t; j < j1; j += MB_NT) {
        const double p = trow[j] / piv;                       // true division, :250
        trow[j] = p;
        P.prow[j] = p;
        if (scanrow >= 0) {
            const double u = same ? p : srow[j] - fs * p;     // what lpx_update will store at T[s,j]
            rule_feed(rule, best, j, u);
        }
    }
    LPX_STAMP_MB(2);
    best = wave_min_idx(best);                               // one partial per wave
    LPX_STAMP_MB(3);
    if (scanrow >= 0 && !P.qsel) {
        if ((t & 63) == 0) { P.part_v[b * (MB_NT / 64) + (t >> 6)] = best.v; P.part_i[b * (MB_NT / 64) + (t >> 6)] = best.i; }
    } else if (scanrow >= 0) {
        // Streaming tableaux: the workgroup that arrives LAST reduces the partials to the next entering column, so that the update kernel's
        // 10^5 waves read one word instead of each repeating a 128-entry reduction in front of their tile (that prologue
        // cost the streaming update 10 % of its bandwidth, tools/kbench/sweep_dir.hip).  Hand-off as MI355X_MICROARCH.md
        // prescribes for cross-XCD data without fences: every partial is an agent-scope (sc1) store, every storing wave
        // waits for its stores, a workgroup barrier, ONE agent-scope add per workgroup; the workgroup whose add returns
        // nblk - 1 loads the partials with agent-scope (sc1) loads, after its add has returned.
        if ((t & 63) == 0) {
            const int slot = b * (MB_NT / 64) + (t >> 6);
            __hip_atomic_store(&P.part_v[slot], best.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&P.part_i[slot], best.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t < 64) {
            int last = 0;
            if (t == 0) last = (__hip_atomic_fetch_add(&P.part_i[MB_CNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == P.nblk - 1) ? 1 : 0;
            last = __builtin_amdgcn_readfirstlane(last);
            if (last) {
                MinIdx x; x.v = rule.forced ? 0.0 : __builtin_inf(); x.i = INT_MAX;
                const int npart = P.nblk * (MB_NT / 64);               // <= 128
                if (t < npart) {
                    x.v = __hip_atomic_load(&P.part_v[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    x.i = __hip_atomic_load(&P.part_i[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (t + 64 < npart) {
                    MinIdx y;
                    y.v = __hip_atomic_load(&P.part_v[t + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    y.i = __hip_atomic_load(&P.part_i[t + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    x = mi_pick(x, y);
                }
                x = wave_min_idx(x);
                int qn;
                if (x.i == INT_MAX) qn = -1;
                else if (rule.forced) { qn = rule.c0 + x.i; if (qn >= C) qn -= C; }
                else qn = x.i;
                if (t == 0) {
                    P.part_i[MB_QREC] = qn;                                // read by the update kernel (next launch)
                    __hip_atomic_store(&P.part_i[MB_CNT], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    if (t == 0) {
        if (b == 0) {
            if (rule.forced) P.fchosen[k] = q; else P.basis[r] = q;     // basis[leaving] = entering, :110
            if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = q; }
            st->status = LPX_RUNNING;
            st->iter = iter + 1; st->r = r; st->q = q;
            st->primal_count = rule.forced ? primal_count : primal_count + 1;
            st->forced_k = rule.forced ? k + 1 : k;
            st->qn = -1; st->qn_valid = (scanrow >= 0) ? 0 : 1;         // no scan row: next column is "none"
            st->c0n = rule.c0;
        }
    }
    LPX_STAMP_MB(4);
    LPX_STAMP_END_MB;
}

// lpx_update for the multi-workgroup protocol: same streaming body; the next entering column comes from
// the select workgroups' partials, and workgroup 0 commits the state record `us` for the next select.
template <int ROWS = UPD_ROWS, int NTH = UPD_NT, int POLICY = 0>
__device__ __forceinline__ void lpx_update_mb_body(double* __restrict__ T, int ld, int Rcap, int Ccap,
                                                   const int32_t* __restrict__ shape,
                                                   const double* __restrict__ prow,
                                                   double* fac0, double* fac1,
                                                   double* __restrict__ rhsbuf,
                                                   const DevState* __restrict__ st, DevState* us,
                                                   const double* __restrict__ part_v,
                                                   const int32_t* __restrict__ part_i, int nblk,
                                                   int forced, int ncw, int nunits, int mixmod = 1)
{
    // The state record is read FIRST: a launch that finds the loop finished (tail of a batch, finished node
    // of a B&B group) must not stream the tableau.
    const int status = st->status;
    const int r = st->r;
    const int lane = threadIdx.x & 63;
    const int R = shape ? shape[0] : Rcap, C = shape ? shape[1] : Ccap;
    if (status != LPX_RUNNING) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { us->status = status; us->iter = st->iter; }
        return;
    }
    // next entering column: set by select directly (skipped pivot / no scan row), or the minimum of the select workgroups'
    // partials.  Streaming forms: the select workgroup that finished last has reduced them to one word (SelParams::qsel)
    // -- 10^5 single-wave workgroups repeating the reduction in front of their tile cost the update 10 % of its bandwidth.
    // Cache-resident form: every wave reduces them here (one load + 6 DPP steps), which is cheaper than the 1.5-2 us the
    // last-workgroup hand-off adds to select when a pivot takes 15 us in all.
    int qn;
    if (st->qn_valid) {
        qn = st->qn;
    } else if constexpr (POLICY != 0) {
        qn = part_i[MB_QREC];
    } else {
        MinIdx x; x.v = forced ? 0.0 : __builtin_inf(); x.i = INT_MAX;
        const int npart = nblk * (MB_NT / 64);               // <= 128: one partial per select wave
        if (lane < npart) { x.v = part_v[lane]; x.i = part_i[lane]; }
        if (lane + 64 < npart) { MinIdx y; y.v = part_v[lane + 64]; y.i = part_i[lane + 64]; x = mi_pick(x, y); }
        x = wave_min_idx(x);
        if (x.i == INT_MAX) qn = -1;
        else if (forced) { qn = st->c0n + x.i; if (qn >= C) qn -= C; }
        else qn = x.i;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        us->status = LPX_RUNNING; us->iter = st->iter; us->qn = qn;
        us->primal_count = st->primal_count; us->forced_k = st->forced_k;
    }
    if (r < 0) return;                                   // skipped pivot: nothing to update
    const int par = (st->iter - 1) & 1;
    upd_inplace_tiles<ROWS, NTH, POLICY, true>(T, ld, R, C, prow, par ? fac1 : fac0, par ? fac0 : fac1, rhsbuf, r, qn,
                                               lane, ncw, nunits, mixmod);
}

// single-tableau and batched (blockIdx.y = node of a branch-and-bound group) entry points
__global__ __launch_bounds__(SEL_NT) void lpx_select(SelParams P, int lds_doubles)
{
    extern __shared__ __align__(16) double sel_lds[];
    lpx_select_body(P, lds_doubles > 0 ? sel_lds : nullptr);
}
__global__ __launch_bounds__(SEL_NT) void lpx_rhs_init(SelParams P) { lpx_rhs_init_body(P); }
__global__ __launch_bounds__(SEL_NT) void lpx_rhs_init_b(const SelParams* __restrict__ arr) { const SelParams P = arr[blockIdx.y]; lpx_rhs_init_body(P); }
__global__ __launch_bounds__(SEL_NT) void lpx_la_init(SelParams P) { lpx_la_init_body(P); }
__global__ __launch_bounds__(MB_NT) void lpx_select_mb(SelParams P) { lpx_select_mb_body(P); }
__global__ __launch_bounds__(SEL_NT) void lpx_select_b(const SelParams* __restrict__ arr, int lds_doubles)
{
    extern __shared__ __align__(16) double sel_lds[];
    const SelParams P = arr[blockIdx.y];
    lpx_select_body(P, lds_doubles > 0 ? sel_lds : nullptr);
}
__global__ __launch_bounds__(SEL_NT) void lpx_la_init_b(const SelParams* __restrict__ arr) { const SelParams P = arr[blockIdx.y]; lpx_la_init_body(P); }
__global__ __launch_bounds__(MB_NT) void lpx_select_mb_b(const SelParams* __restrict__ arr)
{
    const SelParams P = arr[blockIdx.y];
    if ((int)blockIdx.x >= P.nblk) return;          // grid is sized for the widest node of the group
    lpx_select_mb_body(P);
}

__global__ __launch_bounds__(UPD_NT) void lpx_update(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                     const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                     const DevState* st, int ncw, int nunits)
{
    lpx_update_body(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, ncw, nunits);
}
__global__ __launch_bounds__(UPD_NT) void lpx_update_mb(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                        const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                        const DevState* st, DevState* us, const double* part_v,
                                                        const int32_t* part_i, int nblk, int forced, int ncw, int nunits)
{
    lpx_update_mb_body(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, us, part_v, part_i, nblk, forced, ncw, nunits);
}
// streaming variants (tableau larger than the Infinity Cache): see UPDS_ROWS in lpx_tile.h
__global__ __launch_bounds__(UPDS_NT) void lpx_update_s(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                        const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                        const DevState* st, int ncw, int nunits, int mixmod)
{
    lpx_update_body<UPDS_ROWS, UPDS_NT, 1>(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, ncw, nunits, mixmod);
}
__global__ __launch_bounds__(UPDS_NT) void lpx_update_m(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                        const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                        const DevState* st, int ncw, int nunits, int mixmod)
{
    lpx_update_body<UPDS_ROWS, UPDS_NT, 2>(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, ncw, nunits, mixmod);
}
__global__ __launch_bounds__(UPDS_NT) void lpx_update_mb_s(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                           const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                           const DevState* st, DevState* us, const double* part_v,
                                                           const int32_t* part_i, int nblk, int forced, int ncw, int nunits, int mixmod)
{
    lpx_update_mb_body<UPDS_ROWS, UPDS_NT, 1>(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, us, part_v, part_i, nblk, forced, ncw, nunits, mixmod);
}
__global__ __launch_bounds__(UPDS_NT) void lpx_update_mb_m(double* T, int ld, int Rcap, int Ccap, const int32_t* shape,
                                                           const double* prow, double* fac0, double* fac1, double* rhsbuf,
                                                           const DevState* st, DevState* us, const double* part_v,
                                                           const int32_t* part_i, int nblk, int forced, int ncw, int nunits, int mixmod)
{
    lpx_update_mb_body<UPDS_ROWS, UPDS_NT, 2>(T, ld, Rcap, Ccap, shape, prow, fac0, fac1, rhsbuf, st, us, part_v, part_i, nblk, forced, ncw, nunits, mixmod);
}
// batched: every node of the group advances by one pivot per launch pair; grid.x covers the largest node
__global__ __launch_bounds__(UPD_NT) void lpx_update_b(const SelParams* __restrict__ arr)
{
    const SelParams P = arr[blockIdx.y];
    const int ncw = (P.ld + 127) / 128, nunits = ncw * ((P.R + UPD_ROWS - 1) / UPD_ROWS);
    lpx_update_body(P.T, P.ld, P.R, P.C, P.shape, P.prow, P.pcol, P.pcol, P.rhsbuf, P.st, ncw, nunits);
}
__global__ __launch_bounds__(UPD_NT) void lpx_update_mb_b(const SelParams* __restrict__ arr)
{
    const SelParams P = arr[blockIdx.y];
    const int ncw = (P.ld + 127) / 128, nunits = ncw * ((P.R + UPD_ROWS - 1) / UPD_ROWS);
    lpx_update_mb_body(P.T, P.ld, P.R, P.C, P.shape, P.prow, P.col0, P.col1, P.rhsbuf, P.st, P.us, P.part_v, P.part_i,
                       P.nblk, P.mode == MODE_FORCED ? 1 : 0, ncw, nunits);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
#ifdef LPX_STAMPS
hipError_t pivot_fused_stamps(unsigned long long* acc, int clear);     // lpx_pivot_fused.hip
hipError_t group_fused_stamps(unsigned long long* acc, int clear);     // lpx_group_fused.hip
// element-wise sum of the stamps of every file that writes some
hipError_t debug_copy_stamps(unsigned long long* out, int clear)
{
    for (int k = 0; k < 32; ++k) out[k] = 0;
    hipError_t e = stamps_take(out, clear);
    if (e == hipSuccess) e = pivot_fused_stamps(out, clear);
    if (e == hipSuccess) e = group_fused_stamps(out, clear);
    return e;
}
#endif

static constexpr int SEL_LDS_MAX_DOUBLES = 16 * 1024;          // 128 KB of ratios: tableaux up to 16k rows / columns

hipError_t kernels_init()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_select), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * SEL_LDS_MAX_DOUBLES);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_select_b), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * SEL_LDS_MAX_DOUBLES);
    return e;
}

// doubles of dynamic LDS the dual select needs for a tableau of capacity R x C (0 = too long, scan from global memory)
static int select_lds_doubles(int R, int C)
{
    const int L = ((R > C ? R : C) + 1) & ~1;
    return L <= SEL_LDS_MAX_DOUBLES ? L : 0;
}

hipError_t launch_select(const SelParams& p, hipStream_t s)
{
    const int L = select_lds_doubles(p.R, p.C);
    hipLaunchKernelGGL(lpx_select, dim3(1), dim3(SEL_NT), sizeof(double) * L, s, p, L);
    return hipGetLastError();
}

hipError_t launch_select_la(const SelParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_select_la, dim3(1), dim3(SEL_NT), 0, s, p);
    return hipGetLastError();
}

int select_mb_blocks(int C)
{
    int b = (C + MB_NT - 1) / MB_NT;          // at least one column per lane and pass
    if (b < 1) b = 1;
    if (b > 32) b = 32;
    return b;
}

hipError_t launch_select_mb(const SelParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_select_mb, dim3(p.nblk), dim3(MB_NT), 0, s, p);
    return hipGetLastError();
}

// which form the in-place update of a tableau takes: 0 = cache-resident, 2 = mixed-store streaming, 1 = all-nt streaming
int update_policy(int ld, int R) { return policy_for(tableau_bytes(ld, R), UPD_STREAM_BYTES); }
static int update_mixmod(int ld, int R) { return mixmod_for(tableau_bytes(ld, R)); }

// launch geometry of the in-place forms: 8 rows x 256 lanes (pol 0) or 3 rows x 64 lanes per workgroup, units flattened
struct UpdGeom { int nth, ncw, nunits, nblocks; };
static UpdGeom update_geom(int ld, int R, int pol)
{
    const int rows = pol ? UPDS_ROWS : UPD_ROWS;
    UpdGeom g;
    g.nth = pol ? UPDS_NT : UPD_NT;
    g.ncw = (ld + 127) / 128;
    g.nunits = g.ncw * ((R + rows - 1) / rows);
    g.nblocks = (g.nunits + (g.nth / 64) - 1) / (g.nth / 64);
    return g;
}
int update_blocks(int ld, int R) { return update_geom(ld, R, 0).nblocks; }

hipError_t launch_update_mb(const SelParams& p, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    // the streaming forms read the entering column select's last workgroup reduced: both sides follow SelParams::qsel
    const int pol = !p.qsel ? 0 : (update_policy(p.ld, p.R) == 2 ? 2 : 1);
    const UpdGeom g = update_geom(p.ld, p.R, pol);
    const int forced = p.mode == MODE_FORCED ? 1 : 0;
    if (pol == 0)
        return launch_k(lpx_update_mb, dim3(g.nblocks), dim3(g.nth), 0, s, e0, e1, p.T, p.ld, p.R, p.C, p.shape, p.prow, p.col0, p.col1,
                        p.rhsbuf, p.st, p.us, p.part_v, p.part_i, p.nblk, forced, g.ncw, g.nunits);
    return launch_k(pol == 2 ? lpx_update_mb_m : lpx_update_mb_s, dim3(g.nblocks), dim3(g.nth), 0, s, e0, e1, p.T, p.ld, p.R, p.C, p.shape,
                    p.prow, p.col0, p.col1, p.rhsbuf, p.st, p.us, p.part_v, p.part_i, p.nblk, forced, g.ncw, g.nunits, update_mixmod(p.ld, p.R));
}

// one iteration of a whole group: `arr` holds `count` parameter records in device memory
hipError_t launch_group_iter(const SelParams* arr, int count, int dual, int max_nblk, int max_upd_blocks, hipStream_t s, int maxR, int maxC)
{
    if (dual) {
        const int L = select_lds_doubles(maxR, maxC);
        hipLaunchKernelGGL(lpx_select_b, dim3(1, count), dim3(SEL_NT), sizeof(double) * L, s, arr, L);
        hipLaunchKernelGGL(lpx_update_b, dim3(max_upd_blocks, count), dim3(UPD_NT), 0, s, arr);
    } else {
        hipLaunchKernelGGL(lpx_select_mb_b, dim3(max_nblk, count), dim3(MB_NT), 0, s, arr);
        hipLaunchKernelGGL(lpx_update_mb_b, dim3(max_upd_blocks, count), dim3(UPD_NT), 0, s, arr);
    }
    return hipGetLastError();
}
hipError_t launch_group_init(const SelParams* arr, int count, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_la_init_b, dim3(1, count), dim3(SEL_NT), 0, s, arr);
    return hipGetLastError();
}
hipError_t launch_group_rhs_init(const SelParams* arr, int count, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_rhs_init_b, dim3(1, count), dim3(SEL_NT), 0, s, arr);
    return hipGetLastError();
}
hipError_t launch_rhs_init(const SelParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_rhs_init, dim3(1), dim3(SEL_NT), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_la_init(const SelParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_la_init, dim3(1), dim3(SEL_NT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_update(double* T, int ld, int R, int C, const int32_t* shape, const double* prow, double* fac0, double* fac1,
                         double* rhsbuf, const DevState* st, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    const int pol = update_policy(ld, R);
    const UpdGeom g = update_geom(ld, R, pol);
    if (pol == 0)
        return launch_k(lpx_update, dim3(g.nblocks), dim3(g.nth), 0, s, e0, e1, T, ld, R, C, shape, prow, fac0, fac1, rhsbuf, st, g.ncw, g.nunits);
    return launch_k(pol == 2 ? lpx_update_m : lpx_update_s, dim3(g.nblocks), dim3(g.nth), 0, s, e0, e1, T, ld, R, C, shape, prow, fac0, fac1,
                    rhsbuf, st, g.ncw, g.nunits, update_mixmod(ld, R));
}
hipError_t launch_update(const SelParams& p, double* fac0, double* fac1, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    return launch_update(p.T, p.ld, p.R, p.C, p.shape, p.prow, fac0, fac1, p.rhsbuf, p.st, s, e0, e1);
}

}  // namespace lpx
