// lpx_bounded_guard.hip -- the on-chip node with the stall guard (lpx_bounded_node4 / lpx_node_batch_run2 with stall_events > 0),
// gfx950 (CDNA4, wave64).  It is the node of lpx_bounded_node.hip -- one workgroup x 1024 lanes per node, the tableau in the LDS of one
// compute unit, the same layout and the same fit rule (bounded_node_lds_bytes) -- whose dual loop keeps two more values, the
// objective at the last progress and the pivots made since, and selects by Bland's rule (least index) once `stall_events` pivots
// have brought no progress, until the objective moves again.  include/lpx.h ("stall guard") is the contract; DESIGN.md section
// 4.21 has the reasons and the numbers.
//
// It has its own text, as the plunge and the probes have: lpx_bounded_node_onchip and lpx_bounded_nodes_onchip stay the code they
// were, and stall_events = 0 never comes here (the host sends it to those kernels).  Steps 1-5 and 7-9 are the text of
// lpx_bounded_node_body.h; step 6 differs in the places its comments name.  The two new selections are block_min_idx reductions:
// the leaving row on the key (basic index, row), the entering column first on (ratio, column) for the minimum and then on
// (0, column) over the columns within ratio_tol of it.  They use the reduction scratch the node has already, so the kernel needs
// no more LDS, static or dynamic, than the node.
//
// As there, no wait on any other workgroup and no spin loop: every loop is bounded by max_iter, Cm, R or K, so a launch always
// ends.  Bland mode ends a trip with a pivot or with a final status like any other trip.
#include "lpx_bounded.h"

namespace lpx {

static constexpr int GD_NT = SEL_NT, GD_NW = SEL_NW;
static constexpr size_t GD_LDS_TOTAL = 160 * 1024;      // one compute unit
static constexpr size_t GD_LDS_STATIC = 2048;           // as the node reserves for its statics

__device__ __forceinline__ void gd_refuse(const NodeParams& N, int t, int flips, int bad, int inf_k)
{
    if (t == 0) {
        GuardOut* g = reinterpret_cast<GuardOut*>(N.out);
        NodeOut* o = &g->o;
        o->status = -1; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->flips = flips; o->unrepairable = bad; o->inf_k = inf_k;
        o->var = -1; o->candidates = 0; o->x_var = 0.0; o->z = 0.0;
        g->bland_events = 0; g->first_bland = -1;
    }
}

// Workgroup b evaluates P[b] (pinned host memory, read once through a wave-uniform address into scalar registers); the single node
// is a batch of one.  The workgroups share nothing, as in lpx_bounded_nodes_onchip.
__global__ __launch_bounds__(GD_NT) void lpx_bounded_guard_onchip(const NodeParams* __restrict__ P)
{
    const NodeParams N = P[blockIdx.x];
    extern __shared__ double gd_lds[];
    __shared__ double s_v[GD_NW];
    __shared__ int s_i[GD_NW];
    __shared__ int s_out;
    __shared__ int s_tot[GD_NW];
    __shared__ int s_bad[GD_NW];
    __shared__ int s_infk;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();

    // ---- 1. the node's inputs (pinned host memory, read once)
    const NodeIn* in = N.in;
    const int K = in->K, flags = in->flags, nint = in->nint, max_iter = in->max_iter, stall_events = in->stall_events;
    const double eps = in->eps, rtol = in->ratio_tol, cutoff = in->cutoff, ptol = in->tol;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;
    const double* in_lower = reinterpret_cast<const double*>(in + 1);
    const double* in_upper = in_lower + K;
    const int32_t* in_cols = reinterpret_cast<const int32_t*>(in_upper + K);

    double* tile = gd_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);

    // the edit staged on the device, in the layout of the other entry points: lower, upper, shift [K] each, save [2K], cols [K]
    double* e_shift = N.edit + 2 * (size_t)K;
    double* e_save = e_shift + K;
    int32_t* e_cols = reinterpret_cast<int32_t*>(e_save + 2 * (size_t)K);

    // ---- 2. the tableau still untouched: +inf on a flipped column, the shifts, the new ub / lo, the count of the flips
    if (t == 0) s_infk = INT_MAX;
    for (int j = t; j < Cm; j += GD_NT) ub_s[j] = N.ub[j];
    __syncthreads();
    for (int k = t; k < K; k += GD_NT)
        if (in_upper[k] == inf && N.flip[in_cols[k]]) atomicMin(&s_infk, k);
    __syncthreads();
    if (s_infk != INT_MAX) { gd_refuse(N, t, 0, 0, s_infk); return; }
    for (int k = t; k < K; k += GD_NT) {                // the columns are distinct (checked on the host)
        const int j = in_cols[k];
        const double lw = in_lower[k], up = in_upper[k];
        const double uj = ub_s[j], lj = N.lo[j];
        e_save[2 * k] = uj; e_save[2 * k + 1] = lj;
        const double l1 = lw - lj;
        const double u1 = up - lj;                      // +inf stays +inf
        e_shift[k] = N.flip[j] ? uj - u1 : l1;
        e_cols[k] = j;
        const double nu = up - lw;
        N.ub[j] = nu; ub_s[j] = nu;
        N.lo[j] = lw;
    }
    __syncthreads();
    int nflips = 0;
    {
        const double* zrow = N.T + (size_t)m * ld;      // left of the RHS: the shift of the edit does not write it
        int n = 0, bad = 0;
        for (int base = 0; base < Cm; base += GD_NT) {  // uniform trip count
            const int j = base + t;
            bool in_l = false, un = false;
            if (j < Cm) {
                const bool neg = zrow[j] < -eps;
                const double u = ub_s[j];
                in_l = neg && u > 0.0 && u < inf;
                un = neg && u == inf;
            }
            n += __popcll(__ballot(in_l)); bad += __popcll(__ballot(un));
        }
        __syncthreads();
        if (lane == 0) { s_tot[wave] = n; s_bad[wave] = bad; }
        __syncthreads();
        n = 0; bad = 0;
        for (int w = 0; w < GD_NW; ++w) { n += s_tot[w]; bad += s_bad[w]; }
        if (bad > 0) {                                  // refused: ub and lo as they were, nothing else has been written
            for (int k = t; k < K; k += GD_NT) { const int j = in_cols[k]; N.ub[j] = e_save[2 * k]; N.lo[j] = e_save[2 * k + 1]; }
            gd_refuse(N, t, 0, bad, -1);
            return;
        }
        nflips = n;
    }

    // ---- 3. the live window into LDS: a wave per row, lanes along it
    for (int i = wave; i < R; i += GD_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    // ---- 4. the RHS shifts of the edit, k in order: a lane per row
    bool dirty = false;                                 // uniform: the tile differs from the tableau in global memory
    if (K > 0) {
        for (int i = t; i < R; i += GD_NT) {
            double* row = tile + (size_t)i * S;
            double b = row[Cm];
            for (int k = 0; k < K; ++k) {
                const double s = e_shift[k];
                if (s == 0.0) continue;
                const double prod = s * row[e_cols[k]];
                b = b - prod;
            }
            row[Cm] = b;
        }
        dirty = true;
        __syncthreads();
    }

    // ---- 5. the dual-feasibility flips, j ascending: the ordered list (a ballot per wave, a prefix over the wave totals), then
    //         a lane per row walks it -- BOUND FLIP arithmetic, objective row included
    if (nflips > 0) {
        const double* zrow = tile + (size_t)m * S;
        int n = 0;
        for (int base = 0; base < Cm; base += GD_NT) {
            const int j = base + t;
            bool in_l = false;
            if (j < Cm) { const double u = ub_s[j]; in_l = zrow[j] < -eps && u > 0.0 && u < inf; }
            const unsigned long long mi = __ballot(in_l);
            const int before = __popcll(mi & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) s_tot[wave] = __popcll(mi);
            __syncthreads();
            int pre = 0, tot = 0;
            for (int w = 0; w < GD_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
            if (in_l) list[n + pre + before] = j;       // n + pre + before < columns tested so far <= Cm
            n += tot;
        }
        __syncthreads();
        for (int k = t; k < n; k += GD_NT) N.flip[list[k]] ^= 1;
        for (int i = t; i < R; i += GD_NT) {
            double* row = tile + (size_t)i * S;
            double b = row[Cm];
            for (int k = 0; k < n; ++k) {
                const int j = list[k];
                const double a = row[j];
                const double prod = ub_s[j] * a;
                b = b - prod;
                row[j] = -a;
            }
            row[Cm] = b;
        }
        dirty = true;
        __syncthreads();
    }

    // ---- 6. the dual loop: every trip ends the loop or makes at least one event.  The stall guard (include/lpx.h, "stall guard"):
    //         z_ref is the objective at the last progress, stall the pivots since; both are uniform over the workgroup, as is bland
    int iter = 0, k0 = 0, k1 = 0, status = LPX_ITER_LIMIT;
    int stall = 0, bland_events = 0, first_bland = -1;
    double* ratios = buf;
    double* pcol = buf;
    double* zrow = tile + (size_t)m * S;
    double z_ref = zrow[Cm];                            // behind the edit and the flips; the next write of it is behind a barrier
    for (int trip = 0; trip <= max_iter; ++trip) {
        if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
        const double z_now = zrow[Cm];
        if (cut && z_now <= cutoff) { status = LPX_CUTOFF; break; }
        if (z_now < z_ref - eps) { z_ref = z_now; stall = 0; }
        const bool bland = stall >= stall_events;

        // leaving row: first strict minimum of the infeasibilities below -eps; in Bland mode the least basic index among them
        // (the key is the index as a double, exact; equal keys cannot occur in a basis, and the lowest row would win)
        MinIdx mn; mn.v = bland ? inf : -eps; mn.i = INT_MAX;
        for (int i = t; i < m; i += GD_NT) {
            const double b = tile[(size_t)i * S + Cm];
            const int pb = N.basis[i];
            const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
            double w = inf;
            if (b < -eps) w = b;
            else if (u < inf) w = u - b;
            if (bland) { if (w < -eps && (double)pb < mn.v) { mn.v = (double)pb; mn.i = i; } }
            else if (w < mn.v) { mn.v = w; mn.i = i; }
        }
        mn = block_min_idx<GD_NT>(mn, s_v, s_i);
        if (mn.i == INT_MAX) { status = LPX_OPTIMAL; break; }
        const int r = mn.i;
        double* trow = tile + (size_t)r * S;
        const int kind = trow[Cm] < -eps ? 0 : 1;
        const int p = N.basis[r];

        // kind 1: the complement of row r in place, in front of the ratios
        if (kind) {
            const double up = ub_s[p];
            __syncthreads();                            // every lane has read trow[Cm] before it is rewritten
            for (int j = t; j < C; j += GD_NT) trow[j] = bnd_complement(trow[j], j, p, Cm, up);
            if (t == 0) N.flip[p] ^= 1;
            dirty = true;
        }

        // the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
        for (int j = t; j < Cm; j += GD_NT) {
            const double a = trow[j];
            bool part = a < -eps;
            if (skip_fixed) part = part && ub_s[j] > 0.0;
            ratios[j] = part ? zrow[j] / (-a) : inf;
        }
        __syncthreads();

        int q;
        if (bland) {                                    // the lowest column within ratio_tol of the minimum; no hysteresis scan
            MinIdx lo_r; lo_r.v = inf; lo_r.i = INT_MAX;
            for (int j = t; j < Cm; j += GD_NT) { const double v = ratios[j]; if (v < lo_r.v) { lo_r.v = v; lo_r.i = j; } }
            lo_r = block_min_idx<GD_NT>(lo_r, s_v, s_i);
            q = -1;
            if (lo_r.i != INT_MAX) {                    // uniform; a ratio is never NaN where the tableau is finite
                const double band = lo_r.v + rtol;
                MinIdx first; first.v = inf; first.i = INT_MAX;
                for (int j = t; j < Cm; j += GD_NT)
                    if (ratios[j] <= band && first.i == INT_MAX) { first.v = 0.0; first.i = j; }
                first = block_min_idx<GD_NT>(first, s_v, s_i);
                q = first.i != INT_MAX ? first.i : lo_r.i;      // a negative ratio_tol leaves the band empty: the minimum itself
            }
            __syncthreads();                            // as rs_hysteresis ends: every lane is past the ratios and the scratch
        } else q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
        if (long_step && !bland) {
            for (int pass = 0; pass < Cm && q >= 0; ++pass) {       // a column passes at most once: its ratio becomes +inf
                const double uq = ub_s[q];
                if (!(uq < inf)) break;
                const double prod = uq * trow[q];
                const double nb = trow[Cm] - prod;
                if (!(nb < -eps)) break;
                __syncthreads();                        // trow[q] and trow[Cm] read by every lane before the rewrite
                for (int i = t; i < R; i += GD_NT) {
                    double* row = tile + (size_t)i * S;
                    const double a = row[q];
                    const double pr = uq * a;
                    row[Cm] = row[Cm] - pr;
                    row[q] = -a;
                }
                if (t == 0) {
                    N.flip[q] ^= 1;
                    if (iter < N.trace_cap) { N.trace[2 * iter] = -1; N.trace[2 * iter + 1] = q; }
                    ratios[q] = inf;
                }
                ++iter;
                __syncthreads();
                q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
            }
        }
        if (q < 0) { status = LPX_INFEASIBLE; break; } // the complement and the passes stay applied

        // pivot prep: column snapshot, row r normalised in place (it is the pivot row of the update)
        const double piv = trow[q];
        for (int i = t; i < R; i += GD_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
        __syncthreads();
        for (int j = t; j < C; j += GD_NT) trow[j] = trow[j] / piv;
        if (t == 0) {
            N.basis[r] = q;
            if (iter < N.trace_cap) { N.trace[2 * iter] = kind ? -2 - r : r; N.trace[2 * iter + 1] = q; }
        }
        if (bland) { if (bland_events == 0) first_bland = iter; ++bland_events; }
        ++iter; ++stall;
        if (kind) ++k1; else ++k0;
        dirty = true;
        __syncthreads();

        // the rank-1 update with the bits of lpx_update: every row but r, one multiply and one subtract per element
        for (int i = wave; i < R; i += GD_NW) {
            if (i == r) continue;
            const double f = pcol[i];
            double* row = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) {
                const double pr = f * trow[j];
                row[j] = row[j] - pr;
            }
        }
        __syncthreads();
    }
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane

    // ---- 7. the branch pick, as lpx_branch_pick_kernel
    int var = -1, total = 0;
    double x_var = 0.0;
    if (status == LPX_OPTIMAL) {
        double* vals = buf;
        const bool masked = in->has_mask && nint > 0;
        for (int j = t; j < nint; j += GD_NT) vals[j] = 0.0;
        __syncthreads();
        for (int i = t; i < m; i += GD_NT) {
            const int pb = N.basis[i];
            if ((unsigned)pb < (unsigned)nint) vals[pb] = tile[(size_t)i * S + Cm];
        }
        __syncthreads();
        MinIdx best; best.v = inf; best.i = INT_MAX;
        int nc = 0;
        for (int j = t; j < nint; j += GD_NT) {
            if (masked && !N.mask[j]) continue;
            const double v = vals[j];
            double x = N.flip[j] ? ub_s[j] - v : v;
            if (in->lo_used) x = x + N.lo[j];
            const double f = x - __builtin_floor(x);
            if (f > ptol && (1.0 - f) > ptol) {
                const double d = __builtin_fabs(f - 0.5);
                ++nc;
                if (d < best.v) { best.v = d; best.i = j; }
            }
        }
        best = block_min_idx<GD_NT>(best, s_v, s_i);
        block_excl_scan_sum<GD_NT>(nc, s_i, &total);
        if (best.i != INT_MAX) {
            var = best.i;
            const double v = vals[var];
            x_var = N.flip[var] ? ub_s[var] - v : v;
            if (in->lo_used) x_var = x_var + N.lo[var];
        }
    }

    // ---- 8. back to global memory: the tableau when it changed, the contiguous RHS copy, the state record
    if (dirty)
        for (int i = wave; i < R; i += GD_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += GD_NT) N.rhsbuf[i] = tile[(size_t)i * S + Cm];
    if (t == 0) {
        DevState s;
        s.status = status; s.iter = iter; s.r = -1; s.q = -1; s.phase = 2; s.fdf_count = k0; s.dual_iter = k1; s.primal_count = iter;
        s.forced_k = 0; s.qn = -1; s.c0n = 0; s.qn_valid = 0; s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
        *N.st = s;
        // ---- 9. the node record (pinned host memory)
        NodeOut* o = N.out;
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->flips = nflips; o->unrepairable = 0; o->inf_k = -1;
        o->var = var; o->candidates = total; o->x_var = x_var; o->z = zrow[Cm];
        GuardOut* g = reinterpret_cast<GuardOut*>(o);
        g->bland_events = bland_events; g->first_bland = first_bland;
    }
}

hipError_t bounded_guard_init()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_bounded_guard_onchip), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(GD_LDS_TOTAL - GD_LDS_STATIC));
}

hipError_t launch_bounded_guard_onchip(const NodeParams* P, int B, size_t lds, hipStream_t s)
{
    if (!P || B < 1 || lds > GD_LDS_TOTAL - GD_LDS_STATIC) return hipErrorInvalidValue;       // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_guard_onchip, dim3(B), dim3(GD_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
