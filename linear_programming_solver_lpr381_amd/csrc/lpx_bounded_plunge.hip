// lpx_bounded_plunge.hip -- the plunge (lpx_node_batch_plunge), gfx950 (CDNA4, wave64): ONE launch lets a
// workgroup evaluate a CHAIN of up to `depth` branch-and-bound nodes with the tableau staying in the LDS of its compute unit.
// Node 0 is the entry's K triples; after a node that branches, the same workgroup continues into the ceil child, whose tableau
// differs from the one it holds by one bound.  The tile is loaded once and stored once per launch, not once per node.
//
// Launch shape: a grid of B workgroups x 1024 lanes, workgroup b takes P[b] -- as lpx_bounded_nodes_onchip.  The workgroups
// share nothing: no wait, no flag, no atomic between them.  Every loop is bounded: the chain by depth <= 64, the event loop by
// max_iter (at most max_iter + 1 trips), the rest by Cm, R or K.  A launch therefore always ends.
//
// This file has its own text of the node: lpx_bounded_node_body.h and lpx_bounded_node.hip are untouched, so the two existing
// kernels keep their code (section 4.18 measured what sharing the text behind a call costs them).  The arithmetic and its order
// are those of the body, step for step, so that a chain is bit-equal to the same nodes as single on-chip calls:
//   node 0        steps 1, 2 of the body on the entry's triples (the objective row still read from global memory, which holds
//                 the same bits), then step 3, the ONE load of the tile.
//   node s + 1    the one triple (var, ceil(x_var), lo[var] + ub[var]) of node s's pick, in the handle's own terms.  The sum is the
//                 column's current upper bound exactly: integer columns have integral finite bounds (the caller is held to it
//                 for depth > 1), ub was stored as upper - lower, and sums of such integers are exact in double.  The triple
//                 goes through steps 2, 4, 5, 6, 7 with K = 1; step 2 reads the objective row from the tile, which is now the truth.
//   the end       step 8 once: the tile back when dirty, the RHS copy, the state record with the last completed node's counts.
// A record (NodeOut, 64 bytes apart) is written after every node; `steps` is the number of records written.  The chain goes on
// iff status == LPX_OPTIMAL, var >= 0, !(z <= prune) and s + 1 < depth.
//
// A refusal inside the chain (an unrepairable column or +inf on a flipped column at node s + 1) is found with a dirty tile: ub / lo
// of the one column are put back, record s + 1 is marked refused (status -1), the chain ends and step 8 stores the tile as node s
// left it.  A refusal at node 0 is the body's: nothing has been written.
//
// The lower-shift mark: NodeIn::lo_used is what the host knew before the launch.  A child with a non-zero new lower bound raises it
// inside the launch, exactly where a single call's header would carry it.
//
// Edit staging: node 0 uses the body's layout for K triples; an in-chain edit uses the layout for K = 1 at the same base (shift at
// double 2, the saved pair at 3 and 4, the column at 5), which is what the last single call would leave there.  The host sizes the
// staging for max(K, 1) triples.  LDS layout and fit rule: lpx_bounded_node.hip (bounded_node_lds_bytes, lpx_bounded_node_fits).
#include "lpx_bounded.h"       // bnd_complement; through lpx_resident.h rs_hysteresis, through lpx_block.h the reductions

namespace lpx {

static constexpr int PL_NT = SEL_NT, PL_NW = SEL_NW;
static constexpr size_t PL_LDS_MAX = 160 * 1024 - 2048;  // one compute unit less the statics: the rule of bounded_node_fits
static constexpr size_t PL_REC = 64;                     // the records of a chain are 64 bytes apart

__device__ __forceinline__ NodeOut* pl_rec(const NodeParams& N, int s)
{
    return reinterpret_cast<NodeOut*>(reinterpret_cast<char*>(N.out) + PL_REC * (size_t)s);
}

__device__ __forceinline__ void pl_refuse(const NodeParams& N, int s, int t, int bad, int inf_k)
{
    if (t == 0) {
        // the zero goes through an empty asm: the record's constants are then formed here, on this rare path, and not kept in
        // registers across the whole chain (where they spilled to scratch)
        int zero = 0;
        asm volatile("" : "+v"(zero));
        NodeOut* o = pl_rec(N, s);
        o->status = zero - 1; o->events = zero; o->kind0 = zero; o->kind1 = zero; o->flips = zero; o->unrepairable = bad; o->inf_k = inf_k;
        o->var = zero - 1; o->candidates = zero; o->x_var = (double)zero; o->z = (double)zero;
    }
}

// v is the same in every lane: its bits through readfirstlane, so that the compiler keeps it in scalar registers
__device__ __forceinline__ double pl_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(PL_NT) void lpx_bounded_plunge_onchip(const PlungeParams* __restrict__ P)
{
    const PlungeParams Q = P[blockIdx.x];
    const NodeParams N = Q.n;
    extern __shared__ double nd_lds[];
    __shared__ double s_v[PL_NW];
    __shared__ int s_i[PL_NW];
    __shared__ int s_out;
    __shared__ int s_tot[PL_NW];
    __shared__ int s_bad[PL_NW];
    __shared__ int s_infk;

    const int t = threadIdx.x, t0 = t, lane = t & 63, wave = t >> 6;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S0 = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();
    const int depth = Q.depth;
    const double prune = Q.prune;

    // ---- 1. the entry's inputs (pinned host memory, read once)
    const NodeIn* in = N.in;
    const int K = in->K, flags = in->flags, nint = in->nint, max_iter = in->max_iter;
    const double eps = in->eps, rtol = in->ratio_tol, cutoff = in->cutoff, ptol = in->tol;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;
    const double* in_lower = reinterpret_cast<const double*>(in + 1);
    const double* in_upper = in_lower + K;
    const int32_t* in_cols = reinterpret_cast<const int32_t*>(in_upper + K);
    bool lo_used = in->lo_used != 0;

    double* tile = nd_lds;
    double* ub_s = tile + (size_t)R * S0;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);

    // the edit of node 0 staged on the device, in the layout of the other entry points: lower, upper, shift [K] each, save [2K], cols [K]
    double* e_shift = N.edit + 2 * (size_t)K;
    double* e_save = e_shift + K;
    int32_t* e_cols = reinterpret_cast<int32_t*>(e_save + 2 * (size_t)K);
    // the edit of a node inside the chain: the same layout for K = 1
    double* c_shift = N.edit + 2;
    double* c_save = N.edit + 3;
    int32_t* c_cols = reinterpret_cast<int32_t*>(N.edit + 5);

    // ---- 2. node 0, the tableau still untouched: +inf on a flipped column, the shifts, the new ub / lo, the count of the flips
    if (t == 0) s_infk = INT_MAX;
    for (int j = t; j < Cm; j += PL_NT) ub_s[j] = N.ub[j];
    __syncthreads();
    for (int k = t; k < K; k += PL_NT)
        if (in_upper[k] == inf && N.flip[in_cols[k]]) atomicMin(&s_infk, k);
    __syncthreads();
    if (s_infk != INT_MAX) { pl_refuse(N, 0, t, 0, s_infk); if (t == 0) *Q.steps = 1; return; }
    for (int k = t; k < K; k += PL_NT) {                // the columns are distinct (checked on the host)
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
        for (int base = 0; base < Cm; base += PL_NT) {  // uniform trip count
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
        for (int w = 0; w < PL_NW; ++w) { n += s_tot[w]; bad += s_bad[w]; }
        if (bad > 0) {                                  // refused: ub and lo as they were, nothing else has been written
            for (int k = t; k < K; k += PL_NT) { const int j = in_cols[k]; N.ub[j] = e_save[2 * k]; N.lo[j] = e_save[2 * k + 1]; }
            pl_refuse(N, 0, t, bad, -1);
            if (t == 0) *Q.steps = 1;
            return;
        }
        nflips = n;
    }

    // ---- 3. the live window into LDS, ONCE per launch: a wave per row, lanes along it
    for (int i = wave; i < R; i += PL_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S0;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    bool dirty = false;                                 // uniform: the tile differs from the tableau in global memory
    int written = 0;                                    // records written so far
    int g_status = LPX_ITER_LIMIT, g_iter = 0, g_k0 = 0, g_k1 = 0;      // the last completed node, for the state record
    int var = -1;
    double x_var = 0.0;
    for (int s = 0; s < depth; ++s) {
        // The row stride and the lane number go through an empty asm once per node: the compiler then forms the row addresses and
        // the lane predicates of every step inside the node, as the single-node kernel does, and does not carry them in registers
        // across the whole chain (which spilled to scratch).
        int S = S0, t = t0;
        asm volatile("" : "+s"(S), "+v"(t));
        const int lane = t & 63, wave = t >> 6;
        double* zrow = tile + (size_t)m * S;
        int c_col = 0;
        double c_sh = 0.0;
        if (s > 0) {
            // ---- 2'. the ceil child of node s - 1: one triple, the objective row read from the tile
            c_col = var;
            const double lw = __builtin_ceil(x_var);
            const double uj = pl_uniform(ub_s[c_col]), lj = pl_uniform(N.lo[c_col]);
            const int fj = __builtin_amdgcn_readfirstlane((int)N.flip[c_col]);
            const double up = lj + uj;                  // the column's current upper bound (exact: see the header)
            if (__builtin_amdgcn_readfirstlane(up == inf && fj)) { pl_refuse(N, s, t, 0, 0); written = s + 1; break; }
            const double l1 = lw - lj;
            const double u1 = up - lj;
            c_sh = fj ? uj - u1 : l1;
            const double nu = up - lw;
            __syncthreads();                            // every lane has read ub_s, lo and flip of the column
            if (t == 0) {
                c_save[0] = uj; c_save[1] = lj; c_shift[0] = c_sh; c_cols[0] = c_col;
                N.ub[c_col] = nu; ub_s[c_col] = nu;
                N.lo[c_col] = lw;
            }
            __syncthreads();
            int n = 0, bad = 0;
            for (int base = 0; base < Cm; base += PL_NT) {
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
            for (int w = 0; w < PL_NW; ++w) { n += s_tot[w]; bad += s_bad[w]; }
            n = __builtin_amdgcn_readfirstlane(n); bad = __builtin_amdgcn_readfirstlane(bad);
            if (bad > 0) {                              // refused with a dirty tile: ub and lo of the one column back, the tile as node s - 1 left it
                if (t == 0) { N.ub[c_col] = uj; ub_s[c_col] = uj; N.lo[c_col] = lj; }
                pl_refuse(N, s, t, bad, -1);
                written = s + 1;
                __syncthreads();
                break;
            }
            nflips = n;
            if (__builtin_amdgcn_readfirstlane(lw != 0.0)) lo_used = true;             // what the header of a single call would say
        }

        // ---- 4. the RHS shifts of the edit, k in order: a lane per row
        if (s == 0) {
            if (K > 0) {
                for (int i = t; i < R; i += PL_NT) {
                    double* row = tile + (size_t)i * S;
                    double b = row[Cm];
                    for (int k = 0; k < K; ++k) {
                        const double sh = e_shift[k];
                        if (sh == 0.0) continue;
                        const double prod = sh * row[e_cols[k]];
                        b = b - prod;
                    }
                    row[Cm] = b;
                }
                dirty = true;
                __syncthreads();
            }
        } else {
            if (c_sh != 0.0)
                for (int i = t; i < R; i += PL_NT) {
                    double* row = tile + (size_t)i * S;
                    const double prod = c_sh * row[c_col];
                    row[Cm] = row[Cm] - prod;
                }
            dirty = true;
            __syncthreads();
        }

        // ---- 5. the dual-feasibility flips, j ascending: the ordered list (a ballot per wave, a prefix over the wave totals), then
        //         a lane per row walks it -- BOUND FLIP arithmetic, objective row included
        if (nflips > 0) {
            int n = 0;
            for (int base = 0; base < Cm; base += PL_NT) {
                const int j = base + t;
                bool in_l = false;
                if (j < Cm) { const double u = ub_s[j]; in_l = zrow[j] < -eps && u > 0.0 && u < inf; }
                const unsigned long long mi = __ballot(in_l);
                const int before = __popcll(mi & ((1ull << lane) - 1ull));
                __syncthreads();
                if (lane == 0) s_tot[wave] = __popcll(mi);
                __syncthreads();
                int pre = 0, tot = 0;
                for (int w = 0; w < PL_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
                if (in_l) list[n + pre + before] = j;   // n + pre + before < columns tested so far <= Cm
                n += tot;
            }
            __syncthreads();
            for (int k = t; k < n; k += PL_NT) N.flip[list[k]] ^= 1;
            for (int i = t; i < R; i += PL_NT) {
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

        // ---- 6. the dual loop: every trip ends the loop or makes at least one event; the trace starts at 0 for every node
        int iter = 0, k0 = 0, k1 = 0, status = LPX_ITER_LIMIT;
        double* ratios = buf;
        double* pcol = buf;
        for (int trip = 0; trip <= max_iter; ++trip) {
            if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
            if (cut && zrow[Cm] <= cutoff) { status = LPX_CUTOFF; break; }

            // leaving row: first strict minimum of the infeasibilities below -eps
            MinIdx mn; mn.v = -eps; mn.i = INT_MAX;
            for (int i = t; i < m; i += PL_NT) {
                const double b = tile[(size_t)i * S + Cm];
                const int pb = N.basis[i];
                const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
                double w = inf;
                if (b < -eps) w = b;
                else if (u < inf) w = u - b;
                if (w < mn.v) { mn.v = w; mn.i = i; }
            }
            mn = block_min_idx<PL_NT>(mn, s_v, s_i);
            if (mn.i == INT_MAX) { status = LPX_OPTIMAL; break; }
            const int r = mn.i;
            double* trow = tile + (size_t)r * S;
            const int kind = trow[Cm] < -eps ? 0 : 1;
            const int p = N.basis[r];

            // kind 1: the complement of row r in place, in front of the ratios
            if (kind) {
                const double up = ub_s[p];
                __syncthreads();                        // every lane has read trow[Cm] before it is rewritten
                for (int j = t; j < C; j += PL_NT) trow[j] = bnd_complement(trow[j], j, p, Cm, up);
                if (t == 0) N.flip[p] ^= 1;
                dirty = true;
            }

            // the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
            for (int j = t; j < Cm; j += PL_NT) {
                const double a = trow[j];
                bool part = a < -eps;
                if (skip_fixed) part = part && ub_s[j] > 0.0;
                ratios[j] = part ? zrow[j] / (-a) : inf;
            }
            __syncthreads();

            int q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
            if (long_step) {
                for (int pass = 0; pass < Cm && q >= 0; ++pass) {   // a column passes at most once: its ratio becomes +inf
                    const double uq = ub_s[q];
                    if (!(uq < inf)) break;
                    const double prod = uq * trow[q];
                    const double nb = trow[Cm] - prod;
                    if (!(nb < -eps)) break;
                    __syncthreads();                    // trow[q] and trow[Cm] read by every lane before the rewrite
                    for (int i = t; i < R; i += PL_NT) {
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
            for (int i = t; i < R; i += PL_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
            __syncthreads();
            for (int j = t; j < C; j += PL_NT) trow[j] = trow[j] / piv;
            if (t == 0) {
                N.basis[r] = q;
                if (iter < N.trace_cap) { N.trace[2 * iter] = kind ? -2 - r : r; N.trace[2 * iter + 1] = q; }
            }
            ++iter;
            if (kind) ++k1; else ++k0;
            dirty = true;
            __syncthreads();

            // the rank-1 update with the bits of lpx_update: every row but r, one multiply and one subtract per element
            for (int i = wave; i < R; i += PL_NW) {
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
        __syncthreads();                                // basis and flip as lane 0 left them, for every lane

        // ---- 7. the branch pick, as lpx_branch_pick_kernel
        int total = 0;
        var = -1; x_var = 0.0;
        if (status == LPX_OPTIMAL) {
            double* vals = buf;
            const bool masked = in->has_mask && nint > 0;
            for (int j = t; j < nint; j += PL_NT) vals[j] = 0.0;
            __syncthreads();
            for (int i = t; i < m; i += PL_NT) {
                const int pb = N.basis[i];
                if ((unsigned)pb < (unsigned)nint) vals[pb] = tile[(size_t)i * S + Cm];
            }
            __syncthreads();
            MinIdx best; best.v = inf; best.i = INT_MAX;
            int nc = 0;
            for (int j = t; j < nint; j += PL_NT) {
                if (masked && !N.mask[j]) continue;
                const double v = vals[j];
                double x = N.flip[j] ? ub_s[j] - v : v;
                if (lo_used) x = x + N.lo[j];
                const double f = x - __builtin_floor(x);
                if (f > ptol && (1.0 - f) > ptol) {
                    const double d = __builtin_fabs(f - 0.5);
                    ++nc;
                    if (d < best.v) { best.v = d; best.i = j; }
                }
            }
            best = block_min_idx<PL_NT>(best, s_v, s_i);
            block_excl_scan_sum<PL_NT>(nc, s_i, &total);
            if (best.i != INT_MAX) {
                var = best.i;
                const double v = vals[var];
                x_var = N.flip[var] ? ub_s[var] - v : v;
                if (lo_used) x_var = x_var + N.lo[var];
            }
        }

        // ---- 9. the record of node s (pinned host memory), then whether the chain goes on
        // Every lane holds the same values; readfirstlane tells the compiler so, and what the chain carries from node to node
        // then lives in scalar registers.
        const double z = pl_uniform(zrow[Cm]);
        var = __builtin_amdgcn_readfirstlane(var); x_var = pl_uniform(x_var);
        g_status = __builtin_amdgcn_readfirstlane(status); g_iter = __builtin_amdgcn_readfirstlane(iter);
        g_k0 = __builtin_amdgcn_readfirstlane(k0); g_k1 = __builtin_amdgcn_readfirstlane(k1);
        dirty = __builtin_amdgcn_readfirstlane((int)dirty) != 0;
        if (t == 0) {
            NodeOut* o = pl_rec(N, s);
            o->status = g_status; o->events = g_iter; o->kind0 = g_k0; o->kind1 = g_k1; o->flips = nflips; o->unrepairable = 0; o->inf_k = -1;
            o->var = var; o->candidates = total; o->x_var = x_var; o->z = z;
        }
        written = s + 1;
        __syncthreads();                                // the pick's arrays are free for the next node
        if (!(g_status == LPX_OPTIMAL && var >= 0 && !(z <= prune))) break;
    }

    // ---- 8. back to global memory, ONCE per launch: the tableau when it changed, the contiguous RHS copy, the state record
    if (dirty)
        for (int i = wave; i < R; i += PL_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S0;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += PL_NT) N.rhsbuf[i] = tile[(size_t)i * S0 + Cm];
    if (t == 0) {
        DevState st;
        st.status = g_status; st.iter = g_iter; st.r = -1; st.q = -1; st.phase = 2; st.fdf_count = g_k0; st.dual_iter = g_k1; st.primal_count = g_iter;
        st.forced_k = 0; st.qn = -1; st.c0n = 0; st.qn_valid = 0; st.pad[0] = st.pad[1] = st.pad[2] = st.pad[3] = 0;
        *N.st = st;
        *Q.steps = written;
    }
}

hipError_t bounded_plunge_init()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_bounded_plunge_onchip), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)PL_LDS_MAX);
}

hipError_t launch_bounded_plunge_onchip(const PlungeParams* P, int B, size_t lds, hipStream_t s)
{
    if (B < 1 || lds > PL_LDS_MAX) return hipErrorInvalidValue;          // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_plunge_onchip, dim3(B), dim3(PL_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
