// lpx_bounded_plunge.hip -- the plunge (lpx_node_batch_plunge), gfx950 (CDNA4, wave64): ONE launch lets a
// workgroup evaluate a CHAIN of up to `depth` branch-and-bound nodes with the tableau staying in the LDS of its compute unit.
// Node 0 is the entry's K triples; after a node that branches, the same workgroup continues into the ceil child, whose tableau
// differs from the one it holds by one bound.  The tile is loaded once and stored once per launch, not once per node.
//
// Launch shape: a grid of B workgroups x 1024 lanes, workgroup b takes P[b] -- as lpx_bounded_nodes_onchip.  The workgroups
// share nothing: no wait, no flag, no atomic between them.  Every loop is bounded: the chain by depth <= 64, the event loop by
// max_iter (at most max_iter + 1 trips), the rest by Cm, R or K.  A launch therefore always ends.
//
// The node's steps 2b, 5, 6 and 7 are the step files of lpx_onchip.h, the one text every on-chip form includes; what is this
// kernel's own stands here: the chain loop, the once-per-node asm pin of S and t, step 2', the K = 1 shift, the readfirstlane tail
// and the single store.  The arithmetic and its order are those of lpx_bounded_node_body.h, step for step, so that a chain is
// bit-equal to the same nodes as single on-chip calls:
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
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants, the refusal record, oc_uniform; through lpx_bounded.h the shared device pieces

namespace lpx {

__global__ __launch_bounds__(OC_NT) void lpx_bounded_plunge_onchip(const PlungeParams* __restrict__ P)
{
    constexpr int stall_events = 0;                     // no stall guard here yet: this line and the file's switch are all of it
    const PlungeParams Q = P[blockIdx.x];
    const NodeParams N = Q.n;
    extern __shared__ double nd_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ int s_tot[OC_NW];
    __shared__ int s_bad[OC_NW];
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
    int32_t* const basis = N.basis; uint8_t* const flip = N.flip;       // the names of the step files
    int32_t* const trace = N.trace; const int trace_cap = N.trace_cap;

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
    for (int j = t; j < Cm; j += OC_NT) ub_s[j] = N.ub[j];
    __syncthreads();
    for (int k = t; k < K; k += OC_NT)
        if (in_upper[k] == inf && flip[in_cols[k]]) atomicMin(&s_infk, k);
    __syncthreads();
    if (s_infk != INT_MAX) { oc_refuse<false, true>(N, 0, t, 0, s_infk); if (t == 0) *Q.steps = 1; return; }
    for (int k = t; k < K; k += OC_NT) {                // the columns are distinct (checked on the host)
        const int j = in_cols[k];
        const double lw = in_lower[k], up = in_upper[k];
        const double uj = ub_s[j], lj = N.lo[j];
        e_save[2 * k] = uj; e_save[2 * k + 1] = lj;
        const double l1 = lw - lj;
        const double u1 = up - lj;                      // +inf stays +inf
        e_shift[k] = flip[j] ? uj - u1 : l1;
        e_cols[k] = j;
        const double nu = up - lw;
        N.ub[j] = nu; ub_s[j] = nu;
        N.lo[j] = lw;
    }
    __syncthreads();
    int nflips = 0;
    {
        const double* zrow = N.T + (size_t)m * ld;      // left of the RHS: the shift of the edit does not write it
#include "lpx_onchip_count.h"
        if (bad > 0) {                                  // refused: ub and lo as they were, nothing else has been written
            for (int k = t; k < K; k += OC_NT) { const int j = in_cols[k]; N.ub[j] = e_save[2 * k]; N.lo[j] = e_save[2 * k + 1]; }
            oc_refuse<false, true>(N, 0, t, bad, -1);
            if (t == 0) *Q.steps = 1;
            return;
        }
        nflips = n;
    }

    // ---- 3. the live window into LDS, ONCE per launch: a wave per row, lanes along it
    for (int i = wave; i < R; i += OC_NW) {
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
            const double uj = oc_uniform(ub_s[c_col]), lj = oc_uniform(N.lo[c_col]);
            const int fj = __builtin_amdgcn_readfirstlane((int)flip[c_col]);
            const double up = lj + uj;                  // the column's current upper bound (exact: see the header)
            if (__builtin_amdgcn_readfirstlane(up == inf && fj)) { oc_refuse<false, true>(N, s, t, 0, 0); written = s + 1; break; }
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
#include "lpx_onchip_count.h"
            n = __builtin_amdgcn_readfirstlane(n); bad = __builtin_amdgcn_readfirstlane(bad);
            if (bad > 0) {                              // refused with a dirty tile: ub and lo of the one column back, the tile as node s - 1 left it
                if (t == 0) { N.ub[c_col] = uj; ub_s[c_col] = uj; N.lo[c_col] = lj; }
                oc_refuse<false, true>(N, s, t, bad, -1);
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
                for (int i = t; i < R; i += OC_NT) {
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
                for (int i = t; i < R; i += OC_NT) {
                    double* row = tile + (size_t)i * S;
                    const double prod = c_sh * row[c_col];
                    row[Cm] = row[Cm] - prod;
                }
            dirty = true;
            __syncthreads();
        }

        // ---- 5. the dual-feasibility flips, 6. the dual loop; the trace starts at 0 for every node
#include "lpx_onchip_flips.h"
#include "lpx_onchip_dual.h"
        __syncthreads();                                // basis and flip as lane 0 left them, for every lane

        // ---- 7. the branch pick, as lpx_branch_pick_kernel
        int total = 0;
        var = -1; x_var = 0.0;
#include "lpx_onchip_pick.h"

        // ---- 9. the record of node s (pinned host memory), then whether the chain goes on
        // Every lane holds the same values; readfirstlane tells the compiler so, and what the chain carries from node to node
        // then lives in scalar registers.
        const double z = oc_uniform(zrow[Cm]);
        var = __builtin_amdgcn_readfirstlane(var); x_var = oc_uniform(x_var);
        g_status = __builtin_amdgcn_readfirstlane(status); g_iter = __builtin_amdgcn_readfirstlane(iter);
        g_k0 = __builtin_amdgcn_readfirstlane(k0); g_k1 = __builtin_amdgcn_readfirstlane(k1);
        dirty = __builtin_amdgcn_readfirstlane((int)dirty) != 0;
        if (t == 0) {
            NodeOut* o = oc_rec(N, s);
            o->status = g_status; o->events = g_iter; o->kind0 = g_k0; o->kind1 = g_k1; o->flips = nflips; o->unrepairable = 0; o->inf_k = -1;
            o->var = var; o->candidates = total; o->x_var = x_var; o->z = z;
        }
        written = s + 1;
        __syncthreads();                                // the pick's arrays are free for the next node
        if (!(g_status == LPX_OPTIMAL && var >= 0 && !(z <= prune))) break;
    }

    // ---- 8. back to global memory, ONCE per launch: the tableau when it changed, the contiguous RHS copy, the state record
    if (dirty)
        for (int i = wave; i < R; i += OC_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S0;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += OC_NT) N.rhsbuf[i] = tile[(size_t)i * S0 + Cm];
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
    return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_plunge_onchip));
}

hipError_t launch_bounded_plunge_onchip(const PlungeParams* P, int B, size_t lds, hipStream_t s)
{
    if (B < 1 || lds > OC_LDS_MAX) return hipErrorInvalidValue;          // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_plunge_onchip, dim3(B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
