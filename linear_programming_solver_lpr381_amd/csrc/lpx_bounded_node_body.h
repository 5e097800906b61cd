// lpx_bounded_node_body.h -- the body of the on-chip node, included as the text of ALL FOUR of its kernels: lpx_bounded_node_onchip
// (one node, the record a kernel argument) and lpx_bounded_nodes_onchip (the batch, workgroup b takes P[b]) in lpx_bounded_node.hip,
// lpx_bounded_guard_onchip (the batch with the stall guard) in lpx_bounded_guard.hip, and lpx_bounded_fix_onchip (that batch with
// reduced-cost tightening behind the pick, step 7b, under the file switch LPX_ONCHIP_FIX) in lpx_bounded_fix.hip.  Not a header in
// the usual sense: it is a sequence of statements that expects `const NodeParams N` (or `NodeParams N`) in scope and the file's switch GUARD (lpx_onchip.h),
// and may `return` from the kernel.  It is the sequence of its own steps 1-4, 8 and 9; steps 2b, 5, 6 and 7 are the step files that
// the plunge and the probes include too (lpx_onchip_count.h, _flips.h, _dual.h, _pick.h), which find what differs between the
// kernels under the names declared here: basis, flip, trace, trace_cap, dirty, lo_used, max_iter, stall_events.  There is one text
// of the arithmetic, and each kernel is compiled as if the text stood in it.  Why not a __device__ function: with the body behind
// a call -- forced inline; the record by reference, by value or as scalar arguments -- the register allocation of
// lpx_bounded_node_onchip changes (218 instead of 130 SGPR reloads from VGPR lanes in its code, the same 95 VGPRs) and the on-chip
// driver on binary_ip(60, 12) measured 2.5-5.8 % slower than its parent; as included text every kernel keeps the instruction text
// it had when it stood alone (profiles/r18_onchip_text_isa.md).  Where a name is declared matters to that:
// `zrow` stands directly in front of step 5 because a declaration further up moves two instructions of the node kernels.
    extern __shared__ double nd_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ int s_tot[OC_NW];
    __shared__ int s_bad[OC_NW];
    __shared__ int s_infk;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();

    // ---- 1. the node's inputs (pinned host memory, read once)
    const NodeIn* in = N.in;
    const int K = in->K, flags = in->flags, nint = in->nint, max_iter = in->max_iter, stall_events = GUARD ? in->stall_events : 0;
    const double eps = in->eps, rtol = in->ratio_tol, cutoff = in->cutoff, ptol = in->tol;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;
    const double* in_lower = reinterpret_cast<const double*>(in + 1);
    const double* in_upper = in_lower + K;
    const int32_t* in_cols = reinterpret_cast<const int32_t*>(in_upper + K);
    // the names of the step files: what this node writes, its trace, and the lower-shift mark (read where the pick uses it)
    int32_t* const basis = N.basis; uint8_t* const flip = N.flip;
    int32_t* const trace = N.trace; const int trace_cap = N.trace_cap;
    const int32_t& lo_used = in->lo_used;

    double* tile = nd_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);

    // the edit staged on the device, in the layout of the other entry points: lower, upper, shift [K] each, save [2K], cols [K]
    double* e_shift = N.edit + 2 * (size_t)K;
    double* e_save = e_shift + K;
    int32_t* e_cols = reinterpret_cast<int32_t*>(e_save + 2 * (size_t)K);

    // ---- 2. the tableau still untouched: +inf on a flipped column, the shifts, the new ub / lo, the count of the flips
    if (t == 0) s_infk = INT_MAX;
    for (int j = t; j < Cm; j += OC_NT) ub_s[j] = N.ub[j];
    __syncthreads();
    for (int k = t; k < K; k += OC_NT)
        if (in_upper[k] == inf && flip[in_cols[k]]) atomicMin(&s_infk, k);
    __syncthreads();
    if (s_infk != INT_MAX) { oc_refuse<GUARD, false>(N, 0, t, 0, s_infk); return; }
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
            oc_refuse<GUARD, false>(N, 0, t, bad, -1);
            return;
        }
        nflips = n;
    }

    // ---- 3. the live window into LDS: a wave per row, lanes along it
    for (int i = wave; i < R; i += OC_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    // ---- 4. the RHS shifts of the edit, k in order: a lane per row
    bool dirty = false;                                 // uniform: the tile differs from the tableau in global memory
    if (K > 0) {
        for (int i = t; i < R; i += OC_NT) {
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

    // ---- 5. the dual-feasibility flips, 6. the dual loop
    double* zrow = tile + (size_t)m * S;
#include "lpx_onchip_flips.h"
#include "lpx_onchip_dual.h"
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane

    // ---- 7. the branch pick, as lpx_branch_pick_kernel
    int var = -1, total = 0;
    double x_var = 0.0;
#include "lpx_onchip_pick.h"

#if LPX_ONCHIP_FIX      // ---- 7b. reduced-cost bound tightening: the text of lpx_bounded_fix_onchip alone (a preprocessor switch, so
    // that the other kernels of this body keep their instruction text); the kernel declares fix_bound and the list's arrays
    int nfix = 0;
#include "lpx_onchip_fix.h"
#endif

    // ---- 8. back to global memory: the tableau when it changed, the contiguous RHS copy, the state record
    if (dirty)
        for (int i = wave; i < R; i += OC_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += OC_NT) N.rhsbuf[i] = tile[(size_t)i * S + Cm];
    if (t == 0) {
        DevState s;
        s.status = status; s.iter = iter; s.r = -1; s.q = -1; s.phase = 2; s.fdf_count = k0; s.dual_iter = k1; s.primal_count = iter;
        s.forced_k = 0; s.qn = -1; s.c0n = 0; s.qn_valid = 0; s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
        *N.st = s;
        // ---- 9. the node record (pinned host memory)
        NodeOut* o = N.out;
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->flips = nflips; o->unrepairable = 0; o->inf_k = -1;
        o->var = var; o->candidates = total; o->x_var = x_var; o->z = zrow[Cm];
        if (GUARD) { GuardOut* g = reinterpret_cast<GuardOut*>(o); g->bland_events = bland_events; g->first_bland = first_bland; }
#if LPX_ONCHIP_FIX
        o->pad = nfix;                                  // the count of the tightened columns: the record's one spare word
#endif
    }
