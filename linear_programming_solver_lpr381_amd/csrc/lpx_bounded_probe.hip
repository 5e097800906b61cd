// lpx_bounded_probe.hip -- strong-branching probes of a solved branch-and-bound node (lpx_bounded_probe, lpx_node_batch_run_probe;
// contract in include/lpx.h, layout in DESIGN.md section 4.20), gfx950 (CDNA4, wave64).
//
// Launch shape: a grid of (2 * cand_max, B) workgroups x 1024 lanes.  Workgroup (w, e) evaluates ONE child of entry e's handle as it
// stands: candidate c = w >> 1 in the order (|f - 0.5| ascending, column ascending), direction d = w & 1 (0: floor child, 1: ceil
// child).  The workgroups share nothing: no wait, no flag, no spin loop and no atomic between them; each reads the handle, works
// on its own copy in LDS and in its own slice of the workspace, and writes its own record.  Every loop is bounded by probe_iter,
// Cm, R or cand_max (the event loop as in lpx_bounded_node.hip), so a launch always ends.
//
// NOTHING of the handle is written: the tableau, ub, lo, flip, basis, the RHS copy, the state record and the trace are read
// through pointers to const.  What the node kernel keeps in global memory and writes (basis, flip) is copied into the workgroup's
// slice of the workspace first; ub lives in LDS as it does there; lo is read only; the trace is not kept.
//
// The arithmetic of the child is that of lpx_bounded_node_body.h with K = 1 (the edit, the dual-feasibility flips, the dual loop
// with the long-step passes and the cutoff where flagged), operation for operation, so that a record is bit-equal to
// lpx_bounded_node3(..., LPX_NODE_ONCHIP) on a clone of the handle.  Steps 2b, 5 and 6 ARE the node's text, the step files of
// lpx_onchip.h: `basis` and `flip` name this workgroup's slice of the workspace there, no trace is kept and nothing is stored back.
// The candidate passes, the child's edit and the record are this kernel's own; the candidates use the arithmetic of the branch pick
// (lpx_branch_pick_kernel).  Dynamic LDS: that of the node (bounded_node_lds_bytes): tile [R * S], ub [C], buf [max(R, C)].
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h the shared device pieces

namespace lpx {

__device__ __forceinline__ void pb_record(lpx_probe_record* o, int status, int events, int k0, int k1, int flips, int var, int dir,
                                          double x_var, double lower, double upper, double z)
{
    o->status = status; o->events = events; o->kind0 = k0; o->kind1 = k1; o->flips = flips; o->var = var; o->dir = dir; o->pad = 0;
    o->x_var = x_var; o->lower = lower; o->upper = upper; o->z = z;
}

__global__ __launch_bounds__(OC_NT) void lpx_bounded_probe_onchip(const ProbeParams* __restrict__ P)
{
    constexpr int stall_events = 0;                     // no stall guard here yet: this line and the file's switch are all of it
    constexpr int trace_cap = INT_MIN;                              // no trace is kept: no event count lies below it, so the test folds away
    int32_t* const trace = nullptr;
    [[maybe_unused]] bool dirty = false;                            // nothing goes back to the handle
    const ProbeParams N = P[blockIdx.y];
    extern __shared__ double pb_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ int s_tot[OC_NW];
    __shared__ int s_bad[OC_NW];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int w = blockIdx.x;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();
    const int flags = N.flags, nint = N.nint, max_iter = N.probe_iter;
    const double eps = N.eps, rtol = N.ratio_tol, cutoff = N.cutoff, ptol = N.tol;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;

    // ---- 1. early exit: nothing to probe.  Uniform over the workgroup (and over the entry's workgroups: all read the same words).
    {
        const double z0 = N.T[(size_t)m * ld + Cm];
        const bool refused = N.front && N.front->status < 0;
        if (refused || N.st->status != LPX_OPTIMAL || z0 <= N.prune) {
            if (w == 0 && t == 0) { N.head->count = 0; N.head->candidates = 0; N.head->z = z0; }
            return;
        }
    }

    double* tile = pb_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);
    int32_t* basis = N.wbasis + (size_t)w * N.wbasis_stride;       // this workgroup's slice
    uint8_t* flip = N.wflip + (size_t)w * N.wflip_stride;

    // ---- 2. load: ub and the live window into LDS, basis and flip into the slice
    for (int j = t; j < Cm; j += OC_NT) { ub_s[j] = N.ub[j]; flip[j] = N.flip[j]; }
    for (int i = t; i < m; i += OC_NT) basis[i] = N.basis[i];
    for (int i = wave; i < R; i += OC_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    // ---- 3. the candidates, with the arithmetic of the branch pick; candidate c is found by c + 1 passes, each the first
    //         minimum of (distance, column) beyond the pass before it: comparisons only, no arithmetic on the keys
    const int c = w >> 1, dir = w & 1;
    int var = -1, total = 0;
    double x_var = 0.0;
    {
        double* vals = buf;
        const bool masked = N.has_mask && nint > 0;
        for (int j = t; j < nint; j += OC_NT) vals[j] = 0.0;
        __syncthreads();
        for (int i = t; i < m; i += OC_NT) {
            const int pb = basis[i];
            if ((unsigned)pb < (unsigned)nint) vals[pb] = tile[(size_t)i * S + Cm];
        }
        __syncthreads();
        double last_d = -1.0; int last_j = -1;                      // a distance is >= 0: the first pass takes every candidate
        for (int pass = 0; pass <= c; ++pass) {                      // c < cand_max <= 32
            MinIdx best; best.v = inf; best.i = INT_MAX;
            int nc = 0;
            for (int j = t; j < nint; j += OC_NT) {
                if (masked && !N.mask[j]) continue;
                const double v = vals[j];
                double x = flip[j] ? ub_s[j] - v : v;
                if (N.lo_used) x = x + N.lo[j];
                const double f = x - __builtin_floor(x);
                if (f > ptol && (1.0 - f) > ptol) {
                    const double d = __builtin_fabs(f - 0.5);
                    ++nc;
                    const bool beyond = d > last_d || (d == last_d && j > last_j);
                    if (beyond && d < best.v) { best.v = d; best.i = j; }
                }
            }
            best = block_min_idx<OC_NT>(best, s_v, s_i);
            if (pass == 0) block_excl_scan_sum<OC_NT>(nc, s_i, &total);
            if (best.i == INT_MAX) { var = -1; break; }             // fewer than c + 1 candidates
            var = best.i; last_d = best.v; last_j = best.i;
        }
        const int count = total < N.cand_max ? total : N.cand_max;
        if (w == 0 && t == 0) { N.head->count = count; N.head->candidates = total; N.head->z = tile[(size_t)m * S + Cm]; }
        lpx_probe_record* o = N.rec + w;
        if (c >= count || var < 0) {
            if (t == 0) pb_record(o, LPX_PROBE_NONE, 0, 0, 0, 0, -1, dir, 0.0, 0.0, 0.0, 0.0);
            return;
        }
        const double v = vals[var];
        x_var = flip[var] ? ub_s[var] - v : v;
        if (N.lo_used) x_var = x_var + N.lo[var];
    }
    lpx_probe_record* o = N.rec + w;

    // ---- 4. the child's bounds on column var, and its edit as step 2 of the node forms it for K = 1
    const double lj = N.lo[var], uj = ub_s[var];
    const double lw = dir ? __builtin_ceil(x_var) : lj;
    const double up = dir ? lj + uj : __builtin_floor(x_var);
    const bool fl = flip[var] != 0;
    if (up < lw || (up == inf && fl)) {     // what the node call refuses: an empty interval (a bound that is not integral), upper = +inf on a flipped column
        if (t == 0) pb_record(o, -1, 0, 0, 0, 0, var, dir, x_var, lw, up, 0.0);
        return;
    }
    const double l1 = lw - lj;
    const double u1 = up - lj;                                      // +inf stays +inf
    const double shift = fl ? uj - u1 : l1;
    const double nu = up - lw;
    __syncthreads();                                                // every lane has read ub_s[var] and the values of the pick
    if (t == 0) ub_s[var] = nu;
    __syncthreads();
    int nflips = 0;
    {
        const double* zrow = tile + (size_t)m * S;                  // the bits of the tableau's objective row
#include "lpx_onchip_count.h"
        if (bad > 0) {                                              // refused, as the node refuses it
            if (t == 0) pb_record(o, -1, 0, 0, 0, 0, var, dir, x_var, lw, up, 0.0);
            return;
        }
        nflips = n;
    }

    // ---- the RHS shift of the edit: a lane per row
    if (shift != 0.0) {
        for (int i = t; i < R; i += OC_NT) {
            double* row = tile + (size_t)i * S;
            const double prod = shift * row[var];
            row[Cm] = row[Cm] - prod;
        }
    }
    __syncthreads();

    // ---- 5. the dual-feasibility flips and the dual loop (steps 5 and 6 of the node)
    double* zrow = tile + (size_t)m * S;
#include "lpx_onchip_flips.h"
#include "lpx_onchip_dual.h"

    // ---- 6. the record (pinned host memory); nothing goes back to the handle
    if (t == 0) pb_record(o, status, iter, k0, k1, nflips, var, dir, x_var, lw, up, zrow[Cm]);
}

hipError_t bounded_probe_init()
{
    return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_probe_onchip));
}

hipError_t launch_bounded_probe_onchip(const ProbeParams* P, int B, int cand_max, size_t lds, hipStream_t s)
{
    if (B < 1 || cand_max < 1 || cand_max > 32 || lds > OC_LDS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lpx_bounded_probe_onchip, dim3(2 * cand_max, B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
