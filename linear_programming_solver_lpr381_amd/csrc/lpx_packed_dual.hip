// lpx_packed_dual.hip -- packed batches of small bounded LPs by a dual start (lpx_solve_packed_dual, include/lpx.h; DESIGN.md
// section 4.26), gfx950 (CDNA4, wave64): lpx_packed.hip for the models lpx_solve_bounded_dual was built for.  count models of one
// shape come in as contiguous arrays, rows <= or >=, right-hand sides of either sign; ONE launch solves them all, arrays go back.
// Workgroup i builds the tableau of model i in the LDS of its compute unit (a >= row negated while it is stored), counts and makes
// the dual-feasibility flips, runs the on-chip bounded dual loop with or without the long step and extracts the results and the
// duals from LDS.
//
// Launch shape: ONE workgroup x 1024 lanes per model, a grid of count independent workgroups.
//
// Shared-device rules, those of lpx_packed.hip:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic;
//   * every loop is bounded by max_iter, Cm, R, C or n; the dual loop tests the iteration limit first and every trip ends the loop
//     or makes at least one event, so it makes at most max_iter + 1 trips of at most Cm passes each, and a launch always ends;
//   * every value is written with ordinary vector stores from C++; there is no inline assembly beyond what lpx_onchip.h has;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.26).
//
// The arithmetic of the preparation is prepare_dual's (tests/_bounded_long_ref.py): the negation of a >= row, then the lower shift,
// both as the row is stored and read back; steps 2b, 5 and 6 are the included texts of the on-chip node (lpx_onchip_count.h,
// lpx_onchip_flips.h, lpx_onchip_dual.h) with the tolerance of lpx_tableau_dualize(1e-9) for the first two; the extraction is that
// of lpx_packed.hip plus the duals, which are objective-row bits with exact sign changes.
//
// Dynamic LDS (doubles) is the packed primal kernel's, so lpx_packed_fits is the fit rule unchanged:
//   tile [R * S]        R = m + 1, C = n + m + 1, row stride S = C | 1
//   ub   [C]            upper bounds of the columns
//   buf  [max(R, C)]    the lower bounds [n] while the tableau is built; the flip list (int32 [Cm]) of step 5; the ratios [Cm] / the
//                       pivot-column snapshot [R] of the loop; the values v [C - 1] while the results are extracted
// The basis of a model lives in its slice of the basis output, its flip bytes in a work slice of the call's arena.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h bnd_complement, rs_hysteresis and the reductions

#include <climits>
#include <cstring>
#include <mutex>

namespace lpx {

__global__ __launch_bounds__(OC_NT) void lpx_packed_dual_onchip(PackedDualParams N)
{
    extern __shared__ double pd_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ int s_tot[OC_NW];
    __shared__ int s_bad[OC_NW];
    __shared__ double s_const;                          // c.l over the user's c: what the lower shift took out of the optimum
    __shared__ int s_shifted;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t mdl = blockIdx.x;
    const int m = N.m, n = N.n, R = m + 1, C = n + m + 1, Cm = C - 1;
    const int S = C | 1;
    const double inf = __builtin_inf();
    const double eps = N.eps, rtol = N.ratio_tol, cutoff = 0.0;
    const int max_iter = N.max_iter, stall_events = 0;
    const bool min = N.min != 0, has_lower = N.lower != nullptr;
    const bool skip_fixed = false, cut = false, long_step = N.long_step != 0;

    const double* const gc = N.c + mdl * (size_t)N.c_stride;
    const double* const gA = N.A + mdl * (size_t)N.A_stride;
    const double* const gb = N.b + mdl * (size_t)N.b_stride;
    const double* const glo = has_lower ? N.lower + mdl * (size_t)N.lower_stride : nullptr;
    const double* const gup = N.upper ? N.upper + mdl * (size_t)N.upper_stride : nullptr;
    const int32_t* const grel = N.rel ? N.rel + mdl * (size_t)N.rel_stride : nullptr;
    int32_t* const basis = N.basis + mdl * (size_t)m;
    uint8_t* const flip = N.flip + mdl * (size_t)N.flip_stride;
    double* const gx = N.x + mdl * (size_t)n;
    uint8_t* const gat = N.at_upper + mdl * (size_t)n;
    double* const gy = N.y + mdl * (size_t)m;
    double* const gd = N.d + mdl * (size_t)n;

    double* tile = pd_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    double* zrow = tile + (size_t)m * S;

    // ---- 1. the tableau of the model into LDS.  The bounds and the row senses first, with the host path's checks
    int bad = 0;
    for (int j = t; j < n; j += OC_NT) {
        const double l = has_lower ? glo[j] : 0.0;
        const double u = gup ? gup[j] : inf;
        if (!(__builtin_fabs(l) < inf) || !(u >= l)) bad = 1;
        buf[j] = l;
        ub_s[j] = gup ? (__builtin_isinf(u) ? u : u - l) : inf;
        double cj = gc[j];
        if (min) cj = -cj;                              // Min negates c ...
        zrow[j] = -cj;                                  // ... and the objective row is the negation of that: a zero cost gives -0.0
        flip[j] = 0;
    }
    for (int j = n + t; j < Cm; j += OC_NT) { ub_s[j] = inf; flip[j] = 0; }
    if (grel)
        for (int i = t; i < m; i += OC_NT) { const int r = grel[i]; if (r != LPX_LE && r != LPX_GE) bad = 1; }
    // A, coalesced over the whole m x n block: lane t starts at element t and steps by the workgroup.  A >= row is negated here,
    // in front of the lower shift: only signs change, a zero becomes -0.0
    {
        const int dr = OC_NT / n, dc = OC_NT % n;
        int i = t / n, j = t % n;
        for (int k = t; k < m * n; k += OC_NT) {
            const double a = gA[k];
            const bool ge = grel && grel[i] == LPX_GE;
            tile[(size_t)i * S + j] = ge ? -a : a;
            i += dr; j += dc;
            if (j >= n) { j -= n; ++i; }
        }
    }
    // the slack block (the identity), the RHS column of b (negated with its row) and the +0.0 of the objective row behind the costs
    for (int k = t; k < R * R; k += OC_NT) {
        const int i = k / R, jj = k - i * R;            // column n + jj; jj = m is the RHS column
        double v = (i < m && jj == i) ? 1.0 : 0.0;
        if (i < m && jj == m) { const double bi = gb[i]; v = (grel && grel[i] == LPX_GE) ? -bi : bi; }
        tile[(size_t)i * S + n + jj] = v;
    }
    for (int i = t; i < m; i += OC_NT) basis[i] = n + i;
    if (__syncthreads_or(bad)) {                        // uniform: every lane of the workgroup takes the return
        for (int j = t; j < n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; gd[j] = 0.0; }
        for (int i = t; i < m; i += OC_NT) { basis[i] = 0; gy[i] = 0.0; }
        if (t == 0) {
            N.status[mdl] = LPX_EINVAL; N.value[mdl] = 0.0;
            lpx_packed_dual_record* o = N.rec + mdl;
            o->status = LPX_EINVAL; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->passes = 0; o->dualize_flips = 0; o->z = 0.0;
        }
        return;
    }
    // x = l + x': b' = b - A l from LDS over the rows as they are stored, one lane per row, j ascending, one multiply and one subtract
    // per non-zero l_j; a lane without a row sums c.l over the user's c the same way.  A negative b' is what the dual start is for
    if (has_lower) {
        for (int i = t; i < m; i += OC_NT) {
            const double* row = tile + (size_t)i * S;
            double bi = row[Cm];
            for (int j = 0; j < n; ++j) {
                const double l = buf[j];
                if (l != 0.0) { const double prod = row[j] * l; bi = bi - prod; }
            }
            tile[(size_t)i * S + Cm] = bi;
        }
        if (t == (((m + 63) >> 6) << 6)) {              // the first lane of the first wave without a row (m <= 139 under the fit rule)
            double constant = 0.0; int shifted = 0;
            for (int j = 0; j < n; ++j) {
                const double l = buf[j];
                if (l != 0.0) { const double cu = min ? zrow[j] : -zrow[j]; const double prod = cu * l; constant = constant + prod; shifted = 1; }
            }
            s_const = constant; s_shifted = shifted;
        }
    } else if (t == 0) { s_const = 0.0; s_shifted = 0; }
    __syncthreads();                                    // the tile, ub and the flip bytes stand; the lower bounds in buf are dead

    // ---- 2b. the count of the dual-feasibility flips and of the columns no flip can repair, 5. the flips: both with the tolerance
    // of lpx_tableau_dualize(1e-9), whatever the loop's eps is
    int nflips = 0;
    bool dirty = false;                                 // a dead local: nothing is stored back
    {
        const double eps = 1e-9;
        int32_t* list = reinterpret_cast<int32_t*>(buf);
        int unrepairable = 0;
        {
#include "lpx_onchip_count.h"
            nflips = n; unrepairable = bad;
        }
        if (unrepairable > 0) {                         // uniform: the precheck of lpx_solve_bounded_dual
            for (int j = t; j < N.n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; gd[j] = 0.0; }
            for (int i = t; i < m; i += OC_NT) { basis[i] = 0; gy[i] = 0.0; }
            if (t == 0) {
                N.status[mdl] = LPX_EINVAL; N.value[mdl] = 0.0;
                lpx_packed_dual_record* o = N.rec + mdl;
                o->status = LPX_EINVAL; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->passes = 0; o->dualize_flips = 0; o->z = 0.0;
            }
            return;
        }
#include "lpx_onchip_flips.h"
    }

    // ---- 6. the dual loop from the slack basis
    int32_t* const trace = nullptr;
    const int trace_cap = 0;
#include "lpx_onchip_dual.h"
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane
    (void)dirty; (void)cutoff; (void)stall_events;

    // ---- the results from LDS.  v_j = the RHS of the row where j is basic, else +0.0; bit 1 of the flip byte marks a basic j
    double* v = buf;
    for (int j = t; j < Cm; j += OC_NT) v[j] = 0.0;
    __syncthreads();
    for (int i = t; i < m; i += OC_NT) {
        const int pb = basis[i];
        if ((unsigned)pb < (unsigned)Cm) { v[pb] = tile[(size_t)i * S + Cm]; flip[pb] |= 2; }       // the basis holds a column once
    }
    __syncthreads();
    for (int j = t; j < n; j += OC_NT) {
        const int f = flip[j];
        double xj = (f & 1) ? ub_s[j] - v[j] : v[j];
        if (has_lower) xj = xj + glo[j];                // a zero lower bound is added too, as on the host: -0.0 becomes +0.0
        gx[j] = xj;
        gat[j] = ((f & 1) && !(f & 2)) ? 1 : 0;
        const double dj = zrow[j];                      // d_j = c_j - sum_i y_i A_ij in the user's sense
        gd[j] = (min == ((f & 1) != 0)) ? -dj : dj;
    }
    for (int i = t; i < m; i += OC_NT) {                // y_i = d value / d b_i on the user's row
        const double yi = zrow[n + i];
        const bool ge = grel && grel[i] == LPX_GE;
        gy[i] = (ge != min) ? -yi : yi;
    }
    if (t == 0) {
        const double z = zrow[Cm];
        const bool shifted = s_shifted != 0;
        double value = z;                               // the tableau maximises; the user's optimum is -z for a Min model ...
        if (shifted || min) {
            value = min ? -z : z;
            if (shifted) value = value + s_const;       // ... plus the constant the shift took out
        }
        N.status[mdl] = status; N.value[mdl] = value;
        lpx_packed_dual_record* o = N.rec + mdl;
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->passes = iter - k0 - k1; o->dualize_flips = nflips; o->z = z;
    }
}

// ---- the host side of a call: the arena, the pinned block and the stream of lpx_packed.hip (g_packed, lpx_internal.h) ------------
namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int packed_dual_solve(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* out, lpx_stats* st)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t count = (size_t)in->count, m = (size_t)in->m, n = (size_t)in->n;
    const int R = in->m + 1, C = in->n + in->m + 1;
    if (!bounded_node_fits(R, C) || in->m > OC_NT - 64) { set_error("lpx_solve_packed_dual: the shape does not fit"); return LPX_EINVAL; }   // never launched beyond one compute unit

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!a.attr_dual) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_dual_onchip))); a.attr_dual = true; }

    // the arena: the inputs (a shared array once), the results in the order of the pinned block, the flip bytes
    auto models = [&](int64_t stride) { return stride == 0 ? (size_t)1 : count; };
    const size_t in_bytes[6] = {sizeof(double) * n * models(in->c_stride), sizeof(double) * m * n * models(in->A_stride),
                                sizeof(double) * m * models(in->b_stride), in->lower ? sizeof(double) * n * models(in->lower_stride) : 0,
                                in->upper ? sizeof(double) * n * models(in->upper_stride) : 0,
                                in->rel ? sizeof(int32_t) * m * models(in->rel_stride) : 0};
    const void* in_src[6] = {in->c, in->A, in->b, in->lower, in->upper, in->rel};
    const size_t out_bytes[8] = {sizeof(double) * count * n, sizeof(double) * count, sizeof(lpx_packed_dual_record) * count,
                                 sizeof(int32_t) * count, sizeof(int32_t) * count * m, count * n,
                                 sizeof(double) * count * m, sizeof(double) * count * n};     // x, value, rec, status, basis, at_upper, y, d
    size_t in_off[6], out_off[8], at = 0;
    for (int k = 0; k < 6; ++k) { in_off[k] = at; at += up256(in_bytes[k]); }
    const size_t res0 = at;
    for (int k = 0; k < 8; ++k) { out_off[k] = at; at += up256(out_bytes[k]); }
    const size_t res_bytes = at - res0;
    const size_t flip_stride = (n + m + 15) & ~(size_t)15;
    const size_t flip_off = at; at += up256(count * flip_stride);
    if (at > a.dev_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.dev) hipFree(a.dev);
        a.dev = nullptr; a.dev_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&a.dev, at));
        a.dev_bytes = at;
    }
    if (res_bytes > a.pin_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.pin) hipHostFree(a.pin);
        a.pin = nullptr; a.pin_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&a.pin, res_bytes));
        a.pin_bytes = res_bytes;
    }

    PackedDualParams p;
    std::memset(&p, 0, sizeof(p));
    p.c = reinterpret_cast<const double*>(a.dev + in_off[0]); p.A = reinterpret_cast<const double*>(a.dev + in_off[1]);
    p.b = reinterpret_cast<const double*>(a.dev + in_off[2]);
    p.lower = in->lower ? reinterpret_cast<const double*>(a.dev + in_off[3]) : nullptr;
    p.upper = in->upper ? reinterpret_cast<const double*>(a.dev + in_off[4]) : nullptr;
    p.rel = in->rel ? reinterpret_cast<const int32_t*>(a.dev + in_off[5]) : nullptr;
    p.c_stride = in->c_stride; p.A_stride = in->A_stride; p.b_stride = in->b_stride;
    p.lower_stride = in->lower_stride; p.upper_stride = in->upper_stride; p.rel_stride = in->rel_stride;
    p.m = in->m; p.n = in->n; p.min = in->sense == LPX_MIN ? 1 : 0; p.max_iter = o->max_iter;
    p.long_step = (flags & LPX_BDUAL_LONG_STEP) ? 1 : 0;
    p.eps = o->eps; p.ratio_tol = o->ratio_tol;
    p.x = reinterpret_cast<double*>(a.dev + out_off[0]); p.value = reinterpret_cast<double*>(a.dev + out_off[1]);
    p.rec = reinterpret_cast<lpx_packed_dual_record*>(a.dev + out_off[2]); p.status = reinterpret_cast<int32_t*>(a.dev + out_off[3]);
    p.basis = reinterpret_cast<int32_t*>(a.dev + out_off[4]); p.at_upper = reinterpret_cast<uint8_t*>(a.dev + out_off[5]);
    p.y = reinterpret_cast<double*>(a.dev + out_off[6]); p.d = reinterpret_cast<double*>(a.dev + out_off[7]);
    p.flip = reinterpret_cast<uint8_t*>(a.dev + flip_off); p.flip_stride = (int64_t)flip_stride;

    const double t0 = now_ms();
    for (int k = 0; k < 6; ++k)
        if (in_bytes[k]) LPX_HIP_TRY(hipMemcpyAsync(a.dev + in_off[k], in_src[k], in_bytes[k], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_dual_onchip, dim3((unsigned)count), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + res0, res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));       // the one wait
    const double ms = now_ms() - t0;

    const char* res = a.pin - res0;
    const lpx_packed_dual_record* recs = reinterpret_cast<const lpx_packed_dual_record*>(res + out_off[2]);
    std::memcpy(out->x, res + out_off[0], out_bytes[0]);
    std::memcpy(out->value, res + out_off[1], out_bytes[1]);
    std::memcpy(out->status, res + out_off[3], out_bytes[3]);
    if (out->rec) std::memcpy(out->rec, recs, out_bytes[2]);
    if (out->basis) std::memcpy(out->basis, res + out_off[4], out_bytes[4]);
    if (out->at_upper) std::memcpy(out->at_upper, res + out_off[5], out_bytes[5]);
    if (out->y) std::memcpy(out->y, res + out_off[6], out_bytes[6]);
    if (out->d) std::memcpy(out->d, res + out_off[7], out_bytes[7]);
    if (st) {
        std::memset(st, 0, sizeof(*st));
        for (size_t i = 0; i < count; ++i) st->pivots += recs[i].kind0 + recs[i].kind1;
        st->launches = 1; st->loop_ms = ms;
    }
    return 0;
}

}  // namespace lpx
