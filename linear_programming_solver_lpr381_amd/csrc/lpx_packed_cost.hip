// lpx_packed_cost.hip -- packed cost and right-hand-side scenarios warm-started from one solved base (lpx_packed_base_solve_costs,
// include/lpx.h), gfx950 (CDNA4, wave64).  The base of lpx_packed_warm.hip keeps its solved tableau, bounds,
// basis and flip bytes on the device; count cost vectors of that model, each with or without a right-hand side of its own, are
// re-solved in ONE launch.  A cost change leaves the RHS column and with it primal feasibility as the base left them, so workgroup i
// moves the objective row by one m x C product and continues the bounded PRIMAL loop from the base's basis; with a right-hand side
// it then moves the RHS column as lpx_packed_warm.hip does and continues the DUAL loop from the optimum of (c_i, b0).
//
// One kernel, one text: lpx_packed_cost_onchip, one workgroup x 1024 lanes per scenario; whether b is given is a uniform branch.
//
// Shared-device rules, those of lpx_packed_dual.hip:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic;
//   * every loop is bounded by a max_iter, R, C, Cm, m or n; both event loops test their iteration limit first and every trip ends
//     the loop or makes at least one event, so a launch always ends;
//   * every value is written with ordinary vector stores from C++; there is no inline assembly beyond what lpx_onchip.h has;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.30).
//
// The arithmetic of a scenario is the contract of lpx_packed_base_solve_costs in include/lpx.h, steps 1-6, every product and every
// sum separately rounded (-ffp-contract=off).  The primal loop is the text of lpx_packed.hip's (lpx_onchip_primal.h step 2 without
// the trace and the dirty mark), starting from the base's flip bytes; the dual loop is lpx_onchip_dual.h.
//
// Dynamic LDS (doubles) is that of lpx_packed_warm.hip, so lpx_packed_fits is the fit rule unchanged:
//   tile [R * S]        R = m + 1, C = n + m + 1, row stride S = C | 1: odd, so a column walk hits distinct banks
//   ub   [C]            upper bounds of the columns
//   buf  [max(R, C)]    g [C - 1] during the cost move; the primal loop's ratios [m] / pivot-column snapshot [R]; delta_b [m] in
//                       front of the dual loop; that loop's ratios [C - 1] / snapshot; the values v [C - 1] of the extraction
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h bnd_complement, rs_hysteresis and the reductions

#include <climits>
#include <cstring>
#include <mutex>

namespace lpx {

// what the kernel reads and writes: the snapshot of the base, c0 ([n], the base's costs), c ([count][n]), b ([count][m] or null)
struct PackedCostParams {
    const double *c0, *c, *b;
    PackedBaseSnap snap;
    int32_t m, n, min, long_step, p_max_iter, d_max_iter;
    double p_eps, p_ratio_tol, d_eps, d_ratio_tol;
    int32_t* status; double* x; double* value; lpx_packed_cost_record* rec; int32_t* basis; uint8_t* at_upper;   // as lpx_packed_cost_results
    double* y; double* d;
    uint8_t* flip; int64_t flip_stride;                 // work bytes, [count][flip_stride], flip_stride >= n + m
};

__global__ __launch_bounds__(OC_NT) void lpx_packed_cost_onchip(PackedCostParams N)
{
    extern __shared__ double pc_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ double s_const;                          // c_i.l over the user's c_i: what the lower shift took out of the optimum
    __shared__ int s_shifted;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t mdl = blockIdx.x;
    const int m = N.m, n = N.n, R = m + 1, C = n + m + 1, Cm = C - 1;
    const int S = C | 1;
    const double inf = __builtin_inf();
    const bool min = N.min != 0, has_lower = N.snap.lower != nullptr, has_b = N.b != nullptr;

    const double* const glo = N.snap.lower;
    const int32_t* const grel = N.snap.rel;
    const double* const gc = N.c + mdl * (size_t)n;
    int32_t* const basis = N.basis + mdl * (size_t)m;
    uint8_t* const flip = N.flip + mdl * (size_t)N.flip_stride;
    double* const gx = N.x + mdl * (size_t)n;
    uint8_t* const gat = N.at_upper + mdl * (size_t)n;
    double* const gy = N.y + mdl * (size_t)m;
    double* const gd = N.d + mdl * (size_t)n;

    double* tile = pc_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    double* zrow = tile + (size_t)m * S;

    // ---- 1. the base's tile and ub into LDS, its basis and flip bytes into this scenario's slices: the snapshot has the layout
    // of the LDS image, so lane t reads element t and steps by the workgroup
    for (int k = t; k < R * S; k += OC_NT) tile[k] = N.snap.tile[k];
    for (int j = t; j < C; j += OC_NT) ub_s[j] = N.snap.ub[j];
    for (int i = t; i < m; i += OC_NT) basis[i] = N.snap.basis[i];
    // ---- 2. and 3. g in buf (the base's flip byte decides its sign); a cost or a right-hand side that is not finite refuses the
    // scenario
    int bad = 0;
    for (int j = t; j < Cm; j += OC_NT) {
        const uint8_t f = N.snap.flip[j];
        flip[j] = f;
        double g = 0.0;                                 // a slack column has no cost
        if (j < n) {
            const double cj = gc[j];
            if (!(__builtin_fabs(cj) < inf)) bad = 1;
            double dj = cj - N.c0[j];
            if (min) dj = -dj;
            g = (f & 1) ? -dj : dj;
        }
        buf[j] = g;
    }
    if (has_b) {
        const double* const gb = N.b + mdl * (size_t)m;
        for (int k = t; k < m; k += OC_NT) if (!(__builtin_fabs(gb[k]) < inf)) bad = 1;
    }
    if (__syncthreads_or(bad)) {                        // uniform: every lane of the workgroup takes the return
        for (int j = t; j < n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; gd[j] = 0.0; }
        for (int i = t; i < m; i += OC_NT) { basis[i] = 0; gy[i] = 0.0; }
        if (t == 0) {
            N.status[mdl] = LPX_EINVAL; N.value[mdl] = 0.0;
            lpx_packed_cost_record* o = N.rec + mdl;
            o->status = LPX_EINVAL; o->primal_events = 0; o->dual_events = 0; o->pad = 0;
            o->primal_kind0 = 0; o->primal_kind1 = 0; o->primal_flips = 0; o->dual_kind0 = 0; o->dual_kind1 = 0; o->dual_passes = 0;
            o->z = 0.0;
        }
        return;
    }
    // the objective row: one lane per column, the RHS column included; lane j walks column j of the tile for i ascending
    // (consecutive lanes, consecutive addresses) while g of the basic column of row i is one address for all lanes.  The lane of
    // the RHS column sums K first, lane 0 the shift constant.  A lane writes only its own entry of the objective row
    if (t == 0) {
        double constant = 0.0; int shifted = 0;
        if (has_lower)
            for (int j = 0; j < n; ++j) {
                const double l = glo[j];
                if (l != 0.0) { const double prod = gc[j] * l; constant = constant + prod; shifted = 1; }
            }
        s_const = constant; s_shifted = shifted;
    }
    for (int j = t; j < C; j += OC_NT) {
        double K = 0.0;
        if (j == Cm)
            for (int k = 0; k < n; ++k) {
                const double gk = buf[k];
                if ((N.snap.flip[k] & 1) && gk != 0.0) { const double dk = -gk; const double prod = dk * ub_s[k]; K = K + prod; }
            }
        double acc = zrow[j];
        for (int i = 0; i < m; ++i) {
            const double gi = buf[N.snap.basis[i]];
            if (gi != 0.0) { const double prod = gi * tile[(size_t)i * S + j]; acc = acc + prod; }
        }
        if (j < n) { const double gj = buf[j]; if (gj != 0.0) acc = acc - gj; }
        if (j == Cm) acc = acc + K;
        zrow[j] = acc;
    }
    __syncthreads();                                    // the objective row stands; g in buf is dead

    // ---- 4. the primal loop from the base's basis and flip bytes: lpx_onchip_primal.h step 2
    int p_iter = 0, p_k0 = 0, p_k1 = 0, p_flips = 0, p_status = LPX_ITER_LIMIT;
    {
        const double eps = N.p_eps, rtol = N.p_ratio_tol;
        const int max_iter = N.p_max_iter;
        double* ratios = buf;
        double* pcol = buf;
        for (int trip = 0; trip <= max_iter; ++trip) {
            if (p_iter >= max_iter) { p_status = LPX_ITER_LIMIT; break; }
            // ChooseEntering: the event before this one ended on a barrier behind its writes of the objective row
            const int q = block_first_min_below<OC_NT>(zrow, 1, Cm, eps, s_v, s_i);
            if (q < 0) { p_status = LPX_OPTIMAL; break; }

            // the three-way ratios of rows 0..m-1: a column walk of the tile (odd stride: no bank conflict), ub through the basis
            for (int i = t; i < m; i += OC_NT) {
                const double a = tile[(size_t)i * S + q];
                const double b = tile[(size_t)i * S + Cm];
                const int pb = basis[i];
                const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
                double rho = inf;
                if (a > eps) rho = b / a;                                   // basic variable goes to zero
                else if (a < -eps && u < inf) rho = (u - b) / (-a);         // basic variable goes to its upper bound
                ratios[i] = rho;
            }
            __syncthreads();
            const int r = rs_hysteresis(m, rtol, ratios, s_v, s_i, &s_out);
            const double best = r >= 0 ? ratios[r] : inf;
            const double uq = ub_s[q];
            // what the pivot needs of row r as it stands, read by every lane in front of the barrier below
            double* trow = tile + (size_t)(r >= 0 ? r : 0) * S;
            const double a_rq = trow[q];
            const int p = r >= 0 ? basis[r] : -1;
            __syncthreads();                            // every lane is past the ratios and row r before either is rewritten

            if (uq < inf && uq <= best) {               // BOUND FLIP of column q, ties go to the flip: RHS column and column q, R rows
                for (int i = t; i < R; i += OC_NT) {
                    double* row = tile + (size_t)i * S;
                    const double a = row[q];
                    const double prod = uq * a;         // mul, then sub: contraction is off
                    row[Cm] = row[Cm] - prod;
                    row[q] = -a;
                }
                if (t == 0) flip[q] ^= 1;
                ++p_iter; ++p_flips;
                __syncthreads();
                continue;
            }
            if (r < 0) { p_status = LPX_UNBOUNDED; break; }

            // pivot prep: kind 1 (T[r,q] <= eps) leaves at its upper bound, row r complemented in front of the division
            const int kind = a_rq > eps ? 0 : 1;
            const double up = kind ? ub_s[p] : 0.0;
            const double piv = kind ? -a_rq : a_rq;
            for (int i = t; i < R; i += OC_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
            for (int j = t; j < C; j += OC_NT) {        // a lane rewrites the entries of row r that only it reads here
                double v = trow[j];
                if (kind) v = bnd_complement(v, j, p, Cm, up);
                trow[j] = v / piv;
            }
            if (t == 0) {
                if (kind) flip[p] ^= 1;
                basis[r] = q;
            }
            ++p_iter;
            if (kind) ++p_k1; else ++p_k0;
            __syncthreads();

            // the rank-1 update with the bits of lpx_update: every row but r, one multiply and one subtract per element
            for (int i = wave; i < R; i += OC_NW) {
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
    }

    // ---- 5. with b, behind an optimal primal phase: the RHS move of lpx_packed_base_solve and the dual loop.  Every exit of the
    // primal loop is behind a barrier that follows the last read of the ratios and of the pivot-column snapshot, so buf is free
    int final_status = p_status, d_iter = 0, d_k0 = 0, d_k1 = 0;
    if (has_b && p_status == LPX_OPTIMAL) {             // uniform
        const double* const gb = N.b + mdl * (size_t)m;
        for (int k = t; k < m; k += OC_NT) {
            const double dk = gb[k] - N.snap.b0[k];
            buf[k] = (grel && grel[k] == LPX_GE) ? -dk : dk;
        }
        __syncthreads();
        // one lane per row (R <= 140 lanes), k ascending, one multiply and one add per non-zero delta_k; a lane reads and writes
        // its own row only
        if (t < R) {
            double* row = tile + (size_t)t * S;
            double acc = row[Cm];
            for (int k = 0; k < m; ++k) {
                const double dk = buf[k];
                if (dk != 0.0) { const double prod = row[n + k] * dk; acc = acc + prod; }
            }
            row[Cm] = acc;
        }
        __syncthreads();                                // the tile stands; delta in buf is dead

        const double eps = N.d_eps, rtol = N.d_ratio_tol, cutoff = 0.0;
        const int max_iter = N.d_max_iter, stall_events = 0;
        const bool skip_fixed = false, cut = false, long_step = N.long_step != 0;
        bool dirty = false;                             // a dead local: nothing is stored back
        int32_t* const trace = nullptr;
        const int trace_cap = 0;
#include "lpx_onchip_dual.h"
        (void)dirty; (void)cutoff; (void)stall_events;
        final_status = status; d_iter = iter; d_k0 = k0; d_k1 = k1;
    }
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane

    // ---- 6. the results from LDS.  v_j = the RHS of the row where j is basic, else +0.0; bit 1 of the flip byte marks a basic j
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
        N.status[mdl] = final_status; N.value[mdl] = value;
        lpx_packed_cost_record* o = N.rec + mdl;
        o->status = final_status; o->primal_events = p_iter; o->dual_events = d_iter; o->pad = 0;
        o->primal_kind0 = p_k0; o->primal_kind1 = p_k1; o->primal_flips = p_flips;
        o->dual_kind0 = d_k0; o->dual_kind1 = d_k1; o->dual_passes = d_iter - d_k0 - d_k1;
        o->z = z;
    }
}

// ---- the host side: the arena, the pinned block and the stream of lpx_packed.hip (g_packed, lpx_internal.h) ---------------------
namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

bool g_attr_cost = false;                               // the function attribute is set (under g_packed.mu)

}  // namespace

int packed_base_solve_costs(const PackedBase* base, const double* c0, int32_t count32, const double* c, const double* b, int flags,
                            const lpx_run_opts* op, const lpx_run_opts* od, const lpx_packed_cost_results* out, lpx_stats* st)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t count = (size_t)count32, m = (size_t)base->m, n = (size_t)base->n;
    const int R = base->m + 1, C = base->n + base->m + 1;

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!g_attr_cost) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_cost_onchip))); g_attr_cost = true; }

    // the arena: c0, c and b, the results in the order of the pinned block (x, value, rec, status, basis, at_upper, y, d), the
    // flip bytes
    const size_t in_bytes[3] = {sizeof(double) * n, sizeof(double) * count * n, b ? sizeof(double) * count * m : 0};
    const void* in_src[3] = {c0, c, b};
    const size_t out_bytes[8] = {sizeof(double) * count * n, sizeof(double) * count, sizeof(lpx_packed_cost_record) * count,
                                 sizeof(int32_t) * count, sizeof(int32_t) * count * m, count * n,
                                 sizeof(double) * count * m, sizeof(double) * count * n};
    size_t in_off[3], out_off[8], at = 0;
    for (int k = 0; k < 3; ++k) { in_off[k] = at; at += up256(in_bytes[k]); }
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

    PackedCostParams p;
    std::memset(&p, 0, sizeof(p));
    p.c0 = reinterpret_cast<const double*>(a.dev + in_off[0]); p.c = reinterpret_cast<const double*>(a.dev + in_off[1]);
    p.b = b ? reinterpret_cast<const double*>(a.dev + in_off[2]) : nullptr;
    p.snap = base->snap;
    p.m = base->m; p.n = base->n; p.min = base->min;
    p.long_step = (flags & LPX_BDUAL_LONG_STEP) ? 1 : 0;
    p.p_max_iter = op->max_iter; p.d_max_iter = od->max_iter;
    p.p_eps = op->eps; p.p_ratio_tol = op->ratio_tol; p.d_eps = od->eps; p.d_ratio_tol = od->ratio_tol;
    p.x = reinterpret_cast<double*>(a.dev + out_off[0]); p.value = reinterpret_cast<double*>(a.dev + out_off[1]);
    p.rec = reinterpret_cast<lpx_packed_cost_record*>(a.dev + out_off[2]); p.status = reinterpret_cast<int32_t*>(a.dev + out_off[3]);
    p.basis = reinterpret_cast<int32_t*>(a.dev + out_off[4]); p.at_upper = reinterpret_cast<uint8_t*>(a.dev + out_off[5]);
    p.y = reinterpret_cast<double*>(a.dev + out_off[6]); p.d = reinterpret_cast<double*>(a.dev + out_off[7]);
    p.flip = reinterpret_cast<uint8_t*>(a.dev + flip_off); p.flip_stride = (int64_t)flip_stride;

    const double t0 = now_ms();
    for (int k = 0; k < 3; ++k)
        if (in_bytes[k]) LPX_HIP_TRY(hipMemcpyAsync(a.dev + in_off[k], in_src[k], in_bytes[k], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_cost_onchip, dim3((unsigned)count), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + res0, res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));       // the one wait
    const double ms = now_ms() - t0;

    const char* res = a.pin - res0;
    const lpx_packed_cost_record* recs = reinterpret_cast<const lpx_packed_cost_record*>(res + out_off[2]);
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
        for (size_t i = 0; i < count; ++i) st->pivots += recs[i].primal_kind0 + recs[i].primal_kind1 + recs[i].dual_kind0 + recs[i].dual_kind1;
        st->launches = 1; st->loop_ms = ms;
    }
    return 0;
}

}  // namespace lpx
