// lpx_packed.hip -- packed batches of small bounded LPs (lpx_solve_packed, include/lpx.h), gfx950 (CDNA4,
// wave64): count models of one shape come in as contiguous arrays, ONE launch solves them all, arrays go back.  There is no handle
// and no tableau in device memory: workgroup i builds the tableau of model i in the LDS of its compute unit, runs the on-chip
// bounded primal loop on it and extracts the results from LDS.
//
// Launch shape: ONE workgroup x 1024 lanes per model, a grid of count independent workgroups.
//
// Shared-device rules, those of lpx_bounded_primal.hip:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic;
//   * every loop is bounded by max_iter, R, C or n; the event loop tests the iteration limit first and makes exactly one event
//     per trip, so it makes at most max_iter + 1 trips, and a launch always ends;
//   * every value is written with ordinary vector stores from C++; there is no inline assembly beyond what lpx_onchip.h has;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.25).
//
// The arithmetic of the preparation is prepare_bounded's and BuildTableauPrimal's (host/bounded.cpp, host/solvers.cpp), that of
// the loop is lpx_onchip_primal.h step 2 (the text below is that step without the trace and the dirty mark, which have no reader
// here), that of the extraction is lpx_tableau_bounded_solution's and collect()'s: IEEE double, -ffp-contract=off, one multiply
// and one subtract (or add) per element, in the order of the host path.  The results are bit-equal to lpx_solve_bounded2 with
// LPX_NODE_ONCHIP model by model.
//
// Dynamic LDS (doubles) is the on-chip primal loop's, so bounded_node_lds_bytes(m + 1, n + m + 1) is the fit rule unchanged:
//   tile [R * S]        R = m + 1, C = n + m + 1, row stride S = C | 1 (odd: a column walk hits distinct banks)
//   ub   [C]            upper bounds of the columns
//   buf  [max(R, C)]    the lower bounds [n] while the tableau is built; then the ratios [m] / the pivot-column snapshot [R]; the
//                       values v [C - 1] while the results are extracted
// The basis of a model lives in its slice of the basis output, its flip bytes in a work slice of the call's arena (a gather or lane
// 0's few words per event, as the handle forms keep them in global memory).  Bit 1 of a flip byte marks a basic column during the
// extraction.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h bnd_complement, rs_hysteresis and the reductions

#include <cstring>
#include <mutex>

namespace lpx {

__global__ __launch_bounds__(OC_NT) void lpx_packed_primal_onchip(PackedParams N)
{
    extern __shared__ double pk_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ double s_const;                          // c.l over the user's c: what the lower shift took out of the optimum
    __shared__ int s_shifted;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const size_t mdl = blockIdx.x;
    const int m = N.m, n = N.n, R = m + 1, C = n + m + 1, Cm = C - 1;
    const int S = C | 1;
    const double inf = __builtin_inf();
    const double eps = N.eps, rtol = N.ratio_tol;
    const int max_iter = N.max_iter;
    const bool min = N.min != 0, has_lower = N.lower != nullptr;

    const double* const gc = N.c + mdl * (size_t)N.c_stride;
    const double* const gA = N.A + mdl * (size_t)N.A_stride;
    const double* const gb = N.b + mdl * (size_t)N.b_stride;
    const double* const glo = has_lower ? N.lower + mdl * (size_t)N.lower_stride : nullptr;
    const double* const gup = N.upper ? N.upper + mdl * (size_t)N.upper_stride : nullptr;
    int32_t* const basis = N.basis + mdl * (size_t)m;
    uint8_t* const flip = N.flip + mdl * (size_t)N.flip_stride;
    double* const gx = N.x + mdl * (size_t)n;
    uint8_t* const gat = N.at_upper + mdl * (size_t)n;

    double* tile = pk_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    double* zrow = tile + (size_t)m * S;

    // ---- 1. the tableau of the model into LDS.  The bounds first, with the host path's checks: a lower bound that is not finite
    // or !(upper >= lower) refuses the model
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
    // A, coalesced over the whole m x n block: lane t starts at element t and steps by the workgroup
    {
        const int dr = OC_NT / n, dc = OC_NT % n;
        int i = t / n, j = t % n;
        for (int k = t; k < m * n; k += OC_NT) {
            tile[(size_t)i * S + j] = gA[k];
            i += dr; j += dc;
            if (j >= n) { j -= n; ++i; }
        }
    }
    // the slack block (the identity), the RHS column of b and the +0.0 of the objective row behind the costs
    for (int k = t; k < R * R; k += OC_NT) {
        const int i = k / R, jj = k - i * R;            // column n + jj; jj = m is the RHS column
        double v = (i < m && jj == i) ? 1.0 : 0.0;
        if (i < m && jj == m) v = gb[i];
        tile[(size_t)i * S + n + jj] = v;
    }
    for (int i = t; i < m; i += OC_NT) basis[i] = n + i;
    if (__syncthreads_or(bad)) {                        // uniform: every lane of the workgroup takes the return
        for (int j = t; j < n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; }
        for (int i = t; i < m; i += OC_NT) basis[i] = 0;
        if (t == 0) {
            N.status[mdl] = LPX_EINVAL; N.value[mdl] = 0.0;
            lpx_primal_record* o = N.rec + mdl;
            o->status = LPX_EINVAL; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->flips = 0; o->z = 0.0;
        }
        return;
    }
    // x = l + x': b' = b - A l from LDS, one lane per row (the odd row stride keeps the column walk free of bank conflicts), j
    // ascending, one multiply and one subtract per non-zero l_j; lane m sums c.l over the user's c the same way
    int neg = 0;
    if (has_lower) {
        for (int i = t; i < m; i += OC_NT) {
            const double* row = tile + (size_t)i * S;
            double bi = row[Cm];
            for (int j = 0; j < n; ++j) {
                const double l = buf[j];
                if (l != 0.0) { const double prod = row[j] * l; bi = bi - prod; }
            }
            tile[(size_t)i * S + Cm] = bi;
            if (bi < -1e-9) neg = 1;
        }
        if (t == (((m + 63) >> 6) << 6)) {              // the first lane of the first wave without a row (m <= 139 under the fit rule)
            double constant = 0.0; int shifted = 0;
            for (int j = 0; j < n; ++j) {
                const double l = buf[j];
                if (l != 0.0) { const double cu = min ? zrow[j] : -zrow[j]; const double prod = cu * l; constant = constant + prod; shifted = 1; }
            }
            s_const = constant; s_shifted = shifted;
        }
    } else {
        for (int i = t; i < m; i += OC_NT) if (tile[(size_t)i * S + Cm] < -1e-9) neg = 1;
        if (t == 0) { s_const = 0.0; s_shifted = 0; }
    }
    if (__syncthreads_or(neg)) {
        for (int j = t; j < n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; }
        for (int i = t; i < m; i += OC_NT) basis[i] = 0;
        if (t == 0) {
            N.status[mdl] = LPX_E_NEG_RHS; N.value[mdl] = 0.0;
            lpx_primal_record* o = N.rec + mdl;
            o->status = LPX_E_NEG_RHS; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->flips = 0; o->z = 0.0;
        }
        return;
    }

    // ---- 2. the event loop: lpx_onchip_primal.h step 2
    double* ratios = buf;
    double* pcol = buf;
    int iter = 0, k0 = 0, k1 = 0, nflips = 0, status = LPX_ITER_LIMIT;
    for (int trip = 0; trip <= max_iter; ++trip) {
        if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
        // ChooseEntering: the event before this one ended on a barrier behind its writes of the objective row
        const int q = block_first_min_below<OC_NT>(zrow, 1, Cm, eps, s_v, s_i);
        if (q < 0) { status = LPX_OPTIMAL; break; }

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
        __syncthreads();                                // every lane is past the ratios and row r before either is rewritten

        if (uq < inf && uq <= best) {                   // BOUND FLIP of column q, ties go to the flip: RHS column and column q, R rows
            for (int i = t; i < R; i += OC_NT) {
                double* row = tile + (size_t)i * S;
                const double a = row[q];
                const double prod = uq * a;             // mul, then sub: contraction is off
                row[Cm] = row[Cm] - prod;
                row[q] = -a;
            }
            if (t == 0) flip[q] ^= 1;
            ++iter; ++nflips;
            __syncthreads();
            continue;
        }
        if (r < 0) { status = LPX_UNBOUNDED; break; }

        // pivot prep: kind 1 (T[r,q] <= eps) leaves at its upper bound, row r complemented in front of the division
        const int kind = a_rq > eps ? 0 : 1;
        const double up = kind ? ub_s[p] : 0.0;
        const double piv = kind ? -a_rq : a_rq;
        for (int i = t; i < R; i += OC_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
        for (int j = t; j < C; j += OC_NT) {            // a lane rewrites the entries of row r that only it reads here
            double v = trow[j];
            if (kind) v = bnd_complement(v, j, p, Cm, up);
            trow[j] = v / piv;
        }
        if (t == 0) {
            if (kind) flip[p] ^= 1;
            basis[r] = q;
        }
        ++iter;
        if (kind) ++k1; else ++k0;
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

    // ---- 3. the results from LDS.  Every exit of the loop is behind a barrier that follows the last write of the tile, of the
    // basis and of the flip bytes.  v_j = the RHS of the row where j is basic, else +0.0; bit 1 of the flip byte marks a basic j
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
        lpx_primal_record* o = N.rec + mdl;
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->flips = nflips; o->z = z;
    }
}

// ---- the host side of a call: one arena on the device, one pinned block for the results, one stream (PackedArena, lpx_internal.h:
// lpx_packed_dual.hip uses the same one) ---------------------------------------------------------------------------------------
PackedArena g_packed;       // never destroyed, as the handle cache: the HIP runtime may be gone by the time statics are torn down

namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int packed_solve(const lpx_packed_models* in, const lpx_run_opts* o, const lpx_packed_results* out, lpx_stats* st)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t count = (size_t)in->count, m = (size_t)in->m, n = (size_t)in->n;
    const int R = in->m + 1, C = in->n + in->m + 1;
    if (!bounded_node_fits(R, C) || in->m > OC_NT - 64) { set_error("lpx_solve_packed: the shape does not fit"); return LPX_EINVAL; }   // never launched beyond one compute unit

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!a.attr) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_primal_onchip))); a.attr = true; }

    // the arena: the inputs (a shared array once), the results in the order of the pinned block, the flip bytes
    auto models = [&](int64_t stride) { return stride == 0 ? (size_t)1 : count; };
    const size_t in_bytes[5] = {sizeof(double) * n * models(in->c_stride), sizeof(double) * m * n * models(in->A_stride),
                                sizeof(double) * m * models(in->b_stride), in->lower ? sizeof(double) * n * models(in->lower_stride) : 0,
                                in->upper ? sizeof(double) * n * models(in->upper_stride) : 0};
    const void* in_src[5] = {in->c, in->A, in->b, in->lower, in->upper};
    const size_t out_bytes[6] = {sizeof(double) * count * n, sizeof(double) * count, sizeof(lpx_primal_record) * count,
                                 sizeof(int32_t) * count, sizeof(int32_t) * count * m, count * n};    // x, value, rec, status, basis, at_upper
    size_t in_off[5], out_off[6], at = 0;
    for (int k = 0; k < 5; ++k) { in_off[k] = at; at += up256(in_bytes[k]); }
    const size_t res0 = at;
    for (int k = 0; k < 6; ++k) { out_off[k] = at; at += up256(out_bytes[k]); }
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

    PackedParams p;
    std::memset(&p, 0, sizeof(p));
    p.c = reinterpret_cast<const double*>(a.dev + in_off[0]); p.A = reinterpret_cast<const double*>(a.dev + in_off[1]);
    p.b = reinterpret_cast<const double*>(a.dev + in_off[2]);
    p.lower = in->lower ? reinterpret_cast<const double*>(a.dev + in_off[3]) : nullptr;
    p.upper = in->upper ? reinterpret_cast<const double*>(a.dev + in_off[4]) : nullptr;
    p.c_stride = in->c_stride; p.A_stride = in->A_stride; p.b_stride = in->b_stride;
    p.lower_stride = in->lower_stride; p.upper_stride = in->upper_stride;
    p.m = in->m; p.n = in->n; p.min = in->sense == LPX_MIN ? 1 : 0; p.max_iter = o->max_iter;
    p.eps = o->eps; p.ratio_tol = o->ratio_tol;
    p.x = reinterpret_cast<double*>(a.dev + out_off[0]); p.value = reinterpret_cast<double*>(a.dev + out_off[1]);
    p.rec = reinterpret_cast<lpx_primal_record*>(a.dev + out_off[2]); p.status = reinterpret_cast<int32_t*>(a.dev + out_off[3]);
    p.basis = reinterpret_cast<int32_t*>(a.dev + out_off[4]); p.at_upper = reinterpret_cast<uint8_t*>(a.dev + out_off[5]);
    p.flip = reinterpret_cast<uint8_t*>(a.dev + flip_off); p.flip_stride = (int64_t)flip_stride;

    const double t0 = now_ms();
    for (int k = 0; k < 5; ++k)
        if (in_bytes[k]) LPX_HIP_TRY(hipMemcpyAsync(a.dev + in_off[k], in_src[k], in_bytes[k], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_primal_onchip, dim3((unsigned)count), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + res0, res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));       // the one wait
    const double ms = now_ms() - t0;

    const char* res = a.pin - res0;
    const lpx_primal_record* recs = reinterpret_cast<const lpx_primal_record*>(res + out_off[2]);
    std::memcpy(out->x, res + out_off[0], out_bytes[0]);
    std::memcpy(out->value, res + out_off[1], out_bytes[1]);
    std::memcpy(out->status, res + out_off[3], out_bytes[3]);
    if (out->rec) std::memcpy(out->rec, recs, out_bytes[2]);
    if (out->basis) std::memcpy(out->basis, res + out_off[4], out_bytes[4]);
    if (out->at_upper) std::memcpy(out->at_upper, res + out_off[5], out_bytes[5]);
    if (st) {
        std::memset(st, 0, sizeof(*st));
        for (size_t i = 0; i < count; ++i) st->pivots += recs[i].kind0 + recs[i].kind1;
        st->launches = 1; st->loop_ms = ms;
    }
    return 0;
}

}  // namespace lpx
