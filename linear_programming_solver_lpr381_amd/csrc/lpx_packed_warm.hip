// lpx_packed_warm.hip -- packed right-hand-side scenarios warm-started from one solved base (lpx_packed_base_open / _solve / _close,
// include/lpx.h), gfx950 (CDNA4, wave64).  A base model is solved once by the dual start of
// lpx_packed_dual.hip and its solved tableau, bounds, basis and flip bytes are kept on the device; count right-hand sides of that
// model are then re-solved in ONE launch, workgroup i continuing the dual loop from the base's optimal basis for scenario i.
//
// Two kernels, one text (pw_body<BASE>):
//   lpx_packed_base_onchip   ONE workgroup: steps 1, 2b, 5 and 6 of lpx_packed_dual.hip, statement for statement, then the snapshot
//                            (tile, ub, basis, flips, the shift constant) stored into the handle's allocation, then the extraction;
//   lpx_packed_warm_onchip   one workgroup x 1024 lanes per scenario: the snapshot copied into LDS, the RHS column moved by the
//                            slack block times delta, the same loop, the same extraction.
//
// Shared-device rules, those of lpx_packed_dual.hip:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic;
//   * every loop is bounded by max_iter, R, C, Cm, m or n; the dual loop tests the iteration limit first and every trip ends the loop
//     or makes at least one event, so a launch always ends;
//   * every value is written with ordinary vector stores from C++; there is no inline assembly beyond what lpx_onchip.h has;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.29).
//
// The arithmetic of a scenario: delta_k = b_i[k] - b0[k], negated for a >= row; for every row r = 0 .. m of the tile, the objective
// row included, one lane adds T[r][n + k] * delta_k to T[r][C - 1] for k ascending over the non-zero delta_k, one multiply and one
// add each.  The RHS column of a tableau is an affine function of the internal b whose linear part is the slack block, whatever
// pivots, complements and bound flips were made; the objective row and with it dual feasibility stay as the base left them.
//
// Dynamic LDS (doubles) is that of lpx_packed_dual.hip, so lpx_packed_fits is the fit rule unchanged:
//   tile [R * S]        R = m + 1, C = n + m + 1, row stride S = C | 1: odd, so the per-row sums of a scenario, lane r reading
//                       T[r][n + k], fall on 32 distinct banks per half wave
//   ub   [C]            upper bounds of the columns
//   buf  [max(R, C)]    the base: as in lpx_packed_dual.hip; a scenario: delta [m] in front of the loop; then the loop's and the
//                       extraction's scratch
// The snapshot has the layout of the LDS image (row stride S), so a scenario's copy is one coalesced sweep of R * S doubles.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h bnd_complement, rs_hysteresis and the reductions

#include <climits>
#include <cstring>
#include <mutex>

namespace lpx {

namespace {

// every output of a refused model or scenario zeroed, a record of zeros around the status (uniform: every lane takes it)
__device__ __forceinline__ void pw_refuse(const PackedWarmParams& N, size_t mdl, int t)
{
    const int m = N.m, n = N.n;
    double* const gx = N.x + mdl * (size_t)n;
    uint8_t* const gat = N.at_upper + mdl * (size_t)n;
    double* const gd = N.d + mdl * (size_t)n;
    double* const gy = N.y + mdl * (size_t)m;
    int32_t* const basis = N.basis + mdl * (size_t)m;
    for (int j = t; j < n; j += OC_NT) { gx[j] = 0.0; gat[j] = 0; gd[j] = 0.0; }
    for (int i = t; i < m; i += OC_NT) { basis[i] = 0; gy[i] = 0.0; }
    if (t == 0) {
        N.status[mdl] = LPX_EINVAL; N.value[mdl] = 0.0;
        lpx_packed_dual_record* o = N.rec + mdl;
        o->status = LPX_EINVAL; o->events = 0; o->kind0 = 0; o->kind1 = 0; o->passes = 0; o->dualize_flips = 0; o->z = 0.0;
    }
}

template <bool BASE>
__device__ __forceinline__ void pw_body(const PackedWarmParams& N, double* pd_lds)
{
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
    const bool min = N.min != 0, has_lower = N.snap.lower != nullptr;
    const bool skip_fixed = false, cut = false, long_step = N.long_step != 0;

    const double* const glo = N.snap.lower;
    const int32_t* const grel = N.snap.rel;
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

    int nflips = 0;
    bool dirty = false;                                 // a dead local: nothing is stored back
    if constexpr (BASE) {
        const double* const gc = N.c;
        const double* const gA = N.A;
        const double* const gb = N.snap.b0;
        const double* const gup = N.upper;
        // ---- 1. the tableau of the model into LDS.  The bounds and the row senses first, with the host path's checks
        int bad = 0;
        for (int j = t; j < n; j += OC_NT) {
            const double l = has_lower ? glo[j] : 0.0;
            const double u = gup ? gup[j] : inf;
            if (!(__builtin_fabs(l) < inf) || !(u >= l)) bad = 1;
            buf[j] = l;
            ub_s[j] = gup ? (__builtin_isinf(u) ? u : u - l) : inf;
            double cj = gc[j];
            if (min) cj = -cj;                          // Min negates c ...
            zrow[j] = -cj;                              // ... and the objective row is the negation of that: a zero cost gives -0.0
            flip[j] = 0;
        }
        for (int j = n + t; j < Cm; j += OC_NT) { ub_s[j] = inf; flip[j] = 0; }
        if (grel)
            for (int i = t; i < m; i += OC_NT) { const int r = grel[i]; if (r != LPX_LE && r != LPX_GE) bad = 1; }
        // A, coalesced over the whole m x n block.  A >= row is negated here, in front of the lower shift: only signs change
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
            const int i = k / R, jj = k - i * R;        // column n + jj; jj = m is the RHS column
            double v = (i < m && jj == i) ? 1.0 : 0.0;
            if (i < m && jj == m) { const double bi = gb[i]; v = (grel && grel[i] == LPX_GE) ? -bi : bi; }
            tile[(size_t)i * S + n + jj] = v;
        }
        for (int i = t; i < m; i += OC_NT) basis[i] = n + i;
        if (__syncthreads_or(bad)) { pw_refuse(N, mdl, t); return; }       // uniform
        // x = l + x': b' = b - A l from LDS over the rows as they are stored, one lane per row, j ascending, one multiply and one
        // subtract per non-zero l_j; a lane without a row sums c.l over the user's c the same way
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
            if (t == (((m + 63) >> 6) << 6)) {          // the first lane of the first wave without a row (m <= 139 under the fit rule)
                double constant = 0.0; int shifted = 0;
                for (int j = 0; j < n; ++j) {
                    const double l = buf[j];
                    if (l != 0.0) { const double cu = min ? zrow[j] : -zrow[j]; const double prod = cu * l; constant = constant + prod; shifted = 1; }
                }
                s_const = constant; s_shifted = shifted;
            }
        } else if (t == 0) { s_const = 0.0; s_shifted = 0; }
        __syncthreads();                                // the tile, ub and the flip bytes stand; the lower bounds in buf are dead

        // ---- 2b. the count of the dual-feasibility flips and of the columns no flip can repair, 5. the flips: both with the
        // tolerance of lpx_tableau_dualize(1e-9), whatever the loop's eps is
        {
            const double eps = 1e-9;
            int32_t* list = reinterpret_cast<int32_t*>(buf);
            int unrepairable = 0;
            {
#include "lpx_onchip_count.h"
                nflips = n; unrepairable = bad;
            }
            if (unrepairable > 0) { pw_refuse(N, mdl, t); return; }        // uniform: the precheck of lpx_solve_bounded_dual
#include "lpx_onchip_flips.h"
        }
    } else {
        // ---- 1. the base's tile and ub into LDS, its basis and flip bytes into this scenario's slices: the snapshot has the
        // layout of the LDS image, so lane t reads element t and steps by the workgroup
        const double* const gb = N.b + mdl * (size_t)m;
        for (int k = t; k < R * S; k += OC_NT) tile[k] = N.snap.tile[k];
        for (int j = t; j < C; j += OC_NT) ub_s[j] = N.snap.ub[j];
        for (int j = t; j < Cm; j += OC_NT) flip[j] = N.snap.flip[j];
        for (int i = t; i < m; i += OC_NT) basis[i] = N.snap.basis[i];
        // ---- 2. delta in buf; a right-hand side that is not finite refuses the scenario
        int bad = 0;
        for (int k = t; k < m; k += OC_NT) {
            const double bi = gb[k];
            if (!(__builtin_fabs(bi) < inf)) bad = 1;
            const double dk = bi - N.snap.b0[k];
            buf[k] = (grel && grel[k] == LPX_GE) ? -dk : dk;
        }
        if (t == 0) { s_const = *N.snap.constant; s_shifted = *N.snap.shifted; }
        if (__syncthreads_or(bad)) { pw_refuse(N, mdl, t); return; }       // uniform
        // ---- 3. the RHS column, the objective row included: one lane per row (R <= 140 lanes), k ascending, one multiply and
        // one add per non-zero delta_k.  A lane reads and writes its own row only
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
    }

    // ---- 6. the dual loop: from the slack basis (the base) or from the base's basis (a scenario)
    int32_t* const trace = nullptr;
    const int trace_cap = 0;
#include "lpx_onchip_dual.h"
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane
    (void)dirty; (void)cutoff; (void)stall_events; (void)s_tot; (void)s_bad;

    if constexpr (BASE) {
        // ---- the snapshot, in front of the extraction (which marks the basic columns in the flip bytes).  A padding column
        // (S > C) is stored as 0.0: LDS holds nothing there
        for (int k = t; k < R * S; k += OC_NT) { const int j = k % S; N.snap.tile[k] = j < C ? tile[k] : 0.0; }
        for (int j = t; j < C; j += OC_NT) N.snap.ub[j] = ub_s[j];
        for (int j = t; j < Cm; j += OC_NT) N.snap.flip[j] = flip[j];
        for (int i = t; i < m; i += OC_NT) N.snap.basis[i] = basis[i];
        if (t == 0) { *N.snap.constant = s_const; *N.snap.shifted = s_shifted; }
        __syncthreads();
    }

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

}  // namespace

__global__ __launch_bounds__(OC_NT) void lpx_packed_base_onchip(PackedWarmParams N)
{
    extern __shared__ double pw_lds[];
    pw_body<true>(N, pw_lds);
}

__global__ __launch_bounds__(OC_NT) void lpx_packed_warm_onchip(PackedWarmParams N)
{
    extern __shared__ double pw_lds[];
    pw_body<false>(N, pw_lds);
}

// ---- the host side: the arena, the pinned block and the stream of lpx_packed.hip (g_packed, lpx_internal.h); the snapshot is an
// allocation of its own that lives as long as its handle ------------------------------------------------------------------------
namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

bool g_attr_base = false, g_attr_warm = false;          // the function attributes are set (under g_packed.mu)

// the results of a call in the order of the pinned block: x, value, rec, status, basis, at_upper, y, d
struct WarmLayout {
    size_t in_off[3], in_bytes[3], out_off[8], out_bytes[8], res0, res_bytes, flip_off, flip_stride, total;
};

WarmLayout warm_layout(size_t count, size_t m, size_t n, const size_t in_bytes[3])
{
    WarmLayout L;
    size_t at = 0;
    for (int k = 0; k < 3; ++k) { L.in_bytes[k] = in_bytes[k]; L.in_off[k] = at; at += up256(in_bytes[k]); }
    const size_t ob[8] = {sizeof(double) * count * n, sizeof(double) * count, sizeof(lpx_packed_dual_record) * count,
                          sizeof(int32_t) * count, sizeof(int32_t) * count * m, count * n,
                          sizeof(double) * count * m, sizeof(double) * count * n};
    L.res0 = at;
    for (int k = 0; k < 8; ++k) { L.out_bytes[k] = ob[k]; L.out_off[k] = at; at += up256(ob[k]); }
    L.res_bytes = at - L.res0;
    L.flip_stride = (n + m + 15) & ~(size_t)15;
    L.flip_off = at; at += up256(count * L.flip_stride);
    L.total = at;
    return L;
}

int warm_grow(PackedArena& a, const WarmLayout& L)
{
    if (L.total > a.dev_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.dev) hipFree(a.dev);
        a.dev = nullptr; a.dev_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&a.dev, L.total));
        a.dev_bytes = L.total;
    }
    if (L.res_bytes > a.pin_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.pin) hipHostFree(a.pin);
        a.pin = nullptr; a.pin_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&a.pin, L.res_bytes));
        a.pin_bytes = L.res_bytes;
    }
    return 0;
}

void warm_outputs(PackedWarmParams& p, const PackedArena& a, const WarmLayout& L)
{
    p.x = reinterpret_cast<double*>(a.dev + L.out_off[0]); p.value = reinterpret_cast<double*>(a.dev + L.out_off[1]);
    p.rec = reinterpret_cast<lpx_packed_dual_record*>(a.dev + L.out_off[2]); p.status = reinterpret_cast<int32_t*>(a.dev + L.out_off[3]);
    p.basis = reinterpret_cast<int32_t*>(a.dev + L.out_off[4]); p.at_upper = reinterpret_cast<uint8_t*>(a.dev + L.out_off[5]);
    p.y = reinterpret_cast<double*>(a.dev + L.out_off[6]); p.d = reinterpret_cast<double*>(a.dev + L.out_off[7]);
    p.flip = reinterpret_cast<uint8_t*>(a.dev + L.flip_off); p.flip_stride = (int64_t)L.flip_stride;
}

// the pinned block handed out; returns the records
const lpx_packed_dual_record* warm_hand_out(const PackedArena& a, const WarmLayout& L, const lpx_packed_dual_results* out)
{
    const char* res = a.pin - L.res0;
    const lpx_packed_dual_record* recs = reinterpret_cast<const lpx_packed_dual_record*>(res + L.out_off[2]);
    if (!out) return recs;
    std::memcpy(out->x, res + L.out_off[0], L.out_bytes[0]);
    std::memcpy(out->value, res + L.out_off[1], L.out_bytes[1]);
    std::memcpy(out->status, res + L.out_off[3], L.out_bytes[3]);
    if (out->rec) std::memcpy(out->rec, recs, L.out_bytes[2]);
    if (out->basis) std::memcpy(out->basis, res + L.out_off[4], L.out_bytes[4]);
    if (out->at_upper) std::memcpy(out->at_upper, res + L.out_off[5], L.out_bytes[5]);
    if (out->y) std::memcpy(out->y, res + L.out_off[6], L.out_bytes[6]);
    if (out->d) std::memcpy(out->d, res + L.out_off[7], L.out_bytes[7]);
    return recs;
}

}  // namespace

void packed_base_close(PackedBase* base)
{
    if (base->dev) hipFree(base->dev);
    *base = PackedBase();
}

int packed_base_open(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* base_out, PackedBase* base)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t m = (size_t)in->m, n = (size_t)in->n;
    const int R = in->m + 1, C = in->n + in->m + 1;
    if (!bounded_node_fits(R, C) || in->m > OC_NT - 64) { set_error("lpx_packed_base_open: the shape does not fit"); return LPX_EINVAL; }   // never launched beyond one compute unit
    const size_t S = (size_t)(C | 1);

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!g_attr_base) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_base_onchip))); g_attr_base = true; }

    // the snapshot: the doubles, the int32, the bytes
    const size_t snap_bytes[9] = {sizeof(double) * (size_t)R * S, sizeof(double) * (size_t)C, sizeof(double) * m,
                                  in->lower ? sizeof(double) * n : 0, sizeof(double),
                                  sizeof(int32_t) * m, in->rel ? sizeof(int32_t) * m : 0, sizeof(int32_t), (size_t)C - 1};
    size_t snap_off[9], snap_total = 0;
    for (int k = 0; k < 9; ++k) { snap_off[k] = snap_total; snap_total += up256(snap_bytes[k]); }
    LPX_HIP_TRY(hipMalloc((void**)&base->dev, snap_total));
    base->dev_bytes = snap_total; base->m = in->m; base->n = in->n; base->min = in->sense == LPX_MIN ? 1 : 0;
    PackedBaseSnap& sn = base->snap;
    sn.tile = reinterpret_cast<double*>(base->dev + snap_off[0]); sn.ub = reinterpret_cast<double*>(base->dev + snap_off[1]);
    sn.b0 = reinterpret_cast<double*>(base->dev + snap_off[2]);
    sn.lower = in->lower ? reinterpret_cast<double*>(base->dev + snap_off[3]) : nullptr;
    sn.constant = reinterpret_cast<double*>(base->dev + snap_off[4]);
    sn.basis = reinterpret_cast<int32_t*>(base->dev + snap_off[5]);
    sn.rel = in->rel ? reinterpret_cast<int32_t*>(base->dev + snap_off[6]) : nullptr;
    sn.shifted = reinterpret_cast<int32_t*>(base->dev + snap_off[7]);
    sn.flip = reinterpret_cast<uint8_t*>(base->dev + snap_off[8]);

    // the arena: c, A and upper, the results in the order of the pinned block, the flip bytes
    const size_t in_bytes[3] = {sizeof(double) * n, sizeof(double) * m * n, in->upper ? sizeof(double) * n : 0};
    const void* in_src[3] = {in->c, in->A, in->upper};
    const WarmLayout L = warm_layout(1, m, n, in_bytes);
    rc = warm_grow(a, L); if (rc) return rc;

    PackedWarmParams p;
    std::memset(&p, 0, sizeof(p));
    p.c = reinterpret_cast<const double*>(a.dev + L.in_off[0]); p.A = reinterpret_cast<const double*>(a.dev + L.in_off[1]);
    p.upper = in->upper ? reinterpret_cast<const double*>(a.dev + L.in_off[2]) : nullptr;
    p.snap = sn;
    p.m = in->m; p.n = in->n; p.min = base->min; p.max_iter = o->max_iter;
    p.long_step = (flags & LPX_BDUAL_LONG_STEP) ? 1 : 0;
    p.eps = o->eps; p.ratio_tol = o->ratio_tol;
    warm_outputs(p, a, L);

    for (int k = 0; k < 3; ++k)
        if (in_bytes[k]) LPX_HIP_TRY(hipMemcpyAsync(a.dev + L.in_off[k], in_src[k], in_bytes[k], hipMemcpyHostToDevice, a.stream));
    LPX_HIP_TRY(hipMemcpyAsync(sn.b0, in->b, snap_bytes[2], hipMemcpyHostToDevice, a.stream));
    if (in->lower) LPX_HIP_TRY(hipMemcpyAsync(sn.lower, in->lower, snap_bytes[3], hipMemcpyHostToDevice, a.stream));
    if (in->rel) LPX_HIP_TRY(hipMemcpyAsync(sn.rel, in->rel, snap_bytes[6], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_base_onchip, dim3(1), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + L.res0, L.res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));
    const lpx_packed_dual_record* recs = warm_hand_out(a, L, base_out);
    const int status = recs[0].status;
    if (status == LPX_EINVAL)
        set_error("lpx_packed_base_open: the base model was refused (a bound, a rel entry, or an improving variable without an upper bound)");
    else if (status != LPX_OPTIMAL)
        set_error(std::string("lpx_packed_base_open: the base model is ") + (status == LPX_INFEASIBLE ? "infeasible" : "at the iteration limit"));
    return status;
}

int packed_base_solve(const PackedBase* base, int32_t count32, const double* b, int flags, const lpx_run_opts* o,
                      const lpx_packed_dual_results* out, lpx_stats* st)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t count = (size_t)count32, m = (size_t)base->m, n = (size_t)base->n;
    const int R = base->m + 1, C = base->n + base->m + 1;

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!g_attr_warm) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_warm_onchip))); g_attr_warm = true; }

    // the arena: b, the results in the order of the pinned block, the flip bytes
    const size_t in_bytes[3] = {sizeof(double) * count * m, 0, 0};
    const WarmLayout L = warm_layout(count, m, n, in_bytes);
    rc = warm_grow(a, L); if (rc) return rc;

    PackedWarmParams p;
    std::memset(&p, 0, sizeof(p));
    p.b = reinterpret_cast<const double*>(a.dev + L.in_off[0]);
    p.snap = base->snap;
    p.m = base->m; p.n = base->n; p.min = base->min; p.max_iter = o->max_iter;
    p.long_step = (flags & LPX_BDUAL_LONG_STEP) ? 1 : 0;
    p.eps = o->eps; p.ratio_tol = o->ratio_tol;
    warm_outputs(p, a, L);

    const double t0 = now_ms();
    LPX_HIP_TRY(hipMemcpyAsync(a.dev + L.in_off[0], b, in_bytes[0], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_warm_onchip, dim3((unsigned)count), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + L.res0, L.res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));       // the one wait
    const double ms = now_ms() - t0;

    const lpx_packed_dual_record* recs = warm_hand_out(a, L, out);
    if (st) {
        std::memset(st, 0, sizeof(*st));
        for (size_t i = 0; i < count; ++i) st->pivots += recs[i].kind0 + recs[i].kind1;
        st->launches = 1; st->loop_ms = ms;
    }
    return 0;
}

}  // namespace lpx
