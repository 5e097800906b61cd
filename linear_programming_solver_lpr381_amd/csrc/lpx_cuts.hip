// lpx_cuts.hip -- one round of Gomory mixed-integer (GMI) cuts on a device tableau (lpx_tableau_gmi_round, include/lpx.h,
// where the round is defined bit for bit).  Three launches, none of which reads what it writes:
//
//   gmi_scan   one wave per row.  Rows that are no candidates (basic column not integer, or f0 = frac(b_r) outside
//              [away, 1 - away]) are decided from the RHS column, the basis and the integer mask and exit at once; a
//              candidate row is read once with 16-byte nontemporal loads and reduced to max alpha / min nonzero alpha
//              (exact min / max reductions: the result does not depend on the order).  The nonbasic and integer masks
//              of the columns are bit masks in LDS, built from the device basis and the uploaded integer mask.
//   gmi_pick   one workgroup: the dynamism filter, the K picks in rank order, the purge plan from the basis and the RHS
//              column, the row / column maps and the new basis.  The plan record is what the host reads back (counts,
//              source rows, purged columns).
//   gmi_apply  without purges: in place.  One thread per column j < C-1 writes the objective row moved down K rows and the
//              K cut rows at that column (it reads old row m before it writes cut row 0 over it); one thread per old row
//              owns that row's tail (K new zero slack entries and the moved RHS), one thread the tails of the new rows.
//              With purges: one compacting pass into the handle's second tableau buffer, copied back by the host.
//
// The round on a handle with bounds (lpx_tableau_gmi_round_bounded) is the same three launches on the internal representation,
// between two small ones of its own:
//   gmi_mask_bounded   in front: the round's integer array from the caller's flags and the handle's lo / ub (a flagged column
//                      with a fractional bound is continuous).
//   gmi_carry_inplace  behind gmi_apply_inplace: the ub / lo / flip tails of the K new slacks and the contiguous copy of the new
//                      RHS column (rhsbuf); it writes only entries no earlier launch of the round has read.
//   gmi_carry_purge    behind gmi_apply_purge: ub / lo / flip gathered through the plan's column map into staging and the RHS
//                      column of the second buffer into rhsbuf; the host copies the staging back.
// They hold to the shared-device rules at the head of lpx_bounded_primal.hip: no workgroup waits on another, every loop is bounded
// by R or Ccap, plain vector stores, no scratch (resource remarks: DESIGN.md section 4.23).
#include "lpx_append.h"
#include "lpx_block.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace lpx {

static constexpr int GS_NT = 256;            // scan: 4 waves
static constexpr int GS_RPB = 4;             // rows per scan workgroup (one per wave)
static constexpr int GS_NV = 8;              // 16-byte loads in flight per lane
static constexpr int GP_NT = 1024;           // pick: one workgroup
static constexpr int GA_NT = 256;            // apply
static constexpr int GMI_KMAX = 64;          // cuts per round
static constexpr int GMI_PMAX = 2048;        // cut columns a round may purge from
static constexpr int GMI_CMAX = 131072;      // widest handle: nonbasic + integer bit masks of 32 KB in LDS

typedef double gm_d2 __attribute__((ext_vector_type(2)));

struct GmiParams {
    double away, coef_eps, max_dyn, purge_tol;
    int kcap, purge, first_cut, pad;
};

// plan record (device), header read back by the host
struct GmiPlan {
    int ncand, npass, K, P, R2, C2, pad[2];
    int32_t src[GMI_KMAX];
    double f0[GMI_KMAX];
};

__device__ __forceinline__ double gmi_alpha(double a, bool integer, double f0, double ce)
{
    if (integer) {
        const double f = a - floor(a);
        if (f <= ce || f >= 1.0 - ce) return 0.0;
        return f <= f0 ? f / f0 : (1.0 - f) / (1.0 - f0);
    }
    if (fabs(a) <= ce) return 0.0;
    return a > 0 ? a / f0 : -a / (1.0 - f0);
}

// rows: flag (1 = candidate), f0, max alpha, min nonzero alpha (+inf: none), b
__global__ __launch_bounds__(GS_NT) void gmi_scan(const double* __restrict__ T, int ld, int m, int Cm,
                                                  const int32_t* __restrict__ basis, const uint8_t* __restrict__ isint,
                                                  GmiParams g, int32_t* __restrict__ flag, double* __restrict__ f0o,
                                                  double* __restrict__ amaxo, double* __restrict__ amino, double* __restrict__ bo)
{
    extern __shared__ unsigned s_nb[];        // nonbasic bits of the columns [0, Cm), then their integer bits
    __shared__ int s_cand[GS_RPB];
    __shared__ double s_f0[GS_RPB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * GS_RPB;
    if (tid < GS_RPB) {
        const int r = r0 + tid;
        int c = 0; double f0 = 0.0;
        if (r < m) {
            const double b = T[(size_t)r * ld + Cm];
            const int j = basis[r];
            f0 = b - floor(b);
            c = j >= 0 && j < Cm && isint[j] && f0 >= g.away && f0 <= 1.0 - g.away;
            bo[r] = b; flag[r] = c; f0o[r] = f0;
            if (!c) { amaxo[r] = 0.0; amino[r] = __builtin_inf(); }
        }
        s_cand[tid] = c; s_f0[tid] = f0;
    }
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int k = 0; k < GS_RPB; ++k) any |= s_cand[k];
    if (!any) return;                          // uniform over the workgroup

    const int nw = (Cm + 31) >> 5;
    unsigned* s_int = s_nb + nw;
    for (int k = tid; k < nw; k += GS_NT) {
        const int rem = Cm - 32 * k;
        s_nb[k] = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
        unsigned w = 0;
        for (int i = 0; i < 32 && i < rem; ++i) w |= (isint[32 * k + i] ? 1u : 0u) << i;
        s_int[k] = w;
    }
    __syncthreads();
    for (int r = tid; r < m; r += GS_NT) {
        const int j = basis[r];
        if (j >= 0 && j < Cm) atomicAnd(&s_nb[j >> 5], ~(1u << (j & 31)));
    }
    __syncthreads();

    const double ce = g.coef_eps;
    for (int k = wave; k < GS_RPB; k += GS_NT / 64) {
        if (!s_cand[k]) continue;
        const int r = r0 + k;
        const double f0 = s_f0[k];
        const double* row = T + (size_t)r * ld;
        double mx = 0.0, mn = __builtin_inf();
        for (int c0 = 0; c0 < Cm; c0 += 128 * GS_NV) {
            gm_d2 x[GS_NV];
#pragma unroll
            for (int v = 0; v < GS_NV; ++v) {
                const int c = c0 + 128 * v + 2 * lane;          // c + 1 <= Cm < ld: inside the row
                x[v] = gm_d2{0.0, 0.0};
                if (c < Cm) x[v] = __builtin_nontemporal_load(reinterpret_cast<const gm_d2*>(row + c));
            }
#pragma unroll
            for (int v = 0; v < GS_NV; ++v) {
                const int c = c0 + 128 * v + 2 * lane;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int j = c + e;
                    if (j < Cm && ((s_nb[j >> 5] >> (j & 31)) & 1u)) {
                        const double al = gmi_alpha(e ? x[v].y : x[v].x, (s_int[j >> 5] >> (j & 31)) & 1u, f0, ce);
                        if (al > mx) mx = al;
                        if (al > 0 && al < mn) mn = al;
                    }
                }
            }
        }
        mx = -wave_min_f64(-mx);
        mn = wave_min_f64(mn);
        if (lane == 0) { amaxo[r] = mx; amino[r] = mn; }
    }
}

// exclusive rank of an index list entry in ascending order (the entries are distinct)
__device__ __forceinline__ int gmi_rank(const int32_t* s, int n, int v)
{
    int k = 0;
    for (int i = 0; i < n; ++i) k += s[i] < v;
    return k;
}

__global__ __launch_bounds__(GP_NT) void gmi_pick(int m, int Cm, int Rcap, int Ccap, const int32_t* __restrict__ basis,
                                                  const int32_t* __restrict__ flag, const double* __restrict__ f0,
                                                  const double* __restrict__ amax, const double* __restrict__ amin,
                                                  const double* __restrict__ b, GmiParams g, GmiPlan* __restrict__ plan,
                                                  int32_t* __restrict__ pcol_out, int32_t* __restrict__ rowsrc,
                                                  int32_t* __restrict__ colsrc, int32_t* __restrict__ nbasis,
                                                  uint8_t* __restrict__ nbm)
{
    extern __shared__ unsigned s_nb[];        // nonbasic bits of the columns [0, Cm)
    __shared__ int32_t s_rowof[GMI_PMAX];     // row in which cut column first_cut + i is basic, -1 = nonbasic
    __shared__ int32_t s_prow[GMI_PMAX], s_pcol[GMI_PMAX], s_sprow[GMI_PMAX];
    __shared__ int32_t s_src[GMI_KMAX];
    __shared__ double s_f0[GMI_KMAX];
    __shared__ double s_v[GP_NT / 64];
    __shared__ int s_i[GP_NT / 64];
    __shared__ int s_K, s_npass, s_ncand;
    const int tid = threadIdx.x;
    const int R = m + 1, C = Cm + 1;
    const int ncut = Cm - g.first_cut;

    // nonbasic mask, rows of the basic cut columns
    const int nw = (Cm + 31) >> 5;
    for (int k = tid; k < nw; k += GP_NT) {
        const int rem = Cm - 32 * k;
        s_nb[k] = rem >= 32 ? 0xffffffffu : ((1u << rem) - 1u);
    }
    for (int i = tid; i < ncut; i += GP_NT) s_rowof[i] = -1;
    __syncthreads();
    for (int r = tid; r < m; r += GP_NT) {
        const int j = basis[r];
        if (j >= 0 && j < Cm) atomicAnd(&s_nb[j >> 5], ~(1u << (j & 31)));
        if (j >= g.first_cut && j < Cm) s_rowof[j - g.first_cut] = r;
    }
    // counts of candidates and of rows that pass the filter
    int nc = 0, np = 0;
    for (int r = tid; r < m; r += GP_NT)
        if (flag[r]) { ++nc; if (!(amax[r] > g.max_dyn * amin[r])) ++np; }
    __syncthreads();
    {
        int tot = 0;
        (void)block_excl_scan_sum<GP_NT>(nc, s_i, &tot);
        if (tid == 0) s_ncand = tot;
        (void)block_excl_scan_sum<GP_NT>(np, s_i, &tot);
        if (tid == 0) s_npass = tot;
    }
    // purge list in ascending column order (the cut columns are walked in order)
    int P = 0;
    for (int base = 0; base < ncut; base += GP_NT) {
        const int i = base + tid;
        int pr = -1;
        if (g.purge && i < ncut) { const int r = s_rowof[i]; if (r >= 0 && b[r] > g.purge_tol) pr = r; }
        int tot = 0;
        const int pos = block_excl_scan_sum<GP_NT>(pr >= 0 ? 1 : 0, s_i, &tot);
        if (pr >= 0) { s_prow[P + pos] = pr; s_pcol[P + pos] = g.first_cut + i; }
        P += tot;
    }
    __syncthreads();
    // purged rows ascending
    for (int i = tid; i < P; i += GP_NT) s_sprow[gmi_rank(s_prow, P, s_prow[i])] = s_prow[i];
    if (tid == 0) {
        int K = g.kcap;
        K = min(K, Rcap - (R - P));
        K = min(K, Ccap - (C - P));
        K = min(K, s_npass);
        s_K = K > 0 ? K : 0;
    }
    __syncthreads();
    const int K = s_K;

    // the K picks: smallest (|f0 - 0.5|, r) among passing rows, each strictly after the previous pick
    double pk = -1.0; int pr = -1;
    for (int k = 0; k < K; ++k) {
        MinIdx best{__builtin_inf(), INT_MAX};
        for (int r = tid; r < m; r += GP_NT) {
            if (!flag[r] || amax[r] > g.max_dyn * amin[r]) continue;
            const double key = fabs(f0[r] - 0.5);
            if (key < pk || (key == pk && r <= pr)) continue;
            if (key < best.v || (key == best.v && r < best.i)) { best.v = key; best.i = r; }
        }
        best = block_min_idx<GP_NT>(best, s_v, s_i);
        pk = best.v; pr = best.i;
        if (tid == 0) { s_src[k] = pr; s_f0[k] = f0[pr]; }
    }
    __syncthreads();

    const int R2 = R - P + K, C2 = C - P + K, m2 = R2 - 1, Cm2 = C2 - 1;
    if (tid == 0) {
        plan->ncand = s_ncand; plan->npass = s_npass; plan->K = K; plan->P = P; plan->R2 = R2; plan->C2 = C2;
    }
    for (int k = tid; k < K; k += GP_NT) { plan->src[k] = s_src[k]; plan->f0[k] = s_f0[k]; }
    for (int i = tid; i < P; i += GP_NT) pcol_out[i] = s_pcol[i];
    for (int j = tid; j < Cm; j += GP_NT) nbm[j] = (s_nb[j >> 5] >> (j & 31)) & 1u;
    // the new basis and, for the compacting pass only (P > 0), the maps new index -> old index (-1 - k = cut k / slack k)
    for (int i = tid; i < R2; i += GP_NT) {
        int s;
        if (i < m - P) { s = i; for (int q = 0; q < P; ++q) if (s_sprow[q] <= s) ++s; }
        else if (i < m2) s = -1 - (i - (m - P));
        else s = m;
        if (P > 0) rowsrc[i] = s;
        if (i < m2) {
            if (s >= 0) { const int j = basis[s]; nbasis[i] = j - gmi_rank(s_pcol, P, j); }
            else nbasis[i] = Cm - P + (-1 - s);
        }
    }
    for (int j = tid; P > 0 && j < C2; j += GP_NT) {
        int c;
        if (j < Cm - P) { c = j; for (int q = 0; q < P; ++q) if (s_pcol[q] <= c) ++c; }
        else if (j < Cm2) c = -1 - (j - (Cm - P));
        else c = Cm;
        colsrc[j] = c;
    }
}

// the K cut rows of a round as append_rows_inplace (lpx_append.h) writes them: -alpha over the old columns, the unit
// vector of the row's own slack, -1 in the RHS
struct GmiNewRows {
    const double* T; int ld;
    const int32_t* src; const double* f0;       // LDS copies of the plan
    const uint8_t* nbm; const uint8_t* isint; double ce;
    __device__ double body(int k, int j) const
    {
        const double a = T[(size_t)src[k] * ld + j];
        const double al = nbm[j] ? gmi_alpha(a, isint[j] != 0, f0[k], ce) : 0.0;
        return al == 0.0 ? 0.0 : -al;
    }
    __device__ double slack(int k, int i) const { return i == k ? 1.0 : 0.0; }
    __device__ double rhs(int) const { return -1.0; }
};

// In place (no purge): blocks [0, ncb) own the columns j < Cm of the new rows, the rest the tails and the basis.
__global__ __launch_bounds__(GA_NT) void gmi_apply_inplace(double* __restrict__ T, int ld, int m, int Cm, int ncb,
                                                           const GmiPlan* __restrict__ plan, const uint8_t* __restrict__ nbm,
                                                           const uint8_t* __restrict__ isint, const int32_t* __restrict__ nbasis,
                                                           int32_t* __restrict__ basis, double ce)
{
    __shared__ int32_t s_src[GMI_KMAX];
    __shared__ double s_f0[GMI_KMAX];
    const int K = plan->K;
    if ((int)blockIdx.x < ncb) {
        for (int k = threadIdx.x; k < K; k += GA_NT) { s_src[k] = plan->src[k]; s_f0[k] = plan->f0[k]; }
        __syncthreads();
    }
    const GmiNewRows rows{T, ld, s_src, s_f0, nbm, isint, ce};
    const int r = append_rows_inplace(T, ld, m, Cm, K, ncb, GA_NT, rows);
    if (r >= 0 && r < m + K) basis[r] = nbasis[r];
}

// With purges: the new R2 x C2 tableau gathered into T2 (blockIdx.y strides the rows), the new basis from the plan.
__global__ __launch_bounds__(GA_NT) void gmi_apply_purge(const double* __restrict__ T, double* __restrict__ T2, int ld, int Cm,
                                                         int R2, int C2, const GmiPlan* __restrict__ plan,
                                                         const int32_t* __restrict__ rowsrc, const int32_t* __restrict__ colsrc,
                                                         const uint8_t* __restrict__ nbm, const uint8_t* __restrict__ isint,
                                                         const int32_t* __restrict__ nbasis, int32_t* __restrict__ basis, double ce)
{
    const int j = blockIdx.x * GA_NT + threadIdx.x;
    if (blockIdx.y == 0 && j < R2 - 1) basis[j] = nbasis[j];
    if (j >= C2) return;
    const int c = colsrc[j];
    for (int i = blockIdx.y; i < R2; i += gridDim.y) {
        const int s = rowsrc[i];
        double v;
        if (s >= 0) v = c >= 0 ? T[(size_t)s * ld + c] : 0.0;
        else {
            const int k = -1 - s;
            if (c == Cm) v = -1.0;
            else if (c < 0) v = -1 - c == k ? 1.0 : 0.0;
            else {
                const double al = nbm[c] ? gmi_alpha(T[(size_t)plan->src[k] * ld + c], isint[c] != 0, plan->f0[k], ce) : 0.0;
                v = al == 0.0 ? 0.0 : -al;
            }
        }
        T2[(size_t)i * ld + j] = v;
    }
}

// ---- the round on a handle with bounds -----------------------------------------------------------------------------------
// isint[j] for j < Cm: flagged (flags[j], j < nint) and both bounds of the column whole.  lo == nullptr: a handle without bounds.
__global__ __launch_bounds__(GA_NT) void gmi_mask_bounded(int Cm, int nint, const uint8_t* __restrict__ flags,
                                                          const double* __restrict__ lo, const double* __restrict__ ub,
                                                          uint8_t* __restrict__ isint)
{
    const int j = blockIdx.x * GA_NT + threadIdx.x;
    if (j >= Cm) return;
    bool whole = j < nint && flags[j] != 0;
    if (whole && lo) {
        const double l = lo[j], u = ub[j];
        whole = l == floor(l) && (u == __builtin_inf() || u == floor(u));
    }
    isint[j] = whole ? 1 : 0;
}

// In place: new slack k < K is column Cm + k (Cm + K <= Ccap - 1 by the round's capacity rule); rhsbuf[i] = new T[i, Cm + K].
__global__ __launch_bounds__(GA_NT) void gmi_carry_inplace(const double* __restrict__ T, int ld, int R2, int Cm,
                                                           const GmiPlan* __restrict__ plan, double* __restrict__ ub,
                                                           double* __restrict__ lo, uint8_t* __restrict__ flip,
                                                           double* __restrict__ rhsbuf)
{
    const int K = plan->K;
    const int i = blockIdx.x * GA_NT + threadIdx.x;
    if (i < K) { ub[Cm + i] = __builtin_inf(); lo[Cm + i] = 0.0; flip[Cm + i] = 0; }
    if (i < R2) rhsbuf[i] = T[(size_t)i * ld + Cm + K];
}

// With purges: entry j < Ccap of the staging arrays from the column map (a new slack, the RHS column and everything beyond the
// new live shape: unbounded, unshifted, unflipped); rhsbuf[i] = T2[i, C2 - 1].
__global__ __launch_bounds__(GA_NT) void gmi_carry_purge(const double* __restrict__ T2, int ld, int R2, int C2, int Ccap,
                                                         const int32_t* __restrict__ colsrc, const double* __restrict__ ub,
                                                         const double* __restrict__ lo, const uint8_t* __restrict__ flip,
                                                         double* __restrict__ ub2, double* __restrict__ lo2,
                                                         uint8_t* __restrict__ flip2, double* __restrict__ rhsbuf)
{
    const int j = blockIdx.x * GA_NT + threadIdx.x;
    if (j < Ccap) {
        const int c = j < C2 - 1 ? colsrc[j] : -1;
        ub2[j] = c >= 0 ? ub[c] : __builtin_inf();
        lo2[j] = c >= 0 ? lo[c] : 0.0;
        flip2[j] = c >= 0 ? flip[c] : 0;
    }
    if (j < R2) rhsbuf[j] = T2[(size_t)j * ld + C2 - 1];
}

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int gm_workspace(const CutView& v, size_t bytes, char** ws)
{
    if (*v.ws_bytes < bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(v.stream));
        hipFree(*v.ws); *v.ws = nullptr; *v.ws_bytes = 0;
        hipError_t e = malloc_retry((void**)v.ws, bytes);
        if (e != hipSuccess) { set_error(std::string("cut round workspace: ") + hipGetErrorString(e)); return e == hipErrorOutOfMemory ? LPX_ENOMEM : LPX_EDEVICE; }
        *v.ws_bytes = bytes;
    }
    *ws = *v.ws;
    return 0;
}
}  // namespace

int check_cut_opts(const lpx_cut_opts* o, const char* what, int kmin)
{
    if (!o) { set_error(std::string(what) + ": null options"); return LPX_EINVAL; }
    const char* bad = nullptr;
    if (o->cuts_per_round < kmin || o->cuts_per_round > GMI_KMAX) bad = kmin ? "cuts_per_round must be in 1..64" : "cuts_per_round must be in 0..64";
    else if (o->max_rounds < 0) bad = "max_rounds must be >= 0";
    else if (o->max_active < 1) bad = "max_active must be >= 1";
    else if (!(o->away > 0 && o->away <= 0.5)) bad = "away must be in (0, 0.5]";
    else if (!(o->coef_eps >= 0 && o->coef_eps < 0.5)) bad = "coef_eps must be in [0, 0.5)";
    else if (!(o->max_dynamism >= 1)) bad = "max_dynamism must be >= 1";
    else if (o->purge_tol != o->purge_tol) bad = "purge_tol must be a number";
    else if (!(o->int_tol >= 0)) bad = "int_tol must be >= 0";
    if (bad) { set_error(std::string(what) + ": " + bad); return LPX_EINVAL; }
    return 0;
}

int check_cut_opts(const lpx_cut_opts* o, const char* what) { return check_cut_opts(o, what, 1); }

int gmi_round_args(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o, int kmin, const char* what)
{
    if (int rc = check_cut_opts(o, what, kmin)) return rc;
    if (n_mask < 0 || (n_mask > 0 && !is_int)) { set_error(std::string(what) + ": bad integer mask"); return LPX_EINVAL; }
    if (!t) { set_error(std::string(what) + ": null handle"); return LPX_EINVAL; }
    CutView v;
    tableau_cut_view(t, &v, false);
    const int m = v.R - 1, Cm = v.C - 1;
    if (m < 1) { set_error(std::string(what) + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    if (first_cut_col < 1 || first_cut_col > Cm) { set_error(std::string(what) + ": first_cut_col outside [1, C-1]"); return LPX_EINVAL; }
    if (Cm - first_cut_col > GMI_PMAX) { set_error(std::string(what) + ": more than 2048 cut columns"); return LPX_EINVAL; }
    if (v.Ccap > GMI_CMAX) { set_error(std::string(what) + ": handle wider than 131072 columns"); return LPX_EINVAL; }
    return 0;
}

// The round of both entry points behind their argument checks.  cb == nullptr: lpx_tableau_gmi_round.  Else the bounded round: the
// integer array from cb's lo / ub (either null: a handle without bounds, every flagged column passes) and, where cb->ub is set,
// ub / lo / flip and rhsbuf carried to the new shape.
int gmi_round_run(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o, int* n_added,
                  int32_t* src_rows, int* n_purged, int32_t* purged_cols, const CutBounds* cb, const char* what)
{
    CutView v;
    tableau_cut_view(t, &v, false);
    const int m = v.R - 1, Cm = v.C - 1;
    if (int rc = ensure_device()) return rc;
    if (n_added) *n_added = 0;
    if (n_purged) *n_purged = 0;

    const size_t Rc = (size_t)v.Rcap, Cc = (size_t)v.Ccap;
    const size_t b_plan = up256(sizeof(GmiPlan)), b_i = up256(sizeof(int32_t) * Rc), b_d = up256(sizeof(double) * Rc);
    const size_t b_cu8 = up256(Cc), b_ci = up256(sizeof(int32_t) * Cc);
    char* ws = nullptr;
    const size_t b_cd = up256(sizeof(double) * Cc);
    if (int rc = gm_workspace(v, b_plan + 3 * b_i + 4 * b_d + 2 * b_cu8 + 2 * b_ci + (cb ? 2 * b_cu8 + 2 * b_cd : 0), &ws)) return rc;
    GmiPlan* plan = (GmiPlan*)ws; ws += b_plan;
    int32_t* flag = (int32_t*)ws; ws += b_i;
    int32_t* rowsrc = (int32_t*)ws; ws += b_i;
    int32_t* nbasis = (int32_t*)ws; ws += b_i;
    double* f0 = (double*)ws; ws += b_d;
    double* amax = (double*)ws; ws += b_d;
    double* amin = (double*)ws; ws += b_d;
    double* bv = (double*)ws; ws += b_d;
    uint8_t* isint = (uint8_t*)ws; ws += b_cu8;
    uint8_t* nbm = (uint8_t*)ws; ws += b_cu8;
    int32_t* colsrc = (int32_t*)ws; ws += b_ci;
    int32_t* pcol = (int32_t*)ws; ws += b_ci;
    uint8_t* flags = nullptr; uint8_t* flip2 = nullptr; double* ub2 = nullptr; double* lo2 = nullptr;     // the bounded round's
    if (cb) { flags = (uint8_t*)ws; ws += b_cu8; flip2 = (uint8_t*)ws; ws += b_cu8; ub2 = (double*)ws; ws += b_cd; lo2 = (double*)ws; }

    const int nint = n_mask < first_cut_col ? n_mask : first_cut_col;
    std::vector<uint8_t> hint((size_t)Cm, 0);
    for (int j = 0; j < nint; ++j) hint[j] = is_int[j] ? 1 : 0;
    LPX_HIP_TRY(hipMemcpyAsync(cb ? flags : isint, hint.data(), (size_t)Cm, hipMemcpyHostToDevice, v.stream));
    if (cb) {
        hipLaunchKernelGGL(gmi_mask_bounded, dim3((unsigned)((Cm + GA_NT - 1) / GA_NT)), dim3(GA_NT), 0, v.stream, Cm, nint, flags,
                           cb->ub ? cb->lo : nullptr, cb->ub, isint);
        LPX_HIP_TRY(hipGetLastError());
    }

    GmiParams g;
    g.away = o->away; g.coef_eps = o->coef_eps; g.max_dyn = o->max_dynamism; g.purge_tol = o->purge_tol;
    g.kcap = o->cuts_per_round; g.purge = o->purge ? 1 : 0; g.first_cut = first_cut_col; g.pad = 0;
    const size_t lds_nb = sizeof(unsigned) * (size_t)((Cm + 31) / 32);
    hipLaunchKernelGGL(gmi_scan, dim3((unsigned)((m + GS_RPB - 1) / GS_RPB)), dim3(GS_NT), 2 * lds_nb, v.stream,
                       v.T, v.ld, m, Cm, v.basis, isint, g, flag, f0, amax, amin, bv);
    LPX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gmi_pick, dim3(1), dim3(GP_NT), lds_nb, v.stream, m, Cm, v.Rcap, v.Ccap, v.basis, flag, f0, amax, amin, bv,
                       g, plan, pcol, rowsrc, colsrc, nbasis, nbm);
    LPX_HIP_TRY(hipGetLastError());
    GmiPlan hp;
    LPX_HIP_TRY(hipMemcpyAsync(&hp, plan, sizeof(GmiPlan), hipMemcpyDeviceToHost, v.stream));
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    std::vector<int32_t> hpc(hp.P > 0 ? hp.P : 1);
    if (hp.P > 0) LPX_HIP_TRY(hipMemcpyAsync(hpc.data(), pcol, sizeof(int32_t) * hp.P, hipMemcpyDeviceToHost, v.stream));
    if (hp.K == 0 && hp.P == 0) {
        LPX_HIP_TRY(hipStreamSynchronize(v.stream));
        return 0;
    }
    if (hp.P == 0) {
        const int ncb = (Cm + GA_NT - 1) / GA_NT, ntb = (m + hp.K + GA_NT - 1) / GA_NT;
        hipLaunchKernelGGL(gmi_apply_inplace, dim3((unsigned)(ncb + ntb)), dim3(GA_NT), 0, v.stream, v.T, v.ld, m, Cm, ncb,
                           plan, nbm, isint, nbasis, v.basis, o->coef_eps);
        LPX_HIP_TRY(hipGetLastError());
        if (cb && cb->ub) {
            const int n = hp.R2 > hp.K ? hp.R2 : hp.K;
            hipLaunchKernelGGL(gmi_carry_inplace, dim3((unsigned)((n + GA_NT - 1) / GA_NT)), dim3(GA_NT), 0, v.stream, v.T, v.ld, hp.R2,
                               Cm, plan, cb->ub, cb->lo, cb->flip, cb->rhsbuf);
            LPX_HIP_TRY(hipGetLastError());
        }
    } else {
        tableau_cut_view(t, &v, true);
        if (!v.T2) { set_error(std::string(what) + ": no device memory for the compacting pass"); return LPX_ENOMEM; }
        const int gy = hp.R2 < 65535 ? hp.R2 : 65535;
        const int gx = ((hp.C2 > hp.R2 ? hp.C2 : hp.R2) + GA_NT - 1) / GA_NT;
        hipLaunchKernelGGL(gmi_apply_purge, dim3((unsigned)gx, (unsigned)gy), dim3(GA_NT), 0, v.stream, v.T, v.T2, v.ld, Cm,
                           hp.R2, hp.C2, plan, rowsrc, colsrc, nbm, isint, nbasis, v.basis, o->coef_eps);
        LPX_HIP_TRY(hipGetLastError());
        if (cb && cb->ub) {
            const int n = hp.R2 > v.Ccap ? hp.R2 : v.Ccap;
            hipLaunchKernelGGL(gmi_carry_purge, dim3((unsigned)((n + GA_NT - 1) / GA_NT)), dim3(GA_NT), 0, v.stream, v.T2, v.ld, hp.R2,
                               hp.C2, v.Ccap, colsrc, cb->ub, cb->lo, cb->flip, ub2, lo2, flip2, cb->rhsbuf);
            LPX_HIP_TRY(hipGetLastError());
            LPX_HIP_TRY(hipMemcpyAsync(cb->ub, ub2, sizeof(double) * Cc, hipMemcpyDeviceToDevice, v.stream));
            LPX_HIP_TRY(hipMemcpyAsync(cb->lo, lo2, sizeof(double) * Cc, hipMemcpyDeviceToDevice, v.stream));
            LPX_HIP_TRY(hipMemcpyAsync(cb->flip, flip2, Cc, hipMemcpyDeviceToDevice, v.stream));
        }
        LPX_HIP_TRY(hipMemcpyAsync(v.T, v.T2, sizeof(double) * (size_t)hp.R2 * v.ld, hipMemcpyDeviceToDevice, v.stream));
    }
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    if (int rc = lpx_tableau_set_shape(t, hp.R2, hp.C2)) return rc;
    LPX_HIP_TRY(hipMemsetAsync(v.st, 0, sizeof(DevState), v.stream));
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    if (n_added) *n_added = hp.K;
    if (src_rows) for (int k = 0; k < hp.K; ++k) src_rows[k] = hp.src[k];
    if (n_purged) *n_purged = hp.P;
    if (purged_cols) for (int i = 0; i < hp.P; ++i) purged_cols[i] = hpc[i];
    return 0;
}

}  // namespace lpx

using namespace lpx;

extern "C" {

void lpx_default_cut_opts(lpx_cut_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->cuts_per_round = 8; o->max_rounds = 50; o->max_active = 64; o->purge = 1;
    o->away = 1e-3; o->coef_eps = 1e-9; o->max_dynamism = 1e6; o->purge_tol = 1e-9; o->int_tol = 1e-6;
}

int lpx_tableau_gmi_round(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col,
                          const lpx_cut_opts* o, int* n_added, int32_t* src_rows, int* n_purged, int32_t* purged_cols)
{
    static const char* what = "lpx_tableau_gmi_round";
    if (int rc = gmi_round_args(t, is_int, n_mask, first_cut_col, o, 1, what)) return rc;
    return gmi_round_run(t, is_int, n_mask, first_cut_col, o, n_added, src_rows, n_purged, purged_cols, nullptr, what);
}

}  // extern "C"
