// lpx_postopt.hip -- post-optimal edits of a device tableau (lpx_tableau_rhs_update, _objective_update, _add_column,
// _add_row; include/lpx.h defines them bit for bit).  Every edit is one of two combinations over part of the tableau,
// each two launches that read nothing they write:
//
//   po_col_pass     out[i] = base[i] (+) sum_k v_k T[i, cols[k]].  A workgroup owns a tile of PO_CR rows x PO_CT terms
//                   (PO_CT / LPX_POSTOPT_SEG segments).  The lanes walk the tile row by row along the terms -- contiguous
//                   lanes on consecutive columns when the columns are consecutive (the slack block) -- and park the
//                   products in LDS; then one lane per (row, segment) sums its segment there in term order from +0.0 and
//                   writes the sum to a slab.
//   po_col_combine  one lane per row: base, then the segment sums in ascending order; written to the RHS column (RHS update)
//                   or, for a new column, to column C-1 after the RHS has moved to column C.
//   po_row_pass     out[j] = base[j] (+) sum_k w_k T[rows[k], j].  A workgroup owns PO_RT columns (two per lane, 16-byte
//                   loads) and one segment of LPX_POSTOPT_SEG rows, summed in term order from +0.0 into a slab.
//   po_row_combine  one lane per column: base, the segment sums in ascending order, +0.0 in basic columns; written to the
//                   objective row (cost change) or to a staging row (new row).
//   po_append_row   the staging row goes in at row m through append_rows_inplace (lpx_append.h), shared with the GMI round.
//
// No float atomics and no FMA (the library is built -ffp-contract=off): the bits do not depend on the grid.
#include "lpx_append.h"
#include "lpx_block.h"

#include <cstring>
#include <string>
#include <vector>

namespace lpx {

static constexpr int PO_SEG = LPX_POSTOPT_SEG;
static constexpr int PO_NT = 256;
static constexpr int PO_CR = 32;                 // col pass: rows per tile
static constexpr int PO_CT = 256;                // col pass: terms per tile (4 segments)
static constexpr int PO_CS = PO_CT + 1;          // LDS row stride (doubles): consecutive rows start in different banks
static constexpr int PO_RT = 2 * PO_NT;          // row pass: columns per workgroup
static_assert(PO_CT % PO_SEG == 0 && PO_NT == PO_CT, "one lane per term of a tile row");
static_assert(PO_CR * (PO_CT / PO_SEG) <= PO_NT, "one lane per (row, segment) of a tile");

typedef double po_d2 __attribute__((ext_vector_type(2)));

// part[s * R + i] = sum over the terms k of segment s, in order from +0.0, of v[k] * T[i, cols[k]]
__global__ __launch_bounds__(PO_NT) void po_col_pass(const double* __restrict__ T, int ld, int R, int K,
                                                     const int32_t* __restrict__ cols, const double* __restrict__ v,
                                                     double* __restrict__ part)
{
    __shared__ double s_p[PO_CR * PO_CS];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * PO_CR, k0 = blockIdx.y * PO_CT;
    const int k = k0 + tid;
    const bool live = k < K;
    const int c = live ? cols[k] : 0;
    const double w = live ? v[k] : 0.0;
    const int nr = R - i0 < PO_CR ? R - i0 : PO_CR;
#pragma unroll 8
    for (int rr = 0; rr < PO_CR; ++rr) {
        double p = 0.0;
        if (live && rr < nr) p = w * T[(size_t)(i0 + rr) * ld + c];
        s_p[rr * PO_CS + tid] = p;
    }
    __syncthreads();
    const int rr = tid % PO_CR, sg = tid / PO_CR;
    const int ks = k0 + sg * PO_SEG;
    if (sg >= PO_CT / PO_SEG || rr >= nr || ks >= K) return;
    const int n = K - ks < PO_SEG ? K - ks : PO_SEG;
    const double* p = s_p + rr * PO_CS + sg * PO_SEG;
    double s = 0.0;
    for (int t = 0; t < n; ++t) s = s + p[t];
    part[(size_t)(ks / PO_SEG) * R + i0 + rr] = s;
}

// mode 0: T[i, Cm] = T[i, Cm] (+) segments.  mode 1 (new column): base = +0.0 (i < m) / obj (i = m); the RHS moves to
// column Cm + 1 and the result goes to column Cm.
__global__ __launch_bounds__(PO_NT) void po_col_combine(double* __restrict__ T, int ld, int R, int Cm, int nseg,
                                                        const double* __restrict__ part, int mode, double obj)
{
    const int i = blockIdx.x * PO_NT + threadIdx.x;
    if (i >= R) return;
    double* row = T + (size_t)i * ld;
    const double rhs = row[Cm];
    double o = mode == 0 ? rhs : (i == R - 1 ? obj : 0.0);
    for (int s = 0; s < nseg; ++s) o = o + part[(size_t)s * R + i];
    if (mode == 0) {
        row[Cm] = o;
    } else {
        row[Cm + 1] = rhs;
        row[Cm] = o;
    }
}

// part[s * P + j] = sum over the terms k of segment s, in order from +0.0, of w[k] * T[rows[k], j], j < Cw
__global__ __launch_bounds__(PO_NT) void po_row_pass(const double* __restrict__ T, int ld, int Cw, int K,
                                                     const int32_t* __restrict__ rows, const double* __restrict__ w,
                                                     double* __restrict__ part, int P)
{
    const int j = blockIdx.x * PO_RT + 2 * threadIdx.x;
    const int ks = blockIdx.y * PO_SEG;
    const int n = K - ks < PO_SEG ? K - ks : PO_SEG;
    if (j >= Cw) return;
    double s0 = 0.0, s1 = 0.0;
    // j is even and ld a multiple of 16: the pair (j, j + 1) is one aligned 16-byte load inside the row even when j + 1 = Cw
    int t = 0;
    for (; t + 8 <= n; t += 8) {
        po_d2 x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            x[u] = __builtin_nontemporal_load(reinterpret_cast<const po_d2*>(T + (size_t)rows[ks + t + u] * ld + j));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double wk = w[ks + t + u];
            s0 = s0 + wk * x[u].x;
            s1 = s1 + wk * x[u].y;
        }
    }
    for (; t < n; ++t) {
        const po_d2 x = __builtin_nontemporal_load(reinterpret_cast<const po_d2*>(T + (size_t)rows[ks + t] * ld + j));
        const double wk = w[ks + t];
        s0 = s0 + wk * x.x;
        s1 = s1 + wk * x.y;
    }
    double* dst = part + (size_t)blockIdx.y * P;
    dst[j] = s0;
    if (j + 1 < Cw) dst[j + 1] = s1;
}

// basic[j] = 1 for the basic columns; the sparse cost deltas of a cost change subtracted from the objective row
__global__ __launch_bounds__(PO_NT) void po_prep(double* __restrict__ T, int ld, int m, const int32_t* __restrict__ basis,
                                                 uint8_t* __restrict__ basic, int Kd, const int32_t* __restrict__ dcols,
                                                 const double* __restrict__ dd)
{
    const int i = blockIdx.x * PO_NT + threadIdx.x;
    if (i < m) basic[basis[i]] = 1;
    if (i < Kd) {
        double* e = T + (size_t)m * ld + dcols[i];
        *e = *e - dd[i];
    }
}

// mode 0 (cost change): out[j] = T[m, j] (+) segments of column j, j < C, written to row m.
// mode 1 (new row, new shape C + 1): column j < Cm reads column j, the new slack column Cm is base[Cm] unchanged, the RHS
// column Cm + 1 reads the old RHS column Cm; out goes to stage[].  Basic columns are +0.0 in both.
__global__ __launch_bounds__(PO_NT) void po_row_combine(double* __restrict__ T, int ld, int m, int Cm, int nseg,
                                                        const double* __restrict__ part, int P, const uint8_t* __restrict__ basic,
                                                        int mode, const double* __restrict__ base, double* __restrict__ stage)
{
    const int j = blockIdx.x * PO_NT + threadIdx.x;
    const int Cout = mode == 0 ? Cm + 1 : Cm + 2;
    if (j >= Cout) return;
    const int src = mode == 0 ? j : (j < Cm ? j : (j == Cm ? -1 : Cm));
    double o = mode == 0 ? T[(size_t)m * ld + j] : base[j];
    if (src >= 0)
        for (int s = 0; s < nseg; ++s) o = o + part[(size_t)s * P + src];
    if (src >= 0 && src < Cm && basic[src]) o = 0.0;
    if (mode == 0) T[(size_t)m * ld + j] = o;
    else stage[j] = o;
}

struct PoNewRow {
    const double* stage; int Cm;
    __device__ double body(int, int j) const { return stage[j]; }
    __device__ double slack(int, int) const { return stage[Cm]; }
    __device__ double rhs(int) const { return stage[Cm + 1]; }
};

// the staged row in at row m, the objective row to m + 1, a zero slack column at Cm in the old rows; basis[m] = Cm
__global__ __launch_bounds__(PO_NT) void po_append_row(double* __restrict__ T, int ld, int m, int Cm, int ncb,
                                                       const double* __restrict__ stage, int32_t* __restrict__ basis)
{
    const PoNewRow rows{stage, Cm};
    const int r = append_rows_inplace(T, ld, m, Cm, 1, ncb, PO_NT, rows);
    if (r == m) basis[m] = Cm;
}

namespace {

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int po_workspace(const CutView& v, size_t bytes, char** ws)
{
    if (*v.ws_bytes < bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(v.stream));
        hipFree(*v.ws); *v.ws = nullptr; *v.ws_bytes = 0;
        hipError_t e = malloc_retry((void**)v.ws, bytes);
        if (e != hipSuccess) { set_error(std::string("post-optimal workspace: ") + hipGetErrorString(e)); return e == hipErrorOutOfMemory ? LPX_ENOMEM : LPX_EDEVICE; }
        *v.ws_bytes = bytes;
    }
    *ws = *v.ws;
    return 0;
}

int nseg_of(int K) { return (K + PO_SEG - 1) / PO_SEG; }

// argument checks shared by the four entry points (no device access; the handle is a host record)
int check_terms(const char* what, int K, const int32_t* idx, const double* val, int lo, int hi, const char* idx_name)
{
    if (K < 0) { set_error(std::string(what) + ": K < 0"); return LPX_EINVAL; }
    if (K > 0 && (!idx || !val)) { set_error(std::string(what) + ": null term arrays"); return LPX_EINVAL; }
    for (int k = 0; k < K; ++k)
        if (idx[k] < lo || idx[k] >= hi) {
            set_error(std::string(what) + ": " + idx_name + "[" + std::to_string(k) + "] = " + std::to_string(idx[k]) + " outside [" +
                      std::to_string(lo) + ", " + std::to_string(hi) + ")");
            return LPX_EINVAL;
        }
    return 0;
}

// host arrays into the workspace: idx[K] then val[K] (one upload)
int upload_terms(const CutView& v, int K, const int32_t* idx, const double* val, int32_t* didx, double* dval)
{
    if (K == 0) return 0;
    LPX_HIP_TRY(hipMemcpyAsync(didx, idx, sizeof(int32_t) * K, hipMemcpyHostToDevice, v.stream));
    LPX_HIP_TRY(hipMemcpyAsync(dval, val, sizeof(double) * K, hipMemcpyHostToDevice, v.stream));
    return 0;
}

// the edit is complete: new live shape (or the same), loop state reset as lpx_tableau_build_child does
int finish(lpx_tableau* t, const CutView& v, int R, int C)
{
    LPX_HIP_TRY(hipGetLastError());
    if (int rc = lpx_tableau_set_shape(t, R, C)) return rc;
    LPX_HIP_TRY(hipMemsetAsync(v.st, 0, sizeof(DevState), v.stream));
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    return 0;
}

// the column combination over rows [0, R) into the RHS column (mode 0) or a new column (mode 1)
int col_combination(lpx_tableau* t, int K, const int32_t* cols, const double* vals, int mode, double obj)
{
    CutView v;
    tableau_cut_view(t, &v, false);
    const int R = v.R, Cm = v.C - 1, ns = nseg_of(K);
    const size_t b_part = up256(sizeof(double) * (size_t)(ns > 0 ? ns : 1) * R);
    const size_t b_i = up256(sizeof(int32_t) * (size_t)(K > 0 ? K : 1)), b_d = up256(sizeof(double) * (size_t)(K > 0 ? K : 1));
    char* ws = nullptr;
    if (int rc = po_workspace(v, b_part + b_i + b_d, &ws)) return rc;
    double* part = (double*)ws;
    int32_t* dcols = (int32_t*)(ws + b_part);
    double* dv = (double*)(ws + b_part + b_i);
    if (int rc = upload_terms(v, K, cols, vals, dcols, dv)) return rc;
    if (K > 0) {
        hipLaunchKernelGGL(po_col_pass, dim3((unsigned)((R + PO_CR - 1) / PO_CR), (unsigned)((K + PO_CT - 1) / PO_CT)), dim3(PO_NT), 0,
                           v.stream, v.T, v.ld, R, K, dcols, dv, part);
        LPX_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(po_col_combine, dim3((unsigned)((R + PO_NT - 1) / PO_NT)), dim3(PO_NT), 0, v.stream, v.T, v.ld, R, Cm, ns,
                       part, mode, obj);
    return finish(t, v, R, mode == 0 ? v.C : v.C + 1);
}

// the row combination over old columns [0, C): mode 0 into the objective row, mode 1 as a new row at index m
int row_combination(lpx_tableau* t, int K, const int32_t* rows, const double* w, int Kd, const int32_t* dcols, const double* dd,
                    int mode, const double* base)
{
    CutView v;
    tableau_cut_view(t, &v, false);
    const int m = v.R - 1, C = v.C, Cm = C - 1, ns = nseg_of(K);
    const int P = (C + 1 + 15) & ~15;                       // slab row: C + 1 columns rounded up to 16
    const size_t b_part = up256(sizeof(double) * (size_t)(ns > 0 ? ns : 1) * P);
    const size_t b_i = up256(sizeof(int32_t) * (size_t)(K > 0 ? K : 1)), b_d = up256(sizeof(double) * (size_t)(K > 0 ? K : 1));
    const size_t b_di = up256(sizeof(int32_t) * (size_t)(Kd > 0 ? Kd : 1)), b_dd = up256(sizeof(double) * (size_t)(Kd > 0 ? Kd : 1));
    const size_t b_row = up256(sizeof(double) * (size_t)(C + 1)), b_mask = up256((size_t)C);
    char* ws = nullptr;
    if (int rc = po_workspace(v, b_part + b_i + b_d + b_di + b_dd + 2 * b_row + b_mask, &ws)) return rc;
    double* part = (double*)ws; ws += b_part;
    int32_t* drows = (int32_t*)ws; ws += b_i;
    double* dw = (double*)ws; ws += b_d;
    int32_t* ddc = (int32_t*)ws; ws += b_di;
    double* ddd = (double*)ws; ws += b_dd;
    double* dbase = (double*)ws; ws += b_row;
    double* stage = (double*)ws; ws += b_row;
    uint8_t* basic = (uint8_t*)ws;
    if (int rc = upload_terms(v, K, rows, w, drows, dw)) return rc;
    if (int rc = upload_terms(v, Kd, dcols, dd, ddc, ddd)) return rc;
    if (mode == 1) LPX_HIP_TRY(hipMemcpyAsync(dbase, base, sizeof(double) * (size_t)(C + 1), hipMemcpyHostToDevice, v.stream));
    LPX_HIP_TRY(hipMemsetAsync(basic, 0, (size_t)C, v.stream));
    const int np = m > Kd ? m : Kd;
    if (np > 0) {
        hipLaunchKernelGGL(po_prep, dim3((unsigned)((np + PO_NT - 1) / PO_NT)), dim3(PO_NT), 0, v.stream, v.T, v.ld, m, v.basis, basic,
                           Kd, ddc, ddd);
        LPX_HIP_TRY(hipGetLastError());
    }
    if (K > 0) {
        hipLaunchKernelGGL(po_row_pass, dim3((unsigned)((C + PO_RT - 1) / PO_RT), (unsigned)ns), dim3(PO_NT), 0, v.stream, v.T, v.ld, C, K,
                           drows, dw, part, P);
        LPX_HIP_TRY(hipGetLastError());
    }
    const int Cout = mode == 0 ? C : C + 1;
    hipLaunchKernelGGL(po_row_combine, dim3((unsigned)((Cout + PO_NT - 1) / PO_NT)), dim3(PO_NT), 0, v.stream, v.T, v.ld, m, Cm, ns, part,
                       P, basic, mode, dbase, stage);
    if (mode == 0) return finish(t, v, v.R, C);
    LPX_HIP_TRY(hipGetLastError());
    const int ncb = (Cm + PO_NT - 1) / PO_NT, ntb = (m + 1 + PO_NT - 1) / PO_NT;
    hipLaunchKernelGGL(po_append_row, dim3((unsigned)(ncb + ntb)), dim3(PO_NT), 0, v.stream, v.T, v.ld, m, Cm, ncb, stage, v.basis);
    return finish(t, v, v.R + 1, C + 1);
}

// shape record without touching the device
int live_shape(lpx_tableau* t, CutView* v, const char* what)
{
    tableau_cut_view(t, v, false);
    if (v->R < 2) { set_error(std::string(what) + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    return 0;
}

}  // namespace
}  // namespace lpx

using namespace lpx;

extern "C" {

int lpx_tableau_rhs_update(lpx_tableau* t, int K, const int32_t* cols, const double* v)
{
    static const char* what = "lpx_tableau_rhs_update";
    if (!t) { set_error(std::string(what) + ": null handle"); return LPX_EINVAL; }
    CutView s;
    if (int rc = live_shape(t, &s, what)) return rc;
    if (int rc = check_terms(what, K, cols, v, 0, s.C - 1, "cols")) return rc;
    if (int rc = ensure_device()) return rc;
    return col_combination(t, K, cols, v, 0, 0.0);
}

int lpx_tableau_add_column(lpx_tableau* t, int K, const int32_t* cols, const double* v, double obj)
{
    static const char* what = "lpx_tableau_add_column";
    if (!t) { set_error(std::string(what) + ": null handle"); return LPX_EINVAL; }
    CutView s;
    if (int rc = live_shape(t, &s, what)) return rc;
    if (int rc = check_terms(what, K, cols, v, 0, s.C - 1, "cols")) return rc;
    if (s.C + 1 > s.Ccap) { set_error(std::string(what) + ": no spare column capacity (Ccap = C)"); return LPX_EINVAL; }
    if (int rc = ensure_device()) return rc;
    return col_combination(t, K, cols, v, 1, obj);
}

int lpx_tableau_objective_update(lpx_tableau* t, int K, const int32_t* rows, const double* w, int Kd, const int32_t* dcols,
                                 const double* dd)
{
    static const char* what = "lpx_tableau_objective_update";
    if (!t) { set_error(std::string(what) + ": null handle"); return LPX_EINVAL; }
    CutView s;
    if (int rc = live_shape(t, &s, what)) return rc;
    if (int rc = check_terms(what, K, rows, w, 0, s.R - 1, "rows")) return rc;
    if (int rc = check_terms(what, Kd, dcols, dd, 0, s.C - 1, "dcols")) return rc;
    {
        std::vector<uint8_t> seen((size_t)s.C, 0);
        for (int k = 0; k < Kd; ++k) {
            if (seen[dcols[k]]) { set_error(std::string(what) + ": repeated column in dcols"); return LPX_EINVAL; }
            seen[dcols[k]] = 1;
        }
    }
    if (int rc = ensure_device()) return rc;
    return row_combination(t, K, rows, w, Kd, dcols, dd, 0, nullptr);
}

int lpx_tableau_add_row(lpx_tableau* t, int K, const int32_t* rows, const double* w, const double* base)
{
    static const char* what = "lpx_tableau_add_row";
    if (!t) { set_error(std::string(what) + ": null handle"); return LPX_EINVAL; }
    CutView s;
    if (int rc = live_shape(t, &s, what)) return rc;
    if (int rc = check_terms(what, K, rows, w, 0, s.R - 1, "rows")) return rc;
    if (!base) { set_error(std::string(what) + ": null base row"); return LPX_EINVAL; }
    if (s.R + 1 > s.Rcap || s.C + 1 > s.Ccap) { set_error(std::string(what) + ": no spare row and column capacity"); return LPX_EINVAL; }
    if (int rc = ensure_device()) return rc;
    return row_combination(t, K, rows, w, 0, nullptr, nullptr, 1, base);
}

}  // extern "C"
