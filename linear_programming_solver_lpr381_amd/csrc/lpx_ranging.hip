// lpx_ranging.hip -- sensitivity ranging of a solved tableau in one read of HBM (lpx_tableau_ranging / _pairs, include/lpx.h).
//
// On the live R x C window of a handle (m = R - 1, objective row last, RHS column last), with b+_r = max(b_r, +0) and
// d+_j = max(d_j, +0) written as the C expression (x > 0 ? x : 0.0), N the nonbasic columns (j < C - 1, not in basis):
//   column ratio test, every j < C - 1:  col_inc[j] = min_{r: T[r,j] < -eps} b+_r / -T[r,j],  col_dec[j] = min_{r: T[r,j] > eps} b+_r / T[r,j]
//   row ratio test, every r < m:         row_inc[r] = min_{j in N: T[r,j] < -eps} d+_j / -T[r,j], row_dec[r] likewise over T[r,j] > eps
//   min_rhs = min_{r < m} b_r,  min_dj = min_{j in N} d_j
// Every min is the strict minimum with ties to the lowest index (mi_pick); an empty set gives +inf / -1.
//
// rg_pass: one launch over tiles of RG_TR rows x RG_TC columns.  A lane owns 8 columns of its tile's window (4 x 16-B
// nontemporal loads per row, 1 KiB contiguous per wave-instruction) and walks every 4th row of the tile; it keeps the
// column partials of its 8 columns in registers, and each row's partial over the window is one wave min-reduction.  The
// nonbasic mask (LDS, from the device basis), the window of the objective row (registers) and the rows' b+ (LDS) are
// staged once per tile.  Partials go to slabs of (value, index) pairs:
//   columns: [nrb][2][C-1], rows: [ncw][2][m], plus one (value, index) per tile row block / column window for the scalars;
// rg_combine reduces them.  The rule is associative and commutative, so the result does not depend on the order.
#include "lpx_block.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace lpx {

static constexpr int RG_NT = 256;            // 4 waves
static constexpr int RG_TC = 512;            // columns per tile: 4 x 16 B per lane
static constexpr int RG_TR = 128;            // rows per tile: 32 per wave (3 workgroups per CU at 4097 x 12289)
static constexpr int RG_NV = RG_TC / 128;    // 16-B vectors per lane per row
static constexpr int RG_NE = 2 * RG_NV;      // columns per lane

typedef double rg_d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double rg_pos(double x) { return x > 0 ? x : 0.0; }
__device__ __forceinline__ int rg_idx(int i) { return i == INT_MAX ? -1 : i; }

__global__ __launch_bounds__(RG_NT) void rg_pass(const double* __restrict__ T, int ld, int m, int Cm,
                                                 const int32_t* __restrict__ basis, double eps,
                                                 double* __restrict__ colv, int32_t* __restrict__ coli,
                                                 double* __restrict__ rowv, int32_t* __restrict__ rowi,
                                                 double* __restrict__ sclv, int32_t* __restrict__ scli)
{
    __shared__ unsigned char s_nb[RG_TC];
    __shared__ double s_b[RG_TR];
    __shared__ double s_cv[2][RG_TC];
    __shared__ int s_ci[2][RG_TC];
    __shared__ double s_rv[RG_NT / 64];
    __shared__ int s_ri[RG_NT / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cw = blockIdx.x, rb = blockIdx.y;
    const int c0 = cw * RG_TC, r0 = rb * RG_TR;
    const int C1 = Cm + 1;                    // the RHS column

    // nonbasic mask of the window from the device basis
    for (int k = tid; k < RG_TC; k += RG_NT) s_nb[k] = c0 + k < Cm ? 1 : 0;
    __syncthreads();
    for (int r = tid; r < m; r += RG_NT) {
        const int j = basis[r] - c0;
        if (j >= 0 && j < RG_TC) s_nb[j] = 0;
    }
    // b+ of the tile's rows; min_rhs partial of the row block (column window 0 only)
    MinIdx mr{__builtin_inf(), INT_MAX};
    for (int k = tid; k < RG_TR; k += RG_NT) {
        const int r = r0 + k;
        double b = 0.0;
        if (r < m) { b = T[(size_t)r * ld + C1 - 1]; if (b < mr.v) { mr.v = b; mr.i = r; } }
        s_b[k] = rg_pos(b);
    }
    __syncthreads();
    if (cw == 0) {
        mr = block_min_idx<RG_NT>(mr, s_rv, s_ri);        // the value is re-read at the index: -0.0 and +0.0 tie
        if (tid == 0) { sclv[rb] = mr.i == INT_MAX ? mr.v : T[(size_t)mr.i * ld + C1 - 1]; scli[rb] = mr.i; }
    }

    // window of the objective row: d+ of nonbasic columns, NaN marks a basic / out-of-range column
    double dn[RG_NE];
    MinIdx md{__builtin_inf(), INT_MAX};
    const double* Tm = T + (size_t)m * ld;
#pragma unroll
    for (int e = 0; e < RG_NE; ++e) {
        const int lc = 128 * (e >> 1) + 2 * lane + (e & 1), j = c0 + lc;
        dn[e] = __builtin_nan("");
        if (j < Cm && s_nb[lc]) {
            const double d = Tm[j];
            dn[e] = rg_pos(d);
            if (d < md.v) { md.v = d; md.i = j; }
        }
    }
    if (rb == 0) {
        md = block_min_idx<RG_NT>(md, s_rv, s_ri);
        if (tid == 0) { sclv[gridDim.y + cw] = md.i == INT_MAX ? md.v : Tm[md.i]; scli[gridDim.y + cw] = md.i; }
    }

    // the rows: column partials per lane, row partials per wave
    double civ[RG_NE], cdv[RG_NE];
    int cii[RG_NE], cdi[RG_NE];
#pragma unroll
    for (int e = 0; e < RG_NE; ++e) { civ[e] = cdv[e] = __builtin_inf(); cii[e] = cdi[e] = INT_MAX; }
    const int rend = min(r0 + RG_TR, m);
    for (int r = r0 + wave; r < rend; r += RG_NT / 64) {
        const double* row = T + (size_t)r * ld + c0 + 2 * lane;
        double t[RG_NE];
#pragma unroll
        for (int v = 0; v < RG_NV; ++v) {
            rg_d2 x = {0.0, 0.0};
            if (c0 + 128 * v + 2 * lane < Cm) x = __builtin_nontemporal_load(reinterpret_cast<const rg_d2*>(row + 128 * v));
            t[2 * v] = x.x;
            t[2 * v + 1] = c0 + 128 * v + 2 * lane + 1 < Cm ? x.y : 0.0;
        }
        const double bp = s_b[r - r0];
        MinIdx ri{__builtin_inf(), INT_MAX}, rd{__builtin_inf(), INT_MAX};
#pragma unroll
        for (int e = 0; e < RG_NE; ++e) {
            const bool neg = t[e] < -eps, pos = t[e] > eps;
            if (neg || pos) {
                const double den = neg ? -t[e] : t[e];
                const double q = bp / den;
                if (neg) { if (q < civ[e]) { civ[e] = q; cii[e] = r; } }
                else     { if (q < cdv[e]) { cdv[e] = q; cdi[e] = r; } }
                if (dn[e] == dn[e]) {
                    const int j = c0 + 128 * (e >> 1) + 2 * lane + (e & 1);
                    const double p = dn[e] / den;
                    if (neg) { if (p < ri.v) { ri.v = p; ri.i = j; } }
                    else     { if (p < rd.v) { rd.v = p; rd.i = j; } }
                }
            }
        }
        ri = wave_min_idx(ri);
        rd = wave_min_idx(rd);
        if (lane == 0) {
            const size_t o = (size_t)cw * 2 * m + r;
            rowv[o] = ri.v; rowi[o] = ri.i;
            rowv[o + m] = rd.v; rowi[o + m] = rd.i;
        }
    }

    // combine the four waves' column partials in LDS, then one coalesced slab write per column
    for (int w = 0; w < RG_NT / 64; ++w) {
        if (wave == w) {
#pragma unroll
            for (int e = 0; e < RG_NE; ++e) {
                const int lc = 128 * (e >> 1) + 2 * lane + (e & 1);
                MinIdx a{civ[e], cii[e]}, b{cdv[e], cdi[e]};
                if (w > 0) { a = mi_pick(MinIdx{s_cv[0][lc], s_ci[0][lc]}, a); b = mi_pick(MinIdx{s_cv[1][lc], s_ci[1][lc]}, b); }
                s_cv[0][lc] = a.v; s_ci[0][lc] = a.i;
                s_cv[1][lc] = b.v; s_ci[1][lc] = b.i;
            }
        }
        __syncthreads();
    }
    for (int lc = tid; lc < RG_TC; lc += RG_NT) {
        const int j = c0 + lc;
        if (j < Cm) {
            const size_t o = (size_t)rb * 2 * Cm + j;
            colv[o] = s_cv[0][lc]; coli[o] = s_ci[0][lc];
            colv[o + Cm] = s_cv[1][lc]; coli[o + Cm] = s_ci[1][lc];
        }
    }
}

// One thread per column (j < Cm) and per row (r < m) of the outputs; thread 0 of block 0 also reduces the scalars.
// out: col (v: [2][Cm], i: [2][Cm]), row (v: [2][m], i: [2][m]), scalars (v: [2], i: [2]) = {min_rhs, min_dj}.
__global__ __launch_bounds__(RG_NT) void rg_combine(int m, int Cm, int nrb, int ncw,
                                                    const double* __restrict__ colv, const int32_t* __restrict__ coli,
                                                    const double* __restrict__ rowv, const int32_t* __restrict__ rowi,
                                                    const double* __restrict__ sclv, const int32_t* __restrict__ scli,
                                                    double* __restrict__ ov, int32_t* __restrict__ oi)
{
    const int g = blockIdx.x * RG_NT + threadIdx.x;
    if (g < Cm) {
        for (int s = 0; s < 2; ++s) {
            MinIdx a{__builtin_inf(), INT_MAX};
            for (int k = 0; k < nrb; ++k) {
                const size_t o = (size_t)k * 2 * Cm + (size_t)s * Cm + g;
                a = mi_pick(a, MinIdx{colv[o], coli[o]});
            }
            ov[(size_t)s * Cm + g] = a.v; oi[(size_t)s * Cm + g] = rg_idx(a.i);
        }
    } else if (g < Cm + m) {
        const int r = g - Cm;
        for (int s = 0; s < 2; ++s) {
            MinIdx a{__builtin_inf(), INT_MAX};
            for (int k = 0; k < ncw; ++k) {
                const size_t o = (size_t)k * 2 * m + (size_t)s * m + r;
                a = mi_pick(a, MinIdx{rowv[o], rowi[o]});
            }
            ov[2 * (size_t)Cm + (size_t)s * m + r] = a.v; oi[2 * (size_t)Cm + (size_t)s * m + r] = rg_idx(a.i);
        }
    }
    if (g == 0) {
        const size_t o = 2 * (size_t)Cm + 2 * (size_t)m;
        MinIdx a{__builtin_inf(), INT_MAX}, b{__builtin_inf(), INT_MAX};
        if (m > 0) for (int k = 0; k < nrb; ++k) a = mi_pick(a, MinIdx{sclv[k], scli[k]});
        for (int k = 0; k < ncw; ++k) b = mi_pick(b, MinIdx{sclv[nrb + k], scli[nrb + k]});
        ov[o] = a.v; oi[o] = rg_idx(a.i);
        ov[o + 1] = b.v; oi[o + 1] = rg_idx(b.i);
    }
}

// Pair test: one workgroup per pair k, the column ratio test along g_r = T[r,a_k] - T[r,b_k] (one IEEE subtraction).
// out: v [2][K] (inc, dec), i [2][K].
__global__ __launch_bounds__(RG_NT) void rg_pairs(const double* __restrict__ T, int ld, int m, int Cm, double eps,
                                                  const int32_t* __restrict__ pa, const int32_t* __restrict__ pb, int K,
                                                  double* __restrict__ ov, int32_t* __restrict__ oi)
{
    __shared__ double s_v[RG_NT / 64];
    __shared__ int s_i[RG_NT / 64];
    const int k = blockIdx.x;
    const int a = pa[k], b = pb[k];
    MinIdx inc{__builtin_inf(), INT_MAX}, dec{__builtin_inf(), INT_MAX};
    for (int r = threadIdx.x; r < m; r += RG_NT) {
        const double* row = T + (size_t)r * ld;
        const double g = row[a] - row[b];
        const double bp = rg_pos(row[Cm]);
        if (g < -eps) { const double q = bp / -g; if (q < inc.v) { inc.v = q; inc.i = r; } }
        else if (g > eps) { const double q = bp / g; if (q < dec.v) { dec.v = q; dec.i = r; } }
    }
    inc = block_min_idx<RG_NT>(inc, s_v, s_i);
    dec = block_min_idx<RG_NT>(dec, s_v, s_i);
    if (threadIdx.x == 0) {
        ov[k] = inc.v; oi[k] = rg_idx(inc.i);
        ov[K + k] = dec.v; oi[K + k] = rg_idx(dec.i);
    }
}

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the handle's ranging workspace, grown to `bytes` (it is only ever used on the handle's stream)
int rg_workspace(const TableauView& v, size_t bytes, char** ws)
{
    if (*v.ws_bytes < bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(v.stream));
        hipFree(*v.ws); *v.ws = nullptr; *v.ws_bytes = 0;
        hipError_t e = malloc_retry((void**)v.ws, bytes);
        if (e != hipSuccess) { set_error(std::string("ranging workspace: ") + hipGetErrorString(e)); return e == hipErrorOutOfMemory ? LPX_ENOMEM : LPX_EDEVICE; }
        *v.ws_bytes = bytes;
    }
    *ws = *v.ws;
    return 0;
}

int rg_check(double eps, const char* what)
{
    if (!(eps >= 0)) { set_error(std::string(what) + ": eps must be >= 0"); return LPX_EINVAL; }
    return ensure_device();
}
}  // namespace

}  // namespace lpx

using namespace lpx;

extern "C" {

int lpx_tableau_ranging(lpx_tableau* t, double eps,
                        double* col_inc, int32_t* col_inc_at, double* col_dec, int32_t* col_dec_at,
                        double* row_inc, int32_t* row_inc_at, double* row_dec, int32_t* row_dec_at,
                        double* min_rhs, double* min_dj)
{
    if (int rc = rg_check(eps, "lpx_tableau_ranging")) return rc;
    if (!t) { set_error("lpx_tableau_ranging: null handle"); return LPX_EINVAL; }
    TableauView v;
    tableau_view(t, &v);
    const int m = v.R - 1, Cm = v.C - 1;
    const int ncw = (Cm + RG_TC - 1) / RG_TC, nrb = m > 0 ? (m + RG_TR - 1) / RG_TR : 1;
    const size_t nout = 2 * (size_t)Cm + 2 * (size_t)m + 2;
    const size_t b_colv = up256(sizeof(double) * 2 * (size_t)nrb * Cm), b_coli = up256(sizeof(int32_t) * 2 * (size_t)nrb * Cm);
    const size_t b_rowv = up256(sizeof(double) * 2 * (size_t)ncw * (m > 0 ? m : 1)), b_rowi = up256(sizeof(int32_t) * 2 * (size_t)ncw * (m > 0 ? m : 1));
    const size_t b_sclv = up256(sizeof(double) * (size_t)(nrb + ncw)), b_scli = up256(sizeof(int32_t) * (size_t)(nrb + ncw));
    const size_t b_ov = up256(sizeof(double) * nout), b_oi = up256(sizeof(int32_t) * nout);
    char* ws = nullptr;
    if (int rc = rg_workspace(v, b_colv + b_coli + b_rowv + b_rowi + b_sclv + b_scli + b_ov + b_oi, &ws)) return rc;
    double* colv = (double*)ws; ws += b_colv;
    int32_t* coli = (int32_t*)ws; ws += b_coli;
    double* rowv = (double*)ws; ws += b_rowv;
    int32_t* rowi = (int32_t*)ws; ws += b_rowi;
    double* sclv = (double*)ws; ws += b_sclv;
    int32_t* scli = (int32_t*)ws; ws += b_scli;
    double* ov = (double*)ws; ws += b_ov;
    int32_t* oi = (int32_t*)ws;

    hipLaunchKernelGGL(rg_pass, dim3(ncw, nrb), dim3(RG_NT), 0, v.stream, v.T, v.ld, m, Cm, v.basis, eps,
                       colv, coli, rowv, rowi, sclv, scli);
    LPX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rg_combine, dim3((unsigned)((Cm + m + RG_NT - 1) / RG_NT)), dim3(RG_NT), 0, v.stream, m, Cm, nrb, ncw,
                       colv, coli, rowv, rowi, sclv, scli, ov, oi);
    LPX_HIP_TRY(hipGetLastError());
    std::vector<double> hv(nout);
    std::vector<int32_t> hi(nout);
    LPX_HIP_TRY(hipMemcpyAsync(hv.data(), ov, sizeof(double) * nout, hipMemcpyDeviceToHost, v.stream));
    LPX_HIP_TRY(hipMemcpyAsync(hi.data(), oi, sizeof(int32_t) * nout, hipMemcpyDeviceToHost, v.stream));
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    auto put = [](double* dv, int32_t* di, const double* sv, const int32_t* si, int n) {
        if (dv && n > 0) std::memcpy(dv, sv, sizeof(double) * n);
        if (di && n > 0) std::memcpy(di, si, sizeof(int32_t) * n);
    };
    put(col_inc, col_inc_at, hv.data(), hi.data(), Cm);
    put(col_dec, col_dec_at, hv.data() + Cm, hi.data() + Cm, Cm);
    put(row_inc, row_inc_at, hv.data() + 2 * (size_t)Cm, hi.data() + 2 * (size_t)Cm, m);
    put(row_dec, row_dec_at, hv.data() + 2 * (size_t)Cm + m, hi.data() + 2 * (size_t)Cm + m, m);
    if (min_rhs) *min_rhs = hv[nout - 2];
    if (min_dj) *min_dj = hv[nout - 1];
    return 0;
}

int lpx_tableau_ranging_pairs(lpx_tableau* t, double eps, int K, const int32_t* a, const int32_t* b,
                              double* inc, int32_t* inc_at, double* dec, int32_t* dec_at)
{
    if (K < 0 || (K > 0 && (!a || !b))) { set_error("lpx_tableau_ranging_pairs: bad pair list"); return LPX_EINVAL; }
    if (int rc = rg_check(eps, "lpx_tableau_ranging_pairs")) return rc;
    if (!t) { set_error("lpx_tableau_ranging_pairs: null handle"); return LPX_EINVAL; }
    if (K == 0) return 0;
    TableauView v;
    tableau_view(t, &v);
    const int m = v.R - 1, Cm = v.C - 1;
    for (int k = 0; k < K; ++k)
        if (a[k] < 0 || a[k] >= Cm || b[k] < 0 || b[k] >= Cm) { set_error("lpx_tableau_ranging_pairs: column outside [0, C-1)"); return LPX_EINVAL; }
    const size_t b_ab = up256(sizeof(int32_t) * 2 * (size_t)K), b_ov = up256(sizeof(double) * 2 * (size_t)K), b_oi = up256(sizeof(int32_t) * 2 * (size_t)K);
    char* ws = nullptr;
    if (int rc = rg_workspace(v, b_ab + b_ov + b_oi, &ws)) return rc;
    int32_t* dab = (int32_t*)ws; ws += b_ab;
    double* ov = (double*)ws; ws += b_ov;
    int32_t* oi = (int32_t*)ws;
    std::vector<int32_t> hab(2 * (size_t)K);
    std::memcpy(hab.data(), a, sizeof(int32_t) * K);
    std::memcpy(hab.data() + K, b, sizeof(int32_t) * K);
    LPX_HIP_TRY(hipMemcpyAsync(dab, hab.data(), sizeof(int32_t) * 2 * K, hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(rg_pairs, dim3(K), dim3(RG_NT), 0, v.stream, v.T, v.ld, m, Cm, eps, dab, dab + K, K, ov, oi);
    LPX_HIP_TRY(hipGetLastError());
    std::vector<double> hv(2 * (size_t)K);
    std::vector<int32_t> hi(2 * (size_t)K);
    LPX_HIP_TRY(hipMemcpyAsync(hv.data(), ov, sizeof(double) * 2 * K, hipMemcpyDeviceToHost, v.stream));
    LPX_HIP_TRY(hipMemcpyAsync(hi.data(), oi, sizeof(int32_t) * 2 * K, hipMemcpyDeviceToHost, v.stream));
    LPX_HIP_TRY(hipStreamSynchronize(v.stream));
    if (inc) std::memcpy(inc, hv.data(), sizeof(double) * K);
    if (inc_at) std::memcpy(inc_at, hi.data(), sizeof(int32_t) * K);
    if (dec) std::memcpy(dec, hv.data() + K, sizeof(double) * K);
    if (dec_at) std::memcpy(dec_at, hi.data() + K, sizeof(int32_t) * K);
    return 0;
}

}  // extern "C"
