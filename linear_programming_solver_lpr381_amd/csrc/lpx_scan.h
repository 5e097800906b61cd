// lpx_scan.h -- what the select halves share (private to lpx_kernels.hip, lpx_pivot_fused.hip and lpx_group_fused.hip): the
// entering-column rule of the lookahead scans, the slow-path gather, the compact ratio source and the diagnostic stamps.
#pragma once
#include "lpx_block.h"

namespace lpx {

struct ScanRule { int forced; double eps; double thresh; int c0; int C; };

#ifdef LPX_STAMPS
// Diagnostic build only (never shipped): thread 0 accumulates s_memtime deltas per segment into ws[].
#define LPX_STAMP(slot)                                                                        \
    do { if (threadIdx.x == 0) { unsigned long long now_ = __builtin_amdgcn_s_memtime();       \
         reinterpret_cast<unsigned long long*>(P.ws)[(slot)] += now_ - stamp_prev_; stamp_prev_ = now_; } } while (0)
#define LPX_STAMP_BEGIN unsigned long long stamp_prev_ = __builtin_amdgcn_s_memtime(); \
    unsigned long long rt0_ = __builtin_amdgcn_s_memrealtime();
#define LPX_STAMP_END do { if (threadIdx.x == 0) { reinterpret_cast<unsigned long long*>(P.ws)[14] += __builtin_amdgcn_s_memrealtime() - rt0_; \
    reinterpret_cast<unsigned long long*>(P.ws)[15] += 1; } } while (0)
#define LPX_STAMP_MB(slot)                                                                     \
    do { if (threadIdx.x == 0 && blockIdx.x == 1) { unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
         reinterpret_cast<unsigned long long*>(P.part_v + 128)[(slot)] += now_ - stamp_prev_; stamp_prev_ = now_; } } while (0)
#define LPX_STAMP_END_MB do { if (threadIdx.x == 0 && blockIdx.x == 1) { reinterpret_cast<unsigned long long*>(P.part_v + 128)[14] += __builtin_amdgcn_s_memrealtime() - rt0_; \
    reinterpret_cast<unsigned long long*>(P.part_v + 128)[15] += 1; } } while (0)
#else
#define LPX_STAMP_MB(slot) do {} while (0)
#define LPX_STAMP_END_MB do {} while (0)
#define LPX_STAMP(slot) do {} while (0)
#define LPX_STAMP_BEGIN
#define LPX_STAMP_END do {} while (0)
#endif

__device__ __forceinline__ void rule_init(const ScanRule& R, MinIdx& m)
{
    m.v = R.forced ? 0.0 : -R.eps; m.i = INT_MAX;
}
__device__ __forceinline__ void rule_feed(const ScanRule& R, MinIdx& m, int j, double u)
{
    if (R.forced) {
        if (fabs(u) >= R.thresh) { int off = j - R.c0; if (off < 0) off += R.C; if (off < m.i) m.i = off; }
    } else {
        if (j < R.C - 1 && u < m.v) { m.v = u; m.i = j; }      // ChooseEntering, :205-220
    }
}
__device__ __forceinline__ int rule_decode(const ScanRule& R, const MinIdx& m)
{
    if (m.i == INT_MAX) return -1;
    if (!R.forced) return m.i;
    int q = R.c0 + m.i; if (q >= R.C) q -= R.C;
    return q;
}

// Slow path (once per solve, or after a skipped forced pivot): pick the next column from T as it
// stands and gather it plus the RHS column with strided reads.
template <int NT = SEL_NT>
__device__ int la_prepare_from_T(const SelParams& P, int R, int C, double* buf, int scanrow, const ScanRule& rule,
                                 double* s_v, int* s_i)
{
    const size_t ld = (size_t)P.ld;
    int qn = -1;
    if (scanrow >= 0) {
        MinIdx b; rule_init(rule, b);
        const double* srow = P.T + (size_t)scanrow * ld;
        for (int j = threadIdx.x; j < C; j += NT) rule_feed(rule, b, j, srow[j]);
        b = block_min_idx<NT>(b, s_v, s_i);
        qn = rule_decode(rule, b);
    }
    for (int i = threadIdx.x; i < R; i += NT) {
        if (qn >= 0) buf[i] = P.T[(size_t)i * ld + qn];
        P.rhsbuf[i] = P.T[(size_t)i * ld + (C - 1)];
    }
    return qn;
}

// the ratios of pivot k+1's test, formed once per workgroup into its slice of P.ws: the scan then holds 16 ratios per lane
// and nothing else (a scan over T_k's strided column with the correction applied on the fly needed 168 VGPRs, which
// left the update waves of the same kernel 3 waves per SIMD and the sweep 10 us slower)
struct CompactRatio {
    const double* rat;
    __device__ __forceinline__ double den(int i) const { return rat[i]; }
    __device__ __forceinline__ double num(int) const { return 0.0; }
    __device__ __forceinline__ double value(double a, double) const { return a; }
};

#ifdef LPX_STAMPS
// lpx_g_stamps is one copy per code object: this file's copy added to acc[32] (and cleared); debug_copy_stamps sums the files'
static hipError_t stamps_take(unsigned long long* acc, int clear)
{
    unsigned long long v[32], z[32] = {0};
    hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(lpx_g_stamps), sizeof(v));
    for (int k = 0; k < 32 && e == hipSuccess; ++k) acc[k] += v[k];
    if (e == hipSuccess && clear) e = hipMemcpyToSymbol(HIP_SYMBOL(lpx_g_stamps), z, sizeof(z));
    return e;
}
#endif

}  // namespace lpx
