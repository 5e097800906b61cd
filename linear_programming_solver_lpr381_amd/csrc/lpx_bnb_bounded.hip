// lpx_bnb_bounded.hip -- the device side of branch and bound by bound changes, gfx950 (CDNA4, wave64): the two kernels of
// lpx_tableau_dualize, the kernel of lpx_tableau_branch_pick and the small save / restore of the bounds lpx_bounded_node edits.
//
// The representation is the one of lpx_bounded.hip and lpx_bounded_dual.hip: ub[j], flip[j] and the lower shift lo[j] beside the
// tableau.  The arithmetic contract is in include/lpx.h ("branch and bound by bound changes"); DESIGN.md section 4.15 has the
// launch shape.  Built with -ffp-contract=off.  The flagged dual loop (lpx_bounded_dual_run2) is the second instantiation of
// lpx_bounded_dual_select in lpx_bounded_dual.hip.
#include "lpx_block.h"

namespace lpx {

// ---- lpx_tableau_dualize: two launches, neither reads what it writes ---------------------------------------------------------
// Launch 1 (one workgroup): the ordered compaction of J = { j < Cm : T[m,j] < -eps and 0 < ub[j] < +inf } over the objective row,
// 1024 columns per step: a ballot per wave, a prefix over the 16 wave totals, the running count carried from step to step.
// It reads the objective row and ub and writes only `list` and `cnt`.
__global__ __launch_bounds__(SEL_NT) void lpx_dualize_list(const double* __restrict__ zrow, int Cm, const double* __restrict__ ub,
                                                           double eps, int32_t* __restrict__ list, int32_t* __restrict__ cnt)
{
    __shared__ int s_tot[SEL_NW];
    __shared__ int s_bad[SEL_NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double inf = __builtin_inf();
    int n = 0, bad = 0;                                   // uniform: columns listed so far, unrepairable columns so far
    for (int base = 0; base < Cm; base += SEL_NT) {       // uniform trip count: every lane reaches every barrier
        const int j = base + t;
        bool in = false, un = false;
        if (j < Cm) {
            const bool neg = zrow[j] < -eps;
            const double u = ub[j];
            in = neg && u > 0.0 && u < inf;
            un = neg && u == inf;                         // cannot be repaired by a flip: counted, left alone
        }
        const unsigned long long mi = __ballot(in), mu = __ballot(un);
        const int before = __popcll(mi & ((1ull << lane) - 1ull));
        __syncthreads();                                  // the totals of the step before have been read
        if (lane == 0) { s_tot[wave] = __popcll(mi); s_bad[wave] = __popcll(mu); }
        __syncthreads();
        int pre = 0, tot = 0, btot = 0;
        for (int w = 0; w < SEL_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; btot += s_bad[w]; }
        if (in) list[n + pre + before] = j;               // n + pre + before < number of columns tested so far <= Cm
        n += tot; bad += btot;
    }
    if (t == 0) { cnt[0] = n; cnt[1] = bad; }
}

// Launch 2: one lane per row walks the list in order: T[i,Cm] = T[i,Cm] - ub[j]*T[i,j] (one multiply, one subtract: contraction
// is off), T[i,j] = -T[i,j].  A lane reads and writes its own row only; the first workgroup also toggles the flips (the columns
// of the list are distinct).
static constexpr int DZ_NT = 256;

__global__ __launch_bounds__(DZ_NT) void lpx_dualize_apply(double* __restrict__ T, int ld, int R, int Cm, const double* __restrict__ ub,
                                                           uint8_t* __restrict__ flip, const int32_t* __restrict__ list,
                                                           const int32_t* __restrict__ cnt, double* __restrict__ rhsbuf)
{
    const int n = cnt[0];                                 // uniform: a scalar load
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < n; k += DZ_NT) flip[list[k]] ^= 1;
    const int i = blockIdx.x * DZ_NT + threadIdx.x;
    if (i >= R) return;
    double* row = T + (size_t)i * ld;
    double b = row[Cm];
    for (int k = 0; k < n; ++k) {
        const int j = list[k];                            // uniform
        const double a = row[j];
        const double prod = ub[j] * a;
        b = b - prod;
        row[j] = -a;
    }
    row[Cm] = b;
    rhsbuf[i] = b;                                        // the contiguous copy the loops read
}

hipError_t launch_dualize_list(const double* T, int ld, int R, int Cm, const double* ub, double eps, int32_t* list, int32_t* cnt,
                               hipStream_t s)
{
    hipLaunchKernelGGL(lpx_dualize_list, dim3(1), dim3(SEL_NT), 0, s, T + (size_t)(R - 1) * ld, Cm, ub, eps, list, cnt);
    return hipGetLastError();
}

hipError_t launch_dualize_apply(double* T, int ld, int R, int Cm, const double* ub, uint8_t* flip, const int32_t* list,
                                const int32_t* cnt, double* rhsbuf, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_dualize_apply, dim3((R + DZ_NT - 1) / DZ_NT), dim3(DZ_NT), 0, s, T, ld, R, Cm, ub, flip, list, cnt, rhsbuf);
    return hipGetLastError();
}

// ---- ub / lo of the columns a node edits, kept so that a refused edit leaves the handle as it was ------------------------------
__global__ __launch_bounds__(DZ_NT) void lpx_bounds_save(int K, const int32_t* __restrict__ cols, double* __restrict__ ub,
                                                         double* __restrict__ lo, double* __restrict__ save, int restore)
{
    const int k = blockIdx.x * DZ_NT + threadIdx.x;
    if (k >= K) return;
    const int j = cols[k];
    if (restore) { ub[j] = save[2 * k]; lo[j] = save[2 * k + 1]; }
    else { save[2 * k] = ub[j]; save[2 * k + 1] = lo[j]; }
}

hipError_t launch_bounds_save(int K, const int32_t* cols, double* ub, double* lo, double* save, int restore, hipStream_t s)
{
    if (K <= 0) return hipSuccess;
    hipLaunchKernelGGL(lpx_bounds_save, dim3((K + DZ_NT - 1) / DZ_NT), dim3(DZ_NT), 0, s, K, cols, ub, lo, save, restore);
    return hipGetLastError();
}

// ---- lpx_tableau_branch_pick: one workgroup ---------------------------------------------------------------------------------
// The value of every column j < nint is scattered from the basic rows into an array of nint doubles (LDS up to 4096 entries, the
// handle's scratch beyond), x_j is formed exactly as lpx_tableau_bounded_solution forms it, and a block reduction over
// (|f - 0.5|, j) with the lowest index on equal distances picks the branching variable.  Comparisons only: the pick does not
// depend on how the columns are dealt to the lanes.
static constexpr int PICK_LDS_DOUBLES = 4096;

__device__ __forceinline__ double pick_value(const PickParams& p, const double* vals, int j)
{
    const double v = vals[j];
    double x = p.flip[j] ? p.ub[j] - v : v;
    if (p.lo) x = x + p.lo[j];
    return x;
}

__global__ __launch_bounds__(SEL_NT) void lpx_branch_pick_kernel(PickParams p)
{
    __shared__ double s_val[PICK_LDS_DOUBLES];
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];
    const int t = threadIdx.x;
    const int m = p.R - 1, nint = p.nint;
    double* vals = nint <= PICK_LDS_DOUBLES ? s_val : p.ws;
    for (int j = t; j < nint; j += SEL_NT) vals[j] = 0.0;               // a nonbasic column is at +0.0
    __syncthreads();
    for (int i = t; i < m; i += SEL_NT) {
        const int pb = p.basis[i];
        if ((unsigned)pb < (unsigned)nint) vals[pb] = p.T[(size_t)i * p.ld + p.Cm];
    }
    __syncthreads();
    MinIdx best; best.v = __builtin_inf(); best.i = INT_MAX;
    int nc = 0;
    for (int j = t; j < nint; j += SEL_NT) {                            // ascending j per lane: a strict `<` keeps the lowest
        if (p.is_int && !p.is_int[j]) continue;
        const double x = pick_value(p, vals, j);
        const double f = x - __builtin_floor(x);
        if (f > p.tol && (1.0 - f) > p.tol) {
            const double d = __builtin_fabs(f - 0.5);
            ++nc;
            if (d < best.v) { best.v = d; best.i = j; }
        }
    }
    best = block_min_idx(best, s_v, s_i);
    int total = 0;
    block_excl_scan_sum(nc, s_i, &total);
    if (t == 0) {
        const int var = best.i == INT_MAX ? -1 : best.i;
        p.out->var = var;
        p.out->candidates = total;
        p.out->x_var = var >= 0 ? pick_value(p, vals, var) : 0.0;
        p.out->z = p.T[(size_t)m * p.ld + p.Cm];
    }
}

hipError_t launch_branch_pick(const PickParams& p, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_branch_pick_kernel, dim3(1), dim3(SEL_NT), 0, s, p);
    return hipGetLastError();
}

}  // namespace lpx
