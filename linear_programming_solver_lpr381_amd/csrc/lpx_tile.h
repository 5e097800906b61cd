// lpx_tile.h -- what the streaming rank-1 update kernels share (private to lpx_kernels.hip, lpx_pivot_fused.hip and
// lpx_group_fused.hip): tile shapes and size thresholds, the cache-policy switch, the launch helper and the straight-line tile.
#pragma once
#include <cstdlib>
#include <hip/hip_ext.h>
#include "lpx_internal.h"

namespace lpx {

static constexpr int UPD_NT = 256;
static constexpr int UPD_ROWS = 8;
// Streaming variant for tableaux that cannot live in the 256 MiB Infinity Cache: one wave per workgroup, 3 rows per
// wave, non-temporal loads AND stores (`nt`: the lines are not kept in L2 / MALL, where they would only evict each
// other before the next pivot comes round).  Measured on 4097 x 12289 (403 MB), tools/kbench/store_variants.hip:
// 8 rows x 256-lane workgroups, default policy 141.7 us (5.69 TB/s); 3 rows x 64 lanes with nt on both sides 126.9 us
// (6.35 TB/s); nt on one side only, or nt with the 8-row tile, gains nothing.  Below ~1.2x the cache size the default
// policy wins (4096 x 8192 = 256 MiB: 77.7 us vs 83-88 us), so the launcher switches on the tableau's size.
static constexpr int UPDS_NT = 64;
static constexpr int UPDS_ROWS = 3;
static constexpr size_t UPD_STREAM_BYTES = (size_t)292 << 20;   // 306 MB: measured crossover (282 / 298 MB: this kernel wins, 315 MB: the mixed form)
// UPDM: above the cache size, storing ONE of the wave's three rows with the default policy (the other two and all loads
// nontemporal) is worth 5-8 %: that row is written through the Infinity Cache and found there by the next pivot's loads --
// as long as what is kept amounts to about one cache-full.  Measured on the product (tools/probe_policy.py, HIP events) and
// with every store's policy read off the ISA (tools/kbench/sweep_dir.hip, profiles/r02_kbench_sweep_dir.txt):
//   403 / 576 / 784 MB, all nt 126 / 185 / 249 us, LAST row default 116 / 167 / 228 us (first row: 119 / 172 / 229);
//   two rows default: 116 us at 403 MB, 195-202 us at 576 MB (it no longer fits), all default 140 us;
//   1074 / 1441 MB: one row in three no longer fits (347 / 499 us vs 342 / 462 all nt); the same row in every SECOND row
//   block (a sixth of the tableau) 330 / 447 us.
// Hence: one row in three of every `mixmod`-th row block, mixmod = ceil(bytes / 768 MiB); all-nt beyond 8 GiB (unmeasured).
static constexpr size_t UPD_MIXED_BYTES = (size_t)8192 << 20;
static constexpr size_t UPD_MIX_STEP_BYTES = (size_t)768 << 20;
static constexpr size_t FUSED_CACHED_BYTES = (size_t)152 << 20;   // fused (out-of-place) forms: both buffers at home in the Infinity Cache, see fused_policy

// LPX_UPDATE_POLICY=0|1|2 forces one form (diagnostic: tools/probe_policy.py measures the three on one tableau), LPX_UPDATE_MIXMOD=n
// the period of the mixed form; both read once per process.  -1 / 0: not forced.
inline int forced_policy()
{
    static const int forced = [] { const char* e = std::getenv("LPX_UPDATE_POLICY"); return (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : -1; }();
    return forced;
}
inline int forced_mixmod()
{
    static const int forced = [] { const char* e = std::getenv("LPX_UPDATE_MIXMOD"); return e ? std::atoi(e) : 0; }();
    return forced;
}
// which form `bytes` of tableau take: 0 = default policy (they live in the Infinity Cache: up to `cached`), 2 = mixed store policy, 1 = all nt
inline int policy_for(size_t bytes, size_t cached)
{
    if (forced_policy() >= 0) return forced_policy();
    if (bytes <= cached) return 0;
    return bytes <= UPD_MIXED_BYTES ? 2 : 1;
}
// every `mixmod`-th row block of the mixed form keeps one row in three in the cache: about a cache-full of the tableau in all
// (256 MiB at 768 MiB -> every block up to there, every second block up to 1.5 GiB, ...)
inline int mixmod_for(size_t bytes)
{
    if (forced_mixmod() > 0) return forced_mixmod();
    return (int)((bytes + UPD_MIX_STEP_BYTES - 1) / UPD_MIX_STEP_BYTES);
}
inline size_t tableau_bytes(int ld, int R) { return sizeof(double) * (size_t)ld * (size_t)R; }

// One launch; e0/e1 non-null: bracketed by HIP events bound to the kernel.
template <typename... KA, typename... A>
static hipError_t launch_k(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, A... args)
{
    if (e0 && e1) hipExtLaunchKernelGGL(kern, grid, block, lds, s, e0, e1, 0, static_cast<KA>(args)...);
    else hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<KA>(args)...);
    return hipGetLastError();
}

typedef double lpx_d2 __attribute__((ext_vector_type(2)));
// __builtin_nontemporal_load / _store lower to global_load_dwordx4 / global_store_dwordx4 ... nt on gfx950 and stay inside
// hipcc's s_waitcnt bookkeeping (an inline-asm load would not: cdna_hip_programming.md 5.7).
template <bool STREAM> __device__ __forceinline__ double2 upd_load(const double* p)
{
    if constexpr (STREAM) {
        const lpx_d2 v = __builtin_nontemporal_load(reinterpret_cast<const lpx_d2*>(p));
        return make_double2(v.x, v.y);
    } else {
        return *reinterpret_cast<const double2*>(p);
    }
}
template <bool STREAM> __device__ __forceinline__ void upd_store(double* p, double2 o)
{
    if constexpr (STREAM) {
        lpx_d2 v; v.x = o.x; v.y = o.y;
        __builtin_nontemporal_store(v, reinterpret_cast<lpx_d2*>(p));
    } else {
        *reinterpret_cast<double2*>(p) = o;
    }
}

// The same through pointers KNOWN to be global memory.  A kernel that takes its buffers from a parameter record in memory (the
// batched group kernels) sees generic pointers and would issue flat_load / flat_store, which count against both the vector-memory
// and the LDS counter; casting to address space 1 gives global_load_dwordx4 / global_store_dwordx4 as in the single-tableau kernels.
#define LPX_GLOBAL __attribute__((address_space(1)))
// The constant address space, for uniform loads that must stay scalar where stores of the same kernel precede them: only for
// memory that no lane of the launch writes (fused_sweep_strip's factor columns).
#define LPX_CONSTANT __attribute__((address_space(4)))
template <bool STREAM> __device__ __forceinline__ double2 upd_load(const LPX_GLOBAL double* p)
{
    const LPX_GLOBAL lpx_d2* q = (const LPX_GLOBAL lpx_d2*)p;
    lpx_d2 v;
    if constexpr (STREAM) v = __builtin_nontemporal_load(q); else v = *q;
    return make_double2(v.x, v.y);
}
template <bool STREAM> __device__ __forceinline__ void upd_store(LPX_GLOBAL double* p, double2 o)
{
    // The default-policy store is written as two aligned doubles, which the backend's store merging turns into one
    // global_store_dwordx4 (lpx_group_fused_c: 4 of them, as before): as a vector store it would be the nontemporal one but
    // for its metadata, and where a tile spells out both (tile_store) the compiler hoists such a pair out of the branch as ONE
    // store that has lost the policy (seen in lpx_group_fused).  Both facts are the compiler's doing: after a change here or
    // a new toolchain, tools/isa_table.py against the previous build counts the stores per policy and width.
    if constexpr (STREAM) {
        lpx_d2 v; v.x = o.x; v.y = o.y;
        __builtin_nontemporal_store(v, (LPX_GLOBAL lpx_d2*)p);
    } else {
        LPX_GLOBAL double* q = (LPX_GLOBAL double*)__builtin_assume_aligned((void*)p, 16);
        q[0] = o.x; q[1] = o.y;
    }
}

// The straight-line tile every streaming form ends in: a wave's ROWS x 128 block, all rows live, none of them a pivot row,
// nothing to capture.  Loads, arithmetic and stores follow each other without a branch, so the wait counts stay exact (with
// a branch per row the compiler waits for EVERYTHING, the previous row's store acknowledgement included, before each store).
// Three pieces, so that the deferred sweep can apply its D pending pivots between the loads and the stores; P: `double*` or
// `LPX_GLOBAL double*`, const or not.
template <int ROWS, bool NT, typename P>
__device__ __forceinline__ void tile_load(double2 (&v)[ROWS], P sb, size_t ld)
{
#pragma unroll
    for (int k = 0; k < ROWS; ++k) v[k] = upd_load<NT>(sb + (size_t)k * ld);
}
// one pivot: `p` the lane's pair of the normalised pivot row, fac[i0 + k] the factor of the tile's row k
template <int ROWS, typename P>
__device__ __forceinline__ void tile_pivot(double2 (&v)[ROWS], double2 p, P fac, int i0)
{
    double f[ROWS];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) f[k] = fac[i0 + k];
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        v[k].x = v[k].x - f[k] * p.x;           // mul, then sub: contraction is off
        v[k].y = v[k].y - f[k] * p.y;
    }
}
// Mixed form: the LAST row of the wave goes through the Infinity Cache (default policy) in every `mixmod`-th row block,
// everything else is non-temporal; two spelled-out sequences so that no store loses its policy when the compiler merges code
// (checked in the ISA, tools/isa_table.py: hipcc keeps `nt` as metadata only).  MIX: 0 = no mixed form, MIX_INPLACE = the
// in-place kernels' argument (always >= 1), MIX_SWEEP = the out-of-place kernels' (0: no block mixes) -- two spellings of
// the test because each compiles to the code its kernels were measured with.
enum { MIX_NONE = 0, MIX_INPLACE = 1, MIX_SWEEP = 2 };
template <int ROWS, bool NT, int MIX, typename P>
__device__ __forceinline__ void tile_store(P db, size_t ld, const double2 (&v)[ROWS], int rb, int mixmod)
{
    if ((MIX == MIX_INPLACE && (mixmod <= 1 || rb % mixmod == 0)) ||
        (MIX == MIX_SWEEP && mixmod > 0 && (mixmod == 1 || rb % mixmod == 0))) {
#pragma unroll
        for (int k = 0; k < ROWS - 1; ++k) upd_store<true>(db + (size_t)k * ld, v[k]);
        upd_store<false>(db + (size_t)(ROWS - 1) * ld, v[ROWS - 1]);
    } else {
#pragma unroll
        for (int k = 0; k < ROWS; ++k) upd_store<NT>(db + (size_t)k * ld, v[k]);
    }
}
// the whole tile for one pivot (in place: sb == db)
template <int ROWS, bool NT, int MIX, typename SP, typename DP, typename FP>
__device__ __forceinline__ void upd_plain_tile(SP sb, DP db, size_t ld, double2 p, FP fac, int i0, int rb, int mixmod)
{
    double2 v[ROWS];
    tile_load<ROWS, NT>(v, sb, ld);
    tile_pivot<ROWS>(v, p, fac, i0);
    tile_store<ROWS, NT, MIX>(db, ld, v, rb, mixmod);
}

}  // namespace lpx
