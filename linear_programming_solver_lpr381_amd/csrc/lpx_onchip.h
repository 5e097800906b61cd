// lpx_onchip.h -- what the on-chip forms of the bounded branch-and-bound node share as an ordinary header: lpx_bounded_node.hip (the
// node and the batch), lpx_bounded_guard.hip (the guarded node), lpx_bounded_fix.hip (the node with reduced-cost tightening),
// lpx_bounded_plunge.hip and lpx_bounded_probe.hip.  The launch constants, the refusal record
// and the wave-uniform helpers stand here once.  The steps of a node are not functions but included text, one file per step
// (lpx_onchip_count.h, lpx_onchip_flips.h, lpx_onchip_dual.h, lpx_onchip_pick.h; the reason is in lpx_bounded_node_body.h).  The fit
// rule (bounded_node_lds_bytes, bounded_node_fits) is declared in lpx_internal.h, where the host files see it, and defined in
// lpx_bounded_node.hip from the constants below.
#pragma once
#include "lpx_bounded.h"       // bnd_complement; through lpx_resident.h rs_hysteresis, through lpx_block.h the reductions

namespace lpx {

// Whether the kernels of a file carry the stall guard in their dual loop is the file's switch, LPX_ONCHIP_GUARD, defined (0 or 1) in
// front of this header.  The step files read it as the constant GUARD; lpx_onchip_dual.h also has one `#if` on it.
#ifndef LPX_ONCHIP_GUARD
#error "define LPX_ONCHIP_GUARD as 0 or 1 in front of lpx_onchip.h"
#endif
static constexpr bool GUARD = LPX_ONCHIP_GUARD != 0;
// Whether the node body carries the reduced-cost tightening step (lpx_onchip_fix.h, between the pick and the write-back) is a
// second switch of the same kind, LPX_ONCHIP_FIX: 1 in lpx_bounded_fix.hip alone, 0 in every other file, whose kernels keep the
// text they had.  It is read by the preprocessor only: the body has one `#if` on it around the step and one around the count in the
// record (the step's names do not exist in the other kernels, so a constant would not do).
#ifndef LPX_ONCHIP_FIX
#error "define LPX_ONCHIP_FIX as 0 or 1 in front of lpx_onchip.h"
#endif

static constexpr int OC_NT = SEL_NT, OC_NW = SEL_NW;    // one workgroup x 1024 lanes per node, 16 waves
static constexpr size_t OC_LDS_TOTAL = 160 * 1024;      // one compute unit
static constexpr size_t OC_LDS_STATIC = 2048;           // reserved for the statics of a kernel (reduction scratch, counters)
static constexpr size_t OC_LDS_MAX = OC_LDS_TOTAL - OC_LDS_STATIC;     // the most dynamic LDS a launch may ask for
static constexpr size_t OC_REC = 64;                    // the records of a slab (and of a chain) are 64 bytes apart

__device__ __forceinline__ NodeOut* oc_rec(const NodeParams& N, int s)
{
    return reinterpret_cast<NodeOut*>(reinterpret_cast<char*>(N.out) + OC_REC * (size_t)s);
}

// The record of a refused edit, written by lane 0 into record s.  GUARD: the guard record behind it, in the same 64-byte slot.
// LATE (the plunge): the zero goes through an empty asm, so that the record's constants are formed here, on this rare path, and
// not kept in registers across the whole chain (where they spilled to scratch).
template <bool GUARD, bool LATE>
__device__ __forceinline__ void oc_refuse(const NodeParams& N, int s, int t, int bad, int inf_k)
{
    if (t == 0) {
        int zero = 0;
        if (LATE) asm volatile("" : "+v"(zero));
        NodeOut* o = oc_rec(N, s);
        o->status = zero - 1; o->events = zero; o->kind0 = zero; o->kind1 = zero; o->flips = zero; o->unrepairable = bad; o->inf_k = inf_k;
        o->var = zero - 1; o->candidates = zero; o->x_var = (double)zero; o->z = (double)zero;
        if (GUARD) { GuardOut* g = reinterpret_cast<GuardOut*>(o); g->bland_events = 0; g->first_bland = -1; }
    }
}

// v is the same in every lane: its bits through readfirstlane, so that the compiler keeps it in scalar registers
__device__ __forceinline__ double oc_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// the one-time function attribute of an on-chip kernel: it may ask for all the dynamic LDS the fit rule admits
inline hipError_t oc_allow_lds(const void* kernel)
{
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OC_LDS_MAX);
}

}  // namespace lpx
