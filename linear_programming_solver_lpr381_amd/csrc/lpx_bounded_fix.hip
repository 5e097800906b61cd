// lpx_bounded_fix.hip -- the on-chip node with reduced-cost bound tightening (lpx_bounded_node5 / lpx_node_batch_run3 with a finite
// fix_bound), gfx950 (CDNA4, wave64).  It is the node of lpx_bounded_node.hip -- its body, lpx_bounded_node_body.h, included a fourth
// time, here with both file switches on: the stall guard in its dual loop, as in lpx_bounded_guard.hip, and behind the pick step 7b
// (lpx_onchip_fix.h), which tightens the range of every nonbasic integer column whose reduced cost leaves it less room than its
// range before the objective falls to fix_bound, and lists what it tightened.  include/lpx.h ("reduced-cost tightening") is the
// contract; DESIGN.md section 4.24 has the reasons and the numbers.
// One kernel serves the driver: the host sends stall_events = INT_MAX for "no guard", with which the guard's loop never enters
// Bland mode and is the unguarded loop bit for bit.  The same layout, the same fit rule and no more LDS, static or dynamic, than the
// node: the marks of the basic columns live in `buf`, which is free behind the pick.  No wait on any other workgroup, no spin loop
// and no atomic: every loop is bounded by max_iter, Cm, R, K or nint, so a launch always ends.  fix_bound = -inf never comes here
// (the host sends it to the kernels of lpx_bounded_node.hip and lpx_bounded_guard.hip).  A file of its own because a kernel's code
// depends on what else its translation unit holds (profiles/r18_onchip_text_isa.md): the other on-chip kernels keep their text.
#define LPX_ONCHIP_GUARD 1
#define LPX_ONCHIP_FIX 1
#include "lpx_onchip.h"

namespace lpx {

// Workgroup b evaluates P[b] (pinned host memory, read once through a wave-uniform address into scalar registers); the single node
// is a batch of one.  The workgroups share nothing.  The count of the tightened columns goes into the node record's spare word,
// the triples into the entry's own arrays.
__global__ __launch_bounds__(OC_NT) void lpx_bounded_fix_onchip(const FixParams* __restrict__ P)
{
    const NodeParams N = P[blockIdx.x].n;
    const double fix_bound = P[blockIdx.x].fix_bound;
    int32_t* const fcols = P[blockIdx.x].cols;
    double* const flower = P[blockIdx.x].lower;
    double* const fupper = P[blockIdx.x].upper;
#include "lpx_bounded_node_body.h"
}

hipError_t bounded_fix_init() { return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_fix_onchip)); }

hipError_t launch_bounded_fix_onchip(const FixParams* P, int B, size_t lds, hipStream_t s)
{
    if (!P || B < 1 || lds > OC_LDS_MAX) return hipErrorInvalidValue;   // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_fix_onchip, dim3(B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
