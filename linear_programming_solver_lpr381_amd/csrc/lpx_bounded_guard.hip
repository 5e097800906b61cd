// lpx_bounded_guard.hip -- the on-chip node with the stall guard (lpx_bounded_node4 / lpx_node_batch_run2 with stall_events > 0),
// gfx950 (CDNA4, wave64).  It is the node of lpx_bounded_node.hip -- its body, lpx_bounded_node_body.h, included a third time, here
// with the file's switch on -- whose dual loop (lpx_onchip_dual.h) keeps two more values, the objective at the last progress and the
// pivots made since, and selects by Bland's rule (least index) once `stall_events` pivots have brought no progress, until the
// objective moves again.  include/lpx.h ("stall guard") is the contract; DESIGN.md section 4.21 has the reasons and the numbers.
// The same layout, the same fit rule and no more LDS, static or dynamic, than the node; no wait on any other workgroup and no spin
// loop: every loop is bounded by max_iter, Cm, R or K, so a launch always ends.  stall_events = 0 never comes here (the host sends
// it to the kernels of lpx_bounded_node.hip).  A file of its own because the kernel's code depends on what else its translation
// unit holds: alone it is the code it was before the text was shared (profiles/r18_onchip_text_isa.md).
#define LPX_ONCHIP_GUARD 1
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"

namespace lpx {

// Workgroup b evaluates P[b] (pinned host memory, read once through a wave-uniform address into scalar registers); the single node
// is a batch of one.  The workgroups share nothing, as in lpx_bounded_nodes_onchip.  Behind each NodeOut, in the same 64-byte slot,
// the kernel leaves the guard record.
__global__ __launch_bounds__(OC_NT) void lpx_bounded_guard_onchip(const NodeParams* __restrict__ P)
{
    const NodeParams N = P[blockIdx.x];
#include "lpx_bounded_node_body.h"
}

hipError_t bounded_guard_init() { return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_guard_onchip)); }

hipError_t launch_bounded_guard_onchip(const NodeParams* P, int B, size_t lds, hipStream_t s)
{
    if (!P || B < 1 || lds > OC_LDS_MAX) return hipErrorInvalidValue;   // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_guard_onchip, dim3(B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
