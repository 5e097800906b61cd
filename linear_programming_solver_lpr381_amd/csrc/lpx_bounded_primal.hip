// lpx_bounded_primal.hip -- the on-chip form of the bounded-variable PRIMAL simplex (lpx_bounded_run2 with LPX_NODE_ONCHIP,
// lpx_node_batch_primal), gfx950 (CDNA4, wave64): ONE launch runs a whole LP from the basis its handle holds, with the tableau in
// the LDS of one compute unit.  It is the root solve of the on-chip branch-and-bound searches and the "many small LPs" call.
//
// Launch shape: ONE workgroup x 1024 lanes per LP -- a grid of one (lpx_bounded_primal_onchip) or of B independent workgroups on B
// handles (lpx_bounded_primals_onchip).
//
// Shared-device rules, held to in this file and in lpx_onchip_primal.h:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic, within a batch or otherwise;
//   * every loop is bounded by max_iter, R, C or Cm; the event loop tests the iteration limit first and makes exactly one event
//     per trip, so it makes at most max_iter + 1 trips, and a launch always ends;
//   * every value is written with ordinary vector stores from C++; there is no inline assembly beyond what lpx_onchip.h has;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.22).
//
// The arithmetic is the contract "bounded-variable primal simplex" of include/lpx.h, step for step that of the launches form
// (lpx_bounded_select + lpx_update): IEEE double, -ffp-contract=off, true division, one multiply and one subtract per update
// element.  The results are bit-equal to that form.
//
// Dynamic LDS (doubles) is the node's, so bounded_node_lds_bytes / lpx_bounded_node_fits is the fit rule unchanged:
//   tile [R * S]        the live window, row stride S = C | 1 (odd: a column walk hits distinct banks, lpx_bounded_node.hip)
//   ub   [C]            upper bounds of the columns
//   buf  [max(R, C)]    the ratios [m], then the pivot-column snapshot [R]
// basis, flip, the trace and the state record stay in global memory (a gather or lane 0's few words per event); the normalised
// pivot row is row r of the tile itself, which the update leaves alone.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants; through lpx_bounded.h bnd_complement, rs_hysteresis and the reductions

namespace lpx {

__global__ __launch_bounds__(OC_NT) void lpx_bounded_primal_onchip(PrimalParams N)
{
#include "lpx_onchip_primal.h"
}

// The batch: workgroup b solves P[b] on its own handle.  The workgroups share nothing, each writes its own handle's memory and its
// own record only, so the result of an entry does not depend on B, on its place in the grid or on how many workgroups run at once.
// P[b] (pinned host memory) is read once through a wave-uniform address.
__global__ __launch_bounds__(OC_NT) void lpx_bounded_primals_onchip(const PrimalParams* __restrict__ P)
{
    const PrimalParams N = P[blockIdx.x];
#include "lpx_onchip_primal.h"
}

hipError_t bounded_primal_init()
{
    hipError_t e = oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_primal_onchip));
    if (e != hipSuccess) return e;
    return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_primals_onchip));
}

hipError_t launch_bounded_primal_onchip(const PrimalParams& n, hipStream_t s)
{
    if (!bounded_node_fits(n.R, n.C)) return hipErrorInvalidValue;      // never launched beyond the LDS of one compute unit
    hipLaunchKernelGGL(lpx_bounded_primal_onchip, dim3(1), dim3(OC_NT), bounded_node_lds_bytes(n.R, n.C), s, n);
    return hipGetLastError();
}

hipError_t launch_bounded_primals_onchip(const PrimalParams* P, int B, size_t lds, hipStream_t s)
{
    if (B < 1 || lds > OC_LDS_MAX) return hipErrorInvalidValue;         // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_primals_onchip, dim3(B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
