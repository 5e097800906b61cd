// lpx_bounded_node.hip -- the on-chip form of a branch-and-bound node by bound changes (lpx_bounded_node3 with
// LPX_NODE_ONCHIP), gfx950 (CDNA4, wave64): ONE launch evaluates a whole node with the tableau in the LDS of one compute unit.
//
// Launch shape: ONE workgroup x 1024 lanes per node -- a grid of one (lpx_bounded_node_onchip) or of B independent workgroups on B
// handles (lpx_bounded_nodes_onchip, the batch).  There is no wait on any other workgroup and no spin loop anywhere;
// every loop is bounded by max_iter, Cm, R or K (the event loop makes at least one event per trip and tests the iteration limit
// first, so it makes at most max_iter + 1 trips).  A launch therefore always ends, which makes it safe on a shared device.
//
// The arithmetic is that of the contracts in include/lpx.h ("bounded dual simplex", "branch and bound by bound changes",
// "long-step ratio test, objective cutoff and dual start"), step for step the arithmetic of the launches form
// (lpx_bounded_node2: lpx_bounds_save / _shift / _apply, lpx_dualize_list / _apply, lpx_bounded_dual_select or
// lpx_bounded_long_select + lpx_update, lpx_branch_pick_kernel): IEEE double, -ffp-contract=off, true division, one multiply
// and one subtract per update element.  The results are bit-equal to that form.  DESIGN.md section 4.17 has the layout.
//
// The three flags are uniform branches of one kernel, not eight instantiations: each flag guards a few instructions off the
// update loop, so a template would multiply the code by eight without freeing a register.
//
// Dynamic LDS (doubles; bounded_node_lds_bytes is the rule, lpx_bounded_node_fits its public face):
//   tile [R * S]        the live window, row stride S = C | 1.  MI355X LDS: ds_read_b64 serves a wave in two groups of 32 lanes
//                       over 32 eight-byte banks, ds_write_b64 in four groups of 16 over 32 four-byte banks; a column walk puts
//                       lane i at double i * S, which hits distinct banks in both cases iff S is odd.  A row walk is contiguous.
//   ub   [C]            upper bounds of the columns (the edit of this node applied)
//   buf  [max(R, C)]    whatever one step needs and the next does not: the ratios, then the pivot column snapshot; the column
//                       list of the dual-feasibility flips (int32); the values of the pick.  The leaving row needs no array.
// basis, flip, lo, the trace and the state record stay in global memory (a gather or lane 0's few words per event); the
// normalised pivot row is row r of the tile itself, which the update leaves alone.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants, the refusal record; through lpx_bounded.h the shared device pieces

namespace lpx {

size_t bounded_node_lds_bytes(int R, int C)
{
    const size_t S = (size_t)C | 1, mx = (size_t)(R > C ? R : C);
    return sizeof(double) * ((size_t)R * S + (size_t)C + mx);
}

int bounded_node_fits(int R, int C)
{
    if (R < 2 || C < 1) return 0;
    return bounded_node_lds_bytes(R, C) <= OC_LDS_MAX ? 1 : 0;
}

// One node on one workgroup.  The body is lpx_bounded_node_body.h, the text of these two kernels and of the guarded one (the reason
// is in that file): N is uniform over the workgroup, and every `return` of the body is taken by all of its lanes.  The stall guard
// is off in this file; lpx_bounded_guard.hip has it on.
__global__ __launch_bounds__(OC_NT) void lpx_bounded_node_onchip(NodeParams N)
{
#include "lpx_bounded_node_body.h"
}

// The batch (lpx_node_batch_run): a grid of B workgroups, workgroup b evaluates P[b] on its own handle.  The workgroups share
// nothing: no wait, no flag, no atomic between them, each writes its own handle's memory and its own records only, so the result
// of an entry does not depend on B, on its place in the grid or on how many workgroups run at once, and a refused entry's early
// return holds nobody up.  P[b] (pinned host memory) is read once through a wave-uniform address into scalar registers.
__global__ __launch_bounds__(OC_NT) void lpx_bounded_nodes_onchip(const NodeParams* __restrict__ P)
{
    const NodeParams N = P[blockIdx.x];
#include "lpx_bounded_node_body.h"
}

hipError_t bounded_node_init()
{
    hipError_t e = oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_node_onchip));
    if (e != hipSuccess) return e;
    return oc_allow_lds(reinterpret_cast<const void*>(lpx_bounded_nodes_onchip));
}

hipError_t launch_bounded_node_onchip(const NodeParams& n, hipStream_t s)
{
    if (!bounded_node_fits(n.R, n.C)) return hipErrorInvalidValue;      // never launched beyond the LDS of one compute unit
    hipLaunchKernelGGL(lpx_bounded_node_onchip, dim3(1), dim3(OC_NT), bounded_node_lds_bytes(n.R, n.C), s, n);
    return hipGetLastError();
}

hipError_t launch_bounded_nodes_onchip(const NodeParams* P, int B, size_t lds, hipStream_t s)
{
    if (B < 1 || lds > OC_LDS_MAX) return hipErrorInvalidValue;         // the caller checks the fit of every entry
    hipLaunchKernelGGL(lpx_bounded_nodes_onchip, dim3(B), dim3(OC_NT), lds, s, P);
    return hipGetLastError();
}

}  // namespace lpx
