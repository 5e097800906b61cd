// lpx_internal.h -- shared between the HIP kernels and the host-side C ABI of liblpx.so (the handle itself: lpx_handle.h, host only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <functional>
#include <mutex>
#include "../../include/lpx.h"

namespace lpx {

// Device-resident loop state: one instance per tableau handle, written only by the select kernel.
struct DevState {
    int status;          // LPX_RUNNING until a terminal status is reached
    int iter;            // pivots completed (index of the next trace slot)
    int r, q;            // pivot chosen by the last select launch (r < 0: nothing to update)
    int phase;           // 0 = ForceDualFeasibility, 1 = dual loop, 2 = primal loop
    int fdf_count;       // pivots done in phase 0
    int dual_iter;       // pivots done in phase 1
    int primal_count;    // pivots done in phase 2
    int forced_k;        // next entry of the forced-pivot list
    int qn;              // lookahead: entering column of the NEXT pivot (-1 = none), see lpx_select_la
    int c0n;             // multi-workgroup select: start column of the next forced search
    int qn_valid;        // multi-workgroup select: 1 = `qn` above overrides the partial reduction
    int pad[4];          // pad[0]: revised path's Nidx order counter; pad[1]: resident loop abort flag
};

enum { MODE_PRIMAL = 0, MODE_DUAL = 1, MODE_FORCED = 2, MODE_BOUNDED = 3 };

struct SelParams {
    double* T; int ld; int R; int C;    // R, C: CAPACITY of the handle (grid sizing)
    const int32_t* shape;               // device record {R, C} of the tableau currently in the handle
    double* prow;        // [ld]  normalised pivot row  T[r,:]/T[r,q]
    double* pcol;        // [R]   pivot column snapshot T[:,q]        (dual path)
    double* col0;        // [R]   lookahead column buffers, ping-pong   (primal / forced path)
    double* col1;
    double* rhsbuf;      // [R]   contiguous copy of the RHS column
    int32_t* basis;      // [R-1]
    int32_t* trace;      // [2*trace_cap]
    int trace_cap;
    DevState* st;        // written by select (block 0), read by update and the host
    DevState* us;        // multi-workgroup select: written by update (block 0), read by select
    double* part_v; int32_t* part_i; int nblk;   // per-workgroup partial argmins of the lookahead scan
    int qsel;                                    // 1: select's last workgroup reduces them (streaming update forms), 0: every update wave does
    double eps;          // Eps
    double tol_fdf;      // ratio hysteresis in phase 0
    double tol_dual;     // ratio hysteresis in phase 1
    double tol_primal;   // ratio hysteresis in phase 2
    int max_iter, fdf_guard, cleanup, mode;
    const int32_t* frows; const int32_t* fcols; int fcount; double fthresh; int32_t* fchosen;
    double* ws;          // [max(R,C)] global scratch for ratios when they do not fit LDS
    int rcap;            // doubles of dynamic LDS available for ratios (0 = use ws)
};

// the bounded-variable loops (lpx_bounded.hip, lpx_bounded_dual.hip, lpx_bounded_long.hip; shared device pieces in lpx_bounded.h):
// the select parameters plus the bounds kept beside the tableau
struct BndParams {
    SelParams P;
    const double* ub;    // [C-1 capacity] upper bound of every column, +inf = none
    uint8_t* flip;       // [C-1 capacity] 1 = the column stands for u_j - x_j
    int dual;            // the form word: 0 = the primal loop, 1 + flags (LPX_BDUAL_*) = the dual loop with that flag set.  It
                         // picks the kernel instantiation in the launcher, and as part of the record it keeps the cached
                         // graphs of the forms apart.  lpx_bounded_dual_run is 1, _run2 with LPX_BDUAL_SKIP_FIXED is 2.
    const double* cutoff;   // dual loop with LPX_BDUAL_CUTOFF: the handle's device double (a pointer, never the value:
                            // the record keys the cached graph and a driver moves the cutoff at every incumbent); else nullptr
};
hipError_t launch_bounded_select(const BndParams& b, hipStream_t s);
// every form of the dual loop, picked by b.dual (lpx_bounded_long.hip); hipErrorInvalidValue for a word that is no form
hipError_t launch_bounded_dual_select(const BndParams& b, hipStream_t s);

// branch and bound by bound changes (lpx_bnb_bounded.hip)
// list[0..count) = ascending columns j < Cm with T[m,j] < -eps and 0 < ub[j] < +inf; cnt = {count, unrepairable}
hipError_t launch_dualize_list(const double* T, int ld, int R, int Cm, const double* ub, double eps, int32_t* list, int32_t* cnt,
                               hipStream_t s);
// every row: RHS -= ub[j] * T[i,j] for j of the list in order, T[i,j] negated; flip[j] ^= 1; rhsbuf kept current
hipError_t launch_dualize_apply(double* T, int ld, int R, int Cm, const double* ub, uint8_t* flip, const int32_t* list,
                                const int32_t* cnt, double* rhsbuf, hipStream_t s);
// ub / lo of cols[0..K) into save[2K] (restore = 0) or back from it (restore = 1)
hipError_t launch_bounds_save(int K, const int32_t* cols, double* ub, double* lo, double* save, int restore, hipStream_t s);
// the two launches of a bound change: shift[k] from the old lo / ub / flip of cols[k], new ub / lo stored; then T[:,Cm] and rhsbuf
// shifted, k in order (R rows)
hipError_t launch_bounds_shift(int K, const int32_t* cols, const double* lower, const double* upper, double* ub, double* lo,
                               const uint8_t* flip, double* shift, hipStream_t s);
hipError_t launch_bounds_apply(double* T, int ld, int R, int Cm, int K, const int32_t* cols, const double* shift, double* rhsbuf,
                               hipStream_t s);
struct PickParams {
    const double* T; int ld, R, Cm;
    const int32_t* basis; const double* ub; const uint8_t* flip; const double* lo;   // lo = nullptr: no lower shift stored
    int nint; const uint8_t* is_int; double tol;
    double* ws;          // [nint] values when nint is above the on-chip array
    lpx_branch_pick* out;
};
hipError_t launch_branch_pick(const PickParams& p, hipStream_t s);

// the on-chip node (lpx_bounded_node.hip): one launch of one workgroup evaluates a whole node with the tableau in LDS
// What a node call sends: this header and behind it lower[K], upper[K] (double) and cols[K] (int32), in the handle's pinned slab.
struct NodeIn {
    int32_t K, flags, nint, has_mask, max_iter, lo_used;               // lo_used: the handle has stored a lower shift (this edit included)
    int32_t stall_events, pad;                                         // stall_events: read by the guarded node alone (lpx_bounded_guard.hip)
    double eps, ratio_tol, cutoff, tol;
};
static_assert(sizeof(NodeIn) == 64, "the arrays behind the header start on a double");
// What it gets back, written by the kernel into the same slab.  status -1: the edit was refused and the handle is as it was --
// inf_k >= 0: upper[inf_k] = +inf on a flipped column; else `unrepairable` columns that no flip can make dual feasible.
struct NodeOut {
    int32_t status, events, kind0, kind1, flips, unrepairable, inf_k, var, candidates, pad;
    double x_var, z;
};
struct NodeParams {
    double* T; int ld, R, C;             // R, C: the LIVE shape
    double* rhsbuf; int32_t* basis; int32_t* trace; int trace_cap; DevState* st;
    double* ub; double* lo; uint8_t* flip;
    double* edit;                        // device staging of the edit, in the layout of BoundEdit: 5 K doubles and K int32
    const uint8_t* mask;                 // [nint] device copy of the integer mask (read when NodeIn::has_mask)
    const NodeIn* in; NodeOut* out;
};
size_t bounded_node_lds_bytes(int R, int C);        // dynamic LDS of the launch for a live R x C window
int bounded_node_fits(int R, int C);                // pure host arithmetic: 1 iff that and the kernel's statics fit one compute unit
hipError_t bounded_node_init();                     // one-time function attribute
hipError_t launch_bounded_node_onchip(const NodeParams& n, hipStream_t s);
// the batch: workgroup b evaluates P[b] (an array the device can read); lds = the largest entry's bounded_node_lds_bytes
hipError_t launch_bounded_nodes_onchip(const NodeParams* P, int B, size_t lds, hipStream_t s);
// the guarded node (lpx_bounded_guard.hip): the on-chip node with the stall guard of include/lpx.h in its dual loop, NodeIn::stall_events
// > 0.  One batch-shaped kernel: workgroup b evaluates P[b] (an array the device can read); the single node is a batch of one.  Behind
// each NodeOut, in the same 64-byte slot of the slab, it leaves the guard record.
struct GuardOut { NodeOut o; int32_t bland_events, first_bland; };
static_assert(sizeof(GuardOut) == 64, "the node record and the guard record share one 64-byte slot");
hipError_t bounded_guard_init();                    // one-time function attribute
hipError_t launch_bounded_guard_onchip(const NodeParams* P, int B, size_t lds, hipStream_t s);
// the node with reduced-cost tightening (lpx_bounded_fix.hip): the guarded node with step 7b (lpx_onchip_fix.h) behind its pick.
// One batch-shaped kernel; NodeIn::stall_events = INT_MAX stands for "no guard".  fix_bound travels around the node's record, so
// NodeIn and the records of the other kernels stay as they are.  cols / lower / upper: the entry's list of tightened columns, nint
// entries each, in memory the host reads after its one wait; their count comes back in NodeOut::pad, the one spare word of the
// 64-byte record slot (the guard record fills the rest), which no other kernel writes.
struct FixParams { NodeParams n; double fix_bound; int32_t* cols; double* lower; double* upper; };
hipError_t bounded_fix_init();                      // one-time function attribute
hipError_t launch_bounded_fix_onchip(const FixParams* P, int B, size_t lds, hipStream_t s);
// the plunge (lpx_bounded_plunge.hip): workgroup b evaluates a chain of up to P[b].depth nodes with the tile staying in LDS.
// n.out is the first of `depth` records, 64 bytes apart; *steps = the records written; the chain stops at z <= prune.
struct PlungeParams { NodeParams n; double prune; int32_t* steps; int32_t depth, pad; };
hipError_t bounded_plunge_init();                   // one-time function attribute
hipError_t launch_bounded_plunge_onchip(const PlungeParams* P, int B, size_t lds, hipStream_t s);
// the probes (lpx_bounded_probe.hip): workgroup (w, e) evaluates child w of entry P[e]'s handle as it stands and writes rec[w];
// workgroup (0, e) writes *head.  Everything of the handle is read only.  front: the record of the node launched in front of the
// probes on the same stream (status < 0: refused, nothing is probed), or null.  wbasis / wflip: 2 * cand_max slices of the
// workspace, wbasis_stride int32 / wflip_stride bytes apart.
struct ProbeParams {
    const double* T; int ld, R, C;       // R, C: the LIVE shape
    const int32_t* basis; const DevState* st;
    const double* ub; const double* lo; const uint8_t* flip;
    const uint8_t* mask;                 // [nint] device copy of the integer mask (read when has_mask)
    const NodeOut* front;
    int32_t* wbasis; uint8_t* wflip; int32_t wbasis_stride, wflip_stride;
    lpx_probe_head* head; lpx_probe_record* rec;
    double eps, ratio_tol, cutoff, tol, prune;
    int32_t flags, nint, has_mask, lo_used, probe_iter, cand_max;
};
hipError_t bounded_probe_init();                    // one-time function attribute
hipError_t launch_bounded_probe_onchip(const ProbeParams* P, int B, int cand_max, size_t lds, hipStream_t s);
// the on-chip bounded primal loop (lpx_bounded_primal.hip): one launch of one workgroup runs a whole LP from the basis its handle
// holds, with the tableau in LDS.  The LDS rule is the node's (bounded_node_lds_bytes).  out: the 40-byte record of include/lpx.h
// in pinned host memory, the records of a batch 64 bytes apart.
struct PrimalParams {
    double* T; int ld, R, C;             // R, C: the LIVE shape
    double* rhsbuf; int32_t* basis; int32_t* trace; int trace_cap; DevState* st;
    const double* ub; uint8_t* flip;
    double eps, ratio_tol; int32_t max_iter, pad;
    lpx_primal_record* out;
};
hipError_t bounded_primal_init();                   // one-time function attribute
hipError_t launch_bounded_primal_onchip(const PrimalParams& n, hipStream_t s);
// the batch: workgroup b solves P[b] (an array the device can read); lds = the largest entry's bounded_node_lds_bytes
hipError_t launch_bounded_primals_onchip(const PrimalParams* P, int B, size_t lds, hipStream_t s);
// the packed batch (lpx_packed.hip): workgroup i builds model i's tableau in LDS from the packed arrays, runs the same loop and
// extracts its results from LDS.  Every pointer is device memory; a stride is in doubles, 0 = one copy shared by every model.
struct PackedParams {
    const double *c, *A, *b, *lower, *upper;            // lower / upper: or null (0 / +inf)
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
    int32_t m, n, min, max_iter;
    double eps, ratio_tol;
    int32_t* status; double* x; double* value; lpx_primal_record* rec; int32_t* basis; uint8_t* at_upper;     // [count] ... as lpx_packed_results
    uint8_t* flip; int64_t flip_stride;                 // work bytes, [count][flip_stride], flip_stride >= n + m
};
// lpx_solve_packed behind its argument checks: the arena, the copies, the one launch, the one wait
int packed_solve(const lpx_packed_models* in, const lpx_run_opts* o, const lpx_packed_results* out, lpx_stats* st);
// the host side of a packed call, shared by lpx_packed.hip and lpx_packed_dual.hip: one arena on the device, one pinned block for
// the results, one stream, all under one mutex.  Never destroyed, as the handle cache: the HIP runtime may be gone by the time
// statics are torn down.
struct PackedArena {
    std::mutex mu;
    char* dev = nullptr; size_t dev_bytes = 0;
    char* pin = nullptr; size_t pin_bytes = 0;          // the results of a call come back in ONE copy and are handed out from here
    hipStream_t stream = nullptr;
    bool attr = false;                                  // the function attribute of lpx_packed_primal_onchip is set
    bool attr_dual = false;                             // ... of lpx_packed_dual_onchip
    bool attr_bnb = false;                              // ... of lpx_packed_bnb_onchip
    bool attr_bnb_dual = false;                         // ... of lpx_packed_bnb_dual_onchip
};
extern PackedArena g_packed;                            // defined in lpx_packed.hip
// the packed batch by a dual start (lpx_packed_dual.hip): PackedParams plus rel (int32 [m] per model; a stride in int32, 0 = shared;
// null = every row <=), the long-step switch and the duals
struct PackedDualParams {
    const double *c, *A, *b, *lower, *upper;
    const int32_t* rel;
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride, rel_stride;
    int32_t m, n, min, max_iter, long_step, pad;
    double eps, ratio_tol;
    int32_t* status; double* x; double* value; lpx_packed_dual_record* rec; int32_t* basis; uint8_t* at_upper;   // as lpx_packed_dual_results
    double* y; double* d;                               // [count][m], [count][n]
    uint8_t* flip; int64_t flip_stride;                 // work bytes, [count][flip_stride], flip_stride >= n + m
};
// lpx_solve_packed_dual behind its argument checks: the same arena, the copies, the one launch, the one wait
int packed_dual_solve(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* out, lpx_stats* st);
// right-hand-side scenarios warm-started from one solved base (lpx_packed_warm.hip).  The snapshot of a base: one device allocation
// the handle owns, every pointer into it.  tile is the solved tableau with the row stride S = C | 1 of the kernels' LDS image (a
// padding column holds 0.0); lower and rel are null where the model has none; flip holds bit 0 only.
struct PackedBaseSnap {
    double* tile; double* ub; double* b0; double* lower; double* constant;     // [R * S], [C], [m], [n], [1]: c.l, what the shift took out
    int32_t* basis; int32_t* rel; int32_t* shifted;                            // [m], [m], [1]
    uint8_t* flip;                                                             // [C - 1]
};
struct PackedBase {                                     // what an lpx_packed_base holds on the host
    int32_t m = 0, n = 0, min = 0;
    char* dev = nullptr; size_t dev_bytes = 0;
    PackedBaseSnap snap{};
};
// both kernels: the base reads c, A, upper and snap.b0 / lower / rel (uploaded there) and writes the rest of the snapshot; a
// scenario reads the snapshot and its own b ([count][m])
struct PackedWarmParams {
    const double *c, *A, *upper, *b;
    PackedBaseSnap snap;
    int32_t m, n, min, max_iter, long_step, pad;
    double eps, ratio_tol;
    int32_t* status; double* x; double* value; lpx_packed_dual_record* rec; int32_t* basis; uint8_t* at_upper;   // as lpx_packed_dual_results
    double* y; double* d;
    uint8_t* flip; int64_t flip_stride;                 // work bytes, [count][flip_stride], flip_stride >= n + m
};
// lpx_packed_base_open / _solve / _close behind their argument checks.  open: the base's status (0 = LPX_OPTIMAL: *base filled) or
// an error code; the caller frees a base it does not keep with packed_base_close
int packed_base_open(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* base_out, PackedBase* base);
int packed_base_solve(const PackedBase* base, int32_t count, const double* b, int flags, const lpx_run_opts* o,
                      const lpx_packed_dual_results* out, lpx_stats* st);
void packed_base_close(PackedBase* base);
// lpx_packed_base_solve_costs behind its argument checks (lpx_packed_cost.hip): c0 is the host copy of the base's costs ([n]) that
// the API-level handle keeps; b may be null (every scenario keeps b0); op and od are the primal and the dual loop's options
int packed_base_solve_costs(const PackedBase* base, const double* c0, int32_t count, const double* c, const double* b, int flags,
                            const lpx_run_opts* op, const lpx_run_opts* od, const lpx_packed_cost_results* out, lpx_stats* st);
// the packed batch of integer programs (lpx_packed_bnb.hip): PackedParams plus the shared integer mask ([n] bytes or null = every
// variable), the search flags, the three budgets, both ratio tolerances (the root's primal loop, a node's dual loop), the log and
// the work slices ([count][work_stride] bytes: what the search keeps outside LDS)
struct PackedBnbParams {
    const double *c, *A, *b, *lower, *upper;
    const uint8_t* mask;
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
    int32_t m, n, min, max_iter, flags, max_depth, log_cap, pad;        // max_depth: resolved, at least 1
    long long max_nodes, max_events;
    double eps, ratio_tol_root, ratio_tol_node;
    int32_t* status; double* x; double* value; lpx_packed_bnb_record* rec; lpx_bnb_node_log* log;   // as lpx_packed_bnb_results
    long long* pivots;                                  // [count] kind-0 and kind-1 pivots of the root and of every node, for lpx_stats
    char* work; int64_t work_stride;
};
// lpx_solve_packed_bnb behind its argument checks: the same arena, the copies, the one launch, the one wait
int packed_bnb_solve(const lpx_packed_bnb_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out, lpx_stats* st);
// the device bytes of the work slices of such a call (host arithmetic, for the 1 GiB rule)
size_t packed_bnb_work_bytes(int count, int m, int n, int max_depth);
// the packed batch of integer programs by a dual start (lpx_packed_bnb_dual.hip): PackedBnbParams plus rel as PackedDualParams has it;
// ratio_tol_root is that of the root's dual loop
struct PackedBnbDualParams {
    const double *c, *A, *b, *lower, *upper;
    const int32_t* rel;
    const uint8_t* mask;
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride, rel_stride;
    int32_t m, n, min, max_iter, flags, max_depth, log_cap, pad;        // max_depth: resolved, at least 1
    long long max_nodes, max_events;
    double eps, ratio_tol_root, ratio_tol_node;
    int32_t* status; double* x; double* value; lpx_packed_bnb_record* rec; lpx_bnb_node_log* log;   // as lpx_packed_bnb_results
    long long* pivots;                                  // [count] kind-0 and kind-1 pivots of the root and of every node, for lpx_stats
    char* work; int64_t work_stride;
};
// lpx_solve_packed_bnb_dual behind its argument checks: the same arena, the copies, the one launch, the one wait; its work slices
// are those of packed_bnb_work_bytes
int packed_bnb_dual_solve(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out, lpx_stats* st);

// ---- lpx_kernels.hip: the two-launch select and update paths
hipError_t launch_select(const SelParams& p, hipStream_t s);       // gather-based (dual path)
hipError_t launch_select_la(const SelParams& p, hipStream_t s);    // lookahead (primal / forced)
hipError_t launch_la_init(const SelParams& p, hipStream_t s);
// fac0/fac1: factor columns, chosen by pivot parity; nxt by-products go to the other one.
// e0/e1 non-null: bracket the dispatch with HIP events bound to the kernel (hipExtLaunchKernelGGL).
hipError_t launch_update(double* T, int ld, int R, int C, const int32_t* shape, const double* prow, double* fac0, double* fac1,
                         double* rhsbuf, const DevState* st, hipStream_t s,
                         hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the same for the tableau a parameter record describes (T, ld, capacity, shape, pivot row, RHS column, state record)
hipError_t launch_update(const SelParams& p, double* fac0, double* fac1, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// multi-workgroup protocol: select_mb (nblk workgroups) + update_mb (reduces the partials, commits `us`)
hipError_t launch_select_mb(const SelParams& p, hipStream_t s);
hipError_t launch_update_mb(const SelParams& p, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
int select_mb_blocks(int C);
hipError_t launch_group_iter(const SelParams* arr, int count, int dual, int max_nblk, int max_upd_blocks, hipStream_t s,
                             int maxR, int maxC);       // capacity of the largest node: sizes the dual select's LDS
hipError_t launch_group_init(const SelParams* arr, int count, hipStream_t s);
hipError_t launch_group_rhs_init(const SelParams* arr, int count, hipStream_t s);     // dual groups: contiguous RHS copy
hipError_t launch_rhs_init(const SelParams& p, hipStream_t s);
int update_blocks(int ld, int R);
int update_policy(int ld, int R);            // 0 = cache-resident update kernel, 1 = all-nt streaming, 2 = mixed-store streaming
hipError_t kernels_init();          // one-time function attributes

// ---- lpx_nodes.hip: branch-and-bound node assembly (K9)
struct BuildDesc { double* T; int32_t* basis; int32_t* shape; DevState* st; int ld, R, C, cut0; };
hipError_t launch_build_nodes(const double* T0, int ld0, int R0, int C0, const BuildDesc* descs, int count, int maxld, int maxR,
                              const int32_t* cvar, const double* ccoef, const double* czero, const double* crhs, hipStream_t s);
struct ChildDesc { const double* Tp; const int32_t* basis_p; double* T; int32_t* basis; int32_t* shape; DevState* st;
                   int ldp, Rp, Cp, ld, var, ik, is_ge, pad; double bound; };
hipError_t launch_build_children(const ChildDesc* descs, int count, int maxld, int maxR, hipStream_t s);
struct ParkDesc { const double* srcT; double* dstT; const int32_t* srcB; int32_t* dstB; size_t doubles; int m, pad; };
hipError_t launch_park_many(const ParkDesc* descs, int count, int blocks_per_node, hipStream_t s);
struct GatherDesc { const double* T; const int32_t* basis; int ld, R, C, off; };
hipError_t launch_gather_solution(const GatherDesc* descs, int count, double* out_rhs, int32_t* out_basis, hipStream_t s);
hipError_t launch_build_child(const double* Tp, int ldp, int Rp, int Cp, const int32_t* basis_p, double* T, int ld,
                              int var, int ik, int is_ge, double bound, int32_t* basis, hipStream_t s);
hipError_t launch_build_node(const double* T0, int ld0, int R0, int C0, double* T, int ld, int R, int C,
                             const int32_t* cvar, const double* ccoef, const double* czero, const double* crhs,
                             int32_t* basis, hipStream_t s);
hipError_t launch_states_scatter(const SelParams* arr, const DevState* src_pinned, int count, hipStream_t s);
hipError_t launch_states_gather(const SelParams* arr, DevState* dst_pinned, int count, hipStream_t s);

// ---- lpx_pivot_fused.hip: the one-launch primal pivot (K4f) and its deferred pivots
// Fused pivot (primal loop without a per-pivot callback, lpx_pivot_fused / _c): ONE launch applies pivot k
// out of place (buffer b -> buffer 1 - b) and, in its first `nblk` workgroups, selects pivot k + 1 from the tableau it reads.
// P.T / P.prow / P.rhsbuf are the buffers of index 0, the members below those of index 1; P.col0 / P.col1 the factor columns.
struct FusedParams {
    SelParams P;
    double* T1; double* prow1; double* rhs1;
    DevState* rec;       // two state records: a launch reads rec[par] and writes rec[1 - par]; pad[2] = launch count, pad[3] = tableau buffer
    int par;             // set per launch by launch_pivot_fused
    // deferred pivots of the single-tableau run (run_fused; the group step leaves them alone): ring slots of 2 * defer pending
    // pivots -- normalised pivot row [ld], factor column [R capacity], pivot row index -- and the launch's slot
    double* pring; double* fring; int32_t* rring;
    int defer;           // pivots per sweep (LPX_PIVOT_DEFER)
    int lm;              // set per launch by launch_pivot_fused: launch number mod 2 * defer
    // compact form of run_fused: P.T / T1 hold only the nonbasic columns and the RHS (slots), P.ld / P.C / P.shape
    // describe that layout, and `ld_full` is the handle's own leading dimension (the launcher's policy choices follow the handle)
    int compact, ld_full;
    int32_t* slotvar;    // [compact ld] variable of every slot; the RHS slot holds the RHS column's index
    int32_t* pslot;      // [128] slot of every partial argmin (the partials themselves carry the variable: ties break by variable)
    int32_t* qring;      // [2 * defer] entering slot of every ring slot's pivot
    int32_t* caux;       // {slot, ring slot} of a column zeroed for a pivot that was not taken (UNBOUNDED), or -1
};
// the compact form's entry and exit passes (lpx_pivot_fused.hip)
struct CompactIo {
    double* full; int ld, R, C;          // the handle's tableau: leading dimension, LIVE rows and columns
    double* comp; int cld;               // the compact buffer and its leading dimension; C - R + 1 live slots
    const int32_t* basis;                // [R - 1]
    int32_t* vmap;                       // [C] scratch: slot of a nonbasic variable, -2 - row of a basic one
    int32_t* slotvar; int32_t* flag;     // flag: set when a basic column is not a unit vector bit for bit, or the basis is not one
};
hipError_t launch_compact_entry(const CompactIo& io, int32_t* cshape, int32_t* caux, hipStream_t s);
// applies the n pending pivots of the compact buffer `src` and writes the full layout (basic columns as unit vectors)
hipError_t launch_compact_exit(const FusedParams& f, const CompactIo& io, const double* src, int n, int slot0, hipStream_t s);
int fused_policy(int ld, int R);             // 0 = default cache policy (lpx_pivot_fused_c), 2 = streaming mix, 1 = all nt
int pivot_defer_max();                       // deepest deferral the sweep kernels are built for
hipError_t launch_fused_init(const FusedParams& f, hipStream_t s);
// launch L of a run (0: the prologue's): a sweep applying f.defer pending pivots when L is a positive multiple of f.defer,
// else select-only -- one kernel, or two (column launch, row launch) where pivot_select_is_pair(ld, capacity rows).
// rat: the handle's ratio buffer (capacity rows + 1 doubles, then the column launch's scan records: pivot_ratio_bytes(capacity rows)
// in all), which only the pair uses
bool pivot_select_is_pair(int ld, int R);
bool pivot_compact_ok(int ld, int R, int d);   // depth d on this handle can run the compact form (the pair, a strip sweep built for d)
size_t pivot_ratio_bytes(int R);
size_t pivot_stream_bytes();                 // UPD_STREAM_BYTES: a handle above it cannot live in the Infinity Cache (deepest default deferral)
hipError_t launch_pivot_fused(const FusedParams& f, double* rat, long long L, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// the n pivots a finished run left pending (its last record: buffer, count, oldest slot), applied into buffer 0
hipError_t launch_pivot_flush(const FusedParams& f, int buf, int n, int slot0, hipStream_t s);
hipError_t pivot_fused_init();      // one-time function attribute of lpx_pivot_select (the row launch)

// ---- lpx_group_fused.hip: the fused group step (K4g), one launch per step for a whole group of node LPs
hipError_t launch_group_fused_init(const FusedParams* arr, const int* fresh, int nfresh, const DevState* init, hipStream_t s);
hipError_t launch_group_fused_gather(const FusedParams* arr, int count, DevState* out, int* cur, hipStream_t s);
int group_fused_blocks(int ld, int R);
// comp: the group's device-side compaction record (group_fused_comp_ints(cap) ints; the host writes count and list of parity 0 before
// the first launch of a window, the kernel keeps them current from launch to launch)
int group_fused_comp_ints(int cap);
int group_fused_comp_hdr();     // ints in front of the list of a parity region: {count, padding}
hipError_t launch_group_fused(const FusedParams* arr, const int* live, int nlive, int per_node, int lpar, size_t live_bytes, hipStream_t s,
                              int* comp, int cap, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// FP64 matrix-core GEMM (lpx_mfma.hip): C = I - A*B (mode 0, max |C_ij| -> *absmax as double bits) or C = D + A*B (mode 1)
hipError_t launch_dgemm_mfma(const double* A, int lda, const double* B, int ldb, double* C, int ldc, const double* D, int ldd,
                             int M, int N, int K, int mode, unsigned long long* absmax, hipStream_t s);
// blocked Gauss-Jordan inverse (lpx_invert_blocked.hip): n x n in place in A (leading dimension ld), result in X
struct IbWork {
    int n = 0, ld = 0, ncand = 0;
    double *A = nullptr, *X = nullptr, *L = nullptr, *Mr = nullptr, *prow = nullptr;
    void* cand = nullptr; int32_t *ipiv = nullptr, *perm = nullptr; int* status = nullptr;
    std::vector<hipEvent_t> events;
};
int ib_alloc(IbWork& w, int n);
void ib_free(IbWork& w);
int ib_run(IbWork& w, hipStream_t s, double* ms);     // ms: NULL or [2] = panel, update HIP-event ms
// resident group loop (lpx_resident_group.hip): one entry per node of a launch
struct ResNode {
    double* T; int ld, R, C;
    int32_t* basis; int32_t* trace; int trace_cap;
    DevState* st;
    DevState* st_host;       // pinned host mirror of the fields the launch changes (the host reads it instead of copying `st` back)
    unsigned long long* xr;  // [2][mcap][2][2]  (a, rhs) granule pairs per row
    unsigned long long* xp;  // [2][ld+8][2]     pivot row granules, then the header {q}
    unsigned* xgen;
    int mcap, dual;
    double eps, tol_fdf, tol_dual, tol_primal;
    int max_iter, fdf_guard, cleanup;
};
size_t resident_group_lds(int R, int C, int ld, int grid);
hipError_t resident_group_init();
// register-resident variant (lpx_resident_regs.hip): node rows in VGPRs, more nodes per launch
hipError_t resident_regs_init();
int resident_regs_shape(int maxC, int min_ld, int mmax, int* rpw_max);   // 0 = does not fit; else the kernel configuration (1, 2, 3)
size_t resident_regs_lds(int R, int C, int rt, int cfg);
size_t resident_regs_lds_budget();                  // dynamic LDS a workgroup of the register-resident kernel may ask for
hipError_t launch_resnode_states_scatter(const void* nodes_dev, const DevState* src_pinned, int count, hipStream_t s);
hipError_t launch_resident_regs(const void* nodes_dev, int nodes, int grid, int cfg, int rt, size_t lds, int chunk, hipStream_t s);
hipError_t launch_resident_group(const void* nodes_dev, int nodes, int grid, size_t lds, int chunk, hipStream_t s);
// resident primal loop (lpx_resident.hip)
hipError_t resident_init();
int resident_plan(int R, int C, int ld, int* grid, int* rpw, size_t* lds);      // 0 = does not fit on chip
hipError_t launch_resident_primal(double* T, int ld, int R, int C, int grid, int rpw, size_t lds, int mcap,
                                  int32_t* basis, int32_t* trace, int trace_cap, DevState* st,
                                  unsigned long long* xr, unsigned long long* xp, unsigned* xgen,
                                  double eps, double tol, int max_iter, int chunk, hipStream_t s);

// resident primal loop with column-owning workgroups (lpx_resident_col.hip): one exchange per pivot
hipError_t resident_col_init();
int resident_col_plan(int R, int C, int* grid, int* cpw, size_t* lds);          // 0 = does not fit on chip
size_t resident_col_xc_bytes(int grid);
size_t resident_col_xq_bytes(int grid, int R);
hipError_t launch_resident_primal_col(double* T, int ld, int R, int C, int grid, int cpw, size_t lds,
                                      int32_t* basis, int32_t* trace, int trace_cap, DevState* st,
                                      unsigned long long* xc, unsigned long long* xq, unsigned* xgen,
                                      double eps, double tol, int max_iter, int chunk, hipStream_t s);

// What the ranging kernels (lpx_ranging.hip) need of a tableau handle: live shape, buffers, stream, and a workspace the
// handle owns (grown on demand, freed with the handle).
struct TableauView {
    const double* T; int ld, R, C;
    const int32_t* basis;
    hipStream_t stream;
    char** ws; size_t* ws_bytes;
};
void tableau_view(lpx_tableau* t, TableauView* v);

// What the cut round (lpx_cuts.hip) needs beyond that: the capacity, the writable basis and loop state, and the second tableau
// buffer of the fused primal loop (allocated on first use when need_second; T2 = nullptr when it does not fit the device).
struct CutView {
    double* T; double* T2; int ld, R, C, Rcap, Ccap;
    int32_t* basis; DevState* st;
    hipStream_t stream;
    char** ws; size_t* ws_bytes;
};
void tableau_cut_view(lpx_tableau* t, CutView* v, bool need_second);
int check_cut_opts(const lpx_cut_opts* o, const char* what);   // LPX_EINVAL (message set) when o is outside its ranges
int check_cut_opts(const lpx_cut_opts* o, const char* what, int kmin);     // ... with cuts_per_round in kmin..64 (the call above: 1)
// The cut round behind lpx_tableau_gmi_round and lpx_tableau_gmi_round_bounded (lpx_cuts.hip).  gmi_round_args: every argument
// check of include/lpx.h, no device touched.  gmi_round_run: the round; cb == nullptr is the plain round, else the bounded one on
// the handle's bound arrays (all null: a handle without bounds) and its contiguous RHS copy.
struct CutBounds { double* ub; double* lo; uint8_t* flip; double* rhsbuf; };
int gmi_round_args(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o, int kmin, const char* what);
int gmi_round_run(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o, int* n_added,
                  int32_t* src_rows, int* n_purged, int32_t* purged_cols, const CutBounds* cb, const char* what);

void set_error(const std::string& msg);
// Device memory the library keeps for reuse after its owner is gone (the chunk cache of destroyed parent stores, lpx_tableau_nodes.cpp):
// trim_device_caches() gives all of it back; malloc_retry() is hipMalloc that does so and tries once more before it reports
// hipErrorOutOfMemory -- every large allocation of the library goes through it.
void trim_device_caches();
hipError_t malloc_retry(void** p, size_t bytes);
int ensure_device();                // binds a device and sets kernel attributes once
double now_ms();
// hipStreamCreate costs 4-9 ms on this stack (an HSA queue each) while the hardware runs a handful of queues anyway:
// handles borrow one of a few process-wide streams (round robin) and never destroy them.
hipStream_t borrow_stream();

// Generic device-resident loop: enqueue `batch` iterations (eager, hipGraph replay, or event-
// bracketed), poll the device state once per batch, fire pivot callbacks from the trace.
struct LoopCtx {
    hipStream_t stream = nullptr;
    DevState* st = nullptr;            // device
    DevState* hst = nullptr;           // pinned host mirror
    int32_t* trace = nullptr; int trace_cap = 0;
    std::vector<hipEvent_t>* events = nullptr;
    hipGraphExec_t* gexec = nullptr;   // cached graph of *g_batch iterations keyed by *g_key
    int* g_batch = nullptr;
    std::string* g_key = nullptr;
    std::string key;                   // identifies the captured parameter set
    std::function<int(hipStream_t, hipEvent_t, hipEvent_t)> enqueue_iter;  // one iteration
    std::function<int(hipStream_t)> prologue;                               // once, before the loop
    int launches_per_iter = 2;
    bool profile_maps = true;          // pivot k of a batch == k-th enqueued iteration
    std::function<bool(long long)> sweep_launch;   // profile: k-th launch of the loop proper streams the tableau (empty: every one)
    int start_iter = 0;                // pivots already done on this tableau by another path (resident loop hand-over)
};
// graph executables parked for `owner` (the address of a handle's gexec slot): destroyed with the handle, or when its buffers change
void graph_cache_drop_owner(const void* owner);
int run_device_loop(LoopCtx& c, const DevState& init, const lpx_run_opts* o, long long budget,
                    lpx_pivot_cb cb, void* user, lpx_stats* stats);

// Resumable form of the same loop: begin(); { submit(); complete(); } until done(); finish().
// submit() only enqueues (one batch + an async copy of the state to pinned memory), so several
// runs on different streams overlap on the device (lpx_multi_run).
class LoopRun {
public:
    LoopRun() = default;
    LoopRun(const LoopRun&) = delete;
    LoopRun& operator=(const LoopRun&) = delete;
    int begin(const LoopCtx& c, const DevState& init, const lpx_run_opts* o, long long budget,
              lpx_pivot_cb cb, void* user);
    int submit();
    int complete();
    bool done() const { return status_ != LPX_RUNNING || enq_ >= budget_; }
    bool may_submit() const { return enq_ < budget_; }
    int in_flight() const { return head_ - tail_; }
    int finish(lpx_stats* stats);          // returns the final status (or an error)
    ~LoopRun();
private:
    // up to two batches in flight: each submit() copies the state into its own pinned slot and records its own event, so
    // complete() waits for the OLDEST batch only while the next one is already queued behind it (run_device_loop)
    DevState* stage_ = nullptr; hipEvent_t ev_[2] = {nullptr, nullptr}; int head_ = 0, tail_ = 0;
    LoopCtx c_; lpx_run_opts o_{}; long long budget_ = 0, enq_ = 0;
    lpx_pivot_cb cb_ = nullptr; void* user_ = nullptr;
    lpx_stats local_{}; int batch_ = 64; bool graph_ = false;
    int fired_ = 0, iter_before_ = 0, status_ = LPX_RUNNING, init_phase_ = 2;
    long long batch_first_ = 0;     // loop-proper index of the first launch of the batch in flight (profile mode)
    double t0_ = 0;
};

}  // namespace lpx

#define LPX_HIP_TRY(expr)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            lpx::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));             \
            return LPX_EDEVICE;                                                            \
        }                                                                                  \
    } while (0)
