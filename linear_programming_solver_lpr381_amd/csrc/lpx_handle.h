// lpx_handle.h -- the tableau handle and the host helpers its translation units share (lpx_tableau.cpp, lpx_tableau_resident.cpp,
// lpx_tableau_groups.cpp, lpx_tableau_bounded.cpp, lpx_node_batch.cpp, lpx_tableau_nodes.cpp).  Host .cpp files of this directory only: kernels and launchers see lpx_internal.h, never the struct.
#pragma once
#include "lpx_internal.h"

#include <cstring>

struct lpx_tableau {
    int R = 0, C = 0, ld = 0;   // live shape (<= capacity) and leading dimension (from the capacity)
    int Rcap = 0, Ccap = 0;
    char* slab = nullptr;       // device slab holding every small buffer below (all but T)
    char* hslab = nullptr;      // pinned slab holding hst and shape_h
    int32_t* shape = nullptr;   // device record {R, C} read by the kernels
    int32_t* shape_h = nullptr; // pinned staging
    double* T = nullptr;        // [R*ld]
    double* snapT = nullptr;    // snapshot
    double* prow = nullptr;     // [ld]
    double* pcol = nullptr;     // [R]
    double* col0 = nullptr;     // [R] lookahead column buffers (ping-pong)
    double* col1 = nullptr;
    double* rhsbuf = nullptr;   // [R]
    double* ws = nullptr;       // [MB_MAXB * max(R,C)]
    double* part_v = nullptr; int32_t* part_i = nullptr;   // [64] partial argmins of the multi-workgroup select
    lpx::DevState* us = nullptr;    // state record written by the update kernel (multi-workgroup protocol)
    int32_t* basis = nullptr;   // [R-1]
    int32_t* snapBasis = nullptr;
    int32_t* trace = nullptr;   // [2*trace_cap]
    int trace_cap = 0;
    lpx::DevState* st = nullptr;    // device
    lpx::DevState* hst = nullptr;   // pinned host mirror
    bool suspended = false;     // lpx_multi_run_some left this run unfinished: *hst is where it continues
    bool trace_void = false;    // a clone before its first run: the state record is the source's, the trace was not copied and reads empty
    int32_t* frows = nullptr; int32_t* fcols = nullptr; int32_t* fchosen = nullptr; int fcap = 0;
    char* cutbuf = nullptr; char* cutbuf_h = nullptr; int cutcap = 0;   // staging of branching-row descriptors
    hipStream_t stream = nullptr;
    // cached graph of `g_batch` (select, update) pairs
    hipGraphExec_t gexec = nullptr;
    int g_batch = 0;
    std::string g_key;
    std::vector<hipEvent_t> events;
    // resident primal loop: exchange buffers (tagged granules) and the generation counter
    unsigned long long* xr = nullptr; unsigned long long* xp = nullptr; unsigned* xgen = nullptr;
    int32_t* xbasis = nullptr;      // basis as it was when the current resident launch started
    double* xT = nullptr;           // tableau as it was when the current resident launch started (put back if the launch aborts)
    unsigned long long* xc = nullptr; unsigned long long* xq = nullptr;   // column-owning resident kernel: candidates / candidate columns
    size_t xc_bytes = 0, xq_bytes = 0;
    bool resident_off = false;      // a resident launch could not get its workgroups co-resident: stay on the streaming path
    // fused pivot (lpx_pivot_fused): second tableau buffer and the index-1 copies of the small per-pivot vectors, on first use
    double* fT = nullptr; char* fslab = nullptr;
    double* fprow = nullptr; double* frhs = nullptr; lpx::DevState* frec = nullptr;
    double* frat = nullptr;         // [Rcap + 1] ratios of the select-only pair's column launch, then T[m,q], then its scan records (lpx_pivot_ratio; pivot_ratio_bytes)
    char* dring = nullptr; int dring_slots = 0;   // deferred pivots of run_fused: ring of pivot rows, factor columns, row indices
    char* cslab = nullptr;          // compact form of run_fused: its integer maps, on first use
    bool last_compact = false;      // the last run_fused took the compact form (lpx_tableau_last_run_compact)
    bool fused_off = false;         // the second buffer did not fit: stay on the two-launch path
    bool suspended2 = false;        // ... by the two-launch group kernels (it must continue there: no pending pivot, state in *hst)
    bool fsuspended = false; int frec_cur = 0;   // fused group run left unfinished: its records (latest: index frec_cur) are in place
    char* rgws = nullptr; size_t rgws_bytes = 0;  // lpx_tableau_ranging's partial slabs and outputs / the cut round's plan, on first use
    // Bounded-variable family (lpx_tableau_bounded.cpp): everything it keeps beside the tableau, on first use.
    struct __attribute__((visibility("hidden"))) Bounds {
        // bounded-variable loops (lpx_bounded.hip, lpx_bounded_dual.hip): upper bounds and flip states
        double* ub = nullptr; uint8_t* flip = nullptr;          // [Ccap] each
        bool bounds_set = false; int bounds_C = 0;              // live C the bounds were set for
        double* snapUb = nullptr; uint8_t* snapFlip = nullptr; bool snap_bounds = false; int snap_bounds_C = 0;
        int64_t bcounts[3] = {0, 0, 0};                         // events of the last bounded run: kind 0, kind 1, flips
        // lower shift of every column (lpx_tableau_change_bounds): internal column j stands for x_j - lo[j]; allocated with ub
        double* lo = nullptr; double* snapLo = nullptr;         // [Ccap] each
        bool lo_used = false, snap_lo_used = false;             // some change has stored a non-zero lo
        char* chg = nullptr; size_t chg_bytes = 0;              // staging of one bound edit: lower, upper, shift, saved (ub, lo), cols
        // branch and bound by bound changes (lpx_bnb_bounded.hip): the column list of lpx_tableau_dualize with its two counts
        // behind it, the device record of lpx_tableau_branch_pick, the integer mask, and the pinned slab the records come back through
        int32_t* dzl = nullptr; lpx_branch_pick* pickrec = nullptr; uint8_t* pickmask = nullptr; char* nodeslab = nullptr;
        // lpx_bounded_dual_run3: the objective cutoff the select kernel reads, and the host value its copy is made from
        double* cutoff = nullptr; double cutoff_h = 0.0;
        // the on-chip node (lpx_bounded_node3, lpx_bounded_node.hip): the pinned slab its inputs and its record travel through,
        // and the host copy of the integer mask now in pickmask (mask_n bytes; -1: pickmask holds something else)
        char* nodeio = nullptr; size_t nodeio_bytes = 0;
        std::vector<uint8_t> mask_h; int mask_n = -1;
        // the plunge (lpx_node_batch_plunge): whole[j] = 1 iff the host has seen column j's bounds and both are finite and integral
        // (lpx_tableau_set_bounds and every accepted bound edit keep it; empty: nothing known).  Host knowledge only, no device copy.
        std::vector<uint8_t> whole, snap_whole;
        // the probes (lpx_bounded_probe): the device workspace of the private basis / flip copies and the pinned slab of the
        // parameter record, the head and the records, each grown to twice the need
        char* probews = nullptr; size_t probews_bytes = 0;
        char* probeio = nullptr; size_t probeio_bytes = 0;

        void free()
        {
            hipFree(probews); if (probeio) hipHostFree(probeio);
            hipFree(ub); hipFree(flip); hipFree(snapUb); hipFree(snapFlip);
            hipFree(lo); hipFree(snapLo); hipFree(chg);
            hipFree(dzl); hipFree(pickrec); hipFree(pickmask); if (nodeslab) hipHostFree(nodeslab); hipFree(cutoff);
            if (nodeio) hipHostFree(nodeio);
        }
    } bnd;
};

#pragma GCC visibility push(hidden)       // private to liblpx.so
namespace lpx {

// The bounds and the flip states belong to the tableau they describe: lpx_tableau_snapshot / _restore take them along
// (enqueued on the handle's stream; the caller waits).
int bounds_snapshot(lpx_tableau* t);
int bounds_restore(lpx_tableau* t);
// lpx_tableau_clone's share: ub, lo, flip and the marks of src onto dst (same capacity), enqueued on dst's stream
int bounds_clone(const lpx_tableau* src, lpx_tableau* dst);

// The bounded family's checks (lpx_tableau_bounded.cpp), shared with the node batch (lpx_node_batch.cpp).
// The checks set LPX_EINVAL's message with `what` in front and touch no device.
int check_change_args(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const char* what);
int check_pick_args(lpx_tableau* t, int nint, double tol, const void* out, const char* what);
int check_long_flags(int flags, double cutoff, const char* what);
int check_node_opts(const lpx_tableau* t, const lpx_run_opts* o, const char* what);   // R >= 2, no resident form, eps
int check_node_fits(const lpx_tableau* t, const char* what);
int bounded_node_ready(const char* what);       // the one-time attribute of the on-chip node kernels
// what a finished on-chip node leaves on the host side of its handle, and the caller's record filled from the kernel's
void node_onchip_commit(lpx_tableau* t, const NodeOut* rec, bool any_lo, lpx_node_record* out);
// an accepted bound edit, for Bounds::whole: which of the edited columns now have finite integral bounds
void bounds_note_edit(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper);
int bounded_plunge_ready(const char* what);     // the one-time attribute of the plunge kernel
int bounded_guard_ready(const char* what);      // the one-time attribute of the guarded node kernel (lpx_bounded_guard.hip)
// reduced-cost tightening (lpx_bounded_fix.hip), shared by lpx_bounded_node5 and lpx_node_batch_run3
int bounded_fix_ready(const char* what);        // the one-time attribute of its kernel
int check_fix_args(double fix_bound, const lpx_fix_list* fix, int nint, const char* what);      // LPX_EINVAL with `what` in front, no device
size_t fix_list_bytes(int nint);                // the pinned arrays of one entry's list: upper, lower (double) and cols (int32), nint each
void fix_list_place(char* at, int nint, FixParams* p);             // ... and their places in p
// what the tightened columns of a finished node leave on the host side of its handle (as a bound edit with these triples would),
// and the caller's list filled from the kernel's
void fix_commit(lpx_tableau* t, int n, const FixParams& p, lpx_fix_list* fix);
// the probes (lpx_bounded_probe.hip), shared by lpx_bounded_probe and lpx_node_batch_run_probe
int bounded_probe_ready(const char* what);      // the one-time attribute of the probe kernel
int check_probe_args(int cand_max, int probe_iter, const char* what);      // LPX_EINVAL with `what` in front, no device
size_t probe_ws_bytes(const lpx_tableau* t, int cand_max);                 // the workspace of one entry: 2 * cand_max slices
// the parameter record of one entry on handle t as it will stand when the launch runs (lo_used: then); ws: its workspace
void probe_params(const lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, double prune, int nint, const uint8_t* mask_dev,
                  double tol, int cand_max, int probe_iter, bool lo_used, char* ws, const NodeOut* front, lpx_probe_head* head,
                  lpx_probe_record* rec, ProbeParams* p);
// the on-chip bounded primal loop (lpx_bounded_primal.hip), shared by lpx_bounded_run2 and lpx_node_batch_primal
int bounded_primal_ready(const char* what);     // the one-time attribute of its kernels
int bounded_primal_prepare(lpx_tableau* t);     // the device and the bound arrays the loop reads (without bounds: every ub = +inf)
void primal_params(lpx_tableau* t, const lpx_run_opts* o, lpx_primal_record* rec, PrimalParams* n);    // the parameter record of handle t
void primal_onchip_commit(lpx_tableau* t, const lpx_primal_record* rec);   // what a finished launch leaves on the host side of its handle

static constexpr int LPX_RESIDENT_RETRY = -1000;     // internal: first resident launch timed out, state untouched

void drop_graph(lpx_tableau* t);
// Fused pivot: buffers on first use.  Returns false (and remembers it) when the second tableau does not fit the device.
bool fused_buffers(lpx_tableau* t);
SelParams base_params(lpx_tableau* t, const lpx_run_opts* o, int mode);

// The record every run starts from.
inline DevState fresh_state(bool dual)
{
    DevState init; std::memset(&init, 0, sizeof(init));
    init.status = LPX_RUNNING; init.r = -1; init.q = -1; init.qn = -1; init.phase = dual ? 0 : 2;
    return init;
}
// Continue where another path stopped: pivot count, phase and counters of `at` (a primal run has one phase).
inline void resume_from(DevState& init, const DevState& at, bool dual)
{
    init.iter = at.iter; init.phase = dual ? at.phase : 2;
    init.fdf_count = at.fdf_count; init.dual_iter = at.dual_iter; init.primal_count = at.primal_count;
}
// Iterations a run may need: each one pivots, changes phase or terminates.  Every loop adds the slack of its own poll lag.
inline long long pivot_budget(const lpx_run_opts* o, bool dual)
{
    return dual ? (long long)o->fdf_guard + 2LL * o->max_iter : (long long)o->max_iter;
}
// What a finished (or suspended) state record reports; keep_transfers: the one-shot entry points keep their transfer times in s.
inline void stats_from_state(lpx_stats& s, const DevState& d, bool dual, double loop_ms, long long launches, bool keep_transfers)
{
    const double h2d = s.h2d_ms, d2h = s.d2h_ms;
    std::memset(&s, 0, sizeof(s));
    if (keep_transfers) { s.h2d_ms = h2d; s.d2h_ms = d2h; }
    s.pivots = d.iter; s.fdf_pivots = d.fdf_count;
    s.cleanup_pivots = dual ? d.primal_count : 0;
    s.loop_ms = loop_ms; s.launches = launches;
}

// The loop context every tableau loop shares: the handle's stream, records and graph cache, two launches per iteration, a
// fresh state record.  What differs comes in: the bytes that key the captured graph (the loop's parameter record) and the
// per-iteration enqueue; prologue and profile mapping follow p.mode.
template <typename Params, typename Enqueue>
void make_ctx(lpx_tableau* t, const SelParams& p, const Params& key, Enqueue enqueue, LoopCtx& c, DevState& init)
{
    const bool lookahead = p.mode != MODE_DUAL && p.mode != MODE_BOUNDED;
    c.stream = t->stream; c.st = t->st; c.hst = t->hst; c.trace = t->trace; c.trace_cap = t->trace_cap;
    t->trace_void = false;
    c.events = &t->events; c.gexec = &t->gexec; c.g_batch = &t->g_batch; c.g_key = &t->g_key;
    c.key.assign(reinterpret_cast<const char*>(&key), sizeof(key));
    c.enqueue_iter = enqueue;
    if (lookahead)                                       // lookahead path: first entering column + its gather, once
        c.prologue = [p](hipStream_t s) -> int { LPX_HIP_TRY(launch_la_init(p, s)); return 0; };
    else                                                 // dual and bounded paths: contiguous copy of the RHS column, once
        c.prologue = [p](hipStream_t s) -> int { LPX_HIP_TRY(launch_rhs_init(p, s)); return 0; };
    c.launches_per_iter = 2;
    // one profiled update launch = one pivot: not in dual mode (phase hops make the mapping ambiguous) nor in the bounded loop
    // (a launch may hold several events, or none that updates)
    c.profile_maps = lookahead;
    init = fresh_state(p.mode == MODE_DUAL);
}
void make_ctx(lpx_tableau* t, const SelParams& p, LoopCtx& c, DevState& init);      // the (select, update) pair of p.mode
int run_loop(lpx_tableau* t, SelParams p, const lpx_run_opts* o, long long budget,
             lpx_pivot_cb cb, void* user, lpx_stats* stats, int start_iter = 0);
// One LP handed to its streaming loop at the pivot another path had reached (`at`: the record that path left).
int continue_streaming(lpx_tableau* t, const lpx_run_opts* o, bool dual, const DevState& at, lpx_pivot_cb cb, void* user, lpx_stats* st);

// Resident runs (lpx_tableau_resident.cpp).  run_resident: the primal loop of one LP with the tableau in LDS; grid / rpw / lds from
// resident_plan or, col, resident_col_plan.  LPX_RESIDENT_RETRY: the launch was lost, the tableau is the one of its start and the
// streaming kernels continue at pivot *resume_iter.
int run_resident(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* stats,
                 int grid, int rpw, size_t lds, int* resume_iter, bool col = false);
// How a group goes onto the chip: workgroups per node, nodes at a time, LDS per workgroup; nt == 0: rows in LDS
// (lpx_resident_group), else the configuration of the register-resident kernel (lpx_resident_group_r) and the rows a workgroup
// may hold.  slots == 0: the group does not fit.
struct ResGroupPlan { int grid = 0, slots = 0; size_t lds = 0; int nt = 0, rt = 0; };
ResGroupPlan resident_group_plan(lpx_tableau** ts, int count);
// LPX_RESIDENT_RETRY: a launch was lost; statuses mark the unfinished nodes LPX_RUNNING and resume[i] is where node i stands.
int run_resident_group(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                       int* statuses, lpx_stats* stats, const ResGroupPlan& plan, lpx_pivot_cb cb, void* user,
                       DevState* resume = nullptr);
// Fused group run (lpx_tableau_groups.cpp): one launch per step for the whole group.  LPX_RESIDENT_RETRY: the group cannot take
// this path (nothing has been touched then).
int multi_run_fused(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                    int* statuses, lpx_stats* stats, const DevState* inits, int min_active);

}  // namespace lpx
#pragma GCC visibility pop
