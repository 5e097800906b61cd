// lpx_tableau_resident.cpp -- host side of the resident kernels: the exchange buffers, the primal loop of one LP with its tableau in
// LDS (run_resident; lpx_resident.hip, lpx_resident_col.hip), the planner that puts a group of node LPs onto the chip and the
// group loop (run_resident_group; lpx_resident_group.hip, lpx_resident_regs.hip).  Callers: lpx_primal_run / lpx_dual_run
// (lpx_tableau.cpp) and lpx_multi_run (lpx_tableau_groups.cpp).
#include "lpx_handle.h"

#include <cstdlib>
#include <cstring>
#include <vector>

using namespace lpx;

namespace {

// Exchange buffers of the resident kernels (sized for both of them) and the basis snapshot, allocated on first use.
static size_t xr_bytes(const lpx_tableau* t) { return sizeof(unsigned long long) * 8 * (size_t)t->Rcap; }
static size_t xp_bytes(const lpx_tableau* t) { return sizeof(unsigned long long) * (4 * ((size_t)t->ld + 8) + 64); }   // + diagnostic stamps
static int resident_buffers(lpx_tableau* t)
{
    if (t->xr) return 0;
    LPX_HIP_TRY(hipMalloc((void**)&t->xr, xr_bytes(t)));
    LPX_HIP_TRY(hipMalloc((void**)&t->xp, xp_bytes(t)));
    LPX_HIP_TRY(hipMalloc((void**)&t->xgen, sizeof(unsigned)));
    LPX_HIP_TRY(hipMalloc((void**)&t->xbasis, sizeof(int32_t) * (size_t)t->Rcap));
    LPX_HIP_TRY(malloc_retry((void**)&t->xT, sizeof(double) * (size_t)t->Rcap * t->ld));
    LPX_HIP_TRY(hipMemsetAsync(t->xr, 0, xr_bytes(t), t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->xp, 0, xp_bytes(t), t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->xgen, 0, sizeof(unsigned), t->stream));
    return 0;
}
// exchange buffers of the column-owning kernel, sized for the handle's capacity and every grid up to the CU count
static int resident_col_buffers(lpx_tableau* t, int grid)
{
    const size_t xcb = resident_col_xc_bytes(grid > 256 ? grid : 256), xqb = resident_col_xq_bytes(grid > 256 ? grid : 256, t->Rcap);
    if (t->xc && t->xc_bytes >= xcb && t->xq_bytes >= xqb) return 0;
    hipFree(t->xc); hipFree(t->xq); t->xc = nullptr; t->xq = nullptr;
    LPX_HIP_TRY(hipMalloc((void**)&t->xc, xcb));
    LPX_HIP_TRY(hipMalloc((void**)&t->xq, xqb));
    t->xc_bytes = xcb; t->xq_bytes = xqb;
    LPX_HIP_TRY(hipMemsetAsync(t->xc, 0, xcb, t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->xq, 0, xqb, t->stream));
    return 0;
}
static void resident_buffers_clear(lpx_tableau* t)
{
    if (t->xc) { hipMemsetAsync(t->xc, 0, t->xc_bytes, t->stream); hipMemsetAsync(t->xq, 0, t->xq_bytes, t->stream); }
    hipMemsetAsync(t->xr, 0, xr_bytes(t), t->stream);
    hipMemsetAsync(t->xp, 0, xp_bytes(t), t->stream);
    hipStreamSynchronize(t->stream);
}

// Tableau and basis as they were when the current resident launch started: put back after an aborted launch (late workgroups may
// have stored rows of a pivot the others never made).
int restore_launch_start(lpx_tableau* t)
{
    LPX_HIP_TRY(hipMemcpy(t->T, t->xT, sizeof(double) * (size_t)t->R * t->ld, hipMemcpyDeviceToDevice));
    LPX_HIP_TRY(hipMemcpy(t->basis, t->xbasis, sizeof(int32_t) * (size_t)(t->R - 1), hipMemcpyDeviceToDevice));
    return 0;
}

// The pivot callbacks of pivots from + 1 .. to, read from the trace between two launches.
int fire_trace_callbacks(lpx_tableau* t, int from, int to, lpx_pivot_cb cb, void* user)
{
    const int lo = from, hi = to < t->trace_cap ? to : t->trace_cap;
    if (!cb || hi <= lo) return 0;
    std::vector<int32_t> tr(2 * (size_t)(hi - lo));
    LPX_HIP_TRY(hipMemcpy(tr.data(), t->trace + 2 * lo, sizeof(int32_t) * 2 * (hi - lo), hipMemcpyDeviceToHost));
    for (int k = lo; k < hi; ++k) cb(user, k + 1, tr[2 * (k - lo)], tr[2 * (k - lo) + 1]);
    return 0;
}

}  // namespace

// Resident primal loop: one launch runs up to `chunk` pivots with the tableau in LDS; the host only polls the
// 64-byte state record between launches (and fires the pivot callbacks from the trace).
// col: the column-owning kernel (lpx_resident_col.hip; grid / cpw / lds from resident_col_plan), else the row-owning one
int lpx::run_resident(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* stats,
                      int grid, int rpw, size_t lds, int* resume_iter, bool col)
{
    const int mcap = t->Rcap;
    { int rc = resident_buffers(t); if (rc) return rc; }
    if (col) { int rc = resident_col_buffers(t, grid); if (rc) return rc; }
    *t->hst = fresh_state(false);
    t->trace_void = false;
    LPX_HIP_TRY(hipMemcpyAsync(t->st, t->hst, sizeof(DevState), hipMemcpyHostToDevice, t->stream));
    const int chunk = cb ? (o->batch > 0 ? o->batch : 256) : (1 << 30);
    lpx_stats local; std::memset(&local, 0, sizeof(local));
    const double t0 = now_ms();
    int fired = 0, status = LPX_RUNNING;
    for (long long launches = 0; status == LPX_RUNNING; ++launches) {
        if (launches > (long long)o->max_iter + 4) { set_error("resident loop: launch budget exhausted while still running"); return LPX_ITER_LIMIT; }
        // Tableau and basis as of the start of this launch.  A launch that cannot finish normally writes nothing back, but
        // a workgroup that was scheduled late (after the others gave up) may complete a short launch and store its rows:
        // whenever the abort flag is up the host puts this copy back, so the hand-over never sees a half-pivoted tableau.
        LPX_HIP_TRY(hipMemcpyAsync(t->xbasis, t->basis, sizeof(int32_t) * (size_t)(t->R - 1), hipMemcpyDeviceToDevice, t->stream));
        LPX_HIP_TRY(hipMemcpyAsync(t->xT, t->T, sizeof(double) * (size_t)t->R * t->ld, hipMemcpyDeviceToDevice, t->stream));
        if (o->profile) {
            while (t->events.size() < 2) { hipEvent_t e; LPX_HIP_TRY(hipEventCreate(&e)); t->events.push_back(e); }
            LPX_HIP_TRY(hipEventRecord(t->events[0], t->stream));
        }
        if (col)
            LPX_HIP_TRY(launch_resident_primal_col(t->T, t->ld, t->R, t->C, grid, rpw, lds, t->basis, t->trace, t->trace_cap,
                                                   t->st, t->xc, t->xq, t->xgen, o->eps, o->ratio_tol, o->max_iter, chunk, t->stream));
        else
        LPX_HIP_TRY(launch_resident_primal(t->T, t->ld, t->R, t->C, grid, rpw, lds, mcap, t->basis, t->trace, t->trace_cap,
                                           t->st, t->xr, t->xp, t->xgen, o->eps, o->ratio_tol, o->max_iter, chunk, t->stream));
        if (o->profile) LPX_HIP_TRY(hipEventRecord(t->events[1], t->stream));
        local.launches++;
        LPX_HIP_TRY(hipMemcpyAsync(t->hst, t->st, sizeof(DevState), hipMemcpyDeviceToHost, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        if (o->profile) {       // HIP events on the library stream around the persistent kernel: its duration
            float ms = 0.f;
            LPX_HIP_TRY(hipEventElapsedTime(&ms, t->events[0], t->events[1]));
            local.update_ms_sum += ms;
            local.update_launches++;
        }
        if (t->hst->pad[1]) {
            // a bounded wait expired: some workgroup was not resident or died; rows in HBM are those of the last
            // completed launch.  Clear the exchange buffers so that no stale generation can ever match.
            resident_buffers_clear(t);
            set_error("resident loop: an exchange wait expired (workgroups not co-resident?)");
            // Put the tableau and the basis of the launch's start back (late workgroups may have stored rows of a
            // pivot the others never made) and hand over to the streaming kernels, which continue from pivot
            // `resume_iter`.
            { int rc = restore_launch_start(t); if (rc) return rc; }
            t->resident_off = true;
            *resume_iter = fired;
            return LPX_RESIDENT_RETRY;
        }
        status = t->hst->status;
        const int done = t->hst->iter;
        { int rc = fire_trace_callbacks(t, fired, done, cb, user); if (rc) return rc; }
        fired = done;
    }
    local.loop_ms = now_ms() - t0;
    local.pivots = t->hst->iter;
    if (stats) { const double h2d = stats->h2d_ms, d2h = stats->d2h_ms; *stats = local; stats->h2d_ms = h2d; stats->d2h_ms = d2h; }
    return status;
}

// Resident group run: the nodes of a batch are solved a few at a time, each resident in the LDS of its own slice
// of the chip (lpx_resident_group.hip).  Launches are `chunk` pivots long; after each one finished nodes leave and
// waiting ones take their place, so the slices stay busy until the batch is done.
namespace {

struct ResGroupBuf { ResNode* d = nullptr; ResNode* h = nullptr; DevState* hs = nullptr; int cap = 0; hipStream_t stream = nullptr;
                     ParkDesc* pd_d = nullptr; ParkDesc* pd_h = nullptr; };   // pd: descriptors of the snapshot copies (one launch for a whole group)
ResGroupBuf g_resgroup;

// The register-resident variant (node rows in VGPRs): more nodes per launch when a node is wide enough to need many CUs' LDS.
// Returns the nodes per launch it would give (0 = not applicable) and fills grid / lds / nt.
int resident_regs_plan(lpx_tableau** ts, int count, int cus, int* grid, size_t* lds, int* nt, int* rt)
{
    static const bool enabled = [] { const char* e = std::getenv("LPX_RESIDENT_REGS"); return !(e && e[0] == '0'); }();
    if (!enabled) return 0;
    int maxC = 2, mmax = 1, mmin = 1 << 30, min_ld = 1 << 30;
    for (int i = 0; i < count; ++i) { maxC = std::max(maxC, ts[i]->C); mmax = std::max(mmax, ts[i]->R - 1); mmin = std::min(mmin, ts[i]->R - 1); min_ld = std::min(min_ld, ts[i]->ld); }
    int rpw_max = 0;
    const int n = resident_regs_shape(maxC, min_ld, mmax, &rpw_max); // the kernel configuration
    if (!n) return 0;
    int g = (mmax + rpw_max - 1) / rpw_max;                 // workgroups per node: every node's rows per workgroup <= rpw_max
    if (g > mmin || g > cus) return 0;
    { const int rpw = (mmax + g - 1) / g; g = (mmax + rpw - 1) / rpw; }          // no idle workgroups for the tallest node
    size_t need = 0;
    for (int i = 0; i < count; ++i) need = std::max(need, resident_regs_lds(ts[i]->R, ts[i]->C, rpw_max, n));
    if (need > resident_regs_lds_budget()) return 0;
    *grid = g; *lds = need; *nt = n; *rt = rpw_max;
    return cus / g;
}

// The register form for this group, when it applies and puts more nodes on the chip at once than the `lds_slots` the LDS form
// holds (and there are enough nodes to use them); lds_slots = 0: nothing fits the LDS form, the register form alone.
void take_regs_form(lpx_tableau** ts, int count, int cus, int max_slots, int lds_slots, ResGroupPlan* plan)
{
    int rg = 0, rnt = 0, rrt = 0; size_t rlds = 0;
    const int rslots = resident_regs_plan(ts, count, cus, &rg, &rlds, &rnt, &rrt);
    static const bool force_regs = [] { const char* e = std::getenv("LPX_RESIDENT_REGS"); return e && e[0] == '2'; }();   // diagnostic: whenever it applies
    if (rslots < 1 || !(force_regs || (rslots > lds_slots && count > lds_slots))) return;
    plan->grid = rg; plan->slots = std::min(rslots, std::min(count, max_slots)); plan->lds = rlds; plan->nt = rnt; plan->rt = rrt;
}

}  // namespace

ResGroupPlan lpx::resident_group_plan(lpx_tableau** ts, int count)
{
    ResGroupPlan plan;
    hipDeviceProp_t prop; int dev = 0;
    static int cus = 0;
    if (!cus) { if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return plan; cus = prop.multiProcessorCount; }
    const size_t lds_max = 160 * 1024 - 1024;
    // As many nodes per launch as fit: a node takes cus / n workgroups, down to ONE (small node LPs: 240 of them side by side,
    // each in the LDS of one CU).  r01 / early r02 stopped at 8 nodes per launch; a 60-variable 0/1 program went from 7.2 k to
    // 21 k nodes/s when the limit fell (tools/probe_slots.py), node logs and pivot counts unchanged.  LPX_GROUP_SLOTS caps it.
    static const int max_slots = [] { const char* e = std::getenv("LPX_GROUP_SLOTS"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 1 << 20; }();
    // (never more nodes than CUs: a node needs at least one workgroup -- a group of more than 256 nodes divided by zero here before r03)
    int mmin = 1 << 30, mmax = 1;
    for (int i = 0; i < count; ++i) { mmin = std::min(mmin, ts[i]->R - 1); mmax = std::max(mmax, ts[i]->R - 1); }
    for (int n = std::min(std::min(count, max_slots), cus); n >= 1; --n) {
        int g = std::min(cus / n, mmin);              // at most one workgroup per row of the smallest node
        if (g < 1) continue;
        { const int rpw = (mmax + g - 1) / g; g = (mmax + rpw - 1) / rpw; }   // no idle workgroups: the fewest that keep the same rows-per-workgroup for the tallest node
        size_t need = 0;
        for (int i = 0; i < count; ++i) need = std::max(need, resident_group_lds(ts[i]->R, ts[i]->C, ts[i]->ld, g));
        if (need <= lds_max) {
            plan.grid = g; plan.slots = n; plan.lds = need;
            take_regs_form(ts, count, cus, max_slots, n, &plan);
            return plan;
        }
    }
    take_regs_form(ts, count, cus, max_slots, 0, &plan);
    return plan;
}

int lpx::run_resident_group(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                            int* statuses, lpx_stats* stats, const ResGroupPlan& plan, lpx_pivot_cb cb, void* user, DevState* resume)
{
    ResGroupBuf& g = g_resgroup;
    const int grid = plan.grid, slots = plan.slots; const size_t lds = plan.lds;
    if (!g.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    if (g.cap < count) {
        hipFree(g.d); if (g.h) hipHostFree(g.h); if (g.hs) hipHostFree(g.hs);
        hipFree(g.pd_d); if (g.pd_h) hipHostFree(g.pd_h);
        g.d = nullptr; g.h = nullptr; g.hs = nullptr; g.pd_d = nullptr; g.pd_h = nullptr; g.cap = 0;
        const int c = count + 16;
        LPX_HIP_TRY(hipMalloc((void**)&g.d, sizeof(ResNode) * c));
        LPX_HIP_TRY(hipHostMalloc((void**)&g.h, sizeof(ResNode) * c));
        LPX_HIP_TRY(hipHostMalloc((void**)&g.hs, sizeof(DevState) * c));
        LPX_HIP_TRY(hipMalloc((void**)&g.pd_d, sizeof(ParkDesc) * c));
        LPX_HIP_TRY(hipHostMalloc((void**)&g.pd_h, sizeof(ParkDesc) * c));
        g.cap = c;
    }
    const double t0 = now_ms();
    std::vector<ResNode> node(count);
    // Per-node host work adds up when a group is a whole B&B level (8000 warm-started nodes: 0.24 s of stream waits, state uploads and
    // snapshot copies in front of 0.3 s of kernel): every distinct stream is waited for once, the state records go up in one launch,
    // the snapshots of a launch are one multi-copy launch.
    std::vector<hipStream_t> waited;
    auto wait_once = [&](hipStream_t st) -> int {
        for (hipStream_t w : waited) if (w == st) return 0;
        LPX_HIP_TRY(hipStreamSynchronize(st));
        waited.push_back(st);
        return 0;
    };
    for (int i = 0; i < count; ++i) {
        lpx_tableau* t = ts[i];
        { int rc = wait_once(t->stream); if (rc) return rc; }          // node assembly ran on the node's own stream
        t->trace_void = false;
        if (!t->xr) {
            { int rc = resident_buffers(t); if (rc) return rc; }
            LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        }
        const lpx_run_opts* o = dual[i] ? dopts : popts;
        ResNode& n = node[i];
        n.T = t->T; n.ld = t->ld; n.R = t->R; n.C = t->C; n.basis = t->basis; n.trace = t->trace; n.trace_cap = t->trace_cap;
        n.st = t->st; n.xr = t->xr; n.xp = t->xp; n.xgen = t->xgen; n.mcap = t->Rcap; n.dual = dual[i] ? 1 : 0;
        n.eps = o->eps; n.tol_fdf = o->ratio_tol; n.tol_dual = o->ratio_tol; n.tol_primal = dual[i] ? o->eps : o->ratio_tol;
        n.max_iter = o->max_iter; n.fdf_guard = o->fdf_guard; n.cleanup = o->cleanup;
        g.hs[i] = fresh_state(dual[i]);
        n.st_host = &g.hs[i];
    }
    // every node's initial state record: one launch reading the pinned array (node i <-> g.hs[i])
    std::memcpy(g.h, node.data(), sizeof(ResNode) * (size_t)count);
    LPX_HIP_TRY(hipMemcpyAsync(g.d, g.h, sizeof(ResNode) * (size_t)count, hipMemcpyHostToDevice, g.stream));
    LPX_HIP_TRY(launch_resnode_states_scatter(g.d, g.hs, count, g.stream));
    LPX_HIP_TRY(hipStreamSynchronize(g.stream));                        // g.h / g.d are rewritten per launch below
    // launch length: long enough to hide the launch + reload (~30 us), short enough that a node finishing inside a
    // launch does not leave its slice idle for long
    const lpx_run_opts* o0 = dual[0] ? dopts : popts;
    static const int chunk_env = [] { const char* e = std::getenv("LPX_GROUP_CHUNK"); return e ? std::atoi(e) : 0; }();   // diagnostic
    // A group larger than the chip holds at a time goes out as ONE launch all the same (r03): the hardware hands workgroups to compute
    // units in launch order, so the workgroups of node `slots` + k start as those of an earlier node leave -- a finished node's
    // successor starts at once instead of at the next launch boundary, where the chip used to wait for the host (9 % of the cold
    // config-4 search) and for the slowest node of the launch (6 %).  The earliest incomplete node is first in line for every unit
    // that frees up, so it always completes its set; its early workgroups poll meanwhile (bounded waits of ~0.6 s against node
    // run times of milliseconds).  LPX_GROUP_WALK=0: launches of `slots` nodes and 96 pivots, refilled by the host in between.
    static const bool walk_env = [] { const char* e = std::getenv("LPX_GROUP_WALK"); return !(e && e[0] == '0'); }();
    const bool walk = walk_env && cb == nullptr && count > slots;
    const int chunk = cb ? (o0->batch > 0 ? o0->batch : 256) : (walk ? (1 << 20) : (count > slots ? (chunk_env > 0 ? chunk_env : 96) : 1024));
    std::vector<int> live(count);
    for (int i = 0; i < count; ++i) live[i] = i;
    std::vector<int> fired(count, 0);
    std::vector<DevState> before(count);
    std::vector<char> snapped(count, 0);
    // What an aborted launch goes back to: with a pivot callback the state at the START OF THAT LAUNCH (the callbacks of the
    // earlier launches have fired), snapshot per launch; without one (B&B batches) the node's state at its FIRST launch --
    // one snapshot per node instead of one per launch (a node of config 4 takes eight launches), the rare restart repeats
    // the node's pivots on the streaming kernels and ends in the same tableau.
    const bool snap_each_launch = cb != nullptr;
    long long launches = 0;
    while (!live.empty()) {
        const int n = walk ? (int)std::min<size_t>(live.size(), 65535) : ((int)live.size() < slots ? (int)live.size() : slots);   // gridDim.y <= 65535
        int nsnap = 0; size_t maxd = 2;
        for (int k = 0; k < n; ++k) {
            g.h[k] = node[live[k]];
            lpx_tableau* t = ts[live[k]];
            if (snap_each_launch || !snapped[live[k]]) {
                before[live[k]] = g.hs[live[k]];
                ParkDesc& d = g.pd_h[nsnap++];
                d.srcT = t->T; d.dstT = t->xT; d.srcB = t->basis; d.dstB = t->xbasis;
                d.doubles = (size_t)t->R * t->ld; d.m = t->R - 1; d.pad = 0;
                maxd = std::max(maxd, d.doubles);
                snapped[live[k]] = 1;
            }
        }
        if (nsnap > 0) {                        // the snapshots of this launch: one multi-copy launch (lpx_park_many)
            LPX_HIP_TRY(hipMemcpyAsync(g.pd_d, g.pd_h, sizeof(ParkDesc) * (size_t)nsnap, hipMemcpyHostToDevice, g.stream));
            const int bpn = (int)std::min<size_t>(256, std::max<size_t>(1, maxd / 2 / 256 / 4));
            LPX_HIP_TRY(launch_park_many(g.pd_d, nsnap, bpn, g.stream));
        }
        // the kernel writes each node's new state into the pinned mirror (ResNode::st_host): nothing is copied back
        LPX_HIP_TRY(hipMemcpyAsync(g.d, g.h, sizeof(ResNode) * n, hipMemcpyHostToDevice, g.stream));
        if (plan.nt) LPX_HIP_TRY(launch_resident_regs(g.d, n, grid, plan.nt, plan.rt, lds, chunk, g.stream));
        else LPX_HIP_TRY(launch_resident_group(g.d, n, grid, lds, chunk, g.stream));
        LPX_HIP_TRY(hipStreamSynchronize(g.stream));
        bool aborted = false;
        for (int k = 0; k < n; ++k) if (g.hs[live[k]].pad[1]) aborted = true;
        if (aborted) {
            for (int k = 0; k < n; ++k) resident_buffers_clear(ts[live[k]]);
            set_error("resident group loop: an exchange wait expired (workgroups not co-resident?)");
            // A node whose launch aborted goes back to the state of the launch's start (tableau, basis, counters: a late
            // workgroup may have stored rows of a pivot the others never made); the other nodes of the launch finished it
            // normally and keep what they wrote.  The caller finishes every unfinished node on the streaming kernels.
            for (int k = 0; k < n; ++k) {
                if (!g.hs[live[k]].pad[1]) continue;
                lpx_tableau* t = ts[live[k]];
                { int rc = restore_launch_start(t); if (rc) return rc; }
                g.hs[live[k]] = before[live[k]];
                g.hs[live[k]].pad[1] = 0;
                LPX_HIP_TRY(hipMemcpy(t->st, &g.hs[live[k]], sizeof(DevState), hipMemcpyHostToDevice));
            }
            for (int i = 0; i < count; ++i) statuses[i] = g.hs[i].status;      // LPX_RUNNING marks the unfinished ones
            if (resume) std::memcpy(resume, g.hs, sizeof(DevState) * count);
            return LPX_RESIDENT_RETRY;
        }
        ++launches;
        if (launches > 4LL * count * ((long long)popts->max_iter + dopts->max_iter + dopts->fdf_guard) / chunk + 64) {
            set_error("resident group loop: launch budget exhausted while still running"); return LPX_ITER_LIMIT; }
        std::vector<int> next;
        for (int k = 0; k < n; ++k) {
            const int i = live[k];
            const DevState& s = g.hs[i];
            { int rc = fire_trace_callbacks(ts[i], fired[i], s.iter, cb, user); if (rc) return rc; }
            fired[i] = s.iter;
            if (s.status == LPX_RUNNING) next.push_back(i);
        }
        for (size_t k = (size_t)n; k < live.size(); ++k) next.push_back(live[k]);
        live.swap(next);
    }
    const double ms = now_ms() - t0;
    for (int i = 0; i < count; ++i) {
        const DevState& s = g.hs[i];
        *ts[i]->hst = s;
        statuses[i] = s.status;
        if (stats) stats_from_state(stats[i], s, dual[i], ms / (double)count, launches, false);
    }
    return 0;
}
