// lpx_tableau_groups.cpp -- host side of the group runs on the streaming kernels and the C entry points lpx_multi_run*: the two-launch
// group run (lpx_kernels.hip), the fused group run in one call and in two halves (lpx_group_fused.hip), and the per-node loops.
// The resident group run lpx_multi_run tries first is in lpx_tableau_resident.cpp.
#include "lpx_handle.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace lpx;

// ---------------------------------------------------------------------------------------------------
// Batched group run (K9): all tableaux of a group advance one pivot per launch pair (blockIdx.y = node),
// so many small node LPs fill the chip from ONE stream instead of competing for a few hardware queues.
// ---------------------------------------------------------------------------------------------------
namespace {

struct GroupBuf {
    SelParams* d = nullptr; SelParams* h = nullptr; DevState* hs = nullptr; int cap = 0;
    hipStream_t stream = nullptr;
    hipGraphExec_t gexec = nullptr; std::string gkey;
};
GroupBuf g_groups[2];        // [primal, dual]; lpx handles are used from one thread per process

int group_reserve(GroupBuf& g, int count)
{
    if (!g.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    if (count <= g.cap) return 0;
    if (g.gexec) { hipGraphExecDestroy(g.gexec); g.gexec = nullptr; g.gkey.clear(); }
    hipFree(g.d); if (g.h) hipHostFree(g.h); if (g.hs) hipHostFree(g.hs);
    g.d = nullptr; g.h = nullptr; g.hs = nullptr; g.cap = 0;
    const int c = count + 16;
    LPX_HIP_TRY(hipMalloc((void**)&g.d, sizeof(SelParams) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.h, sizeof(SelParams) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.hs, sizeof(DevState) * c));
    g.cap = c;
    return 0;
}

struct GroupRun {
    GroupBuf* g = nullptr; std::vector<int> idx; int dual = 0; int batch = 64; long long budget = 0, enq = 0;
    int max_nblk = 1, max_blocks = 1, maxR = 2, maxC = 2; bool done = true;
    int min_active = 0; bool suspended_exit = false;     // stop (without exhausting the budget) once this few nodes are still running
};

int group_begin(GroupRun& r, lpx_tableau** ts, const lpx_run_opts* o, const DevState* inits = nullptr)
{
    GroupBuf& g = *r.g;
    const int K = (int)r.idx.size();
    int rc = group_reserve(g, K); if (rc) return rc;
    r.batch = o->batch > 0 ? o->batch : 64;
    r.budget = pivot_budget(o, r.dual) + (r.dual ? 8 : 2);
    r.max_nblk = 1; r.max_blocks = 1; r.maxR = 2; r.maxC = 2;
    for (int k = 0; k < K; ++k) {
        lpx_tableau* t = ts[r.idx[k]];
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));               // node assembly ran on the node's own stream
        SelParams p = base_params(t, o, r.dual ? MODE_DUAL : MODE_PRIMAL);
        if (!r.dual && !p.us) { set_error("batched primal run needs the multi-workgroup select"); return LPX_EINVAL; }
        g.h[k] = p;
        if (p.nblk > r.max_nblk) r.max_nblk = p.nblk;
        const int ub = update_blocks(t->ld, t->Rcap);
        if (ub > r.max_blocks) r.max_blocks = ub;
        if (t->Rcap > r.maxR) r.maxR = t->Rcap;
        if (t->Ccap > r.maxC) r.maxC = t->Ccap;
        g.hs[k] = fresh_state(r.dual);
        if (inits) resume_from(g.hs[k], inits[r.idx[k]], r.dual);
    }
    LPX_HIP_TRY(hipMemcpyAsync(g.d, g.h, sizeof(SelParams) * K, hipMemcpyHostToDevice, g.stream));
    LPX_HIP_TRY(launch_states_scatter(g.d, g.hs, K, g.stream));      // every node's initial state record, one launch
    if (!r.dual) LPX_HIP_TRY(launch_group_init(g.d, K, g.stream));
    else LPX_HIP_TRY(launch_group_rhs_init(g.d, K, g.stream));
    // graph of `batch` iterations, keyed by everything baked into the launches
    char keybuf[160];
    std::snprintf(keybuf, sizeof(keybuf), "%p/%d/%d/%d/%d/%d/%d/%d", (void*)g.d, K, r.dual, r.max_nblk, r.max_blocks, r.batch, r.maxR, r.maxC);
    if (o->use_graph && g.gkey != keybuf) {
        if (g.gexec) { hipGraphExecDestroy(g.gexec); g.gexec = nullptr; }
        LPX_HIP_TRY(hipStreamSynchronize(g.stream));
        hipGraph_t graph = nullptr;
        LPX_HIP_TRY(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < r.batch; ++i) {
            hipError_t e = launch_group_iter(g.d, K, r.dual, r.max_nblk, r.max_blocks, g.stream, r.maxR, r.maxC);
            if (e != hipSuccess) { hipStreamEndCapture(g.stream, &graph); if (graph) hipGraphDestroy(graph); set_error("group capture failed"); return LPX_EDEVICE; }
        }
        LPX_HIP_TRY(hipStreamEndCapture(g.stream, &graph));
        hipError_t e = hipGraphInstantiate(&g.gexec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (e != hipSuccess) { g.gexec = nullptr; set_error("group graph instantiate failed"); return LPX_EDEVICE; }
        g.gkey = keybuf;
    }
    r.enq = 0; r.done = false;
    return 0;
}

int group_submit(GroupRun& r, const lpx_run_opts* o)
{
    GroupBuf& g = *r.g;
    const int K = (int)r.idx.size();
    if (o->use_graph && g.gexec) LPX_HIP_TRY(hipGraphLaunch(g.gexec, g.stream));
    else for (int i = 0; i < r.batch; ++i) LPX_HIP_TRY(launch_group_iter(g.d, K, r.dual, r.max_nblk, r.max_blocks, g.stream, r.maxR, r.maxC));
    r.enq += r.batch;
    LPX_HIP_TRY(launch_states_gather(g.d, g.hs, K, g.stream));       // every node's state record into the pinned array, one launch
    return 0;
}

int group_complete(GroupRun& r)
{
    GroupBuf& g = *r.g;
    LPX_HIP_TRY(hipStreamSynchronize(g.stream));
    int running = 0;
    for (size_t k = 0; k < r.idx.size(); ++k) if (g.hs[k].status == LPX_RUNNING) ++running;
    r.done = running == 0 || r.enq >= r.budget;
    if (!r.done && r.min_active > 0 && running <= r.min_active) { r.done = true; r.suspended_exit = true; }
    return 0;
}


// ---------------------------------------------------------------------------------------------------
// Fused group run (K4g, lpx_group_fused): ONE launch per step for the whole group -- update(k) of every live node out of place
// beside select(k+1) of every live node -- and a live list instead of early-exit workgroups: between polls the host drops the
// finished nodes from the grid.  Launches are eager (a launch costs the host ~5 us against a step of tens of microseconds on
// the device, and the grid changes from poll to poll).  Every node needs its second tableau buffer (fused_buffers); a group in
// which one does not get it runs on the two-launch kernels above.  LPX_GROUP_FUSED=0: never (diagnostic).
// ---------------------------------------------------------------------------------------------------
struct FusedGroupBuf {
    FusedParams* d = nullptr; FusedParams* h = nullptr;     // parameter records: device / pinned
    DevState* hs = nullptr;                                  // pinned: initial states in, latest records out
    DevState* ds = nullptr;                                  // device copy of the initial states
    int* live_d = nullptr; int* live_h = nullptr;            // live list (two halves: launches of window w read half w & 1)
    int* comp_d = nullptr; int* comp_h = nullptr;            // device-side compaction record (lpx_group_fused.hip FG_COMP_*) and its pinned staging
    int* fresh_d = nullptr; int* fresh_h = nullptr;
    int* cur_h = nullptr;                                    // pinned: index of every node's latest record
    int cap = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
};

FusedGroupBuf g_fgroups[LPX_ASYNC_SLOTS + 1];   // [0 .. LPX_ASYNC_SLOTS): the asynchronous batches (lpx_multi_run_begin / _end), [LPX_ASYNC_SLOTS]: the synchronous runs

int fused_group_reserve(FusedGroupBuf& g, int count)
{
    static const bool one_stream = [] { const char* e = std::getenv("LPX_ROLL_ONE_STREAM"); return e && e[0] == '1'; }();   // experiment
    if (!g.stream && one_stream && &g >= &g_fgroups[0] && &g < &g_fgroups[LPX_ASYNC_SLOTS])
        for (int k = 0; k < LPX_ASYNC_SLOTS && !g.stream; ++k) if (g_fgroups[k].stream) g.stream = g_fgroups[k].stream;
    if (!g.stream) {
        // LOWEST priority: a window is a dozen chip-filling launches in a row; the small launches the host needs answered while the
        // other batch pivots (solution read-back, parking, child assembly: other streams, default priority) must get their
        // workgroups in as slots free up instead of queueing behind the window (measured: they waited 1-2 ms each without this)
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = 0; }
        if (hipStreamCreateWithPriority(&g.stream, hipStreamNonBlocking, least) != hipSuccess) {
            (void)hipGetLastError();
            LPX_HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
        }
    }
    if (count <= g.cap) return 0;
    hipFree(g.d); hipFree(g.ds); hipFree(g.live_d); hipFree(g.fresh_d); hipFree(g.comp_d);
    if (g.comp_h) hipHostFree(g.comp_h);
    if (g.h) hipHostFree(g.h); if (g.hs) hipHostFree(g.hs); if (g.live_h) hipHostFree(g.live_h);
    if (g.fresh_h) hipHostFree(g.fresh_h); if (g.cur_h) hipHostFree(g.cur_h);
    { hipStream_t st = g.stream; std::vector<hipEvent_t> ev = std::move(g.ev); g = FusedGroupBuf{}; g.stream = st; g.ev = std::move(ev); }
    const int c = count + 16;
    LPX_HIP_TRY(hipMalloc((void**)&g.d, sizeof(FusedParams) * c));
    LPX_HIP_TRY(hipMalloc((void**)&g.ds, sizeof(DevState) * c));
    LPX_HIP_TRY(hipMalloc((void**)&g.live_d, sizeof(int) * 2 * c));
    LPX_HIP_TRY(hipMalloc((void**)&g.fresh_d, sizeof(int) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.h, sizeof(FusedParams) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.hs, sizeof(DevState) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.live_h, sizeof(int) * 2 * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.fresh_h, sizeof(int) * c));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.cur_h, sizeof(int) * c));
    LPX_HIP_TRY(hipMalloc((void**)&g.comp_d, sizeof(int) * group_fused_comp_ints(c)));
    LPX_HIP_TRY(hipHostMalloc((void**)&g.comp_h, sizeof(int) * 2 * (32 + c)));       // two windows' worth of {counts, list of parity 0}
    LPX_HIP_TRY(hipMemsetAsync(g.comp_d, 0, sizeof(int) * group_fused_comp_ints(c), g.stream));
    g.cap = c;
    return 0;
}


// parameter records, initial states and the init launch of a group; returns LPX_RESIDENT_RETRY when the group cannot take the
// fused path (nothing has been touched then)
int fused_prepare(FusedGroupBuf& g, lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                  const DevState* inits, int* per_node_out, int* batch_out, long long* budget_out)
{
    static const bool enabled = [] { const char* e = std::getenv("LPX_GROUP_FUSED"); return !(e && e[0] == '0'); }();
    if (!enabled || count < 1) return LPX_RESIDENT_RETRY;
    for (int i = 0; i < count; ++i) if (ts[i]->fused_off) return LPX_RESIDENT_RETRY;
    for (int i = 0; i < count; ++i) if (!fused_buffers(ts[i])) return LPX_RESIDENT_RETRY;
    { int rc = fused_group_reserve(g, count); if (rc) return rc; }
    int per_node = 1, nfresh = 0, batch = 64;
    long long budget = 0;
    for (int k = 0; k < count; ++k) {
        lpx_tableau* t = ts[k];
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));               // node assembly ran on the node's own stream
        const lpx_run_opts* o = dual[k] ? dopts : popts;
        FusedParams f; std::memset(&f, 0, sizeof(f));
        f.P = base_params(t, o, dual[k] ? MODE_DUAL : MODE_PRIMAL);
        f.T1 = t->fT; f.prow1 = t->fprow; f.rhs1 = t->frhs; f.rec = t->frec;
        const bool cont = t->fsuspended;                            // continues a fused run: its records are in place
        f.par = cont ? (t->frec_cur & 1) : 0;
        g.h[k] = f;
        g.hs[k] = fresh_state(dual[k]);
        if (inits) resume_from(g.hs[k], inits[k], dual[k]);
        if (!cont) g.fresh_h[nfresh++] = k;
        t->fsuspended = false;
        per_node = std::max(per_node, group_fused_blocks(t->ld, t->Rcap));
        batch = o->batch > 0 ? o->batch : 64;
        budget = std::max(budget, pivot_budget(o, dual[k]) + (dual[k] ? 12 : 6));
    }
    batch = (batch + 1) & ~1;           // launches alternate between the two record indices: a window ends where it started
    LPX_HIP_TRY(hipMemcpyAsync(g.d, g.h, sizeof(FusedParams) * count, hipMemcpyHostToDevice, g.stream));
    if (nfresh > 0) {
        LPX_HIP_TRY(hipMemcpyAsync(g.ds, g.hs, sizeof(DevState) * count, hipMemcpyHostToDevice, g.stream));
        LPX_HIP_TRY(hipMemcpyAsync(g.fresh_d, g.fresh_h, sizeof(int) * nfresh, hipMemcpyHostToDevice, g.stream));
        LPX_HIP_TRY(launch_group_fused_init(g.d, g.fresh_d, nfresh, g.ds, g.stream));
    }
    *per_node_out = per_node; *batch_out = batch; *budget_out = budget;
    return 0;
}

// A window's live list into half `half` of the buffer (live = nullptr: every node of the group), and the device's own live list,
// which starts the window equal to it (parity 0: windows are even).  *live_bytes: the tableau bytes of the live nodes.
int fused_stage_live(FusedGroupBuf& g, const int* live, int n, int half, lpx_tableau** ts, size_t* live_bytes)
{
    int* lh = g.live_h + half * g.cap;
    const int hdr = group_fused_comp_hdr();
    int* ch = g.comp_h + half * (32 + g.cap);
    std::memset(ch, 0, sizeof(int) * hdr);
    ch[0] = n;
    *live_bytes = 0;
    for (int k = 0; k < n; ++k) {
        lh[k] = ch[hdr + k] = live ? live[k] : k;
        const lpx_tableau* t = ts[lh[k]];
        *live_bytes += sizeof(double) * (size_t)t->R * t->ld;
    }
    LPX_HIP_TRY(hipMemcpyAsync(g.live_d + half * g.cap, lh, sizeof(int) * n, hipMemcpyHostToDevice, g.stream));
    LPX_HIP_TRY(hipMemcpyAsync(g.comp_d, ch, sizeof(int) * (hdr + n), hipMemcpyHostToDevice, g.stream));
    return 0;
}

// what a run leaves on its handles and reports: latest records in g.hs / g.cur_h
void fused_finish(FusedGroupBuf& g, lpx_tableau** ts, const int* dual, int count, bool unfinished_is_suspended, double ms, long long enq,
                  int* statuses, lpx_stats* stats, double prof_ms, long long prof_n)
{
    for (int k = 0; k < count; ++k) {
        lpx_tableau* t = ts[k];
        const DevState& s = g.hs[k];
        *t->hst = s;
        const bool running = s.status == LPX_RUNNING;
        statuses[k] = running ? (unfinished_is_suspended ? LPX_RUNNING : LPX_ITER_LIMIT) : s.status;
        t->suspended = statuses[k] == LPX_RUNNING;
        t->fsuspended = t->suspended;
        t->frec_cur = g.cur_h[k];
        // a finished node whose last pivot landed in the second buffer: the buffers trade places (every consumer -- solution
        // read-back, parking, child assembly, download -- goes through t->T); an unfinished one keeps its pending pivot where it is
        if (!running && s.pad[3] == 1) { std::swap(t->T, t->fT); drop_graph(t); }
        if (stats) {
            stats_from_state(stats[k], s, dual[k], ms / (double)count, enq / (long long)count + 1, true);
            if (k == 0) { stats[k].update_ms_sum = prof_ms; stats[k].update_launches = prof_n; }   // group-level figures
        }
    }
}

}  // namespace

int lpx::multi_run_fused(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                         int* statuses, lpx_stats* stats, const DevState* inits, int min_active)
{
    FusedGroupBuf& g = g_fgroups[LPX_ASYNC_SLOTS];
    const double t0 = now_ms();
    int per_node = 1, batch = 64; long long budget = 0;
    { const int rc = fused_prepare(g, ts, dual, count, popts, dopts, inits, &per_node, &batch, &budget); if (rc) return rc; }
    std::vector<int> live(count);
    for (int k = 0; k < count; ++k) live[k] = k;
    long long enq = 0; int window = 0; bool suspended_exit = false;
    const bool profile = popts->profile || dopts->profile;      // every launch bracketed by HIP events bound to the dispatch
    double prof_ms = 0.0; long long prof_n = 0;
    if (profile) while ((int)g.ev.size() < 2 * batch) { hipEvent_t e; LPX_HIP_TRY(hipEventCreate(&e)); g.ev.push_back(e); }
    while (!live.empty() && enq < budget) {
        // this window's live list (its own half of the buffer: the previous window's launches may still be reading theirs -- they
        // are not, the poll below waits, but the copy stays safe if the loop ever runs ahead)
        const int* ld_ = g.live_d + (window & 1) * g.cap;
        size_t live_bytes = 0;
        { const int rc = fused_stage_live(g, live.data(), (int)live.size(), window & 1, ts, &live_bytes); if (rc) return rc; }
        for (int i = 0; i < batch; ++i)
            LPX_HIP_TRY(launch_group_fused(g.d, ld_, (int)live.size(), per_node, (int)((enq + i) & 1), live_bytes, g.stream, g.comp_d, g.cap,
                                           profile ? g.ev[2 * i] : nullptr, profile ? g.ev[2 * i + 1] : nullptr));
        enq += batch;
        LPX_HIP_TRY(launch_group_fused_gather(g.d, count, g.hs, g.cur_h, g.stream));
        LPX_HIP_TRY(hipStreamSynchronize(g.stream));
        if (profile) {
            // launches that applied a pivot of at least one node: those up to the largest pivot count of the window's live nodes
            int full = 0;
            for (int k : live) full = std::max(full, g.hs[k].iter);
            const long long first = enq - batch;                   // launch l applies pivot l (the first launch of a run applies none)
            for (int i = 0; i < batch; ++i) {
                if (first + i < 1 || first + i > full) continue;
                float msf = 0.f;
                LPX_HIP_TRY(hipEventElapsedTime(&msf, g.ev[2 * i], g.ev[2 * i + 1]));
                prof_ms += msf; ++prof_n;
            }
        }
        ++window;
        std::vector<int> next;
        for (int k : live) if (g.hs[k].status == LPX_RUNNING) next.push_back(k);
        live.swap(next);
        if (!live.empty() && min_active > 0 && (int)live.size() <= min_active) { suspended_exit = true; break; }
    }
    fused_finish(g, ts, dual, count, suspended_exit, now_ms() - t0, enq, statuses, stats, prof_ms, prof_n);
    return 0;
}

namespace {

// ---- the same in two halves: one window of `steps` pivots of every run of a batch, enqueued and collected separately, so that the
//      host can work on one batch (read-back, parking, assembly of the next nodes) while the other one pivots ----
struct FusedAsync { bool active = false; std::vector<lpx_tableau*> ts; std::vector<int> dual; double t0 = 0; long long enq = 0; hipEvent_t done = nullptr; };
FusedAsync g_fasync[LPX_ASYNC_SLOTS];

// What lpx_multi_run, _some and _begin open with: the default option records, and no null or empty tableau in the group.
int group_args(const char* fn, lpx_tableau** ts, int count, const lpx_run_opts*& popts, const lpx_run_opts*& dopts,
               lpx_run_opts& pd, lpx_run_opts& dd)
{
    if (!popts) { lpx_default_opts(&pd, 0); popts = &pd; }
    if (!dopts) { lpx_default_opts(&dd, 1); dopts = &dd; }
    for (int i = 0; i < count; ++i)
        if (!ts[i] || ts[i]->R < 2) { set_error(std::string(fn) + ": null or empty tableau"); return LPX_EINVAL; }
    return 0;
}

int multi_run_batched(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts,
                             const lpx_run_opts* dopts, int* statuses, lpx_stats* stats, const DevState* inits = nullptr, int min_active = 0)
{
    {   // one launch per step when every node has its second buffer (and none is in the middle of a two-launch run)
        bool any_two_launch = false;
        for (int i = 0; i < count; ++i) if (ts[i]->suspended2) any_two_launch = true;
        if (!any_two_launch) {
            const int rc = multi_run_fused(ts, dual, count, popts, dopts, statuses, stats, inits, min_active);
            if (rc != LPX_RESIDENT_RETRY) return rc;
        }
    }
    GroupRun runs[2];
    for (int w = 0; w < 2; ++w) { runs[w].g = &g_groups[w]; runs[w].dual = w; runs[w].min_active = min_active; }
    for (int i = 0; i < count; ++i) runs[dual[i] ? 1 : 0].idx.push_back(i);
    const double t0 = now_ms();
    for (int w = 0; w < 2; ++w) if (!runs[w].idx.empty()) { int rc = group_begin(runs[w], ts, w ? dopts : popts, inits); if (rc) return rc; }
    for (;;) {
        bool any = false;
        for (int w = 0; w < 2; ++w) if (!runs[w].done) { int rc = group_submit(runs[w], w ? dopts : popts); if (rc) return rc; any = true; }
        if (!any) break;
        for (int w = 0; w < 2; ++w) if (!runs[w].idx.empty() && runs[w].enq > 0 && !runs[w].done) { int rc = group_complete(runs[w]); if (rc) return rc; }
    }
    const double ms = now_ms() - t0;
    for (int w = 0; w < 2; ++w) {
        GroupRun& r = runs[w];
        for (size_t k = 0; k < r.idx.size(); ++k) {
            const DevState& s = r.g->hs[k];
            const int i = r.idx[k];
            *ts[i]->hst = s;
            statuses[i] = s.status == LPX_RUNNING ? (r.suspended_exit ? LPX_RUNNING : LPX_ITER_LIMIT) : s.status;
            ts[i]->suspended = statuses[i] == LPX_RUNNING;          // continues from *hst in the next lpx_multi_run_some
            ts[i]->suspended2 = ts[i]->suspended;
            if (stats) stats_from_state(stats[i], s, w != 0, ms / (double)count, 2 * r.enq / (long long)(r.idx.size() ? r.idx.size() : 1), false);
        }
    }
    return 0;
}

}  // namespace

extern "C" {

int lpx_multi_run_begin(int slot, lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts, int steps)
{
    if (slot < 0 || slot >= LPX_ASYNC_SLOTS || !ts || !dual || count < 1 || steps < 1) { set_error("lpx_multi_run_begin: bad argument"); return LPX_EINVAL; }
    FusedAsync& a = g_fasync[slot];
    if (a.active) { set_error("lpx_multi_run_begin: this slot has a batch in flight (lpx_multi_run_end first)"); return LPX_EINVAL; }
    lpx_run_opts pd, dd;
    { const int rc = group_args("lpx_multi_run_begin", ts, count, popts, dopts, pd, dd); if (rc) return rc; }
    for (int i = 0; i < count; ++i)
        if (ts[i]->suspended2) { set_error("lpx_multi_run_begin: a run suspended on the two-launch kernels cannot continue here"); return LPX_EINVAL; }
    if (popts->profile || dopts->profile) return 1;
    FusedGroupBuf& g = g_fgroups[slot];
    int per_node = 1, batch = 64; long long budget = 0;
    const double t0 = now_ms();
    {
        const int rc = fused_prepare(g, ts, dual, count, popts, dopts, nullptr, &per_node, &batch, &budget);
        if (rc == LPX_RESIDENT_RETRY) return 1;                 // not available for this batch: the caller takes lpx_multi_run_some
        if (rc) return rc;
    }
    steps = (steps + 1) & ~1;
    size_t live_bytes = 0;
    { const int rc = fused_stage_live(g, nullptr, count, 0, ts, &live_bytes); if (rc) return rc; }
    for (int i = 0; i < steps; ++i) LPX_HIP_TRY(launch_group_fused(g.d, g.live_d, count, per_node, i & 1, live_bytes, g.stream, g.comp_d, g.cap));
    LPX_HIP_TRY(launch_group_fused_gather(g.d, count, g.hs, g.cur_h, g.stream));
    if (!a.done) LPX_HIP_TRY(hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    LPX_HIP_TRY(hipEventRecord(a.done, g.stream));              // the two slots may share a stream: wait for THIS window, not for the stream
    a.active = true; a.ts.assign(ts, ts + count); a.dual.assign(dual, dual + count); a.t0 = t0; a.enq = steps;
    return 0;
}

int lpx_multi_run_end(int slot, int* statuses, lpx_stats* stats)
{
    if (slot < 0 || slot >= LPX_ASYNC_SLOTS || !statuses) { set_error("lpx_multi_run_end: bad argument"); return LPX_EINVAL; }
    FusedAsync& a = g_fasync[slot];
    if (!a.active) { set_error("lpx_multi_run_end: no batch in flight in this slot"); return LPX_EINVAL; }
    FusedGroupBuf& g = g_fgroups[slot];
    a.active = false;
    LPX_HIP_TRY(hipEventSynchronize(a.done));
    fused_finish(g, a.ts.data(), a.dual.data(), (int)a.ts.size(), true, now_ms() - a.t0, a.enq, statuses, stats, 0.0, 0);
    return 0;
}

int lpx_multi_run(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts,
                  const lpx_run_opts* dopts, int* statuses, lpx_stats* stats)
{
    if (!ts || !dual || count < 0 || !statuses) { set_error("lpx_multi_run: bad argument"); return LPX_EINVAL; }
    lpx_run_opts pd, dd;
    { const int rc = group_args("lpx_multi_run", ts, count, popts, dopts, pd, dd); if (rc) return rc; }
    bool mb_ok = true;                          // every primal node has the multi-workgroup select's record (the group kernels need it)
    for (int i = 0; i < count; ++i) if (!dual[i] && !ts[i]->us) mb_ok = false;
    // Nodes small enough to live on chip a few at a time (lpx_resident_group.hip): four 8 MB nodes of config 4 run side by
    // side, 25 % faster than 32 of them streaming through HBM.  LPX_RESIDENT_GROUP=0 keeps the batched streaming run.
    static const bool resgroup_env = [] { const char* e = std::getenv("LPX_RESIDENT_GROUP"); return !(e && e[0] == '0'); }();
    if (resgroup_env && count >= 1 && !popts->profile && !dopts->profile && popts->resident >= 0 && dopts->resident >= 0) {
        bool ok = mb_ok;
        for (int i = 0; i < count; ++i) if (ts[i]->resident_off) ok = false;
        const ResGroupPlan plan = ok ? resident_group_plan(ts, count) : ResGroupPlan{};
        if (plan.slots) {
            std::vector<DevState> resume(count);
            const int rc = run_resident_group(ts, dual, count, popts, dopts, statuses, stats, plan, nullptr, nullptr, resume.data());
            if (rc != LPX_RESIDENT_RETRY) return rc;
            // some workgroup could not take part (GPU shared with another process?): finish the unfinished nodes on the
            // batched streaming kernels, from the pivot each of them had reached
            std::vector<lpx_tableau*> sub; std::vector<int> sdual, sidx; std::vector<DevState> sinit;
            for (int i = 0; i < count; ++i) {
                ts[i]->resident_off = true;
                if (statuses[i] == LPX_RUNNING) { sub.push_back(ts[i]); sdual.push_back(dual[i]); sidx.push_back(i); sinit.push_back(resume[i]); }
                else if (stats) { stats_from_state(stats[i], resume[i], dual[i], 0.0, 0, false); *ts[i]->hst = resume[i]; }
            }
            if (!sub.empty()) {
                std::vector<int> sst(sub.size()); std::vector<lpx_stats> sss(sub.size());
                int rc2;
                if (sub.size() >= 2) rc2 = multi_run_batched(sub.data(), sdual.data(), (int)sub.size(), popts, dopts, sst.data(), sss.data(), sinit.data());
                else {
                    // a single straggler: its own streaming loop, continuing at its pivot count
                    rc2 = continue_streaming(sub[0], sdual[0] ? dopts : popts, sdual[0], sinit[0], nullptr, nullptr, &sss[0]);
                    if (rc2 >= 0) { sst[0] = rc2; rc2 = 0; }
                }
                if (rc2) return rc2;
                for (size_t k = 0; k < sub.size(); ++k) { statuses[sidx[k]] = sst[k]; if (stats) stats[sidx[k]] = sss[k]; }
            }
            return 0;
        }
    }
    static const bool batched_env = [] { const char* e = std::getenv("LPX_BATCHED"); return !(e && e[0] == '0'); }();
    if (batched_env && count >= 1 && (popts->profile || dopts->profile)) {
        // profile mode: the fused group launch bracketed by HIP events (stats[0].update_ms_sum / update_launches are the group's)
        const int rc = multi_run_fused(ts, dual, count, popts, dopts, statuses, stats, nullptr, 0);
        if (rc != LPX_RESIDENT_RETRY) return rc;
    }
    if (batched_env && count >= 2 && !popts->profile && !dopts->profile && mb_ok)
        return multi_run_batched(ts, dual, count, popts, dopts, statuses, stats);
    std::vector<LoopRun> runs(count);
    std::vector<char> active(count, 0);
    for (int i = 0; i < count; ++i) {
        lpx_tableau* t = ts[i];
        const lpx_run_opts* o = dual[i] ? dopts : popts;
        SelParams p = base_params(t, o, dual[i] ? MODE_DUAL : MODE_PRIMAL);
        LoopCtx c; DevState init;
        make_ctx(t, p, c, init);
        int rc = runs[i].begin(c, init, o, pivot_budget(o, dual[i]) + (dual[i] ? 8 : 2), nullptr, nullptr);
        if (rc) return rc;
        active[i] = 1;
    }
    int remaining = count;
    while (remaining > 0) {
        for (int i = 0; i < count; ++i) if (active[i]) { int rc = runs[i].submit(); if (rc) return rc; }
        for (int i = 0; i < count; ++i) if (active[i]) {
            int rc = runs[i].complete(); if (rc) return rc;
            if (runs[i].done()) {
                statuses[i] = runs[i].finish(stats ? &stats[i] : nullptr);
                active[i] = 0; --remaining;
            }
        }
    }
    return 0;
}

// lpx_multi_run for a ROLLING batch (warm-started B&B children need a few dozen pivots each, a few of them hundreds): the run
// stops as soon as at most `min_active` nodes are still running and reports them as LPX_RUNNING; the caller hands them in again
// together with fresh nodes and they continue where they stopped (pivot count, phase, counters: the handle remembers).  Without
// it a batch of 64 runs as long as its slowest node while the device idles at the per-step latency floor.  Streaming batched
// kernels only (callers that want the resident group kernel use lpx_multi_run); min_active = 0 runs everything to the end.
int lpx_multi_run_some(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* popts, const lpx_run_opts* dopts,
                       int* statuses, lpx_stats* stats, int min_active)
{
    if (!ts || !dual || count < 0 || !statuses) { set_error("lpx_multi_run_some: bad argument"); return LPX_EINVAL; }
    lpx_run_opts pd, dd;
    { const int rc = group_args("lpx_multi_run_some", ts, count, popts, dopts, pd, dd); if (rc) return rc; }
    bool ok = count >= 1 && !popts->profile && !dopts->profile, resumed = false;
    for (int i = 0; i < count; ++i) {
        if (!dual[i] && !ts[i]->us) ok = false;
        if (ts[i]->suspended) resumed = true;
    }
    if (!ok) {
        if (resumed) { set_error("lpx_multi_run_some: a suspended run cannot continue on this path"); return LPX_EINVAL; }
        return lpx_multi_run(ts, dual, count, popts, dopts, statuses, stats);
    }
    std::vector<DevState> inits(count);
    for (int i = 0; i < count; ++i) {
        inits[i] = ts[i]->suspended ? *ts[i]->hst : fresh_state(dual[i]);
        ts[i]->suspended = false;
    }
    return multi_run_batched(ts, dual, count, popts, dopts, statuses, stats, inits.data(), min_active < count ? min_active : 0);
}

}  // extern "C"
