// lpx_node_batch.cpp -- host side of the batch of on-chip nodes (lpx_node_batch_*, C ABI of include/lpx.h): B nodes on B handles in
// ONE launch of lpx_bounded_nodes_onchip (lpx_bounded_node.hip), one workgroup per node.  Every entry is the on-chip form of
// lpx_bounded_node3 on its handle, bit for bit; the checks and what a finished node leaves on its handle are shared with it
// (lpx_tableau_bounded.cpp, through lpx_handle.h).  lpx_node_batch_run_probe is the same body with the probe launch
// (lpx_bounded_probe.hip) enqueued behind the node launch: two launches, one wait.
// lpx_node_batch_run2 is the same body again with the stall guard (include/lpx.h): stall_events = 0 is lpx_node_batch_run's launch, above 0
// the one launch is lpx_bounded_guard_onchip (lpx_bounded_guard.hip), which leaves a guard record behind each node record.
// lpx_node_batch_run3 is that body once more with reduced-cost tightening (include/lpx.h): when some entry's fix_bound is not -inf the
// one launch is lpx_bounded_fix_onchip (lpx_bounded_fix.hip), whose records carry each entry's fix_bound and the places of its list.
// lpx_node_batch_primal is the batch of bounded PRIMAL solves (lpx_bounded_primal.hip): no edit, no mask, no pick, its own small slab.
// lpx_node_batch_plunge (lpx_bounded_plunge.hip) has its own slab layout and its own walk over a chain's records; what it does as
// the others do -- the checks of the flags and of an entry, the growth of the buffers, the mask, the header and the parameter
// record of an entry, the message of a refusal -- are the sub-steps of the anonymous namespace, called from both.
#include "lpx_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace lpx;

struct lpx_node_batch {
    std::vector<lpx_tableau*> h;            // [W] borrowed
    std::vector<hipStream_t> streams;       // the distinct streams of the handles; streams[0] carries the launch
    char* slab = nullptr; size_t slab_bytes = 0;        // pinned: NodeParams [B], NodeOut [B] (64 bytes each), then per entry NodeIn + triples
    char* edit = nullptr; size_t edit_bytes = 0;        // device: per entry the layout of one bound edit (5 K doubles, K int32)
    uint8_t* mask = nullptr; size_t mask_cap = 0;       // device copy of the integer mask ...
    std::vector<uint8_t> mask_h; int mask_n = -1;       // ... and the host bytes it was made from
    std::vector<int32_t> seen; int32_t call = 0;        // seen[s] == call: slot s is named already in this call
    std::vector<size_t> off_in, off_edit; std::vector<uint8_t> any_lo;      // per entry, kept to spare the steady state its allocations
    std::vector<size_t> off_trip; std::vector<uint8_t> colmark;             // the plunge: an entry's first triple; scratch of its integrality check
    char* probews = nullptr; size_t probews_bytes = 0; std::vector<size_t> off_ws;     // the probes: device workspace, an entry's share of it
};

namespace {

constexpr size_t kOut = 64;
static_assert(sizeof(NodeOut) <= kOut, "slab layout");
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// The launch goes behind whatever a handle's own stream still holds; in the steady state every stream is idle and this waits for
// nothing.  settle_all looks at the distinct streams of ALL W borrowed handles (at most the 8 of the library's pool), not only at
// those of the entries named in `slot`, and the launch always goes on streams[0], the first handle's, whether or not that handle
// takes part.  Both are deliberate and safe: waiting for more streams than the contract names orders the launch behind a superset
// of the work it must follow, and the host waits on streams[0] before it returns, so no handle's own stream can start later work
// on a tableau the kernel is still writing.  Narrowing either would save nothing in the steady state.
int settle(hipStream_t s)
{
    if (hipStreamQuery(s) == hipSuccess) return 0;
    (void)hipGetLastError();
    LPX_HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int settle_all(lpx_node_batch* b) { for (hipStream_t s : b->streams) { int rc = settle(s); if (rc) return rc; } return 0; }

// ---- the sub-steps that node_batch_run and lpx_node_batch_plunge share; messages and the order of the checks are the callers'

int check_flags_cutoff(const std::string& w, int B, int flags, const double* cutoff)
{
    { int r = check_long_flags(flags, 0.0, w.c_str()); if (r) return r; }
    if (flags & LPX_BDUAL_CUTOFF) {
        if (!cutoff) { set_error(w + ": null cutoff with LPX_BDUAL_CUTOFF"); return LPX_EINVAL; }
        for (int i = 0; i < B; ++i) { int r = check_long_flags(flags, cutoff[i], (w + ": entry " + std::to_string(i)).c_str()); if (r) return r; }
    }
    return 0;
}

// the batch itself, B against its W, the default options, and a new number for this call's `seen` marks
int begin_call(const std::string& w, lpx_node_batch* b, int B, const lpx_run_opts*& o, lpx_run_opts& d)
{
    if (!b) { set_error(w + ": null batch"); return LPX_EINVAL; }
    if (B > (int)b->h.size()) { set_error(w + ": B is outside [1, W]"); return LPX_EINVAL; }
    if (!o) { lpx_default_opts(&d, 1); o = &d; }
    if (b->call == INT32_MAX) { std::fill(b->seen.begin(), b->seen.end(), 0); b->call = 0; }
    ++b->call;
    return 0;
}

// entry i names a handle once and is a valid node call on it; at: "name: entry i".  *t = the handle.
int check_entry(lpx_node_batch* b, int slot, int k, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                int nint, double tol, const lpx_node_record* out, const char* at, lpx_tableau** t)
{
    if (slot < 0 || slot >= (int)b->h.size()) { set_error(std::string(at) + ": slot is outside [0, W)"); return LPX_EINVAL; }
    if (b->seen[slot] == b->call) { set_error(std::string(at) + ": slot repeats a handle"); return LPX_EINVAL; }
    b->seen[slot] = b->call;
    *t = b->h[slot];
    int r = check_change_args(*t, k, cols, lower, upper, at); if (r) return r;
    r = check_pick_args(*t, nint, tol, out, at); if (r) return r;
    r = check_node_opts(*t, o, at); if (r) return r;
    return check_node_fits(*t, at);
}

// entry i's place in the slab and in the edit staging (for kedit triples), and its share of the launch's LDS
void place_entry(lpx_node_batch* b, int i, const lpx_tableau* t, int k, int kedit, size_t& in_bytes, size_t& edit_bytes, size_t& lds)
{
    b->off_in[i] = in_bytes; b->off_edit[i] = edit_bytes;
    in_bytes += up16(sizeof(NodeIn) + (size_t)k * (2 * sizeof(double) + sizeof(int32_t)));
    edit_bytes += up16((size_t)kedit * (5 * sizeof(double) + sizeof(int32_t)));
    lds = std::max(lds, bounded_node_lds_bytes(t->R, t->C));
}

// the buffers: grown to twice the need, and only when the need outgrows them
int ensure_buffers(lpx_node_batch* b, size_t need, size_t edit_bytes, size_t ws_bytes)
{
    int r;
    if (need > b->slab_bytes) {
        r = settle_all(b); if (r) return r;
        if (b->slab) hipHostFree(b->slab);
        b->slab = nullptr; b->slab_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&b->slab, 2 * need));
        b->slab_bytes = 2 * need;
    }
    if (edit_bytes > b->edit_bytes) {
        r = settle_all(b); if (r) return r;
        hipFree(b->edit); b->edit = nullptr; b->edit_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&b->edit, 2 * edit_bytes));
        b->edit_bytes = 2 * edit_bytes;
    }
    if (ws_bytes > b->probews_bytes) {
        r = settle_all(b); if (r) return r;
        hipFree(b->probews); b->probews = nullptr; b->probews_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&b->probews, 2 * ws_bytes));
        b->probews_bytes = 2 * ws_bytes;
    }
    return 0;
}

// the device copy of the integer mask, sent again only when its bytes changed
int ensure_mask(lpx_node_batch* b, hipStream_t s, const uint8_t* is_int, int nint)
{
    if (b->mask_n == nint && std::memcmp(b->mask_h.data(), is_int, (size_t)nint) == 0) return 0;
    int r = settle(s); if (r) return r;                                  // an earlier copy may still read mask_h
    if ((size_t)nint > b->mask_cap) {
        hipFree(b->mask); b->mask = nullptr; b->mask_cap = 0;
        LPX_HIP_TRY(hipMalloc((void**)&b->mask, 2 * (size_t)nint));
        b->mask_cap = 2 * (size_t)nint;
    }
    b->mask_h.assign(is_int, is_int + nint);
    LPX_HIP_TRY(hipMemcpyAsync(b->mask, b->mask_h.data(), (size_t)nint, hipMemcpyHostToDevice, s));
    b->mask_n = nint;
    return 0;
}

// entry i's header with its triples in the slab (*in) and its parameter record (*n); cutoff is 0 without LPX_BDUAL_CUTOFF, and the
// caller sets n->out
struct EntryOpts { const lpx_run_opts* o; int flags, nint, stall_events; bool has_mask; double tol; };
void fill_entry(lpx_node_batch* b, int i, lpx_tableau* t, int k, const int32_t* cl, const double* lw, const double* up, double cutoff,
                const EntryOpts& e, NodeIn* in, NodeParams* n)
{
    lpx_tableau::Bounds& bn = t->bnd;
    bool any_lo = false;
    for (int j = 0; j < k; ++j) if (lw[j] != 0.0) any_lo = true;
    b->any_lo[i] = any_lo ? 1 : 0;
    std::memset(in, 0, sizeof(*in));
    in->K = k; in->flags = e.flags; in->nint = e.nint; in->has_mask = e.has_mask ? 1 : 0; in->max_iter = e.o->max_iter;
    in->lo_used = (bn.lo_used || any_lo) ? 1 : 0;
    in->eps = e.o->eps; in->ratio_tol = e.o->ratio_tol; in->cutoff = cutoff; in->tol = e.tol;
    in->stall_events = e.stall_events;
    if (k > 0) {
        double* a = reinterpret_cast<double*>(in + 1);
        std::memcpy(a, lw, sizeof(double) * k);
        std::memcpy(a + k, up, sizeof(double) * k);
        std::memcpy(a + 2 * (size_t)k, cl, sizeof(int32_t) * k);
    }
    std::memset(n, 0, sizeof(*n));
    n->T = t->T; n->ld = t->ld; n->R = t->R; n->C = t->C;
    n->rhsbuf = t->rhsbuf; n->basis = t->basis; n->trace = t->trace; n->trace_cap = t->trace_cap; n->st = t->st;
    n->ub = bn.ub; n->lo = bn.lo; n->flip = bn.flip; n->edit = reinterpret_cast<double*>(b->edit + b->off_edit[i]); n->mask = b->mask;
    n->in = in;
}

// the message of the first entry the kernel refused; at: "name: entry i" (the plunge: with the node inside the chain)
void set_refusal(const std::string& at, const NodeOut* rec)
{
    if (rec->inf_k >= 0) set_error(at + ": upper[" + std::to_string(rec->inf_k) + "] = +inf on a flipped column");
    else set_error(at + ": " + std::to_string(rec->unrepairable) + " column(s) with a negative reduced cost and no upper "
                   "bound: a bound flip cannot restore dual feasibility");
}

}  // namespace

extern "C" {

int lpx_node_batch_create(int W, lpx_tableau* const* handles, lpx_node_batch** out)
{
    const std::string w = "lpx_node_batch_create";
    if (!out || !handles) { set_error(w + ": null argument"); return LPX_EINVAL; }
    if (W < 1 || W > 1024) { set_error(w + ": W is outside [1, 1024]"); return LPX_EINVAL; }
    for (int i = 0; i < W; ++i) {
        const std::string at = w + ": handle " + std::to_string(i);
        lpx_tableau* t = handles[i];
        if (!t) { set_error(at + ": null handle"); return LPX_EINVAL; }
        if (!t->bnd.bounds_set) { set_error(at + ": the handle has no bounds (lpx_tableau_set_bounds first)"); return LPX_EINVAL; }
        if (t->bnd.bounds_C != t->C) { set_error(at + ": the live shape changed since lpx_tableau_set_bounds"); return LPX_EINVAL; }
        int rc = check_node_fits(t, at.c_str()); if (rc) return rc;
    }
    {
        std::vector<lpx_tableau*> sorted(handles, handles + W);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_error(w + ": a handle is named twice"); return LPX_EINVAL; }
    }
    int rc = ensure_device(); if (rc) return rc;
    rc = bounded_node_ready(w.c_str()); if (rc) return rc;
    lpx_node_batch* b = new lpx_node_batch();
    b->h.assign(handles, handles + W);
    for (lpx_tableau* t : b->h)
        if (std::find(b->streams.begin(), b->streams.end(), t->stream) == b->streams.end()) b->streams.push_back(t->stream);
    b->seen.assign((size_t)W, 0);
    b->off_in.resize((size_t)W); b->off_edit.resize((size_t)W); b->any_lo.resize((size_t)W); b->off_trip.resize((size_t)W); b->off_ws.resize((size_t)W);
    *out = b;
    return 0;
}

void lpx_node_batch_destroy(lpx_node_batch* b)
{
    if (!b) return;
    for (hipStream_t s : b->streams) hipStreamSynchronize(s);
    if (b->slab) hipHostFree(b->slab);
    hipFree(b->edit); hipFree(b->mask); hipFree(b->probews);
    delete b;
}

// lpx_node_batch_run (pr = null, name its own) and lpx_node_batch_run_probe in one body: with pr the probe launch goes behind the
// node launch on the same stream and the one wait covers both.
struct ProbeArgs { const double* prune; int cand_max, probe_iter; lpx_probe_head* head; lpx_probe_record* probes; };
// lpx_node_batch_run2 in the same body (gd non-null, never together with pr): with stall_events > 0 the one launch is the guarded
// kernel's (lpx_bounded_guard.hip), which leaves a guard record in the 64-byte slot of each node record.
struct GuardArgs { int stall_events; lpx_guard_record* guard; };
// lpx_node_batch_run3 in the same body (fx non-null, always with gd, never with pr): fix_bound per entry; when one of them is not
// -inf the one launch is the kernel of lpx_bounded_fix.hip, which lists the columns it tightened per entry.
struct FixArgs { const double* fix_bound; lpx_fix_list* fix; };

static int node_batch_run(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                          const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, int nint, const uint8_t* is_int,
                          double tol, lpx_node_record* out, int32_t* rc, const ProbeArgs* pr, const char* name,
                          const GuardArgs* gd = nullptr, const FixArgs* fx = nullptr)
{
    const std::string w = name;
    const int stall_events = gd ? gd->stall_events : 0;
    const double ninf = -1.0 / 0.0;
    bool fixing = false;
    // ---- 1. every argument of every entry, before anything is written and before any device check
    if (!slot || !K || !out || !rc) { set_error(w + ": null " + (!slot ? "slot" : !K ? "K" : !out ? "out" : "rc")); return LPX_EINVAL; }
    if (stall_events < 0) { set_error(w + ": stall_events is negative"); return LPX_EINVAL; }
    if (pr) {
        if (!pr->prune || !pr->head || !pr->probes) { set_error(w + ": null " + (!pr->prune ? "prune" : !pr->head ? "head" : "probes")); return LPX_EINVAL; }
        int r = check_probe_args(pr->cand_max, pr->probe_iter, name); if (r) return r;
    }
    if (B < 1) { set_error(w + ": B is outside [1, W]"); return LPX_EINVAL; }
    { int r = check_flags_cutoff(w, B, flags, cutoff); if (r) return r; }
    if (pr)
        for (int i = 0; i < B; ++i)
            if (pr->prune[i] != pr->prune[i]) { set_error(w + ": entry " + std::to_string(i) + ": prune is NaN"); return LPX_EINVAL; }
    if (fx) {
        if (!fx->fix_bound) { set_error(w + ": null fix_bound"); return LPX_EINVAL; }
        for (int i = 0; i < B; ++i) {
            const lpx_fix_list* fl = fx->fix ? &fx->fix[i] : nullptr;
            if (check_fix_args(fx->fix_bound[i], fl, nint, name))        // again with the entry in front: no string per entry in the steady state
                return check_fix_args(fx->fix_bound[i], fl, nint, (w + ": entry " + std::to_string(i)).c_str());
            if (fx->fix_bound[i] != ninf) fixing = true;
        }
    }
    lpx_run_opts d;
    { int r = begin_call(w, b, B, o, d); if (r) return r; }
    size_t sumK = 0, in_bytes = 0, edit_bytes = 0, lds = 0;
    size_t ws_bytes = 0;
    char at[56];                                                         // "lpx_node_batch_run: entry i", no allocation per entry
    for (int i = 0; i < B; ++i) {
        std::snprintf(at, sizeof at, "%s: entry %d", name, i);
        lpx_tableau* t = nullptr;
        const int k = K[i];
        int r = check_entry(b, slot[i], k, cols ? cols + sumK : nullptr, lower ? lower + sumK : nullptr, upper ? upper + sumK : nullptr, o,
                            nint, tol, out, at, &t);
        if (r) return r;
        place_entry(b, i, t, k, k, in_bytes, edit_bytes, lds);
        if (pr) { b->off_ws[i] = ws_bytes; ws_bytes += probe_ws_bytes(t, pr->cand_max); }
        sumK += (size_t)k;
    }
    int r = ensure_device(); if (r) return r;
    if (pr) { r = bounded_probe_ready(name); if (r) return r; }
    if (fixing) { r = bounded_fix_ready(name); if (r) return r; }
    else if (stall_events > 0) { r = bounded_guard_ready(name); if (r) return r; }
    if (fx && fx->fix) for (int i = 0; i < B; ++i) fx->fix[i].n = 0;
    if (gd && gd->guard) for (int i = 0; i < B; ++i) { gd->guard[i].bland_events = 0; gd->guard[i].first_bland = -1; }

    // ---- 2. the buffers: grown to twice the need, and only when the need outgrows them
    const size_t nrec = pr ? 2 * (size_t)pr->cand_max : 0;
    const size_t o_out = up16(sizeof(NodeParams) * (size_t)B), o_in = o_out + kOut * (size_t)B, o_pp = up16(o_in + in_bytes),
                 o_head = o_pp + up16(sizeof(ProbeParams) * (size_t)B), o_prec = o_head + sizeof(lpx_probe_head) * (size_t)B,
                 o_fp = up16(o_in + in_bytes), o_list = o_fp + up16(sizeof(FixParams) * (size_t)B),     // the tightening: records, lists
                 need = pr ? o_prec + sizeof(lpx_probe_record) * nrec * (size_t)B
                      : fixing ? o_list + fix_list_bytes(nint) * (size_t)B : o_in + in_bytes;
    r = ensure_buffers(b, need, edit_bytes, ws_bytes); if (r) return r;
    hipStream_t s = b->streams[0];
    const bool has_mask = is_int && nint > 0;
    if (has_mask) { r = ensure_mask(b, s, is_int, nint); if (r) return r; }

    // ---- 3. the slab: a parameter record, a header with its triples and a result record per entry
    NodeParams* P = reinterpret_cast<NodeParams*>(b->slab);
    sumK = 0;
    const EntryOpts eo{o, flags, nint, fixing && stall_events == 0 ? INT32_MAX : stall_events, has_mask, tol};   // the fix kernel carries the guard: INT_MAX = never
    FixParams* F = reinterpret_cast<FixParams*>(b->slab + o_fp);
    for (int i = 0; i < B; ++i) {
        lpx_tableau* t = b->h[slot[i]];
        const int k = K[i];
        NodeIn* in = reinterpret_cast<NodeIn*>(b->slab + o_in + b->off_in[i]);
        NodeParams& n = P[i];
        fill_entry(b, i, t, k, cols + sumK, lower + sumK, upper + sumK, (flags & LPX_BDUAL_CUTOFF) ? cutoff[i] : 0.0, eo, in, &n);
        n.out = reinterpret_cast<NodeOut*>(b->slab + o_out + kOut * (size_t)i);
        std::memset(&out[i], 0, sizeof(out[i]));
        out[i].pick.var = -1;
        if (pr)
            probe_params(t, o, flags, in->cutoff, pr->prune[i], nint, has_mask ? b->mask : nullptr, tol, pr->cand_max, pr->probe_iter,
                         in->lo_used != 0, b->probews + b->off_ws[i], n.out, reinterpret_cast<lpx_probe_head*>(b->slab + o_head) + i,
                         reinterpret_cast<lpx_probe_record*>(b->slab + o_prec) + nrec * (size_t)i,
                         reinterpret_cast<ProbeParams*>(b->slab + o_pp) + i);
        if (fixing) {
            n.out->pad = 0;                                              // a refused edit writes no count
            F[i].n = n; F[i].fix_bound = fx->fix_bound[i];
            fix_list_place(b->slab + o_list + fix_list_bytes(nint) * (size_t)i, nint, &F[i]);
        }
        sumK += (size_t)k;
    }

    // ---- 4. behind the handles' own streams, ONE launch (with pr: the probes behind it), ONE wait
    r = settle_all(b); if (r) return r;
    if (fixing) LPX_HIP_TRY(launch_bounded_fix_onchip(F, B, lds, s));
    else if (stall_events > 0) LPX_HIP_TRY(launch_bounded_guard_onchip(P, B, lds, s));
    else LPX_HIP_TRY(launch_bounded_nodes_onchip(P, B, lds, s));
    if (pr) LPX_HIP_TRY(launch_bounded_probe_onchip(reinterpret_cast<const ProbeParams*>(b->slab + o_pp), B, pr->cand_max, lds, s));
    LPX_HIP_TRY(hipStreamSynchronize(s));
    if (pr) {
        std::memcpy(pr->head, b->slab + o_head, sizeof(lpx_probe_head) * (size_t)B);
        std::memcpy(pr->probes, b->slab + o_prec, sizeof(lpx_probe_record) * nrec * (size_t)B);
    }

    // ---- 5. the records
    bool refused = false;
    sumK = 0;
    for (int i = 0; i < B; ++i) {
        lpx_tableau* t = b->h[slot[i]];
        const size_t at0 = sumK;
        sumK += (size_t)K[i];
        const NodeOut* rec = reinterpret_cast<const NodeOut*>(b->slab + o_out + kOut * (size_t)i);
        if ((stall_events > 0 || fixing) && gd->guard) {
            const GuardOut* g = reinterpret_cast<const GuardOut*>(rec);
            gd->guard[i].bland_events = g->bland_events; gd->guard[i].first_bland = g->first_bland;
        }
        if (rec->status < 0) {                                           // refused by the kernel: this handle is as it was
            rc[i] = LPX_EINVAL;
            out[i].unrepairable = rec->unrepairable;
            if (!refused) set_refusal(w + ": entry " + std::to_string(i), rec);
            refused = true;
            continue;
        }
        node_onchip_commit(t, rec, b->any_lo[i] != 0, &out[i]);
        if (K[i] > 0) bounds_note_edit(t, K[i], cols + at0, lower + at0, upper + at0);
        if (fixing && fx->fix_bound[i] != ninf) fix_commit(t, rec->pad, F[i], &fx->fix[i]);
        rc[i] = rec->status;
    }
    return 0;
}

int lpx_node_batch_run(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                       const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, int nint, const uint8_t* is_int,
                       double tol, lpx_node_record* out, int32_t* rc)
{
    return node_batch_run(b, B, slot, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, rc, nullptr, "lpx_node_batch_run");
}

int lpx_node_batch_run2(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                        const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, int stall_events, int nint,
                        const uint8_t* is_int, double tol, lpx_node_record* out, lpx_guard_record* guard, int32_t* rc)
{
    const GuardArgs gd{stall_events, guard};
    return node_batch_run(b, B, slot, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, rc, nullptr, "lpx_node_batch_run2", &gd);
}

int lpx_node_batch_run3(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                        const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, int stall_events, const double* fix_bound,
                        int nint, const uint8_t* is_int, double tol, lpx_node_record* out, lpx_guard_record* guard, lpx_fix_list* fix,
                        int32_t* rc)
{
    const GuardArgs gd{stall_events, guard};
    const FixArgs fx{fix_bound, fix};
    return node_batch_run(b, B, slot, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, rc, nullptr, "lpx_node_batch_run3", &gd, &fx);
}

int lpx_node_batch_run_probe(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                             const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, const double* prune, int nint,
                             const uint8_t* is_int, double tol, int cand_max, int probe_iter, lpx_node_record* out, lpx_probe_head* head,
                             lpx_probe_record* probes, int32_t* rc)
{
    const ProbeArgs pr{prune, cand_max, probe_iter, head, probes};
    return node_batch_run(b, B, slot, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, rc, &pr, "lpx_node_batch_run_probe");
}

// The batch of bounded PRIMAL solves (kernel: lpx_bounded_primals_onchip, lpx_bounded_primal.hip): entry i is the on-chip form of
// lpx_bounded_run2 on handles[slot[i]].  The steps are lpx_node_batch_run's without an edit, a mask or a pick: the slab holds a
// parameter record and a 64-byte result slot per entry.
int lpx_node_batch_primal(lpx_node_batch* b, int B, const int32_t* slot, const lpx_run_opts* o, lpx_primal_record* out, int32_t* rc)
{
    const char* name = "lpx_node_batch_primal";
    const std::string w = name;
    // ---- 1. every argument of every entry, before anything is written and before any device check
    if (!slot || !out || !rc) { set_error(w + ": null " + (!slot ? "slot" : !out ? "out" : "rc")); return LPX_EINVAL; }
    if (B < 1) { set_error(w + ": B is outside [1, W]"); return LPX_EINVAL; }
    lpx_run_opts d;
    if (b && !o) { lpx_default_opts(&d, 0); o = &d; }                    // the primal loop's defaults
    { int r = begin_call(w, b, B, o, d); if (r) return r; }
    if (o->resident > 0) { set_error(w + ": there is no resident form of the bounded loop"); return LPX_EINVAL; }
    size_t lds = 0;
    char at[56];
    for (int i = 0; i < B; ++i) {
        std::snprintf(at, sizeof at, "%s: entry %d", name, i);
        if (slot[i] < 0 || slot[i] >= (int)b->h.size()) { set_error(std::string(at) + ": slot is outside [0, W)"); return LPX_EINVAL; }
        if (b->seen[slot[i]] == b->call) { set_error(std::string(at) + ": slot repeats a handle"); return LPX_EINVAL; }
        b->seen[slot[i]] = b->call;
        const lpx_tableau* t = b->h[slot[i]];
        if (t->R < 2) { set_error(std::string(at) + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
        if (t->bnd.bounds_set && t->bnd.bounds_C != t->C) { set_error(std::string(at) + ": the live shape changed since lpx_tableau_set_bounds"); return LPX_EINVAL; }
        int r = check_node_fits(t, at); if (r) return r;
        lds = std::max(lds, bounded_node_lds_bytes(t->R, t->C));
    }
    int r = ensure_device(); if (r) return r;
    r = bounded_primal_ready(name); if (r) return r;
    for (int i = 0; i < B; ++i) { r = bounded_primal_prepare(b->h[slot[i]]); if (r) return r; }     // steady state: nothing to do

    // ---- 2. the slab: a parameter record and a result slot per entry
    const size_t o_out = up16(sizeof(PrimalParams) * (size_t)B), need = o_out + kOut * (size_t)B;
    static_assert(sizeof(lpx_primal_record) <= kOut, "slab layout");
    r = ensure_buffers(b, need, 0, 0); if (r) return r;
    PrimalParams* P = reinterpret_cast<PrimalParams*>(b->slab);
    for (int i = 0; i < B; ++i) {
        lpx_primal_record* rec = reinterpret_cast<lpx_primal_record*>(b->slab + o_out + kOut * (size_t)i);
        std::memset(rec, 0, sizeof(*rec));
        primal_params(b->h[slot[i]], o, rec, &P[i]);
    }

    // ---- 3. behind the handles' own streams, ONE launch, ONE wait
    hipStream_t s = b->streams[0];
    r = settle_all(b); if (r) return r;
    LPX_HIP_TRY(launch_bounded_primals_onchip(P, B, lds, s));
    LPX_HIP_TRY(hipStreamSynchronize(s));

    // ---- 4. the records
    for (int i = 0; i < B; ++i) {
        const lpx_primal_record* rec = reinterpret_cast<const lpx_primal_record*>(b->slab + o_out + kOut * (size_t)i);
        primal_onchip_commit(b->h[slot[i]], rec);
        out[i] = *rec;
        rc[i] = rec->status;
    }
    return 0;
}

// The plunge: lpx_node_batch_run's steps with a chain of up to depth[i] nodes per entry (kernel: lpx_bounded_plunge.hip).  Its own:
// the checks of depth, prune and the integrality marks, the staging for max(K, 1) triples, the PlungeParams around an entry's
// parameter record, the D-strided records and `steps`.
int lpx_node_batch_plunge(lpx_node_batch* b, int B, const int32_t* slot, const int32_t* K, const int32_t* cols, const double* lower,
                          const double* upper, const lpx_run_opts* o, int flags, const double* cutoff, const double* prune,
                          const int32_t* depth, int D, int nint, const uint8_t* is_int, double tol, lpx_node_record* out,
                          int32_t* steps, int32_t* rc)
{
    const std::string w = "lpx_node_batch_plunge";
    // ---- 1. every argument of every entry, before anything is written and before any device check
    if (!slot || !K || !out || !rc || !depth || !steps || !prune) {
        set_error(w + ": null " + (!slot ? "slot" : !K ? "K" : !out ? "out" : !rc ? "rc" : !depth ? "depth" : !steps ? "steps" : "prune"));
        return LPX_EINVAL;
    }
    if (B < 1) { set_error(w + ": B is outside [1, W]"); return LPX_EINVAL; }
    if (D < 1 || D > 64) { set_error(w + ": D is outside [1, 64]"); return LPX_EINVAL; }
    { int r = check_flags_cutoff(w, B, flags, cutoff); if (r) return r; }
    for (int i = 0; i < B; ++i) {
        const std::string at = w + ": entry " + std::to_string(i);
        if (depth[i] < 1 || depth[i] > D) { set_error(at + ": depth is outside [1, D]"); return LPX_EINVAL; }
        if (prune[i] != prune[i]) { set_error(at + ": prune is NaN"); return LPX_EINVAL; }
    }
    lpx_run_opts d;
    { int r = begin_call(w, b, B, o, d); if (r) return r; }
    size_t sumK = 0, in_bytes = 0, edit_bytes = 0, lds = 0;
    char at[56];
    for (int i = 0; i < B; ++i) {
        std::snprintf(at, sizeof at, "lpx_node_batch_plunge: entry %d", i);
        lpx_tableau* t = nullptr;
        const int k = K[i];
        int r = check_entry(b, slot[i], k, cols ? cols + sumK : nullptr, lower ? lower + sumK : nullptr, upper ? upper + sumK : nullptr, o,
                            nint, tol, out, at, &t);
        if (r) return r;
        if (depth[i] > 1) {
            // a chain branches on the masked-in columns: each must be known to have finite integral bounds once this entry's own
            // triples are in place, so that lo + ub is the upper bound exactly and the ceil child is the driver's
            const std::vector<uint8_t>& whole = t->bnd.whole;
            b->colmark.assign((size_t)nint, 0);
            for (int j = 0; j < k; ++j) {
                const int c = cols[sumK + j];
                if (c >= nint) continue;
                const double lw = lower[sumK + j], up = upper[sumK + j];
                b->colmark[c] = (up < 1.0 / 0.0 && __builtin_floor(lw) == lw && __builtin_floor(up) == up) ? 1 : 2;
            }
            for (int j = 0; j < nint; ++j) {
                if (is_int && !is_int[j]) continue;
                const bool ok = b->colmark[j] ? b->colmark[j] == 1 : ((size_t)j < whole.size() && whole[j]);
                if (!ok) {
                    set_error(std::string(at) + ": depth > 1 needs finite integral bounds on every integer column; column " +
                              std::to_string(j) + " is not known to have them");
                    return LPX_EINVAL;
                }
            }
        }
        b->off_trip[i] = sumK;
        place_entry(b, i, t, k, k > 1 ? k : 1, in_bytes, edit_bytes, lds);    // the in-chain edit uses index 0 of the staging
        sumK += (size_t)k;
    }
    int r = ensure_device(); if (r) return r;
    r = bounded_plunge_ready(w.c_str()); if (r) return r;

    // ---- 2. the buffers: grown to twice the need, and only when the need outgrows them
    const size_t o_out = up16(sizeof(PlungeParams) * (size_t)B), o_steps = o_out + kOut * (size_t)B * (size_t)D,
                 o_in = o_steps + up16(sizeof(int32_t) * (size_t)B), need = o_in + in_bytes;
    r = ensure_buffers(b, need, edit_bytes, 0); if (r) return r;
    hipStream_t s = b->streams[0];
    const bool has_mask = is_int && nint > 0;
    if (has_mask) { r = ensure_mask(b, s, is_int, nint); if (r) return r; }

    // ---- 3. the slab: a parameter record, a header with its triples, D result records and a steps word per entry
    PlungeParams* P = reinterpret_cast<PlungeParams*>(b->slab);
    int32_t* nrec = reinterpret_cast<int32_t*>(b->slab + o_steps);
    const EntryOpts eo{o, flags, nint, 0, has_mask, tol};
    for (int i = 0; i < B; ++i) {
        const size_t at0 = b->off_trip[i];
        PlungeParams& q = P[i];
        std::memset(&q, 0, sizeof(q));
        fill_entry(b, i, b->h[slot[i]], K[i], cols + at0, lower + at0, upper + at0, (flags & LPX_BDUAL_CUTOFF) ? cutoff[i] : 0.0, eo,
                   reinterpret_cast<NodeIn*>(b->slab + o_in + b->off_in[i]), &q.n);
        q.n.out = reinterpret_cast<NodeOut*>(b->slab + o_out + kOut * (size_t)i * (size_t)D);
        q.prune = prune[i]; q.steps = nrec + i; q.depth = depth[i];
        nrec[i] = 0;
        for (int sx = 0; sx < D; ++sx) { std::memset(&out[(size_t)i * D + sx], 0, sizeof(out[0])); out[(size_t)i * D + sx].pick.var = -1; }
        steps[i] = 0;
    }

    // ---- 4. behind the handles' own streams, ONE launch, ONE wait
    r = settle_all(b); if (r) return r;
    LPX_HIP_TRY(launch_bounded_plunge_onchip(P, B, lds, s));
    LPX_HIP_TRY(hipStreamSynchronize(s));

    // ---- 5. the records: a chain's completed nodes in order, each as a single call would have left its handle
    bool refused = false;
    for (int i = 0; i < B; ++i) {
        lpx_tableau* t = b->h[slot[i]];
        const char* base = b->slab + o_out + kOut * (size_t)i * (size_t)D;
        int n = nrec[i];
        if (n < 1 || n > depth[i]) { set_error(w + ": entry " + std::to_string(i) + ": the kernel left no record"); return LPX_EDEVICE; }
        const NodeOut* last = reinterpret_cast<const NodeOut*>(base + kOut * (size_t)(n - 1));
        const bool ref = last->status < 0;                               // refused by the kernel: the handle is as after the node before
        const int good = ref ? n - 1 : n;
        bool any_lo = b->any_lo[i] != 0;
        for (int sx = 0; sx < good; ++sx) {
            const NodeOut* rec = reinterpret_cast<const NodeOut*>(base + kOut * (size_t)sx);
            if (sx > 0) {                                                // the ceil child's lower bound, as the kernel formed it
                const NodeOut* prev = reinterpret_cast<const NodeOut*>(base + kOut * (size_t)(sx - 1));
                if (std::ceil(prev->x_var) != 0.0) any_lo = true;
            }
            node_onchip_commit(t, rec, any_lo, &out[(size_t)i * D + sx]);
        }
        if (good > 0 && K[i] > 0) bounds_note_edit(t, K[i], cols + b->off_trip[i], lower + b->off_trip[i], upper + b->off_trip[i]);
        steps[i] = good;
        if (ref) {
            rc[i] = LPX_EINVAL;
            out[(size_t)i * D + good].unrepairable = last->unrepairable;
            if (!refused) set_refusal(w + ": entry " + std::to_string(i) + (good > 0 ? ": node " + std::to_string(good) : std::string()), last);
            refused = true;
            continue;
        }
        rc[i] = last->status;
    }
    return 0;
}

}  // extern "C"
