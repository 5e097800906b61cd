// lpx_tableau_bounded.cpp -- host side of the bounded-variable family on a tableau handle (C ABI of include/lpx.h): bounds beside
// the tableau, the bounded primal and dual loops, bound changes on a solved tableau, branch and bound by bound changes.
// Kernels: lpx_bounded.hip, lpx_bounded_dual.hip, lpx_bounded_long.hip (their shared pieces: lpx_bounded.h), lpx_bnb_bounded.hip;
// the update is lpx_update.  The on-chip forms: the node (lpx_bounded_node.hip and its siblings) and the primal loop
// (lpx_bounded_run2, lpx_bounded_primal.hip).  The cut round on a handle with bounds and the cut loop at a bounded root
// (lpx_tableau_gmi_round_bounded, lpx_bounded_cut_loop; the round and its kernels: lpx_cuts.hip).
#include "lpx_handle.h"

#include <cstring>
#include <mutex>
#include <vector>

using namespace lpx;

int lpx::bounds_snapshot(lpx_tableau* t)
{
    lpx_tableau::Bounds& b = t->bnd;
    b.snap_bounds = b.bounds_set; b.snap_bounds_C = b.bounds_C;
    if (!b.bounds_set) return 0;
    if (!b.snapUb) {
        LPX_HIP_TRY(hipMalloc((void**)&b.snapUb, sizeof(double) * t->Ccap));
        LPX_HIP_TRY(hipMalloc((void**)&b.snapFlip, t->Ccap));
        LPX_HIP_TRY(hipMalloc((void**)&b.snapLo, sizeof(double) * t->Ccap));
    }
    LPX_HIP_TRY(hipMemcpyAsync(b.snapLo, b.lo, sizeof(double) * t->Ccap, hipMemcpyDeviceToDevice, t->stream));
    b.snap_lo_used = b.lo_used; b.snap_whole = b.whole;
    LPX_HIP_TRY(hipMemcpyAsync(b.snapUb, b.ub, sizeof(double) * t->Ccap, hipMemcpyDeviceToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(b.snapFlip, b.flip, t->Ccap, hipMemcpyDeviceToDevice, t->stream));
    return 0;
}

int lpx::bounds_restore(lpx_tableau* t)
{
    lpx_tableau::Bounds& b = t->bnd;
    if (b.snap_bounds) {
        LPX_HIP_TRY(hipMemcpyAsync(b.ub, b.snapUb, sizeof(double) * t->Ccap, hipMemcpyDeviceToDevice, t->stream));
        LPX_HIP_TRY(hipMemcpyAsync(b.flip, b.snapFlip, t->Ccap, hipMemcpyDeviceToDevice, t->stream));
        LPX_HIP_TRY(hipMemcpyAsync(b.lo, b.snapLo, sizeof(double) * t->Ccap, hipMemcpyDeviceToDevice, t->stream));
        b.bounds_set = true; b.bounds_C = b.snap_bounds_C; b.lo_used = b.snap_lo_used; b.whole = b.snap_whole;
    } else if (b.bounds_set) {      // snapshotted before it had bounds: that tableau had no column flipped or shifted
        LPX_HIP_TRY(hipMemsetAsync(b.flip, 0, t->Ccap, t->stream));
        LPX_HIP_TRY(hipMemsetAsync(b.lo, 0, sizeof(double) * t->Ccap, t->stream));
        b.lo_used = false; b.whole.clear();
    }
    return 0;
}

int lpx::bounds_clone(const lpx_tableau* src, lpx_tableau* dst)
{
    const lpx_tableau::Bounds& a = src->bnd;
    lpx_tableau::Bounds& b = dst->bnd;
    if (!a.bounds_set) return 0;
    LPX_HIP_TRY(hipMalloc((void**)&b.ub, sizeof(double) * dst->Ccap));
    LPX_HIP_TRY(hipMalloc((void**)&b.flip, dst->Ccap));
    LPX_HIP_TRY(hipMalloc((void**)&b.lo, sizeof(double) * dst->Ccap));
    LPX_HIP_TRY(hipMemcpyAsync(b.ub, a.ub, sizeof(double) * dst->Ccap, hipMemcpyDeviceToDevice, dst->stream));
    LPX_HIP_TRY(hipMemcpyAsync(b.flip, a.flip, dst->Ccap, hipMemcpyDeviceToDevice, dst->stream));
    LPX_HIP_TRY(hipMemcpyAsync(b.lo, a.lo, sizeof(double) * dst->Ccap, hipMemcpyDeviceToDevice, dst->stream));
    b.bounds_set = true; b.bounds_C = a.bounds_C; b.lo_used = a.lo_used; b.whole = a.whole;
    return 0;
}

namespace {

// pinned slab: {int32 cnt[2], pad} at 0, lpx_branch_pick at 16
struct NodeSlab { int32_t cnt[4]; lpx_branch_pick pick; };

int bound_buffers(lpx_tableau* t)
{
    if (t->bnd.ub) return 0;
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.ub, sizeof(double) * t->Ccap));
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.flip, t->Ccap));
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.lo, sizeof(double) * t->Ccap));
    return 0;
}

int node_buffers(lpx_tableau* t)
{
    if (t->bnd.dzl) return 0;
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.dzl, sizeof(int32_t) * ((size_t)t->Ccap + 4)));
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.pickrec, sizeof(lpx_branch_pick)));
    LPX_HIP_TRY(hipMalloc((void**)&t->bnd.pickmask, (size_t)t->Ccap));
    LPX_HIP_TRY(hipHostMalloc((void**)&t->bnd.nodeslab, sizeof(NodeSlab)));
    return 0;
}

// every live column unbounded, unflipped and unshifted (a handle without bounds)
int bounds_fill_inf(lpx_tableau* t)
{
    std::vector<double> inf((size_t)t->Ccap, 1.0 / 0.0);
    LPX_HIP_TRY(hipMemcpyAsync(t->bnd.ub, inf.data(), sizeof(double) * t->Ccap, hipMemcpyHostToDevice, t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->bnd.flip, 0, t->Ccap, t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->bnd.lo, 0, sizeof(double) * t->Ccap, t->stream));      // +0.0
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    t->bnd.lo_used = false; t->bnd.whole.clear();
    return 0;
}

// the device, the bound arrays the loops read (without bounds: every column unbounded) and, with node, the buffers of dualize / pick / node
int bounded_ready(lpx_tableau* t, bool node)
{
    int rc = ensure_device(); if (rc) return rc;
    rc = bound_buffers(t); if (rc) return rc;
    if (!t->bnd.bounds_set) { rc = bounds_fill_inf(t); if (rc) return rc; }
    return node ? node_buffers(t) : 0;
}

// bounds present (unless the entry point runs without them) and set for the live shape: LPX_EINVAL with `what` in front otherwise
int check_bounds(const lpx_tableau* t, const char* what, bool required)
{
    const std::string w = what;
    if (!t->bnd.bounds_set && !required) return 0;
    if (!t->bnd.bounds_set) { set_error(w + ": the handle has no bounds (lpx_tableau_set_bounds first)"); return LPX_EINVAL; }
    if (t->bnd.bounds_C != t->C) { set_error(w + ": the live shape changed since lpx_tableau_set_bounds"); return LPX_EINVAL; }
    return 0;
}

}  // namespace

// the argument checks of lpx_tableau_change_bounds (lpx_bounded_node makes the same ones): LPX_EINVAL with `what` in front
int lpx::check_change_args(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const char* what)
{
    const std::string w = what;
    if (!t) { set_error(w + ": null handle"); return LPX_EINVAL; }
    if (K < 0) { set_error(w + ": K is negative"); return LPX_EINVAL; }
    if (K > 0 && (!cols || !lower || !upper)) { set_error(w + ": null array"); return LPX_EINVAL; }
    const int Cm = t->C - 1;
    std::vector<uint8_t> seen((size_t)(Cm > 0 ? Cm : 1), 0);
    for (int k = 0; k < K; ++k) {
        const std::string at = "[" + std::to_string(k) + "]";
        if (cols[k] < 0 || cols[k] >= Cm) { set_error(w + ": cols" + at + " is outside [0, C-1)"); return LPX_EINVAL; }
        if (seen[cols[k]]) { set_error(w + ": cols" + at + " repeats a column"); return LPX_EINVAL; }
        seen[cols[k]] = 1;
        if (lower[k] != lower[k] || upper[k] != upper[k]) { set_error(w + ": bound" + at + " is NaN"); return LPX_EINVAL; }
        if (lower[k] == 1.0 / 0.0 || lower[k] == -1.0 / 0.0) { set_error(w + ": lower" + at + " is not finite"); return LPX_EINVAL; }
        if (upper[k] < lower[k]) { set_error(w + ": upper" + at + " is below lower" + at); return LPX_EINVAL; }
    }
    return check_bounds(t, what, true);
}

int lpx::check_pick_args(lpx_tableau* t, int nint, double tol, const void* out, const char* what)
{
    const std::string w = what;
    if (!t) { set_error(w + ": null handle"); return LPX_EINVAL; }
    if (!out) { set_error(w + ": null out"); return LPX_EINVAL; }
    if (nint < 0 || nint > t->C - 1) { set_error(w + ": nint is outside [0, C-1]"); return LPX_EINVAL; }
    if (!(tol >= 0.0 && tol < 0.5)) { set_error(w + ": tol is not in [0, 0.5)"); return LPX_EINVAL; }
    return 0;
}

namespace {

// One bound edit staged on the device: the caller's arrays in the handle's staging buffer, one layout for every entry point --
// lower, upper, shift, the saved (ub, lo) pairs, cols ([K] each, save [2K]; lpx_tableau_change_bounds leaves the save area unused).
struct BoundEdit { double *lower = nullptr, *upper = nullptr, *shift = nullptr, *save = nullptr; int32_t* cols = nullptr; bool any_lo = false; };

// Refuses +inf on a flipped column (the flip lives on the device; unflipping is not part of an edit), grows the staging buffer
// and enqueues the three copies.  It waits for the handle's stream only before it reads the flips or frees the old buffer.
int stage_bound_edit(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const char* what, BoundEdit* e)
{
    const int Cm = t->C - 1;
    bool any_inf = false;
    for (int k = 0; k < K; ++k) { if (upper[k] == 1.0 / 0.0) any_inf = true; if (lower[k] != 0.0) e->any_lo = true; }
    if (any_inf) {
        std::vector<uint8_t> flip((size_t)Cm);
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        LPX_HIP_TRY(hipMemcpy(flip.data(), t->bnd.flip, Cm, hipMemcpyDeviceToHost));
        for (int k = 0; k < K; ++k)
            if (upper[k] == 1.0 / 0.0 && flip[cols[k]]) {
                set_error(std::string(what) + ": upper[" + std::to_string(k) + "] = +inf on a flipped column");
                return LPX_EINVAL;
            }
    }
    if (K == 0) return 0;
    const size_t need = (size_t)K * (5 * sizeof(double) + sizeof(int32_t));
    if (need > t->bnd.chg_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        hipFree(t->bnd.chg); t->bnd.chg = nullptr; t->bnd.chg_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&t->bnd.chg, 2 * need));
        t->bnd.chg_bytes = 2 * need;
    }
    e->lower = reinterpret_cast<double*>(t->bnd.chg);
    e->upper = e->lower + K; e->shift = e->upper + K; e->save = e->shift + K;
    e->cols = reinterpret_cast<int32_t*>(e->save + 2 * (size_t)K);
    LPX_HIP_TRY(hipMemcpyAsync(e->lower, lower, sizeof(double) * K, hipMemcpyHostToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(e->upper, upper, sizeof(double) * K, hipMemcpyHostToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(e->cols, cols, sizeof(int32_t) * K, hipMemcpyHostToDevice, t->stream));
    return 0;
}

// The bounded loops in one body: dual = 0 is lpx_bounded_run, 1 + flags the dual loop with that set of LPX_BDUAL_* flags
// (lpx_bounded_dual_run is 1).  The value goes into the parameter record (BndParams::dual), so that every form selects its own
// kernel and keys its own cached graph.
int bounded_run(lpx_tableau* t, const lpx_run_opts* o, int dual, lpx_pivot_cb cb, void* user, lpx_stats* st, double cutoff = 0.0,
                const char* name = nullptr)         // name: the entry point in front of the messages where it is not the form's own
{
    const int flags = dual ? dual - 1 : 0;
    const bool lng = flags & (LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF);      // passes and LPX_CUTOFF exist only in these forms
    const std::string w = name ? name : lng ? "lpx_bounded_dual_run3" : dual ? "lpx_bounded_dual_run" : "lpx_bounded_run";
    if (!t) { set_error(w + ": null tableau"); return LPX_EINVAL; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, dual ? 1 : 0); o = &d; }
    if (t->R < 2) { set_error(w + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    if (o->resident > 0) { set_error(w + ": there is no resident form of the bounded " + (dual ? "dual loop" : "loop")); return LPX_EINVAL; }
    int rc = check_bounds(t, w.c_str(), false); if (rc) return rc;
    rc = bounded_ready(t, false); if (rc) return rc;
    BndParams b; std::memset(&b, 0, sizeof(b));
    b.P = base_params(t, o, MODE_BOUNDED);
    b.P.us = nullptr; b.P.part_v = nullptr; b.P.part_i = nullptr; b.P.nblk = 0; b.P.qsel = 0;   // single-workgroup select
    b.ub = t->bnd.ub; b.flip = t->bnd.flip; b.dual = dual;
    if (flags & LPX_BDUAL_CUTOFF) {
        // the value travels beside the parameter record: copied on the handle's stream in front of the run, read through a pointer
        if (!t->bnd.cutoff) LPX_HIP_TRY(hipMalloc((void**)&t->bnd.cutoff, sizeof(double)));
        t->bnd.cutoff_h = cutoff;
        LPX_HIP_TRY(hipMemcpyAsync(t->bnd.cutoff, &t->bnd.cutoff_h, sizeof(double), hipMemcpyHostToDevice, t->stream));
        b.cutoff = t->bnd.cutoff;
    }
    LoopCtx c; DevState init;
    make_ctx(t, b.P, b, [b](hipStream_t s, hipEvent_t e0, hipEvent_t e1) -> int {
        if (b.dual) LPX_HIP_TRY(launch_bounded_dual_select(b, s));
        else LPX_HIP_TRY(launch_bounded_select(b, s));
        // a launch that ended on a flip or on a final status leaves nothing to update: lpx_update returns at once
        LPX_HIP_TRY(launch_update(b.P, b.P.pcol, b.P.pcol, s, e0, e1));
        return 0;
    }, c, init);
    lpx_stats local; std::memset(&local, 0, sizeof(local));
    int64_t* n = t->bnd.bcounts;
    n[0] = n[1] = n[2] = 0;
    rc = run_device_loop(c, init, o, (long long)o->max_iter + 2, cb, user, &local);
    if (rc < 0) return rc;
    // the select kernel counts the pivots per kind in the two counters the dual path uses for its phases; the other events are the
    // flips of the primal loop and the passes of the long step
    n[0] = t->hst->fdf_count; n[1] = t->hst->dual_iter;
    if (!dual || lng) n[2] = (int64_t)t->hst->iter - n[0] - n[1];
    local.pivots = n[0] + n[1]; local.fdf_pivots = 0; local.cleanup_pivots = 0;
    if (st) { const double h2d = st->h2d_ms, d2h = st->d2h_ms; *st = local; st->h2d_ms = h2d; st->d2h_ms = d2h; }
    return rc;
}

// the two dualize launches; the counts stay on the device behind the list
int enqueue_dualize_list(lpx_tableau* t, double eps)
{
    LPX_HIP_TRY(launch_dualize_list(t->T, t->ld, t->R, t->C - 1, t->bnd.ub, eps, t->bnd.dzl + 4, t->bnd.dzl, t->stream));
    return 0;
}
int enqueue_dualize_apply(lpx_tableau* t)
{
    LPX_HIP_TRY(launch_dualize_apply(t->T, t->ld, t->R, t->C - 1, t->bnd.ub, t->bnd.flip, t->bnd.dzl + 4, t->bnd.dzl, t->rhsbuf, t->stream));
    return 0;
}

// the pick launch and the copy of its record into the pinned slab (the caller waits)
int enqueue_pick(lpx_tableau* t, int nint, const uint8_t* is_int, double tol)
{
    if (is_int && nint > 0) {
        LPX_HIP_TRY(hipMemcpyAsync(t->bnd.pickmask, is_int, (size_t)nint, hipMemcpyHostToDevice, t->stream));
        t->bnd.mask_n = -1;                                  // the on-chip node's cached mask is gone
    }
    PickParams p; std::memset(&p, 0, sizeof(p));
    p.T = t->T; p.ld = t->ld; p.R = t->R; p.Cm = t->C - 1;
    p.basis = t->basis; p.ub = t->bnd.ub; p.flip = t->bnd.flip; p.lo = t->bnd.lo_used ? t->bnd.lo : nullptr;
    p.nint = nint; p.is_int = (is_int && nint > 0) ? t->bnd.pickmask : nullptr; p.tol = tol;
    p.ws = t->ws; p.out = t->bnd.pickrec;
    LPX_HIP_TRY(launch_branch_pick(p, t->stream));
    NodeSlab* slab = reinterpret_cast<NodeSlab*>(t->bnd.nodeslab);
    LPX_HIP_TRY(hipMemcpyAsync(&slab->pick, t->bnd.pickrec, sizeof(lpx_branch_pick), hipMemcpyDeviceToHost, t->stream));
    return 0;
}

}  // namespace

int lpx::check_long_flags(int flags, double cutoff, const char* what)
{
    if (flags & ~(LPX_BDUAL_SKIP_FIXED | LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF)) { set_error(std::string(what) + ": unknown flag"); return LPX_EINVAL; }
    if ((flags & LPX_BDUAL_CUTOFF) && cutoff != cutoff) { set_error(std::string(what) + ": cutoff is NaN"); return LPX_EINVAL; }
    return 0;
}

// the option checks of a node call, after its argument checks, and the fit of the on-chip form
int lpx::check_node_opts(const lpx_tableau* t, const lpx_run_opts* o, const char* what)
{
    const std::string w = what;
    if (t->R < 2) { set_error(w + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    if (o->resident > 0) { set_error(w + ": there is no resident form of the bounded dual loop"); return LPX_EINVAL; }
    if (!(o->eps >= 0.0)) { set_error(w + ": eps is negative or NaN"); return LPX_EINVAL; }
    return 0;
}

int lpx::check_node_fits(const lpx_tableau* t, const char* what)
{
    if (bounded_node_fits(t->R, t->C)) return 0;
    set_error(std::string(what) + ": the live " + std::to_string(t->R) + " x " + std::to_string(t->C) + " window does not fit the on-chip form "
              "(lpx_bounded_node_fits)");
    return LPX_EINVAL;
}

int lpx::bounded_node_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_node_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::bounded_plunge_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_plunge_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::bounded_guard_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_guard_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::bounded_fix_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_fix_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::check_fix_args(double fix_bound, const lpx_fix_list* fix, int nint, const char* what)
{
    const char* msg = nullptr;                          // no string is built on the way that every call of a search takes
    if (fix_bound != fix_bound) msg = ": fix_bound is NaN";
    else if (!fix) { if (fix_bound != -1.0 / 0.0) msg = ": null fix"; }
    else if (fix->cap < nint) msg = ": fix->cap is below nint";
    else if (nint > 0 && (!fix->cols || !fix->lower || !fix->upper)) msg = ": null array in fix";
    if (!msg) return 0;
    set_error(std::string(what) + msg);
    return LPX_EINVAL;
}

size_t lpx::fix_list_bytes(int nint) { return ((size_t)nint * (2 * sizeof(double) + sizeof(int32_t)) + 15) & ~(size_t)15; }

void lpx::fix_list_place(char* at, int nint, FixParams* p)
{
    p->upper = reinterpret_cast<double*>(at);
    p->lower = p->upper + nint;
    p->cols = reinterpret_cast<int32_t*>(p->lower + nint);
}

void lpx::fix_commit(lpx_tableau* t, int n, const FixParams& p, lpx_fix_list* fix)
{
    fix->n = n;
    if (n <= 0) return;
    std::memcpy(fix->cols, p.cols, sizeof(int32_t) * (size_t)n);
    std::memcpy(fix->lower, p.lower, sizeof(double) * (size_t)n);
    std::memcpy(fix->upper, p.upper, sizeof(double) * (size_t)n);
    for (int k = 0; k < n; ++k) if (fix->lower[k] != 0.0) t->bnd.lo_used = true;
    bounds_note_edit(t, n, fix->cols, fix->lower, fix->upper);
}

int lpx::bounded_probe_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_probe_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::bounded_primal_ready(const char* what)
{
    static std::once_flag once; static hipError_t init_err = hipSuccess;
    std::call_once(once, [] { init_err = bounded_primal_init(); });
    if (init_err != hipSuccess) { set_error(std::string(what) + ": kernel attribute setup failed: " + hipGetErrorString(init_err)); return LPX_EDEVICE; }
    return 0;
}

int lpx::bounded_primal_prepare(lpx_tableau* t) { return bounded_ready(t, false); }

void lpx::primal_params(lpx_tableau* t, const lpx_run_opts* o, lpx_primal_record* rec, PrimalParams* n)
{
    std::memset(n, 0, sizeof(*n));
    n->T = t->T; n->ld = t->ld; n->R = t->R; n->C = t->C;
    n->rhsbuf = t->rhsbuf; n->basis = t->basis; n->trace = t->trace; n->trace_cap = t->trace_cap; n->st = t->st;
    n->ub = t->bnd.ub; n->flip = t->bnd.flip;
    n->eps = o->eps; n->ratio_tol = o->ratio_tol; n->max_iter = o->max_iter;
    n->out = rec;
}

void lpx::primal_onchip_commit(lpx_tableau* t, const lpx_primal_record* rec)
{
    t->trace_void = false;                  // the loop ran and wrote its trace
    DevState h = fresh_state(false);        // the host mirror, as the loop of the launches form leaves it
    h.status = rec->status; h.iter = rec->events; h.fdf_count = (int)rec->kind0; h.dual_iter = (int)rec->kind1; h.primal_count = rec->events;
    *t->hst = h;
    t->bnd.bcounts[0] = rec->kind0; t->bnd.bcounts[1] = rec->kind1; t->bnd.bcounts[2] = rec->flips;
}

int lpx::check_probe_args(int cand_max, int probe_iter, const char* what)
{
    if (cand_max < 1 || cand_max > 32) { set_error(std::string(what) + ": cand_max is outside [1, 32]"); return LPX_EINVAL; }
    if (probe_iter < 0) { set_error(std::string(what) + ": probe_iter is negative"); return LPX_EINVAL; }
    return 0;
}

namespace {
size_t probe_basis_stride(const lpx_tableau* t) { return ((size_t)(t->R - 1) + 3) & ~(size_t)3; }       // int32 words, 16-byte slices
size_t probe_flip_stride(const lpx_tableau* t) { return ((size_t)(t->C - 1) + 15) & ~(size_t)15; }      // bytes
}  // namespace

size_t lpx::probe_ws_bytes(const lpx_tableau* t, int cand_max)
{
    return 2 * (size_t)cand_max * (sizeof(int32_t) * probe_basis_stride(t) + probe_flip_stride(t));
}

void lpx::probe_params(const lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, double prune, int nint,
                       const uint8_t* mask_dev, double tol, int cand_max, int probe_iter, bool lo_used, char* ws, const NodeOut* front,
                       lpx_probe_head* head, lpx_probe_record* rec, ProbeParams* p)
{
    std::memset(p, 0, sizeof(*p));
    p->T = t->T; p->ld = t->ld; p->R = t->R; p->C = t->C;
    p->basis = t->basis; p->st = t->st; p->ub = t->bnd.ub; p->lo = t->bnd.lo; p->flip = t->bnd.flip;
    p->mask = mask_dev; p->front = front;
    p->wbasis = reinterpret_cast<int32_t*>(ws); p->wbasis_stride = (int32_t)probe_basis_stride(t);
    p->wflip = reinterpret_cast<uint8_t*>(ws + 2 * (size_t)cand_max * sizeof(int32_t) * probe_basis_stride(t));
    p->wflip_stride = (int32_t)probe_flip_stride(t);
    p->head = head; p->rec = rec;
    p->eps = o->eps; p->ratio_tol = o->ratio_tol; p->cutoff = (flags & LPX_BDUAL_CUTOFF) ? cutoff : 0.0; p->tol = tol; p->prune = prune;
    p->flags = flags; p->nint = nint; p->has_mask = mask_dev && nint > 0 ? 1 : 0; p->lo_used = lo_used ? 1 : 0;
    p->probe_iter = probe_iter; p->cand_max = cand_max;
    head->count = 0; head->candidates = 0; head->z = 0.0;
    for (int w = 0; w < 2 * cand_max; ++w) { std::memset(&rec[w], 0, sizeof(rec[w])); rec[w].status = LPX_PROBE_NONE; rec[w].var = -1; rec[w].dir = w & 1; }
}

void lpx::bounds_note_edit(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper)
{
    std::vector<uint8_t>& w = t->bnd.whole;
    if (w.empty()) return;                  // nothing is known about this handle's columns: an edit of some of them changes nothing
    for (int k = 0; k < K; ++k)
        if ((size_t)cols[k] < w.size())
            w[cols[k]] = (upper[k] < 1.0 / 0.0 && __builtin_floor(lower[k]) == lower[k] && __builtin_floor(upper[k]) == upper[k]) ? 1 : 0;
}

void lpx::node_onchip_commit(lpx_tableau* t, const NodeOut* rec, bool any_lo, lpx_node_record* out)
{
    lpx_tableau::Bounds& b = t->bnd;
    t->suspended = t->suspended2 = t->fsuspended = false;
    t->trace_void = false;                  // the node ran and wrote its trace; a refused one leaves a clone's mark standing
    if (any_lo) b.lo_used = true;
    DevState h = fresh_state(false);                                             // the host mirror, as the loop of the launches form leaves it
    h.status = rec->status; h.iter = rec->events; h.fdf_count = rec->kind0; h.dual_iter = rec->kind1; h.primal_count = rec->events;
    *t->hst = h;
    b.bcounts[0] = rec->kind0; b.bcounts[1] = rec->kind1; b.bcounts[2] = (int64_t)rec->events - rec->kind0 - rec->kind1;
    out->status = rec->status; out->events = rec->events; out->kind0 = rec->kind0; out->kind1 = rec->kind1; out->flips = rec->flips;
    out->pick.z = rec->z;
    if (rec->status == LPX_OPTIMAL) { out->pick.var = rec->var; out->pick.candidates = rec->candidates; out->pick.x_var = rec->x_var; }
}

extern "C" {

// ---- bounded-variable primal and dual simplex (select kernels in lpx_bounded.hip / lpx_bounded_dual.hip / lpx_bounded_long.hip, update = lpx_update) ----
int lpx_tableau_set_bounds(lpx_tableau* t, int ncols, const double* ub)
{
    if (!t) { set_error("lpx_tableau_set_bounds: null handle"); return LPX_EINVAL; }
    if (!ub && ncols == 0) { t->bnd.bounds_set = false; t->bnd.bounds_C = 0; t->bnd.whole.clear(); return 0; }
    if (!ub || ncols != t->C - 1) { set_error("lpx_tableau_set_bounds: ncols must be the live C - 1 and ub non-null"); return LPX_EINVAL; }
    for (int j = 0; j < ncols; ++j)
        if (!(ub[j] >= 0.0)) { set_error("lpx_tableau_set_bounds: ub[" + std::to_string(j) + "] is negative or NaN"); return LPX_EINVAL; }
    int rc = ensure_device(); if (rc) return rc;
    rc = bound_buffers(t); if (rc) return rc;
    rc = bounds_fill_inf(t); if (rc) return rc;            // columns beyond the live shape: unbounded; every flip cleared
    LPX_HIP_TRY(hipMemcpy(t->bnd.ub, ub, sizeof(double) * ncols, hipMemcpyHostToDevice));
    t->bnd.bounds_set = true; t->bnd.bounds_C = t->C;
    t->bnd.whole.assign((size_t)ncols, 0);                 // lo is zero everywhere: a column is whole iff its ub is finite and integral
    for (int j = 0; j < ncols; ++j) t->bnd.whole[j] = (ub[j] < 1.0 / 0.0 && __builtin_floor(ub[j]) == ub[j]) ? 1 : 0;
    return 0;
}

int lpx_bounded_counts(lpx_tableau* t, int64_t counts[3])
{
    if (!t || !counts) { set_error("lpx_bounded_counts: null argument"); return LPX_EINVAL; }
    for (int k = 0; k < 3; ++k) counts[k] = t->bnd.bcounts[k];
    return 0;
}

int lpx_bounded_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st) { return bounded_run(t, o, 0, cb, user, st); }
int lpx_bounded_dual_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st) { return bounded_run(t, o, 1, cb, user, st); }

// The bounded primal loop with its form (kernels of the on-chip form: lpx_bounded_primal.hip).  On chip the steady state of a
// call is: the parameter record formed, one kernel launch, one wait, the record read from the handle's pinned slab.
int lpx_bounded_run2(lpx_tableau* t, const lpx_run_opts* o, int form, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    const char* what = "lpx_bounded_run2";
    const std::string w = what;
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error(w + ": unknown form"); return LPX_EINVAL; }
    if (form == LPX_NODE_LAUNCHES || (form == LPX_NODE_AUTO && (!t || cb || !bounded_node_fits(t->R, t->C))))
        return bounded_run(t, o, 0, cb, user, st, 0.0, what);
    if (!t) { set_error(w + ": null tableau"); return LPX_EINVAL; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 0); o = &d; }
    if (t->R < 2) { set_error(w + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    if (o->resident > 0) { set_error(w + ": there is no resident form of the bounded loop"); return LPX_EINVAL; }
    int rc = check_bounds(t, what, false); if (rc) return rc;
    if (cb) { set_error(w + ": the on-chip form has no per-event callback"); return LPX_EINVAL; }
    rc = check_node_fits(t, what); if (rc) return rc;
    rc = bounded_ready(t, false); if (rc) return rc;
    rc = bounded_primal_ready(what); if (rc) return rc;
    lpx_tableau::Bounds& b = t->bnd;
    constexpr size_t kOut = 64;
    static_assert(sizeof(lpx_primal_record) <= kOut, "slab layout");
    if (kOut > b.nodeio_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        if (b.nodeio) hipHostFree(b.nodeio);
        b.nodeio = nullptr; b.nodeio_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&b.nodeio, 2 * kOut));
        b.nodeio_bytes = 2 * kOut;
    }
    lpx_primal_record* rec = reinterpret_cast<lpx_primal_record*>(b.nodeio);
    PrimalParams n;
    primal_params(t, o, rec, &n);
    const double t0 = now_ms();
    LPX_HIP_TRY(launch_bounded_primal_onchip(n, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));                                // the one wait: the record is in the slab
    primal_onchip_commit(t, rec);
    if (st) {
        const double h2d = st->h2d_ms, d2h = st->d2h_ms;
        std::memset(st, 0, sizeof(*st));
        st->h2d_ms = h2d; st->d2h_ms = d2h;
        st->pivots = rec->kind0 + rec->kind1; st->loop_ms = now_ms() - t0; st->launches = 1;
    }
    return rec->status;
}

int lpx_bounded_dual_run2(lpx_tableau* t, const lpx_run_opts* o, int flags, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    if (flags & ~LPX_BDUAL_SKIP_FIXED) { set_error("lpx_bounded_dual_run2: unknown flag"); return LPX_EINVAL; }
    return bounded_run(t, o, 1 + flags, cb, user, st);
}

int lpx_tableau_bounded_solution(lpx_tableau* t, int nvars, double* x, double* z, uint8_t* at_upper)
{
    if (!t || nvars < 0 || nvars > t->C - 1 || (nvars > 0 && !x)) { set_error("lpx_tableau_bounded_solution: bad argument"); return LPX_EINVAL; }
    { int rc = check_bounds(t, "lpx_tableau_bounded_solution", false); if (rc) return rc; }
    const int m = t->R - 1, Cm = t->C - 1;
    std::vector<double> rhs(t->R), ub(Cm, 1.0 / 0.0);
    std::vector<int32_t> basis(m > 0 ? m : 1);
    std::vector<uint8_t> flip(Cm, 0);
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    LPX_HIP_TRY(hipMemcpy2D(rhs.data(), sizeof(double), t->T + Cm, sizeof(double) * t->ld, sizeof(double), t->R, hipMemcpyDeviceToHost));
    if (m > 0) LPX_HIP_TRY(hipMemcpy(basis.data(), t->basis, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    if (t->bnd.bounds_set && Cm > 0) {
        LPX_HIP_TRY(hipMemcpy(ub.data(), t->bnd.ub, sizeof(double) * Cm, hipMemcpyDeviceToHost));
        LPX_HIP_TRY(hipMemcpy(flip.data(), t->bnd.flip, Cm, hipMemcpyDeviceToHost));
    }
    std::vector<double> lo;                             // only where a bound change has stored a non-zero lower shift
    if (t->bnd.bounds_set && t->bnd.lo_used && Cm > 0) {
        lo.resize(Cm);
        LPX_HIP_TRY(hipMemcpy(lo.data(), t->bnd.lo, sizeof(double) * Cm, hipMemcpyDeviceToHost));
    }
    std::vector<double> v(Cm, 0.0);
    std::vector<uint8_t> basic(Cm, 0);
    for (int i = 0; i < m; ++i) if (basis[i] >= 0 && basis[i] < Cm) { v[basis[i]] = rhs[i]; basic[basis[i]] = 1; }
    for (int j = 0; j < nvars; ++j) {
        x[j] = flip[j] ? ub[j] - v[j] : v[j];
        if (!lo.empty()) x[j] = x[j] + lo[j];
        if (at_upper) at_upper[j] = (flip[j] && !basic[j]) ? 1 : 0;
    }
    if (z) *z = rhs[m];
    return 0;
}

// lo, ub and flip of the live columns (each optional); a handle without bounds: unshifted, unbounded, unflipped
static int bound_state(lpx_tableau* t, double* lo, double* ub, uint8_t* flip, const char* what)
{
    const int n = t->C - 1;
    if (!t->bnd.bounds_set || !t->bnd.ub) {
        for (int j = 0; j < n; ++j) { if (lo) lo[j] = 0.0; if (ub) ub[j] = 1.0 / 0.0; if (flip) flip[j] = 0; }
        return 0;
    }
    { int rc = check_bounds(t, what, false); if (rc) return rc; }
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    if (lo && n > 0) LPX_HIP_TRY(hipMemcpy(lo, t->bnd.lo, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (ub && n > 0) LPX_HIP_TRY(hipMemcpy(ub, t->bnd.ub, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (flip && n > 0) LPX_HIP_TRY(hipMemcpy(flip, t->bnd.flip, n, hipMemcpyDeviceToHost));
    return 0;
}

int lpx_tableau_bound_state(lpx_tableau* t, double* lo, double* ub, uint8_t* flip)
{
    if (!t) { set_error("lpx_tableau_bound_state: null handle"); return LPX_EINVAL; }
    return bound_state(t, lo, ub, flip, "lpx_tableau_bound_state");
}

int lpx_tableau_bound_flags(lpx_tableau* t, uint8_t* flip)
{
    if (!t || !flip) { set_error("lpx_tableau_bound_flags: null argument"); return LPX_EINVAL; }
    return bound_state(t, nullptr, nullptr, flip, "lpx_tableau_bound_flags");
}

int lpx_tableau_change_bounds(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper)
{
    int rc = check_change_args(t, K, cols, lower, upper, "lpx_tableau_change_bounds"); if (rc) return rc;
    const int Cm = t->C - 1;
    rc = ensure_device(); if (rc) return rc;
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    BoundEdit e;
    rc = stage_bound_edit(t, K, cols, lower, upper, "lpx_tableau_change_bounds", &e); if (rc) return rc;
    t->suspended = t->suspended2 = t->fsuspended = false;
    if (K > 0) {
        // shift[k] from the old lo / ub / flip of cols[k], new ub / lo stored; then T[:,Cm] and rhsbuf shifted, k in order
        LPX_HIP_TRY(launch_bounds_shift(K, e.cols, e.lower, e.upper, t->bnd.ub, t->bnd.lo, t->bnd.flip, e.shift, t->stream));
        LPX_HIP_TRY(launch_bounds_apply(t->T, t->ld, t->R, Cm, K, e.cols, e.shift, t->rhsbuf, t->stream));
        if (e.any_lo) t->bnd.lo_used = true;
        bounds_note_edit(t, K, cols, lower, upper);
    }
    LPX_HIP_TRY(hipMemsetAsync(t->st, 0, sizeof(DevState), t->stream));      // the loop state, as lpx_tableau_build_child resets it
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));                            // the caller's arrays are free again
    return 0;
}

// ---- branch and bound by bound changes (kernels in lpx_bnb_bounded.hip) ----
int lpx_tableau_dualize(lpx_tableau* t, double eps, int64_t counts[2])
{
    if (!t) { set_error("lpx_tableau_dualize: null handle"); return LPX_EINVAL; }
    if (!counts) { set_error("lpx_tableau_dualize: null counts"); return LPX_EINVAL; }
    if (!(eps >= 0.0)) { set_error("lpx_tableau_dualize: eps is negative or NaN"); return LPX_EINVAL; }
    int rc = check_bounds(t, "lpx_tableau_dualize", true); if (rc) return rc;
    if (t->R < 1 || t->C < 1) { set_error("lpx_tableau_dualize: empty tableau"); return LPX_EINVAL; }
    rc = bounded_ready(t, true); if (rc) return rc;
    t->suspended = t->suspended2 = t->fsuspended = false;
    rc = enqueue_dualize_list(t, eps); if (rc) return rc;
    rc = enqueue_dualize_apply(t); if (rc) return rc;
    NodeSlab* slab = reinterpret_cast<NodeSlab*>(t->bnd.nodeslab);
    LPX_HIP_TRY(hipMemcpyAsync(slab->cnt, t->bnd.dzl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    counts[0] = slab->cnt[0]; counts[1] = slab->cnt[1];
    return 0;
}

int lpx_tableau_branch_pick(lpx_tableau* t, int nint, const uint8_t* is_int, double tol, lpx_branch_pick* out)
{
    int rc = check_pick_args(t, nint, tol, out, "lpx_tableau_branch_pick"); if (rc) return rc;
    rc = check_bounds(t, "lpx_tableau_branch_pick", false); if (rc) return rc;
    if (t->R < 1 || t->C < 1) { set_error("lpx_tableau_branch_pick: empty tableau"); return LPX_EINVAL; }
    rc = bounded_ready(t, true); if (rc) return rc;
    rc = enqueue_pick(t, nint, is_int, tol); if (rc) return rc;
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    *out = reinterpret_cast<NodeSlab*>(t->bnd.nodeslab)->pick;
    return 0;
}

// lpx_bounded_node (flags = LPX_BDUAL_SKIP_FIXED) and lpx_bounded_node2 in one body; `what` is the entry point's name
static int bounded_node(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                        int flags, double cutoff, int nint, const uint8_t* is_int, double tol, lpx_node_record* out, const char* what)
{
    const std::string w = what;
    int rc = check_change_args(t, K, cols, lower, upper, what); if (rc) return rc;
    rc = check_pick_args(t, nint, tol, out, what); if (rc) return rc;
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    if (t->R < 2) { set_error(w + ": tableau needs at least one constraint row"); return LPX_EINVAL; }
    if (o->resident > 0) { set_error(w + ": there is no resident form of the bounded dual loop"); return LPX_EINVAL; }
    if (!(o->eps >= 0.0)) { set_error(w + ": eps is negative or NaN"); return LPX_EINVAL; }
    const int Cm = t->C - 1;
    rc = bounded_ready(t, true); if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    out->pick.var = -1;
    BoundEdit e;
    rc = stage_bound_edit(t, K, cols, lower, upper, what, &e); if (rc) return rc;
    if (K > 0) {
        // the new ub and lo first (small arrays only): the list of the flips needs them, and the tableau is still untouched
        LPX_HIP_TRY(launch_bounds_save(K, e.cols, t->bnd.ub, t->bnd.lo, e.save, 0, t->stream));
        LPX_HIP_TRY(launch_bounds_shift(K, e.cols, e.lower, e.upper, t->bnd.ub, t->bnd.lo, t->bnd.flip, e.shift, t->stream));
    }
    // the list reads the objective row left of the RHS, which the RHS shift of the edit does not write: listing before that
    // shift gives the list of listing after it, and an unrepairable column is found with the tableau as it was
    rc = enqueue_dualize_list(t, o->eps); if (rc) return rc;
    NodeSlab* slab = reinterpret_cast<NodeSlab*>(t->bnd.nodeslab);
    LPX_HIP_TRY(hipMemcpyAsync(slab->cnt, t->bnd.dzl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream));
    // wait 1: the counts (the caller's arrays are free again)
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    out->flips = slab->cnt[0]; out->unrepairable = slab->cnt[1];
    if (out->unrepairable > 0) {
        LPX_HIP_TRY(launch_bounds_save(K, e.cols, t->bnd.ub, t->bnd.lo, e.save, 1, t->stream));     // ub and lo as they were
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        out->flips = 0;
        set_error(w + ": " + std::to_string(out->unrepairable) + " column(s) with a negative reduced cost and no upper "
                  "bound: a bound flip cannot restore dual feasibility");
        return LPX_EINVAL;
    }
    t->suspended = t->suspended2 = t->fsuspended = false;
    if (e.any_lo) t->bnd.lo_used = true;
    bounds_note_edit(t, K, cols, lower, upper);
    if (K > 0) LPX_HIP_TRY(launch_bounds_apply(t->T, t->ld, t->R, Cm, K, e.cols, e.shift, t->rhsbuf, t->stream));
    rc = enqueue_dualize_apply(t); if (rc) return rc;
    // the loop (it resets the state record itself and waits once per batch)
    const int status = bounded_run(t, o, 1 + flags, nullptr, nullptr, nullptr, cutoff);
    if (status < 0) return status;
    out->status = status; out->events = t->hst->iter; out->kind0 = t->bnd.bcounts[0]; out->kind1 = t->bnd.bcounts[1];
    if (status == LPX_OPTIMAL) {
        rc = enqueue_pick(t, nint, is_int, tol); if (rc) return rc;
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));                                    // last wait: the pick record
        out->pick = slab->pick;
    } else {
        // no pick: z as the tableau stands, through the same slab
        LPX_HIP_TRY(hipMemcpyAsync(&slab->pick.z, t->T + (size_t)(t->R - 1) * t->ld + Cm, sizeof(double), hipMemcpyDeviceToHost, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        out->pick.var = -1; out->pick.candidates = 0; out->pick.x_var = 0.0; out->pick.z = slab->pick.z;
    }
    return status;
}

int lpx_bounded_node(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                     int nint, const uint8_t* is_int, double tol, lpx_node_record* out)
{
    return bounded_node(t, K, cols, lower, upper, o, LPX_BDUAL_SKIP_FIXED, 0.0, nint, is_int, tol, out, "lpx_bounded_node");
}

// ---- long-step ratio test and objective cutoff (the dual loop's forms with a flag beyond LPX_BDUAL_SKIP_FIXED) ----
int lpx_bounded_dual_run3(lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    const int rc = check_long_flags(flags, cutoff, "lpx_bounded_dual_run3"); if (rc) return rc;
    if (!t) { set_error("lpx_bounded_dual_run3: null tableau"); return LPX_EINVAL; }
    return bounded_run(t, o, 1 + flags, cb, user, st, cutoff);
}

int lpx_bounded_node2(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int nint, const uint8_t* is_int, double tol, lpx_node_record* out)
{
    const int rc = check_long_flags(flags, cutoff, "lpx_bounded_node2"); if (rc) return rc;
    return bounded_node(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, "lpx_bounded_node2");
}

// ---- the on-chip form of the node (kernel in lpx_bounded_node.hip): one launch, one wait ----
int lpx_bounded_node_fits(int R, int C) { return bounded_node_fits(R, C); }

// The steady state of a call: the inputs written into the handle's pinned slab, one kernel launch, one wait, the record read
// from the same slab.  Allocations and the copy of the integer mask happen only when K outgrows the slab or the mask's bytes change.
// stall_events > 0 (lpx_bounded_node4): the launch is the guarded kernel's (lpx_bounded_guard.hip) as a batch of one, its parameter
// record in the slab behind the triples; everything else is the same call.  fix_bound > -inf (lpx_bounded_node5): the launch is that
// of lpx_bounded_fix.hip, again a batch of one, whose record carries fix_bound and the places of the list behind it in the slab.
static int bounded_node_onchip(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                               int flags, double cutoff, int nint, const uint8_t* is_int, double tol, lpx_node_record* out, const char* what,
                               int stall_events = 0, lpx_guard_record* guard = nullptr, double fix_bound = -1.0 / 0.0,
                               lpx_fix_list* fix = nullptr)
{
    const std::string w = what;
    const bool fixing = fix_bound != -1.0 / 0.0;
    int rc = bounded_ready(t, true); if (rc) return rc;
    rc = fixing ? bounded_fix_ready(what) : stall_events > 0 ? bounded_guard_ready(what) : bounded_node_ready(what); if (rc) return rc;
    if (guard) { guard->bland_events = 0; guard->first_bland = -1; }
    if (fix) fix->n = 0;
    lpx_tableau::Bounds& b = t->bnd;
    std::memset(out, 0, sizeof(*out));
    out->pick.var = -1;
    constexpr size_t kOut = 64, kHdr = kOut + sizeof(NodeIn);
    static_assert(sizeof(NodeOut) <= kOut, "slab layout");
    const size_t o_par = (kHdr + (size_t)K * (2 * sizeof(double) + sizeof(int32_t)) + 15) & ~(size_t)15;
    const size_t o_list = o_par + ((sizeof(FixParams) + 15) & ~(size_t)15);
    const size_t need = fixing ? o_list + fix_list_bytes(nint)
                      : stall_events > 0 ? o_par + sizeof(NodeParams) : kHdr + (size_t)K * (2 * sizeof(double) + sizeof(int32_t));
    if (need > b.nodeio_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        if (b.nodeio) hipHostFree(b.nodeio);
        b.nodeio = nullptr; b.nodeio_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&b.nodeio, 2 * need));
        b.nodeio_bytes = 2 * need;
    }
    const size_t stage = (size_t)K * (5 * sizeof(double) + sizeof(int32_t));     // the layout of BoundEdit
    if (stage > b.chg_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        hipFree(b.chg); b.chg = nullptr; b.chg_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&b.chg, 2 * stage));
        b.chg_bytes = 2 * stage;
    }
    const bool has_mask = is_int && nint > 0;
    if (has_mask && !(b.mask_n == nint && std::memcmp(b.mask_h.data(), is_int, (size_t)nint) == 0)) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));                            // an earlier copy may still read mask_h
        b.mask_h.assign(is_int, is_int + nint);
        LPX_HIP_TRY(hipMemcpyAsync(b.pickmask, b.mask_h.data(), (size_t)nint, hipMemcpyHostToDevice, t->stream));
        b.mask_n = nint;
    }
    bool any_lo = false;
    for (int k = 0; k < K; ++k) if (lower[k] != 0.0) any_lo = true;
    NodeOut* rec = reinterpret_cast<NodeOut*>(b.nodeio);
    NodeIn* in = reinterpret_cast<NodeIn*>(b.nodeio + kOut);
    std::memset(in, 0, sizeof(*in));
    in->K = K; in->flags = flags; in->nint = nint; in->has_mask = has_mask ? 1 : 0; in->max_iter = o->max_iter;
    in->lo_used = (b.lo_used || any_lo) ? 1 : 0;
    in->eps = o->eps; in->ratio_tol = o->ratio_tol; in->cutoff = cutoff; in->tol = tol;
    in->stall_events = fixing && stall_events == 0 ? INT32_MAX : stall_events;    // the fix kernel carries the guard: INT_MAX = never
    if (K > 0) {
        double* a = reinterpret_cast<double*>(in + 1);
        std::memcpy(a, lower, sizeof(double) * K);
        std::memcpy(a + K, upper, sizeof(double) * K);
        std::memcpy(a + 2 * (size_t)K, cols, sizeof(int32_t) * K);
    }
    NodeParams n; std::memset(&n, 0, sizeof(n));
    n.T = t->T; n.ld = t->ld; n.R = t->R; n.C = t->C;
    n.rhsbuf = t->rhsbuf; n.basis = t->basis; n.trace = t->trace; n.trace_cap = t->trace_cap; n.st = t->st;
    n.ub = b.ub; n.lo = b.lo; n.flip = b.flip; n.edit = reinterpret_cast<double*>(b.chg); n.mask = b.pickmask;
    n.in = in; n.out = rec;
    FixParams* F = reinterpret_cast<FixParams*>(b.nodeio + o_par);
    if (fixing) {
        F->n = n; F->fix_bound = fix_bound;
        fix_list_place(b.nodeio + o_list, nint, F);
        rec->pad = 0;                                                            // a refused edit writes no count
        LPX_HIP_TRY(launch_bounded_fix_onchip(F, 1, bounded_node_lds_bytes(t->R, t->C), t->stream));
    } else if (stall_events > 0) {
        NodeParams* P = reinterpret_cast<NodeParams*>(b.nodeio + o_par);
        *P = n;
        LPX_HIP_TRY(launch_bounded_guard_onchip(P, 1, bounded_node_lds_bytes(t->R, t->C), t->stream));
    } else
        LPX_HIP_TRY(launch_bounded_node_onchip(n, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));                                // the one wait: the record is in the slab
    if ((stall_events > 0 || fixing) && guard) {
        const GuardOut* g = reinterpret_cast<const GuardOut*>(rec);
        guard->bland_events = g->bland_events; guard->first_bland = g->first_bland;
    }
    if (rec->status < 0) {                                                       // refused by the kernel: the handle is as it was
        if (rec->inf_k >= 0) { set_error(w + ": upper[" + std::to_string(rec->inf_k) + "] = +inf on a flipped column"); return LPX_EINVAL; }
        out->unrepairable = rec->unrepairable;
        set_error(w + ": " + std::to_string(out->unrepairable) + " column(s) with a negative reduced cost and no upper "
                  "bound: a bound flip cannot restore dual feasibility");
        return LPX_EINVAL;
    }
    node_onchip_commit(t, rec, any_lo, out);
    bounds_note_edit(t, K, cols, lower, upper);
    if (fixing) fix_commit(t, rec->pad, *F, fix);
    return rec->status;
}

int lpx_bounded_node3(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int nint, const uint8_t* is_int, double tol, int form, lpx_node_record* out)
{
    const char* what = "lpx_bounded_node3";
    const std::string w = what;
    int rc = check_long_flags(flags, cutoff, what); if (rc) return rc;
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error(w + ": unknown form"); return LPX_EINVAL; }
    if (form == LPX_NODE_LAUNCHES || (form == LPX_NODE_AUTO && t && !bounded_node_fits(t->R, t->C)))
        return bounded_node(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what);
    rc = check_change_args(t, K, cols, lower, upper, what); if (rc) return rc;
    rc = check_pick_args(t, nint, tol, out, what); if (rc) return rc;
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    rc = check_node_opts(t, o, what); if (rc) return rc;
    rc = check_node_fits(t, what); if (rc) return rc;
    return bounded_node_onchip(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what);
}

// The node with the stall guard (include/lpx.h, "stall guard").  stall_events = 0 is lpx_bounded_node3 in every form; above 0 only
// the on-chip form exists (kernel in lpx_bounded_guard.hip).
int lpx_bounded_node4(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int stall_events, int nint, const uint8_t* is_int, double tol, int form,
                      lpx_node_record* out, lpx_guard_record* guard)
{
    const char* what = "lpx_bounded_node4";
    const std::string w = what;
    int rc = check_long_flags(flags, cutoff, what); if (rc) return rc;
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error(w + ": unknown form"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error(w + ": stall_events is negative"); return LPX_EINVAL; }
    if (guard) { guard->bland_events = 0; guard->first_bland = -1; }
    const bool launches = form == LPX_NODE_LAUNCHES || (form == LPX_NODE_AUTO && t && !bounded_node_fits(t->R, t->C));
    if (launches && stall_events > 0) { set_error(w + ": the stall guard has no launches form"); return LPX_EINVAL; }
    if (launches) return bounded_node(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what);
    rc = check_change_args(t, K, cols, lower, upper, what); if (rc) return rc;
    rc = check_pick_args(t, nint, tol, out, what); if (rc) return rc;
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    rc = check_node_opts(t, o, what); if (rc) return rc;
    rc = check_node_fits(t, what); if (rc) return rc;
    return bounded_node_onchip(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what, stall_events, guard);
}

// The node with reduced-cost tightening (include/lpx.h, "reduced-cost tightening").  fix_bound = -inf is lpx_bounded_node4 in every
// form; any other value needs the on-chip form (kernel in lpx_bounded_fix.hip).
int lpx_bounded_node5(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int stall_events, double fix_bound, int nint, const uint8_t* is_int, double tol, int form,
                      lpx_node_record* out, lpx_guard_record* guard, lpx_fix_list* fix)
{
    const char* what = "lpx_bounded_node5";
    const std::string w = what;
    int rc = check_long_flags(flags, cutoff, what); if (rc) return rc;
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error(w + ": unknown form"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error(w + ": stall_events is negative"); return LPX_EINVAL; }
    rc = check_fix_args(fix_bound, fix, nint, what); if (rc) return rc;
    if (guard) { guard->bland_events = 0; guard->first_bland = -1; }
    if (fix) fix->n = 0;
    const bool fixing = fix_bound != -1.0 / 0.0;
    const bool launches = form == LPX_NODE_LAUNCHES || (form == LPX_NODE_AUTO && t && !bounded_node_fits(t->R, t->C));
    if (launches && stall_events > 0) { set_error(w + ": the stall guard has no launches form"); return LPX_EINVAL; }
    if (launches && fixing) { set_error(w + ": reduced-cost tightening has no launches form"); return LPX_EINVAL; }
    if (launches) return bounded_node(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what);
    rc = check_change_args(t, K, cols, lower, upper, what); if (rc) return rc;
    rc = check_pick_args(t, nint, tol, out, what); if (rc) return rc;
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    rc = check_node_opts(t, o, what); if (rc) return rc;
    rc = check_node_fits(t, what); if (rc) return rc;
    return bounded_node_onchip(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, what, stall_events, guard, fix_bound, fix);
}

// ---- GMI cuts on a handle with bounds, and the cut loop at a bounded root (kernels in lpx_cuts.hip) ----
// The round itself is gmi_round_run's; what the handle keeps beside the tableau follows the reshape here.
static int gmi_round_bounded(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o, int* n_added,
                             int32_t* src_rows, int* n_purged, int32_t* purged_cols, const char* what)
{
    lpx_tableau::Bounds& b = t->bnd;
    const int Cm = t->C - 1;
    std::vector<int32_t> pc((size_t)(Cm - first_cut_col > 0 ? Cm - first_cut_col : 1));
    int K = 0, P = 0;
    CutBounds cb{nullptr, nullptr, nullptr, t->rhsbuf};
    if (b.bounds_set) { cb.ub = b.ub; cb.lo = b.lo; cb.flip = b.flip; }
    t->suspended = t->suspended2 = t->fsuspended = false;
    const int rc = gmi_round_run(t, is_int, n_mask, first_cut_col, o, &K, src_rows, &P, pc.data(), &cb, what);
    if (rc) return rc;
    if (b.bounds_set && (K > 0 || P > 0)) {
        b.bounds_C = t->C;
        if (!b.whole.empty()) {                         // the plunge's host knowledge: purged columns leave, a new slack is not whole
            for (int i = P - 1; i >= 0; --i) if ((size_t)pc[i] < b.whole.size()) b.whole.erase(b.whole.begin() + pc[i]);
            b.whole.resize((size_t)(t->C - 1), 0);
        }
    }
    if (n_added) *n_added = K;
    if (n_purged) *n_purged = P;
    if (purged_cols) for (int i = 0; i < P; ++i) purged_cols[i] = pc[i];
    return 0;
}

int lpx_tableau_gmi_round_bounded(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, const lpx_cut_opts* o,
                                  int* n_added, int32_t* src_rows, int* n_purged, int32_t* purged_cols)
{
    const char* what = "lpx_tableau_gmi_round_bounded";
    int rc = gmi_round_args(t, is_int, n_mask, first_cut_col, o, 0, what); if (rc) return rc;
    rc = check_bounds(t, what, false); if (rc) return rc;
    return gmi_round_bounded(t, is_int, n_mask, first_cut_col, o, n_added, src_rows, n_purged, purged_cols, what);
}

int lpx_bounded_cut_loop(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, int nint, const uint8_t* node_is_int,
                         const lpx_cut_opts* co, const lpx_run_opts* ro, int flags, int form, lpx_cut_loop_record* rec)
{
    const char* what = "lpx_bounded_cut_loop";
    const std::string w = what;
    if (!rec) { set_error(w + ": null record"); return LPX_EINVAL; }
    int rc = gmi_round_args(t, is_int, n_mask, first_cut_col, co, 0, what); if (rc) return rc;
    rc = check_long_flags(flags | LPX_BDUAL_SKIP_FIXED, -1.0 / 0.0, what); if (rc) return rc;
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error(w + ": unknown form"); return LPX_EINVAL; }
    rc = check_pick_args(t, nint, co->int_tol, rec, what); if (rc) return rc;
    rc = check_bounds(t, what, true); if (rc) return rc;
    lpx_run_opts d; if (!ro) { lpx_default_opts(&d, 1); ro = &d; }
    rc = check_node_opts(t, ro, what); if (rc) return rc;
    if (form == LPX_NODE_ONCHIP) {                      // every shape the rounds can reach has to fit: they grow R and C alike
        rc = check_node_fits(t, what); if (rc) return rc;
        const int a = t->Rcap - t->R < t->Ccap - t->C ? t->Rcap - t->R : t->Ccap - t->C;
        if (!bounded_node_fits(t->R + a, t->C + a)) { set_error(w + ": the handle's spare capacity does not fit the on-chip form"); return LPX_EINVAL; }
    }
    double* zb = rec->z_before; double* za = rec->z_after;
    std::memset(rec, 0, sizeof(*rec));
    rec->z_before = zb; rec->z_after = za; rec->status = LPX_OPTIMAL; rec->stop = LPX_CUTLOOP_ROUNDS; rec->pick.var = -1;
    rec->R = t->R; rec->C = t->C;
    const int nflags = flags | LPX_BDUAL_SKIP_FIXED;
    const double cutoff = -1.0 / 0.0;
    rc = lpx_tableau_branch_pick(t, nint, node_is_int, co->int_tol, &rec->pick); if (rc) return rc;
    for (;;) {
        if (rec->pick.var < 0) { rec->stop = LPX_CUTLOOP_INTEGRAL; break; }
        if (rec->rounds >= co->max_rounds) { rec->stop = LPX_CUTLOOP_ROUNDS; break; }
        int K = 0, P = 0;
        rc = gmi_round_bounded(t, is_int, n_mask, first_cut_col, co, &K, nullptr, &P, nullptr, what); if (rc) return rc;
        rec->purged += P; rec->R = t->R; rec->C = t->C;
        if (K == 0) { rec->stop = LPX_CUTLOOP_STALLED; break; }
        rec->added += K;
        const double z0 = rec->pick.z;
        lpx_node_record nr;
        rc = lpx_bounded_node3(t, 0, nullptr, nullptr, nullptr, ro, nflags, cutoff, nint, node_is_int, co->int_tol, form, &nr);
        if (rc < 0) return rc;
        if (zb) zb[rec->rounds] = z0;
        if (za) za[rec->rounds] = nr.pick.z;
        rec->rounds += 1; rec->events += nr.events; rec->status = nr.status; rec->pick = nr.pick;
        if (nr.status == LPX_INFEASIBLE) { rec->stop = LPX_CUTLOOP_INFEASIBLE; break; }
        if (nr.status == LPX_ITER_LIMIT) { rec->stop = LPX_CUTLOOP_ITER_LIMIT; break; }
        if (nr.status != LPX_OPTIMAL) { rec->stop = LPX_CUTLOOP_STATUS; break; }
    }
    if (co->purge && rec->stop <= LPX_CUTLOOP_ROUNDS) {
        lpx_cut_opts po = *co; po.cuts_per_round = 0;
        int K = 0, P = 0;
        rc = gmi_round_bounded(t, is_int, n_mask, first_cut_col, &po, &K, nullptr, &P, nullptr, what); if (rc) return rc;
        rec->purged += P; rec->R = t->R; rec->C = t->C;
    }
    return rec->stop == LPX_CUTLOOP_ITER_LIMIT ? LPX_ITER_LIMIT : 0;
}

// ---- strong-branching probes of the handle as it stands (kernel in lpx_bounded_probe.hip): one launch, one wait, no write to the handle ----
int lpx_bounded_probe(lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, double prune, int nint, const uint8_t* is_int,
                      double tol, int cand_max, int probe_iter, lpx_probe_head* head, lpx_probe_record* out)
{
    const char* what = "lpx_bounded_probe";
    const std::string w = what;
    // the arguments that need no handle first: they answer the same with and without a device, and without a handle
    if (!head || !out) { set_error(w + ": null " + (!head ? "head" : "out")); return LPX_EINVAL; }
    int rc = check_probe_args(cand_max, probe_iter, what); if (rc) return rc;
    if (prune != prune) { set_error(w + ": prune is NaN"); return LPX_EINVAL; }
    rc = check_long_flags(flags, cutoff, what); if (rc) return rc;
    if (!t) { set_error(w + ": null handle"); return LPX_EINVAL; }
    rc = check_pick_args(t, nint, tol, out, what); if (rc) return rc;
    rc = check_bounds(t, what, true); if (rc) return rc;
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    rc = check_node_opts(t, o, what); if (rc) return rc;
    rc = check_node_fits(t, what); if (rc) return rc;
    rc = bounded_ready(t, true); if (rc) return rc;
    rc = bounded_probe_ready(what); if (rc) return rc;
    lpx_tableau::Bounds& b = t->bnd;
    const size_t nrec = 2 * (size_t)cand_max;
    const size_t o_head = (sizeof(ProbeParams) + 15) & ~(size_t)15, o_rec = o_head + 16, need = o_rec + sizeof(lpx_probe_record) * nrec;
    static_assert(sizeof(lpx_probe_head) == 16 && sizeof(lpx_probe_record) == 64, "record layout of include/lpx.h");
    if (need > b.probeio_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        if (b.probeio) hipHostFree(b.probeio);
        b.probeio = nullptr; b.probeio_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&b.probeio, 2 * need));
        b.probeio_bytes = 2 * need;
    }
    const size_t ws = probe_ws_bytes(t, cand_max);
    if (ws > b.probews_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        hipFree(b.probews); b.probews = nullptr; b.probews_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&b.probews, 2 * ws));
        b.probews_bytes = 2 * ws;
    }
    const bool has_mask = is_int && nint > 0;
    if (has_mask && !(b.mask_n == nint && std::memcmp(b.mask_h.data(), is_int, (size_t)nint) == 0)) {
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));                            // an earlier copy may still read mask_h
        b.mask_h.assign(is_int, is_int + nint);
        LPX_HIP_TRY(hipMemcpyAsync(b.pickmask, b.mask_h.data(), (size_t)nint, hipMemcpyHostToDevice, t->stream));
        b.mask_n = nint;
    }
    ProbeParams* P = reinterpret_cast<ProbeParams*>(b.probeio);
    lpx_probe_head* hd = reinterpret_cast<lpx_probe_head*>(b.probeio + o_head);
    lpx_probe_record* rec = reinterpret_cast<lpx_probe_record*>(b.probeio + o_rec);
    probe_params(t, o, flags, cutoff, prune, nint, has_mask ? b.pickmask : nullptr, tol, cand_max, probe_iter, b.lo_used, b.probews,
                 nullptr, hd, rec, P);
    LPX_HIP_TRY(launch_bounded_probe_onchip(P, 1, cand_max, bounded_node_lds_bytes(t->R, t->C), t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));                                // the one wait: head and records are in the slab
    *head = *hd;
    std::memcpy(out, rec, sizeof(lpx_probe_record) * nrec);
    return 0;
}

}  // extern "C"
