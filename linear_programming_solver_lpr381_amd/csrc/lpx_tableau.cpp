// lpx_tableau.cpp -- device-resident tableau handle (lifecycle, transfers, snapshot) and the host side of the single-LP simplex
// loops (C ABI of include/lpx.h).  The resident runs are in lpx_tableau_resident.cpp, the group runs and lpx_multi_run* in
// lpx_tableau_groups.cpp, the bounded-variable family in lpx_tableau_bounded.cpp (its batch of on-chip nodes in
// lpx_node_batch.cpp), node assembly and the parent store in lpx_tableau_nodes.cpp.  Host code only: kernels live in lpx_kernels.hip (two-launch paths) and lpx_pivot_fused.hip.
#include "lpx_handle.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace lpx { const std::string& get_error(); extern int g_device; }

using namespace lpx;

void lpx::tableau_view(lpx_tableau* t, TableauView* v)
{
    v->T = t->T; v->ld = t->ld; v->R = t->R; v->C = t->C;
    v->basis = t->basis; v->stream = t->stream;
    v->ws = &t->rgws; v->ws_bytes = &t->rgws_bytes;
}

void lpx::tableau_cut_view(lpx_tableau* t, CutView* v, bool need_second)
{
    v->T = t->T; v->T2 = need_second && fused_buffers(t) ? t->fT : nullptr;
    v->ld = t->ld; v->R = t->R; v->C = t->C; v->Rcap = t->Rcap; v->Ccap = t->Ccap;
    v->basis = t->basis; v->st = t->st; v->stream = t->stream;
    v->ws = &t->rgws; v->ws_bytes = &t->rgws_bytes;
}

void lpx::drop_graph(lpx_tableau* t)
{
    if (t->gexec) { hipGraphExecDestroy(t->gexec); t->gexec = nullptr; t->g_batch = 0; }
    graph_cache_drop_owner(&t->gexec);          // the parked ones captured the same buffers
}

extern "C" {

int lpx_abi_version(void) { return LPX_ABI_VERSION; }

int lpx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lpx_init(int device)
{
    int n = lpx_device_count();
    if (device < 0 || device >= n) { set_error("lpx_init: device index out of range"); return LPX_EDEVICE; }
    LPX_HIP_TRY(hipSetDevice(device));
    g_device = device;
    return ensure_device();
}

int lpx_last_error(char* buf, int len)
{
    const std::string& e = get_error();
    if (!buf || len <= 0) return (int)e.size();
    std::strncpy(buf, e.c_str(), len - 1);
    buf[len - 1] = 0;
    return (int)e.size();
}

int lpx_device_name(char* buf, int len)
{
    int rc = ensure_device();
    if (rc) return rc;
    hipDeviceProp_t prop;
    LPX_HIP_TRY(hipGetDeviceProperties(&prop, g_device));
    std::snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
}

void lpx_default_opts(lpx_run_opts* o, int dual)
{
    std::memset(o, 0, sizeof(*o));
    o->eps = 1e-9;
    o->ratio_tol = dual ? 1e-12 : 1e-9;
    o->max_iter = 10000;
    o->fdf_guard = 100;
    o->cleanup = 0;
    o->batch = 0;
    static const bool no_graph = [] { const char* e = std::getenv("LPX_GRAPH"); return e && e[0] == '0'; }();
    o->use_graph = no_graph ? 0 : 1;     // LPX_GRAPH=0: diagnostic switch to eager launches
    o->profile = 0;
    o->resident = 0;
}

int lpx_tableau_create(int R, int C, lpx_tableau** out)
{
    if (!out || R < 1 || C < 2) { set_error("lpx_tableau_create: bad shape"); return LPX_EINVAL; }
    int rc = ensure_device();
    if (rc) return rc;
    lpx_tableau* t = new lpx_tableau();
    t->R = R; t->C = C; t->Rcap = R; t->Ccap = C; t->ld = (C + 15) / 16 * 16;
    const size_t tb = sizeof(double) * (size_t)R * t->ld;
    const int wsn = R > C ? R : C;
    t->trace_cap = 1 << 16;
    // One device slab for the tableau and one for everything small around it, one pinned slab for the host mirrors:
    // a B&B pool creates dozens of handles per solve, and 14 hipMallocs + 2 hipHostMallocs each cost 4 ms per handle.
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nb = R > 1 ? (size_t)R - 1 : 1;
    const size_t sz[] = { up(sizeof(double) * t->ld), up(sizeof(double) * R), up(sizeof(double) * R), up(sizeof(double) * R),
                          up(sizeof(double) * R), up(sizeof(double) * (size_t)wsn * 32), up(sizeof(double) * 192),
                          up(sizeof(int32_t) * 256), up(sizeof(DevState)), up(sizeof(int32_t) * nb),
                          up(sizeof(int32_t) * 2 * (size_t)t->trace_cap), up(sizeof(DevState)), up(sizeof(int32_t) * 2) };
    size_t total = 0;
    for (size_t b : sz) total += b;
    hipError_t e_ = malloc_retry((void**)&t->T, tb);
    if (e_ == hipSuccess) e_ = malloc_retry((void**)&t->slab, total);
    if (e_ != hipSuccess) {
        set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e_));
        lpx_tableau_destroy(t);
        return e_ == hipErrorOutOfMemory ? LPX_ENOMEM : LPX_EDEVICE;
    }
    {
        char* p = t->slab; int k = 0;
        t->prow = (double*)p; p += sz[k++];
        t->pcol = (double*)p; p += sz[k++];
        t->col0 = (double*)p; p += sz[k++];
        t->col1 = (double*)p; p += sz[k++];
        t->rhsbuf = (double*)p; p += sz[k++];
        t->ws = (double*)p; p += sz[k++];
        t->part_v = (double*)p; p += sz[k++];      // [128..191]: diagnostic stamps (LPX_STAMPS builds only)
        t->part_i = (int32_t*)p; p += sz[k++];
        t->us = (DevState*)p; p += sz[k++];
        t->basis = (int32_t*)p; p += sz[k++];
        t->trace = (int32_t*)p; p += sz[k++];
        t->st = (DevState*)p; p += sz[k++];
        t->shape = (int32_t*)p; p += sz[k++];
    }
    if (hipHostMalloc((void**)&t->hslab, 256 + sizeof(int32_t) * 2) != hipSuccess ||
        (t->stream = borrow_stream()) == nullptr) {
        set_error("host-pinned state / stream creation failed");
        lpx_tableau_destroy(t);
        return LPX_EDEVICE;
    }
    t->hst = (DevState*)t->hslab; t->shape_h = (int32_t*)(t->hslab + 256);
    static_assert(sizeof(DevState) <= 256, "pinned slab layout");
    hipMemsetAsync(t->T, 0, tb, t->stream);
    hipMemsetAsync(t->slab, 0, total - sz[10] - sz[11] - sz[12], t->stream);      // everything in front of the trace
    hipMemsetAsync(t->st, 0, sizeof(DevState), t->stream);
    t->shape_h[0] = R; t->shape_h[1] = C;
    hipMemcpyAsync(t->shape, t->shape_h, sizeof(int32_t) * 2, hipMemcpyHostToDevice, t->stream);
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    *out = t;
    return 0;
}

void lpx_tableau_destroy(lpx_tableau* t)
{
    if (!t) return;
    if (t->stream) hipStreamSynchronize(t->stream);
    drop_graph(t);
    for (hipEvent_t e : t->events) hipEventDestroy(e);
    hipFree(t->T); hipFree(t->slab); hipFree(t->snapT); hipFree(t->snapBasis);
    hipFree(t->frows); hipFree(t->fcols); hipFree(t->fchosen); hipFree(t->cutbuf);
    hipFree(t->fT); hipFree(t->fslab); hipFree(t->dring); hipFree(t->cslab);
    hipFree(t->rgws);
    t->bnd.free();
    hipFree(t->xr); hipFree(t->xp); hipFree(t->xgen); hipFree(t->xbasis); hipFree(t->xT); hipFree(t->xc); hipFree(t->xq);
    if (t->hslab) hipHostFree(t->hslab);
    if (t->cutbuf_h) hipHostFree(t->cutbuf_h);
    delete t;                       // the stream is borrowed (borrow_stream), not owned
}

// A second handle in the state of the first (include/lpx.h): the live window, the basis, the RHS copy, the bounds and the loop
// state.  The capacity is the source's, so that ld -- and with it every kernel's geometry -- is the same on both.
int lpx_tableau_clone(const lpx_tableau* src, lpx_tableau** out)
{
    if (!src || !out) { set_error("lpx_tableau_clone: null argument"); return LPX_EINVAL; }
    if (src->suspended || src->suspended2 || src->fsuspended) {     // what continues such a run lives beside the state record, and is not copied
        set_error("lpx_tableau_clone: the source is in the middle of a run that lpx_multi_run_some left unfinished");
        return LPX_EINVAL;
    }
    lpx_tableau* c = nullptr;
    int rc = lpx_tableau_create(src->Rcap, src->Ccap, &c); if (rc) return rc;
    auto fail = [&](int code) { lpx_tableau_destroy(c); return code; };
    auto copy = [&]() -> int {
        LPX_HIP_TRY(hipStreamSynchronize(src->stream));              // the source's last run is complete; it is only read from here on
        c->R = src->R; c->C = src->C; c->shape_h[0] = src->R; c->shape_h[1] = src->C;
        LPX_HIP_TRY(hipMemcpyAsync(c->shape, c->shape_h, sizeof(int32_t) * 2, hipMemcpyHostToDevice, c->stream));
        LPX_HIP_TRY(hipMemcpyAsync(c->T, src->T, sizeof(double) * (size_t)src->R * src->ld, hipMemcpyDeviceToDevice, c->stream));
        if (src->R > 1) LPX_HIP_TRY(hipMemcpyAsync(c->basis, src->basis, sizeof(int32_t) * (src->R - 1), hipMemcpyDeviceToDevice, c->stream));
        LPX_HIP_TRY(hipMemcpyAsync(c->rhsbuf, src->rhsbuf, sizeof(double) * src->R, hipMemcpyDeviceToDevice, c->stream));
        LPX_HIP_TRY(hipMemcpyAsync(c->st, src->st, sizeof(DevState), hipMemcpyDeviceToDevice, c->stream));
        *c->hst = *src->hst;
        c->trace_void = true;                                        // the record says how many events the source made; the trace stayed there
        int r = bounds_clone(src, c); if (r) return r;
        LPX_HIP_TRY(hipStreamSynchronize(c->stream));
        return 0;
    };
    rc = copy(); if (rc) return fail(rc);
    *out = c;
    return 0;
}

int lpx_tableau_shape(const lpx_tableau* t, int* R, int* C, int* ld)
{
    if (!t) return LPX_EINVAL;
    if (R) *R = t->R;
    if (C) *C = t->C;
    if (ld) *ld = t->ld;
    return 0;
}

int lpx_tableau_upload(lpx_tableau* t, const double* T, const int32_t* basis)
{
    if (!t || !T) { set_error("lpx_tableau_upload: null argument"); return LPX_EINVAL; }
    t->suspended = t->suspended2 = t->fsuspended = false;
    LPX_HIP_TRY(hipMemcpy2DAsync(t->T, sizeof(double) * t->ld, T, sizeof(double) * t->C,
                                 sizeof(double) * t->C, t->R, hipMemcpyHostToDevice, t->stream));
    if (basis && t->R > 1)
        LPX_HIP_TRY(hipMemcpyAsync(t->basis, basis, sizeof(int32_t) * (t->R - 1), hipMemcpyHostToDevice, t->stream));
    LPX_HIP_TRY(hipMemsetAsync(t->st, 0, sizeof(DevState), t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int lpx_tableau_download(lpx_tableau* t, double* T, int32_t* basis)
{
    if (!t) return LPX_EINVAL;
    if (T)
        LPX_HIP_TRY(hipMemcpy2DAsync(T, sizeof(double) * t->C, t->T, sizeof(double) * t->ld,
                                     sizeof(double) * t->C, t->R, hipMemcpyDeviceToHost, t->stream));
    if (basis && t->R > 1)
        LPX_HIP_TRY(hipMemcpyAsync(basis, t->basis, sizeof(int32_t) * (t->R - 1), hipMemcpyDeviceToHost, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int lpx_tableau_snapshot(lpx_tableau* t)
{
    if (!t) return LPX_EINVAL;
    const size_t tb = sizeof(double) * (size_t)t->R * t->ld;
    if (!t->snapT) {            // sized for the capacity: a later set_shape may grow the live rows
        LPX_HIP_TRY(hipMalloc((void**)&t->snapT, sizeof(double) * (size_t)t->Rcap * t->ld));
        LPX_HIP_TRY(hipMalloc((void**)&t->snapBasis, sizeof(int32_t) * (t->Rcap > 1 ? t->Rcap - 1 : 1)));
    }
    LPX_HIP_TRY(hipMemcpyAsync(t->snapT, t->T, tb, hipMemcpyDeviceToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(t->snapBasis, t->basis, sizeof(int32_t) * (t->R > 1 ? t->R - 1 : 1),
                               hipMemcpyDeviceToDevice, t->stream));
    { int rc = bounds_snapshot(t); if (rc) return rc; }
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int lpx_tableau_restore(lpx_tableau* t)
{
    if (!t || !t->snapT) { set_error("lpx_tableau_restore: no snapshot"); return LPX_EINVAL; }
    t->suspended = t->suspended2 = t->fsuspended = false;
    const size_t tb = sizeof(double) * (size_t)t->R * t->ld;
    LPX_HIP_TRY(hipMemcpyAsync(t->T, t->snapT, tb, hipMemcpyDeviceToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(t->basis, t->snapBasis, sizeof(int32_t) * (t->R > 1 ? t->R - 1 : 1),
                               hipMemcpyDeviceToDevice, t->stream));
    { int rc = bounds_restore(t); if (rc) return rc; }
    LPX_HIP_TRY(hipMemsetAsync(t->st, 0, sizeof(DevState), t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int lpx_tableau_device_ptr(lpx_tableau* t, void** dptr, int* ld)
{
    if (!t) return LPX_EINVAL;
    if (dptr) *dptr = t->T;
    if (ld) *ld = t->ld;
    return 0;
}

#ifdef LPX_STAMPS
static int debug_stamps(void* src, unsigned long long* out, int n, int clear)        // n stamps out, cleared behind the copy
{
    if (!src) return LPX_EINVAL;
    LPX_HIP_TRY(hipMemcpy(out, src, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    if (clear) LPX_HIP_TRY(hipMemset(src, 0, sizeof(unsigned long long) * n));
    return 0;
}
int lpx_debug_resident_col(lpx_tableau* t, unsigned long long* out, int n, int clear) { return debug_stamps(t->xc ? t->xc + 2 * 256 * 2 * 2 : nullptr, out, n, clear); }
int lpx_debug_resident_group(lpx_tableau* t, unsigned long long* out, int n, int clear) { return debug_stamps(t->xp ? t->xp + 4 * ((size_t)t->ld + 8) : nullptr, out, n, clear); }
int lpx_debug_resident(lpx_tableau* t, unsigned long long* out, int n, int clear) { return debug_stamps(t->xp ? t->xp + 4 * (size_t)t->ld : nullptr, out, n, clear); }
extern "C++" { namespace lpx { hipError_t debug_copy_stamps(unsigned long long* out, int clear); } }
int lpx_debug_hs(unsigned long long* out, int clear) { LPX_HIP_TRY(lpx::debug_copy_stamps(out, clear)); return 0; }
int lpx_debug_ws(lpx_tableau* t, unsigned long long* out, int n, int clear) { return debug_stamps(t->us ? t->part_v + 128 : t->ws, out, n, clear); }
#endif

int lpx_tableau_trace(lpx_tableau* t, int32_t* trace, int cap, int* n)
{
    if (!t) return LPX_EINVAL;
    LPX_HIP_TRY(hipMemcpyAsync(t->hst, t->st, sizeof(DevState), hipMemcpyDeviceToHost, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    int k = t->trace_void ? 0 : t->hst->iter;
    if (k > t->trace_cap) k = t->trace_cap;
    if (n) *n = k;
    if (trace && cap > 0) {
        int c = k < cap ? k : cap;
        if (c > 0) LPX_HIP_TRY(hipMemcpy(trace, t->trace, sizeof(int32_t) * 2 * c, hipMemcpyDeviceToHost));
    }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// tableau loops on top of the generic driver (lpx_loop.cpp)
// ---------------------------------------------------------------------------------------------------
namespace {

int enqueue_pair(const SelParams& p, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr)
{
    if (p.mode == MODE_DUAL) {
        LPX_HIP_TRY(launch_select(p, s));
        LPX_HIP_TRY(launch_update(p, p.pcol, p.pcol, s, e0, e1));
    } else if (p.us) {
        LPX_HIP_TRY(launch_select_mb(p, s));
        LPX_HIP_TRY(launch_update_mb(p, s, e0, e1));
    } else {
        LPX_HIP_TRY(launch_select_la(p, s));
        LPX_HIP_TRY(launch_update(p, p.col0, p.col1, s, e0, e1));
    }
    return 0;
}

}  // namespace

void lpx::make_ctx(lpx_tableau* t, const SelParams& p, LoopCtx& c, DevState& init)
{
    make_ctx(t, p, p, [p](hipStream_t s, hipEvent_t e0, hipEvent_t e1) -> int { return enqueue_pair(p, s, e0, e1); }, c, init);
}

int lpx::run_loop(lpx_tableau* t, SelParams p, const lpx_run_opts* o, long long budget,
                  lpx_pivot_cb cb, void* user, lpx_stats* stats, int start_iter)
{
    LoopCtx c; DevState init;
    make_ctx(t, p, c, init);
    c.start_iter = start_iter;
    return run_device_loop(c, init, o, budget, cb, user, stats);
}

// init.iter carries the pivot count, so LoopRun numbers callbacks and reads the trace from there; LoopCtx::start_iter has nothing
// to add (it only acts on a record whose iter is 0, and equals at.iter wherever a caller would set it).
int lpx::continue_streaming(lpx_tableau* t, const lpx_run_opts* o, bool dual, const DevState& at, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    SelParams p = base_params(t, o, dual ? MODE_DUAL : MODE_PRIMAL);
    LoopCtx c; DevState init;
    make_ctx(t, p, c, init);
    resume_from(init, at, dual);
    return run_device_loop(c, init, o, pivot_budget(o, dual) + (dual ? 8 : 2), cb, user, st);
}

SelParams lpx::base_params(lpx_tableau* t, const lpx_run_opts* o, int mode)
{
    SelParams p; std::memset(&p, 0, sizeof(p));
    t->trace_void = false;
    p.T = t->T; p.ld = t->ld; p.R = t->Rcap; p.C = t->Ccap; p.shape = t->shape;
    p.prow = t->prow; p.pcol = t->pcol; p.col0 = t->col0; p.col1 = t->col1; p.rhsbuf = t->rhsbuf; p.basis = t->basis; p.trace = t->trace; p.trace_cap = t->trace_cap;
    p.st = t->st;
    p.eps = o->eps;
    p.tol_fdf = o->ratio_tol; p.tol_dual = o->ratio_tol;
    p.tol_primal = (mode == MODE_DUAL) ? o->eps : o->ratio_tol;
    p.max_iter = o->max_iter; p.fdf_guard = o->fdf_guard; p.cleanup = o->cleanup; p.mode = mode;
    p.ws = t->ws;
    p.rcap = 0;
    static const bool mb_env = [] { const char* e = std::getenv("LPX_SELECT_MB"); return !(e && e[0] == '0'); }();
    if (mode != MODE_DUAL && mb_env) {
        p.us = t->us; p.part_v = t->part_v; p.part_i = t->part_i; p.nblk = select_mb_blocks(t->Ccap); p.qsel = update_policy(t->ld, t->Rcap) != 0 ? 1 : 0;
    }
    return p;
}

bool lpx::fused_buffers(lpx_tableau* t)
{
    if (t->fT) return true;
    if (t->fused_off) return false;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tb = sizeof(double) * (size_t)t->Rcap * t->ld;
    const size_t sz[] = { up(sizeof(double) * t->ld), up(sizeof(double) * t->Rcap), up(2 * sizeof(DevState)),
                          up(pivot_ratio_bytes(t->Rcap)) };
    if (malloc_retry((void**)&t->fT, tb) != hipSuccess || malloc_retry((void**)&t->fslab, sz[0] + sz[1] + sz[2] + sz[3]) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(t->fT); hipFree(t->fslab);
        t->fT = nullptr; t->fslab = nullptr; t->fused_off = true;
        return false;
    }
    t->fprow = (double*)t->fslab;
    t->frhs = (double*)(t->fslab + sz[0]);
    t->frec = (DevState*)(t->fslab + sz[0] + sz[1]);
    t->frat = (double*)(t->fslab + sz[0] + sz[1] + sz[2]);
    hipMemsetAsync(t->fT, 0, tb, t->stream);
    hipMemsetAsync(t->fslab, 0, sz[0] + sz[1] + sz[2] + sz[3], t->stream);
    return true;
}

namespace {

// measured on MI355X with the select-only launch in one kernel at 24.3 us: 4097 x 12289 (403 MB) 118.9 us per
// pivot at d = 1, 34.9 at 12, 35.2 at 16 (the sweep 150 against 164 us); 1025 x 3073 (25 MB) 66 k pivots/s at d = 1, 79 k at 2,
// 82 k at 4, 80 k at 8.  With the select-only step of handles above 64 MB in two launches (lpx_pivot_ratio + lpx_pivot_select,
// 14.2 us together): 28.4 us per pivot at d = 8, 24.5 at 12, 23.0 at 16.  d = 16 against d = 12 in alternating runs of the bench
// (profiles/r14_sweep_bench.txt, three each, one call): 43.04-43.13 k against 39.97-40.24 k pivots/s, slowest against fastest
// +7.0 % (a second call: 42.89-43.23 k) -- so handles that cannot live in the Infinity Cache (above UPD_STREAM_BYTES, 292 MiB)
// run d = 16.  Between 64 MB and 292 MiB the depth stays 12: d = 16 on a handle of that size was not measured.  Up to 64 MB the
// select-only kernel is the one the 25 MB figures were taken with
static constexpr int PIVOT_DEFER_STREAM = 16, PIVOT_DEFER_LARGE = 12, PIVOT_DEFER_SMALL = 4;
static constexpr size_t PIVOT_DEFER_LARGE_BYTES = (size_t)64 << 20;
// Pivots per sweep of run_fused (LPX_PIVOT_DEFER=d, read once; DESIGN.md 4.1 has the measured table behind the default).
static int pivot_defer(int ld, int R)
{
    static const int forced = [] { const char* e = std::getenv("LPX_PIVOT_DEFER"); return e ? std::atoi(e) : 0; }();
    if (forced > 0) return std::min(forced, pivot_defer_max());
    const size_t bytes = sizeof(double) * (size_t)ld * (size_t)R;
    if (bytes > pivot_stream_bytes()) return PIVOT_DEFER_STREAM;
    return bytes > PIVOT_DEFER_LARGE_BYTES ? PIVOT_DEFER_LARGE : PIVOT_DEFER_SMALL;
}

// Ring of the pending pivots (2 * d slots), on first use.
static int defer_ring(lpx_tableau* t, int d)
{
    if (t->dring_slots >= 2 * d) return 0;
    hipFree(t->dring); t->dring = nullptr; t->dring_slots = 0;
    const size_t slots = 2 * (size_t)d;
    const size_t bytes = slots * sizeof(double) * ((size_t)t->ld + (size_t)t->Rcap) + slots * sizeof(int32_t);
    LPX_HIP_TRY(malloc_retry((void**)&t->dring, bytes));
    LPX_HIP_TRY(hipMemsetAsync(t->dring, 0, bytes, t->stream));
    t->dring_slots = (int)slots;
    return 0;
}

// Primal loop with ONE step per pivot: step L selects pivot L; every d-th one (a positive multiple of d) is also the
// sweep that applies the d pivots selected before it, out of place (lpx_pivot_fused<d>), the others select only
// (lpx_pivot_ratio + lpx_pivot_select, two kernels, on handles above 64 MB; lpx_pivot_select_ws, one, on the others --
// lpx_stats.launches counts steps either way).  The state record the host polls is one launch behind the device's, so the loop gets a few iterations
// of slack; when it ends, the pivots still pending are applied (lpx_pivot_flush, into buffer 0), or the tableau, when none
// are, may sit in the second buffer and is brought home (a device-to-device copy of the live rows, ~0.1 ms per 400 MB).
//
// Compact form: a basic column is a unit vector before and after every pivot, so a long run leaves the R - 1 of
// them out.  The entry pass gathers the nonbasic columns and the RHS (slots, in the order of the variables) into the second
// buffer and checks every basic column bit for bit; the loop runs on that buffer and on the handle's own as the pair, with slot
// coordinates in its records; the exit pass applies the pending pivots and writes the full layout back.  No tableau-sized
// allocation: a handle pays for the maps (8 bytes per column).  LPX_PIVOT_COMPACT=0: never, =1: whatever the budget.
// shortest budget, in sweeps, that takes the compact form.  Kernel trace at 4097 x 12289, d = 16: the entry pass 26 + 140 us,
// the exit pass 574 us against the flush's 466, one more host round trip for the flag -- about 0.3 ms -- against 39.5 us off every sweep
static constexpr int COMPACT_MIN_SWEEPS = 8;
static int pivot_compact_env()
{
    static const int v = [] { const char* e = std::getenv("LPX_PIVOT_COMPACT"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    return v;
}
// the maps of the compact form, on first use: slotvar [ld], vmap [Ccap], partial slots [128], ring slots' entering slots, {caux, shape, flag}
static bool compact_buffers(lpx_tableau* t)
{
    if (t->cslab) return true;
    const size_t ints = (size_t)t->ld + (size_t)t->Ccap + 128 + 2 * (size_t)pivot_defer_max() + 8;
    if (malloc_retry((void**)&t->cslab, sizeof(int32_t) * ints) != hipSuccess) { (void)hipGetLastError(); t->cslab = nullptr; return false; }
    return true;
}

static int run_fused(lpx_tableau* t, const SelParams& p, const lpx_run_opts* o, lpx_stats* stats, int start_iter)
{
    const int d = pivot_defer(t->ld, t->Rcap);
    { int rc = defer_ring(t, d); if (rc) return rc; }
    FusedParams f; std::memset(&f, 0, sizeof(f));
    f.P = p; f.T1 = t->fT; f.prow1 = t->fprow; f.rhs1 = t->frhs; f.rec = t->frec;
    f.pring = (double*)t->dring;
    f.fring = f.pring + (size_t)t->dring_slots * t->ld;
    f.rring = (int32_t*)(f.fring + (size_t)t->dring_slots * t->Rcap);
    f.defer = d;
    t->last_compact = false;
    CompactIo io; std::memset(&io, 0, sizeof(io));
    double pass_ms = 0.0;                            // the entry and exit passes: part of loop_ms, no part of launches
    const int cenv = pivot_compact_env();
    if (cenv != 0 && pivot_compact_ok(t->ld, t->Rcap, d) && t->C - t->R >= 1
        && (cenv == 1 || pivot_budget(o, false) >= (long long)COMPACT_MIN_SWEEPS * d) && compact_buffers(t)) {
        int32_t* ci = (int32_t*)t->cslab;
        io.full = t->T; io.ld = t->ld; io.R = t->R; io.C = t->C;
        io.comp = t->fT; io.cld = (t->C - t->R + 1 + 15) / 16 * 16;
        io.basis = t->basis; io.slotvar = ci; io.vmap = ci + t->ld;
        int32_t* pslot = io.vmap + t->Ccap; int32_t* qring = pslot + 128; int32_t* caux = qring + 2 * pivot_defer_max();
        int32_t* cshape = caux + 2; io.flag = cshape + 2;
        const double t0 = now_ms();
        int32_t bad = 0;
        LPX_HIP_TRY(hipMemsetAsync(io.flag, 0, sizeof(int32_t), t->stream));
        LPX_HIP_TRY(launch_compact_entry(io, cshape, caux, t->stream));
        LPX_HIP_TRY(hipMemcpyAsync(&bad, io.flag, sizeof(bad), hipMemcpyDeviceToHost, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        pass_ms += now_ms() - t0;
        if (!bad) {                                  // else: the full path, silently (the handle's tableau has not been touched)
            f.P.T = t->fT; f.T1 = t->T; f.P.ld = io.cld; f.P.C = t->C - t->R + 1; f.P.shape = cshape;
            f.compact = 1; f.ld_full = t->ld;
            f.slotvar = io.slotvar; f.pslot = pslot; f.qring = qring; f.caux = caux;
            t->last_compact = true;
        }
    }
    LoopCtx c; DevState init;
    make_ctx(t, p, c, init);
    c.key.assign(reinterpret_cast<const char*>(&f), sizeof(f));
    // A launch reads state record L % 2 and writes the other one, and ring slot L % 2d is its own.  The prologue's launch is
    // number 0, so the loop proper starts at 1 -- in the captured graph too (it is captured before the prologue runs, hence
    // the counter is preset), and a graph batch is a multiple of 2d so that every replay starts where the capture did.
    auto count = std::make_shared<long long>(1);
    double* rat = t->frat;
    c.enqueue_iter = [f, rat, count](hipStream_t s, hipEvent_t e0, hipEvent_t e1) -> int {
        LPX_HIP_TRY(launch_pivot_fused(f, rat, *count, s, e0, e1)); ++*count; return 0; };
    // the prologue also selects the first pivot, so that every launch of the loop proper has a pivot before it
    c.prologue = [f, rat, count](hipStream_t s) -> int {
        LPX_HIP_TRY(launch_fused_init(f, s)); LPX_HIP_TRY(launch_pivot_fused(f, rat, 0, s)); *count = 1; return 0; };
    c.launches_per_iter = 1;
    c.sweep_launch = [d](long long k) { return (k + 1) % d == 0; };      // k-th launch of the loop proper is launch k + 1
    c.start_iter = start_iter;
    lpx_run_opts oe = *o;
    { const int b = oe.batch > 0 ? oe.batch : 64; oe.batch = (b + 2 * d - 1) / (2 * d) * (2 * d); }
    o = &oe;
    const int rc = run_device_loop(c, init, o, pivot_budget(o, false) + 4, nullptr, nullptr, stats);
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    DevState recs[2];
    LPX_HIP_TRY(hipMemcpy(recs, t->frec, sizeof(recs), hipMemcpyDeviceToHost));
    const DevState& last = recs[1].pad[2] > recs[0].pad[2] ? recs[1] : recs[0];
    const int buf = last.pad[3] & 1, npend = (last.pad[3] >> 1) & 31, slot0 = last.pad[3] >> 8;
    if (f.compact) {
        // buffer 0 is the second buffer: its result expands straight into the handle's tableau; a result in the handle's own
        // memory expands into the second buffer and comes home by the copy below
        const double t0 = now_ms();
        io.full = buf ? t->fT : t->T;
        LPX_HIP_TRY(launch_compact_exit(f, io, buf ? t->T : t->fT, npend, slot0, t->stream));
        if (buf) LPX_HIP_TRY(hipMemcpyAsync(t->T, t->fT, sizeof(double) * (size_t)t->R * t->ld, hipMemcpyDeviceToDevice, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        pass_ms += now_ms() - t0;
    } else
    if (npend > 0) {
        LPX_HIP_TRY(launch_pivot_flush(f, buf, npend, slot0, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
        if (stats) stats->launches += 1;
    } else if (buf == 1) {
        LPX_HIP_TRY(hipMemcpyAsync(t->T, t->fT, sizeof(double) * (size_t)t->R * t->ld, hipMemcpyDeviceToDevice, t->stream));
        LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    }
    if (stats) stats->loop_ms += pass_ms;            // a refused entry pass has cost its time too
    return rc;
}


}  // namespace

extern "C" {

int lpx_tableau_last_run_compact(const lpx_tableau* t) { return t && t->last_compact ? 1 : 0; }

int lpx_primal_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    if (!t) { set_error("lpx_primal_run: null tableau"); return LPX_EINVAL; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 0); o = &d; }
    if (t->R < 2) { set_error("lpx_primal_run: tableau needs at least one constraint row"); return LPX_EINVAL; }
    t->last_compact = false;
    // Tableau small enough to live on chip: persistent workgroups, no per-pivot HBM traffic (lpx_resident.hip).
    static const bool res_env = [] { const char* e = std::getenv("LPX_RESIDENT"); return !(e && e[0] == '0'); }();
    int resume = 0;
    if (o->resident > 0 || (o->resident == 0 && res_env && !o->profile && (o->batch == 0 || o->batch >= 32))) {
        int grid = 0, rpw = 0; size_t lds = 0;
        // LPX_RESIDENT_COL=1: the column-owning variant (lpx_resident_col.hip) when a workgroup's columns fit its LDS.  It was
        // built to save one of the two cross-CU exchanges per pivot and is bit-identical, but measures the same 7.9-8.0 us per
        // pivot on config 2 as the row-owning kernel, so the row-owning one -- which fits more shapes -- stays the default.
        static const bool col_env = [] { const char* e = std::getenv("LPX_RESIDENT_COL"); return e && e[0] == '1'; }();
        bool col = false;
        if (!t->resident_off && col_env && resident_col_plan(t->R, t->C, &grid, &rpw, &lds)) col = true;
        if (!t->resident_off && (col || resident_plan(t->R, t->C, t->ld, &grid, &rpw, &lds))) {
            const int rc = run_resident(t, o, cb, user, st, grid, rpw, lds, &resume, col);
            if (rc != LPX_RESIDENT_RETRY) return rc;
            if (o->resident > 0) return LPX_EDEVICE;        // required, and it could not run
        } else
        if (o->resident > 0) { set_error("lpx_primal_run: resident = 1 but the tableau does not fit the chip's LDS"); return LPX_EINVAL; }
    }
    SelParams p = base_params(t, o, MODE_PRIMAL);
    // without a per-pivot callback: one fused launch per pivot (LPX_FUSED_PIVOT=0: the two-launch in-place kernels)
    static const bool fused_env = [] { const char* e = std::getenv("LPX_FUSED_PIVOT"); return !(e && e[0] == '0'); }();
    if (fused_env && p.us && !cb && fused_buffers(t)) return run_fused(t, p, o, st, resume);
    return run_loop(t, p, o, pivot_budget(o, false) + 2, cb, user, st, resume);
}

int lpx_dual_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    if (!t) { set_error("lpx_dual_run: null tableau"); return LPX_EINVAL; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    if (t->R < 2) { set_error("lpx_dual_run: tableau needs at least one constraint row"); return LPX_EINVAL; }
    static const bool res_env = [] { const char* e = std::getenv("LPX_RESIDENT"); return !(e && e[0] == '0'); }();
    if (o->resident > 0 || (o->resident == 0 && res_env && !o->profile && (o->batch == 0 || o->batch >= 32))) {
        int isdual = 1, status = 0;
        const ResGroupPlan plan = t->resident_off ? ResGroupPlan{} : resident_group_plan(&t, 1);
        if (plan.slots) {
            DevState resume;
            const int rc = run_resident_group(&t, &isdual, 1, o, o, &status, st, plan, cb, user, &resume);
            if (rc == 0) return status;
            if (rc != LPX_RESIDENT_RETRY) return rc;
            t->resident_off = true;
            if (o->resident > 0) return LPX_EDEVICE;
            // hand over to the streaming kernels at the pivot the resident loop had reached
            return continue_streaming(t, o, true, resume, cb, user, st);
        } else
        if (o->resident > 0) { set_error("lpx_dual_run: resident = 1 but the tableau does not fit the chip's LDS"); return LPX_EINVAL; }
    }
    if (!cb) {          // no per-pivot callback: one launch per step (lpx_group_fused, a group of one), update out of place
        int isdual = 1, status = 0;
        const int rc = multi_run_fused(&t, &isdual, 1, o, o, &status, st, nullptr, 0);
        if (rc != LPX_RESIDENT_RETRY) return rc ? rc : status;
    }
    SelParams p = base_params(t, o, MODE_DUAL);
    return run_loop(t, p, o, pivot_budget(o, true) + 8, cb, user, st);
}

int lpx_forced_pivots_run(lpx_tableau* t, const int32_t* rows, const int32_t* cols, int count,
                          double thresh, int32_t* chosen, const lpx_run_opts* o, lpx_stats* st)
{
    if (!t || !rows || !cols || count < 0) { set_error("lpx_forced_pivots_run: bad argument"); return LPX_EINVAL; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 0); o = &d; }
    for (int k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= t->R || cols[k] < 0 || cols[k] >= t->C) {
            set_error("lpx_forced_pivots_run: pivot position outside the tableau"); return LPX_EINVAL;
        }
    if (count > t->fcap) {
        hipFree(t->frows); hipFree(t->fcols); hipFree(t->fchosen);
        t->frows = t->fcols = t->fchosen = nullptr; t->fcap = 0;
        LPX_HIP_TRY(hipMalloc((void**)&t->frows, sizeof(int32_t) * count));
        LPX_HIP_TRY(hipMalloc((void**)&t->fcols, sizeof(int32_t) * count));
        LPX_HIP_TRY(hipMalloc((void**)&t->fchosen, sizeof(int32_t) * count));
        t->fcap = count;
        drop_graph(t);
    }
    if (count > 0) {
        LPX_HIP_TRY(hipMemcpyAsync(t->frows, rows, sizeof(int32_t) * count, hipMemcpyHostToDevice, t->stream));
        LPX_HIP_TRY(hipMemcpyAsync(t->fcols, cols, sizeof(int32_t) * count, hipMemcpyHostToDevice, t->stream));
        LPX_HIP_TRY(hipMemsetAsync(t->fchosen, 0xff, sizeof(int32_t) * count, t->stream));
    }
    SelParams p = base_params(t, o, MODE_FORCED);
    p.frows = t->frows; p.fcols = t->fcols; p.fcount = count; p.fthresh = thresh; p.fchosen = t->fchosen;
    int rc = run_loop(t, p, o, (long long)count + 2, nullptr, nullptr, st);
    if (chosen && count > 0)
        LPX_HIP_TRY(hipMemcpy(chosen, t->fchosen, sizeof(int32_t) * count, hipMemcpyDeviceToHost));
    return rc;
}

static int one_shot(double* T, int R, int C, int32_t* basis, const lpx_run_opts* o, int dual,
                    lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    if (!T || !basis) { set_error("null tableau or basis"); return LPX_EINVAL; }
    lpx_tableau* t = nullptr;
    int rc = lpx_tableau_create(R, C, &t);
    if (rc) return rc;
    double a = now_ms();
    rc = lpx_tableau_upload(t, T, basis);
    double h2d = now_ms() - a;
    if (rc) { lpx_tableau_destroy(t); return rc; }
    lpx_stats local; std::memset(&local, 0, sizeof(local));
    int status = dual ? lpx_dual_run(t, o, cb, user, &local) : lpx_primal_run(t, o, cb, user, &local);
    if (status < 0) { lpx_tableau_destroy(t); return status; }
    a = now_ms();
    rc = lpx_tableau_download(t, T, basis);
    local.d2h_ms = now_ms() - a;
    local.h2d_ms = h2d;
    lpx_tableau_destroy(t);
    if (st) *st = local;
    return rc ? rc : status;
}

int lpx_primal_tableau(double* T, int R, int C, int32_t* basis, double eps, int max_iter,
                       lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    lpx_run_opts o; lpx_default_opts(&o, 0);
    o.eps = eps; o.ratio_tol = eps; o.max_iter = max_iter;
    return one_shot(T, R, C, basis, &o, 0, cb, user, st);
}

int lpx_dual_tableau(double* T, int R, int C, int32_t* basis, double eps, double ratio_tol,
                     int fdf_guard, int max_iter, int cleanup,
                     lpx_pivot_cb cb, void* user, lpx_stats* st)
{
    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.eps = eps; o.ratio_tol = ratio_tol; o.fdf_guard = fdf_guard; o.max_iter = max_iter; o.cleanup = cleanup;
    return one_shot(T, R, C, basis, &o, 1, cb, user, st);
}

}  // extern "C"
