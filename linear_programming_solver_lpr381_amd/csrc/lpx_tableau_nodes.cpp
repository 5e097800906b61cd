// lpx_tableau_nodes.cpp -- host side of node and child assembly on tableau handles, the parent store with its chunk cache, and
// the solution read-backs (C ABI of include/lpx.h).  Kernels: lpx_nodes.hip.
#include "lpx_handle.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace lpx;

namespace {

// Staging of the batched entry points: a pinned buffer and, where asked for, a device buffer of the same size, grown to twice
// the need.  One per thread, shared by the entry points (each has waited for its stream when it returns), and never freed: the
// HIP runtime may be gone when thread-locals are torn down.
struct Scratch {
    char* h = nullptr; char* d = nullptr; size_t cap = 0;    // d: nullptr or cap bytes as well
    int reserve(size_t need, bool device)
    {
        if (need > cap) {
            if (h) hipHostFree(h);
            hipFree(d);
            h = nullptr; d = nullptr; cap = 0;
            LPX_HIP_TRY(hipHostMalloc((void**)&h, 2 * need));
            cap = 2 * need;
        }
        if (device && !d) LPX_HIP_TRY(hipMalloc((void**)&d, cap));
        return 0;
    }
};
Scratch& scratch() { static thread_local Scratch sc; return sc; }

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// waits once on every distinct stream of a list of handles
int sync_distinct_streams(lpx_tableau* const* ts, int count)
{
    for (int i = 0; i < count; ++i) {
        bool seen = false; for (int j = 0; j < i; ++j) if (ts[j]->stream == ts[i]->stream) { seen = true; break; }
        if (!seen) LPX_HIP_TRY(hipStreamSynchronize(ts[i]->stream));
    }
    return 0;
}

// a new tableau is coming: nothing to continue.  The host half of lpx_tableau_set_shape; the caller brings shape_h to the device.
void set_live_shape(lpx_tableau* t, int R, int C)
{
    t->R = R; t->C = C; t->suspended = t->suspended2 = t->fsuspended = false;
    t->shape_h[0] = R; t->shape_h[1] = C;
}

// x[0..nvars) and z of a final tableau from its RHS column [m + 1] and basis [m]
void scatter_solution(const double* rhs, const int32_t* basis, int m, int nvars, double* x, double* z)
{
    if (x) {
        for (int j = 0; j < nvars; ++j) x[j] = 0.0;
        for (int i = 0; i < m; ++i) if (basis[i] >= 0 && basis[i] < nvars) x[basis[i]] = rhs[i];   // FinalizeReport :135-136
    }
    if (z) *z = rhs[m];                                                                           // :138
}

// ---- parent store: final tableaux of solved nodes parked in slab slots (warm-started B&B children) ----------
// Chunks of a destroyed store are kept for the next one (per process, up to LPX_STORE_CACHE_GB, default 64): a warm-started
// search parks thousands of parent tableaux and grows its store by 1 GB allocations, which cost a search that follows other
// GPU work on the same box up to half its time (bench.py's warm B&B leg right after the GPU test suite: 4.5-4.8 k nodes/s
// against 6.8-7.2 k; hipMalloc of memory another process has just released).
std::mutex g_chunk_mu;
std::multimap<size_t, void*> g_chunk_cache;
size_t g_chunk_cached = 0;
size_t chunk_cache_max()
{
    // LPX_STORE_CACHE_GB (clamped to >= 0; default 64).  Whatever the cap, a chunk is only kept while a quarter of the device's memory
    // stays free without it (chunk_release): several ranks sharing one GPU, or a big tableau allocated next, must not find the
    // memory sitting idle in here -- and every large allocation of the library retries once after lpx::trim_device_caches().
    static const size_t v = [] { const char* e = std::getenv("LPX_STORE_CACHE_GB"); long g = e ? std::atol(e) : 64; if (g < 0) g = 0; if (g > 4096) g = 4096; return (size_t)g << 30; }();
    return v;
}
void chunk_cache_drop_all()
{
    std::lock_guard<std::mutex> lk(g_chunk_mu);
    for (auto& kv : g_chunk_cache) hipFree(kv.second);
    g_chunk_cache.clear(); g_chunk_cached = 0;
}
hipError_t chunk_alloc(void** p, size_t bytes)
{
    {
        std::lock_guard<std::mutex> lk(g_chunk_mu);
        auto it = g_chunk_cache.find(bytes);
        if (it != g_chunk_cache.end()) { *p = it->second; g_chunk_cache.erase(it); g_chunk_cached -= bytes; return hipSuccess; }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    // out of memory with chunks of other sizes in the cache: give them back and try once more
    (void)hipGetLastError();
    chunk_cache_drop_all();
    return hipMalloc(p, bytes);
}
void chunk_release(void* p, size_t bytes)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_chunk_mu);
        size_t free_b = 0, total_b = 0;
        const bool roomy = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= total_b / 4;
        if (roomy && g_chunk_cached + bytes <= chunk_cache_max()) { g_chunk_cache.emplace(bytes, p); g_chunk_cached += bytes; return; }
    }
    hipFree(p);
}
}  // namespace

void lpx::trim_device_caches() { chunk_cache_drop_all(); }
hipError_t lpx::malloc_retry(void** p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    trim_device_caches();
    return hipMalloc(p, bytes);
}

struct lpx_store {
    int Rcap = 0, Ccap = 0, ld = 0, per_chunk = 128;
    size_t slot_doubles = 0;                 // Rcap * ld
    std::vector<double*> chunks_T; std::vector<int32_t*> chunks_b;
    std::vector<int> R, C;                   // live shape per slot
    std::vector<int> free_slots;
};

extern "C" {

int lpx_tableau_set_shape(lpx_tableau* t, int R, int C)
{
    if (!t || R < 1 || C < 2 || R > t->Rcap || C > t->Ccap) { set_error("lpx_tableau_set_shape: shape outside the handle's capacity"); return LPX_EINVAL; }
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));          // the pinned staging word may still be in flight
    set_live_shape(t, R, C);
    LPX_HIP_TRY(hipMemcpyAsync(t->shape, t->shape_h, sizeof(int32_t) * 2, hipMemcpyHostToDevice, t->stream));
    return 0;
}

int lpx_tableau_build_node(lpx_tableau* node, const lpx_tableau* root, int ncuts, const int32_t* var,
                           const double* coef, const double* zero, const double* rhs)
{
    if (!node || !root || ncuts < 0 || (ncuts > 0 && (!var || !coef || !zero || !rhs))) { set_error("lpx_tableau_build_node: bad argument"); return LPX_EINVAL; }
    if (root->R + ncuts > node->Rcap || root->C + ncuts > node->Ccap) { set_error("lpx_tableau_build_node: root shape + ncuts exceeds the node handle's capacity"); return LPX_EINVAL; }
    const int n = root->C - root->R;
    for (int k = 0; k < ncuts; ++k) if (var[k] < 0 || var[k] >= n) { set_error("lpx_tableau_build_node: branching variable out of range"); return LPX_EINVAL; }
    { int rc = lpx_tableau_set_shape(node, root->R + ncuts, root->C + ncuts); if (rc) return rc; }   // a refused call leaves the node as it was
    const int need = ncuts > 0 ? ncuts : 1;
    if (need > node->cutcap) {
        hipFree(node->cutbuf); if (node->cutbuf_h) hipHostFree(node->cutbuf_h);
        node->cutbuf = nullptr; node->cutbuf_h = nullptr; node->cutcap = 0;
        const int c = need + 64;
        LPX_HIP_TRY(hipMalloc((void**)&node->cutbuf, (size_t)c * 32));
        LPX_HIP_TRY(hipHostMalloc((void**)&node->cutbuf_h, (size_t)c * 32));
        node->cutcap = c;
    }
    const size_t cap = (size_t)node->cutcap;
    double* hc = reinterpret_cast<double*>(node->cutbuf_h);          // [coef | zero | rhs | var(int32, padded)]
    for (int k = 0; k < ncuts; ++k) { hc[k] = coef[k]; hc[cap + k] = zero[k]; hc[2 * cap + k] = rhs[k]; }
    int32_t* hv = reinterpret_cast<int32_t*>(hc + 3 * cap);
    for (int k = 0; k < ncuts; ++k) hv[k] = var[k];
    LPX_HIP_TRY(hipMemcpyAsync(node->cutbuf, node->cutbuf_h, cap * 32, hipMemcpyHostToDevice, node->stream));
    const double* dc = reinterpret_cast<const double*>(node->cutbuf);
    const double* T0 = root->snapT ? root->snapT : root->T;          // the pristine root tableau
    LPX_HIP_TRY(launch_build_node(T0, root->ld, root->R, root->C, node->T, node->ld, node->R, node->C,
                                  reinterpret_cast<const int32_t*>(dc + 3 * cap), dc, dc + cap, dc + 2 * cap,
                                  node->basis, node->stream));
    LPX_HIP_TRY(hipMemsetAsync(node->st, 0, sizeof(DevState), node->stream));
    return 0;   // stream-ordered: the run that follows on node->stream sees the finished tableau
}

// lpx_tableau_build_node for a group of nodes in one launch: node i gets the cuts [cut_off[i], cut_off[i + 1]) of the
// flattened arrays.  One H2D copy of the packed descriptors and cuts, one kernel, one wait.
int lpx_tableau_build_nodes(lpx_tableau** nodes, const lpx_tableau* root, int count, const int32_t* cut_off,
                            const int32_t* var, const double* coef, const double* zero, const double* rhs)
{
    if (!nodes || !root || count < 0 || !cut_off) { set_error("lpx_tableau_build_nodes: bad argument"); return LPX_EINVAL; }
    if (count == 0) return 0;
    const int total = cut_off[count];
    if (cut_off[0] != 0 || total < 0 || (total > 0 && (!var || !coef || !zero || !rhs))) { set_error("lpx_tableau_build_nodes: bad cut arrays"); return LPX_EINVAL; }
    const int n = root->C - root->R;
    int maxld = 16, maxR = 1;
    for (int i = 0; i < count; ++i) {
        lpx_tableau* t = nodes[i];
        const int nc = cut_off[i + 1] - cut_off[i];
        if (!t || nc < 0) { set_error("lpx_tableau_build_nodes: null node or negative cut count"); return LPX_EINVAL; }
        if (root->R + nc > t->Rcap || root->C + nc > t->Ccap) { set_error("lpx_tableau_build_nodes: root shape + ncuts exceeds a node handle's capacity"); return LPX_EINVAL; }
        maxld = std::max(maxld, t->ld); maxR = std::max(maxR, root->R + nc);
    }
    for (int k = 0; k < total; ++k) if (var[k] < 0 || var[k] >= n) { set_error("lpx_tableau_build_nodes: branching variable out of range"); return LPX_EINVAL; }
    Scratch& sc = scratch();
    const size_t tn = (size_t)(total > 0 ? total : 1);
    const size_t o_desc = 0, o_coef = up16(sizeof(BuildDesc) * (size_t)count), o_zero = o_coef + up16(8 * tn), o_rhs = o_zero + up16(8 * tn),
                 o_var = o_rhs + up16(8 * tn), need = o_var + up16(4 * tn);
    { int rc = sc.reserve(need, true); if (rc) return rc; }
    hipStream_t s = nodes[0]->stream;
    // every node's own stream has to be idle before another stream writes its tableau (and before the scratch is reused)
    { int rc = sync_distinct_streams(nodes, count); if (rc) return rc; }
    BuildDesc* d = reinterpret_cast<BuildDesc*>(sc.h + o_desc);
    for (int i = 0; i < count; ++i) {
        lpx_tableau* t = nodes[i];
        const int nc = cut_off[i + 1] - cut_off[i];
        set_live_shape(t, root->R + nc, root->C + nc);
        d[i].T = t->T; d[i].basis = t->basis; d[i].shape = t->shape; d[i].st = t->st; d[i].ld = t->ld; d[i].R = t->R; d[i].C = t->C; d[i].cut0 = cut_off[i];
    }
    if (total > 0) {
        std::memcpy(sc.h + o_coef, coef, 8 * (size_t)total); std::memcpy(sc.h + o_zero, zero, 8 * (size_t)total);
        std::memcpy(sc.h + o_rhs, rhs, 8 * (size_t)total); std::memcpy(sc.h + o_var, var, 4 * (size_t)total);
    }
    LPX_HIP_TRY(hipMemcpyAsync(sc.d, sc.h, need, hipMemcpyHostToDevice, s));
    const double* T0 = root->snapT ? root->snapT : root->T;          // the pristine root tableau
    LPX_HIP_TRY(launch_build_nodes(T0, root->ld, root->R, root->C, reinterpret_cast<const BuildDesc*>(sc.d + o_desc), count, maxld, maxR,
                                   reinterpret_cast<const int32_t*>(sc.d + o_var), reinterpret_cast<const double*>(sc.d + o_coef),
                                   reinterpret_cast<const double*>(sc.d + o_zero), reinterpret_cast<const double*>(sc.d + o_rhs), s));
    LPX_HIP_TRY(hipStreamSynchronize(s));       // the runs that follow use other streams
    return 0;
}

// ---- parent store (the chunk cache and the slots are above) ----
int lpx_store_create(int Rcap, int Ccap, lpx_store** out)
{
    if (!out || Rcap < 2 || Ccap < 2) { set_error("lpx_store_create: bad shape"); return LPX_EINVAL; }
    int rc = ensure_device(); if (rc) return rc;
    lpx_store* s = new lpx_store();
    s->Rcap = Rcap; s->Ccap = Ccap; s->ld = (Ccap + 15) / 16 * 16;
    s->slot_doubles = (size_t)Rcap * s->ld;
    *out = s;
    return 0;
}

void lpx_store_destroy(lpx_store* s)
{
    if (!s) return;
    // a chunk that enters the cache may be handed to another store at once: nothing (a parking copy, a child assembly reading a
    // parked parent -- they run on the handles' streams) may still be using it.  hipFree used to give this wait for free.
    if (!s->chunks_T.empty()) (void)hipDeviceSynchronize();
    for (double* p : s->chunks_T) chunk_release(p, sizeof(double) * s->slot_doubles * s->per_chunk);
    for (int32_t* p : s->chunks_b) chunk_release(p, sizeof(int32_t) * (size_t)s->Rcap * s->per_chunk);
    delete s;
}

// a free slot of the store, from a new pair of chunks when none is left; `what` prefixes the out-of-memory message
static int store_take_slot(lpx_store* s, const char* what, int* slot)
{
    if (s->free_slots.empty()) {
        double* Tc = nullptr; int32_t* bc = nullptr;
        LPX_HIP_TRY(chunk_alloc((void**)&Tc, sizeof(double) * s->slot_doubles * s->per_chunk));
        hipError_t e = chunk_alloc((void**)&bc, sizeof(int32_t) * (size_t)s->Rcap * s->per_chunk);
        if (e != hipSuccess) { hipFree(Tc); set_error(std::string(what) + ": out of device memory"); return LPX_ENOMEM; }
        const int base = (int)s->chunks_T.size() * s->per_chunk;
        s->chunks_T.push_back(Tc); s->chunks_b.push_back(bc);
        s->R.resize(base + s->per_chunk, 0); s->C.resize(base + s->per_chunk, 0);
        for (int k = s->per_chunk - 1; k >= 0; --k) s->free_slots.push_back(base + k);
    }
    *slot = s->free_slots.back(); s->free_slots.pop_back();
    return 0;
}

static double* store_T(lpx_store* s, int slot) { return s->chunks_T[slot / s->per_chunk] + (size_t)(slot % s->per_chunk) * s->slot_doubles; }
static int32_t* store_b(lpx_store* s, int slot) { return s->chunks_b[slot / s->per_chunk] + (size_t)(slot % s->per_chunk) * s->Rcap; }

int lpx_store_save(lpx_store* s, lpx_tableau* t, int* slot_out)
{
    if (!s || !t || !slot_out) { set_error("lpx_store_save: null argument"); return LPX_EINVAL; }
    if (t->ld != s->ld || t->R > s->Rcap) { set_error("lpx_store_save: tableau does not match the store's capacity class"); return LPX_EINVAL; }
    int slot = -1;
    { int rc = store_take_slot(s, "lpx_store_save", &slot); if (rc) return rc; }
    LPX_HIP_TRY(hipMemcpyAsync(store_T(s, slot), t->T, sizeof(double) * (size_t)t->R * t->ld, hipMemcpyDeviceToDevice, t->stream));
    LPX_HIP_TRY(hipMemcpyAsync(store_b(s, slot), t->basis, sizeof(int32_t) * (t->R - 1), hipMemcpyDeviceToDevice, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));       // the handle may be reused by the caller right away
    s->R[slot] = t->R; s->C[slot] = t->C;
    *slot_out = slot;
    return 0;
}

int lpx_store_release(lpx_store* s, int slot)
{
    if (!s || slot < 0 || slot >= (int)s->R.size()) return LPX_EINVAL;
    s->free_slots.push_back(slot);
    return 0;
}

int lpx_tableau_build_child_from_store(lpx_tableau* child, lpx_store* s, int slot, int var, int row_of_var, int is_ge, double bound)
{
    if (!child || !s || slot < 0 || slot >= (int)s->R.size()) { set_error("lpx_tableau_build_child_from_store: bad argument"); return LPX_EINVAL; }
    const int Rp = s->R[slot], Cp = s->C[slot];
    if (var < 0 || var >= Cp - 1 || row_of_var < 0 || row_of_var >= Rp - 1) { set_error("lpx_tableau_build_child_from_store: variable / row out of range"); return LPX_EINVAL; }
    if (Rp + 1 > child->Rcap || Cp + 1 > child->Ccap) { set_error("lpx_tableau_build_child_from_store: child handle too small"); return LPX_EINVAL; }
    { int rc = lpx_tableau_set_shape(child, Rp + 1, Cp + 1); if (rc) return rc; }
    LPX_HIP_TRY(launch_build_child(store_T(s, slot), s->ld, Rp, Cp, store_b(s, slot), child->T, child->ld,
                                   var, row_of_var, is_ge ? 1 : 0, bound, child->basis, child->stream));
    LPX_HIP_TRY(hipMemsetAsync(child->st, 0, sizeof(DevState), child->stream));
    return 0;
}

// lpx_tableau_build_child_from_store for a group of children in one launch (child i from stores[i] / slots[i]).
int lpx_tableau_build_children_from_store(lpx_tableau** children, lpx_store** stores, const int* slots, int count,
                                          const int32_t* var, const int32_t* row_of_var, const int32_t* is_ge, const double* bound)
{
    if (!children || !stores || !slots || count < 0 || (count > 0 && (!var || !row_of_var || !is_ge || !bound))) { set_error("lpx_tableau_build_children_from_store: bad argument"); return LPX_EINVAL; }
    if (count == 0) return 0;
    Scratch& sc = scratch();
    const size_t need = sizeof(ChildDesc) * (size_t)count;
    { int rc = sc.reserve(need, true); if (rc) return rc; }
    int maxld = 16, maxR = 1;
    for (int i = 0; i < count; ++i) {
        lpx_tableau* ch = children[i]; lpx_store* s = stores[i]; const int slot = slots[i];
        if (!ch || !s || slot < 0 || slot >= (int)s->R.size()) { set_error("lpx_tableau_build_children_from_store: bad child / store / slot"); return LPX_EINVAL; }
        const int Rp = s->R[slot], Cp = s->C[slot];
        if (var[i] < 0 || var[i] >= Cp - 1 || row_of_var[i] < 0 || row_of_var[i] >= Rp - 1) { set_error("lpx_tableau_build_children_from_store: variable / row out of range"); return LPX_EINVAL; }
        if (Rp + 1 > ch->Rcap || Cp + 1 > ch->Ccap) { set_error("lpx_tableau_build_children_from_store: child handle too small"); return LPX_EINVAL; }
        maxld = std::max(maxld, ch->ld); maxR = std::max(maxR, Rp + 1);
    }
    // every child's own stream has to be idle before another stream writes its tableau
    { int rc = sync_distinct_streams(children, count); if (rc) return rc; }
    ChildDesc* d = reinterpret_cast<ChildDesc*>(sc.h);
    for (int i = 0; i < count; ++i) {
        lpx_tableau* ch = children[i]; lpx_store* s = stores[i]; const int slot = slots[i];
        const int Rp = s->R[slot], Cp = s->C[slot];
        set_live_shape(ch, Rp + 1, Cp + 1);
        d[i].Tp = store_T(s, slot); d[i].basis_p = store_b(s, slot); d[i].T = ch->T; d[i].basis = ch->basis; d[i].shape = ch->shape; d[i].st = ch->st;
        d[i].ldp = s->ld; d[i].Rp = Rp; d[i].Cp = Cp; d[i].ld = ch->ld; d[i].var = var[i]; d[i].ik = row_of_var[i]; d[i].is_ge = is_ge[i] ? 1 : 0; d[i].pad = 0;
        d[i].bound = bound[i];
    }
    hipStream_t st = children[0]->stream;
    LPX_HIP_TRY(hipMemcpyAsync(sc.d, sc.h, need, hipMemcpyHostToDevice, st));
    LPX_HIP_TRY(launch_build_children(reinterpret_cast<const ChildDesc*>(sc.d), count, maxld, maxR, st));
    LPX_HIP_TRY(hipStreamSynchronize(st));      // the runs that follow use other streams
    return 0;
}

int lpx_tableau_build_child(lpx_tableau* child, lpx_tableau* parent, int var, int row_of_var, int is_ge, double bound)
{
    if (!child || !parent || child == parent) { set_error("lpx_tableau_build_child: bad argument"); return LPX_EINVAL; }
    if (var < 0 || var >= parent->C - 1 || row_of_var < 0 || row_of_var >= parent->R - 1) { set_error("lpx_tableau_build_child: variable / row out of range"); return LPX_EINVAL; }
    if (parent->R + 1 > child->Rcap || parent->C + 1 > child->Ccap) { set_error("lpx_tableau_build_child: child handle too small"); return LPX_EINVAL; }
    LPX_HIP_TRY(hipStreamSynchronize(parent->stream));              // the parent's final tableau must be complete
    { int rc = lpx_tableau_set_shape(child, parent->R + 1, parent->C + 1); if (rc) return rc; }
    LPX_HIP_TRY(launch_build_child(parent->T, parent->ld, parent->R, parent->C, parent->basis, child->T, child->ld,
                                   var, row_of_var, is_ge ? 1 : 0, bound, child->basis, child->stream));
    LPX_HIP_TRY(hipMemsetAsync(child->st, 0, sizeof(DevState), child->stream));
    return 0;
}

int lpx_tableau_basis(lpx_tableau* t, int32_t* basis)
{
    if (!t || !basis) return LPX_EINVAL;
    if (t->R > 1) LPX_HIP_TRY(hipMemcpyAsync(basis, t->basis, sizeof(int32_t) * (t->R - 1), hipMemcpyDeviceToHost, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

int lpx_tableau_solution2(lpx_tableau* t, int nvars, double* x, double* z, int32_t* basis_out)
{
    if (!t || nvars < 0) { set_error("lpx_tableau_solution: bad argument"); return LPX_EINVAL; }
    const int m = t->R - 1;
    std::vector<double> rhs(t->R);
    std::vector<int32_t> basis(m > 0 ? m : 1);
    LPX_HIP_TRY(hipMemcpy2DAsync(rhs.data(), sizeof(double), t->T + (t->C - 1), sizeof(double) * t->ld,
                                 sizeof(double), t->R, hipMemcpyDeviceToHost, t->stream));
    if (m > 0) LPX_HIP_TRY(hipMemcpyAsync(basis.data(), t->basis, sizeof(int32_t) * m, hipMemcpyDeviceToHost, t->stream));
    LPX_HIP_TRY(hipStreamSynchronize(t->stream));
    scatter_solution(rhs.data(), basis.data(), m, nvars, x, z);
    if (basis_out && m > 0) std::memcpy(basis_out, basis.data(), sizeof(int32_t) * m);
    return 0;
}

int lpx_tableau_solution(lpx_tableau* t, int nvars, double* x, double* z) { return lpx_tableau_solution2(t, nvars, x, z, nullptr); }

// lpx_tableau_solution2 for a batch: x is count x nvars, z has count entries, basis_out (optional) count x basis_stride.
int lpx_multi_solution(lpx_tableau** ts, int count, int nvars, double* x, double* z, int32_t* basis_out, int basis_stride)
{
    if (!ts || count < 0 || nvars < 0) { set_error("lpx_multi_solution: bad argument"); return LPX_EINVAL; }
    if (count == 0) return 0;
    Scratch& sc = scratch();
    size_t rows = 0;
    for (int i = 0; i < count; ++i) {
        if (!ts[i] || ts[i]->R < 1) { set_error("lpx_multi_solution: null or empty tableau"); return LPX_EINVAL; }
        if (basis_out && basis_stride < ts[i]->R - 1) { set_error("lpx_multi_solution: basis_stride too small"); return LPX_EINVAL; }
        rows += (size_t)ts[i]->R;
    }
    const size_t o_desc = 0, o_rhs = up16(sizeof(GatherDesc) * (size_t)count), o_bas = o_rhs + up16(sizeof(double) * rows);
    const size_t need = o_bas + up16(sizeof(int32_t) * rows);
    { int rc = sc.reserve(need, false); if (rc) return rc; }
    GatherDesc* d = reinterpret_cast<GatherDesc*>(sc.h + o_desc);
    double* rhs = reinterpret_cast<double*>(sc.h + o_rhs);
    int32_t* bas = reinterpret_cast<int32_t*>(sc.h + o_bas);
    size_t off = 0;
    for (int i = 0; i < count; ++i) {
        d[i].T = ts[i]->T; d[i].basis = ts[i]->basis; d[i].ld = ts[i]->ld; d[i].R = ts[i]->R; d[i].C = ts[i]->C; d[i].off = (int)off;
        off += (size_t)ts[i]->R;
    }
    // every handle's own stream has to be idle before another stream reads its tableau
    { int rc = sync_distinct_streams(ts, count); if (rc) return rc; }
    hipStream_t s = ts[0]->stream;
    LPX_HIP_TRY(launch_gather_solution(d, count, rhs, bas, s));
    LPX_HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < count; ++i) {
        const int m = ts[i]->R - 1;
        const double* r = rhs + d[i].off; const int32_t* b = bas + d[i].off;
        scatter_solution(r, b, m, nvars, x ? x + (size_t)i * nvars : nullptr, z ? z + i : nullptr);
        if (basis_out && m > 0) std::memcpy(basis_out + (size_t)i * basis_stride, b, sizeof(int32_t) * m);
    }
    return 0;
}

// lpx_store_save for a batch: all copies are enqueued first, each stream is waited for once.
int lpx_store_save_multi(lpx_store** ss, lpx_tableau** ts, int count, int* slots)
{
    if (!ss || !ts || !slots || count < 0) { set_error("lpx_store_save_multi: bad argument"); return LPX_EINVAL; }
    if (count == 0) return 0;
    for (int i = 0; i < count; ++i) {
        lpx_store* s = ss[i]; lpx_tableau* t = ts[i];
        if (!s || !t) { set_error("lpx_store_save_multi: null argument"); return LPX_EINVAL; }
        if (t->ld != s->ld || t->R > s->Rcap) { set_error("lpx_store_save_multi: tableau does not match the store's capacity class"); return LPX_EINVAL; }
    }
    Scratch& sc = scratch();
    const size_t need = sizeof(ParkDesc) * (size_t)count;
    { int rc = sc.reserve(need, true); if (rc) return rc; }
    // the finished runs used the group's stream; the nodes' own streams are idle, make sure
    { int rc = sync_distinct_streams(ts, count); if (rc) return rc; }
    ParkDesc* d = reinterpret_cast<ParkDesc*>(sc.h);
    size_t maxd = 0;
    for (int i = 0; i < count; ++i) {
        lpx_store* s = ss[i]; lpx_tableau* t = ts[i];
        int slot = -1;
        { int rc = store_take_slot(s, "lpx_store_save_multi", &slot); if (rc) return rc; }
        s->R[slot] = t->R; s->C[slot] = t->C;
        slots[i] = slot;
        d[i].srcT = t->T; d[i].dstT = store_T(s, slot); d[i].srcB = t->basis; d[i].dstB = store_b(s, slot);
        d[i].doubles = (size_t)t->R * t->ld; d[i].m = t->R - 1; d[i].pad = 0;
        maxd = std::max(maxd, d[i].doubles);
    }
    hipStream_t st = ts[0]->stream;
    LPX_HIP_TRY(hipMemcpyAsync(sc.d, sc.h, need, hipMemcpyHostToDevice, st));
    const int bpn = (int)std::min<size_t>(256, std::max<size_t>(1, maxd / 2 / 256 / 4));        // ~4 double2 per lane at least
    LPX_HIP_TRY(launch_park_many(reinterpret_cast<const ParkDesc*>(sc.d), count, bpn, st));
    LPX_HIP_TRY(hipStreamSynchronize(st));      // the handles may be reused, the slots read, right away
    return 0;
}

}  // extern "C"
