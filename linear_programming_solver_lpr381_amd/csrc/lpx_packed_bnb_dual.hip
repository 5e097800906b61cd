// lpx_packed_bnb_dual.hip -- packed batches of small integer programs with >= rows (lpx_solve_packed_bnb_dual, include/lpx.h;
// DESIGN.md section 4.28), gfx950 (CDNA4, wave64): lpx_packed_bnb.hip for the models lpx_solve_bnb_bounded_dual was built for.  count
// models of one shape come in as contiguous arrays, rows <= or >=, right-hand sides of either sign; ONE launch runs the WHOLE
// branch and bound of every model, arrays go back.  Workgroup i builds the tableau of model i in the LDS of its compute unit (a >=
// row negated while it is stored), makes the dual-feasibility flips, solves the root with the on-chip bounded dual loop and then
// runs the search of lpx_packed_bnb.hip: the depth-first stack, the bounds diff of a popped node, the node's edit, flips, dual loop
// and pick, the incumbent, the prune and the log.  The tableau never leaves LDS.
//
// Launch shape: ONE workgroup x 1024 lanes per model, a grid of count independent workgroups.
//
// Shared-device rules, those of lpx_packed.hip:
//   * no workgroup waits on any other workgroup; there is no spin loop, no flag and no atomic between workgroups;
//   * every loop is bounded: the search by max_nodes (lane 0 stops it at nodes >= max_nodes, and the loop itself makes at most
//     max_nodes + 1 trips), the root's and a node's event loop by max_iter (at most max_iter + 1 trips of at most Cm passes each),
//     the whole model by max_events (tested in front of every pop), the rest by R, C, n, the depth or K.  All three limits are at
//     least 1 (checked on the host; max_iter at least 0), so a launch always ends;
//   * every value is written with ordinary vector stores from C++; the only inline assembly is the empty register pin of S and t
//     that lpx_packed_bnb.hip has, once per node;
//   * no scratch (the compiler's resource remarks are in DESIGN.md section 4.28).
//
// The arithmetic: part a is lpx_packed_dual.hip steps 1, 2b, 5 and 6, statement for statement, with the integer check of
// ValidateBnbBounded between the bounds check and the rel check (so the root is bit-equal to lpx_solve_bounded_dual); parts b and d
// are lpx_packed_bnb.hip's, kept here a second time: that file's code object stays byte for byte what it was (DESIGN.md section
// 4.28 says why the text is not shared through a header).  The search is bit-equal to lpx_solve_bnb_bounded_dual(...,
// LPX_NODE_ONCHIP) model by model wherever max_events and max_depth do not bind.
//
// Dynamic LDS (doubles) is the packed primal kernel's, so bounded_node_lds_bytes(m + 1, n + m + 1) is the fit rule unchanged:
//   tile [R * S]        R = m + 1, C = n + m + 1, row stride S = C | 1
//   ub   [C]            upper bounds of the columns, as the handle forms keep them: the current upper minus the current lower
//   buf  [max(R, C)]    the lower bounds [n] while the tableau is built; the flip list, the ratios / the pivot-column snapshot of the
//                       root; in a node the ordered list of the edited columns, then the list of the flips, the ratios / the
//                       snapshot, the pick's values, the incumbent's values
// The work slice of a model (PbWork below) and the static LDS record of the counters are those of lpx_packed_bnb.hip.
#define LPX_ONCHIP_GUARD 0
#define LPX_ONCHIP_FIX 0
#include "lpx_onchip.h"        // the launch constants, oc_uniform; through lpx_bounded.h bnd_complement, rs_hysteresis, the reductions

#include <climits>
#include <cstring>
#include <mutex>

namespace lpx {

namespace {

constexpr int PB_RUNNING = -1;                          // the stop word while the search goes on; afterwards an LPX_PBNB_* code

// the counters of one model's search: static LDS, written by lane 0
struct PbState {
    long long nodes, events, flips, incumbents, pruned_bound, pruned_infeasible, pivots;
    double best;
    int sp, depth, max_K, deepest, logged, stop;
};

// the work slice of one model, carved from P.work + model * P.work_stride; every section starts on 8 bytes
struct PbWork {
    double *lo, *root_ub, *cur_ub, *nb_lo, *nb_ub, *shift, *best_x, *path_lo, *path_ub, *stk_lo, *stk_ub;
    int32_t *basis, *path_var, *stk_var, *stk_depth;
    uint8_t* flip;
};

__host__ __device__ inline size_t pb_work_bytes(int m, int n, size_t depth1)
{
    const size_t C = (size_t)n + m + 1, D = (size_t)depth1;
    const size_t doubles = C + 6 * (size_t)n + 4 * D;
    const size_t ints = (((size_t)m + 1) & ~(size_t)1) + 3 * ((D + 1) & ~(size_t)1);
    const size_t bytes = (C + 7) & ~(size_t)7;
    return ((doubles * 8 + ints * 4 + bytes) + 255) & ~(size_t)255;
}

__device__ __forceinline__ PbWork pb_carve(char* base, int m, int n, int depth1)
{
    const size_t C = (size_t)n + m + 1, D = (size_t)depth1, De = (D + 1) & ~(size_t)1;
    PbWork w;
    double* d = reinterpret_cast<double*>(base);
    w.lo = d; d += C;
    w.root_ub = d; d += n; w.cur_ub = d; d += n; w.nb_lo = d; d += n; w.nb_ub = d; d += n; w.shift = d; d += n; w.best_x = d; d += n;
    w.path_lo = d; d += D; w.path_ub = d; d += D; w.stk_lo = d; d += D; w.stk_ub = d; d += D;
    int32_t* i = reinterpret_cast<int32_t*>(d);
    w.basis = i; i += ((size_t)m + 1) & ~(size_t)1;
    w.path_var = i; i += De; w.stk_var = i; i += De; w.stk_depth = i; i += De;
    w.flip = reinterpret_cast<uint8_t*>(i);
    return w;
}

// the log slice of a model behind its first `from` records: zero bits (a record is four doubles wide)
__device__ __forceinline__ void pb_zero_log(const PackedBnbDualParams& P, size_t mdl, int t, int from)
{
    static_assert(sizeof(lpx_bnb_node_log) == 32, "a log record is four doubles wide");
    if (!P.log) return;
    double* z = reinterpret_cast<double*>(P.log + mdl * (size_t)P.log_cap);
    for (long long k = 4ll * from + t; k < 4ll * P.log_cap; k += OC_NT) z[k] = 0.0;
}

// a model that ends in front of the search with an error: zeros around its status, as lpx_solve_packed leaves them
__device__ __forceinline__ void pb_refuse(const PackedBnbDualParams& P, size_t mdl, int t, int n, int code)
{
    double* gx = P.x + mdl * (size_t)n;
    for (int j = t; j < n; j += OC_NT) gx[j] = 0.0;
    pb_zero_log(P, mdl, t, 0);
    if (t == 0) {
        P.status[mdl] = code; P.value[mdl] = 0.0; P.pivots[mdl] = 0;
        lpx_packed_bnb_record* o = P.rec + mdl;
        o->status = code; o->stop = LPX_PBNB_ROOT;
        o->nodes = 0; o->events = 0; o->flips = 0; o->incumbents = 0; o->pruned_bound = 0; o->pruned_infeasible = 0;
        o->max_K = 0; o->deepest = 0; o->root_events = 0; o->logged = 0;
        o->best = -__builtin_inf(); o->constant = 0.0;
    }
}

// lane 0, in front of every node: the limits first, then the pop.  Popping an entry of depth d rewrites path[d - 1].
__device__ __forceinline__ void pb_next(PbState& ss, const PbWork& w, long long max_nodes, long long max_events)
{
    if (ss.sp == 0) { ss.stop = LPX_PBNB_DONE; return; }
    if (ss.nodes >= max_nodes) { ss.stop = LPX_PBNB_NODES; return; }
    if (ss.events >= max_events) { ss.stop = LPX_PBNB_EVENTS; return; }
    const int e = --ss.sp;
    const int d = w.stk_depth[e];
    ss.depth = d;
    if (d > 0) { w.path_var[d - 1] = w.stk_var[e]; w.path_lo[d - 1] = w.stk_lo[e]; w.path_ub[d - 1] = w.stk_ub[e]; }
    ss.nodes++;
}

}  // namespace

__global__ __launch_bounds__(OC_NT) void lpx_packed_bnb_dual_onchip(PackedBnbDualParams P)
{
    constexpr int stall_events = 0;                     // no stall guard here: this line and the file's switch are all of it
    extern __shared__ double pbd_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;
    __shared__ int s_tot[OC_NW];
    __shared__ int s_bad[OC_NW];
    __shared__ double s_const;                          // c.l over the user's c: what the lower shift took out of the optimum
    __shared__ int s_shifted;
    __shared__ PbState ss;

    const int t0 = threadIdx.x;
    const size_t mdl = blockIdx.x;
    const int m = P.m, nv = P.n, R = m + 1, C = nv + m + 1, Cm = C - 1;
    const int S0 = C | 1;
    const double inf = __builtin_inf();
    const double eps = P.eps;
    const int max_iter = P.max_iter;
    const bool min = P.min != 0, has_lower = P.lower != nullptr, has_mask = P.mask != nullptr;

    const double* const gc = P.c + mdl * (size_t)P.c_stride;
    const double* const gA = P.A + mdl * (size_t)P.A_stride;
    const double* const gb = P.b + mdl * (size_t)P.b_stride;
    const double* const glo = has_lower ? P.lower + mdl * (size_t)P.lower_stride : nullptr;
    const double* const gup = P.upper ? P.upper + mdl * (size_t)P.upper_stride : nullptr;
    const int depth1 = P.max_depth + 1;
    const PbWork W = pb_carve(P.work + mdl * (size_t)P.work_stride, m, nv, depth1);
    int32_t* const basis = W.basis; uint8_t* const flip = W.flip;       // the names of the step files
    int32_t* const trace = nullptr; const int trace_cap = 0;
    double* const gx = P.x + mdl * (size_t)nv;

    double* tile = pbd_lds;
    double* ub_s = tile + (size_t)R * S0;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);

    int root_events = 0;
    {
        // ================= a. the root: lpx_packed_dual.hip steps 1, 2b, 5 and 6, with the integer check of ValidateBnbBounded
        // between the bounds check and the rel check
        const int t = t0, lane = t & 63, wave = t >> 6, S = S0;
        const double rtol = P.ratio_tol_root;
        double* zrow = tile + (size_t)m * S;
        const int32_t* const grel = P.rel ? P.rel + mdl * (size_t)P.rel_stride : nullptr;
        int bad = 0;
        for (int j = t; j < nv; j += OC_NT) {
            const double l = has_lower ? glo[j] : 0.0;
            const double u = gup ? gup[j] : inf;
            if (!(__builtin_fabs(l) < inf) || !(u >= l)) bad = 1;
            // an integer variable needs a finite upper bound and integral bounds
            if ((!has_mask || P.mask[j]) && (!(u < inf) || __builtin_floor(l) != l || __builtin_floor(u) != u)) bad = 1;
            buf[j] = l;
            ub_s[j] = gup ? (__builtin_isinf(u) ? u : u - l) : inf;
            double cj = gc[j];
            if (min) cj = -cj;                          // Min negates c ...
            zrow[j] = -cj;                              // ... and the objective row is the negation of that: a zero cost gives -0.0
            flip[j] = 0;
        }
        for (int j = nv + t; j < Cm; j += OC_NT) { ub_s[j] = inf; flip[j] = 0; }
        if (grel)
            for (int i = t; i < m; i += OC_NT) { const int r = grel[i]; if (r != LPX_LE && r != LPX_GE) bad = 1; }
        // A, coalesced over the whole m x n block; a >= row is negated here, in front of the lower shift: only signs change
        {
            const int dr = OC_NT / nv, dc = OC_NT % nv;
            int i = t / nv, j = t % nv;
            for (int k = t; k < m * nv; k += OC_NT) {
                const double a = gA[k];
                const bool ge = grel && grel[i] == LPX_GE;
                tile[(size_t)i * S + j] = ge ? -a : a;
                i += dr; j += dc;
                if (j >= nv) { j -= nv; ++i; }
            }
        }
        for (int k = t; k < R * R; k += OC_NT) {
            const int i = k / R, jj = k - i * R;        // column nv + jj; jj = m is the RHS column
            double v = (i < m && jj == i) ? 1.0 : 0.0;
            if (i < m && jj == m) { const double bi = gb[i]; v = (grel && grel[i] == LPX_GE) ? -bi : bi; }
            tile[(size_t)i * S + nv + jj] = v;
        }
        for (int i = t; i < m; i += OC_NT) basis[i] = nv + i;
        if (__syncthreads_or(bad)) { pb_refuse(P, mdl, t, nv, LPX_EINVAL); return; }    // uniform
        // b' = b - A l over the rows as they are stored; a negative b' is what the dual start is for
        if (has_lower) {
            for (int i = t; i < m; i += OC_NT) {
                const double* row = tile + (size_t)i * S;
                double bi = row[Cm];
                for (int j = 0; j < nv; ++j) {
                    const double l = buf[j];
                    if (l != 0.0) { const double prod = row[j] * l; bi = bi - prod; }
                }
                tile[(size_t)i * S + Cm] = bi;
            }
            if (t == (((m + 63) >> 6) << 6)) {          // the first lane of the first wave without a row
                double constant = 0.0; int shifted = 0;
                for (int j = 0; j < nv; ++j) {
                    const double l = buf[j];
                    if (l != 0.0) { const double cu = min ? zrow[j] : -zrow[j]; const double prod = cu * l; constant = constant + prod; shifted = 1; }
                }
                s_const = constant; s_shifted = shifted;
            }
        } else if (t == 0) { s_const = 0.0; s_shifted = 0; }
        __syncthreads();                                // the tile, ub and the flip bytes stand; the lower bounds in buf are dead

        // ---- 2b. the count of the dual-feasibility flips and of the columns no flip can repair, 5. the flips: both with the
        // tolerance of lpx_tableau_dualize(1e-9), whatever the loop's eps is
        [[maybe_unused]] bool dirty = false;            // a dead local: nothing is stored back
        {
            const double eps = 1e-9;
            int nflips = 0, unrepairable = 0;
            {
#include "lpx_onchip_count.h"
                nflips = n; unrepairable = bad;
            }
            if (unrepairable > 0) { pb_refuse(P, mdl, t, nv, LPX_EINVAL); return; }     // uniform: the precheck of lpx_solve_bounded_dual
#include "lpx_onchip_flips.h"
        }

        // ---- 6. the dual loop from the slack basis: no SKIP_FIXED, no cutoff
        const bool skip_fixed = false, cut = false, long_step = (P.flags & LPX_BDUAL_LONG_STEP) != 0;
        const double cutoff = 0.0;
#include "lpx_onchip_dual.h"
        __syncthreads();                                // basis and flip as lane 0 left them, for every lane
        (void)cutoff;
        status = __builtin_amdgcn_readfirstlane(status);
        root_events = __builtin_amdgcn_readfirstlane(iter);

        if (status != LPX_OPTIMAL) {
            // a root that does not end optimal ends the model with the root's status.  LPX_INFEASIBLE: zeros, the answer of the host
            // driver; LPX_ITER_LIMIT: x and value as lpx_solve_packed_dual extracts them
            const bool infeasible = status == LPX_INFEASIBLE;                          // uniform
            double* v = buf;
            for (int j = t; j < Cm; j += OC_NT) v[j] = 0.0;
            __syncthreads();
            for (int i = t; i < m; i += OC_NT) {
                const int pb = basis[i];
                if ((unsigned)pb < (unsigned)Cm) v[pb] = tile[(size_t)i * S + Cm];
            }
            __syncthreads();
            for (int j = t; j < nv; j += OC_NT) {
                double xj = (flip[j] & 1) ? ub_s[j] - v[j] : v[j];
                if (has_lower) xj = xj + glo[j];
                gx[j] = infeasible ? 0.0 : xj;
            }
            pb_zero_log(P, mdl, t, 0);
            if (t == 0) {
                const double z = zrow[Cm];
                const bool shifted = s_shifted != 0;
                double value = z;
                if (shifted || min) {
                    value = min ? -z : z;
                    if (shifted) value = value + s_const;
                }
                if (infeasible) value = 0.0;
                P.status[mdl] = status; P.value[mdl] = value; P.pivots[mdl] = k0 + k1;
                lpx_packed_bnb_record* o = P.rec + mdl;
                o->status = status; o->stop = LPX_PBNB_ROOT;
                o->nodes = 0; o->events = 0; o->flips = 0; o->incumbents = 0; o->pruned_bound = 0; o->pruned_infeasible = 0;
                o->max_K = 0; o->deepest = 0; o->root_events = root_events; o->logged = 0;
                o->best = -inf; o->constant = s_const;
            }
            return;
        }

        // ================= b. the search starts: the handle's lo, the root and the current bounds, the root node on the stack
        for (int j = t; j < Cm; j += OC_NT) W.lo[j] = 0.0;
        for (int j = t; j < nv; j += OC_NT) { const double u = ub_s[j]; W.root_ub[j] = u; W.cur_ub[j] = u; }
        if (t == 0) {
            ss.nodes = 0; ss.events = 0; ss.flips = 0; ss.incumbents = 0; ss.pruned_bound = 0; ss.pruned_infeasible = 0;
            ss.pivots = k0 + k1;
            ss.best = -inf; ss.sp = 1; ss.depth = 0; ss.max_K = 0; ss.deepest = 0; ss.logged = 0; ss.stop = PB_RUNNING;
            W.stk_depth[0] = 0; W.stk_var[0] = -1; W.stk_lo[0] = 0.0; W.stk_ub[0] = 0.0;
            pb_next(ss, W, P.max_nodes, P.max_events);
        }
    }

    // what the step files expect beside the names above
    const double rtol = P.ratio_tol_node, ptol = 1e-6;
    const int flags = LPX_BDUAL_SKIP_FIXED | P.flags, nint = nv;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;
    const struct { const uint8_t* mask; const double* lo; } N = {P.mask, W.lo};     // lpx_onchip_pick.h reads N.mask and N.lo ...
    const struct { int has_mask; } in_rec = {has_mask ? 1 : 0};
    const auto* const in = &in_rec;                                                  // ... and in->has_mask
    lpx_bnb_node_log* const glog = P.log ? P.log + mdl * (size_t)P.log_cap : nullptr;
    bool lo_used = false;                               // some edit has stored a non-zero lower bound: sticky, as the handle's mark
    [[maybe_unused]] bool dirty = false;                // the step files set it; nothing is stored back here

    for (long long trip = 0; trip <= P.max_nodes; ++trip) {
        __syncthreads();                                // the state record and the path as lane 0 left them
        if (__builtin_amdgcn_readfirstlane(ss.stop) != PB_RUNNING) break;
        // The row stride and the lane number go through an empty asm once per node, as in the plunge: the compiler then forms the
        // row addresses and the lane predicates of every step inside the node and does not carry them across the whole search.
        int S = S0, t = t0;
        asm volatile("" : "+s"(S), "+v"(t));
        const int lane = t & 63, wave = t >> 6;
        double* zrow = tile + (size_t)m * S;
        const int depth = __builtin_amdgcn_readfirstlane(ss.depth);
        const double best = oc_uniform(ss.best);
        const double cutoff = cut ? best + 1e-6 : 0.0;

        // ---- 1. the bounds of the node from its path over the root bounds [0, u']: lane 0 applies the overrides in order (a
        // variable may stand on the path more than once, the deepest entry holds)
        for (int j = t; j < nv; j += OC_NT) { W.nb_lo[j] = 0.0; W.nb_ub[j] = W.root_ub[j]; }
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < depth; ++k) { const int v = W.path_var[k]; W.nb_lo[v] = W.path_lo[k]; W.nb_ub[v] = W.path_ub[k]; }
        __syncthreads();

        // ---- 2. the columns whose bounds differ from those on the tile, in ascending order: a ballot per wave, a prefix over the
        // wave totals (the current lower bounds are lo itself)
        int K = 0;
        for (int base = 0; base < nv; base += OC_NT) {  // uniform trip count
            const int j = base + t;
            bool in_l = false;
            if (j < nv) in_l = W.nb_lo[j] != W.lo[j] || W.nb_ub[j] != W.cur_ub[j];
            const unsigned long long mi = __ballot(in_l);
            const int before = __popcll(mi & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) s_tot[wave] = __popcll(mi);
            __syncthreads();
            int pre = 0, tot = 0;
            for (int w = 0; w < OC_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
            if (in_l) list[K + pre + before] = j;       // K + pre + before < columns tested so far <= nv
            K += tot;
        }
        K = __builtin_amdgcn_readfirstlane(K);
        __syncthreads();

        // ---- 3. the edit, lpx_bounded_node_body.h step 2 on the tile's own ub: +inf on a flipped column refuses; then the shifts,
        // the new ub / lo and the current upper bounds (the columns are distinct)
        int refuse = 0, any_lo = 0;
        for (int k = t; k < K; k += OC_NT) {
            const int j = list[k];
            if (W.nb_ub[j] == inf && flip[j]) refuse = 1;
        }
        refuse = __syncthreads_or(refuse);
        if (!refuse) {
            for (int k = t; k < K; k += OC_NT) {
                const int j = list[k];
                const double lw = W.nb_lo[j], up = W.nb_ub[j];
                const double uj = ub_s[j], lj = W.lo[j];
                const double l1 = lw - lj;
                const double u1 = up - lj;              // +inf stays +inf
                W.shift[k] = flip[j] ? uj - u1 : l1;
                const double nu = up - lw;
                ub_s[j] = nu;
                W.lo[j] = lw; W.cur_ub[j] = up;
                if (lw != 0.0) any_lo = 1;
            }
            if (__syncthreads_or(any_lo)) lo_used = true;
        }
        int nflips = 0;
        if (!refuse) {
            // ---- 2b. the count of the flips and of the columns no flip can repair
#include "lpx_onchip_count.h"
            n = __builtin_amdgcn_readfirstlane(n); bad = __builtin_amdgcn_readfirstlane(bad);
            nflips = n;
            if (bad > 0) refuse = 1;
        }
        if (refuse) {                                   // uniform: the host driver throws here; the model ends LPX_EINVAL
            if (t == 0) ss.stop = LPX_PBNB_REFUSED;
            break;
        }

        // ---- 4. the RHS shifts of the edit, k in order: a lane per row
        if (K > 0) {
            for (int i = t; i < R; i += OC_NT) {
                double* row = tile + (size_t)i * S;
                double b = row[Cm];
                for (int k = 0; k < K; ++k) {
                    const double sh = W.shift[k];
                    if (sh == 0.0) continue;
                    const double prod = sh * row[list[k]];
                    b = b - prod;
                }
                row[Cm] = b;
            }
            __syncthreads();
        }

        // ---- 5. the dual-feasibility flips, 6. the dual loop
#include "lpx_onchip_flips.h"
#include "lpx_onchip_dual.h"
        __syncthreads();                                // basis and flip as lane 0 left them, for every lane

        // ---- 7. the branch pick
        int var = -1, total = 0;
        double x_var = 0.0;
#include "lpx_onchip_pick.h"

        // ---- 8. the decide step of SolveBnbBounded.  Every lane holds the same values; lane 0 keeps the books.
        const double z = oc_uniform(zrow[Cm]);
        var = __builtin_amdgcn_readfirstlane(var); x_var = oc_uniform(x_var);
        const int st = __builtin_amdgcn_readfirstlane(status), ev = __builtin_amdgcn_readfirstlane(iter);
        const int piv = __builtin_amdgcn_readfirstlane(k0 + k1);
        __syncthreads();                                // the pick's values are free
        const bool limit = st == LPX_ITER_LIMIT;
        const bool infeasible = !limit && st == LPX_INFEASIBLE;
        const bool bound = !limit && !infeasible && (st == LPX_CUTOFF || z <= best + 1e-6);
        const bool incumbent = !limit && !infeasible && !bound && var < 0;
        if (incumbent) {
            // x' as lpx_tableau_bounded_solution forms it, its integer entries rounded half to even
            double* v = buf;
            for (int j = t; j < Cm; j += OC_NT) v[j] = 0.0;
            __syncthreads();
            for (int i = t; i < m; i += OC_NT) {
                const int pb = basis[i];
                if ((unsigned)pb < (unsigned)Cm) v[pb] = tile[(size_t)i * S + Cm];
            }
            __syncthreads();
            for (int j = t; j < nv; j += OC_NT) {
                double xj = flip[j] ? ub_s[j] - v[j] : v[j];
                if (lo_used) xj = xj + W.lo[j];
                if (!has_mask || P.mask[j]) xj = __builtin_rint(xj);
                W.best_x[j] = xj;
            }
        }
        if (t == 0) {
            ss.events += ev; ss.flips += nflips; ss.pivots += piv;
            if (K > ss.max_K) ss.max_K = K;
            if (depth > ss.deepest) ss.deepest = depth;
            if (ss.logged < P.log_cap) {
                lpx_bnb_node_log* lg = glog + ss.logged++;
                lg->depth = depth; lg->K = K; lg->status = st; lg->events = ev; lg->flips = nflips; lg->var = var; lg->z = z;
            }
            if (limit) ss.stop = LPX_PBNB_NODE_ITER;
            else if (infeasible) ss.pruned_infeasible++;
            else if (bound) ss.pruned_bound++;
            else if (incumbent) { ss.best = z; ss.incumbents++; }
            // a child at depth + 1 needs max_depth >= depth + 1; the stack then holds at most one sibling per depth 1..depth beside
            // the two pushed, so sp + 2 <= max_depth + 1 follows -- tested all the same, it guards the stores below
            else if (depth + 1 > P.max_depth || ss.sp + 2 > P.max_depth + 1) ss.stop = LPX_PBNB_DEPTH;
            else {                                      // the floor child, then the ceil child, which is explored first
                const int e = ss.sp;
                W.stk_depth[e] = depth + 1; W.stk_var[e] = var; W.stk_lo[e] = W.nb_lo[var]; W.stk_ub[e] = __builtin_floor(x_var);
                W.stk_depth[e + 1] = depth + 1; W.stk_var[e + 1] = var; W.stk_lo[e + 1] = __builtin_ceil(x_var); W.stk_ub[e + 1] = W.nb_ub[var];
                ss.sp = e + 2;
            }
            if (ss.stop == PB_RUNNING) pb_next(ss, W, P.max_nodes, P.max_events);
        }
    }
    __syncthreads();

    // ================= d. the end, as FinishBnbResult
    {
        const int t = t0;
        int stop = __builtin_amdgcn_readfirstlane(ss.stop);
        if (stop == PB_RUNNING) stop = LPX_PBNB_NODES;  // the loop's own bound: cannot be reached, lane 0 stops at max_nodes
        const bool have = ss.incumbents > 0;
        const double best = ss.best;
        int status = LPX_ITER_LIMIT;
        if (stop == LPX_PBNB_DONE) status = have ? LPX_OPTIMAL : LPX_INFEASIBLE;
        if (stop == LPX_PBNB_REFUSED) status = LPX_EINVAL;
        for (int j = t; j < nv; j += OC_NT) {
            double xj = 0.0;
            if (have) { xj = W.best_x[j]; if (has_lower) xj = xj + glo[j]; }
            gx[j] = xj;
        }
        pb_zero_log(P, mdl, t, __builtin_amdgcn_readfirstlane(ss.logged));
        if (t == 0) {
            double value = 0.0;
            if (have) {
                value = min ? -best : best;
                if (s_shifted != 0) value = value + s_const;
            }
            P.status[mdl] = status; P.value[mdl] = value; P.pivots[mdl] = ss.pivots;
            lpx_packed_bnb_record* o = P.rec + mdl;
            o->status = status; o->stop = stop;
            o->nodes = ss.nodes; o->events = ss.events; o->flips = ss.flips; o->incumbents = ss.incumbents;
            o->pruned_bound = ss.pruned_bound; o->pruned_infeasible = ss.pruned_infeasible;
            o->max_K = ss.max_K; o->deepest = ss.deepest; o->root_events = root_events; o->logged = ss.logged;
            o->best = best; o->constant = s_const;
        }
    }
}

// ---- the host side of a call: the arena, the stream and the pinned block of lpx_packed.hip (PackedArena, lpx_internal.h) --------
namespace {

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int packed_bnb_dual_solve(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out, lpx_stats* st)
{
    int rc = ensure_device(); if (rc) return rc;
    const size_t count = (size_t)in->count, m = (size_t)in->m, n = (size_t)in->n;
    const int R = in->m + 1, C = in->n + in->m + 1;
    if (!bounded_node_fits(R, C) || in->m > OC_NT - 64) { set_error("lpx_solve_packed_bnb_dual: the shape does not fit"); return LPX_EINVAL; }   // never launched beyond one compute unit
    const int max_depth = opt->max_depth > 0 ? opt->max_depth : in->n;
    const size_t log_cap = (size_t)opt->log_cap;

    std::lock_guard<std::mutex> lock(g_packed.mu);
    PackedArena& a = g_packed;
    if (!a.stream) LPX_HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    if (!a.attr_bnb_dual) { LPX_HIP_TRY(oc_allow_lds(reinterpret_cast<const void*>(lpx_packed_bnb_dual_onchip))); a.attr_bnb_dual = true; }

    // the arena: the inputs (a shared array once), rel and the mask, the results in the order of the pinned block, the work slices
    auto models = [&](int64_t stride) { return stride == 0 ? (size_t)1 : count; };
    const size_t in_bytes[7] = {sizeof(double) * n * models(in->c_stride), sizeof(double) * m * n * models(in->A_stride),
                                sizeof(double) * m * models(in->b_stride), in->lower ? sizeof(double) * n * models(in->lower_stride) : 0,
                                in->upper ? sizeof(double) * n * models(in->upper_stride) : 0,
                                in->rel ? sizeof(int32_t) * m * models(in->rel_stride) : 0, in->is_int ? n : 0};
    const void* in_src[7] = {in->c, in->A, in->b, in->lower, in->upper, in->rel, in->is_int};
    const size_t out_bytes[6] = {sizeof(double) * count * n, sizeof(double) * count, sizeof(lpx_packed_bnb_record) * count,
                                 sizeof(int32_t) * count, sizeof(int64_t) * count,
                                 sizeof(lpx_bnb_node_log) * count * log_cap};              // x, value, rec, status, pivots, log
    size_t in_off[7], out_off[6], at = 0;
    for (int k = 0; k < 7; ++k) { in_off[k] = at; at += up256(in_bytes[k]); }
    const size_t res0 = at;
    for (int k = 0; k < 6; ++k) { out_off[k] = at; at += up256(out_bytes[k]); }
    const size_t res_bytes = at - res0;
    const size_t work_stride = pb_work_bytes(in->m, in->n, (size_t)max_depth + 1);
    const size_t work_off = at; at += count * work_stride;
    if (at > a.dev_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.dev) hipFree(a.dev);
        a.dev = nullptr; a.dev_bytes = 0;
        LPX_HIP_TRY(hipMalloc((void**)&a.dev, at));
        a.dev_bytes = at;
    }
    if (res_bytes > a.pin_bytes) {
        LPX_HIP_TRY(hipStreamSynchronize(a.stream));
        if (a.pin) hipHostFree(a.pin);
        a.pin = nullptr; a.pin_bytes = 0;
        LPX_HIP_TRY(hipHostMalloc((void**)&a.pin, res_bytes));
        a.pin_bytes = res_bytes;
    }

    lpx_run_opts no;
    lpx_default_opts(&no, 1);
    PackedBnbDualParams p;
    std::memset(&p, 0, sizeof(p));
    p.c = reinterpret_cast<const double*>(a.dev + in_off[0]); p.A = reinterpret_cast<const double*>(a.dev + in_off[1]);
    p.b = reinterpret_cast<const double*>(a.dev + in_off[2]);
    p.lower = in->lower ? reinterpret_cast<const double*>(a.dev + in_off[3]) : nullptr;
    p.upper = in->upper ? reinterpret_cast<const double*>(a.dev + in_off[4]) : nullptr;
    p.rel = in->rel ? reinterpret_cast<const int32_t*>(a.dev + in_off[5]) : nullptr;
    p.mask = in->is_int ? reinterpret_cast<const uint8_t*>(a.dev + in_off[6]) : nullptr;
    p.c_stride = in->c_stride; p.A_stride = in->A_stride; p.b_stride = in->b_stride;
    p.lower_stride = in->lower_stride; p.upper_stride = in->upper_stride; p.rel_stride = in->rel_stride;
    p.m = in->m; p.n = in->n; p.min = in->sense == LPX_MIN ? 1 : 0; p.max_iter = opt->max_iter;
    p.flags = opt->search_flags; p.max_depth = max_depth; p.log_cap = opt->log_cap;
    p.max_nodes = opt->max_nodes; p.max_events = opt->max_events;
    p.eps = no.eps; p.ratio_tol_root = no.ratio_tol; p.ratio_tol_node = no.ratio_tol;   // the root is a dual loop too
    p.x = reinterpret_cast<double*>(a.dev + out_off[0]); p.value = reinterpret_cast<double*>(a.dev + out_off[1]);
    p.rec = reinterpret_cast<lpx_packed_bnb_record*>(a.dev + out_off[2]); p.status = reinterpret_cast<int32_t*>(a.dev + out_off[3]);
    p.pivots = reinterpret_cast<long long*>(a.dev + out_off[4]);
    p.log = log_cap ? reinterpret_cast<lpx_bnb_node_log*>(a.dev + out_off[5]) : nullptr;
    p.work = a.dev + work_off; p.work_stride = (int64_t)work_stride;

    const double t0 = now_ms();
    for (int k = 0; k < 7; ++k)
        if (in_bytes[k]) LPX_HIP_TRY(hipMemcpyAsync(a.dev + in_off[k], in_src[k], in_bytes[k], hipMemcpyHostToDevice, a.stream));
    hipLaunchKernelGGL(lpx_packed_bnb_dual_onchip, dim3((unsigned)count), dim3(OC_NT), bounded_node_lds_bytes(R, C), a.stream, p);
    LPX_HIP_TRY(hipGetLastError());
    LPX_HIP_TRY(hipMemcpyAsync(a.pin, a.dev + res0, res_bytes, hipMemcpyDeviceToHost, a.stream));
    LPX_HIP_TRY(hipStreamSynchronize(a.stream));       // the one wait
    const double ms = now_ms() - t0;

    const char* res = a.pin - res0;
    std::memcpy(out->x, res + out_off[0], out_bytes[0]);
    std::memcpy(out->value, res + out_off[1], out_bytes[1]);
    std::memcpy(out->status, res + out_off[3], out_bytes[3]);
    if (out->rec) std::memcpy(out->rec, res + out_off[2], out_bytes[2]);
    if (out->log && log_cap) std::memcpy(out->log, res + out_off[5], out_bytes[5]);
    if (st) {
        const long long* pv = reinterpret_cast<const long long*>(res + out_off[4]);
        std::memset(st, 0, sizeof(*st));
        for (size_t i = 0; i < count; ++i) st->pivots += pv[i];
        st->launches = 1; st->loop_ms = ms;
    }
    return 0;
}

}  // namespace lpx
