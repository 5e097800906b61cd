// lpx_model_api.cpp -- model-level C ABI (lpx_solve, lpx_parse_text) over the C++ host mirror.
#include "lpx_internal.h"
#include "host/model.h"
#include "../../include/lpx_test.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace lpx;
using namespace lpx::host;

namespace lpx { bool comm_active(int* rank, int* world); }

namespace {

char* dup_str(const std::string& s) { char* p = (char*)std::malloc(s.size() + 1); std::memcpy(p, s.c_str(), s.size() + 1); return p; }
template <class T> T* dup_vec(const std::vector<T>& v) {
    T* p = (T*)std::malloc(sizeof(T) * (v.size() ? v.size() : 1));
    if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}

LPProblem to_problem(const lpx_problem* p)
{
    LPProblem q;
    q.ObjectiveSense = p->sense == LPX_MIN ? Sense::Min : Sense::Max;
    q.C.assign(p->c, p->c + p->n);
    for (int i = 0; i < p->m; ++i) {
        Constraint c;
        c.A.assign(p->A + (size_t)i * p->n, p->A + (size_t)(i + 1) * p->n);
        c.Relation = p->rel[i] == LPX_GE ? Rel::GE : (p->rel[i] == LPX_EQ ? Rel::EQ : Rel::LE);
        c.B = p->b[i];
        q.Constraints.push_back(std::move(c));
    }
    return q;
}

}  // namespace

// test-only stand-ins for the device loops (include/lpx_test.h); never set by a product path
static thread_local lpx_test_seams g_seams = {nullptr, nullptr, nullptr, 0};
extern "C" void lpx_test_set_seams(const lpx_test_seams* s)
{
    if (s) g_seams = *s; else g_seams = lpx_test_seams{nullptr, nullptr, nullptr, 0};
}

static EngineOptions to_engine(const lpx_solve_opts* o)
{
    EngineOptions e;
    e.max_iter = o->max_iter > 0 ? o->max_iter : 10000;
    e.batch = o->batch; e.render_iterations = o->render_iterations != 0;
    e.dual_flags = o->dual_flags; e.bnb_mode = o->bnb_mode; e.bnb_search = o->bnb_search;
    e.concurrent_nodes = o->concurrent_nodes > 0 ? o->concurrent_nodes : 1;
    e.rank = o->rank; e.world = o->world > 0 ? o->world : 1; e.max_nodes = o->max_nodes;
    e.bnb_dive = o->bnb_dive;
    if (o->allreduce_max) {
        auto fn = o->allreduce_max; void* u = o->allreduce_user;
        e.allreduce_max = [fn, u](double* v, int n) { fn(u, v, n); };
    } else {
        // no host callback: the library's own RCCL communicator (lpx_comm_init) carries the exchange
        int crank = 0, cworld = 0;
        if (comm_active(&crank, &cworld)) {
            if (e.world != cworld || e.rank != crank)
                throw LpxException(LPX_EINVAL, "lpx_solve: opts.rank / opts.world (" + std::to_string(e.rank) + " / " + std::to_string(e.world) +
                                               ") differ from the communicator's (" + std::to_string(crank) + " / " + std::to_string(cworld) + ")");
            e.allreduce_max = [](double* v, int n) {
                const int rc = lpx_comm_allreduce_max(v, n);
                if (rc) { char b[512]; lpx_last_error(b, sizeof(b)); throw LpxException(rc, std::string("liblpx: ") + b); }
            };
            // LPX_COMM_SHARD_ONE=1 (diagnostic): a world of ONE still runs the sharded code path -- hand-out, one all-reduce per
            // level / round through RCCL, publication of x -- so that path can be exercised on a single GPU
            static const bool shard_one = [] { const char* v = std::getenv("LPX_COMM_SHARD_ONE"); return v && v[0] == '1'; }();
            e.shard_one = shard_one && cworld == 1;
        }
    }
    if (g_seams.node_lp) {
        auto fn = g_seams.node_lp; void* u = g_seams.user;
        e.test_node_lp = [fn, u](double* T, int R, int C, int32_t* basis, int dual, int repaired, int max_iter, int nvars,
                                 double* x, double* z, int64_t* pivots) { return fn(u, T, R, C, basis, dual, repaired, max_iter, nvars, x, z, pivots); };
    }
    e.test_fail_after_nodes = g_seams.fail_after_nodes;
    if (g_seams.knap_relax) {
        auto fn = g_seams.knap_relax; void* u = g_seams.user;
        e.test_knap_relax = [fn, u](int count, const int32_t* off, const int32_t* fidx, const int8_t* fval, double* profit,
                                    double* weight, int32_t* frac, double* fracval) { return fn(u, count, off, fidx, fval, profit, weight, frac, fracval); };
    }
    return e;
}

static UpdatePivot to_callback(const lpx_solve_opts* o)
{
    UpdatePivot cb;
    if (o->text_cb) {
        auto fn = o->text_cb; void* u = o->text_user;
        cb = [fn, u](const std::string& text, const Highlight* h) {
            fn(u, text.c_str(), h ? h->cells.data() : nullptr, h ? h->R : 0, h ? h->C : 0);
        };
    }
    return cb;
}

static void fill_result(lpx_result* out, const SimplexResult& r, int nvars)
{
    out->status = r.Status;
    out->has_solution = r.HasSolution ? 1 : 0;
    out->optimal_value = r.OptimalValue;
    out->n = (int)r.Solution.size(); out->x = dup_vec(r.Solution);
    out->R = r.R; out->C = r.C; out->T = dup_vec(r.Tableau);
    out->basis = dup_vec(r.Basis);
    out->n_pivots = (int)(r.Trace.size() / 2); out->trace = dup_vec(r.Trace);
    out->report = dup_str(r.Report); out->summary = dup_str(r.Summary);
    out->lp_solves = r.LpSolves; out->nodes = r.Nodes;
    out->n_log = (int)(r.NodeLog.size() / 3); out->node_log = dup_vec(r.NodeLog); out->node_z = dup_vec(r.NodeZ);
    for (size_t i = 0; i < 4 && i < r.NodeZ.size() && r.NodeLog.empty(); ++i) out->aux[i] = r.NodeZ[i];
    for (size_t i = 0; i < 4 && i < r.Aux.size(); ++i) out->aux[i] = r.Aux[i];
    out->stats = r.Stats;
    out->n_cuts = nvars >= 0 ? (int)(r.Cuts.size() / (size_t)(nvars + 1)) : 0; out->cuts = dup_vec(r.Cuts);
}

// ---- SensitivityAnalysis over caller-owned arrays (include/lpx.h) -----------------------------------------
namespace {
struct SensCtx {
    LPProblem q; SimplexResult r;
    SensCtx(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis)
    {
        q = to_problem(p);
        r.HasSolution = T != nullptr;
        if (T && R > 0 && C > 0) r.Tableau.assign(T, T + (size_t)R * C);
        r.R = R; r.C = C;
        if (basis && R > 1) r.Basis.assign(basis, basis + (R - 1));
        const int n = p->n, ns = C - 1 - n;                       // VarNames as BuildTableau names them, PrimalSimplex.cs:200-201
        for (int j = 0; j < n; ++j) r.VarNames.push_back("x" + std::to_string(j + 1));
        for (int j = 0; j < ns; ++j) r.VarNames.push_back("c" + std::to_string(j + 1));
    }
};
int copy_out(const std::string& s, char* buf, int len)
{
    if (buf && len > 0) { std::strncpy(buf, s.c_str(), (size_t)len - 1); buf[len - 1] = 0; }
    return (int)s.size();
}
template <class F> int guarded(const char* what, F&& f)
{
    try { return f(); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    catch (const std::exception& ex) { set_error(std::string(what) + ": " + ex.what()); return LPX_EINVAL; }
}
}  // namespace

// ---- ranging in user terms, shared by lpx_solve_ranging and lpx_session_ranging -----------------------------------------
namespace lpx { namespace host {

void RangingAlloc(lpx_ranging* rg, int n, int m)
{
    const double nan = std::nan(""), inf = HUGE_VAL;
    auto alloc = [](int k, auto fill) { using V = decltype(fill); V* a = (V*)std::malloc(sizeof(V) * (k > 0 ? k : 1)); for (int i = 0; i < k; ++i) a[i] = fill; return a; };
    rg->n = n; rg->m = m; rg->valid = 0; rg->min_rhs = inf; rg->min_dj = inf;
    rg->cost_lo = alloc(n, nan); rg->cost_hi = alloc(n, nan); rg->cost_lo_at = alloc(n, (int32_t)-1); rg->cost_hi_at = alloc(n, (int32_t)-1);
    rg->reduced_cost = alloc(n, nan);
    rg->rhs_lo = alloc(m, nan); rg->rhs_hi = alloc(m, nan); rg->rhs_lo_at = alloc(m, (int32_t)-1); rg->rhs_hi_at = alloc(m, (int32_t)-1);
    rg->dual = alloc(m, nan);
}

void RangeTableau(lpx_tableau* t, const RangingMap& map, RawRanging& raw)
{
    auto chk = [](int rc) { if (rc) { char b[1024]; lpx_last_error(b, sizeof b); throw LpxException(rc, std::string("liblpx: ") + b); } };
    int R = 0, C = 0;
    chk(lpx_tableau_shape(t, &R, &C, nullptr));
    const int mx = R - 1, Cm = C - 1;
    raw.ci.resize(Cm); raw.cd.resize(Cm); raw.cia.resize(Cm); raw.cda.resize(Cm); raw.dj.resize(Cm);
    raw.ri.resize(mx); raw.rd.resize(mx); raw.ria.resize(mx); raw.rda.resize(mx); raw.basis.resize(mx);
    raw.pa.clear(); raw.pb.clear();
    raw.pair_of.assign(map.q->Constraints.size(), -1);
    const int nk = (int)map.row_of.size();
    for (int k = 0; k + 1 < nk; ++k)
        if (map.row_of[k] == map.row_of[k + 1]) {
            raw.pair_of[map.row_of[k]] = (int)raw.pa.size();
            raw.pa.push_back(map.slack_col[k]); raw.pb.push_back(map.slack_col[k + 1]); ++k;
        }
    chk(lpx_tableau_ranging(t, 1e-9, raw.ci.data(), raw.cia.data(), raw.cd.data(), raw.cda.data(), raw.ri.data(), raw.ria.data(),
                            raw.rd.data(), raw.rda.data(), &raw.min_rhs, &raw.min_dj));
    const int K = (int)raw.pa.size();
    raw.pi.resize(K); raw.pd.resize(K); raw.pia.resize(K); raw.pda.resize(K);
    chk(lpx_tableau_ranging_pairs(t, 1e-9, K, raw.pa.data(), raw.pb.data(), raw.pi.data(), raw.pia.data(), raw.pd.data(), raw.pda.data()));
    chk(lpx_tableau_basis(t, raw.basis.data()));
    void* dT = nullptr; int ld = 0;
    chk(lpx_tableau_device_ptr(t, &dT, &ld));
    if (hipMemcpy(raw.dj.data(), (const double*)dT + (size_t)mx * ld, sizeof(double) * Cm, hipMemcpyDeviceToHost) != hipSuccess)
        throw LpxException(LPX_EDEVICE, "ranging: objective row download failed");
}

void RangingToUser(const RangingMap& map, const RawRanging& raw, int status, lpx_ranging* rg)
{
    const double inf = HUGE_VAL;
    rg->min_rhs = raw.min_rhs; rg->min_dj = raw.min_dj;
    if (!(status == LPX_OPTIMAL && raw.min_rhs >= -1e-9 && raw.min_dj >= -1e-9)) return;
    rg->valid = 1;
    const LPProblem& q = *map.q;
    const int n = (int)map.var_col.size(), mx = (int)map.row_of.size();
    const double sigma = q.ObjectiveSense == Sense::Min ? -1.0 : 1.0;
    const std::vector<double>& dj = raw.dj; const std::vector<int32_t>& basis = raw.basis;
    std::vector<int> var_of_col(dj.size(), -1), row_of_var(n, -1);
    for (int j = 0; j < n; ++j) var_of_col[map.var_col[j]] = j;
    for (int k = 0; k < mx; ++k) if (basis[k] >= 0 && basis[k] < (int)dj.size() && var_of_col[basis[k]] >= 0) row_of_var[var_of_col[basis[k]]] = k;
    for (int j = 0; j < n; ++j) {
        const double c = q.C[j];
        const int k = row_of_var[j], col = map.var_col[j];
        if (k < 0) {
            const double dp = dj[col] > 0 ? dj[col] : 0.0;
            if (sigma > 0) { rg->cost_lo[j] = -inf; rg->cost_hi[j] = c + dp; rg->cost_hi_at[j] = col; }
            else           { rg->cost_lo[j] = c - dp; rg->cost_hi[j] = inf; rg->cost_lo_at[j] = col; }
            rg->reduced_cost[j] = -sigma * dj[col];
        } else {
            const double up = sigma > 0 ? raw.ri[k] : raw.rd[k], dn = sigma > 0 ? raw.rd[k] : raw.ri[k];
            rg->cost_lo[j] = c - dn; rg->cost_hi[j] = c + up;
            rg->cost_lo_at[j] = sigma > 0 ? raw.rda[k] : raw.ria[k];
            rg->cost_hi_at[j] = sigma > 0 ? raw.ria[k] : raw.rda[k];
            rg->reduced_cost[j] = 0.0;
        }
    }
    auto leaving = [&](int32_t r) { return r >= 0 ? basis[r] : (int32_t)-1; };
    for (int k = 0; k < mx; ++k) {
        const int i = map.row_of[k];
        const double b = q.Constraints[i].B;
        if (raw.pair_of[i] >= 0) {
            if (map.sign[k] < 0) continue;
            const int h = raw.pair_of[i], s1 = raw.pa[h], s2 = raw.pb[h];
            rg->rhs_lo[i] = b - raw.pd[h]; rg->rhs_hi[i] = b + raw.pi[h];
            rg->rhs_lo_at[i] = leaving(raw.pda[h]); rg->rhs_hi_at[i] = leaving(raw.pia[h]);
            rg->dual[i] = sigma * (dj[s1] - dj[s2]);
        } else {
            const int s = map.slack_col[k];
            const bool pos = map.sign[k] > 0;
            rg->rhs_lo[i] = b - (pos ? raw.cd[s] : raw.ci[s]); rg->rhs_hi[i] = b + (pos ? raw.ci[s] : raw.cd[s]);
            rg->rhs_lo_at[i] = leaving(pos ? raw.cda[s] : raw.cia[s]); rg->rhs_hi_at[i] = leaving(pos ? raw.cia[s] : raw.cda[s]);
            rg->dual[i] = sigma * map.sign[k] * dj[s];
        }
    }
}

}}  // namespace lpx::host

extern "C" {

void lpx_default_solve_opts(lpx_solve_opts* o)
{
    std::memset(o, 0, sizeof(*o));
    o->max_iter = 10000; o->concurrent_nodes = 1; o->world = 1;
}

int lpx_solve(const lpx_problem* p, const char* algorithm, const lpx_solve_opts* o, lpx_result* out)
{
    if (!p || !algorithm || !out) { set_error("lpx_solve: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    try {
        EngineOptions e = to_engine(o);
        UpdatePivot cb = to_callback(o);
        LPProblem q = to_problem(p);
        SimplexResult r;
        // Form1.btnSolve_Click (Form1.cs:249-261) builds the two cutting-plane solvers itself; LPSolver does not
        // know them (Models/LPSolver.cs:18-43), so they are routed here and not in the LPSolver mirror.
        const std::string key = LPSolver::NormalizeAlgorithmKey(algorithm);
        if (key == "cutting plane") r = CuttingPlane(e).Solve(q, cb);
        else if (key == "revised cutting plane" || key == "cutting plane revised") r = CuttingPlaneRevised(e).Solve(q, cb);
        // not in the reference: the device GMI loop (lpx_solve_cuts) with default options
        else if (key == "gmi cutting plane" || key == "gmi") r = GmiCuttingPlane(e).Solve(q, cb);
        else r = LPSolver(e).Solve(q, algorithm, cb);
        fill_result(out, r, p->n);
        return 0;
    } catch (const LpxException& ex) {
        set_error(ex.what());
        return ex.code;
    } catch (const std::exception& ex) {
        set_error(std::string("lpx_solve: ") + ex.what());
        return LPX_EINVAL;
    }
}

// lpx_solve_bounded (dual_start = false) and lpx_solve_bounded_dual (true, with the dual loop's flags) in one body
static int solve_bounded(const lpx_problem* p, const double* lower, const double* upper, bool dual_start, int flags, const lpx_solve_opts* o,
                         lpx_result* out, lpx_bounded_info* info, const char* what, int form = -1)      // form: lpx_solve_bounded2
{
    if (!p || !out) { set_error(std::string(what) + ": null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    if (info) std::memset(info, 0, sizeof(*info));
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    try {
        EngineOptions e = to_engine(o);
        UpdatePivot cb = to_callback(o);
        LPProblem q = to_problem(p);
        std::vector<double> lo, up;
        if (lower) lo.assign(lower, lower + p->n);
        if (upper) up.assign(upper, upper + p->n);
        BoundedInfo bi;
        SimplexResult r = dual_start ? SolveBoundedDual(q, lo, up, flags, e, cb, &bi) : SolveBounded(q, lo, up, e, cb, &bi, nullptr, form);
        fill_result(out, r, p->n);
        if (info) {
            info->ncols = (int)bi.ub.size(); info->n = p->n;
            info->flip = dup_vec(bi.flip); info->ub = dup_vec(bi.ub); info->lower = dup_vec(bi.lower);
        }
        return 0;
    } catch (const LpxException& ex) {
        set_error(ex.what());
        return ex.code;
    } catch (const std::exception& ex) {
        set_error(std::string(what) + ": " + ex.what());
        return LPX_EINVAL;
    }
}

int lpx_solve_bounded(const lpx_problem* p, const double* lower, const double* upper, const lpx_solve_opts* o, lpx_result* out,
                      lpx_bounded_info* info)
{
    return solve_bounded(p, lower, upper, false, 0, o, out, info, "lpx_solve_bounded");
}

int lpx_solve_bounded_dual(const lpx_problem* p, const double* lower, const double* upper, int flags, const lpx_solve_opts* o,
                           lpx_result* out, lpx_bounded_info* info)
{
    return solve_bounded(p, lower, upper, true, flags, o, out, info, "lpx_solve_bounded_dual");
}

// ---- the bounded primal loop with its form, and a batch of models in one launch (host/bounded.cpp) ---------------------------
int lpx_solve_bounded2(const lpx_problem* p, const double* lower, const double* upper, const lpx_solve_opts* o, int form, lpx_result* out,
                       lpx_bounded_info* info)
{
    if (form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO) { set_error("lpx_solve_bounded2: unknown form"); return LPX_EINVAL; }
    return solve_bounded(p, lower, upper, false, 0, o, out, info, "lpx_solve_bounded2", form);
}

int lpx_solve_bounded_batch(int count, const lpx_problem* const* problems, const double* const* lowers, const double* const* uppers,
                            const lpx_solve_opts* o, lpx_result* outs, lpx_bounded_info* infos)
{
    const char* what = "lpx_solve_bounded_batch";
    if (count < 1 || count > 1024) { set_error(std::string(what) + ": count is outside [1, 1024]"); return LPX_EINVAL; }
    if (!problems || !outs) { set_error(std::string(what) + ": null argument"); return LPX_EINVAL; }
    for (int i = 0; i < count; ++i)
        if (!problems[i]) { set_error(std::string(what) + ": model " + std::to_string(i) + ": null problem"); return LPX_EINVAL; }
    std::memset(outs, 0, sizeof(*outs) * (size_t)count);
    if (infos) std::memset(infos, 0, sizeof(*infos) * (size_t)count);
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    if (o->text_cb) { set_error(std::string(what) + ": the on-chip form has no per-event callback (text_cb)"); return LPX_EINVAL; }
    return guarded(what, [&]() -> int {
        EngineOptions e = to_engine(o);
        std::vector<LPProblem> qs; qs.reserve((size_t)count);
        std::vector<const LPProblem*> qp;
        std::vector<std::vector<double>> lo((size_t)count), up((size_t)count);
        for (int i = 0; i < count; ++i) {
            qs.push_back(to_problem(problems[i]));
            if (lowers && lowers[i]) lo[i].assign(lowers[i], lowers[i] + problems[i]->n);
            if (uppers && uppers[i]) up[i].assign(uppers[i], uppers[i] + problems[i]->n);
        }
        for (int i = 0; i < count; ++i) qp.push_back(&qs[i]);
        std::vector<SimplexResult> rs; std::vector<BoundedInfo> bis;
        SolveBoundedBatch(qp, lo, up, e, rs, bis);
        for (int i = 0; i < count; ++i) {
            fill_result(&outs[i], rs[i], problems[i]->n);
            if (infos) {
                infos[i].ncols = (int)bis[i].ub.size(); infos[i].n = problems[i]->n;
                infos[i].flip = dup_vec(bis[i].flip); infos[i].ub = dup_vec(bis[i].ub); infos[i].lower = dup_vec(bis[i].lower);
            }
        }
        return 0;
    });
}

// ---- packed batches: arrays in, one launch, arrays out (host/bounded.cpp CheckPacked, lpx_packed.hip) -------------------------
int lpx_packed_fits(int m, int n)
{
    if (m < 1 || n < 1 || m > (1 << 20) || n > (1 << 20)) return 0;
    return lpx_bounded_node_fits(m + 1, n + m + 1);
}

int lpx_solve_packed(const lpx_packed_models* in, const lpx_run_opts* o, const lpx_packed_results* out, lpx_stats* st)
{
    try { CheckPacked(in, o, out); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 0); o = &d; }
    return packed_solve(in, o, out, st);
}

int lpx_solve_packed_dual(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* out,
                          lpx_stats* st)
{
    try { CheckPackedDual(in, flags, o, out); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    return packed_dual_solve(in, flags, o, out, st);
}

// ---- right-hand-side scenarios warm-started from one solved base (host/bounded.cpp CheckPackedBase*, lpx_packed_warm.hip) -------
struct lpx_packed_base { PackedBase s; std::vector<double> c0; };     // c0: the base's costs, for lpx_packed_base_solve_costs

int lpx_packed_base_open(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* base_out,
                         lpx_packed_base** h)
{
    if (h) *h = nullptr;
    try { CheckPackedBaseOpen(in, flags, o, base_out, h); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    lpx_packed_base* base = new lpx_packed_base();
    const int rc = packed_base_open(in, flags, o, base_out, &base->s);
    if (rc != 0) { packed_base_close(&base->s); delete base; return rc; }     // only an optimal base is kept
    base->c0.assign(in->c, in->c + in->n);
    *h = base;
    return 0;
}

int lpx_packed_base_solve(const lpx_packed_base* h, int32_t count, const double* b, int flags, const lpx_run_opts* o,
                          const lpx_packed_dual_results* out, lpx_stats* st)
{
    try { CheckPackedBaseSolve(h, h ? h->s.m : 0, h ? h->s.n : 0, count, b, flags, o, out); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    lpx_run_opts d; if (!o) { lpx_default_opts(&d, 1); o = &d; }
    return packed_base_solve(&h->s, count, b, flags, o, out, st);
}

int lpx_packed_base_solve_costs(const lpx_packed_base* h, int32_t count, const double* c, const double* b, int flags,
                                const lpx_run_opts* o_primal, const lpx_run_opts* o_dual, const lpx_packed_cost_results* out,
                                lpx_stats* st)
{
    try { CheckPackedBaseSolveCosts(h, h ? h->s.m : 0, h ? h->s.n : 0, count, c, b, flags, o_primal, o_dual, out); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    lpx_run_opts dp, dd;
    if (!o_primal) { lpx_default_opts(&dp, 0); o_primal = &dp; }
    if (!o_dual) { lpx_default_opts(&dd, 1); o_dual = &dd; }
    return packed_base_solve_costs(&h->s, h->c0.data(), count, c, b, flags, o_primal, o_dual, out, st);
}

int lpx_packed_base_close(lpx_packed_base* h)
{
    if (!h) return 0;
    packed_base_close(&h->s);
    delete h;
    return 0;
}

int lpx_solve_packed_bnb(const lpx_packed_bnb_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                         lpx_stats* st)
{
    try { CheckPackedBnb(in, opt, out, packed_bnb_work_bytes); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    return packed_bnb_solve(in, opt, out, st);
}

int lpx_solve_packed_bnb_dual(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                              lpx_stats* st)
{
    try { CheckPackedBnbDual(in, opt, out, packed_bnb_work_bytes); }
    catch (const LpxException& ex) { set_error(ex.what()); return ex.code; }
    return packed_bnb_dual_solve(in, opt, out, st);
}

void lpx_bounded_info_free(lpx_bounded_info* info)
{
    if (!info) return;
    std::free(info->flip); std::free(info->ub); std::free(info->lower);
    std::memset(info, 0, sizeof(*info));
}

// ---- bounded session: lpx_solve_bounded that keeps its handle, then bound edits re-optimised by the bounded dual loop ------
struct lpx_bounded_session { BoundedSession s; };

int lpx_bounded_open(const lpx_problem* p, const double* lower, const double* upper, const lpx_solve_opts* o,
                     lpx_bounded_session** session, lpx_result* out)
{
    if (session) *session = nullptr;
    if (!p || !session || !out) { set_error("lpx_bounded_open: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    lpx_bounded_session* ses = new lpx_bounded_session();
    const int rc = guarded("lpx_bounded_open", [&]() -> int {
        EngineOptions e = to_engine(o);
        UpdatePivot cb = to_callback(o);
        LPProblem q = to_problem(p);
        std::vector<double> lo, up;
        if (lower) lo.assign(lower, lower + p->n);
        if (upper) up.assign(upper, upper + p->n);
        SimplexResult r = SolveBounded(q, lo, up, e, cb, nullptr, &ses->s);
        fill_result(out, r, p->n);
        return 0;
    });
    if (rc != 0) { delete ses; return rc; }
    *session = ses;
    return 0;
}

int lpx_bounded_set_bounds(lpx_bounded_session* s, int K, const int32_t* vars, const double* lower, const double* upper, lpx_result* out)
{
    if (!s || !out) { set_error("lpx_bounded_set_bounds: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    return guarded("lpx_bounded_set_bounds", [&]() -> int {
        SimplexResult r = BoundedSetBounds(s->s, K, vars, lower, upper);
        fill_result(out, r, s->s.n);
        return 0;
    });
}

void lpx_bounded_close(lpx_bounded_session* s) { delete s; }

// ---- branch and bound by bound changes on the root's handle (host/bnb_bounded.cpp) ------------------------------------------
static int solve_bnb_bounded(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int, const lpx_solve_opts* o,
                            int64_t max_nodes, int search_flags, lpx_result* out, lpx_bnb_bounded_info* info, const char* what,
                            int node_form = -1, int divers = 0, lpx_bnb_divers_info* dinfo = nullptr,     // divers > 0: lpx_solve_bnb_bounded4
                            int plunge = 0, lpx_bnb_plunge_info* pinfo = nullptr,                         // plunge > 0: lpx_solve_bnb_bounded5
                            const BnbStrong* strong = nullptr, lpx_bnb_strong_info* sinfo = nullptr,      // strong: lpx_solve_bnb_bounded6, LPX_BRANCH_STRONG
                            int stall_events = -1, lpx_bnb_guard_info* ginfo = nullptr,                   // stall_events >= 0: lpx_solve_bnb_bounded7
                            int root_form = -1,                                                           // lpx_solve_bnb_bounded8: the root's form
                            const lpx_cut_opts* root_cuts = nullptr, lpx_bnb_cut_info* cinfo = nullptr,   // lpx_solve_bnb_bounded9: cuts at the root
                            int tighten = 0, lpx_bnb_fix_info* finfo = nullptr,                           // lpx_solve_bnb_bounded10: reduced-cost tightening
                            bool dual_root = false)                                                       // lpx_solve_bnb_bounded_dual: the root by the dual start
{
    if (!p || !out) { set_error(std::string(what) + ": null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    if (info) std::memset(info, 0, sizeof(*info));
    if (dinfo) std::memset(dinfo, 0, sizeof(*dinfo));
    if (pinfo) std::memset(pinfo, 0, sizeof(*pinfo));
    if (sinfo) std::memset(sinfo, 0, sizeof(*sinfo));
    if (ginfo) std::memset(ginfo, 0, sizeof(*ginfo));
    if (cinfo) std::memset(cinfo, 0, sizeof(*cinfo));
    if (finfo) std::memset(finfo, 0, sizeof(*finfo));
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    return guarded(what, [&]() -> int {
        EngineOptions e = to_engine(o);
        LPProblem q = to_problem(p);
        std::vector<double> lo, up;
        std::vector<uint8_t> mask;
        BnbCutInfo ci;
        if (lower) lo.assign(lower, lower + p->n);
        if (upper) up.assign(upper, upper + p->n);
        if (is_int) mask.assign(is_int, is_int + p->n);
        BnbBoundedInfo bi;
        BnbDiversInfo di;
        BnbPlungeInfo pi;
        BnbStrongInfo si;
        BnbGuardInfo gi;
        BnbFixInfo fi;
        SimplexResult r = dual_root ? SolveBnbBoundedDual(q, lo, up, mask, e, max_nodes, bi, search_flags, node_form)
                        : stall_events >= 0 ? SolveBnbDivers(q, lo, up, mask, e, max_nodes, bi, search_flags, divers, di, nullptr, nullptr, stall_events, &gi, root_form,
                                                             root_cuts, &ci, tighten, &fi)
                        : strong ? SolveBnbDivers(q, lo, up, mask, e, max_nodes, bi, search_flags, divers, di, strong, &si)
                        : plunge ? SolveBnbPlunge(q, lo, up, mask, e, max_nodes, bi, search_flags, divers, plunge, di, pi)
                        : divers ? SolveBnbDivers(q, lo, up, mask, e, max_nodes, bi, search_flags, divers, di)
                                 : SolveBnbBounded(q, lo, up, mask, e, max_nodes, bi, search_flags, node_form);
        fill_result(out, r, p->n);
        if (cinfo) {
            cinfo->ran = ci.ran; cinfo->spare = ci.spare; cinfo->rounds = ci.rounds; cinfo->added = ci.added; cinfo->purged = ci.purged;
            cinfo->stop = ci.stop; cinfo->status = ci.status; cinfo->R = ci.R; cinfo->C = ci.C; cinfo->events = ci.events;
            cinfo->n_z = (int32_t)ci.z_before.size();
            cinfo->z_before = dup_vec(ci.z_before); cinfo->z_after = dup_vec(ci.z_after);
        }
        if (finfo) { finfo->tightened_nodes = fi.tightened_nodes; finfo->tightened_cols = fi.tightened_cols; finfo->max_per_node = fi.max_per_node; }
        if (ginfo) { ginfo->guarded_nodes = gi.guarded_nodes; ginfo->bland_events = gi.bland_events; ginfo->max_events = gi.max_events; }
        if (sinfo) {
            sinfo->probe_launches = si.probe_launches; sinfo->probes = si.probes; sinfo->probe_events = si.probe_events;
            sinfo->probe_limit = si.probe_limit; sinfo->pruned_by_probe = si.pruned_by_probe; sinfo->changed_picks = si.changed_picks;
        }
        if (pinfo) {
            pinfo->launched = pi.launched; pinfo->dropped = pi.dropped; pinfo->longest_chain = pi.longest_chain;
            pinfo->step = dup_vec(pi.step);
        }
        if (dinfo) {
            dinfo->rounds = di.rounds; dinfo->steals = di.steals; dinfo->largest_batch = di.largest_batch;
            dinfo->round = dup_vec(di.round); dinfo->diver = dup_vec(di.diver);
        }
        if (info) {
            info->nodes = bi.nodes; info->events = bi.events; info->flips = bi.flips; info->incumbents = bi.incumbents;
            info->pruned_bound = bi.pruned_bound; info->pruned_infeasible = bi.pruned_infeasible; info->max_K = bi.max_K;
            info->constant = bi.constant;
            info->n_log = (int64_t)bi.log.size(); info->log = dup_vec(bi.log);
        }
        if (bi.limit_rc) { set_error(bi.limit_msg); return bi.limit_rc; }
        return 0;
    });
}

int lpx_solve_bnb_bounded(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                          const lpx_solve_opts* o, int64_t max_nodes, lpx_result* out, lpx_bnb_bounded_info* info)
{
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, 0, out, info, "lpx_solve_bnb_bounded");
}

int lpx_solve_bnb_bounded2(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, lpx_result* out, lpx_bnb_bounded_info* info)
{
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded2");
}

int lpx_solve_bnb_bounded3(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int node_form, lpx_result* out,
                           lpx_bnb_bounded_info* info)
{
    if (node_form != LPX_NODE_LAUNCHES && node_form != LPX_NODE_ONCHIP && node_form != LPX_NODE_AUTO) {
        set_error("lpx_solve_bnb_bounded3: unknown node_form");
        return LPX_EINVAL;
    }
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded3", node_form);
}

// node_form is checked by the driver, behind the bounds and the integer variables
int lpx_solve_bnb_bounded_dual(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                               const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int node_form, lpx_result* out,
                               lpx_bnb_bounded_info* info)
{
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded_dual", node_form, 0, nullptr,
                             0, nullptr, nullptr, nullptr, -1, nullptr, -1, nullptr, nullptr, 0, nullptr, true);
}

int lpx_solve_bnb_bounded4(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, lpx_result* out,
                           lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded4: divers is outside [1, 1024]"); return LPX_EINVAL; }
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded4", -1, divers, dinfo);
}

int lpx_solve_bnb_bounded5(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int plunge, lpx_result* out,
                           lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo, lpx_bnb_plunge_info* pinfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded5: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (plunge < 1 || plunge > 64) { set_error("lpx_solve_bnb_bounded5: plunge is outside [1, 64]"); return LPX_EINVAL; }
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded5", -1, divers, dinfo,
                             plunge, pinfo);
}

int lpx_solve_bnb_bounded6(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int branching, int cand_max,
                           int probe_iter, lpx_result* out, lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo,
                           lpx_bnb_strong_info* sinfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded6: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (branching != LPX_BRANCH_MOST_FRACTIONAL && branching != LPX_BRANCH_STRONG) {
        set_error("lpx_solve_bnb_bounded6: branching is neither LPX_BRANCH_MOST_FRACTIONAL nor LPX_BRANCH_STRONG");
        return LPX_EINVAL;
    }
    if (cand_max < 1 || cand_max > 32) { set_error("lpx_solve_bnb_bounded6: cand_max is outside [1, 32]"); return LPX_EINVAL; }
    if (probe_iter < 0) { set_error("lpx_solve_bnb_bounded6: probe_iter is negative"); return LPX_EINVAL; }
    BnbStrong st; st.cand_max = cand_max; st.probe_iter = probe_iter;
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded6", -1, divers, dinfo,
                             0, nullptr, branching == LPX_BRANCH_STRONG ? &st : nullptr, sinfo);
}

int lpx_solve_bnb_bounded7(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int stall_events, lpx_result* out,
                           lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo, lpx_bnb_guard_info* ginfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded7: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error("lpx_solve_bnb_bounded7: stall_events is negative"); return LPX_EINVAL; }
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded7", -1, divers, dinfo,
                             0, nullptr, nullptr, nullptr, stall_events, ginfo);
}

int lpx_solve_bnb_bounded8(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int stall_events, int root_form,
                           lpx_result* out, lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo, lpx_bnb_guard_info* ginfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded8: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error("lpx_solve_bnb_bounded8: stall_events is negative"); return LPX_EINVAL; }
    if (root_form != LPX_NODE_LAUNCHES && root_form != LPX_NODE_ONCHIP && root_form != LPX_NODE_AUTO) {
        set_error("lpx_solve_bnb_bounded8: unknown root_form");
        return LPX_EINVAL;
    }
    // LPX_NODE_LAUNCHES: the call of lpx_solve_bnb_bounded7 itself (the root through lpx_bounded_run)
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded8", -1, divers, dinfo,
                             0, nullptr, nullptr, nullptr, stall_events, ginfo, root_form == LPX_NODE_LAUNCHES ? -1 : root_form);
}

int lpx_solve_bnb_bounded9(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                           const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int stall_events, int root_form,
                           const lpx_cut_opts* root_cuts, lpx_result* out, lpx_bnb_bounded_info* info, lpx_bnb_divers_info* dinfo,
                           lpx_bnb_guard_info* ginfo, lpx_bnb_cut_info* cinfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded9: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error("lpx_solve_bnb_bounded9: stall_events is negative"); return LPX_EINVAL; }
    if (root_form != LPX_NODE_LAUNCHES && root_form != LPX_NODE_ONCHIP && root_form != LPX_NODE_AUTO) {
        set_error("lpx_solve_bnb_bounded9: unknown root_form");
        return LPX_EINVAL;
    }
    if (root_cuts) if (int rc = check_cut_opts(root_cuts, "lpx_solve_bnb_bounded9")) return rc;
    // root_cuts == NULL: the call of lpx_solve_bnb_bounded8 itself
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded9", -1, divers, dinfo,
                             0, nullptr, nullptr, nullptr, stall_events, ginfo, root_form == LPX_NODE_LAUNCHES ? -1 : root_form, root_cuts, cinfo);
}

int lpx_solve_bnb_bounded10(const lpx_problem* p, const double* lower, const double* upper, const uint8_t* is_int,
                            const lpx_solve_opts* o, int64_t max_nodes, int search_flags, int divers, int stall_events, int root_form,
                            const lpx_cut_opts* root_cuts, int tighten, lpx_result* out, lpx_bnb_bounded_info* info,
                            lpx_bnb_divers_info* dinfo, lpx_bnb_guard_info* ginfo, lpx_bnb_cut_info* cinfo, lpx_bnb_fix_info* finfo)
{
    if (divers < 1 || divers > 1024) { set_error("lpx_solve_bnb_bounded10: divers is outside [1, 1024]"); return LPX_EINVAL; }
    if (stall_events < 0) { set_error("lpx_solve_bnb_bounded10: stall_events is negative"); return LPX_EINVAL; }
    if (root_form != LPX_NODE_LAUNCHES && root_form != LPX_NODE_ONCHIP && root_form != LPX_NODE_AUTO) {
        set_error("lpx_solve_bnb_bounded10: unknown root_form");
        return LPX_EINVAL;
    }
    if (root_cuts) if (int rc = check_cut_opts(root_cuts, "lpx_solve_bnb_bounded10")) return rc;
    if (tighten != 0 && tighten != 1) { set_error("lpx_solve_bnb_bounded10: tighten is neither 0 nor 1"); return LPX_EINVAL; }
    // tighten == 0: the call of lpx_solve_bnb_bounded9 itself
    return solve_bnb_bounded(p, lower, upper, is_int, o, max_nodes, search_flags, out, info, "lpx_solve_bnb_bounded10", -1, divers, dinfo,
                             0, nullptr, nullptr, nullptr, stall_events, ginfo, root_form == LPX_NODE_LAUNCHES ? -1 : root_form, root_cuts, cinfo,
                             tighten, finfo);
}

void lpx_bnb_cut_info_free(lpx_bnb_cut_info* cinfo)
{
    if (!cinfo) return;
    std::free(cinfo->z_before); std::free(cinfo->z_after);
    std::memset(cinfo, 0, sizeof(*cinfo));
}

void lpx_bnb_strong_info_free(lpx_bnb_strong_info* sinfo)
{
    if (sinfo) std::memset(sinfo, 0, sizeof(*sinfo));
}

void lpx_bnb_plunge_info_free(lpx_bnb_plunge_info* pinfo)
{
    if (!pinfo) return;
    std::free(pinfo->step);
    std::memset(pinfo, 0, sizeof(*pinfo));
}

void lpx_bnb_divers_info_free(lpx_bnb_divers_info* dinfo)
{
    if (!dinfo) return;
    std::free(dinfo->round); std::free(dinfo->diver);
    std::memset(dinfo, 0, sizeof(*dinfo));
}

void lpx_bnb_bounded_info_free(lpx_bnb_bounded_info* info)
{
    if (!info) return;
    std::free(info->log);
    std::memset(info, 0, sizeof(*info));
}

int lpx_sensitivity_range_report(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                 const char* target, char* buf, int len)
{
    if (!p || !target) { set_error("lpx_sensitivity_range_report: null argument"); return LPX_EINVAL; }
    return guarded("lpx_sensitivity_range_report", [&]() -> int {
        SensCtx c(p, T, R, C, basis);
        SensitivityAnalysis sa(&c.q, &c.r);
        return copy_out(sa.GetRangeReport(target), buf, len);
    });
}

int lpx_sensitivity_range(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                          const char* target, double* mn, double* mx)
{
    if (!p || !target || !mn || !mx) { set_error("lpx_sensitivity_range: null argument"); return LPX_EINVAL; }
    return guarded("lpx_sensitivity_range", [&]() -> int {
        SensCtx c(p, T, R, C, basis);
        SensitivityAnalysis sa(&c.q, &c.r);
        std::pair<double, double> r = sa.Range(target);
        *mn = r.first; *mx = r.second;
        return 0;
    });
}

int lpx_sensitivity_apply_change(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                 const char* target, double value, int* field, int* index, char* buf, int len)
{
    if (!p || !target) { set_error("lpx_sensitivity_apply_change: null argument"); return LPX_EINVAL; }
    return guarded("lpx_sensitivity_apply_change", [&]() -> int {
        SensCtx c(p, T, R, C, basis);
        SensitivityAnalysis sa(&c.q, &c.r);
        int f = -1, ix = -1;
        sa.Locate(target, &f, &ix);
        std::string msg = sa.ApplyChange(target, value);
        if (field) *field = f;
        if (index) *index = ix;
        return copy_out(msg, buf, len);
    });
}

int lpx_sensitivity_shadow_prices(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                  char* buf, int len)
{
    if (!p) { set_error("lpx_sensitivity_shadow_prices: null argument"); return LPX_EINVAL; }
    return guarded("lpx_sensitivity_shadow_prices", [&]() -> int {
        SensCtx c(p, T, R, C, basis);
        SensitivityAnalysis sa(&c.q, &c.r);
        return copy_out(sa.GetShadowPricesReport(), buf, len);
    });
}

int lpx_sensitivity_solve_duality(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                  const lpx_solve_opts* o, lpx_result* out)
{
    if (!p || !out) { set_error("lpx_sensitivity_solve_duality: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    return guarded("lpx_sensitivity_solve_duality", [&]() -> int {
        SensCtx c(p, T, R, C, basis);
        SensitivityAnalysis sa(&c.q, &c.r, to_engine(o));
        SimplexResult r = sa.SolveUsingDuality();
        fill_result(out, r, -1);
        return 0;
    });
}

int lpx_solve_ranging(const lpx_problem* p, const char* algorithm, const lpx_solve_opts* o, lpx_result* out, lpx_ranging* rg)
{
    if (!p || !algorithm || !out || !rg) { set_error("lpx_solve_ranging: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    std::memset(rg, 0, sizeof(*rg));
    bool dual = false;
    {
        std::string key;
        try { key = LPSolver::NormalizeAlgorithmKey(algorithm); } catch (const std::exception&) {}
        if (key == "dual simplex" || key == "dual") dual = true;
        else if (!(key == "primal simplex" || key == "primal")) {
            set_error(std::string("lpx_solve_ranging: algorithm '") + algorithm + "' has no tableau to range; supported: Primal Simplex, Dual Simplex");
            return LPX_EINVAL;
        }
    }
    if (int rc = ensure_device()) return rc;
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    const int n = p->n;
    RangingAlloc(rg, n, p->m);
    const int rc = guarded("lpx_solve_ranging", [&]() -> int {
        EngineOptions e = to_engine(o);
        UpdatePivot cb = to_callback(o);
        LPProblem q = to_problem(p);
        std::vector<int> row_of, sign;
        PreparedRows(q, dual, (o->dual_flags & LPX_DUAL_FIX_D1) != 0, row_of, sign);
        const int mx = (int)row_of.size();
        RangingMap map;
        map.q = &q; map.row_of = row_of; map.sign = sign;
        for (int j = 0; j < n; ++j) map.var_col.push_back(j);
        for (int k = 0; k < mx; ++k) map.slack_col.push_back(n + k);
        RawRanging raw;
        int status = -1;
        e.on_final_tableau = [&](lpx_tableau* t, int st) {
            status = st;
            if (st != LPX_OPTIMAL) return;
            RangeTableau(t, map, raw);
        };
        SimplexResult r = LPSolver(e).Solve(q, algorithm, cb);
        fill_result(out, r, p->n);
        RangingToUser(map, raw, status, rg);
        return 0;
    });
    if (rc != 0) lpx_ranging_free(rg);
    return rc;
}

int lpx_solve_cuts(const lpx_problem* p, const lpx_solve_opts* o, const lpx_cut_opts* co, lpx_result* out)
{
    if (!p || !out) { set_error("lpx_solve_cuts: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    lpx_cut_opts dc; if (!co) { lpx_default_cut_opts(&dc); co = &dc; }
    if (int rc = check_cut_opts(co, "lpx_solve_cuts")) return rc;
    if (int rc = ensure_device()) return rc;
    lpx_solve_opts d; if (!o) { lpx_default_solve_opts(&d); o = &d; }
    return guarded("lpx_solve_cuts", [&]() -> int {
        SimplexResult r = GmiCuttingPlane(to_engine(o), *co).Solve(to_problem(p), to_callback(o));
        fill_result(out, r, p->n);
        return 0;
    });
}

void lpx_ranging_free(lpx_ranging* rg)
{
    if (!rg) return;
    std::free(rg->cost_lo); std::free(rg->cost_hi); std::free(rg->cost_lo_at); std::free(rg->cost_hi_at); std::free(rg->reduced_cost);
    std::free(rg->rhs_lo); std::free(rg->rhs_hi); std::free(rg->rhs_lo_at); std::free(rg->rhs_hi_at); std::free(rg->dual);
    std::memset(rg, 0, sizeof(*rg));
}

void lpx_result_free(lpx_result* r)
{
    if (!r) return;
    std::free(r->x); std::free(r->T); std::free(r->basis); std::free(r->trace); std::free(r->report);
    std::free(r->summary); std::free(r->node_log); std::free(r->node_z); std::free(r->cuts);
    std::memset(r, 0, sizeof(*r));
}

int lpx_parse_text(const char* text, lpx_parsed* out)
{
    if (!text || !out) { set_error("lpx_parse_text: null argument"); return LPX_EINVAL; }
    std::memset(out, 0, sizeof(*out));
    try {
        LPProblem q = ParseFromText(text);
        const int n = q.NumVars(), m = (int)q.Constraints.size();
        out->sense = q.ObjectiveSense == Sense::Min ? LPX_MIN : LPX_MAX;
        out->n = n; out->m = m;
        out->c = dup_vec(q.C);
        out->A = (double*)std::calloc((size_t)(m ? m : 1) * (n ? n : 1), sizeof(double));
        out->rel = (int32_t*)std::malloc(sizeof(int32_t) * (m ? m : 1));
        out->b = (double*)std::malloc(sizeof(double) * (m ? m : 1));
        for (int i = 0; i < m; ++i) {
            const Constraint& c = q.Constraints[i];
            for (int j = 0; j < n && j < (int)c.A.size(); ++j) out->A[(size_t)i * n + j] = c.A[j];
            if ((int)c.A.size() < n) out->ragged = 1;     // IndexOutOfRange later in BuildTableau (PrimalSimplex.cs:190)
            out->rel[i] = c.Relation == Rel::GE ? LPX_GE : (c.Relation == Rel::EQ ? LPX_EQ : LPX_LE);
            out->b[i] = c.B;
        }
        return 0;
    } catch (const LpxException& ex) {
        set_error(ex.what());
        return ex.code;
    }
}

void lpx_parsed_free(lpx_parsed* p)
{
    if (!p) return;
    std::free(p->c); std::free(p->A); std::free(p->rel); std::free(p->b);
    std::memset(p, 0, sizeof(*p));
}

int lpx_format_number(double v, char* buf, int len)
{
    std::string s = FormatNumber(v);
    if (buf && len > 0) { std::strncpy(buf, s.c_str(), len - 1); buf[len - 1] = 0; }
    return (int)s.size();
}

}  // extern "C"
