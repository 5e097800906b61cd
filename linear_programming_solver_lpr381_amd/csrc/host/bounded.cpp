// host/bounded.cpp -- the bounded-variable primal simplex at the model level (lpx_solve_bounded, include/lpx.h): preparation as
// PrimalSimplex.Solve (Models/PrimalSimplex.cs:57-90), lower bounds shifted away on the host, upper bounds handed to the device
// loop (lpx_bounded_run) beside the tableau instead of as rows.  A bounded session (lpx_bounded_open) is the same solve that
// keeps its handle; its bound edits are lpx_tableau_change_bounds + lpx_bounded_dual_run on that handle.  The dual start
// (lpx_solve_bounded_dual) shares the preparation and solves from the slack basis with lpx_bounded_dual_run3.  With a form
// (lpx_solve_bounded2) the loop is lpx_bounded_run2; lpx_solve_bounded_batch solves many models in one lpx_node_batch_primal.
#include "model.h"

#include <chrono>
#include <cmath>
#include <cstring>

namespace lpx { namespace host {

void CheckVarBounds(const std::string& var, double lower, double upper)
{
    if (!std::isfinite(lower)) throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: lower bound of " + var + " is not finite");
    if (!(upper >= lower)) throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: upper bound of " + var + " is below its lower bound or NaN");
}

namespace {

struct BoundedHandle {
    lpx_tableau* h = nullptr; int R, C, spare;  // R x C: the capacity the handle was made with
    // spare > 0: capacity (R_ + spare, C_ + spare) around a live R_ x C_ window
    BoundedHandle(int R_, int C_, int spare_ = 0) : R(R_ + spare_), C(C_ + spare_), spare(spare_)
    {
        h = acquire_exact_handle(R, C);
        if (spare > 0) { const int rc = lpx_tableau_set_shape(h, R_, C_); if (rc) { release_exact_handle(h, R, C); h = nullptr; throw_lib(rc); } }
    }
    // the handle goes back to a cache shared with the other solvers: without its bounds, its live shape the capacity
    ~BoundedHandle()
    {
        if (!h) return;
        lpx_tableau_set_bounds(h, 0, nullptr);
        if (spare > 0) lpx_tableau_set_shape(h, R, C);
        release_exact_handle(h, R, C);
    }
    lpx_tableau* take() { lpx_tableau* k = h; h = nullptr; return k; }          // a session keeps it
    BoundedHandle(const BoundedHandle&) = delete;
};

struct EventCtx { UpdatePivot cb; const std::vector<std::string>* names; };

void bounded_event(void* user, int iter, int row, int col)
{
    EventCtx* c = static_cast<EventCtx*>(user);
    if (!c->cb) return;
    const std::string head = "BOUNDED TABLEAU Iteration " + std::to_string(iter) + ": ";
    const std::string& v = (*c->names)[col];
    if (row == -1) c->cb(head + "bound flip of " + v + "\n", nullptr);
    else if (row < -1) c->cb(head + "leaving row " + std::to_string(-2 - row) + " at its upper bound, entering " + v + "\n", nullptr);
    else c->cb(head + "leaving row " + std::to_string(row) + ", entering " + v + "\n", nullptr);
}

// What a finished loop left on the handle, in the user's terms: events, tableau, x (lower bounds of open added back), the
// optimum in the user's sense plus the constant the shift took out, the report with its at-upper line.
void collect(lpx_tableau* h, int st, int n, int R, int C, const std::vector<double>& lower, bool min, bool shifted, double constant,
             std::string report, SimplexResult& res, std::vector<uint8_t>* flip_out)
{
    const int Cm = C - 1;
    int nev = 0;
    int rc = lpx_tableau_trace(h, nullptr, 0, &nev); if (rc) throw_lib(rc);
    res.Trace.resize(2 * (size_t)(nev > 0 ? nev : 1));
    rc = lpx_tableau_trace(h, res.Trace.data(), nev, &nev); if (rc) throw_lib(rc);
    res.Trace.resize(2 * (size_t)nev);
    std::vector<double> T((size_t)R * C); std::vector<int32_t> basis((size_t)(R - 1));
    rc = lpx_tableau_download(h, T.data(), basis.data());
    if (rc) throw_lib(rc);
    std::vector<double> x((size_t)n, 0.0); double z = 0.0;
    std::vector<uint8_t> at_upper((size_t)n, 0), flip((size_t)Cm, 0);
    rc = lpx_tableau_bounded_solution(h, n, x.data(), &z, at_upper.data()); if (rc) throw_lib(rc);
    rc = lpx_tableau_bound_flags(h, flip.data()); if (rc) throw_lib(rc);
    if (!lower.empty()) for (int j = 0; j < n; ++j) x[j] = x[j] + lower[j];
    // the tableau maximises; the user's optimum is -z for a Min model, plus the constant the shift took out
    double value = z;
    if (shifted || min) {
        value = min ? -z : z;
        if (shifted) value = value + constant;
    }
    if (st == LPX_UNBOUNDED) report += "UNBOUNDED\n";                                   // :104
    FinalizeText(report, res.Summary, x, value, st);
    std::string at = "  at upper bound:";
    bool any = false;
    for (int j = 0; j < n; ++j) if (at_upper[j]) { at += std::string(any ? "," : "") + " x" + std::to_string(j + 1); any = true; }
    if (!any) at += " none";
    report += at + "\n";
    res.Summary += at.substr(2) + "\n";
    res.Report = report; res.OptimalValue = value; res.Solution = x; res.HasSolution = true; res.Status = st;
    res.Tableau = std::move(T); res.R = R; res.C = C; res.Basis = std::move(basis);
    if (flip_out) *flip_out = flip;
}

}  // namespace

BoundedSession::~BoundedSession()
{
    if (!h) return;
    lpx_tableau_set_bounds(h, 0, nullptr);          // the handle goes back to the shared cache without its bounds
    if (spare > 0) lpx_tableau_set_shape(h, R + spare, C + spare);      // ... and with the shape it was made with
    release_exact_handle(h, R + spare, C + spare);
}

namespace {

// The model as the loops see it: internal tableau with its slack basis, shifted upper bounds, and what the lower shift took out.
struct Prepared {
    std::vector<double> T; int R = 0, C = 0; std::vector<int32_t> basis; std::vector<std::string> varNames;
    std::vector<double> ub; double constant = 0.0; bool shifted = false; std::string report;
};

// dual_start = false: the preparation of lpx_solve_bounded.  true: that of lpx_solve_bounded_dual -- a >= row is negated into a <=
// row instead of being refused, a negative shifted RHS is accepted, and an improving variable without an upper bound is refused.
Prepared prepare_bounded(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                         const EngineOptions& opt, UpdatePivot updatePivot, bool dual_start)
{
    Prepared P;
    const int n = original.NumVars();
    if ((!lower.empty() && (int)lower.size() != n) || (!upper.empty() && (int)upper.size() != n))
        throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: lower / upper need one entry per variable");
    for (int j = 0; j < n; ++j)
        CheckVarBounds("x" + std::to_string(j + 1), lower.empty() ? 0.0 : lower[j], upper.empty() ? 1.0 / 0.0 : upper[j]);
    LPProblem model = original.Clone();
    if (model.ObjectiveSense == Sense::Min) for (double& c : model.C) c = -c;          // :62-63
    for (const Constraint& cons : model.Constraints)
        if ((int)cons.A.size() < n) throw LpxException(LPX_EINVAL, "Index was outside the bounds of the array.");
    // x = l + x': b' = b - A l, one multiply and one subtract per nonzero l_j, j ascending
    if (!lower.empty())
        for (Constraint& cons : model.Constraints)
            for (int j = 0; j < n; ++j)
                if (lower[j] != 0.0) { const double prod = cons.A[j] * lower[j]; cons.B = cons.B - prod; }
    if (dual_start)
        for (Constraint& cons : model.Constraints)
            if (cons.Relation == Rel::GE) {                                             // exact: only signs change
                for (double& a : cons.A) a = -a;
                cons.B = -cons.B; cons.Relation = Rel::LE;
            }
    if (!dual_start) for (const Constraint& cons : model.Constraints) {                 // :66-77
        if (cons.Relation == Rel::GE)
            throw LpxException(LPX_E_GE_PRESENT, "Constraint contains '>=' sign. The Primal Simplex method cannot handle this. Please try the Dual Simplex algorithm instead.");
        if (cons.B < -1e-9)
            throw LpxException(LPX_E_NEG_RHS, "Constraint has a negative RHS value. The Primal Simplex method cannot handle this. Please try the Dual Simplex algorithm instead.");
    }
    double& constant = P.constant;  // c.l in the user's sense
    bool& shifted = P.shifted;
    if (!lower.empty())
        for (int j = 0; j < n; ++j)
            if (lower[j] != 0.0) { const double prod = original.C[j] * lower[j]; constant = constant + prod; shifted = true; }

    LPProblem tableauModel = ExpandEqualitiesToInequalities(model);                     // :80
    P.report = opt.quiet ? std::string() : AppendCanonicalForm(tableauModel);           // :82
    std::vector<double>& T = P.T; int& R = P.R; int& C = P.C; std::vector<int32_t>& basis = P.basis;
    std::vector<std::string>& varNames = P.varNames;
    BuildTableauPrimal(tableauModel, T, R, C, basis, varNames);                         // :85
    if (R < 2) throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: the model has no constraints");
    if (updatePivot) updatePivot(AppendTableau("TABLEAU Iteration", T.data(), R, C, basis, varNames, 0), nullptr);
    const int Cm = C - 1;
    P.ub.assign((size_t)Cm, 1.0 / 0.0);
    if (!upper.empty()) for (int j = 0; j < n; ++j) P.ub[j] = std::isinf(upper[j]) ? upper[j] : upper[j] - (lower.empty() ? 0.0 : lower[j]);
    if (dual_start)
        for (int j = 0; j < n; ++j)
            if (T[(size_t)(R - 1) * C + j] < -1e-9 && std::isinf(P.ub[j]))
                throw LpxException(LPX_EINVAL, "Bounded Dual Simplex: x" + std::to_string(j + 1) + " improves the objective and has no upper "
                                               "bound: a bound flip cannot make it dual feasible");
    return P;
}

// The tail that SolveBounded and SolveBoundedDual share, from the status of the finished loop to the result: the iteration-limit
// throw, the counts, collect, the caller's own report lines (`tail`, given the counts; may be empty), on_final_tableau, names,
// Aux and info.
void finish_solve(lpx_tableau* h, int st, const LPProblem& original, const std::vector<double>& lower, const Prepared& P,
                  const EngineOptions& opt, const std::function<std::string(const int64_t*)>& tail, SimplexResult& res, BoundedInfo* info)
{
    const int n = original.NumVars();
    if (st < 0) throw_lib(st);
    if (st == LPX_ITER_LIMIT) throw LpxException(LPX_ITER_LIMIT, "Iteration limit exceeded.");      // :95-96
    int64_t counts[3] = {0, 0, 0};
    lpx_bounded_counts(h, counts);
    std::vector<uint8_t> flip;
    collect(h, st, n, P.R, P.C, lower, original.ObjectiveSense == Sense::Min, P.shifted, P.constant, P.report, res, &flip);
    if (tail) { const std::string lines = tail(counts); res.Report += lines; res.Summary += lines.substr(2); }
    if (opt.on_final_tableau) opt.on_final_tableau(h, st);
    res.VarNames = P.varNames;
    res.Aux = {(double)counts[0], (double)counts[1], (double)counts[2], P.constant};
    if (info) { info->flip = flip; info->ub = P.ub; info->lower = lower.empty() ? std::vector<double>((size_t)n, 0.0) : lower; }
}

}  // namespace

SimplexResult SolveBounded(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                           const EngineOptions& opt, UpdatePivot updatePivot, BoundedInfo* info, BoundedSession* keep, int form, int max_spare)
{
    const int n = original.NumVars();
    if (form != -1 && form != LPX_NODE_LAUNCHES && form != LPX_NODE_ONCHIP && form != LPX_NODE_AUTO)
        throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: unknown form (none of LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP and LPX_NODE_AUTO)");
    // the on-chip form reports no event: with a callback it is refused below, behind the validation and without a call of it
    Prepared P = prepare_bounded(original, lower, upper, opt, form == LPX_NODE_ONCHIP ? nullptr : updatePivot, false);
    const int R = P.R, C = P.C;
    const bool bounded = !upper.empty() || !lower.empty() || keep;       // a session edits bounds later: its handle always has them
    // the shape is known here, on the host: the refusals of the on-chip form come before any device check
    const bool fits = lpx_bounded_node_fits(R, C) != 0;
    if (form == LPX_NODE_ONCHIP && updatePivot)
        throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: the on-chip form has no per-event callback (text_cb)");
    if (form == LPX_NODE_ONCHIP && !fits)
        throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: the " + std::to_string(R) + " x " + std::to_string(C) +
                                       " tableau does not fit the on-chip form (lpx_bounded_node_fits)");
    const bool onchip = form == LPX_NODE_ONCHIP || (form == LPX_NODE_AUTO && fits && !updatePivot);

    int spare = keep ? max_spare : 0;
    while (spare > 0 && !lpx_bounded_node_fits(R + spare, C + spare)) --spare;

    SimplexResult res;
    BoundedHandle th(R, C, spare);
    int rc = lpx_tableau_upload(th.h, P.T.data(), P.basis.data());
    if (rc) throw_lib(rc);
    if (bounded) { rc = lpx_tableau_set_bounds(th.h, C - 1, P.ub.data()); if (rc) throw_lib(rc); }
    lpx_run_opts o; lpx_default_opts(&o, 0);
    o.max_iter = opt.max_iter;
    o.batch = opt.batch;
    EventCtx ctx{updatePivot, &P.varNames};
    const int st = onchip ? lpx_bounded_run2(th.h, &o, LPX_NODE_ONCHIP, nullptr, nullptr, &res.Stats)
                          : lpx_bounded_run(th.h, &o, updatePivot ? bounded_event : nullptr, &ctx, &res.Stats);
    finish_solve(th.h, st, original, lower, P, opt, nullptr, res, info);
    if (keep) {
        keep->h = th.take(); keep->R = R; keep->C = C; keep->n = n;
        keep->min = original.ObjectiveSense == Sense::Min; keep->shifted = P.shifted; keep->constant = P.constant;
        keep->lower = lower; keep->open_status = st; keep->opt = opt; keep->varNames = P.varNames;
        keep->spare = spare;
        if (max_spare > 0) keep->T0 = P.T;
    }
    return res;
}

// Many independent models in ONE launch (lpx_solve_bounded_batch): every model validated and prepared first, then a handle per
// model, one lpx_node_batch_primal over all of them, and per model the tail of SolveBounded.
void SolveBoundedBatch(const std::vector<const LPProblem*>& problems, const std::vector<std::vector<double>>& lowers,
                       const std::vector<std::vector<double>>& uppers, const EngineOptions& opt, std::vector<SimplexResult>& results,
                       std::vector<BoundedInfo>& infos)
{
    const int count = (int)problems.size();
    if (count < 1 || count > 1024) throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: count is outside [1, 1024]");
    auto named = [](int i, const LpxException& ex) { return LpxException(ex.code, "model " + std::to_string(i) + ": " + ex.what()); };
    std::vector<Prepared> P((size_t)count);
    for (int i = 0; i < count; ++i) {
        try {
            P[i] = prepare_bounded(*problems[i], lowers[i], uppers[i], opt, nullptr, false);
            if (!lpx_bounded_node_fits(P[i].R, P[i].C))
                throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: the " + std::to_string(P[i].R) + " x " + std::to_string(P[i].C) +
                                               " tableau does not fit the on-chip form (lpx_bounded_node_fits)");
        } catch (const LpxException& ex) { throw named(i, ex); }
    }
    std::vector<std::unique_ptr<BoundedHandle>> th;
    std::vector<lpx_tableau*> hs;
    for (int i = 0; i < count; ++i) {
        th.emplace_back(new BoundedHandle(P[i].R, P[i].C));
        lpx_tableau* h = th.back()->h;
        int rc = lpx_tableau_upload(h, P[i].T.data(), P[i].basis.data());
        if (rc) throw_lib(rc);
        // a batch's handles always carry their bounds; every ub = +inf is the run without bounds, bit for bit
        rc = lpx_tableau_set_bounds(h, P[i].C - 1, P[i].ub.data()); if (rc) throw_lib(rc);
        hs.push_back(h);
    }
    lpx_run_opts o; lpx_default_opts(&o, 0);
    o.max_iter = opt.max_iter;
    std::vector<int32_t> slot((size_t)count), rcs((size_t)count, 0);
    for (int i = 0; i < count; ++i) slot[i] = i;
    std::vector<lpx_primal_record> recs((size_t)count);
    struct Batch { lpx_node_batch* b = nullptr; ~Batch() { lpx_node_batch_destroy(b); } } nb;
    int rc = lpx_node_batch_create(count, hs.data(), &nb.b); if (rc) throw_lib(rc);
    const auto t0 = std::chrono::steady_clock::now();
    rc = lpx_node_batch_primal(nb.b, count, slot.data(), &o, recs.data(), rcs.data()); if (rc) throw_lib(rc);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();   // the one launch, shared
    results.assign((size_t)count, SimplexResult());
    infos.assign((size_t)count, BoundedInfo());
    for (int i = 0; i < count; ++i) {
        results[i].Stats.pivots = recs[i].kind0 + recs[i].kind1; results[i].Stats.launches = 1; results[i].Stats.loop_ms = ms;
        try { finish_solve(hs[i], rcs[i], *problems[i], lowers[i], P[i], opt, nullptr, results[i], &infos[i]); }
        catch (const LpxException& ex) { results.resize((size_t)i); infos.resize((size_t)i); throw named(i, ex); }
    }
}

// The argument checks of lpx_solve_packed, all of them host arithmetic independent of count: nothing here looks at a model.  What
// a model can get wrong (its bounds, a negative shifted RHS) is found by its workgroup and comes back as its status.
void CheckPacked(const lpx_packed_models* in, const lpx_run_opts* o, const lpx_packed_results* out)
{
    auto bad = [](const std::string& msg) { return LpxException(LPX_EINVAL, "lpx_solve_packed: " + msg); };
    if (!in || !out) throw bad("null argument");
    if (!in->c || !in->A || !in->b) throw bad("null c, A or b");
    if (!out->status || !out->x || !out->value) throw bad("null status, x or value");
    if (in->count < 1 || in->count > 65536) throw bad("count is outside [1, 65536]");
    if (in->m < 1 || in->n < 1) throw bad("m and n must be at least 1");
    if (in->sense != LPX_MAX && in->sense != LPX_MIN) throw bad("sense is neither LPX_MAX nor LPX_MIN");
    const int64_t m = in->m, n = in->n, count = in->count;
    const struct { const char* name; int64_t stride, packed; } strides[5] = {
        {"c_stride", in->c_stride, n}, {"A_stride", in->A_stride, m * n}, {"b_stride", in->b_stride, m},
        {"lower_stride", in->lower ? in->lower_stride : 0, n}, {"upper_stride", in->upper ? in->upper_stride : 0, n}};
    for (const auto& s : strides)
        if (s.stride != 0 && s.stride != s.packed)
            throw bad(std::string(s.name) + " is neither 0 nor the packed size " + std::to_string(s.packed));
    const int64_t R = m + 1, C = n + m + 1;
    if (!lpx_packed_fits(in->m, in->n))
        throw bad("the " + std::to_string(R) + " x " + std::to_string(C) + " tableau does not fit the on-chip form (lpx_packed_fits)");
    if (o && o->resident > 0) throw bad("there is no resident form of the bounded loop (resident = 1)");
    auto models = [&](int64_t stride) { return stride == 0 ? (int64_t)1 : count; };
    int64_t bytes = 8 * (n * models(in->c_stride) + m * n * models(in->A_stride) + m * models(in->b_stride));
    if (in->lower) bytes += 8 * n * models(in->lower_stride);
    if (in->upper) bytes += 8 * n * models(in->upper_stride);
    bytes += count * (4 + 8 * n + 8);
    if (out->rec) bytes += count * (int64_t)sizeof(lpx_primal_record);
    if (out->basis) bytes += count * 4 * m;
    if (out->at_upper) bytes += count * n;
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs and outputs, above 1 GiB (split the batch)");
}

// The argument checks of lpx_solve_packed_dual: CheckPacked's list in its order (rel_stride among the strides), then a shared rel
// (m reads; a per-model rel is checked by its workgroup), then the flags.
// `what` is the prefix of every message; out_optional: a NULL out is accepted and then counts no output bytes (the base of
// lpx_packed_base_open)
static void check_packed_dual(const std::string& what, const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o,
                              const lpx_packed_dual_results* out, bool out_optional)
{
    auto bad = [&](const std::string& msg) { return LpxException(LPX_EINVAL, what + msg); };
    if (!in || (!out && !out_optional)) throw bad("null argument");
    if (!in->c || !in->A || !in->b) throw bad("null c, A or b");
    if (out && (!out->status || !out->x || !out->value)) throw bad("null status, x or value");
    if (in->count < 1 || in->count > 65536) throw bad("count is outside [1, 65536]");
    if (in->m < 1 || in->n < 1) throw bad("m and n must be at least 1");
    if (in->sense != LPX_MAX && in->sense != LPX_MIN) throw bad("sense is neither LPX_MAX nor LPX_MIN");
    const int64_t m = in->m, n = in->n, count = in->count;
    const struct { const char* name; int64_t stride, packed; } strides[6] = {
        {"c_stride", in->c_stride, n}, {"A_stride", in->A_stride, m * n}, {"b_stride", in->b_stride, m},
        {"lower_stride", in->lower ? in->lower_stride : 0, n}, {"upper_stride", in->upper ? in->upper_stride : 0, n},
        {"rel_stride", in->rel ? in->rel_stride : 0, m}};
    for (const auto& s : strides)
        if (s.stride != 0 && s.stride != s.packed)
            throw bad(std::string(s.name) + " is neither 0 nor the packed size " + std::to_string(s.packed));
    const int64_t R = m + 1, C = n + m + 1;
    if (!lpx_packed_fits(in->m, in->n))
        throw bad("the " + std::to_string(R) + " x " + std::to_string(C) + " tableau does not fit the on-chip form (lpx_packed_fits)");
    if (o && o->resident > 0) throw bad("there is no resident form of the bounded loop (resident = 1)");
    auto models = [&](int64_t stride) { return stride == 0 ? (int64_t)1 : count; };
    int64_t bytes = 8 * (n * models(in->c_stride) + m * n * models(in->A_stride) + m * models(in->b_stride));
    if (in->lower) bytes += 8 * n * models(in->lower_stride);
    if (in->upper) bytes += 8 * n * models(in->upper_stride);
    if (in->rel) bytes += 4 * m * models(in->rel_stride);
    if (out) {
        bytes += count * (4 + 8 * n + 8);
        if (out->rec) bytes += count * (int64_t)sizeof(lpx_packed_dual_record);
        if (out->basis) bytes += count * 4 * m;
        if (out->at_upper) bytes += count * n;
        if (out->y) bytes += count * 8 * m;
        if (out->d) bytes += count * 8 * n;
    }
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs and outputs, above 1 GiB (split the batch)");
    if (in->rel && in->rel_stride == 0)
        for (int64_t i = 0; i < m; ++i)
            if (in->rel[i] != LPX_LE && in->rel[i] != LPX_GE)
                throw bad("rel[" + std::to_string(i) + "] is neither LPX_LE nor LPX_GE (an = row is passed as its pair of rows)");
    if (flags & ~LPX_BDUAL_LONG_STEP) throw bad("unknown flag: flags holds a bit other than LPX_BDUAL_LONG_STEP");
}

void CheckPackedDual(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* out)
{
    check_packed_dual("lpx_solve_packed_dual: ", in, flags, o, out, false);
}

// The argument checks of lpx_packed_base_open: a NULL in or h, then the list of lpx_solve_packed_dual in its order for the base as
// a batch of one whose arrays are all shared; base_out may be NULL.
void CheckPackedBaseOpen(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* base_out,
                         const void* h)
{
    const std::string what = "lpx_packed_base_open: ";
    if (!in || !h) throw LpxException(LPX_EINVAL, what + "null argument");
    lpx_packed_dual_models dm;
    std::memset(&dm, 0, sizeof dm);
    dm.count = 1; dm.m = in->m; dm.n = in->n; dm.sense = in->sense;
    dm.c = in->c; dm.A = in->A; dm.b = in->b; dm.lower = in->lower; dm.upper = in->upper; dm.rel = in->rel;
    check_packed_dual(what, &dm, flags, o, base_out, true);
}

// The argument checks of lpx_packed_base_solve; m and n are the handle's (read only behind the NULL test of the handle).
void CheckPackedBaseSolve(const void* h, int m32, int n32, int32_t count32, const double* b, int flags, const lpx_run_opts* o,
                          const lpx_packed_dual_results* out)
{
    auto bad = [](const std::string& msg) { return LpxException(LPX_EINVAL, "lpx_packed_base_solve: " + msg); };
    if (!h || !b || !out) throw bad("null argument");
    if (!out->status || !out->x || !out->value) throw bad("null status, x or value");
    if (count32 < 1 || count32 > 65536) throw bad("count is outside [1, 65536]");
    if (flags & ~LPX_BDUAL_LONG_STEP) throw bad("unknown flag: flags holds a bit other than LPX_BDUAL_LONG_STEP");
    if (o && o->resident > 0) throw bad("there is no resident form of the bounded loop (resident = 1)");
    const int64_t m = m32, n = n32, count = count32;
    int64_t bytes = 8 * m * count + count * (4 + 8 * n + 8);
    if (out->rec) bytes += count * (int64_t)sizeof(lpx_packed_dual_record);
    if (out->basis) bytes += count * 4 * m;
    if (out->at_upper) bytes += count * n;
    if (out->y) bytes += count * 8 * m;
    if (out->d) bytes += count * 8 * n;
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs and outputs, above 1 GiB (split the batch)");
}

// The argument checks of lpx_packed_base_solve_costs: those of lpx_packed_base_solve in their order with c in the place of b (b may
// be NULL: every scenario keeps b0), either options structure refused for resident = 1, the 1 GiB rule over c0, c, b and the outputs.
void CheckPackedBaseSolveCosts(const void* h, int m32, int n32, int32_t count32, const double* c, const double* b, int flags,
                               const lpx_run_opts* o_primal, const lpx_run_opts* o_dual, const lpx_packed_cost_results* out)
{
    auto bad = [](const std::string& msg) { return LpxException(LPX_EINVAL, "lpx_packed_base_solve_costs: " + msg); };
    if (!h || !c || !out) throw bad("null argument");
    if (!out->status || !out->x || !out->value) throw bad("null status, x or value");
    if (count32 < 1 || count32 > 65536) throw bad("count is outside [1, 65536]");
    if (flags & ~LPX_BDUAL_LONG_STEP) throw bad("unknown flag: flags holds a bit other than LPX_BDUAL_LONG_STEP");
    if ((o_primal && o_primal->resident > 0) || (o_dual && o_dual->resident > 0))
        throw bad("there is no resident form of the bounded loop (resident = 1)");
    const int64_t m = m32, n = n32, count = count32;
    int64_t bytes = 8 * n + 8 * n * count + count * (4 + 8 * n + 8);
    if (b) bytes += 8 * m * count;
    if (out->rec) bytes += count * (int64_t)sizeof(lpx_packed_cost_record);
    if (out->basis) bytes += count * 4 * m;
    if (out->at_upper) bytes += count * n;
    if (out->y) bytes += count * 8 * m;
    if (out->d) bytes += count * 8 * n;
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs and outputs, above 1 GiB (split the batch)");
}

// The argument checks of lpx_solve_packed_bnb: CheckPacked's list in its order up to the fit rule, then the options, and last --
// it needs valid options -- the 1 GiB rule, which counts the log and the work slices (work_bytes: lpx::packed_bnb_work_bytes).
void CheckPackedBnb(const lpx_packed_bnb_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                    size_t (*work_bytes)(int count, int m, int n, int max_depth))
{
    auto bad = [](const std::string& msg) { return LpxException(LPX_EINVAL, "lpx_solve_packed_bnb: " + msg); };
    if (!in || !out) throw bad("null argument");
    if (!in->c || !in->A || !in->b) throw bad("null c, A or b");
    if (!out->status || !out->x || !out->value) throw bad("null status, x or value");
    if (in->count < 1 || in->count > 65536) throw bad("count is outside [1, 65536]");
    if (in->m < 1 || in->n < 1) throw bad("m and n must be at least 1");
    if (in->sense != LPX_MAX && in->sense != LPX_MIN) throw bad("sense is neither LPX_MAX nor LPX_MIN");
    const int64_t m = in->m, n = in->n, count = in->count;
    const struct { const char* name; int64_t stride, packed; } strides[5] = {
        {"c_stride", in->c_stride, n}, {"A_stride", in->A_stride, m * n}, {"b_stride", in->b_stride, m},
        {"lower_stride", in->lower ? in->lower_stride : 0, n}, {"upper_stride", in->upper ? in->upper_stride : 0, n}};
    for (const auto& s : strides)
        if (s.stride != 0 && s.stride != s.packed)
            throw bad(std::string(s.name) + " is neither 0 nor the packed size " + std::to_string(s.packed));
    const int64_t R = m + 1, C = n + m + 1;
    if (!lpx_packed_fits(in->m, in->n))
        throw bad("the " + std::to_string(R) + " x " + std::to_string(C) + " tableau does not fit the on-chip form (lpx_packed_fits)");
    if (!opt) throw bad("null opts");
    if (opt->search_flags & ~(LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF))
        throw bad("unknown flag: search_flags holds a bit other than LPX_BDUAL_LONG_STEP and LPX_BDUAL_CUTOFF");
    if (opt->max_iter < 0) throw bad("max_iter is negative");
    if (opt->max_nodes < 1) throw bad("max_nodes is below 1 (the budgets of a packed search are mandatory)");
    if (opt->max_events < 1) throw bad("max_events is below 1 (the budgets of a packed search are mandatory)");
    if (opt->max_depth < 0) throw bad("max_depth is negative");
    if (opt->log_cap < 0) throw bad("log_cap is negative");
    if (out->log && opt->log_cap == 0) throw bad("log is given but log_cap is 0");
    if (!out->log && opt->log_cap > 0) throw bad("log_cap is positive but log is null");
    auto models = [&](int64_t stride) { return stride == 0 ? (int64_t)1 : count; };
    int64_t bytes = 8 * (n * models(in->c_stride) + m * n * models(in->A_stride) + m * models(in->b_stride));
    if (in->lower) bytes += 8 * n * models(in->lower_stride);
    if (in->upper) bytes += 8 * n * models(in->upper_stride);
    if (in->is_int) bytes += n;
    bytes += count * (4 + 8 * n + 8);
    if (out->rec) bytes += count * (int64_t)sizeof(lpx_packed_bnb_record);
    bytes += count * (int64_t)opt->log_cap * (int64_t)sizeof(lpx_bnb_node_log);
    bytes += (int64_t)work_bytes(in->count, in->m, in->n, opt->max_depth);
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs, outputs, log and work slices, above 1 GiB (split the batch)");
}

// The argument checks of lpx_solve_packed_bnb_dual: CheckPackedBnb's list in its order with rel_stride among the strides, behind the
// fit rule a shared rel (m reads; a per-model rel is checked by its workgroup), then the options and the 1 GiB rule, which counts rel.
void CheckPackedBnbDual(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                        size_t (*work_bytes)(int count, int m, int n, int max_depth))
{
    auto bad = [](const std::string& msg) { return LpxException(LPX_EINVAL, "lpx_solve_packed_bnb_dual: " + msg); };
    if (!in || !out) throw bad("null argument");
    if (!in->c || !in->A || !in->b) throw bad("null c, A or b");
    if (!out->status || !out->x || !out->value) throw bad("null status, x or value");
    if (in->count < 1 || in->count > 65536) throw bad("count is outside [1, 65536]");
    if (in->m < 1 || in->n < 1) throw bad("m and n must be at least 1");
    if (in->sense != LPX_MAX && in->sense != LPX_MIN) throw bad("sense is neither LPX_MAX nor LPX_MIN");
    const int64_t m = in->m, n = in->n, count = in->count;
    const struct { const char* name; int64_t stride, packed; } strides[6] = {
        {"c_stride", in->c_stride, n}, {"A_stride", in->A_stride, m * n}, {"b_stride", in->b_stride, m},
        {"lower_stride", in->lower ? in->lower_stride : 0, n}, {"upper_stride", in->upper ? in->upper_stride : 0, n},
        {"rel_stride", in->rel ? in->rel_stride : 0, m}};
    for (const auto& s : strides)
        if (s.stride != 0 && s.stride != s.packed)
            throw bad(std::string(s.name) + " is neither 0 nor the packed size " + std::to_string(s.packed));
    const int64_t R = m + 1, C = n + m + 1;
    if (!lpx_packed_fits(in->m, in->n))
        throw bad("the " + std::to_string(R) + " x " + std::to_string(C) + " tableau does not fit the on-chip form (lpx_packed_fits)");
    if (in->rel && in->rel_stride == 0)
        for (int64_t i = 0; i < m; ++i)
            if (in->rel[i] != LPX_LE && in->rel[i] != LPX_GE)
                throw bad("rel[" + std::to_string(i) + "] is neither LPX_LE nor LPX_GE (an = row is passed as its pair of rows)");
    if (!opt) throw bad("null opts");
    if (opt->search_flags & ~(LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF))
        throw bad("unknown flag: search_flags holds a bit other than LPX_BDUAL_LONG_STEP and LPX_BDUAL_CUTOFF");
    if (opt->max_iter < 0) throw bad("max_iter is negative");
    if (opt->max_nodes < 1) throw bad("max_nodes is below 1 (the budgets of a packed search are mandatory)");
    if (opt->max_events < 1) throw bad("max_events is below 1 (the budgets of a packed search are mandatory)");
    if (opt->max_depth < 0) throw bad("max_depth is negative");
    if (opt->log_cap < 0) throw bad("log_cap is negative");
    if (out->log && opt->log_cap == 0) throw bad("log is given but log_cap is 0");
    if (!out->log && opt->log_cap > 0) throw bad("log_cap is positive but log is null");
    auto models = [&](int64_t stride) { return stride == 0 ? (int64_t)1 : count; };
    int64_t bytes = 8 * (n * models(in->c_stride) + m * n * models(in->A_stride) + m * models(in->b_stride));
    if (in->lower) bytes += 8 * n * models(in->lower_stride);
    if (in->upper) bytes += 8 * n * models(in->upper_stride);
    if (in->rel) bytes += 4 * m * models(in->rel_stride);
    if (in->is_int) bytes += n;
    bytes += count * (4 + 8 * n + 8);
    if (out->rec) bytes += count * (int64_t)sizeof(lpx_packed_bnb_record);
    bytes += count * (int64_t)opt->log_cap * (int64_t)sizeof(lpx_bnb_node_log);
    bytes += (int64_t)work_bytes(in->count, in->m, in->n, opt->max_depth);
    if (bytes > ((int64_t)1 << 30))
        throw bad("too large: " + std::to_string(bytes) + " bytes of inputs, outputs, log and work slices, above 1 GiB (split the batch)");
}

SimplexResult SolveBoundedDual(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper, int flags,
                               const EngineOptions& opt, UpdatePivot updatePivot, BoundedInfo* info, BoundedSession* keep)
{
    if (flags & ~(LPX_BDUAL_SKIP_FIXED | LPX_BDUAL_LONG_STEP))
        throw LpxException(LPX_EINVAL, "Bounded Dual Simplex: flags holds a bit other than LPX_BDUAL_SKIP_FIXED and LPX_BDUAL_LONG_STEP");
    Prepared P = prepare_bounded(original, lower, upper, opt, updatePivot, true);
    const int R = P.R, C = P.C, Cm = C - 1;

    SimplexResult res;
    BoundedHandle th(R, C);
    int rc = lpx_tableau_upload(th.h, P.T.data(), P.basis.data());
    if (rc) throw_lib(rc);
    rc = lpx_tableau_set_bounds(th.h, Cm, P.ub.data()); if (rc) throw_lib(rc);
    int64_t dz[2] = {0, 0};
    rc = lpx_tableau_dualize(th.h, 1e-9, dz); if (rc) throw_lib(rc);       // every improving column to its other bound
    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.max_iter = opt.max_iter;
    o.batch = opt.batch;
    EventCtx ctx{updatePivot, &P.varNames};
    const int st = lpx_bounded_dual_run3(th.h, &o, flags, 0.0, updatePivot ? bounded_event : nullptr, &ctx, &res.Stats);
    finish_solve(th.h, st, original, lower, P, opt, [&dz](const int64_t* counts) {
        return "  dual start: " + std::to_string(dz[0]) + " dual-feasibility flips, " + std::to_string(counts[2]) + " passes\n";
    }, res, info);
    if (keep) {                                      // as SolveBounded fills it; a dual start makes no spare capacity
        keep->h = th.take(); keep->R = R; keep->C = C; keep->n = original.NumVars();
        keep->min = original.ObjectiveSense == Sense::Min; keep->shifted = P.shifted; keep->constant = P.constant;
        keep->lower = lower; keep->open_status = st; keep->opt = opt; keep->varNames = P.varNames;
        keep->spare = 0;
    }
    return res;
}

SimplexResult BoundedSetBounds(BoundedSession& s, int K, const int32_t* vars, const double* lower, const double* upper)
{
    const char* what = "Bounded session: ";
    if (K < 0) throw LpxException(LPX_EINVAL, std::string(what) + "K is negative");
    if (K > 0 && (!vars || !lower || !upper)) throw LpxException(LPX_EINVAL, std::string(what) + "null array");
    std::vector<uint8_t> seen((size_t)(s.n > 0 ? s.n : 1), 0);
    for (int k = 0; k < K; ++k) {
        if (vars[k] < 0 || vars[k] >= s.n) throw LpxException(LPX_EINVAL, std::string(what) + "variable index " + std::to_string(vars[k]) + " is outside the model");
        const std::string v = "x" + std::to_string(vars[k] + 1);
        if (seen[vars[k]]) throw LpxException(LPX_EINVAL, std::string(what) + v + " is listed twice");
        seen[vars[k]] = 1;
        CheckVarBounds(v, lower[k], upper[k]);
    }
    if (s.open_status != LPX_OPTIMAL) throw LpxException(LPX_EINVAL, std::string(what) + "the open solve did not end OPTIMAL, there is no tableau to continue from");
    // the handle's columns stand for x - l(open): the user's absolute bounds move by that shift, one subtraction each
    std::vector<double> lo((size_t)K), up((size_t)K);
    for (int k = 0; k < K; ++k) {
        const double l0 = s.lower.empty() ? 0.0 : s.lower[vars[k]];
        lo[k] = s.lower.empty() ? lower[k] : lower[k] - l0;
        up[k] = s.lower.empty() ? upper[k] : upper[k] - l0;
    }
    int rc = lpx_tableau_change_bounds(s.h, K, vars, lo.data(), up.data());
    if (rc) throw_lib(rc);
    SimplexResult res;
    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.max_iter = s.opt.max_iter;
    o.batch = s.opt.batch;
    const int st = lpx_bounded_dual_run(s.h, &o, nullptr, nullptr, &res.Stats);
    if (st < 0) throw_lib(st);
    if (st == LPX_ITER_LIMIT) throw LpxException(LPX_ITER_LIMIT, "Iteration limit exceeded.");
    int64_t counts[3] = {0, 0, 0};
    lpx_bounded_counts(s.h, counts);
    collect(s.h, st, s.n, s.R, s.C, s.lower, s.min, s.shifted, s.constant, std::string(), res, nullptr);
    res.VarNames = s.varNames;
    res.Aux = {(double)counts[0], (double)counts[1], 1.0, s.constant};
    return res;
}

}}  // namespace lpx::host
