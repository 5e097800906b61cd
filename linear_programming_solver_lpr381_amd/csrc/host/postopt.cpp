// host/postopt.cpp -- the warm post-optimal session (lpx_session_*, include/lpx.h): one device tableau holds the solved model,
// and every edit of b, c, a new variable or a new constraint is applied by the device combinations of lpx_postopt.hip, then
// re-optimised by a short primal or dual run on the same handle.  Per edit the host moves the edit's own data to the device
// and reads back the basis and the RHS column (x, z); the tableau only when asked for.
#include "model.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace lpx { int ensure_device(); void set_error(const std::string& msg); }

using namespace lpx::host;

struct lpx_session {
    LPProblem q;                          // the user's model as it stands (original + added variables and constraints)
    lpx_session_opts o;
    double sigma = 1.0;                   // -1 for Min: the tableau holds the prepared Max model
    std::vector<int> row_of, sign;        // prepared row k -> user constraint, sign
    std::vector<int> slack_col, var_col;  // prepared row k -> its slack's column; user variable j -> its column
    lpx_tableau* t = nullptr;
    int R = 0, C = 0, Rcap = 0, Ccap = 0;
    int status = LPX_OPTIMAL;             // of the last solve on the handle
    ~lpx_session() { lpx_tableau_destroy(t); }
};

namespace {

[[noreturn]] void throw_po(int rc)
{
    char buf[1024];
    lpx_last_error(buf, sizeof(buf));
    throw LpxException(rc, std::string("liblpx: ") + buf);
}
void chk(int rc) { if (rc < 0) throw_po(rc); }
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T> T* dup_vec(const std::vector<T>& v)
{
    T* p = (T*)std::malloc(sizeof(T) * (v.size() ? v.size() : 1));
    if (!v.empty()) std::memcpy(p, v.data(), sizeof(T) * v.size());
    return p;
}
char* dup_str(const std::string& s) { char* p = (char*)std::malloc(s.size() + 1); std::memcpy(p, s.c_str(), s.size() + 1); return p; }

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

template <class F> int guarded(const char* what, F&& f)
{
    try { return f(); }
    catch (const LpxException& ex) { lpx::set_error(ex.what()); return ex.code; }
    catch (const std::exception& ex) { lpx::set_error(std::string(what) + ": " + ex.what()); return LPX_EINVAL; }
}

// RHS column (R entries) of the live window
void rhs_column(lpx_session* s, std::vector<double>& rhs)
{
    void* d = nullptr; int ld = 0;
    chk(lpx_tableau_device_ptr(s->t, &d, &ld));
    rhs.resize(s->R);
    if (hipMemcpy2D(rhs.data(), sizeof(double), (const double*)d + (s->C - 1), sizeof(double) * ld, sizeof(double), s->R,
                    hipMemcpyDeviceToHost) != hipSuccess)
        throw LpxException(LPX_EDEVICE, "lpx_session: RHS download failed");
}

struct RunOut { int status = LPX_OPTIMAL; lpx_stats st{}; std::vector<int32_t> trace; };

void read_trace(lpx_session* s, RunOut& r)
{
    int n = 0;
    chk(lpx_tableau_trace(s->t, nullptr, 0, &n));
    r.trace.assign(2 * (size_t)(n > 0 ? n : 1), 0);
    chk(lpx_tableau_trace(s->t, r.trace.data(), n, &n));
    r.trace.resize(2 * (size_t)n);
}

RunOut run(lpx_session* s, bool dual, int fdf_guard)
{
    RunOut r;
    lpx_run_opts o; lpx_default_opts(&o, dual ? 1 : 0);
    o.max_iter = s->o.max_iter; o.batch = s->o.batch;
    if (dual) { o.fdf_guard = fdf_guard; o.cleanup = 1; }
    r.status = dual ? lpx_dual_run(s->t, &o, nullptr, nullptr, &r.st) : lpx_primal_run(s->t, &o, nullptr, nullptr, &r.st);
    chk(r.status);
    read_trace(s, r);
    return r;
}

// lpx_session_open's solve (and the cold path): prepare the current model, build it into the handle in the standard layout
// [x | slacks | RHS], lpx_primal_run when every prepared b >= 0, else the repaired dual
RunOut solve_cold(lpx_session* s)
{
    const LPProblem prep = PrepareForTableauDual(s->q, true);
    std::vector<double> T; int R, C; std::vector<int32_t> basis; std::vector<std::string> names;
    BuildTableauPrimal(prep, T, R, C, basis, names);
    PreparedRows(s->q, true, true, s->row_of, s->sign);
    const int n = s->q.NumVars(), mx = R - 1;
    s->var_col.resize(n); s->slack_col.resize(mx);
    for (int j = 0; j < n; ++j) s->var_col[j] = j;
    for (int k = 0; k < mx; ++k) s->slack_col[k] = n + k;
    chk(lpx_tableau_set_shape(s->t, R, C));
    chk(lpx_tableau_upload(s->t, T.data(), basis.data()));
    s->R = R; s->C = C;
    bool nonneg = true;
    for (int i = 0; i < mx; ++i) if (!(T[(size_t)i * C + C - 1] >= 0)) nonneg = false;
    RunOut r = run(s, !nonneg, s->o.max_iter);
    s->status = r.status;
    return r;
}

RunOut solve_dual_if_infeasible(lpx_session* s)
{
    std::vector<double> rhs;
    rhs_column(s, rhs);
    double mn = HUGE_VAL;
    for (int i = 0; i + 1 < s->R; ++i) mn = rhs[i] < mn ? rhs[i] : mn;
    RunOut r;
    if (mn < -1e-9) r = run(s, true, 0);
    s->status = r.status;
    return r;
}

void fill(lpx_session* s, const RunOut& r, int warm, const char* what, lpx_result* out)
{
    std::memset(out, 0, sizeof(*out));
    if (r.status == LPX_ITER_LIMIT) throw LpxException(LPX_ITER_LIMIT, "Iteration limit exceeded.");
    const int n = s->q.NumVars();
    std::vector<double> rhs;
    std::vector<int32_t> basis(s->R - 1);
    rhs_column(s, rhs);
    chk(lpx_tableau_basis(s->t, basis.data()));
    std::vector<int> var_of_col(s->C, -1);
    for (int j = 0; j < n; ++j) var_of_col[s->var_col[j]] = j;
    std::vector<double> x(n, 0.0);
    for (int i = 0; i + 1 < s->R; ++i) if (var_of_col[basis[i]] >= 0) x[var_of_col[basis[i]]] = rhs[i];
    const double z = rhs[s->R - 1];
    out->status = r.status;
    out->has_solution = 1;
    out->optimal_value = s->sigma * z;
    out->n = n; out->x = dup_vec(x);
    out->R = s->R; out->C = s->C;
    if (s->o.want_tableau) {
        std::vector<double> T((size_t)s->R * s->C);
        chk(lpx_tableau_download(s->t, T.data(), nullptr));
        out->T = dup_vec(T);
    }
    out->basis = dup_vec(basis);
    out->n_pivots = (int)(r.trace.size() / 2); out->trace = dup_vec(r.trace);
    const char* stxt = r.status == LPX_OPTIMAL ? "OPTIMAL" : r.status == LPX_UNBOUNDED ? "UNBOUNDED" : r.status == LPX_INFEASIBLE ? "INFEASIBLE" : "?";
    char line[256];
    std::snprintf(line, sizeof line, "%s (%s): %s, z = %.10g, %d pivots\n", what, warm ? "warm" : "cold", stxt, s->sigma * z, out->n_pivots);
    std::string rep = line;
    for (int j = 0; j < n; ++j) rep += "  x" + std::to_string(j + 1) + " = " + FormatRound3(x[j]) + "\n";
    out->report = dup_str(rep);
    out->summary = dup_str(std::string("Status: ") + stxt + "\nz = " + FormatRound3(s->sigma * z) + "\n");
    out->lp_solves = 1;
    out->aux[0] = warm;
    out->stats = r.st;
    out->cuts = nullptr;
}

int check_session(lpx_session* s, lpx_result* res, const char* what)
{
    if (!s || !res) { lpx::set_error(std::string(what) + ": null argument"); return LPX_EINVAL; }
    return 0;
}

// the edit could not be applied warm: the model (already edited) is rebuilt and solved cold on the same handle
int cold(lpx_session* s, const char* what, lpx_result* res)
{
    RunOut r = solve_cold(s);
    fill(s, r, 0, what, res);
    return 0;
}

}  // namespace

extern "C" {

void lpx_default_session_opts(lpx_session_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->extra_rows = 16; o->extra_cols = 16; o->max_iter = 10000;
}

int lpx_session_open(const lpx_problem* p, const lpx_session_opts* o, lpx_session** out, lpx_result* res)
{
    static const char* what = "lpx_session_open";
    if (!p || !out || !res) { lpx::set_error(std::string(what) + ": null argument"); return LPX_EINVAL; }
    *out = nullptr;
    std::memset(res, 0, sizeof(*res));
    lpx_session_opts d; lpx_default_session_opts(&d);
    if (!o) o = &d;
    if (o->extra_rows < 0 || o->extra_cols < 0 || o->max_iter < 0) { lpx::set_error(std::string(what) + ": negative option"); return LPX_EINVAL; }
    if (p->n < 1 || p->m < 1 || !p->c || !p->A || !p->rel || !p->b) { lpx::set_error(std::string(what) + ": the model needs variables and constraints"); return LPX_EINVAL; }
    for (int i = 0; i < p->m; ++i)
        if (p->rel[i] != LPX_LE && p->rel[i] != LPX_GE && p->rel[i] != LPX_EQ) { lpx::set_error(std::string(what) + ": bad relation"); return LPX_EINVAL; }
    if (int rc = lpx::ensure_device()) return rc;
    return guarded(what, [&]() -> int {
        lpx_session* s = new lpx_session();
        try {
            s->q = to_problem(p);
            s->o = *o;
            if (s->o.max_iter == 0) s->o.max_iter = 10000;
            s->sigma = s->q.ObjectiveSense == Sense::Min ? -1.0 : 1.0;
            std::vector<int> row_of, sign;
            PreparedRows(s->q, true, true, row_of, sign);
            const int mx = (int)row_of.size();
            s->Rcap = mx + 1 + s->o.extra_rows;
            s->Ccap = p->n + mx + 1 + s->o.extra_cols;
            chk(lpx_tableau_create(s->Rcap, s->Ccap, &s->t));
            RunOut r = solve_cold(s);
            fill(s, r, 1, "open", res);
            // the first dual run of a handle pays a one-time setup: pay it here, not in the first edit
            if (r.status == LPX_OPTIMAL) {
                const double t0 = now_ms();
                RunOut w = run(s, true, 0);
                res->aux[1] = now_ms() - t0;
                s->status = w.status;
            }
            *out = s;
            return 0;
        } catch (...) {
            delete s;
            throw;
        }
    });
}

int lpx_session_set_rhs(lpx_session* s, int K, const int32_t* cons, const double* b, lpx_result* res)
{
    static const char* what = "lpx_session_set_rhs";
    if (int rc = check_session(s, res, what)) return rc;
    std::memset(res, 0, sizeof(*res));
    const int m = (int)s->q.Constraints.size();
    if (K < 0 || (K > 0 && (!cons || !b))) { lpx::set_error(std::string(what) + ": bad term arrays"); return LPX_EINVAL; }
    for (int k = 0; k < K; ++k) if (cons[k] < 0 || cons[k] >= m) { lpx::set_error(std::string(what) + ": constraint index out of range"); return LPX_EINVAL; }
    return guarded(what, [&]() -> int {
        const bool warm = s->status == LPX_OPTIMAL;
        std::vector<double> delta(m, 0.0);
        std::vector<uint8_t> touched(m, 0);
        std::vector<double> b0(m);
        for (int i = 0; i < m; ++i) b0[i] = s->q.Constraints[i].B;
        for (int k = 0; k < K; ++k) {       // the last value given for a constraint wins
            delta[cons[k]] = b[k] - b0[cons[k]];
            touched[cons[k]] = 1;
            s->q.Constraints[cons[k]].B = b[k];
        }
        if (!warm) return cold(s, "set_rhs", res);
        std::vector<int32_t> cols; std::vector<double> v;
        for (size_t k = 0; k < s->row_of.size(); ++k) {
            const int i = s->row_of[k];
            if (!touched[i]) continue;
            cols.push_back(s->slack_col[k]);
            v.push_back(s->sign[k] < 0 ? -delta[i] : delta[i]);
        }
        chk(lpx_tableau_rhs_update(s->t, (int)cols.size(), cols.data(), v.data()));
        RunOut r = solve_dual_if_infeasible(s);
        fill(s, r, 1, "set_rhs", res);
        return 0;
    });
}

int lpx_session_set_cost(lpx_session* s, int K, const int32_t* vars, const double* c, lpx_result* res)
{
    static const char* what = "lpx_session_set_cost";
    if (int rc = check_session(s, res, what)) return rc;
    std::memset(res, 0, sizeof(*res));
    const int n = s->q.NumVars();
    if (K < 0 || (K > 0 && (!vars || !c))) { lpx::set_error(std::string(what) + ": bad term arrays"); return LPX_EINVAL; }
    for (int k = 0; k < K; ++k) if (vars[k] < 0 || vars[k] >= n) { lpx::set_error(std::string(what) + ": variable index out of range"); return LPX_EINVAL; }
    return guarded(what, [&]() -> int {
        const bool warm = s->status == LPX_OPTIMAL;
        std::vector<double> delta(n, 0.0);
        std::vector<uint8_t> touched(n, 0);
        std::vector<double> c0 = s->q.C;
        for (int k = 0; k < K; ++k) {       // the last value given for a variable wins
            const double d = c[k] - c0[vars[k]];
            delta[vars[k]] = s->sigma < 0 ? -d : d;
            touched[vars[k]] = 1;
            s->q.C[vars[k]] = c[k];
        }
        if (!warm) return cold(s, "set_cost", res);
        std::vector<int32_t> basis(s->R - 1);
        chk(lpx_tableau_basis(s->t, basis.data()));
        std::vector<int> row_of_col(s->C, -1);
        for (int i = 0; i + 1 < s->R; ++i) row_of_col[basis[i]] = i;
        std::vector<int32_t> rows, dcols; std::vector<double> w, dd;
        for (int j = 0; j < n; ++j) {
            if (!touched[j]) continue;
            const int col = s->var_col[j], r = row_of_col[col];
            if (r >= 0) { rows.push_back(r); w.push_back(delta[j]); }
            else { dcols.push_back(col); dd.push_back(delta[j]); }
        }
        chk(lpx_tableau_objective_update(s->t, (int)rows.size(), rows.data(), w.data(), (int)dcols.size(), dcols.data(), dd.data()));
        RunOut r = run(s, false, 0);
        s->status = r.status;
        fill(s, r, 1, "set_cost", res);
        return 0;
    });
}

int lpx_session_add_variable(lpx_session* s, double c, const double* a, lpx_result* res)
{
    static const char* what = "lpx_session_add_variable";
    if (int rc = check_session(s, res, what)) return rc;
    std::memset(res, 0, sizeof(*res));
    if (!a) { lpx::set_error(std::string(what) + ": null column"); return LPX_EINVAL; }
    if (s->C + 1 > s->Ccap) { lpx::set_error(std::string(what) + ": no spare column capacity (opts.extra_cols)"); return LPX_EINVAL; }
    return guarded(what, [&]() -> int {
        const bool warm = s->status == LPX_OPTIMAL;
        const int m = (int)s->q.Constraints.size();
        s->q.C.push_back(c);
        for (int i = 0; i < m; ++i) s->q.Constraints[i].A.push_back(a[i]);
        if (!warm) return cold(s, "add_variable", res);
        std::vector<int32_t> cols; std::vector<double> v;
        for (size_t k = 0; k < s->row_of.size(); ++k) {
            const double ai = a[s->row_of[k]];
            if (ai == 0.0) continue;
            cols.push_back(s->slack_col[k]);
            v.push_back(s->sign[k] < 0 ? -ai : ai);
        }
        const double cp = s->sigma < 0 ? -c : c;
        chk(lpx_tableau_add_column(s->t, (int)cols.size(), cols.data(), v.data(), -cp));
        s->var_col.push_back(s->C - 1);
        s->C += 1;
        RunOut r = run(s, false, 0);
        s->status = r.status;
        fill(s, r, 1, "add_variable", res);
        return 0;
    });
}

int lpx_session_add_constraint(lpx_session* s, const double* a, int rel, double b, lpx_result* res)
{
    static const char* what = "lpx_session_add_constraint";
    if (int rc = check_session(s, res, what)) return rc;
    std::memset(res, 0, sizeof(*res));
    if (!a) { lpx::set_error(std::string(what) + ": null row"); return LPX_EINVAL; }
    if (rel != LPX_LE && rel != LPX_GE && rel != LPX_EQ) { lpx::set_error(std::string(what) + ": bad relation"); return LPX_EINVAL; }
    const int nrows = rel == LPX_EQ ? 2 : 1;
    if (s->R + nrows > s->Rcap || s->C + nrows > s->Ccap) {
        lpx::set_error(std::string(what) + ": no spare capacity (opts.extra_rows / opts.extra_cols)");
        return LPX_EINVAL;
    }
    return guarded(what, [&]() -> int {
        const bool warm = s->status == LPX_OPTIMAL;
        const int n = s->q.NumVars(), i_new = (int)s->q.Constraints.size();
        Constraint cons;
        cons.A.assign(a, a + n);
        cons.Relation = rel == LPX_GE ? Rel::GE : (rel == LPX_EQ ? Rel::EQ : Rel::LE);
        cons.B = b;
        s->q.Constraints.push_back(cons);
        if (!warm) return cold(s, "add_constraint", res);
        std::vector<int> signs;
        if (rel == LPX_LE) signs = {1};
        else if (rel == LPX_GE) signs = {-1};
        else signs = {1, -1};
        for (int sg : signs) {
            std::vector<int32_t> basis(s->R - 1);
            chk(lpx_tableau_basis(s->t, basis.data()));
            std::vector<int> var_of_col(s->C, -1);
            for (int j = 0; j < n; ++j) var_of_col[s->var_col[j]] = j;
            // the prepared row in the new shape: sign * a over the variables' columns, 1 in its own slack, sign * b
            std::vector<double> base((size_t)s->C + 1, 0.0);
            for (int j = 0; j < n; ++j) base[s->var_col[j]] = sg < 0 ? -a[j] : a[j];
            base[s->C - 1] = 1.0;
            base[s->C] = sg < 0 ? -b : b;
            std::vector<int32_t> rows; std::vector<double> w;
            for (int r = 0; r + 1 < s->R; ++r) {
                const int j = var_of_col[basis[r]];
                if (j < 0 || a[j] == 0.0) continue;
                const double ap = sg < 0 ? -a[j] : a[j];
                rows.push_back(r); w.push_back(-ap);
            }
            chk(lpx_tableau_add_row(s->t, (int)rows.size(), rows.data(), w.data(), base.data()));
            s->row_of.push_back(i_new); s->sign.push_back(sg);
            s->slack_col.push_back(s->C - 1);
            s->R += 1; s->C += 1;
        }
        RunOut r = solve_dual_if_infeasible(s);
        fill(s, r, 1, "add_constraint", res);
        return 0;
    });
}

int lpx_session_ranging(lpx_session* s, lpx_ranging* rg)
{
    if (!s || !rg) { lpx::set_error("lpx_session_ranging: null argument"); return LPX_EINVAL; }
    std::memset(rg, 0, sizeof(*rg));
    const int rc = guarded("lpx_session_ranging", [&]() -> int {
        RangingAlloc(rg, s->q.NumVars(), (int)s->q.Constraints.size());
        RangingMap map;
        map.q = &s->q; map.row_of = s->row_of; map.sign = s->sign; map.slack_col = s->slack_col; map.var_col = s->var_col;
        RawRanging raw;
        if (s->status == LPX_OPTIMAL) RangeTableau(s->t, map, raw);
        RangingToUser(map, raw, s->status, rg);
        return 0;
    });
    if (rc != 0) lpx_ranging_free(rg);
    return rc;
}

int lpx_session_shape(const lpx_session* s, int* n_vars, int* n_cons)
{
    if (!s) { lpx::set_error("lpx_session_shape: null session"); return LPX_EINVAL; }
    if (n_vars) *n_vars = s->q.NumVars();
    if (n_cons) *n_cons = (int)s->q.Constraints.size();
    return 0;
}

void lpx_session_close(lpx_session* s) { delete s; }

}  // extern "C"
