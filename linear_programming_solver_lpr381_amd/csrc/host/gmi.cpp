// host/gmi.cpp -- the GMI cutting-plane loop (lpx_solve_cuts, include/lpx.h): root LP, then rounds of device cuts
// (lpx_tableau_gmi_round) each re-optimised in place by the dual loop, all on one device tableau with spare capacity.
// Per round the host reads the RHS column and the basis (integrality test) and the K new cut rows (x-space cuts).
#include "model.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

namespace lpx { int check_cut_opts(const lpx_cut_opts* o, const char* what); }

namespace lpx { namespace host {

namespace {

[[noreturn]] void throw_gmi(int rc)
{
    char buf[1024];
    lpx_last_error(buf, sizeof(buf));
    throw LpxException(rc, std::string("liblpx: ") + buf);
}
void chk(int rc) { if (rc < 0) throw_gmi(rc); }
void chk_hip(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw LpxException(LPX_EDEVICE, std::string("GMI Cutting Plane: ") + what + ": " + hipGetErrorString(e));
}

struct OwnedHandle {
    lpx_tableau* h = nullptr;
    ~OwnedHandle() { lpx_tableau_destroy(h); }
};

void append_trace(lpx_tableau* t, std::vector<int32_t>& out)
{
    int n = 0;
    chk(lpx_tableau_trace(t, nullptr, 0, &n));
    std::vector<int32_t> tr(2 * (size_t)(n > 0 ? n : 1));
    chk(lpx_tableau_trace(t, tr.data(), n, &n));
    out.insert(out.end(), tr.begin(), tr.begin() + 2 * (size_t)n);
}

// rows [r0, r0 + k) of the live window, C columns each
void download_rows(lpx_tableau* t, int r0, int k, int C, std::vector<double>& out)
{
    void* d = nullptr; int ld = 0;
    chk(lpx_tableau_device_ptr(t, &d, &ld));
    out.resize((size_t)k * C);
    if (k == 0) return;
    chk_hip(hipMemcpy2D(out.data(), sizeof(double) * C, (const double*)d + (size_t)r0 * ld, sizeof(double) * ld,
                        sizeof(double) * C, k, hipMemcpyDeviceToHost), "row download");
}

void rhs_and_basis(lpx_tableau* t, int R, int C, std::vector<double>& rhs, std::vector<int32_t>& basis)
{
    void* d = nullptr; int ld = 0;
    chk(lpx_tableau_device_ptr(t, &d, &ld));
    rhs.resize(R); basis.resize(R - 1);
    chk_hip(hipMemcpy2D(rhs.data(), sizeof(double), (const double*)d + (C - 1), sizeof(double) * ld, sizeof(double), R,
                        hipMemcpyDeviceToHost), "RHS download");
    chk(lpx_tableau_basis(t, basis.data()));
}

std::string fmt(double v) { char b[64]; std::snprintf(b, sizeof(b), "%.10g", v); return b; }

}  // namespace

SimplexResult GmiCuttingPlane::Solve(const LPProblem& problem, UpdatePivot updatePivot)
{
    if (int rc = check_cut_opts(&cut, "GMI Cutting Plane")) { char b[512]; lpx_last_error(b, sizeof b); throw LpxException(rc, b); }
    const int n = problem.NumVars();
    const LPProblem prep = PrepareForTableauDual(problem, true);
    std::vector<double> T; int R, C; std::vector<int32_t> basis; std::vector<std::string> names;
    BuildTableauPrimal(prep, T, R, C, basis, names);
    const int mx = R - 1, first_cut = C - 1;
    if (mx < 1) throw LpxException(LPX_EINVAL, "GMI Cutting Plane: the model has no constraints");
    const double sigma = problem.ObjectiveSense == Sense::Min ? -1.0 : 1.0;

    // integer mask: every structural variable; a slack iff its prepared row is integral
    std::vector<uint8_t> is_int(first_cut, 0);
    for (int j = 0; j < n; ++j) is_int[j] = 1;
    for (int k = 0; k < mx; ++k) {
        const Constraint& row = prep.Constraints[k];
        bool integral = row.B == std::floor(row.B);
        for (int j = 0; j < n; ++j) integral = integral && row.A[j] == std::floor(row.A[j]);
        is_int[n + k] = integral ? 1 : 0;
    }
    // x-space rows (A, B) whose slack is s = B - A.x: the prepared rows, then every cut added
    std::vector<std::vector<double>> rowA; std::vector<double> rowB;
    for (int k = 0; k < mx; ++k) { rowA.emplace_back(prep.Constraints[k].A.begin(), prep.Constraints[k].A.begin() + n); rowB.push_back(prep.Constraints[k].B); }
    std::vector<int> colcut;        // cut id (index into rowA) of the cut slack columns first_cut, first_cut + 1, ...

    OwnedHandle th;
    chk(lpx_tableau_create(R + cut.max_active, C + cut.max_active, &th.h));
    chk(lpx_tableau_set_shape(th.h, R, C));
    chk(lpx_tableau_upload(th.h, T.data(), basis.data()));

    SimplexResult res;
    std::string report = "GMI cutting planes (K = " + std::to_string(cut.cuts_per_round) + ", max rounds " +
                         std::to_string(cut.max_rounds) + ", max active " + std::to_string(cut.max_active) + ")\n";
    bool nonneg = true;
    for (int i = 0; i < mx; ++i) if (!(T[(size_t)i * C + C - 1] >= 0)) nonneg = false;
    lpx_stats st{};
    int status;
    if (nonneg) {
        lpx_run_opts o; lpx_default_opts(&o, 0); o.max_iter = opt.max_iter; o.batch = opt.batch;
        status = lpx_primal_run(th.h, &o, nullptr, nullptr, &st);
    } else {
        lpx_run_opts o; lpx_default_opts(&o, 1); o.max_iter = opt.max_iter; o.batch = opt.batch;
        o.fdf_guard = opt.max_iter; o.cleanup = 1;
        status = lpx_dual_run(th.h, &o, nullptr, nullptr, &st);
    }
    chk(status);
    if (status == LPX_ITER_LIMIT) throw LpxException(LPX_ITER_LIMIT, "Iteration limit exceeded.");
    append_trace(th.h, res.Trace);
    res.Stats = st;

    std::vector<double> rhs; std::vector<int32_t> bs;
    int Rc = R, Cc = C;
    rhs_and_basis(th.h, Rc, Cc, rhs, bs);
    const double root_z = sigma * rhs[Rc - 1];
    report += std::string("Root LP (") + (nonneg ? "primal" : "dual") + "): " + (status == LPX_OPTIMAL ? "OPTIMAL" : status == LPX_UNBOUNDED ? "UNBOUNDED" : "INFEASIBLE") +
              ", bound " + fmt(root_z) + ", " + std::to_string(st.pivots) + " pivots\n";
    if (updatePivot) updatePivot(report, nullptr);

    int rounds = 0; int64_t added = 0, purged = 0;
    std::vector<int32_t> src(cut.cuts_per_round), pcols(C + cut.max_active);
    std::vector<double> rows;
    if (status == LPX_OPTIMAL) {
        status = LPX_CUT_INCOMPLETE;
        for (;;) {
            bool integral = true;
            for (int r = 0; r < Rc - 1; ++r) {
                const int j = bs[r];
                if (j < first_cut && is_int[j] && std::fabs(rhs[r] - std::nearbyint(rhs[r])) > cut.int_tol) { integral = false; break; }
            }
            if (integral) { status = LPX_CUT_INTEGER; break; }
            if (rounds >= cut.max_rounds) { report += "Round cap reached\n"; break; }
            int K = 0, P = 0;
            chk(lpx_tableau_gmi_round(th.h, is_int.data(), first_cut, first_cut, &cut, &K, src.data(), &P, pcols.data()));
            // purged cut slacks leave the column list; the new ones go to its end
            for (int i = P - 1; i >= 0; --i) colcut.erase(colcut.begin() + (pcols[i] - first_cut));
            purged += P;
            if (K == 0) { report += "Round " + std::to_string(rounds + 1) + ": no cut passes the filters (stalled)\n"; break; }
            chk(lpx_tableau_shape(th.h, &Rc, &Cc, nullptr));
            download_rows(th.h, Rc - 1 - K, K, Cc, rows);
            const int nold = Cc - 1 - K;                  // columns before the new slacks
            for (int k = 0; k < K; ++k) {
                const double* e = rows.data() + (size_t)k * Cc;
                std::vector<double> a(n, 0.0); double cst = 0.0;
                for (int j = 0; j < nold; ++j) {
                    if (e[j] == 0.0) continue;
                    const double al = -e[j];
                    if (j < n) { a[j] += al; continue; }
                    const int id = j < first_cut ? j - n : colcut[j - first_cut];
                    for (int q = 0; q < n; ++q) a[q] -= al * rowA[id][q];
                    cst += al * rowB[id];
                }
                for (double& v : a) v = -v;                // a'.x + cst >= 1  <=>  -a'.x <= cst - 1
                colcut.push_back((int)rowA.size());
                rowA.push_back(a); rowB.push_back(cst - 1.0);
                res.NodeLog.push_back(rounds + 1); res.NodeLog.push_back(src[k]); res.NodeLog.push_back(nold + k);
            }
            added += K;
            lpx_run_opts o; lpx_default_opts(&o, 1); o.max_iter = opt.max_iter; o.batch = opt.batch;
            o.fdf_guard = 0; o.cleanup = 1;
            lpx_stats ds{};
            const int ds_status = lpx_dual_run(th.h, &o, nullptr, nullptr, &ds);
            chk(ds_status);
            if (ds_status == LPX_ITER_LIMIT) throw LpxException(LPX_ITER_LIMIT, "Iteration limit exceeded (Dual Simplex).");
            append_trace(th.h, res.Trace);
            res.Stats.pivots += ds.pivots; res.Stats.launches += ds.launches; res.Stats.loop_ms += ds.loop_ms;
            res.Stats.fdf_pivots += ds.fdf_pivots; res.Stats.cleanup_pivots += ds.cleanup_pivots;
            ++rounds;
            rhs_and_basis(th.h, Rc, Cc, rhs, bs);
            const double z = sigma * rhs[Rc - 1];
            for (int k = 0; k < K; ++k) res.NodeZ.push_back(z);
            std::string line = "Round " + std::to_string(rounds) + ": +" + std::to_string(K) + " cuts (rows";
            for (int k = 0; k < K; ++k) line += " " + std::to_string(src[k]);
            line += "), -" + std::to_string(P) + " purged, " + std::to_string(Rc) + "x" + std::to_string(Cc) + ", " +
                    std::to_string(ds.pivots) + " dual pivots, ";
            if (ds_status == LPX_INFEASIBLE) { report += line + "LP infeasible: the IP has no integer point\n"; status = LPX_INFEASIBLE; break; }
            line += "bound " + fmt(z) + "\n";
            report += line;
            if (updatePivot) updatePivot(line, nullptr);
            if (ds_status != LPX_OPTIMAL) { status = ds_status; break; }
        }
    }

    // final tableau, x, z
    chk(lpx_tableau_shape(th.h, &Rc, &Cc, nullptr));
    T.assign((size_t)Rc * Cc, 0.0); basis.assign(Rc - 1, 0);
    chk(lpx_tableau_download(th.h, T.data(), basis.data()));
    std::vector<double> x(n, 0.0);
    for (int r = 0; r < Rc - 1; ++r) if (basis[r] < n) x[basis[r]] = T[(size_t)r * Cc + Cc - 1];
    const double z = T[(size_t)(Rc - 1) * Cc + Cc - 1];
    names.resize(Cc - 1);
    for (int j = first_cut; j < Cc - 1; ++j) names[j] = "g" + std::to_string(j - first_cut + 1);

    const char* stxt = status == LPX_CUT_INTEGER ? "OPTIMAL INTEGER" : status == LPX_CUT_INCOMPLETE ? "INCOMPLETE (LP bound)" :
                       status == LPX_INFEASIBLE ? "INFEASIBLE" : status == LPX_UNBOUNDED ? "UNBOUNDED" : "?";
    report += std::string("\nStatus: ") + stxt + "\n";
    for (int j = 0; j < n; ++j) report += "  x" + std::to_string(j + 1) + " = " + FormatRound3(x[j]) + "\n";
    report += "  z = " + FormatRound3(sigma * z) + "\n";
    res.Summary = std::string("Status: ") + stxt + "\nz = " + FormatRound3(sigma * z) + "\nrounds = " + std::to_string(rounds) +
                  ", cuts added = " + std::to_string(added) + ", purged = " + std::to_string(purged) + "\n";
    res.Report = report;
    res.Status = status;
    res.OptimalValue = sigma * z;
    res.Solution = x; res.HasSolution = true;
    res.Tableau = std::move(T); res.R = Rc; res.C = Cc;
    res.Basis = std::move(basis); res.VarNames = std::move(names);
    res.LpSolves = 1 + rounds;
    res.Aux = {(double)rounds, (double)added, (double)purged, root_z};
    for (size_t g = mx; g < rowA.size(); ++g) {
        res.Cuts.insert(res.Cuts.end(), rowA[g].begin(), rowA[g].end());
        res.Cuts.push_back(rowB[g]);
    }
    return res;
}

}}  // namespace lpx::host
