// host/bnb_nodes.cpp -- one node of the BranchAndBound mirror (host/bnb.cpp): its LP, prepared, solved, tested.
//
// Every node is an LP rebuilt from the root model plus its branching rows and re-solved from the slack basis on the GPU, exactly
// as the reference re-solves through LPSolver (Models/Branch&Bound.cs:148); the warm search's children start from their parked
// parent instead.  The searches hand whole groups of nodes to solve_group, which keeps opt.concurrent_nodes of them on the device.
#include "bnb_nodes.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace lpx { namespace host { namespace bnb {

PhaseTimer::PhaseTimer() { const char* e = std::getenv("LPX_BNB_TIMING"); on = e && e[0] == '1'; }
PhaseTimer::~PhaseTimer() { if (on) std::fprintf(stderr, "[lpx bnb] root %.1f ms, build %.1f ms, run %.1f ms, collect %.1f ms (read-back %.1f, parking %.1f), decide %.1f ms, whole solves %.1f ms; no window in flight %d times, %.1f ms (longest %.1f)\n", root, build, run, collect, readback, parking, decide, total, drains, drained, drained_max); }
PhaseTimer g_pt;

std::string last_error() { char b[1024]; lpx_last_error(b, sizeof(b)); return b; }

namespace {

// Creating a handle costs ~4 ms (device and pinned allocations, a stream) and destroying it ~3 ms, so handles outlive the solve
// that made them: a finished pool parks them in a process-wide cache (bounded) and the next solve of the same shape class takes
// them from there.
struct HandleCache {
    std::map<std::pair<int, int>, std::vector<lpx_tableau*>> free_;
    size_t count = 0;
    static constexpr size_t kMax = 512;
    lpx_tableau* take(int R, int C) {
        auto it = free_.find({R, C});
        if (it == free_.end() || it->second.empty()) return nullptr;
        lpx_tableau* t = it->second.back(); it->second.pop_back(); --count;
        return t;
    }
    void park(lpx_tableau* t, int R, int C) {
        if (count >= kMax) { lpx_tableau_destroy(t); return; }
        free_[{R, C}].push_back(t); ++count;
    }
};
HandleCache g_handle_cache;     // never destroyed: the HIP runtime may be gone by the time statics are torn down

}  // namespace

lpx_tableau* HandlePool::get(int R, int C)
{
    auto& v = free_[{R, C}];
    if (!v.empty()) { lpx_tableau* t = v.back(); v.pop_back(); return t; }
    lpx_tableau* t = g_handle_cache.take(R, C);
    if (!t) {
        int rc = lpx_tableau_create(R, C, &t);
        if (rc) throw LpxException(rc, "liblpx: " + last_error());
    }
    all_.push_back(t);
    cap_[t] = {R, C};
    return t;
}
HandlePool::~HandlePool() { for (lpx_tableau* t : all_) g_handle_cache.park(t, cap_[t].first, cap_[t].second); }

void FeasIndex::build(const LPProblem& root)
{
    n = root.NumVars();
    const int m = (int)root.Constraints.size();
    for (int r = 0; r < m; ++r) {
        const Constraint& c = root.Constraints[(size_t)r];
        int nnz = 0; for (int i = 0; i < n; ++i) if (c.A[(size_t)i] != 0.0) ++nnz;
        if (nnz * 8 > n) dense_rows.push_back(r);
        else { Sparse s; s.row = r; for (int i = 0; i < n; ++i) if (c.A[(size_t)i] != 0.0) s.nz.emplace_back(i, c.A[(size_t)i]); sparse.push_back(std::move(s)); }
    }
    const size_t nd = dense_rows.size();
    ATd.assign((size_t)n * nd, 0.0);
    for (size_t d = 0; d < nd; ++d) { const Constraint& c = root.Constraints[(size_t)dense_rows[d]]; for (int i = 0; i < n; ++i) ATd[(size_t)i * nd + d] = c.A[(size_t)i]; }
    built = true;
}

lpx_store* Ctx::store_for(lpx_tableau* h)
{
    const std::pair<int, int> cap = pool.cap_[h];
    auto it = stores.find(cap);
    if (it != stores.end()) return it->second;
    lpx_store* s = nullptr;
    int rc = lpx_store_create(cap.first, cap.second, &s);
    if (rc) throw LpxException(rc, "liblpx: " + last_error());
    stores[cap] = s;
    return s;
}
Ctx::~Ctx() { for (int w = 0; w < 2; ++w) release_exact_handle(root_tpl[w], tplR[w], tplC[w]); for (auto& kv : stores) lpx_store_destroy(kv.second); }

static LPProblem make_node(const LPProblem& root, const std::vector<Cut>& cuts)
{
    LPProblem p = root.Clone();                                   // :233, :242
    for (const Cut& c : cuts) {
        Constraint k; k.A.assign(root.NumVars(), 0.0); k.A[c.var] = 1.0;   // UnitVector, :298-303
        k.Relation = c.rel; k.B = c.bound;
        p.Constraints.push_back(k);
    }
    return p;
}

bool has_ge_or_eq(const LPProblem& p)                             // ChooseAlgorithm, :262-266
{
    for (const Constraint& c : p.Constraints) if (c.Relation == Rel::GE || c.Relation == Rel::EQ) return true;
    return false;
}

bool IsIntegral(const std::vector<double>& x)                     // :268-274
{
    for (double v : x) if (std::fabs(v - std::nearbyint(v)) > EPS) return false;
    return true;
}

static bool rel_ok(Rel rel, double sum, double B)
{
    if (rel == Rel::LE && sum > B + EPS) return false;
    if (rel == Rel::GE && sum < B - EPS) return false;
    if (rel == Rel::EQ && std::fabs(sum - B) > EPS) return false;
    return true;
}

// IsFeasible, :276-294, on the node = root constraints followed by its branching rows (same order as
// the cloned problem of the reference, without materialising the clone)
bool IsFeasible(const std::vector<double>& x, const LPProblem& root, const std::vector<Cut>& cuts)
{
    for (const Constraint& c : root.Constraints) {
        double sum = 0;
        for (size_t i = 0; i < x.size(); ++i) sum += c.A[i] * x[i];
        if (!rel_ok(c.Relation, sum, c.B)) return false;
    }
    for (const Cut& k : cuts) {
        double sum = 0;                                     // UnitVector row: 0*x_i terms add exact zeros
        for (size_t i = 0; i < x.size(); ++i) sum += ((int)i == k.var ? 1.0 : 0.0) * x[i];
        if (!rel_ok(k.rel, sum, k.bound)) return false;
    }
    for (double v : x) if (v < -EPS) return false;
    return true;
}

// The same test with the work laid out for the host's caches: identical sums, hence identical verdicts.
//  * a product with x_i == 0 is +-0 and leaves a running sum unchanged (the sums start at +0 and IEEE addition of a
//    zero never changes a value; the sign of a zero sum plays no part in the comparisons), so zero entries are skipped;
//  * rows with many coefficients are kept transposed ([variable][dense row]): the loop over the rows is contiguous and
//    every row still accumulates its terms in ascending variable order, one rounded multiply and one rounded add each
//    (the host code is built with -ffp-contract=off);
//  * rows with a few coefficients (the x_j <= 1 rows of a binary program) keep a list of their non-zeros;
//  * a branching row is a unit vector: its sum is x_k itself.
// Non-finite values fall back to the plain loop (0 * inf is not a zero).
bool IsFeasibleIndexed(const std::vector<double>& x, const LPProblem& root, const std::vector<Cut>& cuts, FeasIndex& ix)
{
    if (!ix.built) ix.build(root);
    for (double v : x) if (!std::isfinite(v)) return IsFeasible(x, root, cuts);
    for (const Constraint& c : root.Constraints) if ((int)c.A.size() < ix.n) return IsFeasible(x, root, cuts);
    const size_t nd = ix.dense_rows.size();
    std::vector<double> sums(nd, 0.0);
    for (int i = 0; i < ix.n && i < (int)x.size(); ++i) {
        const double xi = x[(size_t)i];
        if (xi == 0.0) continue;
        const double* col = ix.ATd.data() + (size_t)i * nd;
        for (size_t d = 0; d < nd; ++d) sums[d] += col[d] * xi;
    }
    for (size_t d = 0; d < nd; ++d) { const Constraint& c = root.Constraints[(size_t)ix.dense_rows[d]]; if (!rel_ok(c.Relation, sums[d], c.B)) return false; }
    for (const FeasIndex::Sparse& s : ix.sparse) {
        double sum = 0;
        for (const auto& e : s.nz) if ((size_t)e.first < x.size()) sum += e.second * x[(size_t)e.first];
        if (!rel_ok(root.Constraints[(size_t)s.row].Relation, sum, root.Constraints[(size_t)s.row].B)) return false;
    }
    for (const Cut& k : cuts) if (!rel_ok(k.rel, 0.0 + x[(size_t)k.var], k.bound)) return false;
    for (double v : x) if (v < -EPS) return false;
    return true;
}

// The tableau of `p` exactly as PrimalSimplex.Solve / DualSimplex.Solve would prepare it; false where the reference throws
// (BranchAndBound catches that, :150-154).
static bool build_tableau(const LPProblem& p, bool dual, bool repaired, std::vector<double>& T, int& R, int& C, std::vector<int32_t>& basis)
{
    std::vector<std::string> names;
    try {
        if (dual) { BuildTableauPrimal(PrepareForTableauDual(p, repaired), T, R, C, basis, names); return true; }
        LPProblem model = p.Clone();
        if (model.ObjectiveSense == Sense::Min) for (double& v : model.C) v = -v;
        for (const Constraint& k : model.Constraints) if (k.B < -1e-9) return false;      // "negative RHS" exception, PrimalSimplex.cs:73-76
        BuildTableauPrimal(ExpandEqualitiesToInequalities(model), T, R, C, basis, names);
        return true;
    } catch (const LpxException&) { return false; }
}

// Device assembly: the root part of every node tableau is identical, so it is prepared and uploaded
// once per path (primal: ExpandEqualities + BuildTableau; dual: PrepareForTableau + BuildTableau) and a
// node only ships its branching rows.  Returns false when the root part itself throws in the reference
// (then every node of that path throws the same way).
bool ensure_template(Ctx& c, bool dual)
{
    const int w = dual ? 1 : 0;
    if (c.root_tpl[w] || c.tpl_bad[w]) return !c.tpl_bad[w];
    std::vector<double> T; int R, C; std::vector<int32_t> basis;
    if (!build_tableau(*c.root, dual, c.opt.bnb_mode == 1, T, R, C, basis)) { c.tpl_bad[w] = true; return false; }
    c.root_tpl[w] = acquire_exact_handle(R, C);
    c.tplR[w] = R; c.tplC[w] = C;
    int rc = lpx_tableau_upload(c.root_tpl[w], T.data(), basis.data());
    if (rc) throw LpxException(rc, "liblpx: " + last_error());
    return true;
}

// branching rows exactly as PrimalSimplex.Solve / PrepareForTableau would leave them
static void prepare_device(Ctx& c, const std::vector<Cut>& cuts, NodeLP& lp)
{
    lp.dual = has_ge_or_eq(*c.root);
    for (const Cut& k : cuts) if (k.rel != Rel::LE) lp.dual = true;
    if (!ensure_template(c, lp.dual)) { lp.error = true; return; }
    const int w = lp.dual ? 1 : 0;
    const bool fix_d1 = c.opt.bnb_mode == 1;
    for (const Cut& k : cuts) {
        double a = 1.0, z = 0.0, B = k.bound;
        if (!lp.dual) {
            if (B < -1e-9) { lp.error = true; return; }              // "negative RHS" exception, PrimalSimplex.cs:73-76
        } else {
            if (k.rel == Rel::GE) { a *= -1; z *= -1; B *= -1; }      // DualSimplex.cs:141-147
            if (!fix_d1 && B < -1e-9) { a *= -1; z *= -1; B *= -1; }  // :148-153 (defect D1)
        }
        lp.cvar.push_back(k.var); lp.ccoef.push_back(a); lp.czero.push_back(z); lp.crhs.push_back(B);
    }
    lp.R = c.tplR[w] + (int)cuts.size(); lp.C = c.tplC[w] + (int)cuts.size();
    lp.on_device = true;
}

void cold_node(Ctx& c, const std::vector<Cut>& cuts, NodeLP& lp)
{
    if (!c.opt.test_node_lp) return prepare_device(c, cuts, lp);
    const LPProblem p = make_node(*c.root, cuts);                  // test seam: the whole tableau is prepared on the host
    lp.dual = has_ge_or_eq(p);
    lp.error = !build_tableau(p, lp.dual, c.opt.bnb_mode == 1, lp.T, lp.R, lp.C, lp.basis);
}

// a handle for a node `d` levels below the root template `w`.  Capacity classes of 32 levels: one set of handles (and captured
// graphs) serves 32 depths
static lpx_tableau* handle_for_depth(Ctx& c, int w, int d)
{
    const int s = (d + 31) / 32 * 32, slack = s > 0 ? s : 32;
    return c.pool.get(c.tplR[w] + slack, c.tplC[w] + slack);
}

// a node whose tableau was prepared on the host (the test seam's nodes): an exact-size handle and one copy
static void upload(Ctx& c, NodeLP& lp)
{
    lp.h = c.pool.get(lp.R, lp.C);
    int rc = lpx_tableau_upload(lp.h, lp.T.data(), lp.basis.data());
    if (rc) throw LpxException(rc, "liblpx: " + last_error());
    std::vector<double>().swap(lp.T);
}

// Results of a whole batch: one launch + one wait reads every node's solution, the final tableaux that stay as
// parents are parked with all their copies in flight together (a per-node form waits twice per node).
static void collect_group(Ctx& c, std::vector<NodeLP*>& live, const std::vector<int>& st, const std::vector<lpx_stats>& ss, int nvars)
{
    std::vector<NodeLP*> want; std::vector<lpx_tableau*> hs; int maxm = 1;
    for (size_t i = 0; i < live.size(); ++i) {
        NodeLP& lp = *live[i];
        lp.pivots = ss[i].pivots;
        if (c.count_work) { c.out->Stats.pivots += ss[i].pivots; c.out->Stats.launches += ss[i].launches; c.out->Stats.loop_ms += ss[i].loop_ms; }
        if (st[i] < 0) throw LpxException(st[i], "liblpx: " + last_error());
        lp.status = st[i];
        if (st[i] == LPX_ITER_LIMIT) lp.error = true;                    // exception in the reference
        else if (lp.dual && c.opt.bnb_mode == 0) lp.has_solution = false;   // defect D2
        else { want.push_back(&lp); hs.push_back(lp.h); maxm = std::max(maxm, lp.R - 1); }
    }
    if (!want.empty()) {
        std::vector<double> xs((size_t)nvars * want.size()), zs(want.size());
        std::vector<int32_t> bs((size_t)maxm * want.size());
        double t0 = PhaseTimer::now();
        int rc = lpx_multi_solution(hs.data(), (int)hs.size(), nvars, xs.data(), zs.data(), bs.data(), maxm);
        g_pt.readback += PhaseTimer::now() - t0;
        if (rc) throw LpxException(rc, "liblpx: " + last_error());
        std::vector<lpx_store*> stores; std::vector<lpx_tableau*> keep_h; std::vector<NodeLP*> keep_lp;
        for (size_t i = 0; i < want.size(); ++i) {
            NodeLP& lp = *want[i];
            lp.x.assign(xs.begin() + (size_t)i * nvars, xs.begin() + (size_t)(i + 1) * nvars);
            lp.z = zs[i];
            lp.basis_out.assign(std::max(lp.R - 1, 1), 0);
            if (lp.keep && lp.R > 1) std::copy(bs.begin() + (size_t)i * maxm, bs.begin() + (size_t)i * maxm + (lp.R - 1), lp.basis_out.begin());
            lp.has_solution = true;
            if (lp.keep && lp.status == LPX_OPTIMAL) { stores.push_back(c.store_for(lp.h)); keep_h.push_back(lp.h); keep_lp.push_back(&lp); }
        }
        if (!keep_h.empty()) {                                           // park the final tableaux for the children
            std::vector<int> slots(keep_h.size(), -1);
            t0 = PhaseTimer::now();
            rc = lpx_store_save_multi(stores.data(), keep_h.data(), (int)keep_h.size(), slots.data());
            g_pt.parking += PhaseTimer::now() - t0;
            if (rc) throw LpxException(rc, "liblpx: " + last_error());
            for (size_t i = 0; i < keep_lp.size(); ++i) { keep_lp[i]->kstore = stores[i]; keep_lp[i]->kslot = slots[i]; }
        }
    }
    for (NodeLP* lp : live) { c.pool.put(lp->h); lp->h = nullptr; }
}

void solve_group(Ctx& c, std::vector<NodeLP*>& group, int nvars)
{
    lpx_run_opts po, dopt; lpx_default_opts(&po, 0); lpx_default_opts(&dopt, 1);
    po.max_iter = dopt.max_iter = c.opt.max_iter; po.batch = dopt.batch = c.opt.batch;
    if (c.opt.bnb_mode == 1) { dopt.fdf_guard = c.opt.max_iter; dopt.cleanup = 1; }
    if (c.opt.test_fail_after_nodes > 0 && c.budget_used >= c.opt.test_fail_after_nodes && !group.empty())
        throw LpxException(LPX_ENOMEM, "test seam: injected failure of a node group");       // include/lpx_test.h
    bool any_warm = false; for (NodeLP* lp : group) if (lp->warm) any_warm = true;
    bool rolling = false;
    if (any_warm) {                                               // dual feasible start: only the dual loop (and its clean-up) runs
        dopt.fdf_guard = 0; dopt.cleanup = 1;
        // A warm-started node needs a few dozen pivots.  Until r03 the big ones (config 4: 8 MB) streamed 64 at a time through the
        // one-launch-per-step kernel (15.8 MB of HBM traffic per node and pivot), because only four fitted the chip.  Twelve fit now
        // (rows in registers + LDS), a whole group goes out as one launch and the hardware starts the next node as one leaves: the
        // resident loop takes 0.45 ms per node whatever the HBM does -- 11.8 k against 8.2 k nodes/s on the same box, node logs
        // and node objective values bitwise the same.  Streaming rolling batches remain for nodes wider than the register
        // kernel's 1536 columns (and behind LPX_WARM_RESIDENT=0).
        size_t node_bytes = 0; int node_cols = 0;
        for (NodeLP* lp : group) { node_bytes = std::max(node_bytes, sizeof(double) * (size_t)lp->R * (size_t)lp->C); node_cols = std::max(node_cols, lp->C); }
        const bool warm_stream = [] { const char* e = std::getenv("LPX_WARM_RESIDENT"); return e && e[0] == '0'; }();   // read per solve (bench.py times both forms in one process)
        if ((warm_stream || node_cols > 1536) && node_bytes > ((size_t)1 << 20)) {
            dopt.resident = -1; po.resident = -1; rolling = group.size() > 1;
            static const int roll_batch = [] { const char* e = std::getenv("LPX_ROLL_BATCH"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 16; }();   // pivots between polls
            if (rolling && c.opt.batch <= 0) dopt.batch = po.batch = roll_batch;
        }
    }
    if (c.opt.test_node_lp) {          // test seam (include/lpx.h): the device loop is stood in for
        for (NodeLP* lp : group) {
            if (c.count_work) c.out->LpSolves++;
            if (lp->error || lp->R < 2) { lp->error = true; continue; }
            lp->x.assign(nvars, 0.0);
            int64_t piv = 0;
            int st = c.opt.test_node_lp(lp->T.data(), lp->R, lp->C, lp->basis.data(), lp->dual ? 1 : 0, c.opt.bnb_mode,
                                        c.opt.max_iter, nvars, lp->x.data(), &lp->z, &piv);
            c.out->Stats.pivots += piv; lp->pivots = piv; lp->status = st;
            if (st < 0) throw LpxException(st, "test seam: node LP failed");          // as collect_group does for lpx_multi_run
            if (st == LPX_ITER_LIMIT) lp->error = true;
            else lp->has_solution = !(lp->dual && c.opt.bnb_mode == 0);
        }
        return;
    }
    const size_t width = (size_t)std::max(1, c.opt.concurrent_nodes);
    // gives every node of `nodes` a handle and builds its tableau on the device (one launch per kind); appends the admitted ones to `live`
    auto admit = [&](const std::vector<NodeLP*>& nodes, std::vector<NodeLP*>& live) {
        const double t0 = PhaseTimer::now();
        std::vector<NodeLP*> assemble[2];                     // cold nodes built on the device, per root template: ONE launch each
        std::vector<NodeLP*> warm_kids;                       // warm-started children, built from their parked parents: ONE launch
        for (NodeLP* lp : nodes) {
            if (lp->error || lp->R < 2) { if (lp->R < 2) lp->error = true; continue; }
            if (lp->warm) { lp->h = handle_for_depth(c, lp->wslot, lp->depth); warm_kids.push_back(lp); }
            else if (lp->on_device) { const int w = lp->dual ? 1 : 0; lp->h = handle_for_depth(c, w, (int)lp->cvar.size()); assemble[w].push_back(lp); }
            else upload(c, *lp);
            live.push_back(lp);
        }
        for (int w = 0; w < 2; ++w) {
            if (assemble[w].empty()) continue;
            std::vector<lpx_tableau*> nh; std::vector<int32_t> off{0}, var; std::vector<double> coef, zero, rhs;
            for (NodeLP* lp : assemble[w]) {
                nh.push_back(lp->h);
                var.insert(var.end(), lp->cvar.begin(), lp->cvar.end()); coef.insert(coef.end(), lp->ccoef.begin(), lp->ccoef.end());
                zero.insert(zero.end(), lp->czero.begin(), lp->czero.end()); rhs.insert(rhs.end(), lp->crhs.begin(), lp->crhs.end());
                off.push_back((int32_t)var.size());
            }
            int rc = lpx_tableau_build_nodes(nh.data(), c.root_tpl[w], (int)nh.size(), off.data(), var.data(), coef.data(), zero.data(), rhs.data());
            if (rc) throw LpxException(rc, "liblpx: " + last_error());
        }
        if (!warm_kids.empty()) {
            std::vector<lpx_tableau*> ch; std::vector<lpx_store*> st; std::vector<int> slots; std::vector<int32_t> var, row, ge; std::vector<double> bd;
            for (NodeLP* lp : warm_kids) {
                ch.push_back(lp->h); st.push_back(lp->pstore); slots.push_back(lp->pslot);
                var.push_back(lp->cvar.back()); row.push_back(lp->prow); ge.push_back(lp->wis_ge ? 1 : 0); bd.push_back(lp->wbound);
            }
            int rc = lpx_tableau_build_children_from_store(ch.data(), st.data(), slots.data(), (int)ch.size(), var.data(), row.data(), ge.data(), bd.data());
            if (rc) throw LpxException(rc, "liblpx: " + last_error());
        }
        g_pt.build += PhaseTimer::now() - t0;
    };

    // ---- the batch loop, once.  A batch is what is on the device together; the three drivers below differ only in the call that
    //      runs it: refill() tops it up to `width` from the group, retire() reads its finished nodes back and keeps the others.
    struct Batch { std::vector<NodeLP*> inflight; std::vector<lpx_tableau*> hs; std::vector<int> dual; bool running = false; };
    size_t next = 0;                                              // group[next..) has not been admitted yet
    auto refill = [&](Batch& B) {                                 // false: nothing is in flight
        std::vector<NodeLP*> fresh;
        while (next < group.size() && B.inflight.size() + fresh.size() < width) fresh.push_back(group[next++]);
        if (c.count_work) c.out->LpSolves += (int64_t)fresh.size();       // every node reaches _solver.Solve (:148), even if it throws
        admit(fresh, B.inflight);
        B.hs.clear(); B.dual.clear();
        for (NodeLP* lp : B.inflight) { B.hs.push_back(lp->h); B.dual.push_back(lp->dual ? 1 : 0); }
        return !B.inflight.empty();
    };
    // test_feas: also the feasibility test of :175-179 for the finished nodes, here where another batch's window hides it
    auto retire = [&](Batch& B, const std::vector<int>& st, const std::vector<lpx_stats>& ss, bool test_feas) {
        std::vector<NodeLP*> fin, keep; std::vector<int> fst; std::vector<lpx_stats> fss;
        for (size_t i = 0; i < B.inflight.size(); ++i) {
            if (st[i] == LPX_RUNNING) keep.push_back(B.inflight[i]);
            else { fin.push_back(B.inflight[i]); fst.push_back(st[i]); fss.push_back(ss[i]); }
        }
        const double t0 = PhaseTimer::now();
        collect_group(c, fin, fst, fss, nvars);                  // pivots are cumulative per node: counted once, when it finishes
        if (test_feas && (c.feas.built || !fin.empty())) {
            if (!c.feas.built) c.feas.build(*c.root);
            for (NodeLP* lp : fin)
                if (lp->cuts_for_feas && !lp->error && lp->has_solution && !(c.opt.bnb_mode == 1 && lp->status == LPX_INFEASIBLE))
                    lp->feas = IsFeasibleIndexed(lp->x, *c.root, *lp->cuts_for_feas, c.feas) ? 1 : 0;
        }
        g_pt.collect += PhaseTimer::now() - t0;
        B.inflight.swap(keep);
    };

    Batch one;                                                    // the synchronous drivers' batch
    if (rolling) {
        // ROLLING batches (warm-started children on the streaming kernels): most of them need a few dozen pivots, a few need hundreds.
        // NS (two) batches of `width` nodes alternate (lpx_multi_run_begin / _end): while one pivots through a window of `roll_batch`
        // steps, the host reads the other one's finished nodes back, parks their tableaux, tests their solutions and assembles fresh
        // children in their places -- so the device never waits for the host and finished nodes leave the grid after every window.
        static const bool pipelined = [] { const char* e = std::getenv("LPX_ROLL_PIPELINE"); return !(e && e[0] == '0'); }();   // diagnostic: 0 = one batch, synchronous
        const int steps = dopt.batch > 0 ? dopt.batch : 16;
        static const int NS = [] { const char* e = std::getenv("LPX_ROLL_SETS"); const int v = e ? std::atoi(e) : 0; return v >= 2 && v <= LPX_ASYNC_SLOTS ? v : 2; }();
        Batch sets[LPX_ASYNC_SLOTS];
        auto others_running = [&](int s) { for (int k = 0; k < NS; ++k) if (k != s && sets[k].running) return true; return false; };
        bool async_ok = pipelined;
        auto launch = [&](int s) {
            Batch& S = sets[s];
            if (!refill(S)) return;
            const int rc = lpx_multi_run_begin(s, S.hs.data(), S.dual.data(), (int)S.hs.size(), &po, &dopt, steps);
            if (rc < 0) throw LpxException(rc, "liblpx: " + last_error());
            if (rc == 1) { async_ok = false; return; }               // not available: the synchronous loop below takes what is in the sets
            if (g_pt.on && g_pt.drained_at > 0 && !others_running(s)) {
                const double d = PhaseTimer::now() - g_pt.drained_at;
                g_pt.drained += d; g_pt.drains++; g_pt.drained_max = std::max(g_pt.drained_max, d);
            }
            S.running = true;
        };
        auto land = [&](int s) {
            Batch& S = sets[s];
            std::vector<int> st(S.inflight.size()); std::vector<lpx_stats> ss(S.inflight.size());
            const double t0 = PhaseTimer::now();
            const int rc = lpx_multi_run_end(s, st.data(), ss.data());
            g_pt.run += PhaseTimer::now() - t0;
            S.running = false;
            if (g_pt.on && !others_running(s)) g_pt.drained_at = PhaseTimer::now();
            if (rc) throw LpxException(rc, "liblpx: " + last_error());
            retire(S, st, ss, true);
        };
        if (async_ok) {
            try {
                for (int s = 0; s < NS && async_ok; ++s) launch(s);
                while (async_ok && others_running(-1))
                    for (int s = 0; s < NS && async_ok; ++s) {
                        if (!sets[s].running) continue;
                        land(s);
                        launch(s);
                    }
            } catch (...) {
                // a window may still be in flight in another slot: wait for it before the handles go back to the pool
                for (int s = 0; s < NS; ++s) if (sets[s].running) { std::vector<int> st(sets[s].inflight.size()); lpx_multi_run_end(s, st.data(), nullptr); sets[s].running = false; }
                throw;
            }
            if (async_ok) return;
            for (int s = 0; s < NS; ++s) if (sets[s].running) land(s);
        }
        // the slots were not available: the synchronous loop takes over what EVERY set still holds
        for (int s = 0; s < NS; ++s) { one.inflight.insert(one.inflight.end(), sets[s].inflight.begin(), sets[s].inflight.end()); sets[s].inflight.clear(); }
    }
    // synchronous drivers: one batch.  Rolling: it is polled after a window and refilled as nodes finish; otherwise: the plain
    // chunks of `width` nodes, each run to the end.
    while (next < group.size() || !one.inflight.empty()) {
        if (!refill(one)) continue;
        std::vector<int> st(one.hs.size()); std::vector<lpx_stats> ss(one.hs.size());
        const double t0 = PhaseTimer::now();
        int rc;
        if (rolling) {
            static const int roll_div = [] { const char* e = std::getenv("LPX_ROLL_DIV"); const int v = e ? std::atoi(e) : 0; return v > 0 ? v : 2; }();   // diagnostic
            const int min_active = next < group.size() ? (int)std::max<size_t>(1, width / roll_div) : 0;
            rc = lpx_multi_run_some(one.hs.data(), one.dual.data(), (int)one.hs.size(), &po, &dopt, st.data(), ss.data(), min_active);
        } else rc = lpx_multi_run(one.hs.data(), one.dual.data(), (int)one.hs.size(), &po, &dopt, st.data(), ss.data());
        g_pt.run += PhaseTimer::now() - t0;
        if (rc) throw LpxException(rc, "liblpx: " + last_error());
        retire(one, st, ss, false);
    }
}

}}}  // namespace lpx::host::bnb
