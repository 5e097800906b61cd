// host/bnb_bounded.cpp -- branch and bound by bound changes (include/lpx.h): three drivers around one frame.
//   SolveBnbBounded   lpx_solve_bnb_bounded / _bounded2 / _bounded3: the root is SolveBounded keeping its handle, and every node after
//                     it is ONE lpx_bounded_node (flagged search: lpx_bounded_node2 / _node3) call on that handle
//   SolveBnbBoundedDual  lpx_solve_bnb_bounded_dual: the same search (SearchFromRoot) behind the root of SolveBoundedDual, for >= rows
//                     and right-hand sides of either sign
//   SolveBnbDivers    lpx_solve_bnb_bounded4 / 6 / 7 / 10: W handles, a round is ONE lpx_node_batch_run (_run_probe, _run2, _run3)
//   SolveBnbPlunge    lpx_solve_bnb_bounded5: the same rounds with ONE lpx_node_batch_plunge, chains of up to D nodes
// A node is its path of (var, lower, upper) overrides and what a call sends are the columns whose bounds differ from the bounds now
// on the device, in ascending order: no tableau is copied, parked or reshaped, and the node store is a few bytes per node.  Search
// order and pruning are those of Models/Branch&Bound.cs (depth first, ceil child first :253-257, prune at z <= best + EPS :182,
// branch on the fraction closest to 0.5 :197-213).  Its IsFeasible re-check of an incumbent is not mirrored: the dual loop ends
// primal feasible by construction.
// The frame stands once, in the anonymous namespace: the checks, the root step, the pool of handles, the steal step, the bounds
// diff of a popped node, the node log, the incumbent and the result tail.  The three search loops stay three functions: their
// decide steps differ, and the order of their steps is part of the contract (the log is a function of the model, the options, the
// flags, W and D alone).  No helper allocates per round: the scratch vectors are the callers'.
#include "model.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace lpx { namespace host {

namespace {

constexpr double EPS = 1e-6;      // Models/Branch&Bound.cs:24

struct Override { int var; double lo, ub; };
struct Node { int depth; std::vector<Override> path; };

// The checks every driver makes, in this order; a driver adds its own in front of or behind them where the ABI tests pin them.
void ValidateBnbBounded(int n, const std::vector<double>& lower, const std::vector<double>& upper, const std::vector<uint8_t>& is_int,
                        int64_t max_nodes, int search_flags)
{
    if ((!lower.empty() && (int)lower.size() != n) || (!upper.empty() && (int)upper.size() != n))
        throw LpxException(LPX_EINVAL, "Bounded Primal Simplex: lower / upper need one entry per variable");
    if (!is_int.empty() && (int)is_int.size() != n)
        throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: the integer mask needs one entry per variable");
    for (int j = 0; j < n; ++j)         // the checks of SolveBounded, with its messages, in front of the integer ones
        CheckVarBounds("x" + std::to_string(j + 1), lower.empty() ? 0.0 : lower[j], upper.empty() ? 1.0 / 0.0 : upper[j]);
    for (int j = 0; j < n; ++j) {
        if (!is_int.empty() && !is_int[j]) continue;
        const double l = lower.empty() ? 0.0 : lower[j], u = upper.empty() ? 1.0 / 0.0 : upper[j];
        if (!std::isfinite(u) || std::floor(l) != l || std::floor(u) != u)
            throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: integer variable x" + std::to_string(j + 1) +
                                           " needs finite, integral lower and upper bounds");
    }
    if (max_nodes < 0) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: max_nodes is negative");
    if (search_flags & ~(LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF))
        throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: search_flags holds a bit other than LPX_BDUAL_LONG_STEP and LPX_BDUAL_CUTOFF");
}

SimplexResult FinishBnbResult(SimplexResult res, const BnbBoundedInfo& info, const BoundedSession& ses, int n, double best,
                              std::vector<double>& best_x);

// The root: SolveBounded keeping its handle, the records reset, and -- where every node is on chip -- the fit of the root's shape,
// which never changes and so decides for every node.  False: the root ends the search (an unbounded root is reported as that).
bool SolveRoot(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper, const EngineOptions& opt,
               bool onchip, BoundedSession& ses, BoundedInfo& binfo, SimplexResult& res, BnbBoundedInfo& info,
               BnbDiversInfo* dinfo = nullptr, BnbPlungeInfo* pinfo = nullptr, int root_form = -1, int max_spare = 0,
               bool dual_root = false, int search_flags = 0)   // dual_root: the root is the dual start (>= rows, any RHS sign)
{
    EngineOptions ropt = opt; ropt.quiet = true;
    res = dual_root ? SolveBoundedDual(original, lower, upper, search_flags & LPX_BDUAL_LONG_STEP, ropt, nullptr, &binfo, &ses)
                    : SolveBounded(original, lower, upper, ropt, nullptr, &binfo, &ses, root_form, max_spare);
    info = BnbBoundedInfo();
    if (dinfo) *dinfo = BnbDiversInfo();
    if (pinfo) *pinfo = BnbPlungeInfo();
    info.constant = ses.constant;
    res.Nodes = 0; res.LpSolves = 1;
    res.Aux = {0.0, 0.0, 0.0, 0.0};
    if (dual_root && res.Status == LPX_INFEASIBLE) {    // the answer of a search that found no incumbent, without a node
        std::vector<double> none;
        res = FinishBnbResult(std::move(res), info, ses, original.NumVars(), -1.0 / 0.0, none);
        return false;
    }
    if (res.Status != LPX_OPTIMAL) return false;
    if (onchip) {
        int R = 0, C = 0;
        lpx_tableau_shape(ses.h, &R, &C, nullptr);
        if (!lpx_bounded_node_fits(R, C))
            throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: the root tableau (" + std::to_string(R) + " x " + std::to_string(C) +
                                           ") does not fit the on-chip form of the node (lpx_bounded_node_fits)");
    }
    return true;
}

// The result from `res.Nodes` to the report text
SimplexResult FinishBnbResult(SimplexResult res, const BnbBoundedInfo& info, const BoundedSession& ses, int n, double best,
                              std::vector<double>& best_x)
{
    res.Nodes = info.nodes; res.LpSolves = info.nodes + 1;
    res.Aux = {(double)info.nodes, (double)info.events, (double)info.flips, (double)info.incumbents};
    res.Trace.clear();
    if (best_x.empty()) {
        res.Status = LPX_INFEASIBLE; res.HasSolution = false; res.OptimalValue = 0.0;
        res.Solution.assign((size_t)n, 0.0);
        res.Summary = "INFEASIBLE\n"; res.Report = res.Summary;
        return res;
    }
    if (!ses.lower.empty()) for (int j = 0; j < n; ++j) best_x[j] = best_x[j] + ses.lower[j];
    double value = ses.min ? -best : best;
    if (ses.shifted) value = value + ses.constant;
    res.Status = LPX_OPTIMAL; res.HasSolution = true; res.OptimalValue = value; res.Solution = best_x;
    std::string report;
    FinalizeText(report, res.Summary, best_x, value, LPX_OPTIMAL);
    const std::string tail = "  nodes: " + std::to_string(info.nodes) + ", dual events: " + std::to_string(info.events) +
                             ", dual-feasibility flips: " + std::to_string(info.flips) + "\n";
    res.Report = report + tail; res.Summary += tail.substr(2);
    return res;
}

// The handles of the divers: diver 0 is the root's handle, the others are copies of it.  The pool hands the copies and the batch
// back on every way out.
struct Pool {
    std::vector<lpx_tableau*> h; lpx_node_batch* batch = nullptr;
    void open(lpx_tableau* root, int W)
    {
        h.push_back(root);
        for (int d = 1; d < W; ++d) {
            lpx_tableau* c = nullptr;
            const int rc = lpx_tableau_clone(root, &c);
            if (rc) throw_lib(rc);
            h.push_back(c);
        }
        const int rc = lpx_node_batch_create(W, h.data(), &batch);
        if (rc) throw_lib(rc);
    }
    ~Pool() { lpx_node_batch_destroy(batch); for (size_t d = 1; d < h.size(); ++d) lpx_tableau_destroy(h[d]); }
};

// A diver: the bounds now on its handle (cur), those of the node it holds (nb), its own depth-first stack
struct Diver { std::vector<double> cur_lo, cur_ub, nb_lo, nb_ub; std::vector<Node> stack; Node node; };

bool AnyOpen(const std::vector<Diver>& dv) { for (const Diver& d : dv) if (!d.stack.empty()) return true; return false; }

// The steal step: every idle diver takes the oldest entry of the longest stack, lengths as they stand now
void StealForIdle(std::vector<Diver>& dv, BnbDiversInfo& dinfo)
{
    const int W = (int)dv.size();
    for (int d = 0; d < W; ++d) {
        if (!dv[d].stack.empty()) continue;
        int v = 0;
        for (int k = 1; k < W; ++k) if (dv[k].stack.size() > dv[v].stack.size()) v = k;
        if (dv[v].stack.size() < 2) continue;
        dv[d].stack.push_back(std::move(dv[v].stack.front()));
        dv[v].stack.erase(dv[v].stack.begin());
        dinfo.steals++;
    }
}

// The bounds of a node from its path (nb), and the columns in which they differ from the bounds now on the handle (cur) appended to
// cols / clo / cub in ascending order; the return value is their count K
int DiffBounds(const Node& node, const std::vector<double>& root_lo, const std::vector<double>& root_ub, const std::vector<double>& cur_lo,
               const std::vector<double>& cur_ub, std::vector<double>& nb_lo, std::vector<double>& nb_ub, std::vector<int32_t>& cols,
               std::vector<double>& clo, std::vector<double>& cub)
{
    nb_lo = root_lo; nb_ub = root_ub;
    for (const Override& v : node.path) { nb_lo[v.var] = v.lo; nb_ub[v.var] = v.ub; }
    int K = 0;
    for (int j = 0; j < (int)nb_lo.size(); ++j)
        if (nb_lo[j] != cur_lo[j] || nb_ub[j] != cur_ub[j]) { cols.push_back(j); clo.push_back(nb_lo[j]); cub.push_back(nb_ub[j]); ++K; }
    return K;
}

bool NodeLimitReached(int64_t max_nodes, BnbBoundedInfo& info)
{
    if (!(max_nodes > 0 && info.nodes >= max_nodes)) return false;
    info.limit_rc = LPX_ITER_LIMIT;
    info.limit_msg = "Bounded Branch and Bound: node limit of " + std::to_string(max_nodes) + " reached";
    return true;
}

// A node's record into the counts and the log; true: it reached the iteration limit, which ends the search
bool LogNode(BnbBoundedInfo& info, int64_t index, int depth, int K, const lpx_node_record& rec, int max_iter)
{
    info.events += rec.events; info.flips += rec.flips;
    if (K > info.max_K) info.max_K = K;
    lpx_bnb_node_log lg;
    lg.depth = depth; lg.K = K; lg.status = rec.status; lg.events = rec.events; lg.flips = (int32_t)rec.flips;
    lg.var = rec.pick.var; lg.z = rec.pick.z;
    info.log.push_back(lg);
    if (rec.status != LPX_ITER_LIMIT) return false;
    info.limit_rc = LPX_ITER_LIMIT;
    info.limit_msg = "Bounded Branch and Bound: node " + std::to_string(index) + " (depth " + std::to_string(depth) +
                     ") reached the iteration limit of " + std::to_string(max_iter) + " events";
    return true;
}

// The incumbent step (:189-195): the solution the handle holds, its integer columns to the nearest integer
void TakeIncumbent(lpx_tableau* h, int n, const std::vector<uint8_t>& is_int, double z, double& best, std::vector<double>& best_x,
                   BnbBoundedInfo& info)
{
    std::vector<double> x((size_t)n, 0.0);
    const int rs = lpx_tableau_bounded_solution(h, n, x.data(), nullptr, nullptr);
    if (rs) throw_lib(rs);
    for (int j = 0; j < n; ++j) if (is_int.empty() || is_int[j]) x[j] = std::nearbyint(x[j]);
    best = z; best_x = std::move(x);
    info.incumbents++;
}

// The search of SolveBnbBounded and SolveBnbBoundedDual from a solved root on: one node call per popped node on the root's handle
SimplexResult SearchFromRoot(SimplexResult res, BoundedSession& ses, const BoundedInfo& binfo, int n, const std::vector<uint8_t>& is_int,
                             const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info, int search_flags, int node_form)
{
    // the handle's columns stand for x' = x - lower: root bounds [0, ub'] of every variable
    std::vector<double> root_lo((size_t)n, 0.0), root_ub(binfo.ub.begin(), binfo.ub.begin() + n);
    std::vector<double> cur_lo = root_lo, cur_ub = root_ub, nb_lo, nb_ub;
    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.max_iter = opt.max_iter;
    o.batch = opt.batch > 0 ? opt.batch : 16;             // a node takes a handful of events: short batches, same bits
    const uint8_t* mask = is_int.empty() ? nullptr : is_int.data();

    double best = -1.0 / 0.0;
    std::vector<double> best_x;
    std::vector<Node> stack;
    stack.push_back(Node{0, {}});
    std::vector<int32_t> cols; std::vector<double> clo, cub;
    while (!stack.empty()) {
        if (NodeLimitReached(max_nodes, info)) break;
        Node node = std::move(stack.back());
        stack.pop_back();
        const int64_t index = info.nodes++;
        cols.clear(); clo.clear(); cub.clear();
        const int K = DiffBounds(node, root_lo, root_ub, cur_lo, cur_ub, nb_lo, nb_ub, cols, clo, cub);
        lpx_node_record rec;
        // with CUTOFF the loop stops where this node would be pruned by bound anyway; search_flags = 0 stays the old call, messages included
        const double cutoff = (search_flags & LPX_BDUAL_CUTOFF) ? best + EPS : 0.0;
        const int rc = node_form > LPX_NODE_LAUNCHES      // LPX_NODE_LAUNCHES (and -1) stay the old calls, messages included
            ? lpx_bounded_node3(ses.h, K, cols.data(), clo.data(), cub.data(), &o, LPX_BDUAL_SKIP_FIXED | search_flags, cutoff,
                                n, mask, EPS, node_form, &rec)
            : search_flags == 0
            ? lpx_bounded_node(ses.h, K, cols.data(), clo.data(), cub.data(), &o, n, mask, EPS, &rec)
            : lpx_bounded_node2(ses.h, K, cols.data(), clo.data(), cub.data(), &o, LPX_BDUAL_SKIP_FIXED | search_flags, cutoff,
                                n, mask, EPS, &rec);
        if (rc < 0) throw_lib(rc);
        cur_lo = nb_lo; cur_ub = nb_ub;
        if (LogNode(info, index, node.depth, K, rec, o.max_iter)) break;
        if (rec.status == LPX_INFEASIBLE) { info.pruned_infeasible++; continue; }
        const double z = rec.pick.z;
        if (rec.status == LPX_CUTOFF || z <= best + EPS) { info.pruned_bound++; continue; }     // :182
        if (rec.pick.var < 0) { TakeIncumbent(ses.h, n, is_int, z, best, best_x, info); continue; }      // :189-195
        const int v = rec.pick.var;
        Node fl{node.depth + 1, node.path}, ce{node.depth + 1, node.path};
        fl.path.push_back(Override{v, nb_lo[v], std::floor(rec.pick.x_var)});
        ce.path.push_back(Override{v, std::ceil(rec.pick.x_var), nb_ub[v]});
        stack.push_back(std::move(fl));
        stack.push_back(std::move(ce));                                             // explored first (:256)
    }

    return FinishBnbResult(std::move(res), info, ses, n, best, best_x);
}

}  // namespace

SimplexResult SolveBnbBounded(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                              const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                              int search_flags, int node_form)
{
    const int n = original.NumVars();
    ValidateBnbBounded(n, lower, upper, is_int, max_nodes, search_flags);
    if (node_form != -1 && node_form != LPX_NODE_LAUNCHES && node_form != LPX_NODE_ONCHIP && node_form != LPX_NODE_AUTO)
        throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: node_form is none of LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP and LPX_NODE_AUTO");

    BoundedSession ses;
    BoundedInfo binfo;
    SimplexResult res;
    if (!SolveRoot(original, lower, upper, opt, node_form == LPX_NODE_ONCHIP, ses, binfo, res, info)) return res;
    return SearchFromRoot(std::move(res), ses, binfo, n, is_int, opt, max_nodes, info, search_flags, node_form);
}

// lpx_solve_bnb_bounded_dual: SolveBnbBounded whose root is the dual start of SolveBoundedDual, so >= rows, an = row as its pair and
// right-hand sides of either sign are accepted.  A root that ends LPX_INFEASIBLE ends the search with the result of a search that
// found no incumbent (Nodes = 0, LpSolves = 1).  From a solved root on it is SearchFromRoot unchanged.
SimplexResult SolveBnbBoundedDual(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                                  const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                                  int search_flags, int node_form)
{
    const int n = original.NumVars();
    ValidateBnbBounded(n, lower, upper, is_int, max_nodes, search_flags);
    if (node_form != LPX_NODE_LAUNCHES && node_form != LPX_NODE_ONCHIP && node_form != LPX_NODE_AUTO)
        throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: node_form is none of LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP and LPX_NODE_AUTO");

    BoundedSession ses;
    BoundedInfo binfo;
    SimplexResult res;
    if (!SolveRoot(original, lower, upper, opt, node_form == LPX_NODE_ONCHIP, ses, binfo, res, info, nullptr, nullptr, -1, 0, true, search_flags))
        return res;
    return SearchFromRoot(std::move(res), ses, binfo, n, is_int, opt, max_nodes, info, search_flags, node_form);
}

// The search by W divers (lpx_solve_bnb_bounded4, include/lpx.h): W handles in the state of the solved root, each with its own
// current bounds and its own depth-first stack; a round steals for the idle divers, pops one node per diver, evaluates them all
// in ONE lpx_node_batch_run and decides the records in diver order.  Everything around the search is SolveBnbBounded's.  The
// order of the steps is part of the contract: the log is a function of the model, the options, the flags and W alone.
// With `strong` it is the search of lpx_solve_bnb_bounded6(LPX_BRANCH_STRONG): the same rounds with probes behind the nodes.
SimplexResult SolveBnbDivers(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                             const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                             int search_flags, int divers, BnbDiversInfo& dinfo, const BnbStrong* strong, BnbStrongInfo* sinfo,
                             int stall_events, BnbGuardInfo* ginfo, int root_form, const lpx_cut_opts* root_cuts, BnbCutInfo* cinfo,
                             int tighten, BnbFixInfo* finfo)
{
    // tighten = 1 (lpx_solve_bnb_bounded10): the evaluate step is ONE lpx_node_batch_run3 whose entries carry fix_bound = best + EPS of
    // the start of the round (-inf without an incumbent); the decide step applies the reported triples to the bounds it holds for
    // the diver's handle -- the kernel has applied them to the handle already -- and hands them down both children's paths.  The
    // plunge, the probes and the sequential driver have no tightening.
    BnbFixInfo fdummy;
    BnbFixInfo& fi = finfo ? *finfo : fdummy;
    fi = BnbFixInfo();
    const bool tightening = tighten == 1 && stall_events >= 0 && !strong;
    std::vector<lpx_fix_list> fixes; std::vector<double> fix_bounds, fix_lower, fix_upper; std::vector<int32_t> fix_cols;
    // root_cuts != null (lpx_solve_bnb_bounded9): the root's handle gets spare capacity, lpx_bounded_cut_loop runs on it, and the
    // divers start from the handle the loop leaves; nothing else of the search changes (the cuts hold in the whole tree).
    BnbCutInfo cdummy;
    BnbCutInfo& ci = cinfo ? *cinfo : cdummy;
    ci = BnbCutInfo();
    // stall_events >= 0 (lpx_solve_bnb_bounded7): the evaluate step is ONE lpx_node_batch_run2, which with 0 is lpx_node_batch_run;
    // the guard records are counted and nothing else of the search reads them.
    BnbGuardInfo gdummy;
    BnbGuardInfo& gi = ginfo ? *ginfo : gdummy;
    gi = BnbGuardInfo();
    const bool guarded = stall_events >= 0 && !strong;
    std::vector<lpx_guard_record> guards;
    // strong != null (lpx_solve_bnb_bounded6 with LPX_BRANCH_STRONG): the evaluate step is ONE lpx_node_batch_run_probe and the
    // decide step takes the variable and drops the dead children by the probes; everything else is the search below, unchanged.
    BnbStrongInfo sdummy;
    BnbStrongInfo& si = sinfo ? *sinfo : sdummy;
    si = BnbStrongInfo();
    if (strong && (strong->cand_max < 1 || strong->cand_max > 32)) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: cand_max is outside [1, 32]");
    if (strong && strong->probe_iter < 0) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: probe_iter is negative");
    const int n = original.NumVars();
    ValidateBnbBounded(n, lower, upper, is_int, max_nodes, search_flags);
    if (divers < 1 || divers > 1024) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: divers is outside [1, 1024]");

    BoundedSession ses;
    BoundedInfo binfo;
    SimplexResult res;
    if (!SolveRoot(original, lower, upper, opt, true, ses, binfo, res, info, &dinfo, nullptr, root_form, root_cuts ? root_cuts->max_active : 0))
        return res;

    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.max_iter = opt.max_iter;
    const uint8_t* mask = is_int.empty() ? nullptr : is_int.data();
    double best = -1.0 / 0.0;
    std::vector<double> best_x;

    ci.spare = ses.spare;
    if (root_cuts && ses.spare > 0) {
        // the round's flags: the structural ones as given; the slack of prepared row i is integer iff its coefficients and its
        // shifted RHS are integral and every variable with a non-zero coefficient is integer (an = pair: two rows, judged alike)
        const int R = ses.R, C = ses.C, m = R - 1;
        std::vector<uint8_t> flags((size_t)(C - 1), 0);
        for (int j = 0; j < n; ++j) flags[j] = (is_int.empty() || is_int[j]) ? 1 : 0;
        for (int i = 0; i < m; ++i) {
            const double* row = ses.T0.data() + (size_t)i * C;
            bool whole = std::floor(row[C - 1]) == row[C - 1];
            for (int j = 0; j < n && whole; ++j) whole = std::floor(row[j]) == row[j] && (row[j] == 0.0 || flags[j]);
            flags[n + i] = whole ? 1 : 0;
        }
        lpx_cut_loop_record rec; std::memset(&rec, 0, sizeof(rec));
        ci.z_before.assign((size_t)std::max(root_cuts->max_rounds, 1), 0.0); ci.z_after = ci.z_before;
        rec.z_before = ci.z_before.data(); rec.z_after = ci.z_after.data();
        const int rc = lpx_bounded_cut_loop(ses.h, flags.data(), C - 1, C - 1, n, mask, root_cuts, &o, search_flags, LPX_NODE_AUTO, &rec);
        if (rc < 0) throw_lib(rc);
        ci.ran = 1; ci.rounds = rec.rounds; ci.added = rec.added; ci.purged = rec.purged; ci.stop = rec.stop; ci.status = rec.status;
        ci.R = rec.R; ci.C = rec.C; ci.events = rec.events;
        ci.z_before.resize((size_t)rec.rounds); ci.z_after.resize((size_t)rec.rounds);
        if (rec.stop == LPX_CUTLOOP_ITER_LIMIT) {
            info.limit_rc = LPX_ITER_LIMIT;
            info.limit_msg = "Bounded Branch and Bound: cut round " + std::to_string(rec.rounds) + " at the root reached the iteration limit of " +
                             std::to_string(o.max_iter) + " events";
        }
        // INFEASIBLE: a cut of the root LP's own rows leaves no point, so the integer program has none: no node is searched
        if (rec.stop == LPX_CUTLOOP_INFEASIBLE || rec.stop == LPX_CUTLOOP_ITER_LIMIT || rec.stop == LPX_CUTLOOP_STATUS)
            return FinishBnbResult(std::move(res), info, ses, n, best, best_x);
    } else if (root_cuts) {
        ci.z_before.clear(); ci.z_after.clear();
        lpx_tableau_shape(ses.h, &ci.R, &ci.C, nullptr);
    }

    const int W = divers;
    Pool pool;
    pool.open(ses.h, W);

    const std::vector<double> root_lo((size_t)n, 0.0), root_ub(binfo.ub.begin(), binfo.ub.begin() + n);
    std::vector<Diver> dv((size_t)W);
    for (Diver& d : dv) { d.cur_lo = root_lo; d.cur_ub = root_ub; }
    dv[0].stack.push_back(Node{0, {}});
    std::vector<int32_t> slot, Ks, cols, rcs((size_t)W); std::vector<double> clo, cub, cutoffs;
    std::vector<lpx_node_record> recs((size_t)W);
    std::vector<double> prunes; std::vector<lpx_probe_head> heads; std::vector<lpx_probe_record> probes;       // strong branching only
    // the gain of a probe against its node's z, and whether the child it stands for is dead against best as it stands
    auto gain = [](const lpx_probe_record& q, double z) {
        if (q.status == LPX_INFEASIBLE || q.status == LPX_CUTOFF) return 1e12;
        if (q.status < 0) return 1e-6;
        return std::min(std::max(z - q.z, 1e-6), 1e12);
    };
    auto dead = [](const lpx_probe_record& q, double best_now) {
        return q.status == LPX_INFEASIBLE || q.status == LPX_CUTOFF || (q.status == LPX_OPTIMAL && q.z <= best_now + EPS);
    };
    bool stop = false;
    while (!stop && AnyOpen(dv)) {
        // 1. limit, 2. steal
        if (NodeLimitReached(max_nodes, info)) break;
        StealForIdle(dv, dinfo);
        // 3. pop
        slot.clear(); Ks.clear(); cols.clear(); clo.clear(); cub.clear(); cutoffs.clear();
        for (int d = 0; d < W; ++d) {
            Diver& D = dv[d];
            if (D.stack.empty()) continue;
            if (max_nodes > 0 && info.nodes + (int64_t)slot.size() >= max_nodes) break;
            D.node = std::move(D.stack.back());
            D.stack.pop_back();
            const int K = DiffBounds(D.node, root_lo, root_ub, D.cur_lo, D.cur_ub, D.nb_lo, D.nb_ub, cols, clo, cub);
            slot.push_back(d); Ks.push_back(K);
            cutoffs.push_back((search_flags & LPX_BDUAL_CUTOFF) ? best + EPS : 0.0);
        }
        // 4. evaluate
        const int B = (int)slot.size();
        int rc;
        if (strong) {
            prunes.assign((size_t)B, best + EPS);
            heads.resize((size_t)B); probes.resize((size_t)B * 2 * (size_t)strong->cand_max);
            rc = lpx_node_batch_run_probe(pool.batch, B, slot.data(), Ks.data(), cols.data(), clo.data(), cub.data(), &o,
                                          LPX_BDUAL_SKIP_FIXED | search_flags, cutoffs.data(), prunes.data(), n, mask, EPS,
                                          strong->cand_max, strong->probe_iter, recs.data(), heads.data(), probes.data(), rcs.data());
        } else if (tightening) {
            guards.resize((size_t)B);
            fix_bounds.assign((size_t)B, best + EPS);                       // -inf while there is no incumbent
            fixes.resize((size_t)B); fix_cols.resize((size_t)B * n); fix_lower.resize((size_t)B * n); fix_upper.resize((size_t)B * n);
            for (int i = 0; i < B; ++i)
                fixes[i] = lpx_fix_list{n, 0, fix_cols.data() + (size_t)i * n, fix_lower.data() + (size_t)i * n, fix_upper.data() + (size_t)i * n};
            rc = lpx_node_batch_run3(pool.batch, B, slot.data(), Ks.data(), cols.data(), clo.data(), cub.data(), &o,
                                     LPX_BDUAL_SKIP_FIXED | search_flags, cutoffs.data(), stall_events, fix_bounds.data(), n, mask, EPS,
                                     recs.data(), guards.data(), fixes.data(), rcs.data());
        } else if (guarded) {
            guards.resize((size_t)B);
            rc = lpx_node_batch_run2(pool.batch, B, slot.data(), Ks.data(), cols.data(), clo.data(), cub.data(), &o,
                                     LPX_BDUAL_SKIP_FIXED | search_flags, cutoffs.data(), stall_events, n, mask, EPS, recs.data(),
                                     guards.data(), rcs.data());
        } else
            rc = lpx_node_batch_run(pool.batch, B, slot.data(), Ks.data(), cols.data(), clo.data(), cub.data(), &o,
                                    LPX_BDUAL_SKIP_FIXED | search_flags, cutoffs.data(), n, mask, EPS, recs.data(), rcs.data());
        if (rc < 0) throw_lib(rc);
        if (strong) {
            si.probe_launches++;
            for (const lpx_probe_record& q : probes) {
                if (q.status == LPX_PROBE_NONE) continue;
                si.probes++; si.probe_events += q.events;
                if (q.status == LPX_ITER_LIMIT) si.probe_limit++;
            }
        }
        for (int i = 0; i < B; ++i) if (rcs[i] < 0) throw_lib(rcs[i]);
        const int32_t round = (int32_t)dinfo.rounds++;
        if (B > dinfo.largest_batch) dinfo.largest_batch = B;
        // 5. decide, in diver order
        for (int i = 0; i < B; ++i) {
            Diver& D = dv[slot[i]];
            const lpx_node_record& rec = recs[i];
            const Node& node = D.node;
            const int64_t index = info.nodes++;
            const int nfix = tightening ? fixes[i].n : 0;
            for (int k = 0; k < nfix; ++k) { D.nb_lo[fixes[i].cols[k]] = fixes[i].lower[k]; D.nb_ub[fixes[i].cols[k]] = fixes[i].upper[k]; }
            if (nfix > 0) { fi.tightened_nodes++; fi.tightened_cols += nfix; if (nfix > fi.max_per_node) fi.max_per_node = nfix; }
            D.cur_lo = D.nb_lo; D.cur_ub = D.nb_ub;
            const bool limit = LogNode(info, index, node.depth, Ks[i], rec, o.max_iter);
            dinfo.round.push_back(round); dinfo.diver.push_back(slot[i]);
            if (guarded) {
                if (guards[i].bland_events > 0) { gi.guarded_nodes++; gi.bland_events += guards[i].bland_events; }
                if (rec.events > gi.max_events) gi.max_events = rec.events;
            }
            if (limit) { stop = true; break; }
            if (rec.status == LPX_INFEASIBLE) { info.pruned_infeasible++; continue; }
            const double z = rec.pick.z;
            if (rec.status == LPX_CUTOFF || z <= best + EPS) { info.pruned_bound++; continue; }
            if (rec.pick.var < 0) { TakeIncumbent(pool.h[slot[i]], n, is_int, z, best, best_x, info); continue; }
            int v = rec.pick.var;
            double xv = rec.pick.x_var;
            bool push_fl = true, push_ce = true;
            if (strong && heads[i].count >= 1) {
                const lpx_probe_record* pr = &probes[(size_t)i * 2 * (size_t)strong->cand_max];
                int pick = 0;
                double top = -1.0;
                for (int c = 0; c < heads[i].count; ++c) {
                    const double score = gain(pr[2 * c], z) * gain(pr[2 * c + 1], z);
                    if (score > top) { top = score; pick = c; }         // the first maximum
                }
                v = pr[2 * pick].var; xv = pr[2 * pick].x_var;
                if (pick != 0) si.changed_picks++;
                push_fl = !dead(pr[2 * pick], best); push_ce = !dead(pr[2 * pick + 1], best);
                si.pruned_by_probe += (push_fl ? 0 : 1) + (push_ce ? 0 : 1);
                info.log.back().var = v;
            }
            Node fl{node.depth + 1, node.path}, ce{node.depth + 1, node.path};
            for (int k = 0; k < nfix; ++k) {                            // in front of the branching override
                const Override ov{fixes[i].cols[k], fixes[i].lower[k], fixes[i].upper[k]};
                fl.path.push_back(ov); ce.path.push_back(ov);
            }
            fl.path.push_back(Override{v, D.nb_lo[v], std::floor(xv)});
            ce.path.push_back(Override{v, std::ceil(xv), D.nb_ub[v]});
            if (push_fl) D.stack.push_back(std::move(fl));
            if (push_ce) D.stack.push_back(std::move(ce));
        }
    }

    return FinishBnbResult(std::move(res), info, ses, n, best, best_x);
}

// The search by W divers that plunge (lpx_solve_bnb_bounded5, include/lpx.h): SolveBnbDivers whose round is ONE
// lpx_node_batch_plunge -- every diver's workgroup goes on from a node that branches into its ceil child, up to `plunge` nodes,
// with the tableau staying on chip -- and whose decide step walks every diver's chain in order.  The order of the steps is part
// of the contract: the log is a function of the model, the options, the flags, W and D alone.
SimplexResult SolveBnbPlunge(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                             const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                             int search_flags, int divers, int plunge, BnbDiversInfo& dinfo, BnbPlungeInfo& pinfo)
{
    const int n = original.NumVars();
    ValidateBnbBounded(n, lower, upper, is_int, max_nodes, search_flags);
    if (divers < 1 || divers > 1024) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: divers is outside [1, 1024]");
    if (plunge < 1 || plunge > 64) throw LpxException(LPX_EINVAL, "Bounded Branch and Bound: plunge is outside [1, 64]");

    BoundedSession ses;
    BoundedInfo binfo;
    SimplexResult res;
    if (!SolveRoot(original, lower, upper, opt, true, ses, binfo, res, info, &dinfo, &pinfo)) return res;

    const int W = divers, D = plunge;
    Pool pool;
    pool.open(ses.h, W);

    const std::vector<double> root_lo((size_t)n, 0.0), root_ub(binfo.ub.begin(), binfo.ub.begin() + n);
    std::vector<Diver> dv((size_t)W);
    for (Diver& d : dv) { d.cur_lo = root_lo; d.cur_ub = root_ub; }
    dv[0].stack.push_back(Node{0, {}});
    lpx_run_opts o; lpx_default_opts(&o, 1);
    o.max_iter = opt.max_iter;
    const uint8_t* mask = is_int.empty() ? nullptr : is_int.data();

    double best = -1.0 / 0.0;
    std::vector<double> best_x;
    std::vector<int32_t> slot, Ks, caps, cols, rcs((size_t)W), steps((size_t)W); std::vector<double> clo, cub, cutoffs, prunes;
    std::vector<lpx_node_record> recs((size_t)W * (size_t)D);
    bool stop = false;
    while (!stop && AnyOpen(dv)) {
        // 1. limit, 2. steal
        if (NodeLimitReached(max_nodes, info)) break;
        StealForIdle(dv, dinfo);
        // 3. pop, each entry with its cap on nodes: plunge, or what max_nodes leaves after the caps handed out before it
        slot.clear(); Ks.clear(); caps.clear(); cols.clear(); clo.clear(); cub.clear(); cutoffs.clear(); prunes.clear();
        int64_t handed = 0;
        for (int d = 0; d < W; ++d) {
            Diver& Dv = dv[d];
            if (Dv.stack.empty()) continue;
            int cap = D;
            if (max_nodes > 0) {
                const int64_t left = max_nodes - info.nodes - handed;
                if (left <= 0) break;
                if (left < cap) cap = (int)left;
            }
            handed += cap;
            Dv.node = std::move(Dv.stack.back());
            Dv.stack.pop_back();
            const int K = DiffBounds(Dv.node, root_lo, root_ub, Dv.cur_lo, Dv.cur_ub, Dv.nb_lo, Dv.nb_ub, cols, clo, cub);
            slot.push_back(d); Ks.push_back(K); caps.push_back(cap);
            cutoffs.push_back((search_flags & LPX_BDUAL_CUTOFF) ? best + EPS : 0.0);
            prunes.push_back(best + EPS);
        }
        // 4. evaluate
        const int B = (int)slot.size();
        const int rc = lpx_node_batch_plunge(pool.batch, B, slot.data(), Ks.data(), cols.data(), clo.data(), cub.data(), &o,
                                             LPX_BDUAL_SKIP_FIXED | search_flags, cutoffs.data(), prunes.data(), caps.data(), D,
                                             n, mask, EPS, recs.data(), steps.data(), rcs.data());
        if (rc < 0) throw_lib(rc);
        for (int i = 0; i < B; ++i) if (rcs[i] < 0) throw_lib(rcs[i]);
        const int32_t round = (int32_t)dinfo.rounds++;
        if (B > dinfo.largest_batch) dinfo.largest_batch = B;
        for (int i = 0; i < B; ++i) { pinfo.launched += steps[i]; if (steps[i] > pinfo.longest_chain) pinfo.longest_chain = steps[i]; }
        // 5. decide: divers ascending, each diver's records in chain order
        for (int i = 0; i < B && !stop; ++i) {
            Diver& Dv = dv[slot[i]];
            Node node = Dv.node;                                        // the node of record s: depth and path grow along the chain
            const int ns = steps[i];
            for (int s = 0; s < ns; ++s) {
                const lpx_node_record& rec = recs[(size_t)i * D + s];
                const int K = s == 0 ? Ks[i] : 1;
                const bool has_next = s + 1 < ns;
                const int64_t index = info.nodes++;
                const bool limit = LogNode(info, index, node.depth, K, rec, o.max_iter);
                dinfo.round.push_back(round); dinfo.diver.push_back(slot[i]); pinfo.step.push_back(s);
                if (limit) { stop = true; break; }
                if (rec.status == LPX_INFEASIBLE) { info.pruned_infeasible++; break; }
                const double z = rec.pick.z;
                if (rec.status == LPX_CUTOFF || z <= best + EPS) {
                    // the kernel went on past this record against the best of the start of the round; best has moved since
                    info.pruned_bound++;
                    pinfo.dropped += ns - 1 - s;
                    for (int k = s; k + 1 < ns; ++k) {                  // the handle holds the bounds of the last node evaluated
                        const lpx_node_record& rk = recs[(size_t)i * D + k];
                        Dv.nb_lo[rk.pick.var] = std::ceil(rk.pick.x_var);
                    }
                    break;
                }
                if (rec.pick.var < 0) {                                  // always the last record of its chain: the handle holds its x
                    TakeIncumbent(pool.h[slot[i]], n, is_int, z, best, best_x, info);
                    break;
                }
                const int v = rec.pick.var;
                Node fl{node.depth + 1, node.path}, ce{node.depth + 1, node.path};
                fl.path.push_back(Override{v, Dv.nb_lo[v], std::floor(rec.pick.x_var)});
                ce.path.push_back(Override{v, std::ceil(rec.pick.x_var), Dv.nb_ub[v]});
                Dv.stack.push_back(std::move(fl));
                if (has_next) { Dv.nb_lo[v] = std::ceil(rec.pick.x_var); node = std::move(ce); }      // the ceil child is the next record
                else Dv.stack.push_back(std::move(ce));
            }
            Dv.cur_lo = Dv.nb_lo; Dv.cur_ub = Dv.nb_ub;
        }
    }

    return FinishBnbResult(std::move(res), info, ses, n, best, best_x);
}

}}  // namespace lpx::host
