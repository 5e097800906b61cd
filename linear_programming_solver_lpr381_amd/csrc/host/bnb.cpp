// host/bnb.cpp -- BranchAndBound mirror (Models/Branch&Bound.cs:20-304).
//
// Every node is an LP rebuilt from the root model plus its branching rows and re-solved from the
// slack basis on the GPU, exactly as the reference re-solves through LPSolver (:148).  Two modes:
//   faithful (bnb_mode 0)  DualSimplex keeps defects D1/D2: every `>=` child comes back without
//                          Solution/Tableau/Basis and is dropped as "Invalid" (:157-161).
//   repaired (bnb_mode 1)  DualSimplex runs with LPX_DUAL_REPAIRED; INFEASIBLE relaxations are pruned.
// Three searches:
//   bnb_search 0  the reference's recursive DFS, ceil child first (:256-257) -- node order, incumbent
//                 and node log are those of the reference.
//   bnb_search 1  level-synchronous frontier for the sharded node queue: the first levels are
//                 expanded redundantly on every rank until the frontier holds >= world*concurrent
//                 nodes, then frontier[i] belongs to rank i % world and stays local with its
//                 subtree; per level each rank solves its node LPs `concurrent_nodes` at a time
//                 (lpx_multi_run) and ONE all-reduce(max) over {incumbent z, have_work} is exchanged.
//   bnb_search 2  the same level frame with WARM-STARTED children (repaired mode, device only).
// A node's LP -- prepared, solved in groups, tested for feasibility -- is host/bnb_nodes.cpp; the rank protocol of the sharded
// searches is host/sharded.h.
#include "bnb_nodes.h"
#include "sharded.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <thread>

namespace lpx { namespace host {

using namespace bnb;

namespace {

constexpr int MaxDepth = 200;     // :25

enum Outcome { O_ERROR = 0, O_INVALID = 1, O_INFEASIBLE_X = 2, O_PRUNED = 3, O_INCUMBENT = 4, O_NO_FRAC = 5,
               O_BRANCHED = 6, O_DEPTH = 7, O_LP_INFEASIBLE = 8 };

// The feasibility test of :175-179 for a whole level ahead of the decisions: it is a pure function of a node's x (768 rows x 512
// columns at config 4: ~15 us per node, a tenth of the warm-started leg when done one node at a time between the device
// batches), so the nodes of a level are tested on a few host threads; decide() then takes the verdict from NodeLP::feas.  Order
// of the decisions, logs and incumbent updates is untouched.  LPX_HOST_THREADS=n (default: up to 8; 1 = off).
template <class FN>
void precompute_feas(Ctx& c, std::vector<NodeLP>& lps, const std::vector<FN>& frontier, const std::vector<char>& skip)
{
    static const int nthreads = [] {
        const char* e = std::getenv("LPX_HOST_THREADS"); int v = e ? std::atoi(e) : 0;
        if (v <= 0) { v = (int)std::thread::hardware_concurrency(); if (v > 8) v = 8; }
        return v < 1 ? 1 : v; }();
    std::vector<size_t> todo;
    for (size_t i = 0; i < lps.size(); ++i) {
        const NodeLP& lp = lps[i];
        if (skip[i] || lp.error || !lp.has_solution || lp.feas >= 0 || (c.opt.bnb_mode == 1 && lp.status == LPX_INFEASIBLE)) continue;
        todo.push_back(i);
    }
    if (nthreads < 2 || todo.size() < 64) return;
    if (!c.feas.built) c.feas.build(*c.root);
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= todo.size()) break;
            const size_t i = todo[k];
            lps[i].feas = IsFeasibleIndexed(lps[i].x, *c.root, frontier[i].cuts, c.feas) ? 1 : 0;
        }
    };
    std::vector<std::thread> pool;
    const int n = std::min<int>(nthreads, (int)(todo.size() / 32) + 1);
    for (int t = 1; t < n; ++t) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
}

void node_log(Ctx& c, int depth, int outcome, int var, double z)
{
    c.out->NodeLog.push_back(depth); c.out->NodeLog.push_back(outcome); c.out->NodeLog.push_back(var);
    c.out->NodeZ.push_back(z);
}

std::vector<uint8_t> key_of(const std::vector<Cut>& cuts)
{
    std::vector<uint8_t> k(cuts.size());
    for (size_t i = 0; i < cuts.size(); ++i) k[i] = cuts[i].rel == Rel::GE ? 0 : 1;
    return k;
}

void set_incumbent(Ctx& c, const std::vector<double>& x, double z, const std::vector<Cut>& cuts = {})
{
    c.best = z; c.has_best = true;
    c.best_x.resize(x.size());
    for (size_t i = 0; i < x.size(); ++i) c.best_x[i] = std::nearbyint(x[i]);    // RoundInt, :296
    c.best_key = key_of(cuts);
}

// The decision part of SolveNode (:156-230) for a solved relaxation.  Returns the branching
// variable (>= 0) when the node branches, else -1.
int decide(Ctx& c, const std::vector<Cut>& cuts, const NodeLP& lp, int depth, const std::string& name, int& floorVal, int& ceilVal)
{
    if (lp.error) { c.log(name + ": LP relaxation infeasible or error"); node_log(c, depth, O_ERROR, -1, 0.0); return -1; }
    if (!lp.has_solution) {
        c.log(name + ": Invalid Simplex result (missing Solution, Tableau, Basis, or VarNames).");
        node_log(c, depth, O_INVALID, -1, 0.0); return -1;
    }
    if (c.opt.bnb_mode == 1 && lp.status == LPX_INFEASIBLE) { node_log(c, depth, O_LP_INFEASIBLE, -1, lp.z); return -1; }
    const std::vector<double>& x = lp.x; const double z = lp.z;
    if (c.cb) c.log(name + " LP solution: z* = " + FormatF(z, 3));
    if (!(lp.feas >= 0 ? lp.feas == 1 : IsFeasibleIndexed(x, *c.root, cuts, c.feas))) { c.log(name + ": Solution is infeasible for constraints."); node_log(c, depth, O_INFEASIBLE_X, -1, z); return -1; }   // :175-179
    const double bestObj = c.has_best ? c.best : -INFINITY;
    // Sharded searches visit nodes level by level, not in the reference's depth-first order.  Among integer nodes with
    // EXACTLY the incumbent's z the one the reference's DFS reaches first keeps the solution vector (first found wins
    // there, :182-195): smaller DFS-order key.  Counters and the node log are untouched (the node is pruned as always).
    if (c.tie_by_key && c.has_best && z == c.best && IsIntegral(x)) {
        const std::vector<uint8_t> k = key_of(cuts);
        if (c.best_x.empty() || k < c.best_key) {
            c.best_x.resize(x.size());
            for (size_t i = 0; i < x.size(); ++i) c.best_x[i] = std::nearbyint(x[i]);
            c.best_key = k;
        }
    }
    if (z <= bestObj + EPS) { c.log(name + ": Pruned by bound (z* <= current best " + FormatF(bestObj, 3) + ")."); node_log(c, depth, O_PRUNED, -1, z); return -1; }   // :182-186
    if (IsIntegral(x)) {                                                     // :189-195
        set_incumbent(c, x, z, cuts);
        c.log(name + " is integer feasible. Updated BestObjective = " + FormatF(z, 3));
        node_log(c, depth, O_INCUMBENT, -1, z); return -1;
    }
    int fracIndex = -1; double minDist = 1.7976931348623157e308;             // :198-213
    for (int i = 0; i < (int)x.size(); ++i) {
        double fracPart = x[i] - std::floor(x[i]);
        if (fracPart > EPS && (1 - fracPart) > EPS) {
            double dist = std::fabs(fracPart - 0.5);
            if (dist < minDist || (dist == minDist && i < fracIndex)) { minDist = dist; fracIndex = i; }
        }
    }
    if (fracIndex == -1) { node_log(c, depth, O_NO_FRAC, -1, z); return -1; }  // :215-219
    floorVal = (int)std::floor(x[fracIndex]);                                // :222-223
    ceilVal = (int)std::ceil(x[fracIndex]);
    c.log(name + ": Branching on x" + std::to_string(fracIndex + 1) + " = " + FormatF(x[fracIndex], 3) +
          " (floor=" + std::to_string(floorVal) + ", ceil=" + std::to_string(ceilVal) + ")");
    node_log(c, depth, O_BRANCHED, fracIndex, z);
    return fracIndex;
}

// ---- search 0: the reference's recursion (:128-258) ---------------------------------------------------
void SolveNode(Ctx& c, std::vector<Cut>& cuts, int depth, const std::string& name)
{
    if (c.stop) return;
    if (c.opt.max_nodes > 0 && c.out->Nodes >= c.opt.max_nodes) { c.stop = true; return; }
    c.out->Nodes++;
    if (depth > MaxDepth) { c.log(name + ": Maximum recursion depth reached -> prune."); node_log(c, depth, O_DEPTH, -1, 0.0); return; }
    NodeLP lp;
    cold_node(c, cuts, lp);
    std::vector<NodeLP*> g{&lp};
    solve_group(c, g, c.root->NumVars());
    int fl = 0, ce = 0;
    int k = decide(c, cuts, lp, depth, name, fl, ce);
    if (k < 0) return;
    cuts.push_back({k, Rel::GE, (double)ce});
    SolveNode(c, cuts, depth + 1, "Subproblem: x" + std::to_string(k + 1) + " >= " + std::to_string(ce));   // ceil first, :256
    cuts.back() = {k, Rel::LE, (double)fl};
    SolveNode(c, cuts, depth + 1, "Subproblem: x" + std::to_string(k + 1) + " <= " + std::to_string(fl));   // :257
    cuts.pop_back();
}

// ---- searches 1 and 2: level-synchronous frontier, sharded by host/sharded.h -------------------------------------------

// final ownership of the solution vector: among the ranks holding an x for the global best z, the one whose node comes
// first in the reference's DFS order (smallest key) publishes it -- ONE all-reduce for the keys, one for x
void publish_best(Ctx& c, Sharded& sh, int nvars)
{
    constexpr int CH = 5, BITS = 48;                                   // 240 key bits >= MaxDepth + 1 levels
    const int world = sh.world, rank = sh.rank;
    std::vector<double> keys((size_t)world * (CH + 1), -INFINITY);
    const bool cand = c.has_best && !c.best_x.empty();
    if (cand) {
        keys[(size_t)rank * (CH + 1)] = 1.0;                           // "rank holds an x for the best z"
        for (int k = 0; k < CH; ++k) {
            double v = 0.0;
            for (int b = 0; b < BITS; ++b) { const size_t i = (size_t)k * BITS + b; v = v * 2.0 + (i < c.best_key.size() ? c.best_key[i] : 1); }
            keys[(size_t)rank * (CH + 1) + 1 + k] = v;
        }
    }
    sh.max(keys.data(), (int)keys.size());
    int owner = -1;
    for (int r = 0; r < world; ++r) {
        if (keys[(size_t)r * (CH + 1)] != 1.0) continue;
        if (owner < 0) { owner = r; continue; }
        for (int k = 1; k <= CH; ++k) {
            const double a = keys[(size_t)r * (CH + 1) + k], b = keys[(size_t)owner * (CH + 1) + k];
            if (a != b) { if (a < b) owner = r; break; }
        }
    }
    if (owner < 0) return;
    std::vector<double> xs(nvars, -INFINITY);
    if (owner == rank) xs = c.best_x;
    sh.max(xs.data(), nvars);
    c.best_x = xs;
}

// what the ranks must agree on when the replicated phase ends (Sharded::agree): the frontier, branching row by branching row
template <class FN> double frontier_fingerprint(const std::vector<FN>& frontier, bool handed_out)
{
    Fingerprint fp(handed_out);
    fp.mix((uint64_t)frontier.size());
    for (const FN& f : frontier) {
        fp.mix((uint64_t)f.cuts.size());
        for (const Cut& k : f.cuts) { fp.mix((uint64_t)(uint32_t)k.var); fp.mix((uint64_t)(int)k.rel); fp.mix_bits(k.bound); }
    }
    return fp.value();
}

// The two searches are one level frame (level_search below) with a node policy each, which says
//   seed            what the first level starts from (false: there is no search)
//   fill            how a frontier entry becomes a NodeLP
//   branch          how the two children of a branched node are appended, ceil child first
//   release_parent  what goes when an entry leaves the frontier: solved with its level, dropped, or not taken at the hand-out
//   release_result  what goes when a solved node is not branched
//   rebalances      whether node descriptors move between ranks after the exchange (and ride in its vector)
//   guards_decide   whether a throw out of the decisions raises `failed` as one out of the solve does
//   times_decide    whether the decisions are timed into g_pt

// search 1: every node is rebuilt from the root model wherever it is solved, as the reference re-solves every node from scratch
struct FNode { std::vector<Cut> cuts; int depth; };
struct ColdNodes {
    using Node = FNode;
    static constexpr bool rebalances = true, guards_decide = false, times_decide = false;
    bool seed(Ctx&, Sharded&, std::vector<FNode>& frontier) { frontier.push_back(FNode{{}, 0}); return true; }
    void fill(Ctx& c, const FNode& f, NodeLP& lp) { cold_node(c, f.cuts, lp); }
    void branch(std::vector<FNode>& out, const FNode& f, const NodeLP&, int k, int fl, int ce)
    {
        FNode up{f.cuts, f.depth + 1}; up.cuts.push_back({k, Rel::GE, (double)ce});
        FNode dn{f.cuts, f.depth + 1}; dn.cuts.push_back({k, Rel::LE, (double)fl});
        out.push_back(std::move(up)); out.push_back(std::move(dn));
    }
    void release_parent(const FNode&) {}
    void release_result(const NodeLP&) {}
};

// search 2: WARM-STARTED children.  Not the reference's algorithm (it re-solves every node from the slack
// basis): a child starts from its parent's final tableau plus the branching row written in the parent's basis, which is dual
// feasible, so only the dual loop runs -- typically a handful of pivots instead of hundreds.  Same LP optimum per node, hence the
// same B&B optimum; the optimal VERTEX of a degenerate node may differ from a cold solve, so node order and counts are not
// comparable with searches 0/1.
struct WNode { std::vector<Cut> cuts; int depth; lpx_store* store; int slot; int prow; };
struct WarmNodes {
    using Node = WNode;
    static constexpr bool rebalances = false, guards_decide = true, times_decide = true;
    int w = 0;                                                 // the root's template: primal 0 / dual 1
    std::map<std::pair<lpx_store*, int>, int> refs;           // a parked parent serves two children: release its slot when both are built
    // the root is solved cold and parked before the first level
    bool seed(Ctx& c, Sharded& sh, std::vector<WNode>& frontier)
    {
        const bool root_dual = has_ge_or_eq(*c.root);
        if (!ensure_template(c, root_dual)) return false;
        w = root_dual ? 1 : 0;
        NodeLP lp; cold_node(c, {}, lp); lp.keep = true;
        c.budget_used++;
        if (c.count_work) c.out->Nodes++;
        std::vector<NodeLP*> g{&lp};
        try {
            solve_group(c, g, c.root->NumVars());
            int fl = 0, ce = 0;
            const WNode root{{}, 0, nullptr, -1, -1};
            const int k = decide(c, root.cuts, lp, 0, "Root Problem", fl, ce);
            if (k < 0) { release_result(lp); return sh.sharded; }   // sharded: on to the one all-reduce that says every rank ended here
            branch(frontier, root, lp, k, fl, ce);
        } catch (const LpxException& e) {
            // the peers solve the same root and go on to their first level's all-reduce: meet them there
            if (!sh.sharded) throw;
            sh.fail(e); c.stop = true; frontier.clear();
        }
        return true;
    }
    void fill(Ctx& c, const WNode& f, NodeLP& lp)
    {
        const Cut& k = f.cuts.back();
        lp.warm = true; lp.dual = true; lp.keep = true; lp.wslot = w; lp.depth = f.depth;
        lp.pstore = f.store; lp.pslot = f.slot; lp.prow = f.prow;
        lp.cvar.push_back(k.var); lp.wis_ge = (k.rel == Rel::GE); lp.wbound = k.bound;
        lp.R = c.tplR[w] + f.depth; lp.C = c.tplC[w] + f.depth;
        lp.cuts_for_feas = &f.cuts;
    }
    void branch(std::vector<WNode>& out, const WNode& f, const NodeLP& lp, int k, int fl, int ce)
    {
        int ik = -1;
        for (size_t i = 0; i < lp.basis_out.size() && ik < 0; ++i) if (lp.basis_out[i] == k) ik = (int)i;
        if (ik < 0 || lp.kslot < 0) throw LpxException(LPX_EINVAL, "warm start: branching variable is not basic in the parked parent");
        WNode up{f.cuts, f.depth + 1, lp.kstore, lp.kslot, ik}; up.cuts.push_back({k, Rel::GE, (double)ce});
        WNode dn{f.cuts, f.depth + 1, lp.kstore, lp.kslot, ik}; dn.cuts.push_back({k, Rel::LE, (double)fl});
        out.push_back(std::move(up)); out.push_back(std::move(dn));
        refs[{lp.kstore, lp.kslot}] = 2;
    }
    void release_parent(const WNode& f)
    {
        auto it = refs.find({f.store, f.slot});
        if (it != refs.end() && --it->second == 0) { lpx_store_release(f.store, f.slot); refs.erase(it); }
    }
    void release_result(const NodeLP& lp) { if (lp.kslot >= 0) lpx_store_release(lp.kstore, lp.kslot); }
};

// Rebalancing (search 1): node descriptors (branching rows) move, tableaux never do -- a node is rebuilt from the root model
// wherever it is solved, exactly as the reference re-solves every node from scratch (Models/Branch&Bound.cs:148,233-248).
// `vals` is the level's reduced exchange vector: the deepest pooled node in slot 3, rank r's pool size in slot 4 + r (-1 = that
// rank takes no more nodes).
void rebalance(Ctx& c, Sharded& sh, std::vector<FNode>& frontier, const std::vector<double>& vals)
{
    const int world = sh.world, rank = sh.rank;
    std::vector<int64_t> size(world);
    int64_t total = 0, smax = 0, smin = INT64_MAX; int active = 0;
    for (int r = 0; r < world; ++r) { size[r] = (int64_t)vals[4 + r]; if (size[r] >= 0) { total += size[r]; smax = std::max(smax, size[r]); smin = std::min(smin, size[r]); ++active; } }
    const int64_t slack = std::max<int64_t>(2, c.opt.concurrent_nodes);
    if (!(active >= 2 && ((smin == 0 && smax >= 2) || smax - smin > 2 * slack))) return;
    std::vector<int64_t> fin(world, -1);
    { int64_t base = total / active, rem = total % active; int a = 0;
      for (int r = 0; r < world; ++r) if (size[r] >= 0) { fin[r] = base + (a < rem ? 1 : 0); ++a; } }
    struct Move { int from, to; int64_t count; };
    std::vector<Move> moves;
    { int d = 0, t = 0; std::vector<int64_t> give(world, 0), take(world, 0);
      for (int r = 0; r < world; ++r) if (size[r] >= 0) { give[r] = std::max<int64_t>(0, size[r] - fin[r]); take[r] = std::max<int64_t>(0, fin[r] - size[r]); }
      while (d < world && t < world) {
          if (give[d] == 0) { ++d; continue; }
          if (take[t] == 0) { ++t; continue; }
          const int64_t k = std::min(give[d], take[t]);
          moves.push_back({d, t, k}); give[d] -= k; take[t] -= k;
      } }
    int64_t nmoved = 0; for (const Move& mv : moves) nmoved += mv.count;
    if (nmoved <= 0) return;
    const int D = (int)vals[3];
    const size_t stride = 1 + 3 * (size_t)std::max(D, 1);
    std::vector<double> buf((size_t)nmoved * stride, -INFINITY);
    size_t slot = 0;
    for (const Move& mv : moves) {
        if (mv.from == rank)
            for (int64_t k = 0; k < mv.count; ++k) {                 // donors give from the end of their pool
                const FNode f = std::move(frontier.back()); frontier.pop_back();
                double* b = &buf[(slot + (size_t)k) * stride];
                b[0] = (double)f.cuts.size();
                for (size_t e = 0; e < f.cuts.size(); ++e) { b[1 + 3 * e] = f.cuts[e].var; b[2 + 3 * e] = (double)(int)f.cuts[e].rel; b[3 + 3 * e] = f.cuts[e].bound; }
            }
        slot += (size_t)mv.count;
    }
    sh.max(buf.data(), (int)buf.size());
    slot = 0;
    for (const Move& mv : moves) {
        if (mv.to == rank)
            for (int64_t k = 0; k < mv.count; ++k) {
                const double* b = &buf[(slot + (size_t)k) * stride];
                FNode f; const int nc = (int)b[0]; f.depth = nc;
                for (int e = 0; e < nc; ++e) f.cuts.push_back({(int)b[1 + 3 * e], (Rel)(int)b[2 + 3 * e], b[3 + 3 * e]});
                frontier.push_back(std::move(f));
            }
        slot += (size_t)mv.count;
    }
    c.rebalances++; c.moved += nmoved;
}

template <class Policy>
void level_search(Ctx& c, Policy& P)
{
    using Node = typename Policy::Node;
    Sharded sh(c.opt, "the node LPs");
    const int world = sh.world, nvars = c.root->NumVars();
    c.tie_by_key = true;
    // The replicated warm-up only has to seed every rank with a subtree: 2 nodes per rank.  Its solves are
    // redundant across ranks, so only rank 0 counts them (LpSolves / Nodes stay whole-job totals when summed).
    const size_t want = (size_t)world * 2;
    c.count_work = !(sh.replicated && sh.rank != 0);
    c.budget_used = 0; c.budget_cap = c.opt.max_nodes;
    std::vector<Node> frontier;
    if (!P.seed(c, sh, frontier)) return;
    if (sh.sharded && !sh.replicated && !sh.failed) sh.agree(frontier_fingerprint(frontier, false));   // a world of one (LPX_COMM_SHARD_ONE): nothing was replicated
    for (;;) {
        if (sh.replicated && frontier.size() >= want) {
            // hand the replicated frontier out: node i -> rank i % world, subtrees stay local from here on
            const double h = frontier_fingerprint(frontier, true);
            std::vector<Node> mine;
            for (size_t i = 0; i < frontier.size(); ++i) {
                if (sh.mine(i)) mine.push_back(std::move(frontier[i]));
                else P.release_parent(frontier[i]);
            }
            frontier.swap(mine);
            sh.agree(h);
            c.count_work = true;
            if (c.opt.max_nodes > 0) {                                 // the rest of the global budget, split evenly
                const int64_t left = std::max<int64_t>(0, c.opt.max_nodes - c.budget_used);
                c.budget_cap = c.budget_used + (left + world - 1) / world;
            }
        }
        // this level's nodes: the whole frontier (breadth first) or, with bnb_dive, its deepest K nodes
        std::vector<Node> parked;
        if (c.opt.bnb_dive && !sh.replicated && frontier.size() > (size_t)std::max(1, c.opt.concurrent_nodes)) {
            std::stable_sort(frontier.begin(), frontier.end(), [](const Node& a, const Node& b) { return a.depth > b.depth; });
            const size_t K = (size_t)std::max(1, c.opt.concurrent_nodes);
            parked.assign(std::make_move_iterator(frontier.begin() + K), std::make_move_iterator(frontier.end()));
            frontier.resize(K);
        }
        std::vector<NodeLP> lps(frontier.size());
        std::vector<NodeLP*> group;
        std::vector<char> skip(frontier.size(), 0);                    // 1: not solved (budget, failure), 2: too deep
        for (size_t i = 0; i < frontier.size(); ++i) {
            if (sh.failed || c.over_budget()) { skip[i] = 1; c.stop = true; continue; }
            c.budget_used++;
            if (c.count_work) c.out->Nodes++;
            if (frontier[i].depth > MaxDepth) { skip[i] = 2; continue; }
            P.fill(c, frontier[i], lps[i]);
            group.push_back(&lps[i]);
        }
        c.levels++;                 // once per pass, wherever it stands: Aux is read after the loop (the warm search's root is no level)
        std::vector<Node> next;
        auto timed = [&](auto&& f) {
            if (!Policy::times_decide) return f();
            const double t0 = PhaseTimer::now(); const int r = f(); g_pt.decide += PhaseTimer::now() - t0; return r;
        };
        auto decide_level = [&] {
            timed([&] { precompute_feas(c, lps, frontier, skip); return 0; });
            for (size_t i = 0; i < frontier.size(); ++i) {
                if (skip[i] == 1) continue;
                if (skip[i] == 2) { node_log(c, frontier[i].depth, O_DEPTH, -1, 0.0); continue; }
                int fl = 0, ce = 0;
                const int k = timed([&] { return decide(c, frontier[i].cuts, lps[i], frontier[i].depth, "Node", fl, ce); });
                if (k < 0) { P.release_result(lps[i]); continue; }
                P.branch(next, frontier[i], lps[i], k, fl, ce);
            }
        };
        try {
            solve_group(c, group, nvars);
            for (const Node& f : frontier) P.release_parent(f);        // every node of this level is built
            if (Policy::guards_decide) decide_level();
        } catch (const LpxException& e) {
            // a rank that leaves the loop would leave its peers waiting in the level's all-reduce: keep taking part with `failed`
            // up, then stop together (Sharded).  For the warm search LPX_ENOMEM is the plausible one (thousands of ~8 MB parent
            // tableaux are parked); they go with the stores when the search's context is destroyed.
            if (!sh.sharded) throw;
            sh.fail(e); c.stop = true;
            skip.assign(skip.size(), 1); next.clear(); parked.clear();
        }
        if (!Policy::guards_decide) decide_level();
        frontier.swap(next);
        for (Node& f : parked) frontier.push_back(std::move(f));
        if (c.stop) { for (const Node& f : frontier) P.release_parent(f); frontier.clear(); }   // out of budget or failed: this rank takes no more nodes
        const bool have_work = !frontier.empty();
        // the search ended inside the replicated warm-up: the same on every rank if all is well -- one all-reduce says so
        if (sh.sharded && sh.replicated && !have_work) sh.agree(frontier_fingerprint(frontier, false));
        if (!sh.exchanging()) { if (!have_work) break; continue; }
        // ---- X1: ONE all-reduce(max) per level (Sharded::exchange); the cold search adds the deepest pooled node and every
        //      rank's pool size (slot 4 + r; -1 = this rank takes no more nodes: what it received would be dropped at the next
        //      level) for the rebalancing
        std::vector<double> vals(Policy::rebalances ? 6 + (size_t)world : 5, -INFINITY);
        if (Policy::rebalances) {
            int maxd = 0; for (const Node& f : frontier) maxd = std::max(maxd, f.depth);
            vals[3] = (double)maxd;
            vals[4 + sh.rank] = (c.stop || c.over_budget()) ? -1.0 : (double)frontier.size();
        }
        const Sharded::Round r = sh.exchange(vals.data(), (int)vals.size(), c.has_best ? c.best : -INFINITY, have_work);
        if (r.better) { c.best = r.best; c.has_best = true; c.best_x.clear(); c.best_key.clear(); }
        if (r.verdict != Sharded::GO_ON) break;
        if constexpr (Policy::rebalances) rebalance(c, sh, frontier, vals);
    }
    if (sh.sharded && !sh.replicated && !sh.failed) publish_best(c, sh, nvars);
    c.out->Aux = {(double)c.levels, (double)sh.allreduces, (double)c.rebalances, (double)c.moved};
    sh.rethrow();
}

}  // namespace

// BranchAndBound.Solve, Models/Branch&Bound.cs:30-123
SimplexResult BranchAndBound::Solve(const LPProblem& problem, UpdatePivot updatePivot)
{
    BestObjective = -INFINITY; BestSolution.clear(); HasBest = false;
    SimplexResult out;
    struct Whole { double t0 = PhaseTimer::now(); ~Whole() { g_pt.total += PhaseTimer::now() - t0; } } whole;
    Ctx c; c.root = &problem; c.opt = opt; c.cb = updatePivot; c.out = &out;
    c.log("=== Branch & Bound Algorithm ===");
    const char* rootAlgo = has_ge_or_eq(problem) ? "Dual Simplex" : "Primal Simplex";     // :50
    c.log(std::string("Branch & Bound: Using ") + rootAlgo + " for the ROOT LP relaxation.");

    EngineOptions lopt = opt; lopt.dual_flags = opt.bnb_mode == 1 ? LPX_DUAL_REPAIRED : 0;
    lopt.quiet = true;                  // the root LP's Report text is not part of the B&B result (:99-122)
    LPSolver solver(lopt);
    SimplexResult rootRes;
    out.LpSolves = 1;
    try {
        if (opt.test_node_lp) {             // test seam: no device, no root tableau in the result
            NodeLP lp; cold_node(c, {}, lp);
            std::vector<NodeLP*> g{&lp};
            out.LpSolves = 0;
            solve_group(c, g, problem.NumVars());
            if (lp.error) throw LpxException(LPX_EINVAL, "root relaxation failed");
            rootRes.HasSolution = lp.has_solution; rootRes.Solution = lp.x; rootRes.OptimalValue = lp.z;
        } else
        { const double t0 = PhaseTimer::now(); rootRes = solver.Solve(problem, rootAlgo, nullptr); g_pt.root += PhaseTimer::now() - t0; }   // :57
    } catch (const LpxException& ex) {
        if (ex.code == LPX_EDEVICE || ex.code == LPX_ENOMEM) throw;
        c.log(std::string("Root Problem: LP relaxation infeasible or error: ") + ex.what());
        out.Report = "LP relaxation infeasible"; out.Summary = "Error: Infeasible"; out.Status = LPX_INFEASIBLE;
        return out;                                                                       // :59-63
    }
    out.Stats.pivots += rootRes.Stats.pivots;
    if (!rootRes.HasSolution) {                                                           // :66-70
        c.log("Root Problem: Invalid Simplex result (missing Solution, Tableau, Basis, or VarNames).");
        out.Report = "Invalid Simplex result"; out.Summary = "Error: Invalid result"; out.Status = LPX_INFEASIBLE;
        return out;
    }
    std::vector<double> xRoot(rootRes.Solution.begin(), rootRes.Solution.begin() + std::min<size_t>(rootRes.Solution.size(), problem.NumVars()));
    const double zRoot = rootRes.OptimalValue;
    c.log("Root Problem LP solution: z* = " + FormatF(zRoot, 3));

    auto BuildReport = [&]() {                                                            // :99-122
        std::string sb = "Branch & Bound Finished.\n";
        if (!c.has_best) sb += "No integer-feasible solution found.\n";
        else {
            sb += "Best integer z* = " + FormatF(c.best, 3) + "\n";
            sb += "Best integer x* = [";
            for (size_t i = 0; i < c.best_x.size(); ++i) { if (i) sb += ", "; sb += FormatF(c.best_x[i], 3); }
            sb += "]\n";
        }
        out.Report = sb; out.Summary = sb;
        out.OptimalValue = c.has_best ? c.best : -INFINITY;
        out.Solution = c.best_x; out.HasSolution = true;
        out.Tableau = rootRes.Tableau; out.R = rootRes.R; out.C = rootRes.C;
        out.Basis = rootRes.Basis; out.VarNames = rootRes.VarNames;
        out.Status = c.has_best ? LPX_OPTIMAL : LPX_INFEASIBLE;
        BestObjective = out.OptimalValue; BestSolution = c.best_x; HasBest = c.has_best;
    };

    if (IsIntegral(xRoot) && IsFeasible(xRoot, problem, {})) {                                // :85-91
        set_incumbent(c, xRoot, zRoot);
        c.log("Root Problem is already integral and feasible. Branch & Bound not required.");
        BuildReport();
        return out;
    }
    c.log("Root solution is fractional -> starting Branch & Bound.");
    if (opt.bnb_search == 0) {
        std::vector<Cut> cuts;
        SolveNode(c, cuts, 0, "Root Problem");                                            // :95 (root solved a second time)
    } else if (opt.bnb_search == 2 && !opt.test_node_lp && opt.bnb_mode == 1) {
        WarmNodes warm; level_search(c, warm);
    } else {
        ColdNodes cold; level_search(c, cold);
    }
    BuildReport();
    return out;
}

}}  // namespace lpx::host
