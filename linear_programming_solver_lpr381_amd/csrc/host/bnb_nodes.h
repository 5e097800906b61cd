// host/bnb_nodes.h -- private to bnb.cpp (the searches) and bnb_nodes.cpp (a node's LP: prepared, solved in groups, tested).
#pragma once
#include "model.h"

#include <chrono>
#include <map>
#include <string>
#include <vector>

namespace lpx { namespace host { namespace bnb {

constexpr double EPS = 1e-6;      // Models/Branch&Bound.cs:24

struct Cut { int var; Rel rel; double bound; };

// LPX_BNB_TIMING=1: print where the host spends its time (diagnostic)
struct PhaseTimer {
    double build = 0, run = 0, collect = 0, decide = 0, root = 0, total = 0, readback = 0, parking = 0; bool on = false;
    double drained = 0, drained_at = 0, drained_max = 0; int drains = 0;   // rolling batches: time with no window enqueued (the device idles once it has drained)
    PhaseTimer();
    ~PhaseTimer();
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};
extern PhaseTimer g_pt;

std::string last_error();

// pool of device tableaux keyed by shape: nodes of one depth share a shape (handles outlive the solve in a process-wide cache)
struct HandlePool {
    std::map<std::pair<int, int>, std::vector<lpx_tableau*>> free_;
    std::vector<lpx_tableau*> all_;
    std::map<lpx_tableau*, std::pair<int, int>> cap_;
    lpx_tableau* get(int R, int C);
    void put(lpx_tableau* t) { free_[cap_[t]].push_back(t); }
    ~HandlePool();
};

struct NodeLP {
    // result of one relaxation
    bool error = false, has_solution = false;
    int status = LPX_OPTIMAL;
    std::vector<double> x; double z = 0.0;
    int64_t pivots = 0;
    // prepared tableau (host path: test seam) or branching-row descriptors (device assembly)
    std::vector<double> T; int R = 0, C = 0; std::vector<int32_t> basis; bool dual = false;
    bool on_device = false; std::vector<int32_t> cvar; std::vector<double> ccoef, czero, crhs;
    lpx_tableau* h = nullptr;
    // warm start: child of a parent whose final tableau is parked in a store slot
    lpx_store* pstore = nullptr; int pslot = -1; int prow = -1; bool warm = false; bool keep = false;   // keep: park the result
    lpx_store* kstore = nullptr; int kslot = -1; std::vector<int32_t> basis_out;
    double wbound = 0.0; bool wis_ge = false; int wslot = 0; int depth = 0;
    int feas = -1;          // IsFeasible(x) of :175-179 when it has been evaluated ahead of decide() (precompute_feas): 0 / 1
    const std::vector<Cut>* cuts_for_feas = nullptr;   // the node's branching rows, when solve_group may evaluate `feas` itself
};

// index of the root constraints for the per-node feasibility test (IsFeasibleIndexed)
struct FeasIndex {
    bool built = false; int n = 0;
    std::vector<int> dense_rows; std::vector<double> ATd;          // [n][dense_rows.size()]
    struct Sparse { int row; std::vector<std::pair<int, double>> nz; };
    std::vector<Sparse> sparse;
    void build(const LPProblem& root);
};

struct Ctx {
    FeasIndex feas;
    const LPProblem* root; EngineOptions opt; UpdatePivot cb;
    double best = -INFINITY; bool has_best = false; std::vector<double> best_x;
    SimplexResult* out; HandlePool pool; bool stop = false;
    bool count_work = true;      // false while this rank only mirrors the replicated warm-up of rank 0
    // Node budget of the sharded searches.  It is evaluated IDENTICALLY on every rank while the warm-up is replicated
    // (budget_used counts every rank's copy of the same nodes), so all ranks leave that phase together; at the hand-out
    // what is left of the GLOBAL budget (opt.max_nodes) is split evenly and each rank then counts its own nodes.
    int64_t budget_used = 0, budget_cap = 0;
    bool over_budget() const { return budget_cap > 0 && budget_used >= budget_cap; }
    // DFS-order key of the incumbent's node: one bit per branching level, 0 = the ceil child the reference visits first
    // (Models/Branch&Bound.cs:256), 1 = the floor child.  Lexicographically smaller == earlier in the reference's DFS.
    std::vector<uint8_t> best_key; bool tie_by_key = false;
    // statistics of the sharded search (SimplexResult::Aux, with Sharded::allreduces)
    int64_t levels = 0, rebalances = 0, moved = 0;
    std::map<std::pair<int, int>, lpx_store*> stores;
    lpx_store* store_for(lpx_tableau* h);
    // resident root templates: the prepared root tableau as the primal / dual path builds it
    lpx_tableau* root_tpl[2] = {nullptr, nullptr}; int tplR[2] = {0, 0}, tplC[2] = {0, 0}; bool tpl_bad[2] = {false, false};
    ~Ctx();
    void log(const std::string& s) { if (cb) cb(s + "\n", nullptr); }
};

bool has_ge_or_eq(const LPProblem& p);                             // ChooseAlgorithm, :262-266
bool IsIntegral(const std::vector<double>& x);                     // :268-274
bool IsFeasible(const std::vector<double>& x, const LPProblem& root, const std::vector<Cut>& cuts);                        // :276-294
bool IsFeasibleIndexed(const std::vector<double>& x, const LPProblem& root, const std::vector<Cut>& cuts, FeasIndex& ix);  // same verdicts

// a cold node's LP as the reference prepares it: on the host (test seam) or as branching rows for the device to add to the
// resident root template (ensure_template: false when the root part itself throws in the reference)
bool ensure_template(Ctx& c, bool dual);
void cold_node(Ctx& c, const std::vector<Cut>& cuts, NodeLP& lp);

// solves the relaxations of `group`, opt.concurrent_nodes at a time
void solve_group(Ctx& c, std::vector<NodeLP*>& group, int nvars);

}}}  // namespace lpx::host::bnb
