// host/model.h -- C++ mirror of the reference's plugin boundary: data model, ILPAlgorithm,
// LPSolver (Models/PrimalSimplex.cs:8-49, Models/IPLAlgorithm.cs:5-8, Models/LPSolver.cs:16-76).
// Same names, argument meaning and error behaviour as the C# so that tests read like tests of the
// reference; the loops themselves run on the GPU through the C ABI (include/lpx.h).
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/lpx.h"

namespace lpx { namespace host {

enum class Sense { Max, Min };          // Models/PrimalSimplex.cs:8
enum class Rel { LE, GE, EQ };          // Models/PrimalSimplex.cs:9

struct Constraint {                     // Models/PrimalSimplex.cs:11-18
    std::vector<double> A;
    Rel Relation = Rel::LE;
    double B = 0.0;
};

struct LPProblem {                      // Models/PrimalSimplex.cs:20-36
    Sense ObjectiveSense = Sense::Max;
    std::vector<double> C;
    std::vector<Constraint> Constraints;
    int NumVars() const { return (int)C.size(); }
    LPProblem Clone() const { return *this; }
};

// bool[,] highlight of the reference callback: row-major R x C flags (empty = null)
struct Highlight { int R = 0, C = 0; std::vector<uint8_t> cells; };
// Action<string, bool[,]> updatePivot (Models/IPLAlgorithm.cs:7)
using UpdatePivot = std::function<void(const std::string& text, const Highlight* highlight)>;

struct SimplexResult {                  // Models/PrimalSimplex.cs:38-49
    std::string Report, Summary;
    double OptimalValue = 0.0;
    bool HasSolution = false;           // false == Solution/Tableau/Basis/VarNames are null (defect D2)
    std::vector<double> Solution;
    std::vector<double> Tableau; int R = 0, C = 0;      // row-major R x C
    std::vector<int32_t> Basis;
    std::vector<std::string> VarNames;
    // additions of this engine (not in the reference record)
    int Status = LPX_OPTIMAL;           // LPX_OPTIMAL / LPX_UNBOUNDED / LPX_INFEASIBLE
    std::vector<int32_t> Trace;         // (leaving row, entering column) per pivot
    lpx_stats Stats{};
    int64_t LpSolves = 0, Nodes = 0;    // branch-and-bound counters
    std::vector<int32_t> NodeLog;       // B&B: (depth, outcome, branching var) per visited node
    std::vector<double> NodeZ;
    std::vector<double> Cuts;           // cutting plane: (A[0..n), B) per cut, in the order added
    std::vector<double> Aux;            // sharded B&B: {levels, all-reduces, rebalancing rounds, node descriptors moved}
};

// The reference throws System.Exception with fixed messages; `code` is the LPX_E_* of include/lpx.h.
struct LpxException : std::runtime_error {
    int code;
    LpxException(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

struct ILPAlgorithm {                   // Models/IPLAlgorithm.cs:5-8
    virtual ~ILPAlgorithm() = default;
    virtual SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) = 0;
};

// Engine knobs that have no counterpart in the reference (all default to reference behaviour).
struct EngineOptions {
    bool render_iterations = false;  // true: format the whole tableau for every pivot callback as the
                                     // reference does (Models/PrimalSimplex.cs:113-121); needs one
                                     // download per pivot.  false: callbacks get one line per pivot.
    int batch = 0;                   // pivots per host poll (0 = library default)
    int dual_flags = 0;              // 0 faithful (D1/D2 kept); LPX_DUAL_REPAIRED = repaired
    int bnb_mode = 0;                // 0 faithful, 1 repaired
    int bnb_search = 0;              // 0 = reference DFS (ceil first), 1 = level-synchronous sharded
    int64_t max_nodes = 0;           // 0 = unlimited; sharded searches: budget of the WHOLE job (split over the ranks)
    int concurrent_nodes = 1;        // level-synchronous search: node LPs in flight per GPU
    int rank = 0, world = 1;         // level-synchronous search: shard of this process
    // incumbent exchange: called once per level with {best_z, have_work}; must return the MAX over
    // ranks in place (RCCL all-reduce in production, identity for one process).
    std::function<void(double* vals, int count)> allreduce_max;
    bool shard_one = false;          // diagnostic (LPX_COMM_SHARD_ONE): run the sharded code path with world == 1
    int max_iter = 10000;
    int bnb_dive = 0;                // sharded searches: 1 = depth-first-K pool policy
    bool quiet = false;              // internal solves whose Report nobody reads (B&B nodes): skip the canonical-form text,
                                     // hundreds of thousands of formatted numbers for a config-4 model
    // lpx_solve_ranging: called by the primal / dual mirrors with the solve's device tableau and final status after the loop,
    // before the handle goes back to the cache (the tableau has been downloaded already; the hook must not modify it)
    std::function<void(::lpx_tableau* t, int status)> on_final_tableau;
    // test seams (see include/lpx_test.h); never set by product code
    int64_t test_fail_after_nodes = 0;
    std::function<int(double* T, int R, int C, int32_t* basis, int dual, int repaired, int max_iter, int nvars,
                      double* x, double* z, int64_t* pivots)> test_node_lp;
    std::function<int(int count, const int32_t* off, const int32_t* fidx, const int8_t* fval, double* profit,
                      double* weight, int32_t* frac, double* fracval)> test_knap_relax;
};

enum { LPX_DUAL_FIX_D1 = 1, LPX_DUAL_FIX_D2 = 2, LPX_DUAL_SOUND = 4, LPX_DUAL_REPAIRED = 7 };

class PrimalSimplex : public ILPAlgorithm {             // Models/PrimalSimplex.cs:52-305
public:
    explicit PrimalSimplex(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& original, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class DualSimplex : public ILPAlgorithm {               // Models/DualSimplex.cs:11-313
public:
    explicit DualSimplex(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& original, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class RevisedPrimalSimplex : public ILPAlgorithm {      // Models/RevisedPrimalSimplex.cs:12-458
public:
    explicit RevisedPrimalSimplex(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& original, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class BranchAndBound : public ILPAlgorithm {            // Models/Branch&Bound.cs:20-304
public:
    explicit BranchAndBound(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
    double BestObjective = -1.0 / 0.0;
    std::vector<double> BestSolution; bool HasBest = false;
private:
    EngineOptions opt;
};

class BranchAndBoundRevised : public ILPAlgorithm {     // Models/BranchAndBoundRevised.cs:17-390
public:
    explicit BranchAndBoundRevised(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class BranchAndBoundKnapsack : public ILPAlgorithm {    // Models/BranchAndBoundKnapsack.cs:12-548
public:
    explicit BranchAndBoundKnapsack(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class CuttingPlane : public ILPAlgorithm {              // Models/CuttingPlane.cs:9-164
public:
    explicit CuttingPlane(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

class CuttingPlaneRevised : public ILPAlgorithm {       // Models/CuttingPlaneRevised.cs:9-112
public:
    explicit CuttingPlaneRevised(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt;
};

// GMI cutting-plane loop on the device (not in the reference; lpx_solve_cuts in include/lpx.h defines it): the root LP and
// every re-optimisation run on one handle with capacity for max_active cut rows, the cut rounds are lpx_tableau_gmi_round.
class GmiCuttingPlane : public ILPAlgorithm {
public:
    GmiCuttingPlane(const EngineOptions& o, const lpx_cut_opts& co) : opt(o), cut(co) {}
    explicit GmiCuttingPlane(const EngineOptions& o = {}) : opt(o) { lpx_default_cut_opts(&cut); }
    SimplexResult Solve(const LPProblem& problem, UpdatePivot updatePivot = nullptr) override;
private:
    EngineOptions opt; lpx_cut_opts cut;
};

// Models/SensitivityAnalysis.cs:11-297.  `problem` is mutated by ApplyChange, as in the
// reference; `result` must carry Tableau/Basis/VarNames (the constructor checks, :24-43).
class SensitivityAnalysis {
public:
    SensitivityAnalysis(LPProblem* problem, const SimplexResult* result, const EngineOptions& o = {});
    std::string GetRangeReport(const std::string& target) const;          // :47-76
    std::string ApplyChange(const std::string& target, double value);     // :78-107
    std::string GetShadowPricesReport() const;                            // :109-128
    SimplexResult SolveUsingDuality() const;                              // :130-219
    std::pair<double, double> Range(const std::string& target) const;     // GetRangeReport's numbers
    void Locate(const std::string& target, int* field, int* index) const;  // entry ApplyChange assigns
    std::pair<double, double> GetConstraintRange(int index) const;                    // :277-298
    std::pair<double, double> GetBasicVariableObjectiveRange(int basicVarRow) const;  // :250-275
    std::pair<double, double> GetNonBasicVariableRange(const std::string& varName) const;   // :229-248
private:
    bool basis_contains(int col) const;
    int constraint_index(const std::string& target) const;
    int var_column(const std::string& target) const;
    LPProblem* problem; const SimplexResult* result; EngineOptions opt;
};

class LPSolver {                                        // Models/LPSolver.cs:6-77
public:
    explicit LPSolver(const EngineOptions& o = {}) : opt(o) {}
    SimplexResult Solve(const LPProblem& problem, const std::string& algorithm, UpdatePivot updatePivot = nullptr);
    static std::string NormalizeAlgorithmKey(const std::string& algorithm);   // :61-76
    std::vector<double> FinalTableau; int FinalR = 0, FinalC = 0; bool HasFinalTableau = false;   // :11
private:
    EngineOptions opt;
};

// a failed call of the C ABI as the exception of the model level: LpxException(rc, "liblpx: " + the library's last error) (solvers.cpp)
[[noreturn]] void throw_lib(int rc);

// Bounded-variable primal simplex at the model level (lpx_solve_bounded, include/lpx.h; bounded.cpp): lower / upper are empty
// (0 / +inf) or hold one entry per variable.
struct BoundedInfo { std::vector<uint8_t> flip; std::vector<double> ub, lower; };
// the (lower, upper) pair of the variable called `var` ("x3"): lower finite, upper >= lower; LpxException(LPX_EINVAL) otherwise
void CheckVarBounds(const std::string& var, double lower, double upper);
// A bounded session (lpx_bounded_open): the handle SolveBounded solved on, kept with what turns its tableau back into the
// user's terms.  The destructor hands the handle back.
struct BoundedSession {
    ::lpx_tableau* h = nullptr; int R = 0, C = 0, n = 0;
    bool min = false, shifted = false; double constant = 0.0;      // objective sense, and the constant c.l of open's shift
    std::vector<double> lower;                                      // open's lower bounds (empty = none): the host-side shift
    int open_status = -1; EngineOptions opt; std::vector<std::string> varNames;
    int spare = 0;                                                  // rows and columns of capacity beyond R x C (SolveBounded's max_spare)
    std::vector<double> T0;                                         // with max_spare > 0: the prepared tableau [R * C], for the slack flags of the cut rounds
    BoundedSession() = default;
    BoundedSession(const BoundedSession&) = delete;
    ~BoundedSession();
};
SimplexResult SolveBounded(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                           const EngineOptions& opt, UpdatePivot updatePivot, BoundedInfo* info, BoundedSession* keep = nullptr,
                           int form = -1,              // lpx_solve_bounded2: LPX_NODE_* of the loop (lpx_bounded_run2); -1: lpx_bounded_run
                           int max_spare = 0);         // with keep: the handle gets the largest a <= max_spare spare rows and columns for which
                                                       // (R + a, C + a) still satisfies lpx_bounded_node_fits (keep->spare = a)
// count independent models in ONE lpx_node_batch_primal launch (lpx_solve_bounded_batch); an error names its model ("model i: ")
void SolveBoundedBatch(const std::vector<const LPProblem*>& problems, const std::vector<std::vector<double>>& lowers,
                       const std::vector<std::vector<double>>& uppers, const EngineOptions& opt, std::vector<SimplexResult>& results,
                       std::vector<BoundedInfo>& infos);
// the argument checks of lpx_solve_packed (LPX_EINVAL, no device, no look at any model); the call itself is lpx::packed_solve
void CheckPacked(const lpx_packed_models* in, const lpx_run_opts* o, const lpx_packed_results* out);
// the argument checks of lpx_solve_packed_dual, the same way; the call itself is lpx::packed_dual_solve
void CheckPackedDual(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* out);
// the argument checks of lpx_packed_base_open (h: where the handle goes) and lpx_packed_base_solve (h: the handle, m and n its
// shape), the same way; the calls themselves are lpx::packed_base_open and lpx::packed_base_solve
void CheckPackedBaseOpen(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o, const lpx_packed_dual_results* base_out,
                         const void* h);
void CheckPackedBaseSolve(const void* h, int m, int n, int32_t count, const double* b, int flags, const lpx_run_opts* o,
                          const lpx_packed_dual_results* out);
// the argument checks of lpx_packed_base_solve_costs, the same way (b may be NULL); the call itself is lpx::packed_base_solve_costs
void CheckPackedBaseSolveCosts(const void* h, int m, int n, int32_t count, const double* c, const double* b, int flags,
                               const lpx_run_opts* o_primal, const lpx_run_opts* o_dual, const lpx_packed_cost_results* out);
// the argument checks of lpx_solve_packed_bnb, the same way; work_bytes is lpx::packed_bnb_work_bytes; the call itself is lpx::packed_bnb_solve
void CheckPackedBnb(const lpx_packed_bnb_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                    size_t (*work_bytes)(int count, int m, int n, int max_depth));
// the argument checks of lpx_solve_packed_bnb_dual, the same way (rel among them); the call itself is lpx::packed_bnb_dual_solve
void CheckPackedBnbDual(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                        size_t (*work_bytes)(int count, int m, int n, int max_depth));
// The dual start (lpx_solve_bounded_dual): >= rows and negative right-hand sides accepted, slack basis, dualize, lpx_bounded_dual_run3(flags)
SimplexResult SolveBoundedDual(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper, int flags,
                               const EngineOptions& opt, UpdatePivot updatePivot, BoundedInfo* info,
                               BoundedSession* keep = nullptr);     // the handle kept as SolveBounded keeps it (no spare)
// new absolute bounds of user variables vars[k] on a session: lpx_tableau_change_bounds + lpx_bounded_dual_run (lpx_bounded_set_bounds)
SimplexResult BoundedSetBounds(BoundedSession& s, int K, const int32_t* vars, const double* lower, const double* upper);

// Branch and bound by bound changes on the root's handle (lpx_solve_bnb_bounded, host/bnb_bounded.cpp).  limit_rc: 0, or
// LPX_ITER_LIMIT with limit_msg when a node reached max_iter or the search reached max_nodes (the result holds the incumbent so far).
struct BnbBoundedInfo {
    int64_t nodes = 0, events = 0, flips = 0, incumbents = 0, pruned_bound = 0, pruned_infeasible = 0, max_K = 0;
    double constant = 0.0;
    std::vector<lpx_bnb_node_log> log;
    int limit_rc = 0; std::string limit_msg;
};
SimplexResult SolveBnbBounded(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                              const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                              int search_flags = 0,       // lpx_solve_bnb_bounded2: LPX_BDUAL_LONG_STEP / LPX_BDUAL_CUTOFF on every node
                              int node_form = -1);        // lpx_solve_bnb_bounded3: LPX_NODE_* of every node call; -1: the calls of _bounded / _bounded2
// lpx_solve_bnb_bounded_dual: the same search behind the root of SolveBoundedDual (>= rows, right-hand sides of either sign)
SimplexResult SolveBnbBoundedDual(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                                  const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                                  int search_flags, int node_form);
// The search by W divers (lpx_solve_bnb_bounded4): every node on chip, one lpx_node_batch_run per round.
struct BnbDiversInfo { int64_t rounds = 0, steals = 0, largest_batch = 0; std::vector<int32_t> round, diver; };
// Strong branching (lpx_solve_bnb_bounded6 with LPX_BRANCH_STRONG): SolveBnbDivers whose round is ONE lpx_node_batch_run_probe and
// whose decide step chooses the variable, and drops the dead children, by the probes of up to cand_max candidates.
struct BnbStrong { int cand_max = 4, probe_iter = 0; };
// The stall guard (lpx_solve_bnb_bounded7): nodes with a pivot in Bland mode, those pivots, the most events of one node.
struct BnbGuardInfo { int64_t guarded_nodes = 0, bland_events = 0, max_events = 0; };
// The cut loop at the root (lpx_solve_bnb_bounded9): the loop's record; ran = 0 with spare = 0 (no capacity that keeps the nodes on chip).
struct BnbCutInfo { int ran = 0, spare = 0, rounds = 0, added = 0, purged = 0, stop = 0, status = 0, R = 0, C = 0; int64_t events = 0;
                    std::vector<double> z_before, z_after; };
// Reduced-cost tightening (lpx_solve_bnb_bounded10): nodes that tightened a column, the columns, the most of one node.
struct BnbFixInfo { int64_t tightened_nodes = 0, tightened_cols = 0, max_per_node = 0; };
struct BnbStrongInfo { int64_t probe_launches = 0, probes = 0, probe_events = 0, probe_limit = 0, pruned_by_probe = 0, changed_picks = 0; };
SimplexResult SolveBnbDivers(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                             const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                             int search_flags, int divers, BnbDiversInfo& dinfo, const struct BnbStrong* strong = nullptr,
                             struct BnbStrongInfo* sinfo = nullptr,
                             int stall_events = -1,       // lpx_solve_bnb_bounded7: >= 0, the round is ONE lpx_node_batch_run2 (never with strong)
                             struct BnbGuardInfo* ginfo = nullptr,
                             int root_form = -1,          // lpx_solve_bnb_bounded8: LPX_NODE_* of the root solve; -1: lpx_bounded_run
                             const lpx_cut_opts* root_cuts = nullptr,     // lpx_solve_bnb_bounded9: lpx_bounded_cut_loop at the root, the divers start from its handle
                             struct BnbCutInfo* cinfo = nullptr,
                             int tighten = 0,             // lpx_solve_bnb_bounded10: 1, the round is ONE lpx_node_batch_run3 (never with strong)
                             struct BnbFixInfo* finfo = nullptr);
// The search by W divers that plunge (lpx_solve_bnb_bounded5): one lpx_node_batch_plunge per round, up to `plunge` nodes per diver.
struct BnbPlungeInfo { int64_t launched = 0, dropped = 0, longest_chain = 0; std::vector<int32_t> step; };
SimplexResult SolveBnbPlunge(const LPProblem& original, const std::vector<double>& lower, const std::vector<double>& upper,
                             const std::vector<uint8_t>& is_int, const EngineOptions& opt, int64_t max_nodes, BnbBoundedInfo& info,
                             int search_flags, int divers, int plunge, BnbDiversInfo& dinfo, BnbPlungeInfo& pinfo);

// LPParser.ParseFromText, Models/LPParser.cs:9-79.  Throws LpxException(LPX_E_PARSE, message).
LPProblem ParseFromText(const std::string& input);

// Text formats of the reference (Models/PrimalSimplex.cs:259-304 and friends), see format.cpp
std::string FormatNumber(double v);                 // ToString("0.###")
std::string FormatF(double v, int decimals);        // ToString("F3"/"F6", InvariantCulture)
std::string FormatRound3(double v);                 // $"{Math.Round(v, 3):0.###}"
std::string FormatShortest(double v);               // double.ToString(): shortest round-trippable digits
double RoundHalfEven(double v, int decimals);       // Math.Round(v, decimals)
std::string AppendTableau(const std::string& title, const double* T, int R, int C,
                          const std::vector<int32_t>& basis, const std::vector<std::string>& varNames, int iter);
std::string AppendCanonicalForm(const LPProblem& model);
std::string MatrixToString(const double* M, int r, int c);
std::string BuildIterationBlock(int iter, const std::vector<int32_t>& Bidx, const std::vector<int32_t>& Nidx,
                                const std::vector<std::string>& names, const double* Binv, int m,
                                const std::vector<double>& xB, double z, const std::vector<double>* rN,
                                int entering, const std::vector<double>* d, double bestTheta, double eps);

// helpers shared by the solver mirrors (solvers.cpp)
// FinalizeReport, Models/PrimalSimplex.cs:130-159: status line, x, z* appended to the report and the summary
void FinalizeText(std::string& report, std::string& summary, const std::vector<double>& x, double z, int status);
void BuildTableauPrimal(const LPProblem& expanded, std::vector<double>& T, int& R, int& C,
                        std::vector<int32_t>& basis, std::vector<std::string>& varNames);
LPProblem ExpandEqualitiesToInequalities(const LPProblem& model);
LPProblem PrepareForTableauDual(const LPProblem& original, bool fix_d1);
// Expanded rows of the tableau PrimalSimplex (dual = false) / DualSimplex builds from `original`: row k comes from constraint
// row_of[k], multiplied by sign[k] (+1 / -1) -- the sign preparation actually applied, defect D1 included (fix_d1 = false).
void PreparedRows(const LPProblem& original, bool dual, bool fix_d1, std::vector<int>& row_of, std::vector<int>& sign);

// Handles of whole-model solves and of the B&B root templates, kept from one solve to the next (creating a handle costs ~4 ms of device
// and pinned allocations, destroying it ~3 ms: two root solves and two templates were 25-30 ms of every search).  Exact shapes only --
// these handles are never rebuilt to another size -- small tableaux only (<= 32 MB), a bounded number; everything else is created and
// destroyed as before.  acquire: a cached handle of that shape or a new one (throws LpxException); release: back to the cache or destroyed.
::lpx_tableau* acquire_exact_handle(int R, int C);
void release_exact_handle(::lpx_tableau* t, int R, int C);

// Ranging of a solved device tableau in user terms (lpx_solve_ranging, lpx_session_ranging).  Prepared row k comes from constraint
// row_of[k] with sign[k] and owns slack column slack_col[k]; user variable j is tableau column var_col[j].
struct RangingMap {
    const LPProblem* q = nullptr;
    std::vector<int> row_of, sign, slack_col, var_col;
};
struct RawRanging {                     // lpx_tableau_ranging / _pairs of the final tableau, its basis and objective row
    std::vector<double> ci, cd, ri, rd, dj, pi, pd;
    std::vector<int32_t> cia, cda, ria, rda, basis, pia, pda, pa, pb;
    std::vector<int> pair_of;
    double min_rhs = 1.0 / 0.0, min_dj = 1.0 / 0.0;
};
void RangingAlloc(lpx_ranging* rg, int n, int m);                  // every array NaN / -1, valid = 0
void RangeTableau(::lpx_tableau* t, const RangingMap& map, RawRanging& raw);
void RangingToUser(const RangingMap& map, const RawRanging& raw, int status, lpx_ranging* rg);

}
}  // namespace lpx::host
