// lpx_cli -- Linux stand-in for the reference's WinForms host (Form1.cs), over the C ABI of liblpx.so only.
//
//   lpx_cli [--algorithm NAME] [--repaired] [--iterations] [--ranging] [--cuts-per-round K] [--cut-rounds N]
//           [--set-rhs I=V]... [--set-cost J=V]... [--upper J=V]... [--lower J=V]... [--binary] [--bnb-bounded [--long-step] [--cutoff] [--node-form F] [--divers W] [--plunge D] [--branching R [--candidates N] [--probe-iter L]] [--stall-events S] [--root-form F] [--root-cuts N [--cuts-per-round K]] [--tighten]] [--bounded-form F] [--bounded [--rhs-file F]] [--bounded-dual [--long-step] --rhs-file F] [--binary --bnb-bounded [--long-step] [--cutoff] --rhs-file F] [--bnb-bounded --dual-root [--long-step] [--cutoff] [--node-form F | --rhs-file F]] [--export FILE] INPUT.txt
//
// Does what Form1 does around the solvers: reads the model text (Import, Form1.cs:284-296), parses it with the LPParser
// grammar (lpx_parse_text, Models/LPParser.cs:9-79), runs the algorithm chosen by its dropdown name (btnSolve_Click,
// Form1.cs:231-279), shows the iteration text followed by "Final Report:" and "Summary:" (:277-278), and can write the
// export file layout of BtnExport_Click (:308-315).  C only touches include/lpx.h: this is also the link test of the
// boundary from a compiled host.  --ranging (Primal / Dual Simplex) solves through lpx_solve_ranging and prints the ranging
// report of the final tableau after the summary.  --cuts-per-round / --cut-rounds (GMI Cutting Plane) solve through
// lpx_solve_cuts with those options.  --set-rhs I=V (b_I = V) and --set-cost J=V (c_J = V), 1-based and repeatable, are
// applied in the order given after the solve, each as a warm edit of one lpx_session (re-optimised on the device from the
// previous basis), and each re-solve's summary is printed.  --upper J=V / --lower J=V (bounds of x_J, 1-based, repeatable) and
// --binary (every u_j = 1) select the bounded-variable primal simplex (lpx_solve_bounded): the bounds cost no rows.  --bounded selects it without any bound.  --bounded --rhs-file F solves the model once per line of F (m numbers, the
// right-hand sides of that run) as ONE packed call (lpx_solve_packed) with c, A and the bounds shared by every run, and prints one
// line "status value x1 .. xn" per right-hand side.  --bounded-dual [--long-step] --rhs-file F does the same by the dual start
// (lpx_solve_packed_dual): >= rows and negative right-hand sides are accepted, an = row is refused; with --warm-base the input's own
// right-hand side is solved once and every line continues from that base (lpx_packed_base_open / _solve); --cost-file F [--rhs-file G] beside
// --warm-base re-solves a cost vector per line of F (with G: and the right-hand side of the same line) from that base (lpx_packed_base_solve_costs).  --bnb-bounded --rhs-file F (with
// --binary or --upper bounds, and --long-step / --cutoff) solves the model as an integer program once per line of F as ONE packed
// call (lpx_solve_packed_bnb): a whole branch and bound per right-hand side in one kernel launch, the same line per run.
// --bnb-bounded --dual-root runs the search from a dual start (lpx_solve_bnb_bounded_dual; with --rhs-file F lpx_solve_packed_bnb_dual):
// >= rows and negative right-hand sides are accepted, an = row is refused under --rhs-file.  There is no CPU fallback: without a gfx950 device the solve fails with LPX_EDEVICE.
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/lpx.h"

static std::string g_iterations;
static void on_text(void*, const char* text, const uint8_t*, int, int) { g_iterations += text; }

// Column names as BuildTableau gives them (x1..xn, then c1.. for the slacks); -1 = none.
static std::string col_name(int j, int n) { return j < 0 ? "-" : (j < n ? "x" : "c") + std::to_string(j < n ? j + 1 : j - n + 1); }

static std::string ranging_table(const lpx_ranging& g)
{
    std::string s = "\n\nRanging:\n";
    if (!g.valid) {
        char b[160];
        std::snprintf(b, sizeof b, "  not available: the final tableau is not optimal and feasible (min rhs %.17g, min d_j %.17g)\n", g.min_rhs, g.min_dj);
        return s + b;
    }
    char b[256];
    std::snprintf(b, sizeof b, "  %-8s %24s %24s %8s %8s %24s\n", "variable", "cost low", "cost high", "enters", "enters", "reduced cost");
    s += b;
    for (int j = 0; j < g.n; ++j) {
        std::snprintf(b, sizeof b, "  %-8s %24.17g %24.17g %8s %8s %24.17g\n", col_name(j, g.n).c_str(), g.cost_lo[j], g.cost_hi[j],
                      col_name(g.cost_lo_at[j], g.n).c_str(), col_name(g.cost_hi_at[j], g.n).c_str(), g.reduced_cost[j]);
        s += b;
    }
    std::snprintf(b, sizeof b, "  %-8s %24s %24s %8s %8s %24s\n", "row", "rhs low", "rhs high", "leaves", "leaves", "dual");
    s += b;
    for (int i = 0; i < g.m; ++i) {
        std::snprintf(b, sizeof b, "  %-8s %24.17g %24.17g %8s %8s %24.17g\n", ("b" + std::to_string(i + 1)).c_str(), g.rhs_lo[i], g.rhs_hi[i],
                      col_name(g.rhs_lo_at[i], g.n).c_str(), col_name(g.rhs_hi_at[i], g.n).c_str(), g.dual[i]);
        s += b;
    }
    return s;
}

// The key lpx_solve matches algorithm names by (LPSolver.NormalizeAlgorithmKey, Models/LPSolver.cs:61-76): lower case, every
// "algorithm" removed, runs of white space collapsed to one blank, none at either end.
static std::string algorithm_key(const std::string& name)
{
    std::string low;
    for (char ch : name) low += (char)std::tolower((unsigned char)ch);
    for (size_t p; (p = low.find("algorithm")) != std::string::npos;) low.erase(p, 9);
    std::string key; bool sp = false;
    for (char ch : low) {
        if (std::isspace((unsigned char)ch)) { sp = true; continue; }
        if (sp && !key.empty()) key += ' ';
        sp = false; key += ch;
    }
    return key;
}

// the lines of a scenario file (--cost-file, --rhs-file beside it): `width` numbers per line, blank lines skipped.  0, or the exit
// code behind a message
static int read_rows(const std::string& path, const char* option, int width, std::vector<double>& out, int& count)
{
    std::ifstream rf(path);
    if (!rf) { std::fprintf(stderr, "Error reading file: %s\n", path.c_str()); return 66; }
    std::string line;
    count = 0;
    while (std::getline(rf, line)) {
        std::istringstream ls(line);
        std::vector<double> row; double v;
        while (ls >> v) row.push_back(v);
        if (row.empty() && ls.eof()) continue;          // a blank line
        if ((int)row.size() != width || !ls.eof()) {
            std::fprintf(stderr, "lpx_cli: %s: line %d does not hold %d numbers\n", option, count + 1, width);
            return 65;
        }
        out.insert(out.end(), row.begin(), row.end()); ++count;
    }
    return 0;
}

int main(int argc, char** argv)
{
    std::string algorithm = "Primal Simplex", input, exportPath;
    bool repaired = false, iterations = false, ranging = false, cut_set = false, algo_set = false, binary = false, bnb_bounded = false;
    bool bounded_flag = false;  // --bounded: the bounded primal simplex even without a bound
    std::string rhs_file;       // --rhs-file F beside --bounded: one packed call (lpx_solve_packed), a right-hand side per line of F
    bool dual_root = false;     // --dual-root beside --bnb-bounded: the search from a dual start (lpx_solve_bnb_bounded_dual; with --rhs-file lpx_solve_packed_bnb_dual)
    bool bounded_dual = false;  // --bounded-dual beside --rhs-file: that packed call by the dual start (lpx_solve_packed_dual)
    std::string cost_file;      // --cost-file F beside --bounded-dual --warm-base: a cost vector per line of F, every line re-solved from the base (lpx_packed_base_solve_costs); with --rhs-file G line k of F goes with line k of G
    bool warm_base = false;     // --warm-base beside --bounded-dual --rhs-file: the input's own right-hand side solved once, every line of F from that base (lpx_packed_base_open / _solve)
    int search_flags = 0;       // --long-step / --cutoff beside --bnb-bounded
    int node_form = -1;         // --node-form beside --bnb-bounded: LPX_NODE_*; -1 = not given
    int divers = 0;             // --divers W beside --bnb-bounded: the search by W divers (lpx_solve_bnb_bounded4); 0 = not given
    int plunge = 0;             // --plunge D beside --bnb-bounded: up to D nodes per diver and launch (lpx_solve_bnb_bounded5); 0 = not given
    int branching = -1;         // --branching R beside --bnb-bounded: LPX_BRANCH_* (lpx_solve_bnb_bounded6); -1 = not given
    int candidates = 4;         // --candidates N: the columns probed per node by --branching strong
    int probe_iter = -1;        // --probe-iter L: the event limit of a probe; -1 = the node's
    int stall_events = -1;      // --stall-events S beside --bnb-bounded: the stall guard (lpx_solve_bnb_bounded7); -1 = not given
    int bounded_form = -1;      // --bounded-form F: LPX_NODE_* of the bounded primal solve (lpx_solve_bounded2); -1 = not given
    bool tighten = false;       // --tighten beside --bnb-bounded --divers: reduced-cost bound tightening at every node (lpx_solve_bnb_bounded10)
    int root_cuts = -1;         // --root-cuts N beside --bnb-bounded --divers: N rounds of GMI cuts at the root (lpx_solve_bnb_bounded9; K = --cuts-per-round); -1 = not given
    int root_form = -1;         // --root-form F beside --bnb-bounded --divers: LPX_NODE_* of the root solve (lpx_solve_bnb_bounded8); -1 = not given
    struct Bound { bool upper; int index; double value; std::string text; };
    std::vector<Bound> bounds;
    lpx_cut_opts co; lpx_default_cut_opts(&co);
    struct Edit { bool rhs; int index; double value; std::string text; };
    std::vector<Edit> edits;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--algorithm" && i + 1 < argc) { algorithm = argv[++i]; algo_set = true; }
        else if (a == "--binary") binary = true;
        else if (a == "--bnb-bounded") bnb_bounded = true;
        else if (a == "--bounded") bounded_flag = true;
        else if (a == "--bounded-dual") bounded_dual = true;
        else if (a == "--warm-base") warm_base = true;
        else if (a == "--dual-root") dual_root = true;
        else if (a == "--rhs-file" && i + 1 < argc) rhs_file = argv[++i];
        else if (a == "--cost-file" && i + 1 < argc) cost_file = argv[++i];
        else if (a == "--long-step") search_flags |= LPX_BDUAL_LONG_STEP;
        else if (a == "--cutoff") search_flags |= LPX_BDUAL_CUTOFF;
        else if (a == "--node-form" && i + 1 < argc) {
            const std::string v = argv[++i];
            node_form = v == "launches" ? LPX_NODE_LAUNCHES : v == "onchip" ? LPX_NODE_ONCHIP : v == "auto" ? LPX_NODE_AUTO : -2;
            if (node_form == -2) { std::fprintf(stderr, "lpx_cli: --node-form takes launches, onchip or auto, got '%s'\n", v.c_str()); return 64; }
        }
        else if ((a == "--bounded-form" || a == "--root-form") && i + 1 < argc) {
            const std::string v = argv[++i];
            const int f = v == "launches" ? LPX_NODE_LAUNCHES : v == "onchip" ? LPX_NODE_ONCHIP : v == "auto" ? LPX_NODE_AUTO : -2;
            if (f == -2) { std::fprintf(stderr, "lpx_cli: %s takes launches, onchip or auto, got '%s'\n", a.c_str(), v.c_str()); return 64; }
            (a == "--bounded-form" ? bounded_form : root_form) = f;
        }
        else if (a == "--divers" && i + 1 < argc) {
            const std::string v = argv[++i];
            char* end = nullptr;
            const long w = std::strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || w < 1 || w > 1024) { std::fprintf(stderr, "lpx_cli: --divers takes a count in [1, 1024], got '%s'\n", v.c_str()); return 64; }
            divers = (int)w;
        }
        else if (a == "--plunge" && i + 1 < argc) {
            const std::string v = argv[++i];
            char* end = nullptr;
            const long d = std::strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || d < 1 || d > 64) { std::fprintf(stderr, "lpx_cli: --plunge takes a depth in [1, 64], got '%s'\n", v.c_str()); return 64; }
            plunge = (int)d;
        }
        else if (a == "--stall-events" && i + 1 < argc) {
            const std::string v = argv[++i];
            char* end = nullptr;
            const long x = std::strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || x < 0 || x > 1000000000) { std::fprintf(stderr, "lpx_cli: --stall-events takes a non-negative pivot count, got '%s'\n", v.c_str()); return 64; }
            stall_events = (int)x;
        }
        else if (a == "--branching" && i + 1 < argc) {
            const std::string v = argv[++i];
            branching = v == "most_fractional" ? LPX_BRANCH_MOST_FRACTIONAL : v == "strong" ? LPX_BRANCH_STRONG : -2;
            if (branching == -2) { std::fprintf(stderr, "lpx_cli: --branching takes most_fractional or strong, got '%s'\n", v.c_str()); return 64; }
        }
        else if ((a == "--candidates" || a == "--probe-iter") && i + 1 < argc) {
            const std::string v = argv[++i];
            char* end = nullptr;
            const long x = std::strtol(v.c_str(), &end, 10);
            const bool cand = a == "--candidates";
            if (end == v.c_str() || *end || x < (cand ? 1 : 0) || x > (cand ? 32 : 1000000000)) {
                std::fprintf(stderr, cand ? "lpx_cli: --candidates takes a count in [1, 32], got '%s'\n"
                                          : "lpx_cli: --probe-iter takes a non-negative event limit, got '%s'\n", v.c_str());
                return 64;
            }
            (cand ? candidates : probe_iter) = (int)x;
        }
        else if ((a == "--upper" || a == "--lower") && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t eq = v.find('=');
            char* end = nullptr;
            const long idx = eq == std::string::npos ? 0 : std::strtol(v.c_str(), &end, 10);
            if (eq == std::string::npos || end != v.c_str() + eq || idx < 1) {
                std::fprintf(stderr, "lpx_cli: %s takes INDEX=VALUE with a 1-based index, got '%s'\n", a.c_str(), v.c_str());
                return 64;
            }
            const char* val = v.c_str() + eq + 1;
            const double x = std::strtod(val, &end);
            if (end == val || *end) { std::fprintf(stderr, "lpx_cli: bad value in %s %s\n", a.c_str(), v.c_str()); return 64; }
            bounds.push_back({a == "--upper", (int)idx - 1, x, a + " " + v});
        }
        else if (a == "--repaired") repaired = true;
        else if (a == "--iterations") iterations = true;
        else if (a == "--ranging") ranging = true;
        else if (a == "--cuts-per-round" && i + 1 < argc) { co.cuts_per_round = std::atoi(argv[++i]); cut_set = true; }
        else if (a == "--root-cuts" && i + 1 < argc) {
            const std::string v = argv[++i];
            char* end = nullptr;
            const long w = std::strtol(v.c_str(), &end, 10);
            if (end == v.c_str() || *end || w < 0 || w > 1000000) { std::fprintf(stderr, "lpx_cli: --root-cuts takes a number of rounds >= 0, got '%s'\n", v.c_str()); return 64; }
            root_cuts = (int)w;
        }
        else if (a == "--tighten") tighten = true;
        else if (a == "--cut-rounds" && i + 1 < argc) { co.max_rounds = std::atoi(argv[++i]); cut_set = true; }
        else if ((a == "--set-rhs" || a == "--set-cost") && i + 1 < argc) {
            const std::string v = argv[++i];
            const size_t eq = v.find('=');
            char* end = nullptr;
            const long idx = eq == std::string::npos ? 0 : std::strtol(v.c_str(), &end, 10);
            if (eq == std::string::npos || end != v.c_str() + eq || idx < 1) {
                std::fprintf(stderr, "lpx_cli: %s takes INDEX=VALUE with a 1-based index, got '%s'\n", a.c_str(), v.c_str());
                return 64;
            }
            const char* val = v.c_str() + eq + 1;
            const double x = std::strtod(val, &end);
            if (end == val || *end) { std::fprintf(stderr, "lpx_cli: bad value in %s %s\n", a.c_str(), v.c_str()); return 64; }
            edits.push_back({a == "--set-rhs", (int)idx - 1, x, a + " " + v});
        }
        else if (a == "--export" && i + 1 < argc) exportPath = argv[++i];
        else if (a == "--help" || a == "-h") {
            std::printf("usage: lpx_cli [--algorithm NAME] [--repaired] [--iterations] [--ranging] [--cuts-per-round K] [--cut-rounds N]\n"
                        "               [--upper J=V]... [--lower J=V]... [--binary] [--bnb-bounded [--long-step] [--cutoff] [--node-form F] [--divers W] [--plunge D] [--branching R [--candidates N] [--probe-iter L]] [--stall-events S] [--root-form F] [--root-cuts N [--cuts-per-round K]] [--tighten]] [--bounded-form F]\n"
                        "               [--bounded [--rhs-file F]] [--bounded-dual [--long-step] --rhs-file F] [--export FILE] INPUT.txt\n"
                        "               [--binary --bnb-bounded [--long-step] [--cutoff] --rhs-file F]\n"
                        "               [--bounded-dual [--long-step] --warm-base --rhs-file F]\n"
                        "               [--bounded-dual [--long-step] --warm-base --cost-file F [--rhs-file G]]\n"
                        "               [--bnb-bounded --dual-root [--long-step] [--cutoff] [--node-form F | --rhs-file F]]\n"
                        "  NAME: Primal Simplex | Revised Primal Simplex | Dual Simplex | Branch and Bound |\n"
                        "        Revised Branch and Bound | Branch and Bound Knapsack | Cutting Plane | Revised Cutting Plane |\n"
                        "        GMI Cutting Plane (gmi) | Bounded Primal Simplex\n"
                        "  --ranging: after the summary, the cost / RHS ranges, reduced costs and duals of the final tableau\n"
                        "             (Primal Simplex and Dual Simplex only)\n"
                        "  --cuts-per-round K, --cut-rounds N: GMI Cutting Plane options (defaults 8 and 50)\n"
                        "  --upper J=V, --lower J=V, --binary: bounds of x_J (1-based, repeatable) / every u_j = 1, kept beside the tableau\n"
                        "             by the Bounded Primal Simplex (no rows are added); not with --ranging, the cut options or another algorithm\n"
                        "  --bnb-bounded: with --binary / --upper / --lower, every variable integer: branch and bound by bound changes on the\n"
                        "             root's device tableau (every variable needs a finite, integral upper bound)\n"
                        "  --long-step, --cutoff: with --bnb-bounded, every node's dual loop uses the long-step (bound-flipping) ratio test /\n"
                        "             stops as soon as its objective has fallen to the incumbent (lpx_solve_bnb_bounded2)\n"
                        "  --node-form launches|onchip|auto: with --bnb-bounded, how a node is evaluated (lpx_solve_bnb_bounded3): by the\n"
                        "             launches of lpx_bounded_node2, in one launch with the tableau on chip, or on chip iff it fits\n"
                        "  --divers W: with --bnb-bounded, the search by W handles diving at once, one on-chip node per diver and one kernel\n"
                        "             launch per round (lpx_solve_bnb_bounded4); not with --node-form launches\n"
                        "  --plunge D: with --bnb-bounded, a diver goes on from a node that branches into its ceil child, up to D nodes per\n"
                        "             launch with the tableau staying on chip (lpx_solve_bnb_bounded5); without --divers it means --divers 1\n"
                        "  --branching most_fractional|strong: with --bnb-bounded, the branching rule (lpx_solve_bnb_bounded6; without\n"
                        "             --divers it means --divers 1): strong probes both children of up to N = --candidates (default 4, at most 32)\n"
                        "             fractional columns of every node on chip, --probe-iter L events each at most (default: the node's limit),\n"
                        "             and branches on the largest product of the two objective losses; not with --plunge above 1\n"
                        "  --stall-events S: with --bnb-bounded, the stall guard (lpx_solve_bnb_bounded7; without --divers it means --divers 1):\n"
                        "             after S pivots without progress of the objective a node selects by Bland's rule until the objective moves,\n"
                        "             so a node that cycles ends; 0 = no guard, 50 is a reasonable value; not with --node-form launches,\n"
                        "             --plunge above 1 or --branching\n"
                        "  --bounded-form launches|onchip|auto: the bounded primal solve (--binary / --upper / --lower without --bnb-bounded) as\n"
                        "             launches per pivot (the default) or in ONE kernel launch with the tableau on chip (lpx_solve_bounded2)\n"
                        "  --bounded: the Bounded Primal Simplex even without a bound.  --bounded --rhs-file F: the model once per line of F (m\n"
                        "             numbers: the right-hand sides of that run) as ONE packed call (lpx_solve_packed: one upload, one kernel\n"
                        "             launch, one read-back; c, A and the bounds shared); prints a line \"status value x1 .. xn\" per run\n"
                        "  --bounded-dual [--long-step] --rhs-file F: the same by the dual start (lpx_solve_packed_dual): >= rows and negative\n"
                        "             right-hand sides are accepted, an = row is refused; --long-step: the bound-flipping ratio test\n"
                        "  --bounded-dual [--long-step] --warm-base --rhs-file F: the input's own right-hand side is solved once and kept on the\n"
                        "             device (lpx_packed_base_open); every line of F is then re-solved from that base's optimal basis in ONE kernel\n"
                        "             launch (lpx_packed_base_solve); the same line per run\n"
                        "  --bounded-dual [--long-step] --warm-base --cost-file F [--rhs-file G]: the input's own model is solved once and kept on\n"
                        "             the device; every line of F (n numbers, the costs c) is re-solved from that base in ONE kernel launch\n"
                        "             (lpx_packed_base_solve_costs): the objective row is moved and the bounded primal loop continues.  With G,\n"
                        "             line k of F goes with line k of G (m numbers) and the dual loop follows; unequal line counts are refused\n"
                        "  --bnb-bounded --rhs-file F: the model as an integer program once per line of F as ONE packed call (lpx_solve_packed_bnb:\n"
                        "             a whole branch and bound per right-hand side in one kernel launch; at most 100000 nodes and 2000000 events\n"
                        "             per run); with --binary or --upper bounds and --long-step / --cutoff; the same line per run\n"
                        "  --dual-root: with --bnb-bounded, the search from a dual start (lpx_solve_bnb_bounded_dual): >= constraints and negative\n"
                        "             right-hand sides are accepted; with --long-step / --cutoff / --node-form and the bound flags only.  With\n"
                        "             --rhs-file F the packed call lpx_solve_packed_bnb_dual, a line per right-hand side; an = constraint is refused\n"
                        "  --root-cuts N: with --bnb-bounded --divers, cut-and-branch (lpx_solve_bnb_bounded9): up to N rounds of --cuts-per-round K\n"
                        "             (default 8) GMI cuts at the solved root, then the search from that tableau; not with --plunge or --branching\n"
                        "  --root-form launches|onchip|auto: with --bnb-bounded --divers, how the root LP is solved (lpx_solve_bnb_bounded8);\n"
                        "             the node log does not depend on it; not with --plunge or --branching\n"
                        "  --tighten: with --bnb-bounded --divers, reduced-cost bound tightening (lpx_solve_bnb_bounded10): from the first incumbent\n"
                        "             on, a node that ends optimal shrinks the range of every nonbasic integer column whose reduced cost leaves it\n"
                        "             less room than its range, for the node's subtree; not with --node-form launches, --plunge or --branching\n"
                        "  --set-rhs I=V, --set-cost J=V: after the solve, b_I = V / c_J = V (1-based, repeatable), applied in order,\n"
                        "             each re-optimised warm on the device from the previous basis; each re-solve's summary is printed\n");
            return 0;
        } else input = a;
    }
    if (root_cuts >= 0) { co.max_rounds = root_cuts; cut_set = false; }      // --cuts-per-round is the root loop's K then
    if (cut_set) {
        const std::string key = algorithm_key(algorithm);
        if (key != "gmi cutting plane" && key != "gmi") { std::fprintf(stderr, "lpx_cli: --cuts-per-round / --cut-rounds need --algorithm \"GMI Cutting Plane\"\n"); return 64; }
        if (ranging) { std::fprintf(stderr, "lpx_cli: --ranging does not combine with --cuts-per-round / --cut-rounds\n"); return 64; }
    }
    if (dual_root && (!bnb_bounded || bounded_flag || bounded_dual || divers || plunge || branching >= 0 || stall_events >= 0 || root_form >= 0 ||
                      root_cuts >= 0 || tighten || bounded_form >= 0 || iterations || ranging || repaired || cut_set || algo_set || !edits.empty() ||
                      !exportPath.empty() || (!rhs_file.empty() && node_form >= 0))) {
        std::fprintf(stderr, "lpx_cli: --dual-root needs --bnb-bounded and combines only with --long-step / --cutoff, --node-form (without --rhs-file), "
                             "--rhs-file and --upper / --lower / --binary\n");
        return 64;
    }
    const bool bounded = binary || !bounds.empty() || bounded_flag || bounded_dual;
    const bool packed_bnb = bnb_bounded && !rhs_file.empty() && !bounded_dual && !bounded_flag;     // --bnb-bounded --rhs-file F
    if (packed_bnb && (node_form >= 0 || divers || plunge || branching >= 0 || stall_events >= 0 || root_form >= 0 || root_cuts >= 0 || tighten ||
                       bounded_form >= 0 || iterations || !edits.empty() || !exportPath.empty())) {
        std::fprintf(stderr, "lpx_cli: --bnb-bounded --rhs-file combines only with --long-step / --cutoff and --upper / --lower / --binary\n");
        return 64;
    }
    if (!cost_file.empty() && !(bounded_dual && warm_base)) { std::fprintf(stderr, "lpx_cli: --cost-file needs --bounded-dual --warm-base\n"); return 64; }
    if (bounded_dual && warm_base && rhs_file.empty() && cost_file.empty()) {
        std::fprintf(stderr, "lpx_cli: --bounded-dual --warm-base needs --rhs-file or --cost-file\n");
        return 64;
    }
    if (bounded_dual && ((rhs_file.empty() && cost_file.empty()) || bounded_flag || bnb_bounded || bounded_form >= 0 || iterations || !edits.empty() || !exportPath.empty() ||
                         (search_flags & ~LPX_BDUAL_LONG_STEP))) {
        std::fprintf(stderr, "lpx_cli: --bounded-dual needs --rhs-file and combines only with --long-step and --upper / --lower / --binary\n");
        return 64;
    }
    if (warm_base && !bounded_dual) { std::fprintf(stderr, "lpx_cli: --warm-base needs --bounded-dual --rhs-file\n"); return 64; }
    if (!bounded_dual && !packed_bnb && !rhs_file.empty() && (!bounded_flag || bnb_bounded || bounded_form >= 0 || iterations || !edits.empty() || !exportPath.empty())) {
        std::fprintf(stderr, "lpx_cli: --rhs-file needs --bounded and combines only with --upper / --lower / --binary\n");
        return 64;
    }
    if (bnb_bounded && !bounded) { std::fprintf(stderr, "lpx_cli: --bnb-bounded needs --binary or --upper bounds\n"); return 64; }
    if (search_flags && !bnb_bounded && !bounded_dual) { std::fprintf(stderr, "lpx_cli: --long-step / --cutoff need --bnb-bounded\n"); return 64; }
    if (node_form >= 0 && !bnb_bounded) { std::fprintf(stderr, "lpx_cli: --node-form needs --bnb-bounded\n"); return 64; }
    if (divers && !bnb_bounded) { std::fprintf(stderr, "lpx_cli: --divers needs --bnb-bounded\n"); return 64; }
    if (plunge && !bnb_bounded) { std::fprintf(stderr, "lpx_cli: --plunge needs --bnb-bounded\n"); return 64; }
    if (plunge && node_form == LPX_NODE_LAUNCHES) { std::fprintf(stderr, "lpx_cli: --plunge evaluates every node on chip: not with --node-form launches\n"); return 64; }
    if (branching >= 0 && !bnb_bounded) { std::fprintf(stderr, "lpx_cli: --branching needs --bnb-bounded\n"); return 64; }
    if (branching >= 0 && plunge > 1) { std::fprintf(stderr, "lpx_cli: --branching decides between a node and its children: not with --plunge above 1\n"); return 64; }
    if (branching >= 0 && node_form == LPX_NODE_LAUNCHES) { std::fprintf(stderr, "lpx_cli: --branching evaluates every node on chip: not with --node-form launches\n"); return 64; }
    if (stall_events >= 0 && !bnb_bounded) { std::fprintf(stderr, "lpx_cli: --stall-events needs --bnb-bounded\n"); return 64; }
    if (stall_events >= 0 && node_form == LPX_NODE_LAUNCHES) { std::fprintf(stderr, "lpx_cli: --stall-events: the stall guard has no launches form: not with --node-form launches\n"); return 64; }
    if (stall_events >= 0 && plunge > 1) { std::fprintf(stderr, "lpx_cli: --stall-events: the plunge has no stall guard: not with --plunge above 1\n"); return 64; }
    if (stall_events >= 0 && branching >= 0) { std::fprintf(stderr, "lpx_cli: --stall-events: the probes have no stall guard: not with --branching\n"); return 64; }
    if (bounded_form >= 0 && (!bounded || bnb_bounded)) { std::fprintf(stderr, "lpx_cli: --bounded-form needs --binary or --upper / --lower bounds, without --bnb-bounded\n"); return 64; }
    if (root_form >= 0 && !(bnb_bounded && divers)) { std::fprintf(stderr, "lpx_cli: --root-form needs --bnb-bounded --divers\n"); return 64; }
    if (root_form >= 0 && (plunge || branching >= 0)) { std::fprintf(stderr, "lpx_cli: --root-form: the plunge and the strong-branching drivers have no root form\n"); return 64; }
    if (root_cuts >= 0 && !(bnb_bounded && divers)) { std::fprintf(stderr, "lpx_cli: --root-cuts needs --bnb-bounded --divers\n"); return 64; }
    if (root_cuts >= 0 && (plunge || branching >= 0)) { std::fprintf(stderr, "lpx_cli: --root-cuts: the plunge and the strong-branching drivers have no root cuts\n"); return 64; }
    if (tighten && !(bnb_bounded && divers)) { std::fprintf(stderr, "lpx_cli: --tighten needs --bnb-bounded --divers\n"); return 64; }
    if (tighten && node_form == LPX_NODE_LAUNCHES) { std::fprintf(stderr, "lpx_cli: --tighten: reduced-cost tightening has no launches form: not with --node-form launches\n"); return 64; }
    if (tighten && (plunge || branching >= 0)) { std::fprintf(stderr, "lpx_cli: --tighten: the plunge and the strong-branching drivers have no tightening\n"); return 64; }
    if ((root_cuts >= 0 || tighten) && root_form < 0) root_form = LPX_NODE_LAUNCHES;
    if (root_form >= 0 && stall_events < 0) stall_events = 0;
    if (stall_events >= 0) { plunge = 0; if (!divers) divers = 1; }
    if (branching >= 0) { plunge = 0; if (!divers) divers = 1; }
    if (plunge && !divers) divers = 1;
    if (divers && node_form == LPX_NODE_LAUNCHES) { std::fprintf(stderr, "lpx_cli: --divers evaluates every node on chip: not with --node-form launches\n"); return 64; }
    if (bounded) {
        if (ranging) { std::fprintf(stderr, "lpx_cli: --upper / --lower / --binary do not combine with --ranging\n"); return 64; }
        if (cut_set) { std::fprintf(stderr, "lpx_cli: --upper / --lower / --binary do not combine with --cuts-per-round / --cut-rounds\n"); return 64; }
        if (algo_set && algorithm_key(algorithm) != "bounded primal simplex") {
            std::fprintf(stderr, "lpx_cli: --upper / --lower / --binary select the Bounded Primal Simplex, not --algorithm \"%s\"\n", algorithm.c_str());
            return 64;
        }
    }
    if (input.empty()) { std::fprintf(stderr, "lpx_cli: no input file (try --help)\n"); return 64; }
    std::ifstream f(input);
    if (!f) { std::fprintf(stderr, "Error reading file: %s\n", input.c_str()); return 66; }
    std::stringstream ss; ss << f.rdbuf();
    const std::string text = ss.str();

    lpx_parsed p;
    char err[1024];
    if (lpx_parse_text(text.c_str(), &p) != 0) { lpx_last_error(err, sizeof err); std::fprintf(stderr, "%s\n", err); return 65; }
    lpx_problem prob; prob.sense = p.sense; prob.n = p.n; prob.m = p.m; prob.c = p.c; prob.A = p.A; prob.rel = p.rel; prob.b = p.b;
    lpx_solve_opts o; lpx_default_solve_opts(&o);
    o.text_cb = on_text;
    o.render_iterations = iterations ? 1 : 0;
    // the on-chip form of the bounded solve reports no event: without --iterations no text is asked for, so it may be chosen
    if (bounded_form > LPX_NODE_LAUNCHES && !iterations) o.text_cb = nullptr;
    if (repaired) { o.dual_flags = 7; o.bnb_mode = 1; }
    lpx_result r;
    lpx_ranging rg;
    std::vector<double> lo((size_t)(p.n > 0 ? p.n : 1), 0.0), up((size_t)(p.n > 0 ? p.n : 1), binary ? 1.0 : 1.0 / 0.0);
    for (const Bound& bd : bounds) {
        if (bd.index >= p.n) { std::fprintf(stderr, "lpx_cli: %s: index out of range\n", bd.text.c_str()); lpx_parsed_free(&p); return 64; }
        (bd.upper ? up : lo)[bd.index] = bd.value;
    }
    if (!cost_file.empty()) {
        // the input's own model is the base; a cost vector per line of F and, with --rhs-file G, a right-hand side per line of G
        for (int i = 0; i < p.m; ++i)
            if (p.rel[i] == LPX_EQ) {
                std::fprintf(stderr, "lpx_cli: --bounded-dual --cost-file: an = constraint is not accepted (pass it as its <= and >= pair)\n");
                lpx_parsed_free(&p); return 65;
            }
        std::vector<double> costs, rhs;
        int count = 0, rhs_count = 0;
        int frc = read_rows(cost_file, "--cost-file", p.n, costs, count);
        if (frc == 0 && !rhs_file.empty()) frc = read_rows(rhs_file, "--rhs-file", p.m, rhs, rhs_count);
        if (frc != 0) { lpx_parsed_free(&p); return frc; }
        if (count == 0) { std::fprintf(stderr, "lpx_cli: --cost-file holds no cost vector\n"); lpx_parsed_free(&p); return 65; }
        if (!rhs_file.empty() && rhs_count != count) {
            std::fprintf(stderr, "lpx_cli: --cost-file holds %d lines and --rhs-file holds %d\n", count, rhs_count);
            lpx_parsed_free(&p); return 65;
        }
        std::vector<int32_t> status((size_t)(count > 0 ? count : 1));
        std::vector<double> x((size_t)(count > 0 ? count : 1) * (size_t)(p.n > 0 ? p.n : 1)), value((size_t)(count > 0 ? count : 1));
        lpx_packed_cost_results cr; std::memset(&cr, 0, sizeof cr);
        cr.status = status.data(); cr.x = x.data(); cr.value = value.data();
        lpx_run_opts ro; lpx_default_opts(&ro, 1);
        lpx_packed_base_model bm; std::memset(&bm, 0, sizeof bm);
        bm.m = p.m; bm.n = p.n; bm.sense = p.sense;
        bm.c = p.c; bm.A = p.A; bm.b = p.b; bm.lower = lo.data(); bm.upper = up.data(); bm.rel = p.rel;
        lpx_packed_base* base = nullptr;
        int prc = lpx_packed_base_open(&bm, search_flags & LPX_BDUAL_LONG_STEP, &ro, nullptr, &base);
        if (prc == 0) prc = lpx_packed_base_solve_costs(base, count, costs.data(), rhs_file.empty() ? nullptr : rhs.data(),
                                                        search_flags & LPX_BDUAL_LONG_STEP, nullptr, &ro, &cr, nullptr);
        lpx_packed_base_close(base);
        if (prc != 0) { lpx_parsed_free(&p); lpx_last_error(err, sizeof err); std::fprintf(stderr, "%s\n", err); return prc == LPX_EDEVICE ? 69 : 70; }
        for (int i = 0; i < count; ++i) {
            std::printf("%d %.17g", status[i], value[i]);
            for (int j = 0; j < p.n; ++j) std::printf(" %.17g", x[(size_t)i * p.n + j]);
            std::printf("\n");
        }
        lpx_parsed_free(&p);
        return 0;
    }
    if (!rhs_file.empty()) {
        // one packed call: a right-hand side per line, everything else shared at stride 0
        for (int i = 0; i < p.m; ++i) {
            if (dual_root && p.rel[i] == LPX_EQ) {
                std::fprintf(stderr, "lpx_cli: --dual-root --rhs-file: an = constraint is not accepted (pass it as its <= and >= pair)\n");
                lpx_parsed_free(&p); return 65;
            }
            if (dual_root) continue;
            if (bounded_dual && p.rel[i] == LPX_EQ) {
                std::fprintf(stderr, "lpx_cli: --bounded-dual --rhs-file: an = constraint is not accepted (pass it as its <= and >= pair)\n");
                lpx_parsed_free(&p); return 65;
            }
            if (!bounded_dual && p.rel[i] != LPX_LE) { std::fprintf(stderr, "lpx_cli: --rhs-file: every constraint must be <=\n"); lpx_parsed_free(&p); return 65; }
        }
        std::ifstream rf(rhs_file);
        if (!rf) { std::fprintf(stderr, "Error reading file: %s\n", rhs_file.c_str()); lpx_parsed_free(&p); return 66; }
        std::vector<double> rhs;
        std::string line;
        int count = 0;
        while (std::getline(rf, line)) {
            std::istringstream ls(line);
            std::vector<double> row; double v;
            while (ls >> v) row.push_back(v);
            if (row.empty() && ls.eof()) continue;      // a blank line
            if ((int)row.size() != p.m || !ls.eof()) {
                std::fprintf(stderr, "lpx_cli: --rhs-file: line %d does not hold %d numbers\n", count + 1, p.m);
                lpx_parsed_free(&p); return 65;
            }
            rhs.insert(rhs.end(), row.begin(), row.end()); ++count;
        }
        std::vector<int32_t> status((size_t)(count > 0 ? count : 1));
        std::vector<double> x((size_t)(count > 0 ? count : 1) * (size_t)(p.n > 0 ? p.n : 1)), value((size_t)(count > 0 ? count : 1));
        int prc;
        if (packed_bnb) {                               // c, A and the bounds: stride 0; every variable integer, as --bnb-bounded
            lpx_packed_bnb_models bm; std::memset(&bm, 0, sizeof bm);
            bm.count = count; bm.m = p.m; bm.n = p.n; bm.sense = p.sense;
            bm.c = p.c; bm.A = p.A; bm.b = rhs.data(); bm.lower = lo.data(); bm.upper = up.data();
            bm.b_stride = p.m;
            lpx_packed_bnb_opts bo; std::memset(&bo, 0, sizeof bo);
            lpx_run_opts ro; lpx_default_opts(&ro, 1);
            bo.search_flags = search_flags; bo.max_iter = ro.max_iter;
            bo.max_depth = binary && bounds.empty() ? 0 : 4 * p.n + 64;    // a general integer is branched on more than once
            bo.max_nodes = 100000; bo.max_events = 2000000;
            lpx_packed_bnb_results br; std::memset(&br, 0, sizeof br);
            br.status = status.data(); br.x = x.data(); br.value = value.data();
            if (dual_root) {                            // the same call from a dual start: rel too at stride 0
                lpx_packed_bnb_dual_models dm; std::memset(&dm, 0, sizeof dm);
                dm.count = count; dm.m = p.m; dm.n = p.n; dm.sense = p.sense;
                dm.c = p.c; dm.A = p.A; dm.b = rhs.data(); dm.lower = lo.data(); dm.upper = up.data(); dm.rel = p.rel;
                dm.b_stride = p.m;
                prc = lpx_solve_packed_bnb_dual(&dm, &bo, &br, nullptr);
            } else
            prc = lpx_solve_packed_bnb(&bm, &bo, &br, nullptr);
        } else if (bounded_dual) {                             // c, A, rel and the bounds: stride 0, one copy for every run
            lpx_packed_dual_models dm; std::memset(&dm, 0, sizeof dm);
            dm.count = count; dm.m = p.m; dm.n = p.n; dm.sense = p.sense;
            dm.c = p.c; dm.A = p.A; dm.b = rhs.data(); dm.lower = lo.data(); dm.upper = up.data(); dm.rel = p.rel;
            dm.b_stride = p.m;
            lpx_packed_dual_results dr; std::memset(&dr, 0, sizeof dr);
            dr.status = status.data(); dr.x = x.data(); dr.value = value.data();
            lpx_run_opts ro; lpx_default_opts(&ro, 1);
            if (warm_base) {                            // the input's own right-hand side is the base; every line continues from it
                lpx_packed_base_model bm; std::memset(&bm, 0, sizeof bm);
                bm.m = p.m; bm.n = p.n; bm.sense = p.sense;
                bm.c = p.c; bm.A = p.A; bm.b = p.b; bm.lower = lo.data(); bm.upper = up.data(); bm.rel = p.rel;
                lpx_packed_base* base = nullptr;
                prc = lpx_packed_base_open(&bm, search_flags & LPX_BDUAL_LONG_STEP, &ro, nullptr, &base);
                if (prc == 0) prc = lpx_packed_base_solve(base, count, rhs.data(), search_flags & LPX_BDUAL_LONG_STEP, &ro, &dr, nullptr);
                lpx_packed_base_close(base);
            } else
            prc = lpx_solve_packed_dual(&dm, search_flags & LPX_BDUAL_LONG_STEP, &ro, &dr, nullptr);
        } else {
            lpx_packed_models pm; std::memset(&pm, 0, sizeof pm);
            pm.count = count; pm.m = p.m; pm.n = p.n; pm.sense = p.sense;
            pm.c = p.c; pm.A = p.A; pm.b = rhs.data(); pm.lower = lo.data(); pm.upper = up.data();
            pm.b_stride = p.m;                          // c, A and the bounds: stride 0, one copy for every run
            lpx_packed_results pr; std::memset(&pr, 0, sizeof pr);
            pr.status = status.data(); pr.x = x.data(); pr.value = value.data();
            lpx_run_opts ro; lpx_default_opts(&ro, 0);
            prc = lpx_solve_packed(&pm, &ro, &pr, nullptr);
        }
        if (prc != 0) { lpx_parsed_free(&p); lpx_last_error(err, sizeof err); std::fprintf(stderr, "%s\n", err); return prc == LPX_EDEVICE ? 69 : 70; }
        for (int i = 0; i < count; ++i) {
            std::printf("%d %.17g", status[i], value[i]);
            for (int j = 0; j < p.n; ++j) std::printf(" %.17g", x[(size_t)i * p.n + j]);
            std::printf("\n");
        }
        lpx_parsed_free(&p);
        return 0;
    }
    lpx_bnb_cut_info cinfo; std::memset(&cinfo, 0, sizeof cinfo);
    lpx_bnb_fix_info finfo; std::memset(&finfo, 0, sizeof finfo);
    const int rc = bnb_bounded && tighten ? lpx_solve_bnb_bounded10(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, stall_events, root_form,
                                                                    root_cuts >= 0 ? &co : nullptr, 1, &r, nullptr, nullptr, nullptr, &cinfo, &finfo)
                 : bnb_bounded && root_cuts >= 0 ? lpx_solve_bnb_bounded9(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, stall_events, root_form, &co, &r, nullptr, nullptr, nullptr, &cinfo)
                 : bnb_bounded && root_form >= 0 ? lpx_solve_bnb_bounded8(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, stall_events, root_form, &r, nullptr, nullptr, nullptr)
                 : bnb_bounded && stall_events >= 0 ? lpx_solve_bnb_bounded7(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, stall_events, &r, nullptr, nullptr, nullptr)
                 : bnb_bounded && branching >= 0 ? lpx_solve_bnb_bounded6(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, branching, candidates,
                                                                         probe_iter >= 0 ? probe_iter : o.max_iter > 0 ? o.max_iter : 10000, &r, nullptr, nullptr, nullptr)
                 : bnb_bounded && plunge ? lpx_solve_bnb_bounded5(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, plunge, &r, nullptr, nullptr, nullptr)
                 : bnb_bounded && divers ? lpx_solve_bnb_bounded4(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, divers, &r, nullptr, nullptr)
                 : bnb_bounded && dual_root ? lpx_solve_bnb_bounded_dual(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, node_form >= 0 ? node_form : LPX_NODE_LAUNCHES, &r, nullptr)
                 : bnb_bounded && node_form >= 0 ? lpx_solve_bnb_bounded3(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, node_form, &r, nullptr)
                 : bnb_bounded && search_flags ? lpx_solve_bnb_bounded2(&prob, lo.data(), up.data(), nullptr, &o, 0, search_flags, &r, nullptr)
                 : bnb_bounded ? lpx_solve_bnb_bounded(&prob, lo.data(), up.data(), nullptr, &o, 0, &r, nullptr)
                 : bounded && bounded_form >= 0 ? lpx_solve_bounded2(&prob, lo.data(), up.data(), &o, bounded_form, &r, nullptr)
                 : bounded ? lpx_solve_bounded(&prob, lo.data(), up.data(), &o, &r, nullptr) : ranging ? lpx_solve_ranging(&prob, algorithm.c_str(), &o, &r, &rg)
                 : cut_set ? lpx_solve_cuts(&prob, &o, &co, &r) : lpx_solve(&prob, algorithm.c_str(), &o, &r);
    if (rc != 0) { lpx_parsed_free(&p); lpx_last_error(err, sizeof err); std::fprintf(stderr, "%s\n", err); return rc == LPX_EDEVICE ? 69 : 70; }
    std::string shown = g_iterations;
    shown += "\n\nFinal Report:\n"; shown += r.report ? r.report : "";
    shown += "\n\nSummary:\n"; shown += r.summary ? r.summary : "";
    if (root_cuts >= 0) {
        shown += "root cuts: " + std::to_string(cinfo.rounds) + " rounds, " + std::to_string(cinfo.added) + " added, " + std::to_string(cinfo.purged) +
                 " purged, search on " + std::to_string(cinfo.R) + " x " + std::to_string(cinfo.C) + (cinfo.ran ? "\n" : " (no spare capacity on chip: no round)\n");
        lpx_bnb_cut_info_free(&cinfo);
    }
    if (tighten)
        shown += "tightening: " + std::to_string(finfo.tightened_cols) + " columns on " + std::to_string(finfo.tightened_nodes) + " nodes, at most " +
                 std::to_string(finfo.max_per_node) + " on one\n";
    if (ranging) shown += ranging_table(rg);
    if (!edits.empty()) {
        lpx_session* ses = nullptr;
        lpx_result sr;
        int src = lpx_session_open(&prob, nullptr, &ses, &sr);
        if (src == 0) lpx_result_free(&sr);
        for (size_t e = 0; src == 0 && e < edits.size(); ++e) {
            const Edit& ed = edits[e];
            const int32_t idx = ed.index;
            if ((ed.rhs && idx >= p.m) || (!ed.rhs && idx >= p.n)) {
                std::fprintf(stderr, "lpx_cli: %s: index out of range\n", ed.text.c_str());
                lpx_session_close(ses); lpx_parsed_free(&p); lpx_result_free(&r);
                if (ranging) lpx_ranging_free(&rg);
                return 64;
            }
            src = ed.rhs ? lpx_session_set_rhs(ses, 1, &idx, &ed.value, &sr) : lpx_session_set_cost(ses, 1, &idx, &ed.value, &sr);
            if (src != 0) break;
            char head[256];
            std::snprintf(head, sizeof head, "\n\nRe-solve after %s (%s, %d pivots):\n", ed.text.c_str(), sr.aux[0] != 0 ? "warm" : "cold",
                          sr.n_pivots);
            shown += head; shown += sr.summary ? sr.summary : "";
            lpx_result_free(&sr);
        }
        lpx_session_close(ses);
        if (src != 0) {
            lpx_last_error(err, sizeof err); std::fprintf(stderr, "%s\n", err);
            lpx_parsed_free(&p); lpx_result_free(&r);
            if (ranging) lpx_ranging_free(&rg);
            return src == LPX_EDEVICE ? 69 : 70;
        }
    }
    lpx_parsed_free(&p);
    std::fputs(shown.c_str(), stdout); std::fputc('\n', stdout);
    if (!exportPath.empty()) {
        std::ofstream w(exportPath);
        w << "Linear Program:\n" << text << "\n\nIterations:\n" << shown << "\n";
    }
    lpx_result_free(&r);
    if (ranging) lpx_ranging_free(&rg);
    return 0;
}
