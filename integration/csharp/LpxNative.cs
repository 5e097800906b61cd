// LpxNative.cs -- P/Invoke declarations of liblpx.so (include/lpx.h), for the reference application
// Jellyman750/Linear_Programming_Solver_LPR381.  Shipped as source: no .NET toolchain exists in the build image, so this
// file has NOT been compiled here; every entry point below is exercised through the same C ABI by tests/test_gpu_*.py.
//
// Layouts mirror include/lpx.h field by field (LayoutKind.Sequential, cdecl).  Nothing from include/lpx_test.h appears here.
using System;
using System.Runtime.InteropServices;

namespace Linear_Programming_Solver.Native
{
    [StructLayout(LayoutKind.Sequential)]
    public struct LpxStats                       // lpx_stats
    {
        public long pivots, launches;
        public double loop_ms, h2d_ms, d2h_ms, update_ms_sum;
        public long update_launches, fdf_pivots, cleanup_pivots;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxProblem              // lpx_problem  (LPProblem, Models/PrimalSimplex.cs:20-36)
    {
        public int sense, n, m;                  // sense: 0 = Max, 1 = Min (enum Sense, :8)
        public double* c;                        // [n]
        public double* A;                        // [m*n] row-major
        public int* rel;                         // [m]   0 = LE, 1 = GE, 2 = EQ (enum Rel, :9)
        public double* b;                        // [m]
    }

    [UnmanagedFunctionPointer(CallingConvention.Cdecl)]
    public delegate void LpxPivotCb(IntPtr user, int iter, int row, int col);
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)]
    public unsafe delegate void LpxAllreduceMax(IntPtr user, double* vals, int count);
    [UnmanagedFunctionPointer(CallingConvention.Cdecl)]
    public unsafe delegate void LpxTextCb(IntPtr user, byte* text, byte* highlight, int R, int C);

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxSolveOpts                   // lpx_solve_opts
    {
        public int max_iter, batch, render_iterations, dual_flags, bnb_mode, bnb_search, concurrent_nodes, rank, world;
        public long max_nodes;
        public IntPtr allreduce_max, allreduce_user;     // LpxAllreduceMax via Marshal.GetFunctionPointerForDelegate
        public IntPtr text_cb, text_user;                // LpxTextCb
        public int bnb_dive;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxResult               // lpx_result  (SimplexResult, Models/PrimalSimplex.cs:38-49)
    {
        public int status, has_solution;
        public double optimal_value;
        public int n; public double* x;
        public int R, C; public double* T;
        public int* basis;
        public int n_pivots; public int* trace;
        public byte* report; public byte* summary;
        public long lp_solves, nodes;
        public int n_log; public int* node_log; public double* node_z;
        public fixed double aux[4];
        public LpxStats stats;
        public int n_cuts; public double* cuts;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxRanging              // lpx_ranging  (lpx_solve_ranging; no counterpart in the reference)
    {
        public int n, m, valid;
        public double min_rhs, min_dj;
        public double* cost_lo; public double* cost_hi; public int* cost_lo_at; public int* cost_hi_at;
        public double* reduced_cost;
        public double* rhs_lo; public double* rhs_hi; public int* rhs_lo_at; public int* rhs_hi_at;
        public double* dual;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxSessionOpts                 // lpx_session_opts  (lpx_session_open; not in the reference)
    {
        public int extra_rows, extra_cols, max_iter, batch, want_tableau;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxCutOpts                     // lpx_cut_opts  (lpx_solve_cuts / lpx_tableau_gmi_round; not in the reference)
    {
        public int cuts_per_round, max_rounds, max_active, purge;
        public double away, coef_eps, max_dynamism, purge_tol, int_tol;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxBranchPick                  // lpx_branch_pick  (lpx_tableau_branch_pick)
    {
        public int var, candidates;
        public double x_var, z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxNodeRecord                  // lpx_node_record  (lpx_bounded_node)
    {
        public int status, events;
        public long kind0, kind1, flips, unrepairable;
        public LpxBranchPick pick;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxBnbNodeLog                  // lpx_bnb_node_log  (one node of lpx_solve_bnb_bounded)
    {
        public int depth, K, status, events, flips, var;
        public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxBnbBoundedInfo       // lpx_bnb_bounded_info  (free with lpx_bnb_bounded_info_free)
    {
        public long nodes, events, flips, incumbents, pruned_bound, pruned_infeasible, max_K;
        public double constant;
        public long n_log;
        public LpxBnbNodeLog* log;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxBnbDiversInfo        // lpx_bnb_divers_info  (free with lpx_bnb_divers_info_free)
    {
        public long rounds, steals, largest_batch;
        public int* round, diver;                // [n_log of the LpxBnbBoundedInfo] each
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxBnbPlungeInfo        // lpx_bnb_plunge_info  (free with lpx_bnb_plunge_info_free)
    {
        public long launched, dropped, longest_chain;
        public int* step;                        // [n_log of the LpxBnbBoundedInfo]
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxProbeHead                   // lpx_probe_head: 16 bytes
    {
        public int count, candidates;            // candidates probed (0 = nothing was probed) of how many fractional integer columns
        public double z;                         // T[m,Cm] of the handle
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxProbeRecord                 // lpx_probe_record: 64 bytes; status -1 = refused, -2 (LPX_PROBE_NONE) = no probe
    {
        public int status, events, kind0, kind1, flips, var, dir, pad;      // dir: 0 = floor child, 1 = ceil child
        public double x_var, lower, upper, z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxBnbStrongInfo               // lpx_bnb_strong_info: 48 bytes of counters (lpx_bnb_strong_info_free zeroes them)
    {
        public long probe_launches, probes, probe_events, probe_limit, pruned_by_probe, changed_picks;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxPrimalRecord                // lpx_primal_record: 40 bytes, one entry of lpx_node_batch_primal
    {
        public int status, events;               // LPX_OPTIMAL / LPX_UNBOUNDED / LPX_ITER_LIMIT; pivots and flips
        public long kind0, kind1, flips;
        public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedModels         // lpx_packed_models: count models of one shape as contiguous arrays
    {
        public int count, m, n, sense;           // every row is <=
        public double* c, A, b;                  // [count][n], [count][m][n] row-major, [count][m]
        public double* lower, upper;             // [count][n] or null (0 / +inf)
        public long c_stride, A_stride, b_stride, lower_stride, upper_stride;   // doubles between models; 0 = one shared copy
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedResults        // lpx_packed_results: caller-allocated; rec, basis, at_upper may be null
    {
        public int* status; public double* x; public double* value;
        public LpxPrimalRecord* rec; public int* basis; public byte* at_upper;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedDualModels     // lpx_packed_dual_models: lpx_packed_models plus the row senses
    {
        public int count, m, n, sense;           // rows are <= or >=
        public double* c, A, b;                  // [count][n], [count][m][n] row-major, [count][m]
        public double* lower, upper;             // [count][n] or null (0 / +inf)
        public long c_stride, A_stride, b_stride, lower_stride, upper_stride;   // doubles between models; 0 = one shared copy
        public int* rel;                         // [count][m] of LPX_LE (0) / LPX_GE (1), or null = every row is <=
        public long rel_stride;                  // int32 between models: m, or 0 = one shared copy
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxPackedDualRecord            // lpx_packed_dual_record: 48 bytes, one model of lpx_solve_packed_dual
    {
        public int status, events;               // LPX_OPTIMAL / LPX_INFEASIBLE / LPX_ITER_LIMIT / LPX_EINVAL; pivots and passes
        public long kind0, kind1, passes, dualize_flips;
        public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedDualResults    // lpx_packed_dual_results: caller-allocated; the last five may be null
    {
        public int* status; public double* x; public double* value;
        public LpxPackedDualRecord* rec; public int* basis; public byte* at_upper;
        public double* y; public double* d;      // [count][m] duals, [count][n] reduced costs, in the user's sense
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxPackedCostRecord            // lpx_packed_cost_record: 72 bytes, one scenario of lpx_packed_base_solve_costs
    {
        public int status;                       // LPX_OPTIMAL / LPX_UNBOUNDED / LPX_INFEASIBLE / LPX_ITER_LIMIT / LPX_EINVAL
        public int primal_events, dual_events, pad;
        public long primal_kind0, primal_kind1, primal_flips;   // the primal loop: pivots of either kind, bound flips
        public long dual_kind0, dual_kind1, dual_passes;        // the dual loop (all 0 without b)
        public double z;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedCostResults    // lpx_packed_cost_results: caller-allocated; the last five may be null
    {
        public int* status; public double* x; public double* value;
        public LpxPackedCostRecord* rec; public int* basis; public byte* at_upper; public double* y; public double* d;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedBaseModel      // lpx_packed_base_model: the one model of lpx_packed_base_open
    {
        public int m, n, sense;
        public double* c, A, b;                  // [n], [m][n] row-major, [m]: b is the base right-hand side
        public double* lower, upper;             // [n] or null (0 / +inf)
        public int* rel;                         // [m] of LPX_LE (0) / LPX_GE (1), or null = every row is <=
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedBnbModels      // lpx_packed_bnb_models: lpx_packed_models plus the integer mask
    {
        public int count, m, n, sense;           // every row is <=
        public double* c, A, b;                  // [count][n], [count][m][n] row-major, [count][m]
        public double* lower, upper;             // [count][n] or null (0 / +inf)
        public long c_stride, A_stride, b_stride, lower_stride, upper_stride;   // doubles between models; 0 = one shared copy
        public byte* is_int;                     // [n], shared by every model, or null = every variable is integer
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedBnbDualModels  // lpx_packed_bnb_dual_models: lpx_packed_dual_models plus the integer mask
    {
        public int count, m, n, sense;
        public double* c, A, b;                  // [count][n], [count][m][n] row-major, [count][m]
        public double* lower, upper;             // [count][n] or null (0 / +inf)
        public long c_stride, A_stride, b_stride, lower_stride, upper_stride;   // doubles between models; 0 = one shared copy
        public int* rel;                         // [count][m] of LPX_LE (0) / LPX_GE (1), or null = every row is <=
        public long rel_stride;                  // ints between models: m, or 0 = one shared copy
        public byte* is_int;                     // [n], shared by every model, or null = every variable is integer
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxPackedBnbOpts               // lpx_packed_bnb_opts: the flags and the budgets of one model's search
    {
        public int search_flags, max_iter, max_depth, log_cap;   // LPX_BDUAL_LONG_STEP (2) | LPX_BDUAL_CUTOFF (4); max_depth 0 = n
        public long max_nodes, max_events;       // both at least 1
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxPackedBnbRecord             // lpx_packed_bnb_record: 88 bytes, one model of lpx_solve_packed_bnb
    {
        public int status, stop;                 // stop: LPX_PBNB_* 0 done, 1 root, 2 nodes, 3 node_iter, 4 events, 5 depth, 6 refused
        public long nodes, events, flips, incumbents, pruned_bound, pruned_infeasible;
        public int max_K, deepest, root_events, logged;
        public double best, constant;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxPackedBnbResults     // lpx_packed_bnb_results: caller-allocated; rec and log may be null
    {
        public int* status; public double* x; public double* value;
        public LpxPackedBnbRecord* rec; public LpxBnbNodeLog* log;   // [count], [count][log_cap]
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxGuardRecord                 // lpx_guard_record: 8 bytes
    {
        public int bland_events, first_bland;    // pivots made in Bland mode; event index of the first, -1 = none
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxBnbGuardInfo                // lpx_bnb_guard_info: 24 bytes of counters, nothing to free
    {
        public long guarded_nodes, bland_events, max_events;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxFixList              // lpx_fix_list: 32 bytes; the caller owns the arrays (cap entries each, cap >= nint)
    {
        public int cap, n;                       // in: capacity; out: columns tightened
        public int* cols;                        // out [n]: ascending
        public double* lower;                    // out [n]: the triples a bound edit would take
        public double* upper;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct LpxBnbFixInfo                  // lpx_bnb_fix_info: 24 bytes of counters, nothing to free
    {
        public long tightened_nodes, tightened_cols, max_per_node;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxCutLoopRecord        // lpx_cut_loop_record (lpx_bounded_cut_loop); z_before / z_after: the caller's [max_rounds] or null
    {
        public int rounds, added, purged, stop;
        public int status, R, C, pad;
        public long events;
        public LpxBranchPick pick;
        public double* z_before;
        public double* z_after;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxBnbCutInfo           // lpx_bnb_cut_info (lpx_solve_bnb_bounded9; free with lpx_bnb_cut_info_free)
    {
        public int ran, spare, rounds, added, purged, stop, status, R, C, n_z;
        public long events;
        public double* z_before;
        public double* z_after;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct LpxBoundedInfo          // lpx_bounded_info  (lpx_solve_bounded; free with lpx_bounded_info_free)
    {
        public int ncols, n;
        public byte* flip;
        public double* ub;
        public double* lower;
    }

    public static unsafe class Lpx
    {
        const string Lib = "lpx";                // liblpx.so (Linux) next to the executable / on LD_LIBRARY_PATH

        public const int OPTIMAL = 0, UNBOUNDED = 1, INFEASIBLE = 2, ITER_LIMIT = 3;
        public const int CUTOFF = 5;             // "CUTOFF": lpx_bounded_dual_run3 / lpx_bounded_node2 with LPX_BDUAL_CUTOFF only
        public const int E_GE_PRESENT = -10, E_NEG_RHS = -11, E_REVISED_PRECOND = -12, E_SINGULAR = -13,
                         E_KNAP_SHAPE = -14, E_UNKNOWN_ALGO = -15, E_PARSE = -16;

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_abi_version();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_device_count();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_init(int device);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_last_error(byte[] buf, int len);

        // ---- X1: the incumbent exchange of a sharded search, one process per GPU (include/lpx.h lpx_comm_*): the library owns an
        //      RCCL communicator; BestObjective (Models/Branch&Bound.cs:182,191) / _bestValue (Models/BranchAndBoundKnapsack.cs:124)
        //      become one ncclAllReduce(ncclMax, ncclDouble) per level / round.  lpx_init(localGpu) first.
        public const int COMM_ID_BYTES = 128;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_comm_unique_id(byte[] id);          // rank 0
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_comm_init(int rank, int world, byte[] id);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_comm_init_tcp(int rank, int world, [MarshalAs(UnmanagedType.LPUTF8Str)] string host, int port);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_comm_allreduce_max(double* vals, int count);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_comm_info(out int rank, out int world, out long allreduces, out double allreduceMs, out int rcclVersion);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_comm_destroy();

        // ---- loop-level entry points: the reference keeps its own model preparation and reports (INTEGRATION.md section 2) ----
        // replaces the while(true) of PrimalSimplex.Solve, Models/PrimalSimplex.cs:92-124
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_primal_tableau(double* T, int R, int C, int* basis, double eps, int maxIter,
                                                    LpxPivotCb cb, IntPtr user, out LpxStats st);
        // replaces ForceDualFeasibility + the loop of DualSimplex.Solve, Models/DualSimplex.cs:24,36-113
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_dual_tableau(double* T, int R, int C, int* basis, double eps, double ratioTol,
                                                  int fdfGuard, int maxIter, int cleanup, LpxPivotCb cb, IntPtr user, out LpxStats st);
        // replaces the for-loop of RevisedPrimalSimplex.Solve, Models/RevisedPrimalSimplex.cs:58-142
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_revised_solve(double* A, int m, int n, double* c, double* b, int* Bidx, int* Nidx,
                                                   double* xB, out double z, double eps, int maxIter,
                                                   LpxPivotCb cb, IntPtr user, out LpxStats st);
        // batched ComputeRelaxation, Models/BranchAndBoundKnapsack.cs:431-491
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_knapsack_create(double* profit, double* weight, int n, double cap, out IntPtr k);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_knapsack_destroy(IntPtr k);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_knapsack_relax_batch(IntPtr k, int count, int* off, int* fixIdx, sbyte* fixVal,
                                                          double* profit, double* weight, int* fracIdx, double* fracVal);

        // ---- model-level entry point: ILPAlgorithm.Solve as dispatched by LPSolver.Solve (Models/LPSolver.cs:16-59) ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_default_solve_opts(out LpxSolveOpts o);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve(ref LpxProblem p, [MarshalAs(UnmanagedType.LPUTF8Str)] string algorithm,
                                           ref LpxSolveOpts o, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_result_free(ref LpxResult r);

        // ---- ranging of the final tableau (Primal / Dual Simplex), include/lpx.h; free both records afterwards ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_ranging(ref LpxProblem p, [MarshalAs(UnmanagedType.LPUTF8Str)] string algorithm,
                                                   ref LpxSolveOpts o, out LpxResult result, out LpxRanging ranging);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_ranging_free(ref LpxRanging r);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_ranging(IntPtr t, double eps, double* colInc, int* colIncAt, double* colDec, int* colDecAt,
                                                     double* rowInc, int* rowIncAt, double* rowDec, int* rowDecAt,
                                                     double* minRhs, double* minDj);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_ranging_pairs(IntPtr t, double eps, int K, int* a, int* b,
                                                           double* inc, int* incAt, double* dec, int* decAt);

        // ---- GMI cutting planes on the device (not in the reference), include/lpx.h ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_default_cut_opts(out LpxCutOpts o);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_cuts(ref LpxProblem p, ref LpxSolveOpts o, ref LpxCutOpts co, out LpxResult result);
        // srcRows: [cuts_per_round] or null; purgedCols: [C-1 - firstCutCol] (the cut columns before the round, NOT max_active) or null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_gmi_round(IntPtr t, byte* isInt, int nMask, int firstCutCol, ref LpxCutOpts o,
                                                       out int nAdded, int* srcRows, out int nPurged, int* purgedCols);

        // warm post-optimal edits of a device tableau (include/lpx.h, lpx_postopt.hip; not in the reference)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_rhs_update(IntPtr t, int K, int* cols, double* v);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_objective_update(IntPtr t, int K, int* rows, double* w, int Kd, int* dcols, double* dd);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_add_column(IntPtr t, int K, int* cols, double* v, double obj);
        // baseRow: [C+1] in the new shape
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_add_row(IntPtr t, int K, int* rows, double* w, double* baseRow);
        // the model-level session: what SensitivityAnalysis.ApplyChange (Models/SensitivityAnalysis.cs:78-107) leaves to a re-solve
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_default_session_opts(out LpxSessionOpts o);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_open(ref LpxProblem p, ref LpxSessionOpts o, out IntPtr session, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_set_rhs(IntPtr s, int K, int* cons, double* b, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_set_cost(IntPtr s, int K, int* vars, double* c, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_add_variable(IntPtr s, double c, double* a, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_add_constraint(IntPtr s, double* a, int rel, double b, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_ranging(IntPtr s, out LpxRanging rg);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_session_shape(IntPtr s, out int nVars, out int nCons);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_session_close(IntPtr s);

        // ---- bounded-variable primal simplex (not in the reference), include/lpx.h: bounds beside the tableau, no bound rows ----
        // lower / upper: [n] or null (0 / +inf); info: receives flip / ub / lower of the final tableau
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bounded(ref LpxProblem p, double* lower, double* upper, ref LpxSolveOpts o,
                                                   out LpxResult result, out LpxBoundedInfo info);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bounded_info_free(ref LpxBoundedInfo info);
        // ub: [C-1], +inf = unbounded; null with ncols = 0 removes the bounds
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_set_bounds(IntPtr t, int ncols, double* ub);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_bound_flags(IntPtr t, byte* flip);
        // opts: an lpx_run_opts or IntPtr.Zero for the defaults; trace rows: (r, q) pivot, (-2 - r, q) pivot to the upper bound, (-1, q) flip
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_run(IntPtr t, IntPtr opts, LpxPivotCb cb, IntPtr user, out LpxStats st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_bounded_counts(IntPtr t, long* counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_bounded_solution(IntPtr t, int nvars, double* x, out double z, byte* atUpper);

        // ---- bounded dual simplex and bound changes on a solved tableau (not in the reference), include/lpx.h ----
        // lo / ub / flip: [C-1] each or null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_bound_state(IntPtr t, double* lo, double* ub, byte* flip);
        // new absolute bounds lower[k] <= x_cols[k] <= upper[k], in place: only the RHS column moves
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_change_bounds(IntPtr t, int K, int* cols, double* lower, double* upper);
        // trace rows: (r, q) basic variable below zero, (-2 - r, q) basic variable above its upper bound
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_dual_run(IntPtr t, IntPtr opts, LpxPivotCb cb, IntPtr user, out LpxStats st);
        // a bounded session: lpx_solve_bounded that keeps its handle, then bound edits of original variables (0-based)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_open(ref LpxProblem p, double* lower, double* upper, ref LpxSolveOpts o,
                                                  out IntPtr session, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_set_bounds(IntPtr s, int K, int* vars, double* lower, double* upper, out LpxResult result);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bounded_close(IntPtr s);
        // branch and bound by bound changes on one device tableau (LPX_BDUAL_SKIP_FIXED = 1: fixed columns do not enter)
        public const int LPX_BDUAL_SKIP_FIXED = 1;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_dualize(IntPtr t, double eps, long* counts);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_dual_run2(IntPtr t, IntPtr opts, int flags, LpxPivotCb cb, IntPtr user, out LpxStats st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_branch_pick(IntPtr t, int nint, byte* is_int, double tol, out LpxBranchPick pick);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_node(IntPtr t, int K, int* cols, double* lower, double* upper, IntPtr opts,
                                                  int nint, byte* is_int, double tol, out LpxNodeRecord record);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                       long max_nodes, out LpxResult result, out LpxBnbBoundedInfo info);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern void lpx_bnb_bounded_info_free(ref LpxBnbBoundedInfo info);
        // long-step ratio test, objective cutoff and dual start (flags of lpx_bounded_dual_run3; search_flags of lpx_solve_bnb_bounded2)
        public const int LPX_BDUAL_LONG_STEP = 2;
        public const int LPX_BDUAL_CUTOFF = 4;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_dual_run3(IntPtr t, IntPtr opts, int flags, double cutoff, LpxPivotCb cb, IntPtr user, out LpxStats st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_node2(IntPtr t, int K, int* cols, double* lower, double* upper, IntPtr opts, int flags, double cutoff,
                                                   int nint, byte* is_int, double tol, out LpxNodeRecord record);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded2(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, out LpxResult result, out LpxBnbBoundedInfo info);
        // the on-chip form of a node: one launch per node with the tableau in LDS (form of lpx_bounded_node3; node_form of lpx_solve_bnb_bounded3)
        public const int LPX_NODE_LAUNCHES = 0;
        public const int LPX_NODE_ONCHIP = 1;
        public const int LPX_NODE_AUTO = 2;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_bounded_node_fits(int R, int C);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_node3(IntPtr t, int K, int* cols, double* lower, double* upper, IntPtr opts, int flags, double cutoff,
                                                   int nint, byte* is_int, double tol, int form, out LpxNodeRecord record);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded3(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int node_form, out LpxResult result, out LpxBnbBoundedInfo info);
        // a batch of on-chip nodes per launch (handles: W IntPtr of lpx_tableau_create / _clone; records: B LpxNodeRecord) and the search by W divers
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_clone(IntPtr src, out IntPtr clone);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_node_batch_create(int W, IntPtr* handles, out IntPtr batch);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_node_batch_destroy(IntPtr batch);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_run(IntPtr batch, int B, int* slot, int* K, int* cols, double* lower, double* upper, IntPtr opts,
                                                    int flags, double* cutoff, int nint, byte* is_int, double tol, LpxNodeRecord* records, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded4(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, out LpxResult result,
                                                        out LpxBnbBoundedInfo info, out LpxBnbDiversInfo dinfo);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bnb_divers_info_free(ref LpxBnbDiversInfo dinfo);
        // the plunge: records is [B * D], entry-major; steps and rc are [B]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_plunge(IntPtr batch, int B, int* slot, int* K, int* cols, double* lower, double* upper, IntPtr opts,
                                                       int flags, double* cutoff, double* prune, int* depth, int D, int nint, byte* is_int,
                                                       double tol, LpxNodeRecord* records, int* steps, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded5(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, int plunge, out LpxResult result,
                                                        out LpxBnbBoundedInfo info, out LpxBnbDiversInfo dinfo, out LpxBnbPlungeInfo pinfo);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bnb_plunge_info_free(ref LpxBnbPlungeInfo pinfo);
        // strong branching by probes: records is [2 * cand_max] / [B * 2 * cand_max], entry-major; branching 0 = most fractional, 1 = strong
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_probe(IntPtr tableau, IntPtr opts, int flags, double cutoff, double prune, int nint, byte* is_int,
                                                   double tol, int cand_max, int probe_iter, out LpxProbeHead head, LpxProbeRecord* records);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_run_probe(IntPtr batch, int B, int* slot, int* K, int* cols, double* lower, double* upper, IntPtr opts,
                                                          int flags, double* cutoff, double* prune, int nint, byte* is_int, double tol,
                                                          int cand_max, int probe_iter, LpxNodeRecord* records, LpxProbeHead* heads,
                                                          LpxProbeRecord* probes, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded6(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, int branching, int cand_max,
                                                        int probe_iter, out LpxResult result, out LpxBnbBoundedInfo info,
                                                        out LpxBnbDiversInfo dinfo, out LpxBnbStrongInfo sinfo);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bnb_strong_info_free(ref LpxBnbStrongInfo sinfo);
        // the stall guard: stall_events = 0 is lpx_bounded_node3 / lpx_node_batch_run / lpx_solve_bnb_bounded4; guard / guards may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_node4(IntPtr tableau, int K, int* cols, double* lower, double* upper, IntPtr opts, int flags,
                                                   double cutoff, int stall_events, int nint, byte* is_int, double tol, int form,
                                                   out LpxNodeRecord record, LpxGuardRecord* guard);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_run2(IntPtr batch, int B, int* slot, int* K, int* cols, double* lower, double* upper, IntPtr opts,
                                                     int flags, double* cutoff, int stall_events, int nint, byte* is_int, double tol,
                                                     LpxNodeRecord* records, LpxGuardRecord* guards, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded7(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, int stall_events, out LpxResult result,
                                                        out LpxBnbBoundedInfo info, out LpxBnbDiversInfo dinfo, out LpxBnbGuardInfo ginfo);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bounded_dual(ref LpxProblem p, double* lower, double* upper, int flags, ref LpxSolveOpts o,
                                                        out LpxResult result, out LpxBoundedInfo info);
        // ---- the bounded primal loop on chip: one launch per LP, a batch per launch.  form / root_form: LPX_NODE_* ----
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_run2(IntPtr t, IntPtr opts, int form, LpxPivotCb cb, IntPtr user, out LpxStats st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_primal(IntPtr batch, int B, int* slot, IntPtr opts, LpxPrimalRecord* records, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bounded2(ref LpxProblem p, double* lower, double* upper, ref LpxSolveOpts o, int form,
                                                    out LpxResult result, out LpxBoundedInfo info);
        // problems / lowers / uppers: [count] pointers (lowers, uppers and their entries may be null); results / infos: [count]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bounded_batch(int count, LpxProblem** problems, double** lowers, double** uppers, ref LpxSolveOpts o,
                                                         LpxResult* results, LpxBoundedInfo* infos);
        // packed batches: arrays in, ONE launch, arrays out; opts: lpx_run_opts or IntPtr.Zero, st may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_packed_fits(int m, int n);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_packed(ref LpxPackedModels models, IntPtr opts, ref LpxPackedResults results, LpxStats* st);
        // the same by a dual start: >= rows and negative right-hand sides; flags: 0 or LPX_BDUAL_LONG_STEP (2)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_packed_dual(ref LpxPackedDualModels models, int flags, IntPtr opts, ref LpxPackedDualResults results,
                                                       LpxStats* st);
        // right-hand-side scenarios warm-started from one solved base: open keeps the solved tableau on the device (handle: an opaque
        // pointer, null unless the base ends LPX_OPTIMAL; baseOut may be null), solve re-solves count right-hand sides ([count][m]) in ONE launch
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_packed_base_open(ref LpxPackedBaseModel model, int flags, IntPtr opts, LpxPackedDualResults* baseOut,
                                                      out IntPtr handle);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_packed_base_solve(IntPtr handle, int count, double* b, int flags, IntPtr opts, ref LpxPackedDualResults results,
                                                       LpxStats* st);
        // cost scenarios from the same base: c [count][n], b [count][m] or null (every scenario keeps the base's right-hand side);
        // oPrimal / oDual: the options of the primal and of the dual loop, or IntPtr.Zero for each loop's defaults
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_packed_base_solve_costs(IntPtr handle, int count, double* c, double* b, int flags, IntPtr oPrimal, IntPtr oDual,
                                                             ref LpxPackedCostResults results, LpxStats* st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_packed_base_close(IntPtr handle);
        // packed batches of small integer programs: the whole branch and bound of every model in ONE launch
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_packed_bnb(ref LpxPackedBnbModels models, ref LpxPackedBnbOpts opts, ref LpxPackedBnbResults results,
                                                      LpxStats* st);
        // integer programs with >= rows: the search from a dual start, host-driven and packed (options, record and results of lpx_solve_packed_bnb)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded_dual(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                            long max_nodes, int search_flags, int node_form, out LpxResult result, out LpxBnbBoundedInfo info);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_packed_bnb_dual(ref LpxPackedBnbDualModels models, ref LpxPackedBnbOpts opts, ref LpxPackedBnbResults results,
                                                           LpxStats* st);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded8(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, int stall_events, int root_form,
                                                        out LpxResult result, out LpxBnbBoundedInfo info, out LpxBnbDiversInfo dinfo,
                                                        out LpxBnbGuardInfo ginfo);

        // GMI cuts on a handle with bounds and cut-and-branch at the bounded root (include/lpx.h; lpx_cuts.hip).  LPX_CUTLOOP_*: 0 integral,
        // 1 stalled, 2 rounds used up, 3 infeasible, 4 iteration limit, 5 another status.  rootCuts null: lpx_solve_bnb_bounded8 bit for bit
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_gmi_round_bounded(IntPtr t, byte* isInt, int nMask, int firstCutCol, ref LpxCutOpts o,
                                                               out int nAdded, int* srcRows, out int nPurged, int* purgedCols);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_cut_loop(IntPtr t, byte* isInt, int nMask, int firstCutCol, int nint, byte* nodeIsInt,
                                                      ref LpxCutOpts co, IntPtr opts, int flags, int form, ref LpxCutLoopRecord rec);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded9(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                        long max_nodes, int search_flags, int divers, int stall_events, int root_form,
                                                        LpxCutOpts* root_cuts, out LpxResult result, out LpxBnbBoundedInfo info,
                                                        out LpxBnbDiversInfo dinfo, out LpxBnbGuardInfo ginfo, out LpxBnbCutInfo cinfo);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_bnb_cut_info_free(ref LpxBnbCutInfo cinfo);

        // reduced-cost bound tightening (include/lpx.h; lpx_bounded_fix.hip).  fix_bound = -inf: lpx_bounded_node4 / lpx_node_batch_run2 bit
        // for bit; tighten = 0: lpx_solve_bnb_bounded9 bit for bit
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_bounded_node5(IntPtr tableau, int K, int* cols, double* lower, double* upper, IntPtr opts, int flags,
                                                   double cutoff, int stall_events, double fix_bound, int nint, byte* is_int, double tol, int form,
                                                   out LpxNodeRecord record, LpxGuardRecord* guard, LpxFixList* fix);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_node_batch_run3(IntPtr batch, int B, int* slot, int* K, int* cols, double* lower, double* upper, IntPtr opts,
                                                     int flags, double* cutoff, int stall_events, double* fix_bound, int nint, byte* is_int, double tol,
                                                     LpxNodeRecord* records, LpxGuardRecord* guards, LpxFixList* fixes, int* rc);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_solve_bnb_bounded10(ref LpxProblem p, double* lower, double* upper, byte* is_int, ref LpxSolveOpts o,
                                                         long max_nodes, int search_flags, int divers, int stall_events, int root_form,
                                                         LpxCutOpts* root_cuts, int tighten, out LpxResult result, out LpxBnbBoundedInfo info,
                                                         out LpxBnbDiversInfo dinfo, out LpxBnbGuardInfo ginfo, out LpxBnbCutInfo cinfo,
                                                         out LpxBnbFixInfo finfo);

        // ---- branch-and-bound node and child assembly on device handles, the parent store and the batched read-back, include/lpx.h ----
        // any of R / C / ld may be null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_shape(IntPtr t, int* R, int* C, int* ld);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_tableau_set_shape(IntPtr t, int R, int C);
        // the root tableau (its snapshot if one was taken) plus ncuts unit rows: coef[k] at var[k], the signed zero zero[k] elsewhere, rhs[k]
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_build_node(IntPtr node, IntPtr root, int ncuts, int* var, double* coef, double* zero, double* rhs);
        // cutOff: [count + 1], cutOff[0] = 0; node i gets the rows [cutOff[i], cutOff[i + 1]) of the flattened arrays
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_build_nodes(IntPtr* nodes, IntPtr root, int count, int* cutOff, int* var, double* coef, double* zero, double* rhs);
        // the parent's final tableau plus the row of x_var <= bound (isGe = 0) or x_var >= bound (isGe = 1); x_var is basic in rowOfVar
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_build_child(IntPtr child, IntPtr parent, int var, int rowOfVar, int isGe, double bound);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_store_create(int Rcap, int Ccap, out IntPtr store);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern void lpx_store_destroy(IntPtr store);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_store_save(IntPtr store, IntPtr t, out int slot);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_store_release(IntPtr store, int slot);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)] public static extern int lpx_store_save_multi(IntPtr* stores, IntPtr* ts, int count, int* slots);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_build_child_from_store(IntPtr child, IntPtr store, int slot, int var, int rowOfVar, int isGe, double bound);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_tableau_build_children_from_store(IntPtr* children, IntPtr* stores, int* slots, int count,
                                                                       int* var, int* rowOfVar, int* isGe, double* bound);
        // x: count x nvars, z: [count], basisOut: count x basisStride or null
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int lpx_multi_solution(IntPtr* ts, int count, int nvars, double* x, double* z, int* basisOut, int basisStride);

        public static string LastError()
        {
            var b = new byte[1024];
            lpx_last_error(b, b.Length);
            int len = Array.IndexOf(b, (byte)0);
            return System.Text.Encoding.UTF8.GetString(b, 0, len < 0 ? b.Length : len);
        }
    }
}
