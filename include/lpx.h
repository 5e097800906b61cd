/*
 * lpx.h -- C ABI of liblpx.so, the MI355X (gfx950) simplex / branch-and-bound engine.
 *
 * This is the drop-in boundary for the hot path of Jellyman750/Linear_Programming_Solver_LPR381.
 * The reference is managed C# with no native interface of its own; each entry point below names
 * the reference loop it replaces (paths relative to Linear_Programming_Solver/ in the reference)
 * and is what a P/Invoke shim inside the reference's ILPAlgorithm implementations
 * (Models/IPLAlgorithm.cs:5-8) would bind -- see INTEGRATION.md for that shim.
 *
 * Conventions
 *   - plain C types only; every buffer is caller-owned unless a *_free function is named;
 *   - tableaux are row-major `double[R*C]` exactly as C#'s `double[R,C]` (zero-copy under
 *     `fixed (double* p = T)`): R = m+1 rows with the objective row LAST, C = n+m+1 columns
 *     with the RHS column LAST (Models/PrimalSimplex.cs:179-203);
 *   - return value >= 0 is a solver status, < 0 an error; lpx_last_error() has the message;
 *   - nothing here falls back to the CPU: without a gfx950 device every compute entry point
 *     returns LPX_EDEVICE.
 */
#ifndef LPX_H
#define LPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPX_ABI_VERSION 1

/* ---- status (soft outcomes the reference reports as text) and errors (its exceptions) ------- */
enum {
    LPX_OPTIMAL    = 0,   /* "OPTIMAL"    Models/PrimalSimplex.cs:126 */
    LPX_UNBOUNDED  = 1,   /* "UNBOUNDED"  Models/PrimalSimplex.cs:102-106 */
    LPX_INFEASIBLE = 2,   /* "INFEASIBLE" Models/DualSimplex.cs:92-96 */
    LPX_ITER_LIMIT = 3,   /* exception "Iteration limit exceeded." Models/PrimalSimplex.cs:95-96 */
    LPX_RUNNING    = 4,   /* internal: loop not finished */
    LPX_CUTOFF     = 5,   /* "CUTOFF": lpx_bounded_dual_run3 / _node2 with LPX_BDUAL_CUTOFF stopped at T[m,Cm] <= cutoff; no other
                             entry point returns it */
    /* outcomes of the cutting-plane consumers (lpx_result.status for "Cutting Plane" / "Revised Cutting Plane";
       LPX_CUT_INTEGER / LPX_CUT_INCOMPLETE also for "GMI Cutting Plane", lpx_solve_cuts) */
    LPX_CUT_INTEGER     = 0,  /* "Status: OPTIMAL INTEGER" Models/CuttingPlane.cs:91-104, CuttingPlaneRevised.cs:49-57 */
    LPX_CUT_INCOMPLETE  = 10, /* 50 iterations used up, Models/CuttingPlane.cs:132-137, CuttingPlaneRevised.cs:70-77 */
    LPX_CUT_ERROR       = 11, /* "Error: ..." summaries, Models/CuttingPlane.cs:42-74,116-124 */
    LPX_CUT_NOT_OPTIMAL = 12, /* Models/CuttingPlaneRevised.cs:27-35 */
    LPX_EINVAL     = -1,
    LPX_EDEVICE    = -2,  /* no usable gfx950 device / HIP failure */
    LPX_ENOMEM     = -3,
    LPX_E_GE_PRESENT      = -10, /* Models/PrimalSimplex.cs:70 */
    LPX_E_NEG_RHS         = -11, /* Models/PrimalSimplex.cs:75 */
    LPX_E_REVISED_PRECOND = -12, /* Models/RevisedPrimalSimplex.cs:21 */
    LPX_E_SINGULAR        = -13, /* Models/RevisedPrimalSimplex.cs:426 */
    LPX_E_KNAP_SHAPE      = -14, /* Models/BranchAndBoundKnapsack.cs:66-69 */
    LPX_E_UNKNOWN_ALGO    = -15, /* Models/LPSolver.cs:39-42 */
    LPX_E_PARSE           = -16  /* Models/LPParser.cs exceptions */
};

/* Per-pivot event, fired on the calling thread between batches, in pivot order.  Replaces the
 * reference's per-iteration `updatePivot(text, bool[,])` callback (Models/PrimalSimplex.cs:113-121),
 * which formats the whole tableau; hosts that want to render it call lpx_tableau_download. */
typedef void (*lpx_pivot_cb)(void* user, int iter, int row, int col);

typedef struct lpx_stats {
    int64_t pivots;          /* completed pivots */
    int64_t launches;        /* kernel launches enqueued (including early-exit ones) */
    double  loop_ms;         /* host wall time of the device-resident loop (no H2D/D2H) */
    double  h2d_ms;          /* upload time of one-shot entry points */
    double  d2h_ms;
    double  update_ms_sum;   /* profile mode only: sum of HIP-event durations of the kernel that streams the tableau (the rank-1
                              * update; the fused update + select launch of lpx_primal_run) */
    int64_t update_launches; /* profile mode only: launches included in update_ms_sum */
    int64_t fdf_pivots;      /* dual: pivots spent in ForceDualFeasibility */
    int64_t cleanup_pivots;  /* dual, repaired mode: pivots of the primal clean-up phase */
} lpx_stats;

typedef struct lpx_run_opts {
    double eps;        /* Eps, 1e-9 (Models/PrimalSimplex.cs:55, Models/DualSimplex.cs:13) */
    double ratio_tol;  /* hysteresis of the ratio scans: 1e-9 primal (:235), 1e-12 dual (:85,:220) */
    int    max_iter;   /* 10000 (Models/PrimalSimplex.cs:54, Models/DualSimplex.cs:39) */
    int    fdf_guard;  /* dual: ForceDualFeasibility guard, 100 (Models/DualSimplex.cs:202) */
    int    cleanup;    /* dual: 1 = repaired-mode primal clean-up phase */
    int    batch;      /* pivots enqueued between host polls of the device state; 0 = default */
    int    use_graph;  /* 1 = replay a captured hipGraph per batch, 0 = eager launches */
    int    profile;    /* 1 = eager, every update kernel bracketed by HIP events (roofline leg) */
    int    resident;   /* primal loop with the whole tableau resident in LDS (one persistent workgroup per CU,
                          csrc/lpx_resident.hip) when it fits the chip: 0 = automatic, 1 = require it
                          (LPX_EINVAL when the tableau does not fit), -1 = never (streaming kernels) */
} lpx_run_opts;

void lpx_default_opts(lpx_run_opts* o, int dual);

/* ---- library / device ----------------------------------------------------------------------- */
int         lpx_abi_version(void);
int         lpx_device_count(void);              /* 0 when no GPU is visible */
int         lpx_init(int device);                /* binds this process to one GPU (one process per GPU) */
int         lpx_last_error(char* buf, int len);  /* copies the last error message of this thread */
int         lpx_device_name(char* buf, int len);

/* ---- X1: the incumbent exchange between the processes of a sharded search (one process per GPU) ------------------
 * Replaces, for a node queue sharded over the GPUs of one node, the compare-and-update of the single incumbent field the
 * reference keeps (`BestObjective`, Models/Branch&Bound.cs:182,191; `_bestValue`, Models/BranchAndBoundKnapsack.cs:124,
 * 157-160): ONE all-reduce(MAX) over FP64 per level / per round, RCCL over xGMI (ncclAllReduce, ncclMax, ncclDouble) on a
 * communicator the library owns.  RCCL is bound at run time (dlopen of librccl.so.1; LPX_RCCL_LIB overrides the path), so
 * single-GPU hosts need no RCCL.  Call after lpx_init(local GPU).  While a communicator exists, lpx_solve uses it for every
 * sharded search whose lpx_solve_opts.allreduce_max is NULL (opts.rank / opts.world must then equal the communicator's). */
#define LPX_COMM_ID_BYTES 128
int lpx_comm_unique_id(uint8_t* id /* [LPX_COMM_ID_BYTES] */);   /* rank 0; the host ships the bytes to the other ranks */
int lpx_comm_init(int rank, int world, const uint8_t* id);       /* collective over all ranks: ncclCommInitRank */
/* The same for hosts without a side channel: rank 0 serves the id on host:port (TCP), the others fetch it there. */
int lpx_comm_init_tcp(int rank, int world, const char* host, int port);
int lpx_comm_allreduce_max(double* vals, int count);             /* MAX over ranks, in place (host buffer) */
/* rank = -1 / world = 0 when no communicator exists; counters since lpx_comm_init.  Any pointer may be NULL. */
int lpx_comm_info(int* rank, int* world, int64_t* allreduces, double* allreduce_ms, int* rccl_version);
int lpx_comm_destroy(void);

/* ---- device-resident tableau ---------------------------------------------------------------- */
/* HBM layout: row-major with the leading dimension padded to a multiple of 16 doubles (128 B) so
 * that every row starts on a cache line and 16-byte vector accesses are aligned even for odd C. */
typedef struct lpx_tableau lpx_tableau;

int  lpx_tableau_create(int R, int C, lpx_tableau** out);
void lpx_tableau_destroy(lpx_tableau* t);
int  lpx_tableau_upload(lpx_tableau* t, const double* T, const int32_t* basis /* [R-1] or NULL */);
int  lpx_tableau_download(lpx_tableau* t, double* T, int32_t* basis /* may be NULL */);
int  lpx_tableau_snapshot(lpx_tableau* t);       /* keep a device copy of the current tableau+basis */
int  lpx_tableau_restore(lpx_tableau* t);        /* D2D restore from the snapshot, resets the loop state */
int  lpx_tableau_device_ptr(lpx_tableau* t, void** dptr, int* ld);
int  lpx_tableau_trace(lpx_tableau* t, int32_t* trace /* [2*cap] */, int cap, int* n);
int  lpx_tableau_shape(const lpx_tableau* t, int* R, int* C, int* ld);
/* A handle created for (Rcap, Ccap) can hold any smaller tableau: the kernels read the live shape from a
 * device record, so one handle (and its captured hipGraph) serves every depth of a B&B tree. */
int  lpx_tableau_set_shape(lpx_tableau* t, int R, int C);
/* 1 if the last lpx_primal_run on this handle swept a compact tableau without the basic columns (streamed handles, long runs), else 0 */
int  lpx_tableau_last_run_compact(const lpx_tableau* t);

/* The hot loops.  Each iteration is two launches on one stream:
 *   select  -- ChooseEntering + ChooseLeaving (+ pivot-row normalisation and pivot-column snapshot)
 *   update  -- the rank-1 Gauss-Jordan update T[i,:] -= T[i,q] * T[r,:]  (i != r)
 * or, for lpx_primal_run without a per-pivot callback, ONE: the update written out of place into a second tableau buffer
 * the library keeps beside the handle's own, with the next pivot's select in the same grid (the result is brought back
 * into the handle's buffer before the call returns; LPX_FUSED_PIVOT=0 in the environment keeps the two-launch form).  */

/* PrimalSimplex.Solve's while(true), Models/PrimalSimplex.cs:92-124
 * (ChooseEntering :205-220, ChooseLeaving :222-243, Pivot :245-257). */
int lpx_primal_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st);

/* DualSimplex.Solve steps 3 and 5, Models/DualSimplex.cs:24 + :36-113
 * (ForceDualFeasibility :195-228, leaving row :45-55, entering column :76-91, Pivot :232-246). */
int lpx_dual_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st);

/* Pivot (Models/PrimalSimplex.cs:245-257) on caller-chosen positions: for k in [0,count):
 * r = rows[k]; q = first column >= cols[k] (wrapping) with |T[r,q]| >= thresh; pivot(r,q).
 * chosen[k] = q or -1.  The headline rank-1-update benchmark and the bitwise kernel parity tests. */
int lpx_forced_pivots_run(lpx_tableau* t, const int32_t* rows, const int32_t* cols, int count,
                          double thresh, int32_t* chosen, const lpx_run_opts* o, lpx_stats* st);

/* x[basis[i]] = T[i,last] for basis[i] < nvars, *z = T[m,last] (FinalizeReport,
 * Models/PrimalSimplex.cs:130-138) without downloading the tableau. */
int lpx_tableau_solution(lpx_tableau* t, int nvars, double* x, double* z);

/* Node assembly on the device: `node` becomes the tableau
 * BuildTableau (Models/PrimalSimplex.cs:179-203) would produce for the root model plus `ncuts` unit
 * rows (Models/Branch&Bound.cs:233-248); the node handle needs capacity for root shape + ncuts and takes
 * that shape.  Row k has coef[k] at column var[k], zero[k] (a signed zero: the
 * reference's `A[j] *= -1` turns 0 into -0) elsewhere, its own slack, and rhs[k].  `root` holds the
 * prepared root tableau (its snapshot if one was taken) and is not modified.  Stream-ordered with
 * the run that follows on `node`. */
int lpx_tableau_build_node(lpx_tableau* node, const lpx_tableau* root, int ncuts, const int32_t* var,
                           const double* coef, const double* zero, const double* rhs);

/* The same for a group of nodes in one launch: node i gets the branching rows [cut_off[i], cut_off[i+1]) of the flattened
 * arrays (cut_off has count + 1 entries, cut_off[0] = 0).  Returns when the nodes are built. */
int lpx_tableau_build_nodes(lpx_tableau** nodes, const lpx_tableau* root, int count, const int32_t* cut_off,
                            const int32_t* var, const double* coef, const double* zero, const double* rhs);

/* Warm start of a branch-and-bound child (NOT what the reference does -- it re-solves every
 * node from the slack basis, Models/Branch&Bound.cs:148): `child` becomes `parent`'s final tableau plus the row
 * of `x_var <= bound` (is_ge = 0) or `x_var >= bound` (is_ge = 1) written in the parent's basis, where
 * `row_of_var` is the row in which x_var is basic.  The result is dual feasible; run it with lpx_dual_run /
 * lpx_multi_run and fdf_guard = 0.  `child` needs capacity for the parent's shape + 1. */
int lpx_tableau_build_child(lpx_tableau* child, lpx_tableau* parent, int var, int row_of_var, int is_ge, double bound);
int lpx_tableau_basis(lpx_tableau* t, int32_t* basis /* [R-1] */);
int lpx_tableau_solution2(lpx_tableau* t, int nvars, double* x, double* z, int32_t* basis_out /* [R-1] or NULL */);
/* The same for a batch of solved nodes in ONE launch + one wait (the reads of FinalizeReport, Models/PrimalSimplex.cs:135-138,
 * for every node of a branch-and-bound group): x is count x nvars, z has count entries, basis_out (or NULL) count x basis_stride. */
int lpx_multi_solution(lpx_tableau** ts, int count, int nvars, double* x, double* z, int32_t* basis_out, int basis_stride);
/* Parent store: a solved node parks its final tableau in a slab slot (one D2D copy) and gives its handle
 * back; its children are assembled from the slot.  Slots are sized for one capacity class (same Rcap/Ccap as
 * the handles that use the store) and allocated 128 at a time. */
typedef struct lpx_store lpx_store;
int  lpx_store_create(int Rcap, int Ccap, lpx_store** out);
void lpx_store_destroy(lpx_store* s);   /* its device chunks stay with the process for the next store (up to LPX_STORE_CACHE_GB, default 64) */
int  lpx_store_save(lpx_store* s, lpx_tableau* t, int* slot_out);
int  lpx_store_release(lpx_store* s, int slot);
/* The same for a batch of solved nodes (stores[i] / ts[i] / slots[i]): all copies are enqueued, then one wait per stream. */
int  lpx_store_save_multi(lpx_store** stores, lpx_tableau** ts, int count, int* slots);
int  lpx_tableau_build_child_from_store(lpx_tableau* child, lpx_store* s, int slot, int var, int row_of_var,
                                        int is_ge, double bound);

/* The same for a group of children in one launch (child i from stores[i] / slots[i]); returns when they are built. */
int  lpx_tableau_build_children_from_store(lpx_tableau** children, lpx_store** stores, const int* slots, int count,
                                           const int32_t* var, const int32_t* row_of_var, const int32_t* is_ge, const double* bound);

/* Branch-and-bound node batches: runs `count` independent tableaux to completion,
 * interleaving their batches on their own streams so that small node LPs overlap on one GPU.
 * dual[i] selects lpx_dual_run (1) or lpx_primal_run (0) semantics; statuses[i] gets each status. */
int lpx_multi_run(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* primal_opts,
                  const lpx_run_opts* dual_opts, int* statuses, lpx_stats* stats /* [count] or NULL */);

/* The same for a rolling batch: returns as soon as at most `min_active` runs are unfinished and reports those as LPX_RUNNING;
 * handed in again (with fresh tableaux beside them) they continue where they stopped.  Batched streaming kernels only. */
int lpx_multi_run_some(lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* primal_opts,
                       const lpx_run_opts* dual_opts, int* statuses, lpx_stats* stats /* [count] or NULL */, int min_active);

/* The same in two halves, for hosts that keep TWO OR MORE rolling batches (slots 0 .. LPX_ASYNC_SLOTS - 1) so that one pivots while
 * another is read back, decided on and refilled: _begin enqueues `steps` pivots (rounded up to even) of every run of the batch -- fresh
 * tableaux and runs a previous window left as LPX_RUNNING alike -- on the slot's own stream and returns at once; _end waits for
 * that window and reports as lpx_multi_run_some does (LPX_RUNNING = unfinished, hand it in again).  Between the two calls the
 * batch's handles must not be touched.  _begin returns 1 (nothing enqueued) when the one-launch-per-step kernels cannot take
 * the batch (a second tableau buffer did not fit, profile mode): use lpx_multi_run_some then. */
#define LPX_ASYNC_SLOTS 4   /* slot = 0 .. LPX_ASYNC_SLOTS - 1 */
int lpx_multi_run_begin(int slot, lpx_tableau** ts, const int* dual, int count, const lpx_run_opts* primal_opts,
                        const lpx_run_opts* dual_opts, int steps);
int lpx_multi_run_end(int slot, int* statuses, lpx_stats* stats /* [count of the _begin] or NULL */);

/* ---- one-shot entry points on host buffers (what the C# shim binds) -------------------------- */
/* Replaces the loop of PrimalSimplex.Solve (Models/PrimalSimplex.cs:92-124) on the `double[,]`
 * built by BuildTableau (:179-203).  T and basis are updated in place. */
int lpx_primal_tableau(double* T, int R, int C, int32_t* basis, double eps, int max_iter,
                       lpx_pivot_cb cb, void* user, lpx_stats* st);
/* Replaces ForceDualFeasibility + the loop of DualSimplex.Solve (Models/DualSimplex.cs:24,:36-113). */
int lpx_dual_tableau(double* T, int R, int C, int32_t* basis, double eps, double ratio_tol,
                     int fdf_guard, int max_iter, int cleanup,
                     lpx_pivot_cb cb, void* user, lpx_stats* st);

/* ---- revised primal simplex (device-resident) ------------------------------------------------ */
/* Replaces the loop of RevisedPrimalSimplex.Solve (Models/RevisedPrimalSimplex.cs:58-142):
 * pricing  r_N = c_N - (c_B B^-1) N  (MultiplyRow :365-378, Subtract :388-393),
 * entering = first strict minimum below -Eps in Nidx LIST order (:76-83),
 * direction d = B^-1 a_q (Multiply :325-336), ratio test with 1e-12 hysteresis (:99-112),
 * basis bookkeeping Bidx[r]=q; Nidx.RemoveAt(pos); Nidx.Add(leaving) (:121-124).
 * Where the reference re-inverts B from scratch every iteration (Invert :402-456, 4m^3 flop) the
 * engine applies the mathematically equal rank-1 (product-form) update to the device-resident
 * (m+1)x(m+1) matrix [[B^-1, x_B], [c_B B^-1, z]] with the same update kernel as the tableau path:
 * same pivot sequence away from ties, objective within 1e-9 relative (DESIGN.md "Revised path").
 *
 * A: m x n row-major structural columns (the slack identity is implicit); c[n]: costs of the
 * standardised MINIMISATION (c = -C for a Max model, :153-154); b[m] >= -1e-9 (:19-21 is the
 * caller's precondition check). */
typedef struct lpx_revised lpx_revised;
int  lpx_revised_create(int m, int n, const double* A, const double* c, const double* b, lpx_revised** out);
void lpx_revised_destroy(lpx_revised* r);
int  lpx_revised_run(lpx_revised* r, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st);
/* Bidx[m]; Nidx[n] in the reference's list order; xB[m]; *z = c_B . x_B of the minimised model. */
int  lpx_revised_result(lpx_revised* r, int32_t* Bidx, int32_t* Nidx, double* xB, double* z);
int  lpx_revised_binv(lpx_revised* r, double* Binv /* [m*m] row-major */);
/* What the reference prints per iteration (BuildIterationBlock, Models/RevisedPrimalSimplex.cs:191-246), as
 * left by the LAST completed iteration: rc[n+m] = reduced cost of every column as priced at its start
 * (+inf for columns that were basic then; rN of :71 is rc gathered in that iteration's Nidx order) and
 * d[m] = B^-1 a_entering (:96).  theta* (:105) equals xB[leaveRow] after the update.  Either may be NULL. */
int  lpx_revised_iteration_view(lpx_revised* r, double* rc, double* d);
/* K7': recompute [[B^-1, x_B], [c_B B^-1, z]] from the current basis with the device Gauss-Jordan below
 * (what the reference does every iteration, :128-133).  lpx_revised_set_refactor(r, k) makes
 * lpx_revised_run do it after every k iterations (0 = only when the drift policy below asks for it, the default). */
int  lpx_revised_refactor(lpx_revised* r);
int  lpx_revised_set_refactor(lpx_revised* r, int every);
/* How lpx_revised_refactor rebuilds B^-1.  0 (default) = the reference's Invert on the device, bit for bit (:402-456).
 * 1 = fast: Newton-Schulz refinement X <- X + X (I - B X) of the maintained inverse, two dense m x m x m contractions on the
 * FP64 matrix cores (v_mfma_f64_16x16x4_f64); it rounds differently from Invert (bar: same pivots, z within 1e-9,
 * |B^-1 B - I| <= 1e-9) and falls back to mode 0 by itself when the maintained inverse is too far off to contract.
 * 2 = blocked: B inverted from scratch by lpx_invert_blocked's kernels (no bit-equality with Invert), then R = I - B B^-1 once
 * on the matrix cores; last_residual of lpx_revised_refactor_stats = max |R_ij|.  3 = fast as 1, with 2 instead of 0 as the
 * fallback (counted in fast_fallbacks).  Any other mode: LPX_EINVAL. */
int  lpx_revised_set_refactor_mode(lpx_revised* r, int mode);
/* Drift control of the product-form inverse (the reference never drifts: it re-inverts every iteration).  Every
 * `check_every` iterations lpx_revised_run evaluates two residuals on the device -- rho = max_i |(B x_B)_i - b_i| / (1 + max_i |b_i|)
 * and, for a fixed probe vector v of order one, rho2 = max_i |(B^-1 (B v))_i - v_i| / (1 + max|v|), which sees an error of B^-1 in
 * directions b does not excite (three m x m sweeps in all) -- and refactorises when max(rho, rho2) > tol.  Default: check_every = 256, tol = 1e-9; check_every = 0 switches it off.
 * lpx_revised_set_refactor(r, k > 0) replaces it by an unconditional refactorisation every k iterations. */
int  lpx_revised_set_drift_policy(lpx_revised* r, int check_every, double tol);
int  lpx_revised_residual(lpx_revised* r, double* rel /* max(rho, rho2) */, double* abs_ /* max_i |(B x_B)_i - b_i| */);
/* Counters since creation; gemm_ms / gemm_calls: HIP-event time and number of the matrix-core contractions (2 m^3 flop each)
 * of the LAST fast refactorisation.  Any pointer may be NULL. */
int  lpx_revised_refactor_stats(lpx_revised* r, int* refactors, int* fast_steps, int* fast_fallbacks, double* last_residual,
                                double* gemm_ms, int* gemm_calls);
/* Measurement: mean HIP-event duration [us] of each kernel of the engine's four-launch iteration -- us[0] rv_price (r_N = c_N - pi N,
 * MultiplyRow + Subtract :71-72), us[1] rv_pick (entering candidate :76-83, column copy :95), us[2] rv_upd_ftran (d = B^-1 a_q, Multiply
 * :96, fused with the previous pivot's update of [[B^-1, x_B]]), us[3] rv_select2 (ratio test :99-112, bookkeeping :121-124) -- over up to
 * `iters` real iterations from the handle's current basis; *measured = iterations that completed a pivot. */
int  lpx_revised_profile(lpx_revised* r, int iters, double* us /* [4] */, int* measured);
/* Invert (Models/RevisedPrimalSimplex.cs:402-456), bit for bit: Gauss-Jordan with partial pivoting on
 * [M | I]; M and inv are n x n row-major host buffers.  Returns 0 or LPX_E_SINGULAR (:426). */
int  lpx_invert(const double* M, int n, double* inv);
/* The same inverse by blocked Gauss-Jordan elimination with partial pivoting, in place on the device, almost all of its
 * 2 n^3 flop as rank-64 updates on the FP64 matrix cores.  Pivot rule as Invert (first row with the largest |a| in the
 * updated column, singular if |pivot| < 1e-9), but the rounding differs (FMA accumulation), so the result is not bitwise
 * Invert's and a matrix within rounding of the 1e-9 threshold may be decided differently.  Host buffers as lpx_invert.
 * Returns 0, LPX_E_SINGULAR ("Singular basis encountered.") or LPX_EDEVICE without a GPU.  ms: NULL, or [2] receiving the
 * HIP-event milliseconds of the panels and of the updates (this synchronises per call; NULL adds no synchronisation). */
int  lpx_invert_blocked(const double* M, int n, double* inv, double* ms);
int  lpx_revised_trace(lpx_revised* r, int32_t* trace /* [2*cap]: (leaveRow, entering) */, int cap, int* n);
/* one-shot on host buffers */
int  lpx_revised_solve(const double* A, int m, int n, const double* c, const double* b,
                       int32_t* Bidx, int32_t* Nidx, double* xB, double* z,
                       double eps, int max_iter, lpx_pivot_cb cb, void* user, lpx_stats* st);

/* ---- 0/1 knapsack branch and bound: batched bounds ------------------------------------------- */
/* Items are kept in HBM in the reference's ratio order (Models/BranchAndBoundKnapsack.cs:75-79).
 * lpx_knapsack_relax_batch evaluates ComputeRelaxation (:431-491) for `count` nodes in one launch, one
 * workgroup per node.  Node k is the list of its fixed decisions fix_idx[off[k]..off[k+1]) (ORIGINAL
 * item indices, ascending) with values fix_val (0/1) -- the reference's int[n] Assigned (:25) without
 * the undecided entries.  Outputs per node: profit (= bound), weight, the fractional item's position in
 * ratio order (-1 if none) and its fraction.  With non-negative weights a node costs one wave and a search over prefix
 * sums; a negative weight selects the scan kernel (one workgroup reads all n items per node) without any switch, as
 * LPX_KNAP_SCAN=1 does for any data (tests/test_gpu_knapsack_edges.py covers it). */
typedef struct lpx_knapsack lpx_knapsack;
int  lpx_knapsack_create(const double* profit, const double* weight, int n, double cap, lpx_knapsack** out);
void lpx_knapsack_destroy(lpx_knapsack* k);
int  lpx_knapsack_order(lpx_knapsack* k, int32_t* order /* [n]: ratio rank -> original index */);
int  lpx_knapsack_relax_batch(lpx_knapsack* k, int count, const int32_t* off, const int32_t* fix_idx,
                              const int8_t* fix_val, double* profit, double* weight, int32_t* frac_idx,
                              double* frac_val);
/* Same, plus each node's two children in the same launch: outputs have 3*count entries, slot 3k = node k itself,
 * 3k+1 / 3k+2 = node k with its fractional item (the one the search branches on, :180) additionally fixed to 0 / 1 --
 * what the best-first loop (:207-209, :267-269) asks for when it pops node k.  frac_idx = -2 in the child slots when
 * node k has no fractional item.  Needs non-negative weights (lpx_knapsack_has_prefix). */
int  lpx_knapsack_relax_batch2(lpx_knapsack* k, int count, const int32_t* off, const int32_t* fix_idx,
                               const int8_t* fix_val, double* profit, double* weight, int32_t* frac_idx,
                               double* frac_val);
int  lpx_knapsack_has_prefix(lpx_knapsack* k);
/* Device-resident node store: the best-first loop makes every node as "its parent plus one decision" (:207-209, :267-269), so
 * fixed lists never travel.  Job j derives the node `parent[j]` (-1 = the root, nothing fixed; else an id returned earlier)
 * + `item[j]` fixed to `val[j]`, keeps its list in HBM under the new id child[j], and returns what lpx_knapsack_relax_batch2
 * returns for it: slot 3j the node itself, 3j+1 / 3j+2 the node with its fractional item fixed to 0 / 1 -- whose lists are
 * stored too, under the ids child[j] + 1 / child[j] + 2 (meaningful when frac_idx[3j] >= 0).  48 bytes go to the device per
 * job instead of the whole list.  Needs non-negative weights (lpx_knapsack_has_prefix). */
int  lpx_knapsack_expand_batch(lpx_knapsack* k, int count, const int64_t* parent, const int32_t* item, const int8_t* val,
                               int64_t* child, double* profit, double* weight, int32_t* frac_idx, double* frac_val);
/* The same in two halves (the children of Models/BranchAndBoundKnapsack.cs:207-209,:267-269 evaluated AHEAD of the loop that
 * asks for them), so that the host can work while the device does: _begin enqueues the batch (ids in child[] are valid
 * at once), _finish waits for it and hands out the 3 * count results.  One batch in flight per handle. */
int  lpx_knapsack_expand_begin(lpx_knapsack* k, int count, const int64_t* parent, const int32_t* item, const int8_t* val, int64_t* child);
int  lpx_knapsack_expand_finish(lpx_knapsack* k, double* profit, double* weight, int32_t* frac_idx, double* frac_val);
/* The stored list of a node (ORIGINAL item indices ascending, values 0/1); *depth = its length. */
int  lpx_knapsack_node_list(lpx_knapsack* k, int64_t node, int32_t* idx, int8_t* val, int cap, int* depth);

/* ---- model level: the reference's plugin boundary through a C ABI ------------------------------ */
/* `ILPAlgorithm.Solve(LPProblem, Action<string,bool[,]>) -> SimplexResult` (Models/IPLAlgorithm.cs:5-8)
 * as dispatched by `LPSolver.Solve(problem, algorithmName, cb)` (Models/LPSolver.cs:16-59).  The host
 * side (model preparation, tableau construction, report text, B&B tree) is the C++ mirror in
 * csrc/host/; the loops run on the GPU.  Used by tools/lpx_cli and the Python binding. */
enum { LPX_MAX = 0, LPX_MIN = 1 };                 /* Sense, Models/PrimalSimplex.cs:8 */
enum { LPX_LE = 0, LPX_GE = 1, LPX_EQ = 2 };       /* Rel,   Models/PrimalSimplex.cs:9 */

typedef struct lpx_problem {                       /* LPProblem, Models/PrimalSimplex.cs:20-36 */
    int sense, n, m;
    const double* c;      /* [n]   C */
    const double* A;      /* [m*n] Constraints[i].A, row-major */
    const int32_t* rel;   /* [m]   Constraints[i].Relation */
    const double* b;      /* [m]   Constraints[i].B */
} lpx_problem;

typedef struct lpx_solve_opts {
    int max_iter;          /* 0 = 10000 */
    int batch;             /* 0 = default */
    int render_iterations; /* 1 = text callback receives the whole formatted tableau per pivot */
    int dual_flags;        /* 0 = faithful DualSimplex (defects D1/D2), 7 = repaired */
    int bnb_mode;          /* 0 = faithful, 1 = repaired */
    int bnb_search;        /* 0 = reference DFS, 1 = level-synchronous sharded frontier (every node re-solved from the
                              slack basis, as the reference), 2 = the same with warm-started children */
    int concurrent_nodes;  /* node LPs in flight per GPU (level search) */
    int rank, world;       /* shard of this process (level search / knapsack rounds) */
    int64_t max_nodes;     /* 0 = unlimited; sharded searches: node budget of the WHOLE job, split over the ranks */
    /* incumbent exchange, MAX over ranks in place (RCCL all-reduce in production); NULL = 1 process */
    void (*allreduce_max)(void* user, double* vals, int count);
    void* allreduce_user;
    /* Action<string,bool[,]>: text + optional R x C highlight mask (NULL = none) */
    void (*text_cb)(void* user, const char* text, const uint8_t* highlight, int R, int C);
    void* text_user;
    int bnb_dive;          /* sharded searches: 0 = whole frontier per round (breadth first), 1 = only the deepest
                              `concurrent_nodes` nodes of the pool per round (depth-first-K: reaches incumbents early) */
} lpx_solve_opts;

typedef struct lpx_result {                        /* SimplexResult, Models/PrimalSimplex.cs:38-49 */
    int status;            /* LPX_OPTIMAL / LPX_UNBOUNDED / LPX_INFEASIBLE */
    int has_solution;      /* 0 == Solution/Tableau/Basis/VarNames are null in the reference (defect D2, revised) */
    double optimal_value;  /* OptimalValue */
    int n; double* x;      /* Solution [n] */
    int R, C; double* T;   /* Tableau [R*C] */
    int32_t* basis;        /* Basis [R-1] */
    int n_pivots; int32_t* trace;   /* (row, col) per pivot */
    char* report; char* summary;    /* Report, Summary */
    int64_t lp_solves, nodes;       /* branch and bound */
    int n_log; int32_t* node_log;   /* [3*n_log]: depth, outcome, branching variable */
    double* node_z;                 /* [n_log] */
    double aux[4];                  /* revised: {z_original, z_internal}; knapsack: {relaxations, popped, expanded, max_heap};
                                       sharded B&B: {levels, all-reduces, rebalancing rounds, node descriptors moved} */
    lpx_stats stats;
    int n_cuts; double* cuts;       /* cutting plane: [n_cuts*(nvars+1)] = (A[0..nvars), B) per cut, in the order added */
} lpx_result;

void lpx_default_solve_opts(lpx_solve_opts* o);
/* Returns 0 and fills *out, or the negative LPX_E_* code of the exception the reference would throw
 * (message via lpx_last_error). LPX_ITER_LIMIT (3) is returned for its iteration-limit exceptions. */
int  lpx_solve(const lpx_problem* p, const char* algorithm, const lpx_solve_opts* o, lpx_result* out);
void lpx_result_free(lpx_result* r);

typedef struct lpx_parsed { int sense, n, m; double* c; double* A; int32_t* rel; double* b; int ragged; } lpx_parsed;
/* LPParser.ParseFromText, Models/LPParser.cs:9-79 */
int  lpx_parse_text(const char* text, lpx_parsed* out);
void lpx_parsed_free(lpx_parsed* p);
/* ToString("0.###") as the reference renders tableau cells (Models/PrimalSimplex.cs:280) */
int  lpx_format_number(double v, char* buf, int len);

/* ---- consumers of SimplexResult.Tableau / Basis ------------------------------------
 * CuttingPlane / CuttingPlaneRevised (Models/CuttingPlane.cs:13-139, Models/CuttingPlaneRevised.cs:14-78) are
 * reached through lpx_solve with the menu names Form1.cs:249-261 uses: "Cutting Plane", "Revised Cutting Plane".
 *
 * SensitivityAnalysis (Models/SensitivityAnalysis.cs:11-297) over a problem and the final (T, basis) of a solve of
 * it; VarNames are the reference's x1..xn, c1..cm.  Every call repeats the constructor's checks (:24-43) and
 * returns the negative code with the reference's message in lpx_last_error.  Text is copied into buf (NUL
 * terminated, truncated to len); the return value is the full length.  The reference indexes the tableau as if
 * its objective row came first (:122,:237,:263,:279) -- kept. */
int lpx_sensitivity_range_report(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                 const char* target, char* buf, int len);                  /* GetRangeReport :47-76 */
int lpx_sensitivity_range(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                          const char* target, double* min, double* max);                   /* its numbers, :229-298 */
/* ApplyChange :78-107.  The model belongs to the caller: *field = 0 -> Constraints[*index].B = value,
 * 1 -> C[*index] = value is what the reference would have assigned. */
int lpx_sensitivity_apply_change(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                 const char* target, double value, int* field, int* index, char* buf, int len);
int lpx_sensitivity_shadow_prices(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                  char* buf, int len);                                     /* GetShadowPricesReport :109-128 */
/* SolveUsingDuality :130-219: builds the dual model and runs "Dual Simplex" on it (opts->dual_flags as lpx_solve). */
int lpx_sensitivity_solve_duality(const lpx_problem* p, const double* T, int R, int C, const int32_t* basis,
                                  const lpx_solve_opts* o, lpx_result* out);

/* ---- ranging of a solved tableau on the device (not in the reference; csrc/lpx_ranging.hip) -------
 * On the handle's current R x C window (m = R-1, objective row last, RHS column last), b_r = T[r,C-1], d_j = T[m,j],
 * b+ = (b > 0 ? b : 0.0), d+ likewise, N = columns j < C-1 not in basis[0..m):
 *   col_inc[j] = min over r < m with T[r,j] < -eps of b+_r / -T[r,j]   (j < C-1, basic columns included)
 *   col_dec[j] = min over r < m with T[r,j] >  eps of b+_r /  T[r,j]
 *   row_inc[r] = min over j in N with T[r,j] < -eps of d+_j / -T[r,j]  (r < m)
 *   row_dec[r] = min over j in N with T[r,j] >  eps of d+_j /  T[r,j]
 *   *min_rhs = min over r < m of b_r, *min_dj = min over j in N of d_j
 * Strict minimum, ties to the lowest index; an empty set gives +inf and index -1; *_at is the row (col_*) or column
 * (row_*) attaining it.  One read of the tableau; T, basis, snapshot, trace and captured graphs are left untouched.
 * Any output pointer may be NULL.  eps < 0: LPX_EINVAL; no device: LPX_EDEVICE (checked before the handle). */
int lpx_tableau_ranging(lpx_tableau* t, double eps,
                        double* col_inc, int32_t* col_inc_at, double* col_dec, int32_t* col_dec_at,  /* [C-1] or NULL */
                        double* row_inc, int32_t* row_inc_at, double* row_dec, int32_t* row_dec_at,  /* [R-1] or NULL */
                        double* min_rhs, double* min_dj);
/* The column ratio test along g_r = T[r,a[k]] - T[r,b[k]] (one IEEE subtraction) for K column pairs (equality rows). */
int lpx_tableau_ranging_pairs(lpx_tableau* t, double eps, int K, const int32_t* a, const int32_t* b,
                              double* inc, int32_t* inc_at, double* dec, int32_t* dec_at);   /* [K] or NULL */

/* Ranging report of a solved model in user terms.  *_at: tableau column (x1..xn = 0..n-1, then the slacks) or -1;
 * cost_*_at names the column that enters at that end, rhs_*_at the basic variable that leaves.  valid = 1 only when the
 * solve is OPTIMAL and min_rhs >= -1e-9 and min_dj >= -1e-9; otherwise every array holds NaN / -1. */
typedef struct lpx_ranging {
    int n, m, valid;
    double min_rhs, min_dj;                          /* of the final tableau (+inf when no tableau was ranged) */
    double* cost_lo; double* cost_hi; int32_t* cost_lo_at; int32_t* cost_hi_at;
    double* reduced_cost;                            /* [n] d(optimal objective) / d(lower bound of x_j) */
    double* rhs_lo; double* rhs_hi; int32_t* rhs_lo_at; int32_t* rhs_hi_at;
    double* dual;                                    /* [m] d(optimal objective) / d(b_i) */
} lpx_ranging;
/* lpx_solve plus the ranging report, computed on the solve's own device tableau before its handle is released.  `out` is
 * what lpx_solve returns for the same inputs.  Primal Simplex and Dual Simplex (and their aliases) only: any other
 * algorithm is LPX_EINVAL.  Free with lpx_ranging_free (and `out` with lpx_result_free). */
int  lpx_solve_ranging(const lpx_problem* p, const char* algorithm, const lpx_solve_opts* o, lpx_result* out, lpx_ranging* rg);
void lpx_ranging_free(lpx_ranging* rg);

/* ---- GMI cutting planes on the device (not in the reference; csrc/lpx_cuts.hip) ---------------
 * On the handle's live R x C window (m = R-1 rows, objective row last, RHS column last), b_r = T[r,C-1], basic columns from
 * the device basis.  Column j is integer iff j < min(n_mask, first_cut_col) and is_int[j] != 0; every other column (cut
 * slacks included) is continuous.  frac(v) = v - floor(v) (IEEE floor, one subtraction).
 *   Source rows: row r < m is a candidate when basis[r] is integer and f0 = frac(b_r) lies in [away, 1 - away].  Candidates
 *   are ranked by |f0 - 0.5| ascending, ties to the lower r; the first K whose cut passes the dynamism filter are taken,
 *   K = min(cuts_per_round, free capacity after purging) where free capacity = min(Rcap - (R - P), Ccap - (C - P)).
 *   Cut of row r (Gomory mixed-integer): sum over nonbasic j < C-1 of alpha_j x_j >= 1, alpha_j = 0 for basic j; a = T[r,j]:
 *     integer j:    f = frac(a); alpha = 0 if f <= coef_eps or f >= 1 - coef_eps, else f / f0 if f <= f0, else (1 - f) / (1 - f0)
 *     continuous j: alpha = 0 if |a| <= coef_eps, else a / f0 if a > 0, else -a / (1 - f0)
 *   Dynamism filter: reject when max alpha > max_dynamism * (min nonzero alpha); a row with no nonzero alpha passes (its
 *   cut 0 >= 1 proves the IP infeasible).
 *   Appended row: -alpha.x + s = -1 with s basic in it: entries (alpha_j == 0 ? +0.0 : -alpha_j), 1.0 in s's column, -1.0 in
 *   the RHS.  The objective row is unchanged and every new slack has d = 0: the tableau stays dual feasible.
 *   Purge (purge != 0, before appending): a cut is inactive when its slack column (a column in [first_cut_col, C-1)) is
 *   basic in a row r with b_r > purge_tol; that row and that column are deleted (the column is the unit vector e_r, so this
 *   is exact).  Remaining rows and columns keep their order; basis indices are renumbered.
 *   New shape: R' = R - P + K, C' = C - P + K; the cut rows go just above the objective row in selection order, their
 *   slacks just before the RHS column.
 * The basis is updated and the loop state reset (as lpx_tableau_build_child does); snapshot, trace and captured graphs are
 * left alone.  With K = P = 0 nothing is touched. */
typedef struct lpx_cut_opts {
    int    cuts_per_round;   /* K, default 8, 1..64 */
    int    max_rounds;       /* default 50 (the reference's cap, Models/CuttingPlane.cs:19) */
    int    max_active;       /* cut rows alive at once = capacity reserved by lpx_solve_cuts, default 64 */
    int    purge;            /* default 1 */
    double away, coef_eps, max_dynamism, purge_tol, int_tol;   /* 1e-3, 1e-9, 1e6, 1e-9, 1e-6 */
} lpx_cut_opts;
void lpx_default_cut_opts(lpx_cut_opts* o);
/* One round on a handle, which needs capacity for the result shape.  src_rows gets the K source rows in selection order
 * (row indices of the tableau before the round; K <= cuts_per_round), purged_cols the P purged columns ascending (column
 * indices before the round).  P can be as large as the number of cut columns before the round, C-1 - first_cut_col: it is
 * not bounded by max_active (that option only sizes lpx_solve_cuts' handle), so size purged_cols by that number.
 * Argument errors return LPX_EINVAL before any device check, with the tableau untouched: o outside its ranges
 * (cuts_per_round 1..64, max_rounds >= 0, max_active >= 1, 0 < away <= 0.5, 0 <= coef_eps < 0.5, max_dynamism >= 1,
 * purge_tol not NaN, int_tol >= 0), n_mask < 0, is_int NULL with n_mask > 0, a NULL handle, first_cut_col outside [1, C-1], more than
 * 2048 cut columns, a handle wider than 131072 columns, R < 2.  No device: LPX_EDEVICE. */
int  lpx_tableau_gmi_round(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col,
                           const lpx_cut_opts* o, int* n_added, int32_t* src_rows /* [K] or NULL */,
                           int* n_purged, int32_t* purged_cols /* [C-1 - first_cut_col] or NULL */);
/* The whole solver with explicit options; lpx_solve(p, "GMI Cutting Plane" or "gmi", ...) is this with defaults.  Every
 * structural variable is integer; the model is prepared as Dual Simplex prepares it with defect D1 fixed (Min/Max, <=, >=,
 * =); the slack of a prepared row is integer iff its coefficients and RHS are integral.  Root LP: lpx_primal_run when every
 * prepared RHS is >= 0, else the repaired dual (fdf_guard = max_iter, cleanup = 1).  Each round: integer basics within
 * int_tol of integral -> LPX_CUT_INTEGER; else lpx_tableau_gmi_round; 0 cuts added -> LPX_CUT_INCOMPLETE (stalled); else
 * lpx_dual_run (fdf_guard = 0, cleanup = 1), LPX_INFEASIBLE there -> the IP is infeasible (LPX_INFEASIBLE); max_rounds
 * used up -> LPX_CUT_INCOMPLETE.  The root LP's own LPX_UNBOUNDED / LPX_INFEASIBLE are returned as such.
 * out: optimal_value = final LP bound in the user's sense; x, T, basis of the final tableau; trace = the pivots of the root
 * LP and of every round, in order; lp_solves = 1 + rounds; aux = {rounds, cuts added, cuts purged, root LP bound};
 * node_log = (round, source row, slack column) per added cut with node_z = the LP bound after that round; cuts = every cut
 * ever added, in x-space as LE rows (A[0..n), B).  Argument errors as lpx_tableau_gmi_round (co NULL = defaults). */
int  lpx_solve_cuts(const lpx_problem* p, const lpx_solve_opts* o, const lpx_cut_opts* co, lpx_result* out);

/* ---- post-optimal edits on the device (not in the reference; csrc/lpx_postopt.hip) ------------
 * On the handle's live R x C window (m = R-1, objective row last, RHS column last, Cm = C-1), basic columns from the device
 * basis.  Every edit is one of two combinations, each with a fixed summation order:
 *   column combination  out[i] = base[i] (+) sum_k v[k] * T[i, cols[k]]      for i in [0, R)
 *   row combination     out[j] = base[j] (+) sum_k w[k] * T[rows[k], j]      for the columns j of the output
 * where "(+) sum" means: the K terms are cut into segments of LPX_POSTOPT_SEG consecutive terms (k = 0 .. SEG-1, SEG ..
 * 2 SEG-1, ...); each term is one IEEE multiply; each segment is summed sequentially in term order starting from +0.0;
 * out = base, then out = out + (segment sum) for the segments in ascending order.  No FMA.  K = 0 gives out = base.  The
 * bits do not depend on the launch geometry or on the handle's capacity.
 *
 * lpx_tableau_rhs_update:  column combination with base = T[:, Cm], written back into T[:, Cm] (row m included: z moves by
 *   y.delta).  cols[k] in [0, Cm).
 * lpx_tableau_add_column:  column combination with base[i] = +0.0 for i < m and base[m] = obj (= -c' for a new column of cost
 *   c'); the RHS column moves to index C and the result becomes column Cm; the new shape is R x (C+1).  Needs Ccap > C.
 * lpx_tableau_objective_update:  base[j] = T[m, j], then base[dcols[k]] = base[dcols[k]] - dd[k] (one IEEE subtraction per
 *   touched column; dcols distinct, in [0, Cm)); row combination over j in [0, C) with rows[k] in [0, m); every basic column
 *   of the output is written as +0.0; the result replaces row m.
 * lpx_tableau_add_row:  base holds C+1 entries in the NEW shape: [0, Cm) the prepared row's old columns, Cm its own slack
 *   (1.0 for a fresh slack), C its RHS.  Row combination with rows[k] in [0, m): output column j < Cm reads column j, output
 *   column Cm (the new slack) is base[Cm] unchanged, output column C reads the old RHS column Cm; every basic column is +0.0.
 *   The result goes in as row m, the objective row moves to m+1, every old row gets +0.0 in the new slack column Cm and its
 *   RHS moved to column C; basis[m] = Cm.  The new shape is (R+1) x (C+1).  Needs Rcap > R and Ccap > C.
 * After each edit the live shape is (re)set and the loop state reset as lpx_tableau_build_child does; the basis is unchanged
 * but for the appended row's slack.  Snapshot, trace buffer and captured graphs are left alone: a later lpx_tableau_restore
 * brings back the tableau as it was snapshotted, with its own shape's contents, and does not undo or redo the edit.
 * Argument errors return LPX_EINVAL before any device check, with the tableau untouched: a NULL handle, R < 2, K < 0 or
 * Kd < 0, NULL term arrays with K > 0, an index outside its range, repeated dcols, a NULL base, no spare capacity.  No
 * device: LPX_EDEVICE. */
#define LPX_POSTOPT_SEG 64
int lpx_tableau_rhs_update(lpx_tableau* t, int K, const int32_t* cols, const double* v);
int lpx_tableau_objective_update(lpx_tableau* t, int K, const int32_t* rows, const double* w, int Kd, const int32_t* dcols,
                                 const double* dd);
int lpx_tableau_add_column(lpx_tableau* t, int K, const int32_t* cols, const double* v, double obj);
int lpx_tableau_add_row(lpx_tableau* t, int K, const int32_t* rows, const double* w, const double* base /* [C+1] */);

/* A model-level warm session: one handle holds the solved model and takes edits, each re-optimised on the device from the
 * current basis.  The model is prepared as lpx_solve_cuts prepares its root (Dual Simplex preparation with defect D1 fixed:
 * Min -> Max with c negated, >= rows negated, = rows as the pair (a, b), (-a, -b)); prepared row k comes from constraint
 * row_of[k] with sign[k] = +-1 and owns slack column `slack_col[k]`.  lpx_session_open: lpx_primal_run when every prepared
 * b >= 0, else the repaired dual (fdf_guard = max_iter, cleanup = 1); for an all-<= model with b >= 0 this is the trace, basis
 * and objective of lpx_solve(p, "Primal Simplex").  The first dual run of a handle pays a one-time setup: when the open
 * solve ended OPTIMAL, open pays it with one dual run (fdf_guard = 0, cleanup = 1) on the solved tableau, which is primal and
 * dual feasible and takes no pivot, after res has been filled, and reports its host wall in res->aux[1] (milliseconds).
 * Edits (each fills `res` for the edited model; res->trace / res->stats cover this edit's pivots only; res->aux[0] = 1 for a
 * warm edit, 0 when the session was not optimal and the edited model was rebuilt and solved cold on the same handle):
 *   set_rhs(K, cons, b):  delta_k = sign_k * (b_new - b_old) on every prepared row k of each constraint, through
 *                         lpx_tableau_rhs_update over the slack columns; then lpx_dual_run (fdf_guard = 0, cleanup = 1) when
 *                         min_i b_i < -1e-9, else no pivot.
 *   set_cost(K, vars, c): delta' = sigma * (c_new - c_old) (sigma = -1 for Min); basic variables become row weights, nonbasic
 *                         ones sparse deltas of lpx_tableau_objective_update; then lpx_primal_run.
 *   add_variable(c, a):   a'_k = sign_k * a[row_of[k]] over the slack columns (lpx_tableau_add_column, obj = -sigma c); the
 *                         new column goes just before the RHS; then lpx_primal_run.
 *   add_constraint(a, rel, b): 1 prepared row for <= / >=, 2 for = (lpx_tableau_add_row each; weights -a' of the basic
 *                         structural variables); then lpx_dual_run as set_rhs.
 * res->x covers the original variables, then the added ones in order; res->T is filled only with opts.want_tableau.
 * Running out of capacity returns LPX_EINVAL with the session unchanged.  lpx_session_ranging ranges the current basis as
 * lpx_solve_ranging does (columns in *_at are the session tableau's). */
typedef struct lpx_session lpx_session;
typedef struct lpx_session_opts {
    int extra_rows;        /* spare prepared rows for added constraints, default 16 */
    int extra_cols;        /* spare columns for added variables and constraint slacks, default 16 */
    int max_iter;          /* 0 = 10000 */
    int batch;             /* 0 = default */
    int want_tableau;      /* 1 = download the tableau into res->T after every call (R x C of the live window) */
} lpx_session_opts;
void lpx_default_session_opts(lpx_session_opts* o);
int  lpx_session_open(const lpx_problem* p, const lpx_session_opts* o, lpx_session** s, lpx_result* res);
int  lpx_session_set_rhs(lpx_session* s, int K, const int32_t* cons, const double* b, lpx_result* res);
int  lpx_session_set_cost(lpx_session* s, int K, const int32_t* vars, const double* c, lpx_result* res);
int  lpx_session_add_variable(lpx_session* s, double c, const double* a /* [m_user] */, lpx_result* res);
int  lpx_session_add_constraint(lpx_session* s, const double* a /* [n_cur] */, int rel, double b, lpx_result* res);
int  lpx_session_ranging(lpx_session* s, lpx_ranging* rg);
/* current user-level shape: variables (original + added) and constraints (original + added); any pointer may be NULL */
int  lpx_session_shape(const lpx_session* s, int* n_vars, int* n_cons);
void lpx_session_close(lpx_session* s);

/* ---- bounded-variable primal simplex on the device (not in the reference; csrc/lpx_bounded.hip) --
 * A primal simplex loop on the handle's live R x C window (m = R-1 rows, objective row last, RHS column last, Cm = C-1) in
 * which every column j < Cm has an upper bound ub[j] in [0, +inf] kept BESIDE the tableau, with a one-byte state flip[j]:
 * flip[j] = 1 means that column j currently stands for u_j - x_j.  Invariant: every nonbasic column is at 0 in its current
 * representation; a basic value lies in [0, ub[basis[i]]].  A 0/1 variable costs no row and no slack column.
 * All arithmetic is IEEE double, no FMA, true division.  One EVENT per iteration:
 *   1. Entering column q: ChooseEntering exactly as lpx_primal_run (first index of the strict minimum of T[m, 0..Cm) below
 *      -eps).  None: LPX_OPTIMAL.
 *   2. Ratio scan, rows i = 0..m-1 in ascending order, a = T[i,q], b_i = T[i,Cm], p = basis[i]:
 *        a >  eps:                     rho = b_i / a,                kind 0 (the basic variable goes to zero)
 *        a < -eps and ub[p] < +inf:    rho = (ub[p] - b_i) / (-a),   kind 1 (the basic variable goes to its upper bound;
 *                                      one subtraction, one negation, one division)
 *        otherwise the row does not take part.
 *      A row is accepted iff rho < best - ratio_tol (the sequential hysteresis of ChooseLeaving; best starts at +inf); the
 *      last accepted row is r, with its kind.
 *   3. Decision:
 *        ub[q] < +inf and ub[q] <= best: BOUND FLIP (ties go to the flip; it moves no other column).  For every row i in
 *          [0, R), the objective row included: T[i,Cm] = T[i,Cm] - ub[q] * T[i,q] (one multiply, one subtract), then
 *          T[i,q] = -T[i,q]; flip[q] ^= 1.  Basis unchanged.  Trace entry (-1, q).
 *        else no accepted row: LPX_UNBOUNDED.
 *        else kind 1: ROW COMPLEMENT of row r first, p = basis[r]: T[r,j] = -T[r,j] for every j < Cm, j != p (T[r,p] stays,
 *          it is the 1.0 of a basic column); T[r,Cm] = ub[p] - T[r,Cm]; flip[p] ^= 1.  Then the ordinary pivot on (r, q).
 *          Trace entry (-2 - r, q).
 *        else kind 0: the ordinary pivot on (r, q).  Trace entry (r, q).
 *      The ordinary pivot is Pivot (Models/PrimalSimplex.cs:245-257): row r divided by the pivot, every other row
 *      T[i,:] -= T[i,q] * T[r,:] with separate multiply and subtract, basis[r] = q.
 *   4. Before step 1, events done >= max_iter (flips and pivots alike) is LPX_ITER_LIMIT, tested where lpx_primal_run tests
 *      its pivot count.  The per-pivot callback receives (iter, row, col) with the trace's encoding.
 * With every ub = +inf the loop is lpx_primal_run bit for bit (same trace, same tableau).  The result depends on nothing but
 * the tableau, basis, ub and the options: not on the batch length, on graph replay, or on how many flips share a launch.
 * Tableaux of any m are accepted: the ratios of a tableau with more than 4096 rows go through global scratch instead of LDS.
 *
 * lpx_tableau_set_bounds: ncols must be the live C-1; every ub[j] in [0, +inf]; clears every flip.  ub == NULL with
 *   ncols == 0 removes the bounds.  Bounds belong to the live shape they were set for.
 *   lpx_tableau_upload leaves ub and flip as they are (a host may download a tableau with its flags and bring it back): set the
 *   bounds again after uploading another model.
 * lpx_tableau_bound_flags: flip[C-1] (all zero for a handle without bounds).
 * lpx_bounded_run: options eps, ratio_tol, max_iter, batch, use_graph, profile as lpx_primal_run reads them (profile runs
 *   eager launches; update_ms_sum is not collected, a launch here does not map to one update); resident = 1 is LPX_EINVAL (there
 *   is no resident form).  A handle without bounds runs with every ub = +inf.  If the live C has changed since
 *   lpx_tableau_set_bounds the run is LPX_EINVAL.  lpx_stats.pivots counts kind-0 and kind-1 pivots; lpx_tableau_trace
 *   returns the events.  lpx_bounded_counts: events of the last run: kind 0, kind 1, flips.
 * lpx_tableau_snapshot / lpx_tableau_restore carry ub and flip with the tableau; restoring a snapshot taken before the handle
 *   had bounds clears every flip.  lpx_tableau_ranging, lpx_tableau_gmi_round and the post-optimal edits on a handle with
 *   flips set see the internal representation (flipped columns stand for u_j - x_j); they are not bound-aware
 *   (lpx_tableau_gmi_round_bounded is the round that is, and it carries the bounds across its reshape).
 * lpx_tableau_bounded_solution: v_j = RHS of the row where j is basic, else +0.0; x[j] = flip[j] ? ub[j] - v_j : v_j (one
 *   subtraction); *z = T[m,Cm]; at_upper[j] = 1 iff j is nonbasic and flipped.  nvars <= C-1.
 * Argument errors return LPX_EINVAL before any device check, with the handle untouched: a NULL handle, ncols not the live
 * C-1, a negative or NaN bound, R < 2, resident = 1.  No device: LPX_EDEVICE. */
int lpx_tableau_set_bounds(lpx_tableau* t, int ncols, const double* ub);
int lpx_tableau_bound_flags(lpx_tableau* t, uint8_t* flip /* [C-1] */);
int lpx_bounded_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st);
int lpx_bounded_counts(lpx_tableau* t, int64_t counts[3]);
int lpx_tableau_bounded_solution(lpx_tableau* t, int nvars, double* x, double* z, uint8_t* at_upper /* [nvars] or NULL */);

/* The model level: lower[j] <= x_j <= upper[j] without a row per bound.  Preparation as PrimalSimplex.Solve prepares (Min
 * negates c; a >= row is LPX_E_GE_PRESENT; = rows become the <= pair), then the shift x = l + x': b'_i = b_i - sum_j A_ij l_j
 * with j ascending, one multiply and one subtract per nonzero l_j; u'_j = u_j - l_j; any b'_i < -1e-9 is LPX_E_NEG_RHS with
 * the reference's message.  lower[j] must be finite and upper[j] must be +inf or >= lower[j]: a NaN, an infinite lower bound
 * or upper[j] < lower[j] is LPX_EINVAL (checked first, before any device check).  Slack columns get +inf.
 * out: x in the user's variables (l_j added back), optimal_value in the user's sense including the constant c.l, T / basis
 * the final internal tableau, trace the events, stats, aux = {kind-0 pivots, kind-1 pivots, flips, constant c.l}, report and
 * summary in the Primal Simplex layout with one added line naming the variables at their upper bound.  info (or NULL):
 * ncols = C-1, flip[ncols], ub[ncols] (shifted), n, lower[n]; free with lpx_bounded_info_free.  With lower == upper == NULL
 * the result equals lpx_solve(p, "Primal Simplex") in trace, basis, tableau bits, x and, for Max models, optimal_value.
 * lpx_solve(p, "Bounded Primal Simplex", ...) is this call without bounds. */
typedef struct lpx_bounded_info {
    int ncols, n;
    uint8_t* flip;         /* [ncols] */
    double* ub;            /* [ncols] shifted upper bounds, +inf for slacks */
    double* lower;         /* [n] */
} lpx_bounded_info;
int  lpx_solve_bounded(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] or NULL = +inf */,
                       const lpx_solve_opts* o, lpx_result* out, lpx_bounded_info* info /* or NULL */);
void lpx_bounded_info_free(lpx_bounded_info* info);

/* ---- bounded dual simplex and bound changes on a solved tableau (not in the reference; csrc/lpx_bounded_dual.hip, DESIGN.md
 * section 4.14) --
 * The representation of the bounded primal loop above, plus a LOWER SHIFT lo[j] (double) for every column j < Cm: internal
 * column j stands for x_j - lo[j] when flip[j] = 0 and for ub[j] - (x_j - lo[j]) when flip[j] = 1.  lpx_tableau_set_bounds sets
 * every lo[j] to +0.0; lpx_tableau_snapshot / _restore carry lo with ub and flip; lpx_tableau_upload leaves it alone.
 * lpx_tableau_bounded_solution adds lo[j] to x[j] (one addition, after the subtraction of a flipped column), but only on a
 * handle where a change has stored a non-zero lo since the last lpx_tableau_set_bounds; on every other handle its output is
 * what it was without this section.  lpx_tableau_bound_state: lo, ub, flip of the live C-1 columns, each array [C-1] or NULL;
 * a handle without bounds reports lo = 0, ub = +inf, flip = 0.
 *
 * lpx_tableau_change_bounds(t, K, cols, lower, upper): new ABSOLUTE bounds lower[k] <= x_cols[k] <= upper[k] on a handle that
 * has bounds, in place on the live window (R rows, the objective row included, Cm = C-1).  IEEE double, no FMA; the bits do not
 * depend on launch geometry or capacity.  For k = 0..K-1 in order, j = cols[k]:
 *   1. l' = lower[k] - lo[j], u' = upper[k] - lo[j] (one subtraction each; +inf stays +inf).
 *   2. s = flip[j] ? ub[j] - u' : l'.
 *   3. For every row i in [0, R): T[i,Cm] = T[i,Cm] - s * T[i,j] (one multiply, one subtract) -- for a basic column too, where
 *      only its own row really moves.  The whole pass is skipped when s == 0.0.
 *   4. ub[j] = upper[k] - lower[k]; lo[j] = lower[k].
 * Flips, basis and every column other than the RHS stay as they were, and so does the objective row apart from its RHS: a
 * dual-feasible tableau stays dual feasible (a basic value may now lie below 0 or above its bound: lpx_bounded_dual_run
 * repairs that).  The loop state is reset as lpx_tableau_build_child resets it.
 * LPX_EINVAL before any device check, nothing touched: a NULL handle, K < 0, NULL arrays with K > 0, a column outside
 * [0, Cm), a repeated column, a NaN bound, an infinite lower, upper < lower, a handle without bounds or whose live C changed
 * since lpx_tableau_set_bounds.  upper = +inf on a column whose flip is set is LPX_EINVAL too (after the device check, the flip
 * lives on the device; the handle is untouched): unflipping is not part of this edit.  No device: LPX_EDEVICE.
 *
 * lpx_bounded_dual_run: a dual simplex on this representation.  Precondition, not checked: every nonbasic column has
 * T[m,j] >= -eps.  One EVENT per iteration; IEEE double, no FMA, true division:
 *   1. Events done >= max_iter: LPX_ITER_LIMIT (tested where lpx_bounded_run tests its limit, before anything else).
 *   2. Leaving row, rows i = 0..m-1 in ascending order, b = T[i,Cm], p = basis[i]:
 *        b < -eps:                 w_i = b,           kind 0 (the basic variable is below zero)
 *        else ub[p] < +inf:        w_i = ub[p] - b,   kind 1 (one subtraction; negative when the variable is above its bound)
 *        otherwise the row does not take part.
 *      r = first index of the strict minimum of w below -eps (the `v < mostNeg` scan of lpx_dual_run, mostNeg starting at
 *      -eps).  No such row: LPX_OPTIMAL.
 *   3. Kind 1: the ROW COMPLEMENT of row r as defined above for the primal loop, p = basis[r]: T[r,j] = -T[r,j] for every
 *      j < Cm, j != p; T[r,Cm] = ub[p] - T[r,Cm]; flip[p] ^= 1.  The row's RHS is now below -eps.
 *   4. Entering column, columns j = 0..Cm-1 in ascending order, a = T[r,j] (after the complement): a column takes part iff
 *      a < -eps, ratio = T[m,j] / (-a), accepted iff ratio < best - ratio_tol (best starts at +inf); the last accepted column
 *      is q -- the entering rule of lpx_dual_run.  No column: LPX_INFEASIBLE; a complement applied in step 3 stays applied (the
 *      tableau is still a valid representation), no event is recorded.
 *   5. The ordinary pivot on (r, q), basis[r] = q.  Trace entry (r, q) for kind 0, (-2 - r, q) for kind 1; the per-pivot
 *      callback receives the same encoding.
 * Options eps, ratio_tol, max_iter, batch, use_graph, profile as lpx_bounded_run reads them; fdf_guard and cleanup are not read;
 * resident = 1 is LPX_EINVAL.  o == NULL: lpx_default_opts(o, 1), the dual loop's defaults.  lpx_stats.pivots = events;
 * lpx_bounded_counts returns {kind 0, kind 1, 0}.  A handle without bounds runs with every ub = +inf and is then
 * lpx_dual_run(fdf_guard = 0, cleanup = 0) bit for bit.  The result depends on nothing but the tableau, basis, ub, flip and the
 * options: not on the batch length, on graph replay or on the callback.  Any m and Cm: w and the ratios are held on chip up to
 * 4096 entries each and go through global scratch beyond that. */
int lpx_tableau_bound_state(lpx_tableau* t, double* lo /* [C-1] or NULL */, double* ub /* [C-1] or NULL */, uint8_t* flip /* [C-1] or NULL */);
int lpx_tableau_change_bounds(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper);
int lpx_bounded_dual_run(lpx_tableau* t, const lpx_run_opts* o, lpx_pivot_cb cb, void* user, lpx_stats* st);

/* The model level: a bounded session.  lpx_bounded_open is lpx_solve_bounded that keeps its handle: same validation, same
 * messages, res equal to lpx_solve_bounded's for the same inputs.  lpx_bounded_set_bounds takes the user's ABSOLUTE bounds
 * lower[k] <= x_vars[k] <= upper[k] of original variables (0-based), applies them with lpx_tableau_change_bounds and
 * re-optimises with lpx_bounded_dual_run from the tableau as it stands.  res: x in the user's variables, optimal_value in the
 * user's sense with the constant of open included, T / basis the internal tableau, trace / stats of this edit only,
 * aux = {kind-0 events, kind-1 events, 1, constant}, status LPX_OPTIMAL or LPX_INFEASIBLE (x and optimal_value then describe
 * the tableau as it stands); LPX_ITER_LIMIT is the return value, as elsewhere.  A session left INFEASIBLE stays usable:
 * loosening the bounds continues from the tableau as it stands.  A session whose open solve was not LPX_OPTIMAL returns
 * LPX_EINVAL with a message.  Validation (before any device check): a NULL session or res, K < 0, NULL arrays with K > 0, a
 * variable outside [0, n), a repeated variable, a lower bound that is not finite, an upper bound below its lower bound or NaN
 * -- the last two with lpx_solve_bounded's messages.  upper = +inf on a variable whose column is flipped is LPX_EINVAL, as in
 * lpx_tableau_change_bounds. */
typedef struct lpx_bounded_session lpx_bounded_session;
int  lpx_bounded_open(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] or NULL = +inf */,
                      const lpx_solve_opts* o, lpx_bounded_session** session, lpx_result* res);
int  lpx_bounded_set_bounds(lpx_bounded_session* s, int K, const int32_t* vars, const double* lower, const double* upper,
                            lpx_result* res);
void lpx_bounded_close(lpx_bounded_session* s);

/* ---- branch and bound by bound changes on one device tableau (not in the reference; csrc/lpx_bnb_bounded.hip,
 * csrc/host/bnb_bounded.cpp) --
 * A node of the search is a list of (column, lower, upper) triples applied to ONE handle whose shape never changes: the bound
 * change of the section above, a repair of dual feasibility by bound flips, a dual loop in which fixed columns do not enter,
 * and the pick of the branching variable.  No tableau is copied, parked or reshaped.  All arithmetic is IEEE double, no FMA,
 * true division; no result depends on launch geometry, capacity, batch length or graph replay.
 *
 * lpx_tableau_dualize(t, eps, counts): dual-feasibility flips on the live window (R rows, Cm = C-1).  J is the ascending list of
 * the columns j < Cm with T[m,j] < -eps and 0 < ub[j] < +inf.  For j in J in that order and every row i in [0, R), the
 * objective row included:
 *   1. T[i,Cm] = T[i,Cm] - ub[j] * T[i,j] (one multiply, one subtract),
 *   2. T[i,j] = -T[i,j],
 * and flip[j] ^= 1 -- the arithmetic of the BOUND FLIP of lpx_bounded_run.  The contiguous RHS copy the loops read is kept
 * current.  A column with T[m,j] < -eps and ub[j] = +inf cannot be repaired: it is left alone and counted.  A column with
 * ub[j] == 0 is left alone and not counted (its reduced cost may stay negative: it does not enter the flagged loop below).
 * Basic columns have reduced cost exactly 0 after a pivot, so the test needs no basis lookup.  counts = {flips, unrepairable}.
 * Why it is needed: a fixed column that stayed out of the flagged loop may carry a negative reduced cost; when a later node
 * relaxes its bound, the flip puts the column at its other bound, where its reduced cost is the negation.
 * LPX_EINVAL before any device check: a NULL handle or counts, eps negative or NaN, a handle without bounds or whose live C
 * changed since lpx_tableau_set_bounds.
 *
 * lpx_bounded_dual_run2(t, o, flags, cb, user, st): lpx_bounded_dual_run with flags.  flags = 0 is lpx_bounded_dual_run bit for
 * bit.  LPX_BDUAL_SKIP_FIXED: in step 4 of the dual contract a column takes part iff a < -eps AND ub[j] > 0.0; everything else
 * is lpx_bounded_dual_run.  Precondition of the flagged form, not checked: every nonbasic column with ub[j] > 0 has
 * T[m,j] >= -eps (lpx_tableau_dualize establishes it).  Why: on branch-and-bound nodes the unflagged rule cycles through
 * degenerate pivots on fixed columns (ub = 0), which can never change the point; kept out, they cost nothing.  Any other flag
 * bit is LPX_EINVAL.  The cached graphs of the two forms on one handle are kept apart.
 *
 * lpx_tableau_branch_pick(t, nint, is_int, tol, out): for j < nint, x_j is exactly the value lpx_tableau_bounded_solution
 * returns (v_j = RHS of the row where j is basic, else +0.0; x_j = flip[j] ? ub[j] - v_j : v_j; + lo[j] on a handle that has
 * stored a non-zero lower shift).  f = x_j - floor(x_j).  j is a candidate iff is_int[j] != 0 (is_int == NULL: every j) and
 * f > tol and (1 - f) > tol (one subtraction).  dist = |f - 0.5|.  The pick is the candidate of least dist, ties to the lowest
 * index: the rule of Models/Branch&Bound.cs:197-213.  out = {var or -1, candidates, x_var (0.0 without a pick), z = T[m,Cm]}.
 * LPX_EINVAL before any device check: a NULL handle or out, nint outside [0, Cm], tol not in [0, 0.5), a handle whose live C
 * changed since lpx_tableau_set_bounds.  A handle without bounds is read with ub = +inf, flip = 0, lo = 0.
 *
 * lpx_bounded_node(t, K, cols, lower, upper, o, nint, is_int, tol, out): one node in one call --
 * lpx_tableau_change_bounds(t, K, cols, lower, upper), lpx_tableau_dualize(t, o->eps), lpx_bounded_dual_run2(t, o,
 * LPX_BDUAL_SKIP_FIXED), and on LPX_OPTIMAL lpx_tableau_branch_pick(t, nint, is_int, tol); the bits are those of the four calls
 * in a row.  o == NULL: lpx_default_opts(o, 1).  The return value is the loop's status (or an error);
 * out = {status, events, kind-0 events, kind-1 events, dual-feasibility flips, unrepairable, pick}; without LPX_OPTIMAL the
 * pick is {-1, 0, 0.0, T[m,Cm] as it stands}.  K = 0 is allowed.  A column that would be unrepairable after the change is
 * LPX_EINVAL with a message, found before the tableau is touched: ub and lo are put back and the handle is as it was.
 * Argument errors are those of lpx_tableau_change_bounds, plus nint outside [0, Cm], tol not in [0, 0.5), a NULL out and
 * resident = 1; they are checked before any device check and leave the handle untouched.  No device: LPX_EDEVICE. */
#define LPX_BDUAL_SKIP_FIXED 1
typedef struct lpx_branch_pick {
    int32_t var;           /* branching column, -1 = none (every integer column is integral within tol) */
    int32_t candidates;    /* fractional integer columns */
    double x_var;          /* value of the pick */
    double z;              /* T[m,Cm] */
} lpx_branch_pick;
typedef struct lpx_node_record {
    int32_t status;        /* LPX_OPTIMAL / LPX_INFEASIBLE / LPX_ITER_LIMIT */
    int32_t events;        /* events of the dual loop */
    int64_t kind0, kind1;  /* ... per kind */
    int64_t flips;         /* dual-feasibility flips */
    int64_t unrepairable;
    lpx_branch_pick pick;
} lpx_node_record;
int lpx_tableau_dualize(lpx_tableau* t, double eps, int64_t counts[2]);
int lpx_bounded_dual_run2(lpx_tableau* t, const lpx_run_opts* o, int flags, lpx_pivot_cb cb, void* user, lpx_stats* st);
int lpx_tableau_branch_pick(lpx_tableau* t, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol, lpx_branch_pick* out);
int lpx_bounded_node(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                     int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol, lpx_node_record* out);

/* The model level: max / min c.x, A x <= b, lower <= x <= upper, x_j integer where is_int[j] != 0 (NULL: every variable).
 * Validation and preparation are those of lpx_solve_bounded (same messages, same lower shift); additionally every integer
 * variable needs finite, integral lower and upper bounds, else LPX_EINVAL with a message naming the variable -- which is why
 * a column never has to be unflipped to +inf.  The handle's columns stand for x' = x - lower; the search works on x'.
 *   Root: lpx_bounded_run.  UNBOUNDED is reported as that.  Then a depth-first stack on the root's handle; node 0 is the root
 *   itself (K = 0).  A node is its path of (var, lower', upper') overrides of the root bounds.
 *   Entering a node: the node's bounds are compared with the bounds now on the device and ONE lpx_bounded_node call carries the
 *   differing columns in ascending column order (the order is part of the contract: the RHS bits depend on it); o->max_iter is
 *   the event limit of a node, tol = 1e-6 and nint = n.
 *   INFEASIBLE: pruned.  z <= best + 1e-6 (EPS, Models/Branch&Bound.cs:182; z = T[m,Cm], best starts at -inf): pruned by bound.
 *   pick.var < 0: a new incumbent, best = z; x' is read once with lpx_tableau_bounded_solution and its integer entries are
 *   rounded as BestSolution is (:192, Math.Round: half to even).  Otherwise the children are [ceil(x'_var), U'] and
 *   [L', floor(x'_var)] on var; the ceil child is explored first (:253-257).
 * The reference's IsFeasible re-check of an incumbent is not mirrored: the dual loop ends primal feasible by construction.
 * A node that reaches max_iter ends the solve with return value LPX_ITER_LIMIT and a message naming the node; there is no
 * fallback.  Reaching max_nodes (0 = none) returns LPX_ITER_LIMIT too.  In both cases out holds the incumbent so far.
 * out: status LPX_OPTIMAL or LPX_INFEASIBLE (no incumbent) or the root's LPX_UNBOUNDED; x in the user's variables (lower
 * added back); optimal_value in the user's sense (-z for Min) plus the constant c.lower, as lpx_solve_bounded; nodes;
 * lp_solves = nodes + 1; aux = {nodes, dual events, dual-feasibility flips, incumbents found}; T / basis and stats are the root
 * solve's (the internal tableau after lpx_bounded_run), the trace is empty; the summary ends with a line of the counters.
 * info (or NULL): counters {pruned by bound, pruned infeasible, largest K, constant} and one log record per node in the order
 * visited; free with lpx_bnb_bounded_info_free. */
typedef struct lpx_bnb_node_log {
    int32_t depth, K, status, events, flips, var;     /* var: branching variable, -1 = none */
    double z;                                         /* T[m,Cm] after the node's loop */
} lpx_bnb_node_log;
typedef struct lpx_bnb_bounded_info {
    int64_t nodes, events, flips, incumbents, pruned_bound, pruned_infeasible, max_K;
    double constant;
    int64_t n_log;
    lpx_bnb_node_log* log;   /* [n_log] */
} lpx_bnb_bounded_info;
int  lpx_solve_bnb_bounded(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                           const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                           lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */);
void lpx_bnb_bounded_info_free(lpx_bnb_bounded_info* info);

/* ---- long-step ratio test, objective cutoff and dual start (not in the reference; csrc/lpx_bounded_long.hip,
 * csrc/host/bounded.cpp, csrc/host/bnb_bounded.cpp) --
 * lpx_bounded_dual_run3(t, o, flags, cutoff, cb, user, st): lpx_bounded_dual_run2 with two more flags.  flags with neither
 * LPX_BDUAL_LONG_STEP nor LPX_BDUAL_CUTOFF is lpx_bounded_dual_run2(flags) bit for bit (same kernels, same cached graphs).  All
 * arithmetic is IEEE double, no FMA, true division.  The steps are those of lpx_bounded_dual_run, with these changes:
 *   1b. (LPX_BDUAL_CUTOFF only) After the iteration-limit test of step 1 and before the leaving row: T[m,Cm] <= cutoff is
 *       LPX_CUTOFF.  Nothing is touched and no event is recorded.  In the dual loop T[m,Cm] only falls, so LPX_OPTIMAL implies
 *       T[m,Cm] > cutoff.  cutoff = -inf never fires; NaN is LPX_EINVAL.  Without the flag the value is not read.
 *   3.  The complement of a kind-1 row is applied before step 4, as in lpx_bounded_dual_run; every pass below works on the
 *       complemented row (this decides the bits of T[r,Cm]).
 *   4.  (LPX_BDUAL_LONG_STEP only) The ratios rho[j] are formed ONCE, exactly as in step 4 of lpx_bounded_dual_run (+inf = the
 *       column does not take part; with LPX_BDUAL_SKIP_FIXED a column takes part iff a < -eps and ub[j] > 0).  Then repeat:
 *         4.1 q = the last column accepted by the sequential scan rho[j] < best - ratio_tol, j ascending, best from +inf.
 *         4.2 No q: LPX_INFEASIBLE.  Passes already made stay applied and stay in the trace (the tableau is still a valid
 *             representation, with row r below zero and no column left that can raise it).
 *         4.3 If ub[q] < +inf: nb = T[r,Cm] - ub[q] * T[r,q] (one multiply, one subtract).
 *         4.4 If ub[q] < +inf and nb < -eps, column q PASSES -- the BOUND FLIP of lpx_bounded_run on column q: for every row i
 *             in [0, R), the objective row included, T[i,Cm] = T[i,Cm] - ub[q] * T[i,q] (one multiply, one subtract), then
 *             T[i,q] = -T[i,q]; flip[q] ^= 1; the contiguous RHS copy is kept current.  Trace entry (-1, q); the pass counts as
 *             an event.  rho[q] = +inf, back to 4.1.
 *         4.5 Otherwise q enters: step 5 as in lpx_bounded_dual_run.
 *       A column passes at most once per pivot (at most Cm passes per launch).  The iteration limit is tested in step 1 only, so
 *       a run ends with at most max_iter + Cm events.  Trace entries beyond the trace capacity are dropped, as elsewhere.
 * lpx_bounded_counts returns {kind 0, kind 1, passes}; lpx_stats.pivots = kind 0 + kind 1; the per-pivot callback sees the
 * passes with the trace's encoding.  The result depends on nothing but the tableau, basis, ub, flip, the options, flags and
 * cutoff: not on the batch length, on graph replay, on the callback or on launch geometry.  The cutoff is not part of what keys
 * the cached graph of a loop: two runs with equal options and different cutoffs each obey their own.  Any m and Cm, with the
 * LDS-or-scratch rule of lpx_bounded_dual_run at 4096.  The cached graphs of all flag sets on one handle are kept apart.
 * LPX_EINVAL before any device check: a flag bit outside the three ("unknown flag"), a NaN cutoff with LPX_BDUAL_CUTOFF, a NULL
 * handle, and the argument errors of lpx_bounded_dual_run.
 *
 * lpx_bounded_node2(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out): lpx_bounded_node with the loop's flags and
 * cutoff passed through to lpx_bounded_dual_run3.  flags = LPX_BDUAL_SKIP_FIXED is lpx_bounded_node bit for bit.  out->status may
 * be LPX_CUTOFF; the pick is then {-1, 0, 0.0, T[m,Cm] as it stands}.  The record is unchanged: passes = events - kind0 - kind1.
 *
 * lpx_solve_bnb_bounded2(p, lower, upper, is_int, o, max_nodes, search_flags, out, info): lpx_solve_bnb_bounded whose nodes are
 * lpx_bounded_node2 calls with flags = LPX_BDUAL_SKIP_FIXED | search_flags; search_flags is a subset of {LPX_BDUAL_LONG_STEP,
 * LPX_BDUAL_CUTOFF}, anything else is LPX_EINVAL.  search_flags = 0 is lpx_solve_bnb_bounded with a bit-equal node log.  With
 * LPX_BDUAL_CUTOFF every node call carries cutoff = best + 1e-6 (the driver's own addition; -inf before the first incumbent).  A
 * node that ends LPX_CUTOFF is counted in pruned_bound and its log record carries status LPX_CUTOFF and z as it stood.
 *
 * lpx_solve_bounded_dual(p, lower, upper, flags, o, out, info): the dual start -- the bounded dual loop as the root solver of the
 * models lpx_solve_bounded refuses.  Preparation is that of lpx_solve_bounded (same validation, same messages, same lower shift)
 * with two differences: a >= row is negated into a <= row (every coefficient and the RHS negated, which is exact), and a negative
 * shifted RHS is accepted.  Precheck, on the host before any device check: a variable whose internal objective-row entry (-c_j
 * for Max, c_j for Min) is below -1e-9 and whose upper bound is +inf cannot be made dual feasible -- LPX_EINVAL with a message
 * naming the first such variable.  Solve: slack basis, lpx_tableau_set_bounds, lpx_tableau_dualize(1e-9),
 * lpx_bounded_dual_run3(flags, cutoff unused: LPX_BDUAL_CUTOFF in flags is LPX_EINVAL here, as is any unknown bit).
 * out and info are laid out as lpx_solve_bounded's; aux = {kind-0 pivots, kind-1 pivots, passes, constant c.l}; the summary ends
 * with a line of the dualize flips and the passes.  Status is LPX_OPTIMAL or LPX_INFEASIBLE (x and optimal_value then describe the
 * tableau as it stands); LPX_ITER_LIMIT is the return value, as in lpx_solve_bounded. */
#define LPX_BDUAL_LONG_STEP 2
#define LPX_BDUAL_CUTOFF 4
int lpx_bounded_dual_run3(lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, lpx_pivot_cb cb, void* user, lpx_stats* st);
int lpx_bounded_node2(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                      lpx_node_record* out);
int lpx_solve_bnb_bounded2(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                           const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                           int search_flags, lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */);
int lpx_solve_bounded_dual(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] or NULL = +inf */,
                           int flags, const lpx_solve_opts* o, lpx_result* out, lpx_bounded_info* info /* or NULL */);

/* ---- the on-chip form of a node (not in the reference; csrc/lpx_bounded_node.hip) --
 * lpx_bounded_node3(t, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, form, out): lpx_bounded_node2 with a choice of
 * how the node is evaluated.  form = LPX_NODE_LAUNCHES is lpx_bounded_node2, bit for bit.  LPX_NODE_ONCHIP evaluates the whole
 * node -- the bound edit, the dual-feasibility flips, the flagged dual loop with its rank-1 updates, the branch pick -- in ONE
 * kernel launch of one workgroup with the live window in the LDS of one compute unit; the host makes one launch and one wait.
 * Every output is bit-equal to the launches form on the same inputs: the record, the trace, the tableau, basis, flip, ub, lo,
 * lpx_bounded_counts and the status (LPX_OPTIMAL, LPX_INFEASIBLE, LPX_ITER_LIMIT, LPX_CUTOFF), and so is everything read from the
 * handle afterwards (lpx_tableau_download / _trace / _bound_state / _bounded_solution / _snapshot / _restore, a following node of
 * either form).  LPX_NODE_AUTO is LPX_NODE_ONCHIP iff lpx_bounded_node_fits(R, C) for the live shape, else LPX_NODE_LAUNCHES.
 * lpx_bounded_node_fits(R, C): pure host arithmetic, no device check.  1 iff R >= 2, C >= 1 and
 *   8 * (R * (C | 1) + C + max(R, C)) <= 160 KiB - 2 KiB
 * (the tile with an odd row stride, the bounds, one array shared by the ratios, the pivot column, the flip list and the pick; 2 KiB
 * are kept for the kernel's reduction scratch).  It holds whenever R >= 2 and R*C + 2*(R + C) <= 18000.
 * Argument errors are those of lpx_bounded_node2 with the new name in front, plus an unknown form; all are checked before any
 * device check and leave the handle untouched, and so is LPX_NODE_ONCHIP on a shape that does not fit ("does not fit").  An
 * unrepairable column and upper = +inf on a flipped column are found by the kernel, before it has touched the tableau: LPX_EINVAL
 * with the messages of lpx_bounded_node2, the handle as it was.  resident = 1 stays LPX_EINVAL; batch, use_graph and profile are
 * not read by the on-chip form.
 *
 * lpx_solve_bnb_bounded3(p, lower, upper, is_int, o, max_nodes, search_flags, node_form, out, info): lpx_solve_bnb_bounded2 whose
 * nodes are lpx_bounded_node3(form = node_form) calls.  node_form = LPX_NODE_LAUNCHES is the existing driver with a bit-equal
 * log; the other forms give the same log too.  An unknown node_form is LPX_EINVAL before any device check; LPX_NODE_ONCHIP with a
 * root that does not fit is LPX_EINVAL with a message before the search starts. */
#define LPX_NODE_LAUNCHES 0
#define LPX_NODE_ONCHIP 1
#define LPX_NODE_AUTO 2
int lpx_bounded_node_fits(int R, int C);
int lpx_bounded_node3(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                      int flags, double cutoff, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                      int form, lpx_node_record* out);
int lpx_solve_bnb_bounded3(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                           const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                           int search_flags, int node_form, lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */);

/* ---- a batch of on-chip nodes per launch, and a search by W divers (not in the reference; csrc/lpx_bounded_node.hip,
 * csrc/lpx_node_batch.cpp, csrc/host/bnb_bounded.cpp) --
 * lpx_tableau_clone(src, out): a new handle on the source's device with the source's capacity (at least the live window), holding
 * device-to-device copies of the live R x C window, the basis, the contiguous RHS copy, ub / lo / flip with the lo-used mark (if
 * the source has bounds), and the loop state record with its host mirror.  Not copied: the snapshot, the trace (lpx_tableau_trace
 * on the clone reports no entry until the clone's first run), the cached graphs, the callbacks, the node slabs; the clone's
 * lpx_bounded_counts are zero.  The source is left bit for bit as it was.  lpx_tableau_download / _shape / _bound_state /
 * _bounded_solution read the same bits from both handles, and any run or node call on the clone gives the bits it gives on the
 * source.  A source that lpx_multi_run_some left in the middle of a run is refused (LPX_EINVAL): what continues such a run is not
 * part of the copy.  That and a NULL argument are LPX_EINVAL before any device check; no device: LPX_EDEVICE.
 *
 * lpx_node_batch_create(W, handles, out): a batch that BORROWS W handles (1 <= W <= 1024; they outlive the batch, and the caller
 * destroys them).  They must be pairwise distinct and on one device, each with bounds set for its live shape and with a live shape
 * that satisfies lpx_bounded_node_fits; the shapes may differ.  Anything else is LPX_EINVAL before any device check.  The batch
 * owns one pinned slab (a parameter record, the node's header with its triples behind it, and the result record per entry), the
 * device staging of the edits and one device copy of the integer mask, which is sent again only when its bytes change; the
 * buffers grow to twice the need, never inside a call whose need they already hold.
 *
 * lpx_node_batch_run(b, B, slot, K, cols, lower, upper, o, flags, cutoff, nint, is_int, tol, out, rc): ONE kernel launch of B
 * workgroups evaluates B nodes, 1 <= B <= W; entry i runs on handles[slot[i]] with the K[i] triples that follow those of the
 * entries before it in cols / lower / upper (sum of K entries each).  The slots are pairwise distinct.  o, flags, nint, is_int and
 * tol are shared by all entries; cutoff[i] is read only with LPX_BDUAL_CUTOFF.
 *   Contract: for every i, out[i] and rc[i] and everything readable from handles[slot[i]] afterwards -- tableau, basis, ub, lo,
 *   flip, trace, lpx_bounded_counts, the solution, the host mirror of the state, a following node of any form -- are bit-equal to
 *   what lpx_bounded_node3(handles[slot[i]], K[i], ..., cutoff[i], ..., LPX_NODE_ONCHIP, &out[i]) gives on a handle in the same
 *   state.  The result does not depend on B, on the slot numbers, on the other entries, or on how many workgroups run at once: the
 *   workgroups share nothing and never wait on one another, and every loop of the kernel is bounded, so a launch ends whatever B
 *   is (B may exceed the number of compute units).  A handle not named in slot is untouched.
 *   Steady-state host work: the slab is written, the launch is ordered behind outstanding work on the handles' streams, ONE kernel
 *   launch, ONE wait, B records read.
 *   Errors: every argument error of lpx_bounded_node3 is checked for every entry before anything is written; further argument
 *   errors are a NULL slot, K, out or rc, B outside [1, W], a NULL batch, a slot out of range or repeated, a NULL cutoff with
 *   LPX_BDUAL_CUTOFF.  All are LPX_EINVAL before any device check and touch no handle; the message of an entry's error starts
 *   "lpx_node_batch_run: entry i:".  The two refusals the kernel finds (an unrepairable column, upper = +inf on a flipped column)
 *   are per entry: rc[i] = LPX_EINVAL, out[i].unrepairable is set, that handle is as it was, the other entries complete, the call
 *   returns 0 and lpx_last_error carries the lowest refused entry's message (the text of lpx_bounded_node2 behind the entry's
 *   prefix).  Otherwise the call returns 0 and rc[i] is the entry's status.
 *
 * lpx_solve_bnb_bounded4(p, lower, upper, is_int, o, max_nodes, search_flags, divers, out, info, dinfo): the search of
 * lpx_solve_bnb_bounded3 with every node on chip, by W = divers handles diving at once (1 <= W <= 1024, else LPX_EINVAL before any
 * device check).  Validation, root solve, result record, summary and value conversion are those of lpx_solve_bnb_bounded3; a root
 * that does not fit is LPX_EINVAL with its message, before the search.  Diver 0 is the root's handle, divers 1 .. W-1 are
 * lpx_tableau_clone's of it taken after the root solve.  Each diver has its own current bounds and its own stack of (depth, path);
 * diver 0 starts with the root node, the others empty; best starts at -inf.  One round, in this order (the order is part of the
 * contract: the log depends on it):
 *   1. Limit: max_nodes > 0 and nodes >= max_nodes ends the solve with the node-limit return of lpx_solve_bnb_bounded.
 *   2. Steal: for d = 0 .. W-1 in order with diver d's stack empty: v = the diver with the longest stack, ties to the lowest
 *      index, lengths as they stand now; if that stack holds at least 2 entries its bottom (oldest) entry moves to d and steals++;
 *      otherwise d sits the round out.
 *   3. Pop: for d ascending, each diver with a non-empty stack pops its top while nodes + popped < max_nodes (or no limit).  The
 *      node's columns are those whose bounds differ from diver d's current bounds, in ascending column order.
 *   4. Evaluate: one lpx_node_batch_run over the popped nodes, flags = LPX_BDUAL_SKIP_FIXED | search_flags, every entry with
 *      cutoff = best + 1e-6 as best stood at the start of the round.  largest_batch is the largest B seen.
 *   5. Decide: the records in ascending diver order, each exactly as lpx_solve_bnb_bounded treats a node: nodes++, the counters,
 *      the log record with round[] and diver[]; LPX_ITER_LIMIT ends the solve at that record (later records of the round are
 *      dropped); infeasible; LPX_CUTOFF or z <= best + 1e-6 against best as updated by lower-index divers of the same round;
 *      incumbent (x from lpx_tableau_bounded_solution on that diver's handle); otherwise the floor child, then the ceil child, go
 *      onto diver d's own stack.
 *   6. Repeat while any stack is non-empty.
 * divers = 1 is lpx_solve_bnb_bounded3(..., LPX_NODE_ONCHIP, ...) with a bit-equal log.  The result is a function of the model, the
 * options, the flags and W alone; it does not depend on timing.  Another W visits other nodes, and the plain dual loop
 * (search_flags without LPX_BDUAL_LONG_STEP) can meet a node on which it makes max_iter events, which ends the solve with
 * LPX_ITER_LIMIT as in lpx_solve_bnb_bounded: measured on binary_ip(128, 64), where W = 4, 64 and 256 end that way and W = 1 and 16
 * do not.  LPX_BDUAL_LONG_STEP makes such a node rare, not impossible: a search with the long step ends
 * that way under strong branching.  The cause is cycling at a dual degenerate vertex;
 * lpx_solve_bnb_bounded7 with stall_events > 0 ends such nodes (the stall guard below).  dinfo (or NULL): rounds, steals, largest_batch and, per log
 * record, the round and the diver that evaluated it ([info->n_log] each); free with lpx_bnb_divers_info_free. */
typedef struct lpx_node_batch lpx_node_batch;
typedef struct lpx_bnb_divers_info {
    int64_t rounds, steals, largest_batch;
    int32_t* round;          /* [n_log of the lpx_bnb_bounded_info] */
    int32_t* diver;          /* [n_log] */
} lpx_bnb_divers_info;
int  lpx_tableau_clone(const lpx_tableau* src, lpx_tableau** out);
int  lpx_node_batch_create(int W, lpx_tableau* const* handles, lpx_node_batch** out);
void lpx_node_batch_destroy(lpx_node_batch* b);
int  lpx_node_batch_run(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const int32_t* K /* [B] */,
                        const int32_t* cols, const double* lower, const double* upper /* concatenated, sum of K */,
                        const lpx_run_opts* o, int flags, const double* cutoff /* [B]; read only with LPX_BDUAL_CUTOFF */,
                        int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                        lpx_node_record* out /* [B] */, int32_t* rc /* [B] */);
int  lpx_solve_bnb_bounded4(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */,
                            lpx_bnb_divers_info* dinfo /* or NULL */);
void lpx_bnb_divers_info_free(lpx_bnb_divers_info* dinfo);

/* ---- the plunge: up to D nodes per diver and launch, the tableau staying in LDS (not in the reference;
 * csrc/lpx_bounded_plunge.hip, csrc/lpx_node_batch.cpp, csrc/host/bnb_bounded.cpp) --
 * lpx_node_batch_plunge(b, B, slot, K, cols, lower, upper, o, flags, cutoff, prune, depth, D, nint, is_int, tol, out, steps, rc):
 * lpx_node_batch_run whose entry i is a CHAIN of up to depth[i] nodes (1 <= depth[i] <= D <= 64) evaluated by one workgroup in ONE
 * launch; the tile is loaded into LDS once and stored once per launch.  out is [B * D], entry-major.
 *   The chain of entry i.  Node 0 is the entry's K[i] triples.  After node s its record is written, and the chain goes on iff
 *   status == LPX_OPTIMAL, pick.var >= 0, !(pick.z <= prune[i]) and s + 1 < depth[i].  Node s + 1 is then the ceil child of node s:
 *   the one triple (var, ceil(x_var), lo[var] + ub[var]) in the handle's own terms (lpx_tableau_bound_state).  The sum is the
 *   column's current upper bound exactly when the bounds of the integer columns are finite and integral, which is why a
 *   depth[i] > 1 is refused (LPX_EINVAL) unless every column j < nint that is_int lets in is KNOWN to the handle to have such
 *   bounds: lpx_tableau_set_bounds and every accepted bound edit record it on the host (a clone, a snapshot and a restore carry
 *   it), and the entry's own triples count.  prune[i] is always read (-inf: nothing is pruned); cutoff[i] only with LPX_BDUAL_CUTOFF.
 *   Contract: for every i, out[i*D .. i*D + steps[i]), rc[i] and everything readable from handles[slot[i]] afterwards -- tableau,
 *   basis, ub, lo, flip, trace, lpx_bounded_counts, the solution, the state's host mirror, a following node of any form -- are
 *   bit-equal to steps[i] calls of lpx_bounded_node3(..., LPX_NODE_ONCHIP, ...) one after another on a handle in the same state:
 *   the first with the entry's triples, each later one with the one ceil triple above, the same cutoff[i] and flags, stopped by
 *   the rule above.  The trace is that of the last node.  rc[i] is the last node's status.  D = 1 gives lpx_node_batch_run.
 *   Errors: those of lpx_node_batch_run under the new name, plus a NULL depth, steps or prune, D outside [1, 64], a depth[i]
 *   outside [1, D], a NaN prune[i] and the integrality rule above; all LPX_EINVAL before any device check, an entry's message
 *   starting "lpx_node_batch_plunge: entry i:".  A refusal the kernel finds at node 0 is lpx_node_batch_run's: rc[i] = LPX_EINVAL,
 *   steps[i] = 0, out[i*D].unrepairable set, the handle as it was.  One found at node s + 1 (the tile is dirty by then: ub / lo of
 *   the one column are put back and the tile is stored as node s left it) gives rc[i] = LPX_EINVAL, steps[i] = s + 1 completed
 *   nodes, out[i*D + steps[i]].unrepairable set and the handle as after node s; the message names "node s + 1".
 *
 * lpx_solve_bnb_bounded5(p, lower, upper, is_int, o, max_nodes, search_flags, divers, plunge, out, info, dinfo, pinfo):
 * lpx_solve_bnb_bounded4 whose divers plunge, 1 <= plunge = D <= 64 (else LPX_EINVAL before any device check).  Everything around
 * the search is lpx_solve_bnb_bounded4's.  One round, in this order (the order is part of the contract):
 *   1. Limit and 2. Steal: as lpx_solve_bnb_bounded4.
 *   3. Pop: for d ascending, each diver with a non-empty stack gets the cap depth_d = D, or with max_nodes > 0
 *      min(D, max_nodes - nodes - the caps handed out to lower divers in this round); the first diver whose cap would be 0 ends the
 *      popping.  The node's columns are those whose bounds differ from the diver's current bounds, ascending.
 *   4. Evaluate: ONE lpx_node_batch_plunge, flags = LPX_BDUAL_SKIP_FIXED | search_flags, every entry with prune = best + 1e-6 as
 *      best stood at the start of the round, and with cutoff = that value under LPX_BDUAL_CUTOFF.  launched grows by the records
 *      the kernel wrote, longest_chain is the longest chain seen.
 *   5. Decide: divers ascending, each diver's records in chain order, every record exactly as lpx_solve_bnb_bounded4 treats a
 *      node (nodes++, the counters, the log record with round[], diver[] and step[], the record's index in its chain; record s
 *      has depth = the popped node's depth + s and K = 1 for s > 0):
 *        LPX_ITER_LIMIT ends the solve at that record;  infeasible ends the chain;
 *        LPX_CUTOFF or z <= best + 1e-6, best as updated by lower-index divers of this round: pruned by bound.  The kernel may
 *          have gone on past such a record, against the older best: the later records of the chain are DROPPED -- not counted,
 *          not logged, dropped grows by their number;
 *        an incumbent is always the last record of its chain, so lpx_tableau_bounded_solution on the diver's handle is its x;
 *        a branch followed by a further record pushes only the floor child: the ceil child IS that next record;
 *        a branch that is the last record of its chain pushes the floor child, then the ceil child.
 *      The diver's current bounds afterwards are those of the last node the kernel evaluated, dropped or not.
 *   6. Repeat while any stack is non-empty.
 * plunge = 1 gives lpx_solve_bnb_bounded4's log, round[] and diver[] bit for bit.  divers = 1 with any plunge gives the log of
 * lpx_solve_bnb_bounded3(..., LPX_NODE_ONCHIP, ...) bit for bit with dropped = 0: within a chain no incumbent appears before the
 * last record, so the sequential best is the round's.  pinfo (or NULL): launched, dropped, longest_chain and per log record its
 * step ([info->n_log]); free with lpx_bnb_plunge_info_free. */
typedef struct lpx_bnb_plunge_info {
    int64_t launched, dropped, longest_chain;
    int32_t* step;           /* [n_log of the lpx_bnb_bounded_info] */
} lpx_bnb_plunge_info;
int  lpx_node_batch_plunge(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const int32_t* K /* [B] */,
                           const int32_t* cols, const double* lower, const double* upper /* concatenated, sum of K */,
                           const lpx_run_opts* o, int flags, const double* cutoff /* [B]; read only with LPX_BDUAL_CUTOFF */,
                           const double* prune /* [B] */, const int32_t* depth /* [B] */, int D,
                           int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                           lpx_node_record* out /* [B*D], entry-major */, int32_t* steps /* [B] */, int32_t* rc /* [B] */);
int  lpx_solve_bnb_bounded5(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, int plunge /* D, 1..64 */, lpx_result* out,
                            lpx_bnb_bounded_info* info /* or NULL */, lpx_bnb_divers_info* dinfo /* or NULL */,
                            lpx_bnb_plunge_info* pinfo /* or NULL */);
void lpx_bnb_plunge_info_free(lpx_bnb_plunge_info* pinfo);

/* -- strong branching by on-chip probes (kernel: csrc/lpx_bounded_probe.hip; host: csrc/lpx_tableau_bounded.cpp,
 * csrc/lpx_node_batch.cpp, csrc/host/bnb_bounded.cpp) --
 * A PROBE evaluates one child of a solved node on a private copy and reports how the child ends; the handle is only read.  One
 * launch of a grid of (2 * cand_max, B) independent workgroups probes up to cand_max candidates of B handles, both children each.
 *
 * lpx_bounded_probe(t, o, flags, cutoff, prune, nint, is_int, tol, cand_max, probe_iter, head, out): probes handle t AS IT STANDS,
 * one launch and one wait.  NOTHING of the handle changes: tableau, bounds, lower shifts, flip states, basis, RHS copy, state
 * record, trace and counts read the same before and after.  The handle must have bounds and fit the on-chip form of the node
 * (lpx_bounded_node_fits).
 *   Nothing to probe: head = {0, 0, T[m,Cm]} and every out[w].status = LPX_PROBE_NONE when the handle's loop state (the status
 *   its last run or node left on the device) is not LPX_OPTIMAL, or when T[m,Cm] <= prune (prune = -inf: never).
 *   Candidates: x_j and its fraction f for j < nint exactly as lpx_tableau_branch_pick forms them (mask, tol, lo where the handle
 *   has stored one); the candidates are ordered by (|f - 0.5| ascending, j ascending), with comparisons only.  head.candidates
 *   is their number, head.count = min(candidates, cand_max) of them are probed, head.z = T[m,Cm].
 *   out[2 c + d] is the probe of candidate c (in that order), direction d: d = 0 the floor child [lo[j], floor(x_j)], d = 1 the
 *   ceil child [ceil(x_j), lo[j] + ub[j]] (one addition).  Records with c >= count have status LPX_PROBE_NONE.
 *   The record {status, events, kind0, kind1, flips, z} is bit-equal to what
 *   lpx_bounded_node3(clone, 1, {var}, {lower}, {upper}, o with max_iter = probe_iter, flags, cutoff, ..., LPX_NODE_ONCHIP) reports
 *   on an lpx_tableau_clone of the handle; var, dir, x_var, lower, upper say which call that is.  A child that call refuses
 *   (LPX_EINVAL: upper below lower, which needs a bound that is not integral; an unrepairable column) has status -1 and zeros.  probe_iter = 0 gives LPX_ITER_LIMIT with no event.
 *   LPX_EINVAL before any device check, the handle untouched, every message starting "lpx_bounded_probe:": a NULL t, head or out;
 *   cand_max outside [1, 32]; probe_iter < 0; a NaN prune; an unknown flag; a NaN cutoff with LPX_BDUAL_CUTOFF; nint outside
 *   [0, C-1]; tol outside [0, 0.5); no bounds; resident = 1; a negative or NaN eps; a shape that does not fit.  No device:
 *   LPX_EDEVICE; there is no host fallback.
 *
 * lpx_node_batch_run_probe(b, B, slot, K, cols, lower, upper, o, flags, cutoff, prune, nint, is_int, tol, cand_max, probe_iter,
 * out, head, probes, rc): the launch of lpx_node_batch_run and, behind it on the same stream, the probe launch on the same
 * entries, with ONE wait for both.  out and rc are lpx_node_batch_run's, bit for bit, and so is every handle afterwards; head[i]
 * and probes[i * 2 * cand_max + w] are what lpx_bounded_probe(handles[slot[i]], o, flags, cutoff[i], prune[i], ...) gives on the
 * handle after its node.  An entry whose node the kernel refused has head {0, 0, z as it stands} and no probe.  The probes share
 * the node's flags and o (max_iter replaced by probe_iter).  Errors: those of lpx_node_batch_run under the new name, plus a NULL
 * prune, head or probes, cand_max outside [1, 32], probe_iter < 0 and "entry i: prune is NaN".
 *
 * lpx_solve_bnb_bounded6(p, lower, upper, is_int, o, max_nodes, search_flags, divers, branching, cand_max, probe_iter, out, info,
 * dinfo, sinfo): the search of lpx_solve_bnb_bounded4 with a branching rule.  branching = LPX_BRANCH_MOST_FRACTIONAL is
 * lpx_solve_bnb_bounded4 bit for bit, with no probe launch (cand_max and probe_iter are still checked).  branching =
 * LPX_BRANCH_STRONG changes two steps of its round:
 *   4. Evaluate: ONE lpx_node_batch_run_probe, every entry with prune = best + 1e-6 as best stands at the start of the round (and
 *      cutoff = that value under LPX_BDUAL_CUTOFF), flags = LPX_BDUAL_SKIP_FIXED | search_flags for nodes and probes alike.
 *   5. Decide: as lpx_solve_bnb_bounded4 up to the point where a node branches.  If its head.count >= 1, with z the node's z:
 *      gain of a probe = 1e12 if it ended LPX_INFEASIBLE or LPX_CUTOFF, 1e-6 if it was refused (status -1), else
 *      min(max(z - z_probe, 1e-6), 1e12) (LPX_ITER_LIMIT included).  score of a candidate = gain_floor * gain_ceil.  The
 *      branching variable is the candidate of the FIRST maximum score in candidate order, x_var its value; the children are
 *      formed from it as before.  A child is DEAD if its probe ended LPX_INFEASIBLE or LPX_CUTOFF, or ended LPX_OPTIMAL with
 *      z_probe <= best + 1e-6, best as it stands at this decision.  A dead child is not pushed; it counts in pruned_by_probe and
 *      not in nodes.  The live children are pushed floor first, so the ceil child is explored first.  The log's var is the
 *      chosen variable.  head.count = 0 on a branching node: the rule of lpx_solve_bnb_bounded4.
 *   sinfo: probe_launches (rounds with a probe launch), probes (records that ran: status != LPX_PROBE_NONE), probe_events (the sum
 *   of their events), probe_limit (those that ended LPX_ITER_LIMIT), pruned_by_probe, changed_picks (branching nodes whose
 *   variable differs from candidate 0, the pick of lpx_tableau_branch_pick).  Plain counters: lpx_bnb_strong_info_free zeroes it.
 *   LPX_EINVAL before any device check: those of lpx_solve_bnb_bounded4 under the new name, branching outside {0, 1}, cand_max
 *   outside [1, 32], probe_iter < 0.  The result is a function of the model, the options, the flags, W, cand_max and probe_iter.
 *   The rule visits other nodes than lpx_solve_bnb_bounded4, so what that entry says about a node that makes max_iter events
 *   holds here for other searches: binary_ip(128, 64) with both flags, W = 1, cand_max = 4 and ample probes ends that way
 *   (DESIGN.md section 4.20).  The stall guard below does not reach the probes or this search. */
#define LPX_PROBE_NONE (-2)
#define LPX_BRANCH_MOST_FRACTIONAL 0
#define LPX_BRANCH_STRONG 1
typedef struct lpx_probe_head {          /* 16 bytes */
    int32_t count;         /* candidates probed: min(candidates, cand_max); 0 = nothing was probed */
    int32_t candidates;    /* fractional integer columns */
    double z;              /* T[m,Cm] of the handle */
} lpx_probe_head;
typedef struct lpx_probe_record {        /* 64 bytes */
    int32_t status;        /* LPX_OPTIMAL / LPX_INFEASIBLE / LPX_ITER_LIMIT / LPX_CUTOFF; -1 = refused; LPX_PROBE_NONE = no probe */
    int32_t events, kind0, kind1;        /* events of the child's dual loop, and its pivots per kind */
    int32_t flips;         /* dual-feasibility flips of the child */
    int32_t var, dir;      /* column; 0 = floor child, 1 = ceil child */
    int32_t pad;
    double x_var;          /* value of the column at the node */
    double lower, upper;   /* the child's bounds on it, as lpx_bounded_node3 takes them */
    double z;              /* T[m,Cm] of the child where its loop stopped */
} lpx_probe_record;
typedef struct lpx_bnb_strong_info {     /* 48 bytes */
    int64_t probe_launches, probes, probe_events, probe_limit, pruned_by_probe, changed_picks;
} lpx_bnb_strong_info;
int  lpx_bounded_probe(lpx_tableau* t, const lpx_run_opts* o, int flags, double cutoff, double prune,
                       int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol, int cand_max /* 1..32 */,
                       int probe_iter, lpx_probe_head* head, lpx_probe_record* out /* [2*cand_max] */);
int  lpx_node_batch_run_probe(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const int32_t* K /* [B] */,
                              const int32_t* cols, const double* lower, const double* upper /* concatenated, sum of K */,
                              const lpx_run_opts* o, int flags, const double* cutoff /* [B]; read only with LPX_BDUAL_CUTOFF */,
                              const double* prune /* [B] */, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                              int cand_max /* 1..32 */, int probe_iter, lpx_node_record* out /* [B] */, lpx_probe_head* head /* [B] */,
                              lpx_probe_record* probes /* [B*2*cand_max], entry-major */, int32_t* rc /* [B] */);
int  lpx_solve_bnb_bounded6(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, int branching, int cand_max /* 1..32 */, int probe_iter,
                            lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */, lpx_bnb_divers_info* dinfo /* or NULL */,
                            lpx_bnb_strong_info* sinfo /* or NULL */);
void lpx_bnb_strong_info_free(lpx_bnb_strong_info* sinfo);

/* ---- the stall guard: Bland's rule once a node stops making progress (not in the reference; csrc/lpx_bounded_guard.hip,
 * csrc/lpx_node_batch.cpp, csrc/host/bnb_bounded.cpp) --
 * The leaving rule of lpx_bounded_dual_run (most negative infeasibility) with the hysteresis ratio test has no anti-cycling
 * property: on a dual degenerate vertex of an integer model the loop can repeat a sequence of bases for ever, the objective
 * standing still, until max_iter ends the node and with it the search.  The guard is an integer argument, not a flag:
 * stall_events = S >= 0, and S = 0 gives the existing loop bit for bit.  For S > 0 the loop of lpx_bounded_dual_run3 keeps two
 * more values per node evaluation:
 *   z_ref   starts as T[m,Cm] as it stands when the loop is entered, after the edit and the dual-feasibility flips;
 *   stall   starts at 0.
 * At the top of every trip, behind step 1 and step 1b: if T[m,Cm] < z_ref - eps (one subtract, one compare), then z_ref = T[m,Cm]
 * and stall = 0.  The trip runs in BLAND MODE iff stall >= S.  Every pivot, in either mode, adds 1 to stall; passes of the long
 * step do not.  A trip in Bland mode differs from an ordinary trip in three places only:
 *   2.  Leaving row: among the rows with w_i < -eps, w_i exactly as in step 2, the row whose basic column index basis[i] is
 *       least (equal indices cannot occur in a basis; the lowest row would win).  None: LPX_OPTIMAL.  Kind and complement as ever.
 *   4.  Entering column: the ratios rho[j] formed once, exactly as in step 4, LPX_BDUAL_SKIP_FIXED honoured.  mn = their minimum;
 *       mn = +inf: LPX_INFEASIBLE.  Otherwise q = the lowest j with rho[j] <= mn + ratio_tol (one addition).  There is no
 *       hysteresis scan.  (A negative ratio_tol leaves no such j; q is then the first index of the minimum.)
 *   4.1-4.5  No passes of the long step.
 * The pivot arithmetic, the trace entry, kind0 / kind1, the cutoff test and the event limit are unchanged.  Bland's rule cannot
 * cycle while it is on, and it is on until the objective has moved by more than eps, so a node either makes progress every S + a
 * bounded number of pivots or ends.  lpx_guard_record reports the pivots made in Bland mode and the event index of the first.
 *
 * lpx_bounded_node4(t, K, cols, lower, upper, o, flags, cutoff, stall_events, nint, is_int, tol, form, out, guard): stall_events = 0
 * is lpx_bounded_node3 in every form, bit for bit (same kernels), guard = {0, -1}.  stall_events > 0 needs the on-chip form and
 * runs the guarded kernel: ONE launch, ONE wait, the same LDS rule (lpx_bounded_node_fits).  LPX_EINVAL before any device check:
 * stall_events < 0 ("stall_events is negative"); stall_events > 0 with LPX_NODE_LAUNCHES, or with LPX_NODE_AUTO on a shape that
 * does not fit ("the stall guard has no launches form"); and the argument errors of lpx_bounded_node3 with the new name in front.
 * guard may be NULL.  What the call leaves on the handle is what lpx_bounded_node3 leaves.
 *
 * lpx_node_batch_run2(b, B, slot, K, cols, lower, upper, o, flags, cutoff, stall_events, nint, is_int, tol, out, guard, rc):
 * lpx_node_batch_run's contract word for word, with lpx_bounded_node4(..., stall_events, ..., LPX_NODE_ONCHIP, &out[i], &guard[i])
 * as the single-node equal of entry i and "lpx_node_batch_run2" in front of the messages; stall_events is one value for the batch
 * and a negative one is LPX_EINVAL.  stall_events = 0 is lpx_node_batch_run bit for bit.  guard ([B]) may be NULL.
 *
 * lpx_solve_bnb_bounded7(p, lower, upper, is_int, o, max_nodes, search_flags, divers, stall_events, out, info, dinfo, ginfo): the
 * search of lpx_solve_bnb_bounded4 with step 4 done by lpx_node_batch_run2(stall_events).  stall_events = 0 is
 * lpx_solve_bnb_bounded4 bit for bit.  ginfo (or NULL): guarded_nodes (nodes with a pivot in Bland mode), bland_events (those
 * pivots) and max_events (the most events any one node made); plain counters, no free function.  LPX_EINVAL before any device
 * check: those of lpx_solve_bnb_bounded4 under the new name and stall_events < 0.  On a search where the guard never fires the
 * log is lpx_solve_bnb_bounded4's bit for bit.  stall_events = 50 is a reasonable value (DESIGN.md section 4.21 has counts at 20,
 * 50 and 200).  The launches form, the plunge, the probes and strong branching have no guard. */
typedef struct lpx_guard_record {        /* 8 bytes */
    int32_t bland_events;  /* pivots made in Bland mode */
    int32_t first_bland;   /* event index of the first of them, -1 = none */
} lpx_guard_record;
typedef struct lpx_bnb_guard_info {      /* 24 bytes */
    int64_t guarded_nodes, bland_events, max_events;
} lpx_bnb_guard_info;
int  lpx_bounded_node4(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                       int flags, double cutoff, int stall_events, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                       int form, lpx_node_record* out, lpx_guard_record* guard /* or NULL */);
int  lpx_node_batch_run2(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const int32_t* K /* [B] */,
                         const int32_t* cols, const double* lower, const double* upper /* concatenated, sum of K */,
                         const lpx_run_opts* o, int flags, const double* cutoff /* [B]; read only with LPX_BDUAL_CUTOFF */,
                         int stall_events, int nint, const uint8_t* is_int /* [nint] or NULL = all */, double tol,
                         lpx_node_record* out /* [B] */, lpx_guard_record* guard /* [B] or NULL */, int32_t* rc /* [B] */);
int  lpx_solve_bnb_bounded7(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, int stall_events, lpx_result* out,
                            lpx_bnb_bounded_info* info /* or NULL */, lpx_bnb_divers_info* dinfo /* or NULL */,
                            lpx_bnb_guard_info* ginfo /* or NULL */);

/* ---- the bounded primal loop on chip: one launch per LP, a batch of LPs per launch -------------------------------------------
 *
 * The on-chip form of lpx_bounded_run (kernels in lpx_bounded_primal.hip): ONE launch of one workgroup runs
 * the whole loop of the contract "bounded-variable primal simplex" above, steps 1-4 unchanged, with the live window in the LDS of
 * one compute unit.  The LDS layout is the on-chip node's, so lpx_bounded_node_fits(R, C) is the fit rule unchanged.
 *
 * lpx_bounded_run2(t, o, form, cb, user, st): form is LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP or LPX_NODE_AUTO.
 *   LPX_NODE_LAUNCHES is lpx_bounded_run bit for bit: the same code path, the same cached graphs.
 *   LPX_NODE_ONCHIP makes ONE launch and ONE wait.  Of the options eps, ratio_tol and max_iter are read; batch, use_graph and
 *     profile are not.  st (or NULL): pivots = kind-0 + kind-1 pivots, launches = 1, loop_ms the host wall of the call's launch and
 *     wait.  The status and everything readable from the handle afterwards are bit-equal to the launches form on a handle in the
 *     same state: the tableau, basis, ub, lo, flip, the trace (entries beyond the trace capacity are dropped, as there),
 *     lpx_bounded_counts, lpx_tableau_bounded_solution, snapshot and restore, a following lpx_bounded_run and a following
 *     lpx_bounded_node* of any form.  A handle without bounds runs with every ub = +inf and is then lpx_primal_run bit for bit, as
 *     the launches form is.
 *   LPX_NODE_AUTO is LPX_NODE_ONCHIP iff lpx_bounded_node_fits(R, C) for the live shape and cb == NULL, else LPX_NODE_LAUNCHES.
 *   LPX_EINVAL before any device check, the handle untouched: an unknown form ("unknown form"); LPX_NODE_ONCHIP on a shape that
 *   does not fit ("does not fit") or with a callback ("no per-event callback": the events of one launch are not reported one by
 *   one); resident = 1; and the argument errors of lpx_bounded_run with the new name in front.
 *
 * lpx_node_batch_primal(b, B, slot, o, out, rc): ONE launch of B workgroups solves B LPs on the batch's handles, 1 <= B <= W, the
 * slots pairwise distinct.  For every i, out[i], rc[i] (the status, or a negative error) and everything readable from
 * handles[slot[i]] are bit-equal to lpx_bounded_run2(handles[slot[i]], o, LPX_NODE_ONCHIP, NULL, NULL, NULL) on a handle in the
 * same state.  The workgroups share nothing, so the result of an entry is independent of B, of the slot numbers and of the other
 * entries; B may exceed the number of compute units.  Argument errors are checked for every entry before anything is written and
 * are LPX_EINVAL before any device check with no handle touched: null batch / slot / out / rc, B outside [1, W], a slot outside
 * [0, W), a repeated slot, resident = 1, a live shape that changed since lpx_tableau_set_bounds or does not fit.  The steady state
 * of a call: the slab is written, one launch, one wait, B records are read. */
typedef struct lpx_primal_record {       /* 40 bytes */
    int32_t status;        /* LPX_OPTIMAL, LPX_UNBOUNDED or LPX_ITER_LIMIT */
    int32_t events;        /* pivots and flips */
    int64_t kind0, kind1;  /* pivots whose leaving variable went to zero / to its upper bound */
    int64_t flips;         /* bound flips */
    double  z;             /* T[m, C-1] as the loop left it */
} lpx_primal_record;
int  lpx_bounded_run2(lpx_tableau* t, const lpx_run_opts* o, int form, lpx_pivot_cb cb, void* user, lpx_stats* st);
int  lpx_node_batch_primal(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const lpx_run_opts* o,
                           lpx_primal_record* out /* [B] */, int32_t* rc /* [B] */);

/* The model level.
 * lpx_solve_bounded2(p, lower, upper, o, form, out, info): lpx_solve_bounded whose loop is lpx_bounded_run2(form).
 *   LPX_NODE_LAUNCHES is lpx_solve_bounded with equal results.  LPX_NODE_ONCHIP gives the same out and info apart from
 *   stats.launches (1) and the times; the shape is known on the host after preparation, so a model that does not fit ("does not
 *   fit") and a text_cb ("no per-event callback") are LPX_EINVAL before any device check, behind lpx_solve_bounded's own
 *   validation messages.  LPX_NODE_AUTO is on chip iff the model fits and there is no text_cb.  An unknown form is LPX_EINVAL.
 * lpx_solve_bounded_batch(count, problems, lowers, uppers, o, outs, infos): 1 <= count <= 1024 independent models of any mix of
 *   shapes; lowers / uppers are NULL or hold count pointers (each NULL or [n of that model]); infos is NULL or [count].  All models
 *   are validated and prepared first (an error names the model: "model i: ...") and every one must fit the on-chip form; then the
 *   call makes count handles, ONE lpx_node_batch_primal launch and count results, each equal to
 *   lpx_solve_bounded2(problems[i], ..., LPX_NODE_ONCHIP, &outs[i], &infos[i]).  A model that reaches the iteration limit makes
 *   the call return LPX_ITER_LIMIT ("model i: Iteration limit exceeded.").  On any error outs and infos come back zeroed.
 * lpx_solve_bnb_bounded8(p, lower, upper, is_int, o, max_nodes, search_flags, divers, stall_events, root_form, out, info, dinfo,
 *   ginfo): lpx_solve_bnb_bounded7 whose root is solved by lpx_bounded_run2(root_form).  LPX_NODE_LAUNCHES is
 *   lpx_solve_bnb_bounded7 bit for bit; every form gives a bit-equal node log and a bit-equal result apart from the root's
 *   stats.launches.  An unknown root_form is LPX_EINVAL before any device check ("unknown root_form"); the root's shape always
 *   has to fit, as in lpx_solve_bnb_bounded4.  The plunge and the strong-branching drivers have no root_form. */
int  lpx_solve_bounded2(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] or NULL = +inf */,
                        const lpx_solve_opts* o, int form, lpx_result* out, lpx_bounded_info* info /* or NULL */);
int  lpx_solve_bounded_batch(int count, const lpx_problem* const* problems, const double* const* lowers /* or NULL */,
                             const double* const* uppers /* or NULL */, const lpx_solve_opts* o, lpx_result* outs /* [count] */,
                             lpx_bounded_info* infos /* [count] or NULL */);
int  lpx_solve_bnb_bounded8(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, int stall_events, int root_form, lpx_result* out,
                            lpx_bnb_bounded_info* info /* or NULL */, lpx_bnb_divers_info* dinfo /* or NULL */,
                            lpx_bnb_guard_info* ginfo /* or NULL */);

/* ---- packed batches of small bounded LPs: arrays in, ONE launch, arrays out (csrc/lpx_packed.hip) --------
 *
 * count models of ONE shape (m rows, every row <=; n variables) as contiguous arrays.  A call makes at most one host-to-device
 * copy per input array, ONE kernel launch of count workgroups, one device-to-host copy and one wait, each independent of count;
 * there is no handle, no tableau in device memory and no host work per model.  Workgroup i builds the tableau of model i in the
 * LDS of its compute unit (the preparation of lpx_solve_bounded, bit for bit: Min negates c, b' = b - A l with j ascending and one
 * multiply and one subtract per non-zero l_j, u' = u - l, slack basis), validates it, runs the event loop of the on-chip bounded
 * primal form unchanged and extracts x, the optimum, the record, the basis and the at-upper flags from LDS.
 *
 * A stride is the number of doubles between two models of an array: the packed size (n for c, lower and upper; m*n for A; m for b)
 * or 0, which means ONE copy that every model shares (only that copy is uploaded).  lower / upper may be NULL (0 / +inf).
 *
 * lpx_packed_fits(m, n) == lpx_bounded_node_fits(m + 1, n + m + 1) for m, n >= 1, else 0: pure host arithmetic.
 *
 * lpx_solve_packed(in, o, out, st) returns 0 once the launch ran; the outcome of model i is status[i]: LPX_OPTIMAL, LPX_UNBOUNDED,
 * LPX_ITER_LIMIT (x, value, basis and at_upper are then the point at which the loop stopped), LPX_EINVAL (a lower bound that is
 * not finite, or an upper bound below its lower bound or NaN) or, behind that check, LPX_E_NEG_RHS (a b'_i < -1e-9).  A model with a
 * negative status has x, value, basis and at_upper zeroed and a record of zeros around that status; the other models are unaffected.
 * Of o the fields eps, ratio_tol and max_iter are read; NULL is lpx_default_opts(o, 0).  st (or NULL): pivots = the kind-0 and kind-1
 * pivots of all models, launches = 1, loop_ms the host wall of the copies, the launch and the wait.
 *
 * For every i, status[i], x, value, rec, basis and at_upper are bit-equal to what lpx_solve_bounded2(model i, lower_i, upper_i, o,
 * LPX_NODE_ONCHIP, ...) returns (a negative status[i] is that call's return code), and do not depend on count, on i, on the other
 * models or on whether an array is shared.
 *
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_solve_packed: ": a NULL in, out, c, A, b,
 * status, x or value; count outside [1, 65536]; m or n below 1; a sense other than LPX_MAX / LPX_MIN; a stride that is neither 0
 * nor the packed size; a shape with lpx_packed_fits(m, n) == 0 ("R x C ... does not fit"); resident = 1; more than 1 GiB of input
 * plus output bytes ("too large": chunking is the caller's business).  No device: LPX_EDEVICE.  The device buffers of a call are
 * one arena that is kept for the next call and grows when needed; like the handle cache it lives as long as the process. */
typedef struct lpx_packed_models {
    int32_t count, m, n, sense;        /* one shape for all; every row is <= */
    const double *c, *A, *b;           /* [count][n], [count][m][n] row-major, [count][m] */
    const double *lower, *upper;       /* [count][n] or NULL (0 / +inf) */
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
                                       /* doubles between models: the packed size (n, m*n, m, n, n),
                                          or 0 = ONE copy shared by every model */
} lpx_packed_models;
typedef struct lpx_packed_results {    /* caller-allocated; each of the last three may be NULL */
    int32_t* status;  double* x;  double* value;           /* [count], [count][n], [count] */
    lpx_primal_record* rec;  int32_t* basis;  uint8_t* at_upper;   /* [count], [count][m], [count][n] */
} lpx_packed_results;
int lpx_packed_fits(int m, int n);
int lpx_solve_packed(const lpx_packed_models* in, const lpx_run_opts* o /* or NULL */, const lpx_packed_results* out,
                     lpx_stats* st /* or NULL */);

/* ---- packed batches by a dual start: >= rows and negative right-hand sides (csrc/lpx_packed_dual.hip) ---
 *
 * lpx_solve_packed_dual(in, flags, o, out, st) is lpx_solve_packed for the models lpx_solve_bounded_dual was built for: count models
 * of ONE shape whose rows are <= or >= (rel, [count][m] of LPX_LE / LPX_GE; rel_stride m, or 0 = one copy shared by every model;
 * rel = NULL: every row is <=) and whose shifted right-hand sides may have either sign.  The same arena, the same stream, at most
 * one copy per input array, ONE launch of count workgroups, one read-back and one wait.  Workgroup i
 *   1. builds the tableau of model i in LDS: Min negates c; a >= row is negated while it is stored (every coefficient and b_i:
 *      exact), then b' = b - A l and u' = u - l as in lpx_solve_packed, slack basis; no test of the sign of b';
 *   2. refuses the model (LPX_EINVAL) for a lower bound that is not finite, an upper bound below its lower bound or NaN, a rel
 *      entry that is neither LPX_LE nor LPX_GE, and, behind those, for a column whose objective-row entry is below -1e-9 while its
 *      upper bound is +inf (the precheck of lpx_solve_bounded_dual: no bound flip can make it dual feasible);
 *   3. makes the dual-feasibility flips of lpx_tableau_dualize(1e-9), j ascending;
 *   4. runs the dual loop of lpx_bounded_dual_run3(flags) from the slack basis with o's eps, ratio_tol and max_iter;
 *   5. extracts x, the optimum, the record, the basis, the at-upper flags and the duals from LDS.
 * flags is 0 or LPX_BDUAL_LONG_STEP; any other bit is LPX_EINVAL ("unknown flag"), LPX_BDUAL_CUTOFF included, as in
 * lpx_solve_bounded_dual.  The fit rule is lpx_packed_fits(m, n) unchanged.
 *
 * status[i]: LPX_OPTIMAL, LPX_INFEASIBLE, LPX_ITER_LIMIT or LPX_EINVAL.  For LPX_INFEASIBLE and LPX_ITER_LIMIT the outputs describe
 * the tableau as the loop left it.  A refused model has every output zeroed and a record of zeros around its status; the other
 * models are unaffected.  There is no LPX_E_NEG_RHS here.  Of o the fields eps, ratio_tol and max_iter are read; NULL is
 * lpx_default_opts(o, 1).  st (or NULL): pivots = the kind-0 and kind-1 pivots of all models, launches = 1, loop_ms the host wall.
 *
 * For every i, status, x, value, basis, at_upper and the counts of the record are bit-equal to lpx_solve_bounded_dual(model i,
 * lower_i, upper_i, flags, ...) (at the iteration limit, where that call returns an error, to the contract above), and do not depend
 * on count, on i, on the other models or on whether an array is shared.
 *
 * The duals are objective-row entries with exact sign changes, in the user's sense and on the user's rows:
 *   y[i] = T[m, n+i], negated iff exactly one of (row i is >=, the sense is Min) holds:        y_i = d value / d b_i;
 *   d[j] = T[m, j],   negated iff (the sense is Min) == (column j is flipped):                   d_j = c_j - sum_i y_i A_ij.
 *
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_solve_packed_dual: ": the list of
 * lpx_solve_packed in its order (rel_stride among the strides: neither 0 nor m), then a shared rel (rel_stride 0)
 * holding anything but LPX_LE / LPX_GE, then an unknown flag.  A per-model rel is checked by its workgroup.  No device:
 * LPX_EDEVICE. */
typedef struct lpx_packed_dual_models {
    int32_t count, m, n, sense;        /* one shape for all */
    const double *c, *A, *b;           /* [count][n], [count][m][n] row-major, [count][m] */
    const double *lower, *upper;       /* [count][n] or NULL (0 / +inf) */
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
                                       /* doubles between models: the packed size, or 0 = ONE shared copy */
    const int32_t* rel;                /* [count][m] of LPX_LE / LPX_GE, or NULL = every row is <= */
    int64_t rel_stride;                /* int32 between models: m, or 0 = ONE shared copy */
} lpx_packed_dual_models;
typedef struct lpx_packed_dual_record {  /* 48 bytes */
    int32_t status;        /* LPX_OPTIMAL, LPX_INFEASIBLE, LPX_ITER_LIMIT or LPX_EINVAL */
    int32_t events;        /* pivots and passes of the loop */
    int64_t kind0, kind1;  /* pivots whose leaving variable went to zero / to its upper bound */
    int64_t passes;        /* long-step passes (bound flips inside the ratio test) */
    int64_t dualize_flips; /* dual-feasibility flips in front of the loop */
    double  z;             /* T[m, C-1] as the loop left it */
} lpx_packed_dual_record;
typedef struct lpx_packed_dual_results { /* caller-allocated; each of the last five may be NULL */
    int32_t* status;  double* x;  double* value;           /* [count], [count][n], [count] */
    lpx_packed_dual_record* rec;  int32_t* basis;  uint8_t* at_upper;   /* [count], [count][m], [count][n] */
    double* y;  double* d;                                 /* [count][m], [count][n] */
} lpx_packed_dual_results;
int lpx_solve_packed_dual(const lpx_packed_dual_models* in, int flags, const lpx_run_opts* o /* or NULL */,
                          const lpx_packed_dual_results* out, lpx_stats* st /* or NULL */);

/* ---- packed right-hand-side scenarios warm-started from one solved base (csrc/lpx_packed_warm.hip) ----
 *
 * The commonest packed batch is count right-hand sides of ONE model.  lpx_packed_base_open solves that model once for a base
 * right-hand side and keeps the solved tableau on the device; lpx_packed_base_solve then re-solves count right-hand sides in ONE
 * launch, every workgroup continuing the dual loop from the base's optimal basis.  After any pivots, complements and bound flips the
 * RHS column of a tableau is an affine function of the internal b whose linear part is the slack block (columns n .. n+m-1), so a new
 * right-hand side costs one (m+1) x m product and leaves the objective row, and with it dual feasibility, untouched.
 *
 * lpx_packed_base_open(in, flags, o, base_out, &h) performs, for the base model, exactly steps 1-5 of lpx_solve_packed_dual;
 * base_out (or NULL), the results structure of that call for count = 1, is bit-equal to lpx_solve_packed_dual with count = 1.  In an
 * allocation that the handle owns it keeps on the device: the solved tile, the bounds ub, the basis and the flip bytes, the user's b
 * and rel, the lower bounds and the shift constant.  The fit rule is lpx_packed_fits(m, n).  flags is 0 or LPX_BDUAL_LONG_STEP.  It
 * returns 0 and a handle only when the base ends LPX_OPTIMAL; otherwise it returns that status (LPX_INFEASIBLE, LPX_ITER_LIMIT, or
 * LPX_EINVAL for a model its workgroup refuses) and *h = NULL.  LPX_EINVAL before any device check, the outputs untouched (*h is set
 * to NULL wherever h is given), every message starting "lpx_packed_base_open: ": a NULL in or h; then the list of
 * lpx_solve_packed_dual in its order for count = 1 and shared arrays (a NULL c, A or b; with base_out given, a NULL status, x or
 * value; m or n below 1; the sense; the fit rule; resident = 1; more than 1 GiB; a rel entry that is neither LPX_LE nor LPX_GE; an
 * unknown flag).  No device: LPX_EDEVICE.
 *
 * lpx_packed_base_solve(h, count, b, flags, o, out, st) makes one upload of b ([count][m], the user's right-hand sides), ONE launch
 * of count workgroups, one read-back and one wait, on the arena and the stream of lpx_solve_packed.  Workgroup i
 *   1. copies the base's tile and ub into LDS, the basis and the flip bytes into its own slices;
 *   2. forms delta_k = b_i[k] - b0[k], negated for a >= row; a b_i[k] that is not finite refuses the scenario (LPX_EINVAL: its
 *      outputs zeroed, a record of zeros around the status);
 *   3. updates the RHS column: for every row r = 0 .. m, the objective row included,
 *          acc = T[r][C-1];  for k = 0 .. m-1 ascending with delta_k != 0.0:  prod = T[r][n+k] * delta_k;  acc = acc + prod
 *      (one multiply and one add, separately rounded; no other arithmetic: an all-zero delta leaves every bit as the base left it);
 *   4. runs the dual loop of lpx_bounded_dual_run3(flags) from the base's basis with o's eps, ratio_tol and max_iter
 *      (NULL: lpx_default_opts(o, 1)) and this call's flags (0 or LPX_BDUAL_LONG_STEP);
 *   5. extracts x, value, the record, the basis, at_upper, y and d exactly as lpx_solve_packed_dual does; in the record
 *      dualize_flips = 0 and events counts this scenario's loop only.
 * status[i]: LPX_OPTIMAL, LPX_INFEASIBLE, LPX_ITER_LIMIT (the limit is tested first, as in the loop) or LPX_EINVAL.  The results do
 * not depend on count, on i or on the other scenarios.  The handle is only read: several solves may follow one open, and several
 * handles may be open at once.  Per-scenario costs are lpx_packed_base_solve_costs (below); per-scenario bounds are not offered.
 * st (or NULL) as in lpx_solve_packed_dual.
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_packed_base_solve: ": a NULL h, b or out;
 * a NULL status, x or value; count outside [1, 65536]; an unknown flag; resident = 1; more than 1 GiB of input plus output bytes.
 * No device: LPX_EDEVICE.
 *
 * lpx_packed_base_close(h) frees the device allocation and the handle; NULL is allowed.  Returns 0. */
typedef struct lpx_packed_base lpx_packed_base;            /* opaque */
typedef struct lpx_packed_base_model {
    int32_t m, n, sense;
    const double *c, *A, *b;           /* [n], [m][n] row-major, [m]: b is the base right-hand side */
    const double *lower, *upper;       /* [n] or NULL (0 / +inf) */
    const int32_t* rel;                /* [m] of LPX_LE / LPX_GE, or NULL = every row is <= */
} lpx_packed_base_model;
int lpx_packed_base_open(const lpx_packed_base_model* in, int flags, const lpx_run_opts* o /* or NULL */,
                         const lpx_packed_dual_results* base_out /* or NULL: count = 1 */, lpx_packed_base** h);
int lpx_packed_base_solve(const lpx_packed_base* h, int32_t count, const double* b /* [count][m] */, int flags,
                          const lpx_run_opts* o /* or NULL */, const lpx_packed_dual_results* out, lpx_stats* st /* or NULL */);
int lpx_packed_base_close(lpx_packed_base* h);             /* NULL is allowed */

/* ---- packed cost and right-hand-side scenarios from the same solved base (csrc/lpx_packed_cost.hip) ------
 *
 * Costs are the other half of a scenario workload: price sweeps, stochastic programmes, a moving objective, pricing sub-problems.
 * A cost change leaves the RHS column of the base's solved tableau untouched, so the base's basis stays primal feasible; only the
 * objective row moves, by one m x C product, and the bounded PRIMAL loop continues from the base's basis.  A scenario that changes
 * c and b is the two moves in turn: the primal loop runs to the optimum of (c_i, b0), which is dual feasible again, then the
 * slack-block move of lpx_packed_base_solve is applied and the dual loop runs.  The handle remembers the base's c (a host copy
 * made by lpx_packed_base_open).
 *
 * lpx_packed_base_solve_costs(h, count, c, b, flags, o_primal, o_dual, out, st) makes one upload of c0, c ([count][n], the user's
 * costs) and, if given, b ([count][m]; NULL: every scenario keeps b0), ONE launch of count workgroups, one read-back and one wait,
 * on the arena and the stream of lpx_solve_packed.  Every product and every sum below is separately rounded, in the stated order.
 * Workgroup i
 *   1. copies the base's tile and ub into LDS, the basis and the flip bytes into its own slices (step 1 of lpx_packed_base_solve);
 *   2. refuses the scenario if any c_i[j], or any b_i[k] when b is given, is not finite (LPX_EINVAL: its outputs zeroed, a record
 *      of zeros around the status);
 *   3. moves the objective row:
 *          delta_j = c_i[j] - c0[j], negated for a Min model;
 *          g_j = -delta_j if bit 0 of flip[j] is set, else delta_j, for j < n;  g_j = 0 for the slack columns;
 *          K = 0;  for j ascending over the flipped columns with delta_j != 0.0:  prod = delta_j * ub[j];  K = K + prod;
 *          for every column j = 0 .. C-1, the RHS column included:
 *              acc = T[m][j];
 *              for i = 0 .. m-1 ascending with g_basis[i] != 0.0:  prod = g_basis[i] * T[i][j];  acc = acc + prod;
 *              for j < n with g_j != 0.0:  acc = acc - g_j;
 *              for j = C-1:  acc = acc + K;
 *              T[m][j] = acc
 *      and nothing else: an all-zero delta leaves every bit as the base left it.  The shift constant of the user's optimum is
 *      re-summed from c_i: sum of c_i[j] * l_j for j ascending over l_j != 0.0, the statement the base uses;
 *   4. runs the bounded primal loop (steps 1-4 of "bounded-variable primal simplex", the loop of lpx_solve_packed) from the base's
 *      basis and flip bytes with o_primal's eps, ratio_tol and max_iter (NULL: lpx_default_opts(o, 0)).  LPX_UNBOUNDED or
 *      LPX_ITER_LIMIT ends the scenario with that status; the dual loop is then not run;
 *   5. with b only: applies steps 2-3 of lpx_packed_base_solve (the slack-block move) to the tile as the primal loop left it, then
 *      runs the dual loop of lpx_bounded_dual_run3(flags) with o_dual's eps, ratio_tol and max_iter (NULL: lpx_default_opts(o, 1))
 *      and this call's flags (0 or LPX_BDUAL_LONG_STEP); the loop counts its own events from 0 and tests its limit first;
 *   6. extracts x, value, basis, at_upper, y and d exactly as lpx_packed_base_solve does, with the re-summed constant, for every
 *      status but LPX_EINVAL.
 * status[i]: LPX_OPTIMAL, LPX_UNBOUNDED, LPX_INFEASIBLE, LPX_ITER_LIMIT or LPX_EINVAL.  A scenario whose primal phase ends
 * LPX_UNBOUNDED is reported LPX_UNBOUNDED even when its b_i would make it infeasible: the phases run in turn and the first one to
 * fail ends the scenario.  The results do not depend on count, on i or on the other scenarios; the handle is only read.  st (or
 * NULL): pivots = the sum of the four pivot counters of all scenarios, launches = 1, loop_ms the host wall.
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_packed_base_solve_costs: ": a NULL h, c or
 * out; a NULL status, x or value; count outside [1, 65536]; an unknown flag; resident = 1 in either opts; more than 1 GiB of input
 * plus output bytes.  No device: LPX_EDEVICE. */
typedef struct lpx_packed_cost_record {   /* 72 bytes */
    int32_t status;                        /* OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT or LPX_EINVAL */
    int32_t primal_events, dual_events, pad;
    int64_t primal_kind0, primal_kind1, primal_flips;   /* the primal loop: pivots of either kind, bound flips */
    int64_t dual_kind0, dual_kind1, dual_passes;        /* the dual loop (all 0 without b) */
    double  z;                             /* T[m, C-1] as the last loop left it */
} lpx_packed_cost_record;
typedef struct lpx_packed_cost_results {   /* lpx_packed_dual_results with this record; the last five may be NULL */
    int32_t* status; double* x; double* value;
    lpx_packed_cost_record* rec; int32_t* basis; uint8_t* at_upper; double* y; double* d;
} lpx_packed_cost_results;
int lpx_packed_base_solve_costs(const lpx_packed_base* h, int32_t count,
                                const double* c /* [count][n] */, const double* b /* [count][m] or NULL = b0 */,
                                int flags /* 0 or LPX_BDUAL_LONG_STEP: the dual loop */,
                                const lpx_run_opts* o_primal /* or NULL: lpx_default_opts(.,0) */,
                                const lpx_run_opts* o_dual   /* or NULL: lpx_default_opts(.,1) */,
                                const lpx_packed_cost_results* out, lpx_stats* st /* or NULL */);

/* ---- packed batches of small integer programs: a whole branch and bound per workgroup (csrc/lpx_packed_bnb.hip, DESIGN.md
 * section 4.27) ---------------------------------------------------------------------------------------------------------------
 *
 * lpx_solve_packed_bnb(in, opt, out, st) is lpx_solve_packed for integer programs: count models of ONE shape (m rows, every row <=;
 * n variables; is_int, [n] bytes shared by every model, or NULL = every variable is integer) as contiguous arrays with the strides
 * of lpx_solve_packed.  The same arena, the same stream, at most one copy per input array, ONE launch of count workgroups, one
 * read-back and one wait, whatever count and whatever the number of nodes.  Workgroup i
 *   a. builds the tableau of model i in LDS and validates it as lpx_solve_packed does (LPX_EINVAL for a bound, LPX_E_NEG_RHS);
 *      behind the bounds check every integer variable needs a finite upper bound and integral lower and upper bounds, else the
 *      model is LPX_EINVAL; then the root LP runs in the on-chip bounded primal loop with eps, ratio_tol of lpx_default_opts(o, 0)
 *      and the call's max_iter.  A root that does not end LPX_OPTIMAL ends the model with the root's status, x and value as
 *      lpx_solve_packed gives them (stop = LPX_PBNB_ROOT);
 *   b. runs the search of lpx_solve_bnb_bounded3(..., LPX_NODE_ONCHIP) itself, the same steps in the same order, with the tableau
 *      never leaving LDS: the limits, the pop of the depth-first stack, the node's bounds from its path over the root bounds
 *      [0, u'], the columns whose bounds differ from those on the tableau in ascending order, the bound edit, the dual-feasibility
 *      flips, the dual loop with LPX_BDUAL_SKIP_FIXED | search_flags, ratio_tol of lpx_default_opts(o, 1) and, under
 *      LPX_BDUAL_CUTOFF, cutoff = best + 1e-6, the pick (tol 1e-6, nint = n, the mask) and the decide step: LPX_INFEASIBLE prunes;
 *      LPX_CUTOFF or z <= best + 1e-6 prunes by bound; no fractional integer variable is an incumbent (x' as
 *      lpx_tableau_bounded_solution forms it, integer entries rounded half to even, best = z); otherwise the floor child is pushed,
 *      then the ceil child, which is explored first;
 *   c. finishes as lpx_solve_bnb_bounded does: x = the incumbent plus lower when a lower array was given, value = -best for Min,
 *      plus the constant c.lower where a lower bound was non-zero.
 * The fit rule is lpx_packed_fits(m, n) unchanged.  What the search keeps outside LDS (the handle's lower shifts and flip bytes,
 * the bounds, the path, the stack, the incumbent) is a work slice of the arena per model.
 *
 * The three budgets are per model and mandatory: max_nodes and max_events at least 1, max_iter (events per node and of the root
 * loop) at least 0; max_depth is the deepest node a model may hold (0 = n; a binary model never goes deeper than n).
 *
 * status[i]: LPX_OPTIMAL (the stack ran empty with an incumbent), LPX_INFEASIBLE (it ran empty without one), LPX_ITER_LIMIT (a
 * budget stopped the search and rec[i].stop says which; x and value are the incumbent so far, or zeros while incumbents == 0), the
 * root's LPX_UNBOUNDED / LPX_ITER_LIMIT, LPX_EINVAL / LPX_E_NEG_RHS as in lpx_solve_packed (zeros around the status), and LPX_EINVAL
 * with stop = LPX_PBNB_REFUSED for a node edit lpx_bounded_node3 would refuse (the host driver fails with that call's error there).
 * One model's outcome never affects another's.  stop: LPX_PBNB_DONE (the stack ran empty), _ROOT (the model ended at or in front of
 * the root LP), _NODES (max_nodes nodes were evaluated and the stack is not empty), _NODE_ITER (a node made max_iter events), _EVENTS
 * (the nodes evaluated so far made max_events dual events or more; tested where max_nodes is, in front of a pop, behind it),
 * _DEPTH (a node at depth max_depth would branch), _REFUSED.
 *
 * For every i: status, x, value, nodes, events, flips, incumbents, pruned_bound, pruned_infeasible, max_K and the first log_cap log
 * records are bit-equal to lpx_solve_bnb_bounded3(model i, lower_i, upper_i, is_int, max_iter, max_nodes, search_flags,
 * LPX_NODE_ONCHIP) wherever max_events and max_depth do not bind (where that call returns LPX_ITER_LIMIT, its out holds the same
 * incumbent), and do not depend on count, on i, on the other models or on whether an array is shared.  deepest is the largest
 * depth of an evaluated node, root_events the events of the root loop, logged = min(nodes, log_cap), best the internal objective
 * of the incumbent (-inf: none), constant = c.lower over the non-zero lower bounds.  The log slice of a model behind its `logged`
 * records is zero.
 *
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_solve_packed_bnb: ": the list of
 * lpx_solve_packed in its order up to the fit rule; then a NULL opt, a search_flags bit outside LPX_BDUAL_LONG_STEP |
 * LPX_BDUAL_CUTOFF ("unknown flag"), a negative max_iter; then max_nodes or max_events below 1, a negative max_depth or log_cap, log
 * non-NULL with log_cap == 0 or log NULL with log_cap > 0; last, because it needs valid options, more than 1 GiB of inputs, outputs,
 * log and work slices ("too large").  No device: LPX_EDEVICE.  st (or NULL): pivots = the kind-0 and kind-1 pivots of every root
 * and node, launches = 1, loop_ms the host wall of the copies, the launch and the wait. */
#define LPX_PBNB_DONE      0
#define LPX_PBNB_ROOT      1
#define LPX_PBNB_NODES     2
#define LPX_PBNB_NODE_ITER 3
#define LPX_PBNB_EVENTS    4
#define LPX_PBNB_DEPTH     5
#define LPX_PBNB_REFUSED   6
typedef struct lpx_packed_bnb_models {  /* lpx_packed_models plus the mask */
    int32_t count, m, n, sense;        /* one shape for all; every row is <= */
    const double *c, *A, *b;           /* [count][n], [count][m][n] row-major, [count][m] */
    const double *lower, *upper;       /* [count][n] or NULL (0 / +inf) */
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
                                       /* doubles between models: the packed size, or 0 = ONE shared copy */
    const uint8_t* is_int;             /* [n], shared by every model, or NULL = every variable is integer */
} lpx_packed_bnb_models;
typedef struct lpx_packed_bnb_opts {
    int32_t search_flags;              /* subset of LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF */
    int32_t max_iter;                  /* events per node and of the root loop, >= 0 */
    int32_t max_depth;                 /* deepest node a model may hold; 0 = n */
    int32_t log_cap;                   /* log records kept per model, 0 = none */
    int64_t max_nodes, max_events;     /* per model, both >= 1 */
} lpx_packed_bnb_opts;
typedef struct lpx_packed_bnb_record {  /* 88 bytes */
    int32_t status, stop;              /* status[i] again; LPX_PBNB_* */
    int64_t nodes, events, flips, incumbents, pruned_bound, pruned_infeasible;
    int32_t max_K, deepest, root_events, logged;
    double best, constant;             /* internal z of the incumbent (-inf: none); c.lower */
} lpx_packed_bnb_record;
typedef struct lpx_packed_bnb_results { /* caller-allocated; status, x, value required; rec and log may be NULL */
    int32_t* status;  double* x;  double* value;           /* [count], [count][n], [count] */
    lpx_packed_bnb_record* rec;  lpx_bnb_node_log* log;    /* [count], [count][log_cap] */
} lpx_packed_bnb_results;
int lpx_solve_packed_bnb(const lpx_packed_bnb_models* in, const lpx_packed_bnb_opts* opt, const lpx_packed_bnb_results* out,
                         lpx_stats* st /* or NULL */);

/* ---- integer programs with >= rows: branch and bound from a dual start, host-driven and packed (csrc/host/bnb_bounded.cpp,
 * csrc/lpx_packed_bnb_dual.hip) -------------------------------------------------------------------------
 *
 * lpx_solve_bnb_bounded_dual(p, lower, upper, is_int, o, max_nodes, search_flags, node_form, out, info) is lpx_solve_bnb_bounded3
 * with one difference: the root is the dual start of lpx_solve_bounded_dual, not lpx_solve_bounded.  So a >= row is accepted
 * (negated into a <= row), an = row is taken as its pair, and a shifted right-hand side may be negative: covering models, models
 * with rows of both senses and right-hand sides that cross zero.  The root runs the flips of lpx_tableau_dualize(1e-9) and then
 * lpx_bounded_dual_run3 with lpx_default_opts(o, 1), the caller's max_iter and flags = search_flags & LPX_BDUAL_LONG_STEP (no
 * LPX_BDUAL_SKIP_FIXED and no cutoff at the root).  Every integer variable has a finite upper bound, so on a pure integer program
 * the precheck of the dual start always passes; it can only name a continuous variable ("improves the objective and has no upper
 * bound", LPX_EINVAL).
 * Order of refusals: the checks of lpx_solve_bnb_bounded (bounds, then the integer variables, max_nodes, search_flags), then an
 * unknown node_form (LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP or LPX_NODE_AUTO), then the preparation.
 * A root that ends LPX_INFEASIBLE ends the search with the result of a search without an incumbent: status LPX_INFEASIBLE,
 * has_solution 0, value 0, x zeros, summary "INFEASIBLE\n", nodes 0, lp_solves 1; the call returns 0.  A root at the iteration
 * limit fails as lpx_solve_bounded_dual does.  From a solved root on the search, the info, the log and the limits are those of
 * lpx_solve_bnb_bounded3, and LPX_NODE_LAUNCHES and LPX_NODE_ONCHIP give bit-equal node logs.  Unlike a search over <= rows this
 * one can end LPX_INFEASIBLE with nodes > 0. */
int lpx_solve_bnb_bounded_dual(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                               const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o /* or NULL */,
                               int64_t max_nodes /* 0 = none */, int search_flags, int node_form, lpx_result* out,
                               lpx_bnb_bounded_info* info /* or NULL */);

/* lpx_solve_packed_bnb_dual(in, opt, out, st) is lpx_solve_packed_bnb for the models above: the options, record, results, log
 * records and stop codes of lpx_solve_packed_bnb, the rows of lpx_solve_packed_dual (rel: LPX_LE / LPX_GE per row, per model or
 * shared).  The same arena, stream and pinned block, at most one copy per input array, ONE launch of count workgroups, one
 * read-back and one wait.  The fit rule is lpx_packed_fits(m, n).  Workgroup i
 *   a. builds the tableau of model i in LDS as lpx_solve_packed_dual does (Min negates c, a >= row is negated while it is stored,
 *      b' = b - A l, u' = u - l, the slack basis) and checks, in this order, the bounds, the integer variables (a finite upper
 *      bound, integral lower and upper bounds) and rel: LPX_EINVAL.  Then the dual-feasibility flips with eps 1e-9 (a column no
 *      flip can repair is the precheck of lpx_solve_bounded_dual: LPX_EINVAL) and the on-chip dual loop as the root loop, with
 *      ratio_tol of lpx_default_opts(o, 1), the call's max_iter, the long step under LPX_BDUAL_LONG_STEP, no LPX_BDUAL_SKIP_FIXED
 *      and no cutoff.  There is no LPX_E_NEG_RHS and no LPX_UNBOUNDED on this call.  A root that ends LPX_INFEASIBLE ends the
 *      model with x zeros, value 0, nodes 0 and root_events set (the answer of the host driver); a root at LPX_ITER_LIMIT ends it
 *      with x and value as lpx_solve_packed_dual extracts them; both with stop = LPX_PBNB_ROOT;
 *   b. runs the search of lpx_solve_packed_bnb part b, the same steps in the same order;
 *   c. finishes as lpx_solve_packed_bnb does.  status LPX_INFEASIBLE with stop = LPX_PBNB_DONE (the stack ran empty without an
 *      incumbent) can be reached on this call.
 * root_events counts the pivots and passes of the root loop; flips, events and the log count nodes only.
 *
 * For every i: status, x, value, nodes, events, flips, incumbents, pruned_bound, pruned_infeasible, max_K and the first log_cap log
 * records are bit-equal to lpx_solve_bnb_bounded_dual(model i, ..., LPX_NODE_ONCHIP) wherever max_events and max_depth do not
 * bind, and do not depend on count, on i, on the other models or on whether an array is shared.
 *
 * LPX_EINVAL before any device check, the outputs untouched, every message starting "lpx_solve_packed_bnb_dual: ": the list of
 * lpx_solve_packed_bnb in its order up to the fit rule, with rel_stride among the strides (neither 0 nor m); behind the fit rule a
 * shared rel (rel_stride 0) holding anything but LPX_LE / LPX_GE; then the option checks and the 1 GiB rule of
 * lpx_solve_packed_bnb, which here counts rel.  A per-model rel is checked by its workgroup.  No device: LPX_EDEVICE.  st as in
 * lpx_solve_packed_bnb. */
typedef struct lpx_packed_bnb_dual_models {   /* lpx_packed_dual_models plus the mask */
    int32_t count, m, n, sense;        /* one shape for all */
    const double *c, *A, *b;           /* [count][n], [count][m][n] row-major, [count][m] */
    const double *lower, *upper;       /* [count][n] or NULL (0 / +inf) */
    int64_t c_stride, A_stride, b_stride, lower_stride, upper_stride;
                                       /* doubles between models: the packed size, or 0 = ONE shared copy */
    const int32_t* rel;                /* [count][m] of LPX_LE / LPX_GE, or NULL = every row is <= */
    int64_t rel_stride;                /* int32 between models: m, or 0 = ONE shared copy */
    const uint8_t* is_int;             /* [n], shared by every model, or NULL = every variable is integer */
} lpx_packed_bnb_dual_models;
int lpx_solve_packed_bnb_dual(const lpx_packed_bnb_dual_models* in, const lpx_packed_bnb_opts* opt,
                              const lpx_packed_bnb_results* out, lpx_stats* st /* or NULL */);

/* ---- GMI cuts on a handle with bounds, and the cut loop at a bounded root (csrc/lpx_cuts.hip, csrc/lpx_tableau_bounded.cpp,
 * DESIGN.md section 4.23) --------------------------------------------------------------------------------------------------
 * An internal column of a bounded handle stands for x'_j = x_j - lo_j, or for ub_j - (x_j - lo_j) when it is flipped; x'_j >= 0
 * and a nonbasic column sits at 0.  A GMI cut of a row in the internal variables needs no more than that and the integrality of
 * the x'_j it treats as integer, so the arithmetic of lpx_tableau_gmi_round is valid on the internal representation as it stands,
 * and the appended row is an ordinary equality row that every later bound edit, dualize flip and row complement re-expresses
 * like any other.  Cuts derived under the root's bounds hold in the whole tree below it.
 *
 * lpx_tableau_gmi_round_bounded(t, is_int, n_mask, first_cut_col, o, n_added, src_rows, n_purged, purged_cols): the round of
 *   lpx_tableau_gmi_round, bit for bit on the internal representation (candidates, ranking, alphas, dynamism filter, appended
 *   rows, purge rule, new shape, outputs), with these differences:
 *   - Column j is integer iff j < min(n_mask, first_cut_col), is_int[j] != 0, lo[j] == floor(lo[j]) and (ub[j] == +inf or
 *     ub[j] == floor(ub[j])), with lo / ub the handle's (lpx_tableau_bound_state); decided on the device.  A flagged column with
 *     a fractional bound is continuous; a handle without bounds passes every flagged column.  Source rows use the same notion
 *     for their basic column.
 *   - The bounds follow the reshape: surviving columns keep ub, lo and flip in order, every new slack gets ub = +inf, lo = 0,
 *     flip = 0, and the shape the bounds belong to becomes the new C.  Every bounded entry point, lpx_tableau_clone and
 *     lpx_tableau_snapshot / _restore accept the handle afterwards; the contiguous RHS copy the bounded kernels read is rewritten.
 *   - cuts_per_round = 0 is allowed: a purge-only call.
 *   Argument errors as lpx_tableau_gmi_round (cuts_per_round 0..64), plus bounds that were set for another live C
 *   ("the live shape changed since lpx_tableau_set_bounds"): LPX_EINVAL before any device check, the handle untouched.
 *
 * lpx_bounded_cut_loop(t, is_int, n_mask, first_cut_col, nint, node_is_int, co, ro, flags, form, rec): rounds of cuts on a
 *   solved (OPTIMAL) bounded handle with spare capacity.  is_int / n_mask / first_cut_col are the round's; nint / node_is_int
 *   ([nint] or NULL = all) are the pick's (lpx_tableau_branch_pick, tol = co->int_tol).  Each round:
 *     1. the pick of the tableau as it stands (round one: lpx_tableau_branch_pick; later: the pick of the last re-optimisation)
 *        has var < 0 -> stop LPX_CUTLOOP_INTEGRAL;
 *     2. rounds == co->max_rounds -> stop LPX_CUTLOOP_ROUNDS;
 *     3. lpx_tableau_gmi_round_bounded; K == 0 -> stop LPX_CUTLOOP_STALLED (its purges are counted);
 *     4. lpx_bounded_node3 with no bound edit (K = 0), flags | LPX_BDUAL_SKIP_FIXED, cutoff -inf (given only with
 *        LPX_BDUAL_CUTOFF in flags), tol = co->int_tol, in `form` (LPX_NODE_AUTO: decided per round by lpx_bounded_node_fits;
 *        both forms are bit-equal).  LPX_INFEASIBLE -> the integer program is infeasible, stop LPX_CUTLOOP_INFEASIBLE;
 *        LPX_ITER_LIMIT -> stop LPX_CUTLOOP_ITER_LIMIT; any other status but LPX_OPTIMAL -> stop LPX_CUTLOOP_STATUS.
 *   Then, if co->purge is set and the stop is none of INFEASIBLE / ITER_LIMIT / STATUS, one purge-only call (cuts_per_round = 0);
 *   it needs no re-optimisation, a purged row has a basic slack.
 *   rec: rounds = re-optimisations made; added / purged = cuts over all calls; events = events of the re-optimisations;
 *   stop; status = the last re-optimisation's (LPX_OPTIMAL when there was none); R, C = the final live shape; pick = the pick of
 *   the final tableau (z = T[m,Cm] in every case); z_before[i] / z_after[i] (each NULL or [co->max_rounds], the caller's) =
 *   T[m,Cm] in front of and behind round i < rounds.  Returns 0, or LPX_ITER_LIMIT with the record filled.
 *   LPX_EINVAL before any device check, the handle untouched: everything lpx_tableau_gmi_round_bounded and lpx_bounded_node3
 *   refuse (flags outside LPX_BDUAL_LONG_STEP | LPX_BDUAL_CUTOFF | LPX_BDUAL_SKIP_FIXED, unknown form, LPX_NODE_ONCHIP on a
 *   shape that does not fit or whose spare capacity min(Rcap - R, Ccap - C) added to R and C does not, nint outside [0, C-1],
 *   ...), a NULL rec, a handle without bounds. */
#define LPX_CUTLOOP_INTEGRAL   0
#define LPX_CUTLOOP_STALLED    1
#define LPX_CUTLOOP_ROUNDS     2
#define LPX_CUTLOOP_INFEASIBLE 3
#define LPX_CUTLOOP_ITER_LIMIT 4
#define LPX_CUTLOOP_STATUS     5
typedef struct lpx_cut_loop_record {
    int32_t rounds, added, purged, stop;
    int32_t status, R, C, pad;
    int64_t events;
    lpx_branch_pick pick;
    double* z_before;       /* in: NULL or [max_rounds] */
    double* z_after;        /* in: NULL or [max_rounds] */
} lpx_cut_loop_record;
int  lpx_tableau_gmi_round_bounded(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col,
                                   const lpx_cut_opts* o, int* n_added, int32_t* src_rows /* [K] or NULL */,
                                   int* n_purged, int32_t* purged_cols /* [C-1 - first_cut_col] or NULL */);
int  lpx_bounded_cut_loop(lpx_tableau* t, const uint8_t* is_int, int n_mask, int first_cut_col, int nint,
                          const uint8_t* node_is_int /* [nint] or NULL */, const lpx_cut_opts* co, const lpx_run_opts* ro /* or NULL */,
                          int flags, int form, lpx_cut_loop_record* rec);

/* lpx_solve_bnb_bounded9(p, lower, upper, is_int, o, max_nodes, search_flags, divers, stall_events, root_form, root_cuts, out, info,
 *   dinfo, ginfo, cinfo): lpx_solve_bnb_bounded8 with cut-and-branch at the root.  root_cuts = NULL is lpx_solve_bnb_bounded8 bit
 *   for bit (cinfo comes back zeroed).  Otherwise:
 *   - The root handle is made with `a` spare rows and columns, a = the largest value <= root_cuts->max_active for which
 *     (R + a, C + a) still satisfies lpx_bounded_node_fits; the round's free-capacity rule then keeps every later node on chip.
 *     a = 0 runs no round (cinfo->ran = 0, cinfo->spare = 0) and the search is that of lpx_solve_bnb_bounded8.
 *   - The round's flags: the structural is_int as given (NULL = all); the slack of prepared row i is integer iff every
 *     coefficient of the row is integral, its shifted RHS is integral and every variable with a non-zero coefficient in it is
 *     integer; an = row is a pair of rows and gives two slacks, judged alike.  first_cut_col = n_mask = C - 1.
 *   - lpx_bounded_cut_loop(root handle, flags, C-1, C-1, n, is_int, root_cuts, the node options, search_flags, LPX_NODE_AUTO).
 *     It ends LPX_CUTLOOP_INFEASIBLE: the result is LPX_INFEASIBLE with 0 nodes.  LPX_CUTLOOP_ITER_LIMIT: the call returns
 *     LPX_ITER_LIMIT with 0 nodes.  LPX_CUTLOOP_INTEGRAL: the search still runs; its first node is the incumbent.  Otherwise the
 *     search by W divers runs from the final handle: the clones are made after the loop, the root bounds are the model's, and
 *     nothing else of the driver changes (cuts derived under the root's bounds hold in the whole tree).
 *   cinfo (or NULL): ran, spare, the loop's rounds / added / purged / events / stop / status, the shape R x C the search runs on,
 *   and z_before / z_after [n_z = rounds] (T[m,Cm] around every round, internal sense); free with lpx_bnb_cut_info_free.
 *   Root cuts are defined for this driver alone: the sequential driver with node_form = LPX_NODE_LAUNCHES (lpx_solve_bnb_bounded3),
 *   the plunge (lpx_solve_bnb_bounded5) and strong branching (lpx_solve_bnb_bounded6) have no root_cuts.  LPX_EINVAL before any
 *   device check: everything lpx_solve_bnb_bounded8 refuses, and root_cuts outside the ranges of lpx_tableau_gmi_round
 *   (cuts_per_round 1..64). */
typedef struct lpx_bnb_cut_info {
    int32_t ran, spare, rounds, added, purged, stop, status, R, C, n_z;
    int64_t events;
    double* z_before; double* z_after;      /* [n_z] */
} lpx_bnb_cut_info;
int  lpx_solve_bnb_bounded9(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                            const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                            int search_flags, int divers /* W, 1..1024 */, int stall_events, int root_form,
                            const lpx_cut_opts* root_cuts /* or NULL */, lpx_result* out, lpx_bnb_bounded_info* info /* or NULL */,
                            lpx_bnb_divers_info* dinfo /* or NULL */, lpx_bnb_guard_info* ginfo /* or NULL */,
                            lpx_bnb_cut_info* cinfo /* or NULL */);
void lpx_bnb_cut_info_free(lpx_bnb_cut_info* cinfo);

/* ---- reduced-cost tightening: a node that branches shrinks the ranges of its subtree (not in the reference;
 * csrc/lpx_bounded_fix.hip, csrc/lpx_onchip_fix.h, csrc/lpx_node_batch.cpp, csrc/host/bnb_bounded.cpp) --
 * A node that ends LPX_OPTIMAL leaves a dual feasible objective row, and from the first incumbent on a driver has a bound to
 * beat.  The rule works on the handle's internal variables (the search is internally a Max; z = T[m,Cm]) and is driven by one
 * double, fix_bound; -inf turns it off.  It runs only when the node ended LPX_OPTIMAL and z > fix_bound, in the same launch,
 * behind the branch pick (the pick sees the bounds as they were).  For every column j < nint it applies when all of these hold:
 *   - the mask admits j (is_int NULL or is_int[j] != 0);
 *   - j is not basic (the basic columns are marked through the basis; none is inferred from a zero);
 *   - d = T[m,j] satisfies d > eps.
 * With g = (z - fix_bound) / d (one subtract, one IEEE divide) and t = floor(g), column j is tightened iff t < ub[j], and then
 * ub[j] = t.  A column with flip[j] != 0 also gets lo[j] = (lo[j] + ub_old[j]) - t, and the handle's mark that a lower shift is
 * stored is set as a bound edit with the reported triples would set it.  Nothing beside ub and lo changes: a nonbasic column
 * stands at 0, so its range change has a zero RHS shift; the tableau, the RHS, the basis, the flip states and the trace stay.
 * The tightened columns are reported in ascending j, each as the absolute triple (col, lower, upper) in the handle's x' space
 * that a bound edit would take: unflipped (j, lo[j], lo[j] + t); flipped (j, up - t, up) with up = lo[j] + ub_old[j].
 * DEFINING PROPERTY: after the call, ub, lo, flip, the tableau and the basis are bit-equal to those of a twin handle that ran the
 * same node with tightening off and then one more node call carrying exactly the reported triples; that call makes 0 events and
 * 0 flips.  WHY IT IS VALID: in the internal variables z(x') = z - sum d_j x'_j over the nonbasic columns, so a point with
 * x'_j >= t + 1 has an objective <= z - d (t + 1) <= fix_bound, which with fix_bound = best + 1e-6 is the driver's own prune
 * test.  The admitted columns are expected to have finite ranges, as the integer columns of every driver have: on a column
 * with ub = +inf any finite t becomes its upper bound, which is valid and harmless but with a fix_bound far below z is merely
 * a huge number.  Integer columns only (no slack, no continuous column), and local only: the tightening holds for the subtree of the
 * node; nothing is fixed again at the root when an incumbent improves.
 *
 * lpx_bounded_node5(t, K, cols, lower, upper, o, flags, cutoff, stall_events, fix_bound, nint, is_int, tol, form, out, guard, fix):
 * fix_bound = -inf is lpx_bounded_node4 in every form, bit for bit (same kernels), fix->n = 0.  Any other fix_bound needs the
 * on-chip form and runs lpx_bounded_fix_onchip: ONE launch, ONE wait, the same LDS rule (lpx_bounded_node_fits); that kernel
 * carries the stall guard, and with stall_events = 0 its loop is the unguarded one bit for bit.  fix is caller-owned: cap entries
 * in each of cols / lower / upper; n comes back, the first n entries are the triples.  LPX_EINVAL before any device check:
 * fix_bound is NaN ("fix_bound is NaN"); fix with cap < nint ("fix->cap is below nint") or, with nint > 0, a null array; no fix
 * with a fix_bound other than -inf ("null fix"); such a fix_bound with LPX_NODE_LAUNCHES, or with LPX_NODE_AUTO on a shape that
 * does not fit ("reduced-cost tightening has no launches form"); and the argument errors of lpx_bounded_node4 with the new name
 * in front.  guard and, with fix_bound = -inf, fix may be NULL.  A refused edit leaves n = 0.
 *
 * lpx_node_batch_run3(b, B, slot, K, cols, lower, upper, o, flags, cutoff, stall_events, fix_bound, nint, is_int, tol, out, guard,
 * fix, rc): lpx_node_batch_run2's contract word for word, with lpx_bounded_node5(..., stall_events, fix_bound[i], ...,
 * LPX_NODE_ONCHIP, &out[i], &guard[i], &fix[i]) as the single-node equal of entry i and "lpx_node_batch_run3" in front of the
 * messages.  fix_bound [B] is per entry and never NULL; fix [B] may be NULL only when every fix_bound[i] is -inf.  Entries with
 * -inf tighten nothing whatever the others do.  When every entry is -inf the launch is lpx_node_batch_run2's.
 *
 * lpx_solve_bnb_bounded10(p, lower, upper, is_int, o, max_nodes, search_flags, divers, stall_events, root_form, root_cuts, tighten,
 * out, info, dinfo, ginfo, cinfo, finfo): lpx_solve_bnb_bounded9 with the flag tighten (0 or 1, anything else is LPX_EINVAL:
 * "tighten is neither 0 nor 1").  tighten = 0 is lpx_solve_bnb_bounded9 bit for bit.  With tighten = 1 the rounds change in two
 * steps only.  Step 4 is ONE lpx_node_batch_run3 in which every entry's fix_bound is best + 1e-6 as best stood at the start of
 * the round, or -inf while there is no incumbent.  Step 5, for every record with reported triples: they are applied to the bounds
 * the driver holds for that diver's handle (the kernel has applied them to the handle already), and, where the node branches,
 * appended to both children's paths in front of the branching override.  The log stays a function of the model, the options,
 * the flags, W and tighten.  finfo (or NULL): tightened_nodes (nodes that tightened a column), tightened_cols (their sum) and
 * max_per_node; plain counters, no free function.  The default stays off: no speed-up is promised.
 * The plunge, the probes with strong branching and the sequential driver of the launches form have no tightening. */
typedef struct lpx_fix_list {            /* 32 bytes */
    int32_t cap;           /* in: entries the three arrays hold, >= nint */
    int32_t n;             /* out: columns tightened */
    int32_t* cols;         /* out [n]: ascending */
    double* lower;         /* out [n]: the triples a bound edit would take, in the handle's x' space */
    double* upper;
} lpx_fix_list;
typedef struct lpx_bnb_fix_info {        /* 24 bytes */
    int64_t tightened_nodes, tightened_cols, max_per_node;
} lpx_bnb_fix_info;
int  lpx_bounded_node5(lpx_tableau* t, int K, const int32_t* cols, const double* lower, const double* upper, const lpx_run_opts* o,
                       int flags, double cutoff, int stall_events, double fix_bound, int nint,
                       const uint8_t* is_int /* [nint] or NULL = all */, double tol, int form, lpx_node_record* out,
                       lpx_guard_record* guard /* or NULL */, lpx_fix_list* fix /* NULL only with fix_bound = -inf */);
int  lpx_node_batch_run3(lpx_node_batch* b, int B, const int32_t* slot /* [B] */, const int32_t* K /* [B] */,
                         const int32_t* cols, const double* lower, const double* upper /* concatenated, sum of K */,
                         const lpx_run_opts* o, int flags, const double* cutoff /* [B]; read only with LPX_BDUAL_CUTOFF */,
                         int stall_events, const double* fix_bound /* [B] */, int nint,
                         const uint8_t* is_int /* [nint] or NULL = all */, double tol, lpx_node_record* out /* [B] */,
                         lpx_guard_record* guard /* [B] or NULL */, lpx_fix_list* fix /* [B] */, int32_t* rc /* [B] */);
int  lpx_solve_bnb_bounded10(const lpx_problem* p, const double* lower /* [n] or NULL = 0 */, const double* upper /* [n] */,
                             const uint8_t* is_int /* [n] or NULL = all */, const lpx_solve_opts* o, int64_t max_nodes /* 0 = none */,
                             int search_flags, int divers /* W, 1..1024 */, int stall_events, int root_form,
                             const lpx_cut_opts* root_cuts /* or NULL */, int tighten /* 0 or 1 */, lpx_result* out,
                             lpx_bnb_bounded_info* info /* or NULL */, lpx_bnb_divers_info* dinfo /* or NULL */,
                             lpx_bnb_guard_info* ginfo /* or NULL */, lpx_bnb_cut_info* cinfo /* or NULL */,
                             lpx_bnb_fix_info* finfo /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LPX_H */
