// lpx_pivot_fused.hip -- the one-launch primal pivot (K4f) and its deferred pivots: sweep kernels of every depth,
// the select-only kernels (one launch through the workspace; the column and row launches of the pair), the flush and their launchers.  Built with -ffp-contract=off like every tile (lpx_kernels.hip).
// Compact form (the _cm kernels, lpx_compact_*): a long run on a streamed handle sweeps a tableau of the nonbasic
// columns and the RHS only.  A column is then a SLOT; F.slotvar names its variable.  Pivot k (entering slot s, row r): the column
// launch stores +0.0 over the stored column s once its values are in the factor column of the ring slot (the slot holds the leaving
// variable from here on, a unit column); the row launch takes the pivot element from that factor column, counts row r as 1.0 and the
// objective row as +0.0 at s, writes +0.0 into the pending pivot rows at s, and the lane that owns s does the bookkeeping in
// variables (basis, trace, slotvar).  The entering rule compares variables, the partial argmins carry the slot beside them.  A pivot
// selected by a sweep launch is zeroed by the next column launch (or the exit pass).  Sweep bodies are untouched: they see a
// narrower tableau.  Every other run uses the kernels without the flag, whose arithmetic and order are what they were.
#include <algorithm>
#include "lpx_scan.h"
#include "lpx_tile.h"

namespace lpx {

// ------------------------------------------------------------------------------------------------
// Fused pivot (primal loop without a per-pivot callback, any size): update(k) OUT OF PLACE + select(k+1), one launch.
//
// With the update in place, select(k+1) has to wait for update(k): it reads column q', row r' and the objective row of
// T_{k+1}.  All three are rank-1 corrections of the same parts of T_k with data select(k) already produced (the factor
// column and the normalised pivot row of pivot k) -- so if update(k) writes T_{k+1} into a SECOND buffer and leaves T_k
// alone, select(k+1) depends on nothing update(k) produces and runs beside it: the first `nblk` workgroups of this grid are
// lpx_select_mb's workgroups reading T_k through the correction `T_k[i,j] - fac_k[i] * prow_k[j]` (the very mul-then-sub
// the update stores, so every value is bit-identical to what the two-launch path reads back from memory), the others are
// the streaming update's waves.  A pivot then costs the sweep alone (117.7 us at 4097 x 12289 against 117.4 + 10.0);
// tools/kbench/oop.hip measured the shape first: a ping-pong sweep is as fast as the in-place one (115.5 vs 116.0 us),
// 256-lane workgroups cost it 1.6 us, and 32 select-shaped workgroups at the head of the grid another 0.5 us.
// Smaller tableaux gain more (tools/probe_fused_mid.py: 1.03-1.42x from 129 x 385 to 308 MB); cache policy: fused_policy below.
//
// Nothing is read and written inside one launch: everything a launch reads carries the index `c` of the CURRENT state
// record (RHS column) or a ring slot of a pending pivot, or is the source tableau; everything it writes carries 1 - c, its own
// ring slot, or is the destination tableau -- the state records included: a launch reads record `par` and writes record
// 1 - par, and `par` (like the ring slot) is a launch argument (graph batches are multiples of 2d, so a replay starts where the
// capture did).  Which buffer holds the stored tableau is part of the record (pad[3], with the pending count: fp_rec below);
// pad[2] counts launches, for the host to find the last record written.
//   record c:  (r, q) = pivot k, the newest selected but not yet applied    qn = entering column of pivot k+1
//   ring slot of pivot k: T_k[r,:] / T_k[r,q],  T_k[:,q],  r        rhs[c] = T_k[:,C-1]
// P.st is the host's copy of the current record, written by select's first workgroup: one launch behind.
// A terminal status can be found with pivots still pending: the host applies them (lpx_pivot_flush) before the run returns.
// ------------------------------------------------------------------------------------------------
static constexpr int FP_NT = 256;

__global__ __launch_bounds__(SEL_NT) void lpx_fused_init(FusedParams F)
{
    __shared__ double s_v[SEL_NW];
    __shared__ int s_i[SEL_NW];
    const SelParams& P = F.P;
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    ScanRule rule; rule.forced = 0; rule.eps = P.eps; rule.thresh = P.fthresh; rule.C = C; rule.c0 = 0;
    // first entering column (ChooseEntering on the objective row as it stands) and the RHS column of record 0
    int qn = -1;
    if (P.st->status == LPX_RUNNING) qn = la_prepare_from_T(P, R, C, P.col0, R - 1, rule, s_v, s_i);
    if (threadIdx.x == 0) {
        DevState x = *P.st;
        x.qn = qn; x.r = -1; x.q = -1; x.pad[2] = 1; x.pad[3] = 0;
        F.rec[0] = x;
        x.pad[2] = 0;
        F.rec[1] = x;
        P.part_i[MB_CNT] = 0;
    }
}

// Deferred pivots (LPX_PIVOT_DEFER = d, run_fused).  A sweep moves the whole tableau however many pivots it applies, and
// select(k+1) needs only column q, the RHS column, row r and the objective row of T_{k+1} -- each of them the stored tableau
// with the pending pivots applied on the fly.  So launch L of a run (L = 0: the prologue's) is
//   L % d != 0 or L == 0: select-only (nsel workgroups): pivot L from the stored tableau + the n = L % d pending pivots
//   otherwise:            sweep: applies pending pivots L-d .. L-1 out of place (oldest first, the very mul-then-sub of d
//                         single sweeps: every element's value is bit-identical) beside select of pivot L from the source
// Pivot L's normalised row, factor column and row go to ring slot L % 2d (`lm`, a launch argument): a launch reads the slots of
// the n <= d pivots before it and writes its own, never one it reads.  d = 1 is the one-pivot-per-sweep kernel of r02 / r03.
// Record field pad[3] (fp_rec): bit 0 = buffer of the stored tableau, bits 1-5 = pivots pending after the launch, bits 8- =
// ring slot of the oldest -- the host flushes them (lpx_pivot_flush) when the run is over.
// (deepest deferral FP_DMAX: lpx_block.h)
// rows per sweep wave: each pending pivot row a lane loads (from L2) serves ROWS rows of the stream; three rows as in r03 while
// one or two pivots are applied, eight beyond (at three rows the pivot-row reads grew the d = 8 sweep from 118 to 162 us; at
// eight, 140 us).  Twelve and sixteen rows spill 12-96 VGPRs inside the 80 the select half leaves (waves_per_eu(6) below).
// tools/kbench/deferred_sweep.hip (profiles/r14_kbench_deferred_sweep.txt) confirmed those reads as what a pending pivot costs:
// with the pairs out of a register this tile runs 130 us at d = 8, 12 and 16 alike (shipped: 134-138, 144, 156 us).  The pending
// rows staged in LDS once per workgroup (4 rows x 4 waves on one column window) ran 123 / 126 / 132 us there and 128 / 135 /
// 144-147 us in this kernel, 9-12 % under this tile at equal depth -- and 2.6-3.8 % on the headline at d = 16, short of the 5 %
// a change of this loop is held to, so the tile stays (DESIGN.md 4.1 and 9.9 have the numbers and what is left to try).
// Strips (fused_sweep_strip, the streaming kernels of d >= 3): a wave loads its D pairs ONCE and walks FP_STRIP_BLOCKS row blocks
// of fp_rows(D) rows with them in VGPRs; the blocks keep the tile above (loads, D x (mul, sub), stores by policy).  The kbench's
// strip rows (profiles/r15_kbench_deferred_sweep.txt, d = 16): two blocks 132.6 us at 2 waves per SIMD, 136-137 at 3, 140 at 4;
// four blocks 136 / 145 / 146; sixteen 190 at 3 (1.04 rounds of resident waves: the tail) and 149 at 4 -- longer strips buy nothing
// beyond the halved pair traffic.  In this kernel two blocks run 135-137 us at d = 16 and 135 at d = 12 (the tile above: 159-160 and
// 149), the same built for 2 and for 3 waves per SIMD (141-151 VGPRs: three waves either way); for 4 it spills and runs 241 us.
__host__ __device__ constexpr int fp_rows(int D) { return D <= 2 ? UPDS_ROWS : 8; }
__host__ __device__ constexpr int fp_rec(int buf, int npend, int slot0) { return buf | (npend << 1) | (slot0 << 8); }
// ring slot of pending pivot s (0 = oldest) of n before the launch with ring index lm
__device__ __forceinline__ int fp_slot(int lm, int n, int s, int ring) { const int k = lm - n + s; return k < 0 ? k + ring : k; }

#ifdef LPX_STAMPS
// Diagnostic build only: phase stamps of the select-only launches (tools/diag_pivot_select_stamps.py).  Workgroup 0's lane 0 keeps
// the s_memtime deltas in registers and adds them to lpx_g_stamps[8 + slot] when the launch ends (a store per stamp would put
// its own round trip into the next phase).  LPX_FS_W first waits for wave 0's loads, so that a phase which only issues loads
// owns their latency; that serialises phases the shipped kernel overlaps, so the phases' sum exceeds the unstamped duration
// (slot 20 has the launch's own s_memrealtime span).  Slots of the one-launch form (lpx_pivot_select_ws): 0 record load and
// branch, 1 column gather, 2 pending chain, 3 ratio store and barrier, 4 scan, 5 piv chain, 6 row loop, 7 wave and hand-off
// reduction, 8 tail stores, 9 gather trips, 10-12 gather per trip (the third and later trips together), 20 realtime, 21 launches,
// 22 pending pivots summed.  The row launch of the pair (lpx_pivot_select) uses the same range: 0 record, shape and scan records
// (and, in this build, the wait for the operands issued beside them), 4 the replay, 3 the exact scan behind a tie (9 counts those
// steps), 1 issue of the three loads behind r and the objective row's chain, 5 - 8 and 20 - 22 as above; the column
// launch has its own (LPX_FC_*, below).
#define LPX_FS_BEGIN(on) const bool fs_on_ = (on) && blockIdx.x == 0 && threadIdx.x == 0; unsigned long long fs_acc_[13] = {0}; \
    unsigned long long fs_prev_ = __builtin_amdgcn_s_memtime(); const unsigned long long fs_rt0_ = __builtin_amdgcn_s_memrealtime();
#define LPX_FS(slot) do { if (fs_on_) { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); fs_acc_[(slot)] += n_ - fs_prev_; fs_prev_ = n_; } } while (0)
#define LPX_FS_W(slot) do { if (fs_on_) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); } LPX_FS(slot); } while (0)
#define LPX_FS_TRIP(trip) do { if (fs_on_) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    const unsigned long long n_ = __builtin_amdgcn_s_memtime(), d_ = n_ - fs_prev_; fs_prev_ = n_; fs_acc_[1] += d_; fs_acc_[9] += 1; \
    if ((trip) == 0) fs_acc_[10] += d_; else if ((trip) == 1) fs_acc_[11] += d_; else fs_acc_[12] += d_; } } while (0)
#define LPX_FS_TIE() do { if (fs_on_) fs_acc_[9] += 1; } while (0)
#define LPX_FS_END(npend) do { if (fs_on_) { _Pragma("unroll") for (int k_ = 0; k_ < 13; ++k_) lpx_g_stamps[8 + k_] += fs_acc_[k_]; \
    lpx_g_stamps[28] += __builtin_amdgcn_s_memrealtime() - fs_rt0_; lpx_g_stamps[29] += 1; lpx_g_stamps[30] += (unsigned long long)(npend); } } while (0)
#else
#define LPX_FS_BEGIN(on)
#define LPX_FS(slot) do {} while (0)
#define LPX_FS_W(slot) do {} while (0)
#define LPX_FS_TRIP(trip) do {} while (0)
#define LPX_FS_TIE() do {} while (0)
#define LPX_FS_END(npend) do {} while (0)
#endif

// select(k+1): the first nsel workgroups of a sweep launch, the whole of a select-only launch.  `sweeps`: this launch applies
// its n pending pivots too (the stored tableau changes buffer).  U: rows in flight per lane in the column pass (the sweep
// kernels' register budget of waves_per_eu(6) holds U = 4 with two spilled VGPRs, U = 6 spilled 19; the select-only kernel has no such budget).
// Compact form (CM instantiations): columns are slots.  The entering rule compares VARIABLES (F.slotvar), so a
// candidate carries its variable in MinIdx::i and its slot beside it; cm_feed / cm_pick / cm_wave_min are rule_feed / mi_pick /
// wave_min_idx with the slot carried along (variables are unique, so the winner's lane is the one that holds its variable).
__device__ __forceinline__ void cm_feed(MinIdx& m, int& mslot, int j, int var, double u)
{
    if (u < m.v || (u == m.v && m.i != INT_MAX && var < m.i)) { m.v = u; m.i = var; mslot = j; }      // the initial -eps is no candidate
}
__device__ __forceinline__ void cm_pick(MinIdx& a, int& aslot, MinIdx b, int bslot)
{
    if (b.v < a.v || (b.v == a.v && b.i < a.i)) { a = b; aslot = bslot; }
}
__device__ __forceinline__ MinIdx cm_wave_min(MinIdx x, int& slot)
{
    const MinIdx r = wave_min_idx(x);
    const unsigned long long mk = __ballot(x.i == r.i);      // never empty: some lane holds the winner (or every lane INT_MAX and slot -1)
    slot = __builtin_amdgcn_readlane(slot, __ffsll((long long)mk) - 1);
    return r;
}

template <int U, int SU, int NC = 0, bool CM = false>
__device__ __forceinline__ void fused_select(const FusedParams& F, int n_, bool sweeps)
{
    const int n = NC > 0 ? NC : n_;                          // NC: the count known at compile time (d = 1: r03's select)
    __shared__ double s_fs;
    const SelParams& P = F.P;
    const int t = threadIdx.x, b = blockIdx.x;
    const int lm = F.lm, ring = 2 * F.defer;
    // Which record is current comes with the LAUNCH (lm's parity), not from the records: the workgroups of a launch start over
    // its whole duration, and one that started after workgroup 0 had written the next record must not take that for the
    // current one.  (A first form compared sequence numbers on the device; it passed every test because select finishes late
    // and the scalar cache kept serving the old line -- and broke when a second process shared the GPU.)
    const int c = lm & 1;
    LPX_FS_BEGIN(!sweeps)
    const DevState cur = F.rec[c];
    DevState* nxt = F.rec + (c ^ 1);
    const int status = cur.status, seq = cur.pad[2], buf = cur.pad[3] & 1;
    const int nbuf = sweeps ? (buf ^ 1) : buf;               // where the stored tableau lives once this launch is over
    const int nsel = P.nblk;
    if (b == 0 && t == 0) *P.st = cur;                        // the host's copy: one launch behind
    LPX_FS_W(0);
    if (status != LPX_RUNNING) {
        if (b == 0 && t == 0) { DevState x = cur; x.pad[2] = seq + 1; *nxt = x; }
        return;
    }
    const int R = P.shape ? P.shape[0] : P.R, C = P.shape ? P.shape[1] : P.C;
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const double* __restrict__ src = buf ? F.T1 : P.T;
    double* __restrict__ prown = F.pring + (size_t)lm * ld;
    double* __restrict__ facn = F.fring + (size_t)lm * fld;
    const double* __restrict__ rhsc = c ? F.rhs1 : P.rhsbuf;
    double* __restrict__ rhsn = c ? P.rhsbuf : F.rhs1;
    const int m = R - 1;
    const int iter = cur.iter, primal_count = cur.primal_count;
    const int q = cur.qn;
    int final_status = LPX_RUNNING, r = -1;
    // loop head, Models/PrimalSimplex.cs:95-106
    if (primal_count >= P.max_iter) final_status = LPX_ITER_LIMIT;
    else if (q < 0) final_status = LPX_OPTIMAL;
    double fs = 0.0;
    if (final_status == LPX_RUNNING) {
        // T_{k+1}[i,q] and T_{k+1}[i,C-1] as the sweep stores them: the column through every pending pivot (row r_s: the
        // normalised pivot row), the RHS column kept current in rhsc up to the newest pending pivot, which is applied here.
        // The pending pivots' scalars are uniform loads beside the column's (staging them in LDS behind a barrier cost the
        // 25 MB tableau's loop 14 %: two more round trips per pivot)
        const int sn = fp_slot(lm, n, n - 1, ring);
        const int rl = n ? cur.r : -1;                       // the newest pending pivot is the record's
        const double prhs = n ? F.pring[(size_t)sn * ld + (C - 1)] : 0.0;
        double* rat = P.ws + (size_t)b * (size_t)(P.R > P.C ? P.R : P.C);
        for (int i0 = 0; i0 < R; i0 += U * FP_NT) {
            double v[U], h[U], fl[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = min(R - 1, i0 + u * FP_NT + t);    // clamped, not guarded: a guarded load waits for its own branch
                v[u] = src[(size_t)i * ld + q]; h[u] = rhsc[i];
            }
            LPX_FS_TRIP(i0 / (U * FP_NT));
            // oldest first; the newest pivot's factors are kept for the RHS correction
#pragma unroll SU
            for (int s = 0; s < n; ++s) {
                const int sl = fp_slot(lm, n, s, ring);
                const double* __restrict__ fac = F.fring + (size_t)sl * fld;
                const double pq = F.pring[(size_t)sl * ld + q];
                const int rs = s == n - 1 ? rl : F.rring[sl];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = min(R - 1, i0 + u * FP_NT + t);
                    fl[u] = fac[i];
                    const double nv = v[u] - fl[u] * pq;     // mul, then sub: contraction is off
                    v[u] = i == rs ? pq : nv;
                }
            }
            LPX_FS_W(2);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * FP_NT + t;
                if (i < R) {
                    const double dn = v[u];
                    const double nm = n == 0 ? h[u] : (i == rl ? prhs : h[u] - fl[u] * prhs);
                    rat[i] = dn > P.eps ? nm / dn : __builtin_inf();     // ChooseLeaving's ratio, :229-241
                    if (b == 0) { facn[i] = dn; rhsn[i] = nm; }          // factors of pivot k+1, numerators of the test after it
                    if (i == m) s_fs = dn;                               // T_{k+1}[m,q]: row m belongs to exactly one lane
                }
            }
            LPX_FS(3);
        }
        __syncthreads();                                     // the slice of ratios is complete (and visible: same CU)
        LPX_FS(3);
        fs = s_fs;
        r = block_hysteresis_segments<FP_NT / 64>(m, P.tol_primal, CompactRatio{rat});
        LPX_FS(4);
        if (r < 0) final_status = LPX_UNBOUNDED;
    }
    if (final_status != LPX_RUNNING) {
        if (b == 0 && t == 0) {
            DevState x = cur;
            x.status = final_status; x.r = -1; x.q = -1; x.qn = -1; x.pad[2] = seq + 1;
            x.pad[3] = fp_rec(nbuf, sweeps ? 0 : n, fp_slot(lm, n, 0, ring));
            *nxt = x;
        }
        return;
    }

    ScanRule rule; rule.forced = 0; rule.eps = P.eps; rule.thresh = P.fthresh; rule.C = C; rule.c0 = 0;
    const int per = (C + nsel - 1) / nsel;
    const int j0 = b * per, j1 = min(C, j0 + per);
    const double* trow = src + (size_t)r * ld;
    const double* orow = src + (size_t)m * ld;
    auto pslot = [&](int s) { return fp_slot(lm, n, s, ring); };
    auto prs = [&](int s) { return s == n - 1 ? cur.r : F.rring[pslot(s)]; };     // the newest: the record's
    auto pfr = [&](int s) { return F.fring[(size_t)pslot(s) * fld + r]; };
    auto pfm = [&](int s) { return F.fring[(size_t)pslot(s) * fld + m]; };
    double piv = trow[q];                                    // T_{k+1}[r,q], the column's own chain
    for (int s = 0; s < n; ++s) {
        const double pq = F.pring[(size_t)pslot(s) * ld + q];
        const double nv = piv - pfr(s) * pq;
        piv = r == prs(s) ? pq : nv;
    }
    LPX_FS_W(5);
    MinIdx best; rule_init(rule, best);
    int bslot = -1;                                          // CM: the slot of `best`, whose index is a variable
#pragma unroll 2
    for (int j = j0 + t; j < j1; j += FP_NT) {
        double tr = trow[j], ov = orow[j];                   // -> T_{k+1}[r,j], T_{k+1}[m,j] (m is never a pivot row)
#pragma unroll SU
        for (int s = 0; s < n; ++s) {
            const double pc = F.pring[(size_t)pslot(s) * ld + j];
            const double nt = tr - pfr(s) * pc;
            tr = r == prs(s) ? pc : nt;
            ov = ov - pfm(s) * pc;
        }
        if constexpr (CM) {
            // slot q from here on holds the LEAVING variable: a unit column, 1.0 in row r and +0.0 in the objective row.  The lane
            // that owns it does the pivot's bookkeeping in variables: nobody else reads basis[r] or slotvar[q] in this launch
            int var = F.slotvar[j];
            if (j == q) {
                const int lv = P.basis[r];
                tr = 1.0; ov = 0.0;
                P.basis[r] = var;                                // basis[leaving] = entering, :110
                if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = var; }
                F.slotvar[j] = lv; F.qring[lm] = q;
                var = lv;
            }
            const double p = tr / piv;
            prown[j] = p;
            const double u = ov - fs * p;
            if (j < C - 1) cm_feed(best, bslot, j, var, u);
        } else {
        const double p = tr / piv;                               // true division, :250
        prown[j] = p;
        const double u = ov - fs * p;                            // what the sweep of pivot k+1 will store at T[m,j]
        rule_feed(rule, best, j, u);
        }
    }
    LPX_FS_W(6);
    if constexpr (CM) best = cm_wave_min(best, bslot);
    else best = wave_min_idx(best);
    // last-workgroup reduction of the partial argmins: the hand-off of lpx_select_mb (agent-scope stores, wait, barrier, one add)
    if ((t & 63) == 0) {
        const int slot = b * (FP_NT / 64) + (t >> 6);
        __hip_atomic_store(&P.part_v[slot], best.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&P.part_i[slot], best.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (CM) __hip_atomic_store(&F.pslot[slot], bslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t < 64) {
        int last = 0;
        if (t == 0) last = (__hip_atomic_fetch_add(&P.part_i[MB_CNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsel - 1) ? 1 : 0;
        last = __builtin_amdgcn_readfirstlane(last);
        if (last) {
            MinIdx x; x.v = __builtin_inf(); x.i = INT_MAX;
            int xs = -1;
            const int npart = nsel * (FP_NT / 64);               // <= 128
            if (t < npart) {
                x.v = __hip_atomic_load(&P.part_v[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.i = __hip_atomic_load(&P.part_i[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (CM) xs = __hip_atomic_load(&F.pslot[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (t + 64 < npart) {
                MinIdx y;
                y.v = __hip_atomic_load(&P.part_v[t + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                y.i = __hip_atomic_load(&P.part_i[t + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (CM) cm_pick(x, xs, y, __hip_atomic_load(&F.pslot[t + 64], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                else
                x = mi_pick(x, y);
            }
            if constexpr (CM) { x = cm_wave_min(x, xs); if (x.i != INT_MAX) x.i = xs; }     // the record's qn is a slot
            else
            x = wave_min_idx(x);
            if (t == 0) {
                nxt->qn = (x.i == INT_MAX) ? -1 : x.i;           // the one field of the record this workgroup writes
                __hip_atomic_store(&P.part_i[MB_CNT], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    LPX_FS_W(7);
    if (b == 0 && t == 0) {
        if constexpr (!CM) {                                     // CM: the lane that owns slot q has done these, in variables
        P.basis[r] = q;                                          // basis[leaving] = entering, :110
        if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = q; }
        }
        F.rring[lm] = r;
        nxt->status = LPX_RUNNING; nxt->iter = iter + 1; nxt->r = r; nxt->q = q;
        nxt->phase = cur.phase; nxt->fdf_count = cur.fdf_count; nxt->dual_iter = cur.dual_iter;
        nxt->primal_count = primal_count + 1; nxt->forced_k = cur.forced_k; nxt->c0n = 0; nxt->qn_valid = 0;
        nxt->pad[0] = cur.pad[0]; nxt->pad[1] = cur.pad[1]; nxt->pad[2] = seq + 1;
        nxt->pad[3] = sweeps ? fp_rec(nbuf, 1, lm) : fp_rec(nbuf, n + 1, fp_slot(lm, n, 0, ring));
    }
    LPX_FS_W(8);
    LPX_FS_END(n);
}

// The sweep: T_{k+1} = T_{k+1-D} with pending pivots k+1-D .. k applied, out of place, oldest first.  Each lane keeps the
// D pivot-row pairs of its two columns in VGPRs; the factors of a wave's three rows are scalar loads.
// NT: nontemporal loads and (mixmod permitting) stores -- the streaming forms; false: default policy throughout, for a pair of
// buffers that lives in the Infinity Cache together (lpx_pivot_fused_c)
template <bool NT, int D, int ROWS = fp_rows(D)>
__device__ __forceinline__ void fused_sweep(const FusedParams& F, int ncw, int nunits, int mixmod)
{
    const SelParams& P = F.P;
    const int t = threadIdx.x;
    const int lm = F.lm;
    constexpr int ring = 2 * D;
    const DevState& cur = F.rec[lm & 1];
    const int status = cur.status, buf = cur.pad[3] & 1, rnew = cur.r;     // rnew: the newest pending pivot's row
    const int nsel = P.nblk;
    const int R = P.shape ? P.shape[0] : P.R;
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const double* __restrict__ src = buf ? F.T1 : P.T;
    double* __restrict__ dst = buf ? P.T : F.T1;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int unit = ((int)blockIdx.x - nsel) * (FP_NT / 64) + wave;
    if (unit >= nunits) return;
    const int cw = unit % ncw, rb = unit / ncw;
    const int col = cw * 128 + lane * 2;
    if (col >= P.ld) return;
    const int row0 = rb * ROWS;
    if (row0 >= R) return;
    bool hit = false;                                        // a pending pivot row in this wave's rows: the row-wise path
#pragma unroll
    for (int s = 0; s < D; ++s) hit |= (unsigned)((s == D - 1 ? rnew : F.rring[fp_slot(lm, D, s, ring)]) - row0) < (unsigned)ROWS;
    if (status != LPX_RUNNING) return;                       // a run that is over leaves its pending pivots to lpx_pivot_flush
    const double* sb = src + (size_t)row0 * ld + col;
    double* db = dst + (size_t)row0 * ld + col;
    if (row0 + ROWS <= R && !hit) {
        double2 v[ROWS];
        tile_load<ROWS, NT>(v, sb, ld);
#pragma unroll
        for (int s = 0; s < D; ++s) {
            const int sl = fp_slot(lm, D, s, ring);
            const double2 p = *reinterpret_cast<const double2*>(F.pring + (size_t)sl * ld + col);
            tile_pivot<ROWS>(v, p, F.fring + (size_t)sl * fld + row0, 0);
        }
        tile_store<ROWS, NT, NT ? MIX_SWEEP : MIX_NONE>(db, ld, v, rb, mixmod);
        return;
    }
#pragma unroll 1
    for (int k = 0; k < ROWS; ++k) {
        const int i = row0 + k;
        if (i >= R) break;
        double2 o = upd_load<NT>(sb + (size_t)k * ld);
#pragma unroll 1
        for (int s = 0; s < D; ++s) {
            const int sl = fp_slot(lm, D, s, ring);
            const double2 p = *reinterpret_cast<const double2*>(F.pring + (size_t)sl * ld + col);
            const double f = F.fring[(size_t)sl * fld + i];
            double2 u;
            u.x = o.x - f * p.x;
            u.y = o.y - f * p.y;
            o = i == F.rring[sl] ? p : u;                    // row r_s: the normalised pivot row
        }
        upd_store<NT>(db + (size_t)k * ld, o);
    }
}

// The streaming sweep of d >= 3 in strips: unit -> (strip, column window), window fastest; a strip is FP_STRIP_BLOCKS blocks of
// fp_rows(D) rows.  The D pairs and the D pending rows are loaded once per wave; per block: the tableau loads, the factor
// scalars and the stores of the tile above, same operations in the same order (oldest pending pivot first, mul then sub).
//   factors    through the constant address space.  Behind the first block's stores the compiler cannot show that a plain global
//              load is not clobbered inside the kernel and issues it as a vector load behind s_waitcnt vmcnt(0) -- one dependent
//              round trip per pending pivot and block (210-240 us in the kbench).  No launch writes a ring slot it reads (see the
//              head of this file), so the address space says what is true and the loads stay s_load_dwordx16.
//   hit block  a block that holds a pending pivot's row takes a block-uniform branch: the same tile, rolled over the pivots and
//              straight-line over the rows, row r_s taking the pair.  The pair comes from L2 again (a register array cannot be
//              indexed by a loop counter; unrolled, the selects cost 16 VGPRs and 76-116 bytes of scratch on every block): 16
//              dependent round trips for at most D blocks in R / 8, against 8 x D in the row-wise path.  kbench, 16 spread rows,
//              d = 16: the tile above 157 -> 183 us, this form 137.5 -> 139 us.
//   tail       only the block that runs past R keeps the per-row guard (the row-wise loop of fused_sweep).
template <bool NT, int D>
__device__ __forceinline__ void fused_sweep_strip(const FusedParams& F, int ncw, int nunits, int mixmod)
{
    constexpr int ROWS = fp_rows(D), S = FP_STRIP_BLOCKS, ring = 2 * D;
    const SelParams& P = F.P;
    const int t = threadIdx.x;
    const int lm = F.lm;
    const DevState& cur = F.rec[lm & 1];
    const int status = cur.status, buf = cur.pad[3] & 1, rnew = cur.r;     // rnew: the newest pending pivot's row
    const int nsel = P.nblk;
    const int R = P.shape ? P.shape[0] : P.R;
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const double* __restrict__ src = buf ? F.T1 : P.T;
    double* __restrict__ dst = buf ? P.T : F.T1;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int unit = ((int)blockIdx.x - nsel) * (FP_NT / 64) + wave;
    if (unit >= nunits) return;
    const int cw = unit % ncw, strip = unit / ncw;
    const int col = cw * 128 + lane * 2;
    if (col >= P.ld) return;
    const int row0 = strip * (S * ROWS);
    if (row0 >= R) return;
    int rs[D];
#pragma unroll
    for (int s = 0; s < D; ++s) rs[s] = s == D - 1 ? rnew : F.rring[fp_slot(lm, D, s, ring)];
    if (status != LPX_RUNNING) return;                       // a run that is over leaves its pending pivots to lpx_pivot_flush
    double2 p[D];
#pragma unroll
    for (int s = 0; s < D; ++s) p[s] = *reinterpret_cast<const double2*>(F.pring + (size_t)fp_slot(lm, D, s, ring) * ld + col);
    const LPX_CONSTANT double* fc = (const LPX_CONSTANT double*)F.fring;
    const int nfull = min(S, (R - row0) / ROWS);             // full blocks of this strip
    const double* sb = src + (size_t)row0 * ld + col;
    double* db = dst + (size_t)row0 * ld + col;
#pragma unroll 1
    for (int b = 0; b < nfull; ++b) {
        const int r0 = row0 + b * ROWS;
        bool hit = false;                                    // a pending pivot row in this block
#pragma unroll
        for (int s = 0; s < D; ++s) hit |= (unsigned)(rs[s] - r0) < (unsigned)ROWS;
        double2 v[ROWS];
        tile_load<ROWS, NT>(v, sb, ld);
        if (!hit) {
#pragma unroll
            for (int s = 0; s < D; ++s) tile_pivot<ROWS>(v, p[s], fc + (size_t)fp_slot(lm, D, s, ring) * fld + r0, 0);
        } else {
#pragma unroll 1
            for (int s = 0; s < D; ++s) {
                const int sl = fp_slot(lm, D, s, ring);
                const double2 ps = *reinterpret_cast<const double2*>(F.pring + (size_t)sl * ld + col);
                const int r = s == D - 1 ? rnew : F.rring[sl];
                const LPX_CONSTANT double* f = fc + (size_t)sl * fld + r0;
#pragma unroll
                for (int k = 0; k < ROWS; ++k) {
                    double2 u;
                    u.x = v[k].x - f[k] * ps.x;              // mul, then sub: contraction is off
                    u.y = v[k].y - f[k] * ps.y;
                    v[k] = r0 + k == r ? ps : u;             // row r_s: the normalised pivot row
                }
            }
        }
        tile_store<ROWS, NT, NT ? MIX_SWEEP : MIX_NONE>(db, ld, v, strip * S + b, mixmod);
        sb += (size_t)ROWS * ld; db += (size_t)ROWS * ld;
    }
    if (nfull == S) return;
#pragma unroll 1
    for (int i = row0 + nfull * ROWS; i < min(R, row0 + (nfull + 1) * ROWS); ++i) {     // the block that runs past R
        double2 o = upd_load<NT>(src + (size_t)i * ld + col);
#pragma unroll 1
        for (int s = 0; s < D; ++s) {
            const int sl = fp_slot(lm, D, s, ring);
            const double2 ps = *reinterpret_cast<const double2*>(F.pring + (size_t)sl * ld + col);
            const double f = F.fring[(size_t)sl * fld + i];
            double2 u;
            u.x = o.x - f * ps.x;
            u.y = o.y - f * ps.y;
            o = i == F.rring[sl] ? ps : u;                   // row r_s: the normalised pivot row
        }
        upd_store<NT>(dst + (size_t)i * ld + col, o);
    }
}

// waves_per_eu(6): 80 VGPRs.  The sweep half alone needs 28 (D = 1) to 64 (D = 16); the select half sets the budget and spills
// (code-object metadata): 2 VGPRs in lpx_pivot_fused<1, 2>, 2-4 in _c<1..8>, 8-14 in _c<9..16>.  The strip forms (the streaming
// kernels of d >= 3) hold D pairs and a block and are built for three waves per SIMD (fp_strip_wpe): 103 VGPRs at D = 3, 109 at
// 8, 139 at 12, 151 at 16, no scratch -- four waves where they fit, three from D = 12.  The select half needs about 86 and spills
// nothing there.
// -- the defaults run lpx_pivot_fused<16> above 292 MiB (the 403 MB headline), lpx_pivot_fused<12> from 152 MB to there,
// _c<12> (14) from 64 to 152 MB and lpx_pivot_fused_c<4> (2) up to 64 MB (config 2's 25 MB).
// Without the hint the r03 kernel took 86 VGPRs = 5 waves per SIMD (8.46 k pivots/s against 8.57 k at 6).
__host__ __device__ constexpr int fp_strip_wpe(int D) { return D <= 2 ? 6 : 3; }
template <int D>
__global__ __launch_bounds__(FP_NT) __attribute__((amdgpu_waves_per_eu(fp_strip_wpe(D)))) void lpx_pivot_fused(FusedParams F, int ncw, int nunits, int mixmod)
{
    if ((int)blockIdx.x < F.P.nblk) {
        if (D == 1) fused_select<4, 1, 1>(F, 1, true);
        else fused_select<4, 1>(F, F.defer, true);           // == D; a run-time count keeps its loops rolled
    } else if constexpr (D <= 2) fused_sweep<true, D>(F, ncw, nunits, mixmod);
    else fused_sweep_strip<true, D>(F, ncw, nunits, mixmod);
}
// the compact form's sweep launch: the strip sweep as it is (a slot is a column to it), the select half in slots and variables
template <int D>
__global__ __launch_bounds__(FP_NT) __attribute__((amdgpu_waves_per_eu(fp_strip_wpe(D)))) void lpx_pivot_fused_cm(FusedParams F, int ncw, int nunits, int mixmod)
{
    static_assert(D >= 3, "the compact form runs the strip sweeps only");
    if ((int)blockIdx.x < F.P.nblk) fused_select<4, 1, 0, true>(F, F.defer, true);
    else fused_sweep_strip<true, D>(F, ncw, nunits, mixmod);
}
template <int D>
__global__ __launch_bounds__(FP_NT) __attribute__((amdgpu_waves_per_eu(6))) void lpx_pivot_fused_c(FusedParams F, int ncw, int nunits, int mixmod)
{
    if ((int)blockIdx.x < F.P.nblk) {
        if (D == 1) fused_select<4, 1, 1>(F, 1, true);
        else fused_select<4, 1>(F, F.defer, true);
    } else fused_sweep<false, D>(F, ncw, nunits, mixmod);
}
// select-only launch: the L % d pending pivots stay where they are.  This form (ratios through the workgroup's slice of P.ws,
// the column in trips of U x 256 rows) serves tableaux of more than SELP_LDS_ROWS rows and handles of at most SELP_MIN_MB; the pair
// lpx_pivot_ratio + lpx_pivot_select below serves the others.
template <int U, int SU>
__global__ __launch_bounds__(FP_NT) void lpx_pivot_select_ws(FusedParams F)
{
    fused_select<U, SU>(F, F.lm % F.defer, false);
}

// The select-only step shaped for latency: two launches, cut where the work changes shape.  Neither moves any tableau; what they
// cost is the length of their chains of dependent memory round trips.  In one launch (the form before this one) each of the 32
// workgroups pulled all R lines of column q and the factor columns of the pending pivots through its own compute unit, only to
// find the same row r as the 31 others: two thirds of that launch.  Now
//   lpx_pivot_ratio  (column launch)  ceil(Rcap / SELC_ROWS) workgroups, one row per lane: T_{k+1}[i,q] through the n pending
//                    pivots, the RHS correction and the ratio of row i -> facn, rhsn and the handle's ratio buffer (Rcap + 1
//                    doubles; the last one is T_{k+1}[m,q]), and one scan record per workgroup behind it (SelcRec, lpx_block.h)
//   lpx_pivot_select (row launch)     the nsel workgroups of every select: the leaving row from the scan records (the ratios
//                    themselves only behind a tie), row r and the objective row through the pending pivots, one partial argmin
//                    per workgroup -- handed off to the last arriver only where the next step is not this pair -- the next record
// Both all-to-all exchanges of a pivot (column q to every row and r back; the objective row to one argmin) cross a kernel boundary
// anyway, so neither is paid a second time inside a launch: the column launch reduces each 256 rows to what the hysteresis chain
// needs of them, and the entering column of 1 <= n <= d - 2 is reduced from the partials by the next column launch (n >= 2 there).
// The kernel boundary between them publishes the column launch's plain stores; a hand-off inside one launch would need a spin
// wait on workgroups that HIP does not promise to be co-resident.  Same loads of the same values and the same
// arithmetic as fused_select<.., ..>(F, n, false).  Rounds of the column launch:
//   round 1  the record and the live shape, for n >= 2 the partial argmins of the step before as well (leaves: status not
//            running, iteration cap met, no entering column -- the row launch alone decides terminal states and writes the next
//            record, the column launch only patches rec[c].qn for it; workgroups past the live rows)
//   round 2  T[i,q], rhs[i], the factor columns of the n live pending pivots (one instantiation per n) and the pending pivots'
//            scalars (one vector load per wave: lane k holds pq and r of pending pivot k, read back with v_readlane), all in
//            flight together -- the chain then runs in registers
// and of the row launch:
//   round 1  the record, the live shape and the scan records (their address does not depend on the record); r from the records
//            (behind a tie: one more round, the ratio buffer -> LDS (dynamic), and the exact scan).  In flight behind the scan
//            records, from the launch arguments alone: the pending pivot rows of the workgroup's columns (a share of the
//            capacity, not of the live columns) and the pending pivots' rows; behind the record, beside the replay: the objective
//            row, pq and the objective row's factors of the pending pivots
//   round 2  the three loads that need r: the n factors of row r, the pivot element and row r of the workgroup's columns
//   round 3  one partial per workgroup (block_min_idx first: 8 waves x 32 workgroups would overflow the 128 entries), with the
//            hand-off of fused_select for n = 0 and n = d - 1
// (The column launch with its factor columns, RHS column and pending rows issued in round 1 as well, the row clamped by the
// capacity, and its scan record in one exchange was built and measured in r17: it did not lower the pair's time and is not here.)
// The record bookkeeping and the hand-off are copies of fused_select's: shared helpers moved instructions in all 32 sweep
// kernels.  (SELC_*, SELP_*: lpx_block.h, beside the other select kernels' launch constants)

__device__ __forceinline__ double lane_f64(double x, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), k), __builtin_amdgcn_readlane(__double2loint(x), k));
}

#ifdef LPX_STAMPS
// The column launch's stamps, first wave of workgroup 0, lpx_g_stamps[21 ..]: 21 record load and leave tests, 22 round 2 (every
// load waited for), 23 chain and stores, 24 realtime span, 25 launches, 26 pending pivots summed.
#define LPX_FC_BEGIN() const bool fc_on_ = blockIdx.x == 0 && threadIdx.x == 0; unsigned long long fc_acc_[3] = {0}; \
    unsigned long long fc_prev_ = __builtin_amdgcn_s_memtime(); const unsigned long long fc_rt0_ = __builtin_amdgcn_s_memrealtime();
#define LPX_FC_W(slot) do { if (fc_on_) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    const unsigned long long n_ = __builtin_amdgcn_s_memtime(); fc_acc_[(slot)] += n_ - fc_prev_; fc_prev_ = n_; } } while (0)
#define LPX_FC_END(npend) do { if (fc_on_) { _Pragma("unroll") for (int k_ = 0; k_ < 3; ++k_) lpx_g_stamps[21 + k_] += fc_acc_[k_]; \
    lpx_g_stamps[24] += __builtin_amdgcn_s_memrealtime() - fc_rt0_; lpx_g_stamps[25] += 1; lpx_g_stamps[26] += (unsigned long long)(npend); } } while (0)
#else
#define LPX_FC_BEGIN()
#define LPX_FC_W(slot) do {} while (0)
#define LPX_FC_END(npend) do {} while (0)
#endif

// the column launch through N pending pivots (N known at compile time: exactly N factor columns in flight)
template <int N>
__device__ __forceinline__ void pivot_ratio_patch(const FusedParams& F, int c, int q)
{
    if (N >= 2 && blockIdx.x == 0 && threadIdx.x == 0) F.rec[c].qn = q;
}
struct SelcExchange { double v[SELC_ROWS / 64]; int i[SELC_ROWS / 64]; int n[SELC_ROWS / 64]; };      // the waves' shares of the scan record
template <int N, bool CM = false>
__device__ __forceinline__ void pivot_ratio_rows(const FusedParams& F, double* __restrict__ rat, SelcExchange& X)
{
    const SelParams& P = F.P;
    const int t = threadIdx.x;
    const int lm = F.lm, ring = 2 * F.defer, c = lm & 1;     // the current record comes with the launch: see fused_select
    LPX_FC_BEGIN()
    // round 1: the live shape beside the record
    int R = P.R, C = P.C;
    if (P.shape) { R = P.shape[0]; C = P.shape[1]; }
    // N >= 2: the step before this one was a row launch that left without a hand-off (lpx_pivot_select: 1 <= n <= d - 2), so the
    // entering column is still its nsel partial argmins.  Every wave loads them in this round (lane k: partial k, lanes past the
    // last repeat it) and reduces them as the last-arriver did -- the same wave_min_idx, the same q, tie-break included.
    MinIdx part; part.v = 0.0; part.i = 0;
    int pslot = -1;                                          // CM: the partial's slot (its index is a variable)
    if (N >= 2) {
        const int k = min(t & 63, P.nblk - 1);
        part.v = P.part_v[k]; part.i = P.part_i[k];
        if constexpr (CM) pslot = F.pslot[k];
    }
    const DevState cur = F.rec[c];
    // the partials' loads stay in this round: left alone, they sink behind the leave tests.  The record and the shape are named so
    // that their loads come first and keep their scalar form
    if (N >= 2) asm volatile("" :: "s"(cur.status), "s"(cur.primal_count), "s"(cur.r), "s"(cur.pad[3]), "s"(R), "s"(C) : "memory");
    const int status = cur.status, primal_count = cur.primal_count, rnew = cur.r, buf = cur.pad[3] & 1;
    int q = cur.qn;
    if (status != LPX_RUNNING || primal_count >= P.max_iter) return;     // the row launch writes the record of a run that is over
    if (N >= 2) {
        if constexpr (CM) { part = cm_wave_min(part, pslot); q = part.i == INT_MAX ? -1 : pslot; }
        else {
        part = wave_min_idx(part);
        q = part.i == INT_MAX ? -1 : part.i;
        }
    }
    // N >= 2: the record gets its entering column from workgroup 0 (pivot_ratio_patch), for the row launch of this step to read
    // behind the kernel boundary; nothing in this launch reads the field, every wave has its own q.  The store comes last, or
    // every load behind it would lose its scalar form
    if (q < 0) { pivot_ratio_patch<N>(F, c, q); return; }    // optimal: the row launch says so
    if ((int)blockIdx.x * SELC_ROWS >= R) return;            // the grid follows the capacity
    LPX_FC_W(0);
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const double* __restrict__ src = buf ? F.T1 : P.T;
    double* __restrict__ facn = F.fring + (size_t)lm * fld;
    const double* __restrict__ rhsc = c ? F.rhs1 : P.rhsbuf;
    double* __restrict__ rhsn = c ? P.rhsbuf : F.rhs1;
    const int m = R - 1;
    const int i = blockIdx.x * SELC_ROWS + t;
    const int ic = min(i, m);                                // clamped, not guarded: a guarded load waits for its own branch
    // round 2: the column, the RHS column, the N factor columns and, last (the wave waits for them in issue order, so the chain's
    // first v_readlane waits for the whole round), the pending pivots' scalars: lane k of every wave holds pq and r of pending
    // pivot k (0 = oldest; lanes past the newest repeat it)
    // CM: the stored column is read and then zeroed by this very lane (a slot that holds a basic variable is +0.0 throughout, the
    // objective row included), so the pointer it goes through is not the restrict-qualified one
    double* srcw = buf ? F.T1 : P.T;
    double v0 = CM ? srcw[(size_t)ic * ld + q] : src[(size_t)ic * ld + q];
    const double h = rhsc[ic];
    double f[N > 0 ? N : 1], pqv = 0.0, prhs = 0.0;
    int rsv = -1;
    if (N > 0) {
#pragma unroll
        for (int s = 0; s < N; ++s) f[s] = F.fring[(size_t)fp_slot(lm, N, s, ring) * fld + ic];
        prhs = F.pring[(size_t)fp_slot(lm, N, N - 1, ring) * ld + (C - 1)];
        const size_t kslot = (size_t)fp_slot(lm, N, min(t & 63, N - 1), ring);
        pqv = F.pring[kslot * ld + q];
        rsv = F.rring[kslot];
    }
    LPX_FC_W(1);
    // T_{k+1}[i,q] and T_{k+1}[i,C-1] as the sweep stores them: the column through every pending pivot, oldest first (row r_s: the
    // normalised pivot row), the RHS column kept current in rhsc up to the newest pending pivot, which is applied here
    if constexpr (CM && N == 1) {
        // the pending pivot may be one that a sweep launch selected: its select half could not zero the slot's column while the
        // sweep's waves were writing it.  It is zeroed here (again, harmlessly, behind the prologue), and read as zero
        if (q == cur.q) v0 = 0.0;
        if (i < R) srcw[(size_t)i * ld + cur.q] = 0.0;
    }
    double v = v0;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        const double pq = lane_f64(pqv, s);
        const int rs = s == N - 1 ? rnew : __builtin_amdgcn_readlane(rsv, s);     // the newest: the record's
        const double nv = v - f[s] * pq;                     // mul, then sub: contraction is off
        v = ic == rs ? pq : nv;
    }
    const double dn = v;
    const double nm = N == 0 ? h : (ic == rnew ? prhs : h - f[N > 0 ? N - 1 : 0] * prhs);
    double ratio = dn > P.eps ? nm / dn : __builtin_inf();   // ChooseLeaving's ratio, :229-241
    // every lane computes (the clamped ones their copy of row m); only the stores are guarded.  The empty asm keeps it so: with
    // the arithmetic sunk into the guarded block, the loads go with it and the v_readlane above, which cannot, waits for its own
    // round first
    asm volatile("" : "+v"(ratio));
    if (i < R) {
        rat[i] = ratio;
        facn[i] = dn; rhsn[i] = nm;                          // factors of pivot k+1, numerators of the test after it
        if constexpr (CM) srcw[(size_t)i * ld + q] = 0.0;    // its values live on in facn: the slot now holds the leaving variable
        if (i == m) rat[P.R] = dn;                           // T_{k+1}[m,q]: row m belongs to exactly one lane
    }
    // The workgroup's scan record (SelcRec, lpx_block.h) over its live constraint rows i < m, with the expressions of
    // block_hysteresis_segments: the minimum and its first row (wave_min_idx, then mi_pick over the waves), then the rows inside
    // the band [v, v + tol].  Two exchanges among the waves through X; the row launch replays the chain over the records.
    constexpr int NW = SELC_ROWS / 64;
    const int wave = t >> 6;
    MinIdx lmin; lmin.v = i < m ? ratio : __builtin_inf(); lmin.i = i;
    const double rt = lmin.v;
    lmin = wave_min_idx(lmin);
    if ((t & 63) == 0) { X.v[wave] = lmin.v; X.i[wave] = lmin.i; }
    __syncthreads();
    lmin.v = X.v[0]; lmin.i = X.i[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { MinIdx y; y.v = X.v[w]; y.i = X.i[w]; lmin = mi_pick(lmin, y); }
    const int inband = __popcll(__ballot(i < m && (rt - P.tol_primal) <= lmin.v));
    if ((t & 63) == 0) X.n[wave] = inband;
    __syncthreads();
    if (t == 0) {
        int alone = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) alone += X.n[w];
        SelcRec rec; rec.v = lmin.v; rec.i = alone == 1 ? lmin.i : -1; rec.pad = 0;
        reinterpret_cast<SelcRec*>(rat + selc_rec_offset(P.R))[blockIdx.x] = rec;
    }
    pivot_ratio_patch<N>(F, c, q);
    LPX_FC_W(2);
    LPX_FC_END(N);
}

template <bool CM>
__device__ __forceinline__ void pivot_ratio_switch(const FusedParams& F, double* __restrict__ rat, SelcExchange& X)
{
    switch (F.lm % F.defer) {
    case 0: pivot_ratio_rows<0, CM>(F, rat, X); break;
    case 1: pivot_ratio_rows<1, CM>(F, rat, X); break;
    case 2: pivot_ratio_rows<2, CM>(F, rat, X); break;
    case 3: pivot_ratio_rows<3, CM>(F, rat, X); break;
    case 4: pivot_ratio_rows<4, CM>(F, rat, X); break;
    case 5: pivot_ratio_rows<5, CM>(F, rat, X); break;
    case 6: pivot_ratio_rows<6, CM>(F, rat, X); break;
    case 7: pivot_ratio_rows<7, CM>(F, rat, X); break;
    case 8: pivot_ratio_rows<8, CM>(F, rat, X); break;
    case 9: pivot_ratio_rows<9, CM>(F, rat, X); break;
    case 10: pivot_ratio_rows<10, CM>(F, rat, X); break;
    case 11: pivot_ratio_rows<11, CM>(F, rat, X); break;
    case 12: pivot_ratio_rows<12, CM>(F, rat, X); break;
    case 13: pivot_ratio_rows<13, CM>(F, rat, X); break;
    case 14: pivot_ratio_rows<14, CM>(F, rat, X); break;
    default: pivot_ratio_rows<SELP_PMAX, CM>(F, rat, X); break;
    }
}
// the compact form's column launch
__global__ __launch_bounds__(SELC_ROWS) void lpx_pivot_ratio_cm(FusedParams F, double* __restrict__ rat)
{
    __shared__ SelcExchange X;
    pivot_ratio_switch<true>(F, rat, X);
}

__global__ __launch_bounds__(SELC_ROWS) void lpx_pivot_ratio(FusedParams F, double* __restrict__ rat)
{
    __shared__ SelcExchange X;
    switch (F.lm % F.defer) {                                // pending pivots: the launch's own argument, no load
    case 0: pivot_ratio_rows<0>(F, rat, X); break;
    case 1: pivot_ratio_rows<1>(F, rat, X); break;
    case 2: pivot_ratio_rows<2>(F, rat, X); break;
    case 3: pivot_ratio_rows<3>(F, rat, X); break;
    case 4: pivot_ratio_rows<4>(F, rat, X); break;
    case 5: pivot_ratio_rows<5>(F, rat, X); break;
    case 6: pivot_ratio_rows<6>(F, rat, X); break;
    case 7: pivot_ratio_rows<7>(F, rat, X); break;
    case 8: pivot_ratio_rows<8>(F, rat, X); break;
    case 9: pivot_ratio_rows<9>(F, rat, X); break;
    case 10: pivot_ratio_rows<10>(F, rat, X); break;
    case 11: pivot_ratio_rows<11>(F, rat, X); break;
    case 12: pivot_ratio_rows<12>(F, rat, X); break;
    case 13: pivot_ratio_rows<13>(F, rat, X); break;
    case 14: pivot_ratio_rows<14>(F, rat, X); break;
    default: pivot_ratio_rows<SELP_PMAX>(F, rat, X); break;
    }
}
static_assert(SELP_PMAX == 15, "lpx_pivot_ratio: one case per pending count");

template <bool CM>
__device__ __forceinline__ void pivot_select_body(const FusedParams& F, const double* __restrict__ rat, const SelcRec* recs)
{
    extern __shared__ double sp_rat[];                       // the ratios of the test, one per row of the handle
    __shared__ double s_v[SELP_NT / 64];
    __shared__ int s_i[SELP_NT / 64];
    __shared__ int s_s[SELP_NT / 64];                        // CM: the slots of the waves' candidates
    const SelParams& P = F.P;
    const int t = threadIdx.x, b = blockIdx.x, lane = t & 63;
    const int lm = F.lm, ring = 2 * F.defer;
    const int n = lm % F.defer;
    const int c = lm & 1;                                    // the current record comes with the launch: see fused_select
    LPX_FS_BEGIN(true)
    // round 1: the column launch's scan records, the live shape and the record together.  The records' address follows the capacity
    // (a launch argument), so no load waits for another: lane k of every wave holds record k (lanes past the last repeat it)
    // (`recs` is the ratio buffer's tail, rat + selc_rec_offset(P.R), as an argument of its own: a load through the restrict-qualified
    // `rat` may pass the asm below and is sunk to its first use, behind the row operands' loads -- the replay then waits for all of them)
    const SelcRec srec = recs[min(lane, selc_recs(P.R) - 1)];
    const double fs = rat[P.R];                              // T_{k+1}[m,q]
    int R = P.R, C = P.C;
    if (P.shape) { R = P.shape[0]; C = P.shape[1]; }
    const DevState cur = F.rec[c];
    DevState* nxt = F.rec + (c ^ 1);
    // Still round 1, behind the scan records (vmcnt counts in issue order: the replay's wait leaves these in flight): what follows
    // from the launch arguments alone.  The pending pivot rows at this lane's first column, in groups of SELP_SB, and the pending
    // pivots' rows (lane k of every wave: pending pivot k, 0 = oldest; lanes past the newest repeat it; n = 0, the prologue's
    // launch, names the slot before its own and uses nothing of it).  The live shape arrives in this same round, so a workgroup's
    // columns follow the capacity: rows of the ring are ld doubles, the loads are in bounds, and a lane past the live columns
    // feeds and stores nothing (below).
    const int nsel = P.nblk;
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const int per = (P.C + nsel - 1) / nsel;
    const int j0 = b * per, j1c = min(P.C, j0 + per);
    const int jc0 = min(j0 + t, P.C - 1);
    const size_t kslot = (size_t)fp_slot(lm, n, min(lane, n - 1), ring);
    auto pslot = [&](int s) { return (size_t)fp_slot(lm, n, min(s, n - 1), ring); };
    asm volatile("" ::: "memory");                           // the scan records' load stays in front
    double pc0[SELP_PMAX];                                   // pending pivot rows at this lane's first column
#pragma unroll
    for (int k = 0; k < SELP_SB; ++k) pc0[k] = F.pring[pslot(k) * ld + jc0];
#pragma unroll
    for (int k = SELP_SB; k < SELP_PMAX; ++k) pc0[k] = 0.0;
    if (n > SELP_SB) {
#pragma unroll
        for (int k = SELP_SB; k < SELP_PMAX; ++k) pc0[k] = F.pring[pslot(k) * ld + jc0];
    }
    const int rsv = F.rring[kslot];                          // pending pivot `ks`: its row as the ring has it
    int var0 = 0;                                            // CM: the variable in this lane's first slot
    if constexpr (CM) var0 = F.slotvar[jc0];
    // the record's loads stay here, in flight beside the scan records' (which the clobber holds in place): left alone, the compiler sinks them
    asm volatile("" :: "s"(cur.status), "s"(cur.qn), "s"(cur.pad[3]), "s"(R) : "memory");
    const int status = cur.status, seq = cur.pad[2], buf = cur.pad[3] & 1;
    if (b == 0 && t == 0) *P.st = cur;                        // the host's copy: one launch behind
    LPX_FS_W(0);
    if (status != LPX_RUNNING) {
        if (b == 0 && t == 0) { DevState x = cur; x.pad[2] = seq + 1; *nxt = x; }
        return;
    }
    const double* __restrict__ src = buf ? F.T1 : P.T;
    double* __restrict__ prown = F.pring + (size_t)lm * ld;
    const int m = R - 1;
    const int iter = cur.iter, primal_count = cur.primal_count;
    const int q = cur.qn;
    int final_status = LPX_RUNNING, r = -1;
    // loop head, Models/PrimalSimplex.cs:95-106
    if (primal_count >= P.max_iter) final_status = LPX_ITER_LIMIT;
    else if (q < 0) final_status = LPX_OPTIMAL;
    auto prs = [&](int s) { return s == n - 1 ? cur.r : __builtin_amdgcn_readlane(rsv, s); };     // the newest: the record's
    const double* __restrict__ orow = src + (size_t)m * ld;
    const int j1 = min(j1c, C);                              // the live columns of this workgroup's share of the capacity
    double pqv = 0.0, pfmv = 0.0;                            // T_s[r_s,q] / pivot and T_s[m,q_s] of pending pivot `ks`
    double ov0 = 0.0;                                        // objective row at this lane's first column
    if (final_status == LPX_RUNNING) {
        // behind the record, beside the replay: what needs the record (buffer, q) or the live m, but not r
        ov0 = orow[jc0];
        if constexpr (!CM) pqv = F.pring[kslot * ld + q];
        pfmv = F.fring[kslot * fld + m];
        asm volatile("" ::: "memory");
        // The leaving row: the hysteresis chain of block_hysteresis_segments replayed over the S records of the live rows (S
        // follows the live m; records past it are stale and take no part).  Every lane of every workgroup holds the same
        // records, so a segment that would be entered through a tie sends all of them to the exact scan together.
        // First the same short cut as wave_hysteresis_argmin's, one level up: if the least record is alone in its band among the
        // records too, and its row alone inside its segment, the chain ends on that row whatever it accepted on the way (every
        // earlier best is a ratio r with fl(r - tol) above the minimum; nothing behind can be lower by tol) -- a wave reduction
        // and a ballot instead of a loop of S dependent branches (1.6 us over the headline's 16 records).
        const int S = selc_recs(m);
        double best = __builtin_inf();
        int tie = -1;
        MinIdx g; g.v = lane < S ? srec.v : __builtin_inf(); g.i = lane;
        const double myv = g.v;
        g = wave_min_idx(g);
        const int gi = __builtin_amdgcn_readlane(srec.i, g.i);
        if (g.v < __builtin_inf() && __popcll(__ballot((myv - P.tol_primal) <= g.v)) == 1 && gi >= 0) r = gi;
        else {
            for (int sgi = 0; sgi < S; ++sgi) {
                const double v = lane_f64(srec.v, sgi);
                if (!(v < best - P.tol_primal)) continue;    // nothing in this segment beats the carried best
                const int i = __builtin_amdgcn_readlane(srec.i, sgi);
                if (i < 0) { tie = sgi; break; }
                best = v; r = i;
            }
        }
        LPX_FS(4);
        if (tie >= 0) {
            // ties: the ratios into LDS and the exact scan from that segment on, best and position carried (any start is valid
            // there).  The passes follow the capacity: SELP_RU x SELP_NT rows each, the headline's 4097 in one
            for (int i0 = 0; i0 < P.R; i0 += SELP_RU * SELP_NT) {
                double x[SELP_RU];
#pragma unroll
                for (int u = 0; u < SELP_RU; ++u) x[u] = rat[min(P.R, i0 + u * SELP_NT + t)];
#pragma unroll
                for (int u = 0; u < SELP_RU; ++u) {
                    const int i = i0 + u * SELP_NT + t;
                    if (i < P.R) sp_rat[i] = x[u];
                }
            }
            __syncthreads();                                 // the ratios are in LDS
            LPX_FS_TIE();
            r = wave_hysteresis_argmin(m, P.tol_primal, CompactRatio{sp_rat}, tie * SELC_ROWS, best, r);
            LPX_FS(3);
        }
        if (r < 0) final_status = LPX_UNBOUNDED;
    }
    if (final_status != LPX_RUNNING) {
        if (b == 0 && t == 0) {
            DevState x = cur;
            x.status = final_status; x.r = -1; x.q = -1; x.qn = -1; x.pad[2] = seq + 1;
            x.pad[3] = fp_rec(buf, n, fp_slot(lm, n, 0, ring));
            *nxt = x;
            // CM: the column launch has zeroed slot q for a pivot that is not taken; the exit pass puts it back from ring slot lm
            if constexpr (CM) { if (final_status == LPX_UNBOUNDED) { F.caux[0] = q; F.caux[1] = lm; } }
        }
        return;
    }

    ScanRule rule; rule.forced = 0; rule.eps = P.eps; rule.thresh = P.fthresh; rule.C = C; rule.c0 = 0;
    const double* __restrict__ trow = src + (size_t)r * ld;
    // round 2, the three loads that need r: row r's factors (lane k: pending pivot k), the pivot element T_{k+1}[r,q] -- the
    // column's own chain waits for those -- and row r at this lane's first column.  Everything else is in flight since round 1.
    const double pfrv = F.fring[kslot * fld + r];
    // CM: the column launch has zeroed the stored slot q; the pivot element and its chain are that launch's facn[r], the same bits
    double piv = CM ? F.fring[(size_t)lm * fld + r] : trow[q];
    const double tr0 = trow[jc0];
    int lv = 0;                                              // CM: the leaving variable (used by the lane that owns slot q)
    if constexpr (CM) lv = P.basis[r];
    LPX_FS(1);
    // while those three are in flight: the objective row through the pending pivots, which needs none of them (the same
    // mul-then-sub, oldest first, that the row loop applies to a later pass's columns)
    double ov1 = ov0;
#pragma unroll
    for (int k = 0; k < SELP_PMAX; ++k) {
        if (k < n) ov1 = ov1 - lane_f64(pfmv, k) * pc0[k];
    }
    asm volatile("" : "+v"(ov1));                            // in front of the chain's wait, not behind it
    if constexpr (!CM) {
    for (int s = 0; s < n; ++s) {
        const double pq = lane_f64(pqv, s);
        const double nv = piv - lane_f64(pfrv, s) * pq;
        piv = r == prs(s) ? pq : nv;
    }
    }
    LPX_FS_W(5);
    MinIdx best; rule_init(rule, best);
    int bslot = -1;                                          // CM: the slot of `best`, whose index is a variable
    for (int jb = j0; jb < j1; jb += SELP_NT) {
        const int j = jb + t, jc = min(j, C - 1);
        int var = var0;
        if constexpr (CM) { if (jb != j0) var = F.slotvar[jc]; }
        double tr = tr0, ov = ov1, pc[SELP_PMAX];
#pragma unroll
        for (int k = 0; k < SELP_PMAX; ++k) pc[k] = pc0[k];
        if (jb != j0) {                                      // more columns than lanes: the later ones are loaded here
            tr = trow[jc]; ov = orow[jc];
            if (n > 0) {
#pragma unroll
                for (int k = 0; k < SELP_SB; ++k) pc[k] = F.pring[pslot(k) * ld + jc];
            }
            if (n > SELP_SB) {
#pragma unroll
                for (int k = SELP_SB; k < SELP_PMAX; ++k) pc[k] = F.pring[pslot(k) * ld + jc];
            }
#pragma unroll
            for (int k = 0; k < SELP_PMAX; ++k) {
                if (k < n) ov = ov - lane_f64(pfmv, k) * pc[k];
            }
        }
        // -> T_{k+1}[r,j]; T_{k+1}[m,j] is `ov` already (m is never a pivot row)
#pragma unroll
        for (int k = 0; k < SELP_PMAX; ++k) {
            if (k < n) {
                const double nt = tr - lane_f64(pfrv, k) * pc[k];
                tr = r == prs(k) ? pc[k] : nt;
            }
        }
        if constexpr (CM) {
            if (j < j1) {
                // slot q from here on holds the LEAVING variable: a unit column, 1.0 in row r and +0.0 in the objective row, and +0.0
                // in every pending pivot's row (written here: the one store into a ring slot this launch also reads -- by this lane
                // alone, above).  The lane that owns the slot does the pivot's bookkeeping in variables: nobody else
                // uses basis[r] or slotvar[q] in this launch
                if (j == q) {
                    tr = 1.0; ov = 0.0;
                    P.basis[r] = var;                            // basis[leaving] = entering, :110
                    if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = var; }
                    F.slotvar[j] = lv; F.qring[lm] = q;
                    for (int k = 0; k < n; ++k) F.pring[pslot(k) * ld + j] = 0.0;
                    var = lv;
                }
                const double p = tr / piv;
                prown[j] = p;
                const double u = ov - fs * p;
                if (j < C - 1) cm_feed(best, bslot, j, var, u);
            }
        } else
        if (j < j1) {
            const double p = tr / piv;                           // true division, :250
            prown[j] = p;
            const double u = ov - fs * p;                        // what the sweep of pivot k+1 will store at T[m,j]
            rule_feed(rule, best, j, u);
        }
    }
    LPX_FS_W(6);
    // one partial per workgroup, then the last-workgroup reduction of fused_select (agent-scope stores, wait, one add) -- where
    // the next step's consumer expects nxt->qn: the sweep's fused_select (n = d - 1) or, behind the prologue (n = 0), a column
    // launch with one pivot pending.  With 1 <= n <= d - 2 the next step is the pair again, its column launch reduces the partials
    // itself (pivot_ratio_rows, N >= 2) and the kernel boundary publishes them: no wait, no counter, no last arriver.  (The switch
    // is uniform and follows the launch arguments; part_i[MB_CNT] is left at zero.)
    // The block's argmin with one barrier: s_v / s_i have no other user in this kernel (the exact scan behind a tie works on
    // sp_rat), so nothing has to be protected in front of the stores, and the eight waves' entries take three steps of the scan
    static_assert(SELP_NT / 64 == 8, "lanes8_min_idx: one entry per wave");
    if constexpr (CM) {
        best = cm_wave_min(best, bslot);
        if (lane == 0) { s_v[t >> 6] = best.v; s_i[t >> 6] = best.i; s_s[t >> 6] = bslot; }
        __syncthreads();
        best.v = s_v[lane & 7]; best.i = s_i[lane & 7]; bslot = s_s[lane & 7];
        best = cm_wave_min(best, bslot);                     // every entry eight times over: the minimum of the eight
    } else {
    best = wave_min_idx(best);
    if (lane == 0) { s_v[t >> 6] = best.v; s_i[t >> 6] = best.i; }
    __syncthreads();
    best.v = s_v[lane & 7]; best.i = s_i[lane & 7];
    best = lanes8_min_idx(best);
    }
    if (n >= 1 && n <= F.defer - 2) {
        if (t == 0) { P.part_v[b] = best.v; P.part_i[b] = best.i; if constexpr (CM) F.pslot[b] = bslot; }
    } else if (t < 64) {
        if (t == 0) {
            __hip_atomic_store(&P.part_v[b], best.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&P.part_i[b], best.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (CM) __hip_atomic_store(&F.pslot[b], bslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int last = 0;
        if (t == 0) last = (__hip_atomic_fetch_add(&P.part_i[MB_CNT], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsel - 1) ? 1 : 0;
        last = __builtin_amdgcn_readfirstlane(last);
        if (last) {
            MinIdx x; x.v = __builtin_inf(); x.i = INT_MAX;
            int xs = -1;
            if (t < nsel) {                                      // nsel <= MB_MAXB = 64 partials
                x.v = __hip_atomic_load(&P.part_v[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                x.i = __hip_atomic_load(&P.part_i[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if constexpr (CM) xs = __hip_atomic_load(&F.pslot[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if constexpr (CM) { x = cm_wave_min(x, xs); if (x.i != INT_MAX) x.i = xs; }     // the record's qn is a slot
            else
            x = wave_min_idx(x);
            if (t == 0) {
                nxt->qn = (x.i == INT_MAX) ? -1 : x.i;           // the one field of the record this workgroup writes
                __hip_atomic_store(&P.part_i[MB_CNT], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    LPX_FS_W(7);
    if (b == 0 && t == 0) {
        if constexpr (!CM) {                                     // CM: the lane that owns slot q has done these, in variables
        P.basis[r] = q;                                          // basis[leaving] = entering, :110
        if (iter < P.trace_cap) { P.trace[2 * iter] = r; P.trace[2 * iter + 1] = q; }
        }
        F.rring[lm] = r;
        nxt->status = LPX_RUNNING; nxt->iter = iter + 1; nxt->r = r; nxt->q = q;
        nxt->phase = cur.phase; nxt->fdf_count = cur.fdf_count; nxt->dual_iter = cur.dual_iter;
        nxt->primal_count = primal_count + 1; nxt->forced_k = cur.forced_k; nxt->c0n = 0; nxt->qn_valid = 0;
        nxt->pad[0] = cur.pad[0]; nxt->pad[1] = cur.pad[1]; nxt->pad[2] = seq + 1;
        nxt->pad[3] = fp_rec(buf, n + 1, fp_slot(lm, n, 0, ring));
    }
    LPX_FS_W(8);
    LPX_FS_END(n);
}
__global__ __launch_bounds__(SELP_NT) void lpx_pivot_select(FusedParams F, const double* __restrict__ rat, const SelcRec* recs)
{
    pivot_select_body<false>(F, rat, recs);
}
// the compact form's row launch
__global__ __launch_bounds__(SELP_NT) void lpx_pivot_select_cm(FusedParams F, const double* __restrict__ rat, const SelcRec* recs)
{
    pivot_select_body<true>(F, rat, recs);
}

// End of a run: the n pivots still pending (record: buffer, count, oldest slot) applied to the stored tableau, written to
// buffer 0 (in place when it is already there: every element is read and written by one lane).
__global__ __launch_bounds__(256) void lpx_pivot_flush(FusedParams F, int buf, int n, int slot0)
{
    const SelParams& P = F.P;
    const int R = P.shape ? P.shape[0] : P.R;
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (i >= R || j >= P.ld) return;
    const size_t ld = (size_t)P.ld, fld = (size_t)P.R;
    const int ring = 2 * F.defer;
    const double* src = buf ? F.T1 : P.T;
    double v = src[(size_t)i * ld + j];
    for (int s = 0; s < n; ++s) {
        const int sl = slot0 + s < ring ? slot0 + s : slot0 + s - ring;
        const double pc = F.pring[(size_t)sl * ld + j];
        const double nv = v - F.fring[(size_t)sl * fld + i] * pc;
        v = i == F.rring[sl] ? pc : nv;
    }
    P.T[(size_t)i * ld + j] = v;
}

// ------------------------------------------------------------------------------------------------
// Compact form: the entry and exit passes of a run.  Variables v < C - 1, slots in the order of the variables.
// ------------------------------------------------------------------------------------------------
static constexpr int CE_NT = 1024;
// one workgroup: vmap[v] = slot of a nonbasic variable, -2 - row of a basic one; slotvar; the compact shape; flag on a bad basis
__global__ __launch_bounds__(CE_NT) void lpx_compact_map(CompactIo io, int32_t* cshape, int32_t* caux)
{
    __shared__ int s_cnt[CE_NT];
    const int t = threadIdx.x, nv = io.C - 1, m = io.R - 1;
    for (int v = t; v < nv; v += CE_NT) io.vmap[v] = 0;
    if (t == 0) { cshape[0] = io.R; cshape[1] = io.C - io.R + 1; caux[0] = -1; caux[1] = 0; }
    __syncthreads();
    for (int k = t; k < m; k += CE_NT) {
        const int v = io.basis[k];
        if (v < 0 || v >= nv || atomicCAS(&io.vmap[v], 0, -2 - k) != 0) *io.flag = 1;    // out of range, or named twice
    }
    __syncthreads();
    const int per = (nv + CE_NT - 1) / CE_NT, v0 = min(nv, t * per), v1 = min(nv, v0 + per);
    int cnt = 0;
    for (int v = v0; v < v1; ++v) cnt += io.vmap[v] == 0;
    s_cnt[t] = cnt;
    __syncthreads();
    if (t == 0) { int run = 0; for (int k = 0; k < CE_NT; ++k) { const int c = s_cnt[k]; s_cnt[k] = run; run += c; } }
    __syncthreads();
    int slot = s_cnt[t];
    for (int v = v0; v < v1; ++v) {
        if (io.vmap[v] == 0) { io.vmap[v] = slot; io.slotvar[slot] = v; ++slot; }
    }
    if (t == 0) { io.vmap[nv] = io.C - io.R; io.slotvar[io.C - io.R] = nv; }              // the RHS: the last slot
}
// vmap from slotvar and basis as a run left them (the exit pass's gather)
__global__ __launch_bounds__(256) void lpx_compact_unmap(CompactIo io)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= io.C - io.R) io.vmap[io.slotvar[k]] = k;
    if (k < io.R - 1) io.vmap[io.basis[k]] = -2 - k;
}
// one lane per element of the full tableau: a nonbasic column goes to its slot, a basic one is checked -- bit for bit 1.0 in its
// row and +0.0 elsewhere, the objective row included; anything else (a -0.0, a value one ulp off) raises the flag and the run
// takes the full path.  The lane of the RHS column also clears the padding behind the last slot.
__global__ __launch_bounds__(256) void lpx_compact_gather(CompactIo io)
{
    const int i = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (i >= io.R || v >= io.C) return;
    const double x = io.full[(size_t)i * io.ld + v];
    const int mp = io.vmap[v];
    if (mp >= 0) {
        io.comp[(size_t)i * io.cld + mp] = x;
        if (v == io.C - 1) for (int j = mp + 1; j < io.cld; ++j) io.comp[(size_t)i * io.cld + j] = 0.0;
    } else {
        const double want = i == -2 - mp ? 1.0 : 0.0;
        if (__double_as_longlong(x) != __double_as_longlong(want)) *io.flag = 1;
    }
}
// End of a compact run: lpx_pivot_flush in slots (the n pending pivots applied, oldest first), scattered into the full layout with
// the basic columns written as unit vectors and the padding as zero.  Two columns take their stored values from elsewhere: with
// one pivot pending, its slot reads as zero (a sweep launch may have selected it: see the column launch); the slot zeroed for a
// pivot that was not taken (UNBOUNDED, caux) comes back from that step's factor column, which is the column through all n.
__global__ __launch_bounds__(256) void lpx_compact_exit(FusedParams F, CompactIo io, const double* src, int n, int slot0)
{
    const int i = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (i >= io.R || v >= io.ld) return;
    double x = 0.0;
    if (v < io.C) {
        const int mp = io.vmap[v];
        if (mp < 0) x = i == -2 - mp ? 1.0 : 0.0;
        else if (mp == F.caux[0]) x = F.fring[(size_t)F.caux[1] * F.P.R + i];
        else {
            const size_t cld = (size_t)io.cld, fld = (size_t)F.P.R;
            const int ring = 2 * F.defer;
            x = (n == 1 && mp == F.qring[slot0]) ? 0.0 : src[(size_t)i * cld + mp];
            for (int s = 0; s < n; ++s) {
                const int sl = slot0 + s < ring ? slot0 + s : slot0 + s - ring;
                const double pc = F.pring[(size_t)sl * cld + mp];
                const double nx = x - F.fring[(size_t)sl * fld + i] * pc;
                x = i == F.rring[sl] ? pc : nx;
            }
        }
    }
    io.full[(size_t)i * io.ld + v] = x;
}

// Cache policy of the fused launch.  Two buffers share the Infinity Cache, so the default policy only pays while BOTH fit with
// room to spare; beyond that the streaming mix wins at every size, well below the in-place kernels' own crossover
// (tools/probe_fused_mid.py, us per pivot, two-launch in place / fused default policy / fused streaming mix):
//    57 MB 24.1 / 21.4 / 22.8     101 MB 37.8 / 30.5 / 34.3     157 MB 53.5 / 49.2 / 49.1     190 MB 64.5 / 65.5 / 58.3
//   227 MB 73.1 / 77.2 / 69.0     266 MB 86.1 / 91.1 / 80.3     308 MB 102.7 / 92.4 / 92.2    403 MB 128.3 / 120.0 / 120.2
int fused_policy(int ld, int R) { return policy_for(tableau_bytes(ld, R), FUSED_CACHED_BYTES); }

hipError_t launch_fused_init(const FusedParams& f, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_fused_init, dim3(1), dim3(SEL_NT), 0, s, f);
    return hipGetLastError();
}

using FusedKernel = void (*)(FusedParams, int, int, int);
template <int... Ds> struct FusedTable {
    static constexpr FusedKernel nt[] = { lpx_pivot_fused<Ds>... };
    static constexpr FusedKernel c[] = { lpx_pivot_fused_c<Ds>... };
};
using FusedKernels = FusedTable<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>;
static_assert(sizeof(FusedKernels::nt) / sizeof(FusedKernel) == FP_DMAX, "one sweep kernel per depth");

int pivot_defer_max() { return FP_DMAX; }

static hipError_t launch_pivot_select_ws(const FusedParams& f, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    return launch_k(lpx_pivot_select_ws<6, 4>, dim3(f.P.nblk), dim3(FP_NT), 0, s, e0, e1, f);
}

// The select-only step of handles above SELP_MIN_MB with at most SELP_LDS_ROWS rows: the column launch, then the row launch.  An
// event pair brackets both (e0 in front of the first, e1 behind the second).
static hipError_t launch_pivot_select_pair(const FusedParams& f, double* rat, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    const dim3 gc((f.P.R + SELC_ROWS - 1) / SELC_ROWS), gr(f.P.nblk);        // the column grid follows the capacity
    const size_t lds = sizeof(double) * (size_t)f.P.R;
    const SelcRec* recs = reinterpret_cast<const SelcRec*>(rat + selc_rec_offset(f.P.R));
    if (f.compact) {
        if (e0 && e1) {
            hipExtLaunchKernelGGL(lpx_pivot_ratio_cm, gc, dim3(SELC_ROWS), 0, s, e0, nullptr, 0, f, rat);
            hipExtLaunchKernelGGL(lpx_pivot_select_cm, gr, dim3(SELP_NT), lds, s, nullptr, e1, 0, f, (const double*)rat, recs);
        } else {
            hipLaunchKernelGGL(lpx_pivot_ratio_cm, gc, dim3(SELC_ROWS), 0, s, f, rat);
            hipLaunchKernelGGL(lpx_pivot_select_cm, gr, dim3(SELP_NT), lds, s, f, (const double*)rat, recs);
        }
    } else if (e0 && e1) {
        hipExtLaunchKernelGGL(lpx_pivot_ratio, gc, dim3(SELC_ROWS), 0, s, e0, nullptr, 0, f, rat);
        hipExtLaunchKernelGGL(lpx_pivot_select, gr, dim3(SELP_NT), lds, s, nullptr, e1, 0, f, (const double*)rat, recs);
    } else {
        hipLaunchKernelGGL(lpx_pivot_ratio, gc, dim3(SELC_ROWS), 0, s, f, rat);
        hipLaunchKernelGGL(lpx_pivot_select, gr, dim3(SELP_NT), lds, s, f, (const double*)rat, recs);
    }
    return hipGetLastError();
}

size_t pivot_stream_bytes() { return UPD_STREAM_BYTES; }
size_t pivot_ratio_bytes(int R) { return selc_ratio_bytes(R); }
bool pivot_select_is_pair(int ld, int R) { return R <= SELP_LDS_ROWS && tableau_bytes(ld, R) > ((size_t)SELP_MIN_MB << 20); }

// The compact form's sweep kernels: the depths of the defaults and one small one; a run of another depth keeps the full layout.
static FusedKernel compact_kernel(int d)
{
    switch (d) {
    case 3: return lpx_pivot_fused_cm<3>;
    case 4: return lpx_pivot_fused_cm<4>;
    case 8: return lpx_pivot_fused_cm<8>;
    case 12: return lpx_pivot_fused_cm<12>;
    case 16: return lpx_pivot_fused_cm<16>;
    default: return nullptr;
    }
}
// a run of depth d on this handle (leading dimension, capacity rows) can take the compact form: the select-only pair and a strip sweep
bool pivot_compact_ok(int ld, int R, int d)
{
    return pivot_select_is_pair(ld, R) && fused_policy(ld, R) != 0 && d >= 3 && compact_kernel(d) != nullptr;
}

hipError_t launch_pivot_fused(const FusedParams& f0, double* rat, long long L, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    FusedParams f = f0;
    const int d = f.defer;
    if (d < 1 || d > FP_DMAX) return hipErrorInvalidValue;
    f.lm = (int)(L % (2 * d)); f.par = f.lm & 1;
    const bool sweep = L > 0 && L % d == 0;
    // the compact form: the handle's own leading dimension decides what runs (the pair, the policy, the store mix -- what the handle
    // ran before), the compact one only the sweep's geometry
    const int ld = f.compact ? f.ld_full : f.P.ld, R = f.P.R;
    if (!sweep) {
        // The pair (ratios through the handle's ratio buffer into LDS) while the handle's rows fit the cap, the one-launch form
        // through the workspace beyond it -- and at small sizes: the pair's predecessor (one launch, ratios in LDS, SELP_SB factor
        // columns fetched whatever n is) ran the 403 MB headline 5 % faster than the workspace form and config 2's 25 MB streaming
        // loop (d = 4, 1 to 3 pivots pending, 1025 rows) 22 % slower (82.4 k -> 64.0 k pivots/s).  64 MB is not a measured
        // crossover: nothing between 25 and 403 MB was run, so the switch sits where the depth default changes
        // (PIVOT_DEFER_LARGE_BYTES, lpx_tableau.cpp) and up to 64 MB a handle runs exactly what it ran before.  Whether the pair,
        // which fetches only the n live factor columns and costs a kernel boundary, would serve the small handles too was not run.
        if (pivot_select_is_pair(ld, R)) return rat ? launch_pivot_select_pair(f, rat, s, e0, e1) : hipErrorInvalidValue;
        return launch_pivot_select_ws(f, s, e0, e1);
    }
    const int rows = fp_rows(d);
    const int pol = fused_policy(ld, R);
    const int strip = (pol != 0 && d >= 3) ? FP_STRIP_BLOCKS : 1;           // the streaming kernels of d >= 3: a wave per strip of blocks
    const int ncw = (f.P.ld + 127) / 128, nunits = ncw * (((R + rows - 1) / rows + strip - 1) / strip);
    const int nblocks = f.P.nblk + (nunits + (FP_NT / 64) - 1) / (FP_NT / 64);
    int mixmod = pol == 2 ? mixmod_for(tableau_bytes(ld, R)) : 0;            // 0: every store nontemporal
    // the stored-through row is the last of every mixmod-th block: at `rows` per block the block period shrinks in proportion so
    // that about the same share of BLOCKS keeps a row in the cache.  mixmod = 1 (the 403 MB headline) stays 1: one row in eight
    // instead of one in three goes through the cache at eight rows per block -- the sweep's PMC traffic stays 1.029x of
    // 16 R C; the other share was not measured
    if (mixmod > 1) mixmod = std::max(1, mixmod * UPDS_ROWS / rows);
    if (f.compact && !pivot_compact_ok(ld, R, d)) return hipErrorInvalidValue;
    const FusedKernel kern = f.compact ? compact_kernel(d) : pol == 0 ? FusedKernels::c[d - 1] : FusedKernels::nt[d - 1];   // both buffers in the Infinity Cache: default policy
    return launch_k(kern, dim3(nblocks), dim3(FP_NT), 0, s, e0, e1, f, ncw, nunits, mixmod);
}

hipError_t launch_pivot_flush(const FusedParams& f, int buf, int n, int slot0, hipStream_t s)
{
    const int R = f.P.R, ld = f.P.ld;
    hipLaunchKernelGGL(lpx_pivot_flush, dim3((ld + 255) / 256, R), dim3(256), 0, s, f, buf, n, slot0);
    return hipGetLastError();
}

hipError_t launch_compact_entry(const CompactIo& io, int32_t* cshape, int32_t* caux, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_compact_map, dim3(1), dim3(CE_NT), 0, s, io, cshape, caux);
    hipLaunchKernelGGL(lpx_compact_gather, dim3((io.C + 255) / 256, io.R), dim3(256), 0, s, io);
    return hipGetLastError();
}

hipError_t launch_compact_exit(const FusedParams& f, const CompactIo& io, const double* src, int n, int slot0, hipStream_t s)
{
    hipLaunchKernelGGL(lpx_compact_unmap, dim3((std::max(io.R, io.C - io.R + 1) + 255) / 256), dim3(256), 0, s, io);
    hipLaunchKernelGGL(lpx_compact_exit, dim3((io.ld + 255) / 256, io.R), dim3(256), 0, s, f, io, src, n, slot0);
    return hipGetLastError();
}

// once per process (ensure_device): the dynamic LDS lpx_pivot_select (the row launch) may ask for
hipError_t pivot_fused_init()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_pivot_select), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * SELP_LDS_ROWS);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(lpx_pivot_select_cm), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * SELP_LDS_ROWS);
}
#ifdef LPX_STAMPS
hipError_t pivot_fused_stamps(unsigned long long* acc, int clear) { return stamps_take(acc, clear); }
#endif

}  // namespace lpx
