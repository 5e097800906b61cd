// lpx_bounded_node_body.h -- the body of the on-chip node (lpx_bounded_node.hip), included as the text of BOTH of its kernels:
// lpx_bounded_node_onchip (one node, the record a kernel argument) and lpx_bounded_nodes_onchip (the batch, workgroup b takes
// P[b]).  Not a header in the usual sense: it is a sequence of statements that expects `const NodeParams N` (or `NodeParams N`)
// in scope and may `return` from the kernel.  There is one text of the arithmetic, and each kernel is compiled as if the text
// stood in it.  Why not a __device__ function: with the body behind a call -- forced inline; the record by reference, by value
// or as scalar arguments -- the register allocation of lpx_bounded_node_onchip changes (218 instead of 130 SGPR reloads from VGPR
// lanes in its code, the same 95 VGPRs) and the on-chip driver on binary_ip(60, 12) measured 2.5-5.8 % slower than its parent;
// as included text the kernel keeps the parent's allocation.
    extern __shared__ double nd_lds[];
    __shared__ double s_v[ND_NW];
    __shared__ int s_i[ND_NW];
    __shared__ int s_out;
    __shared__ int s_tot[ND_NW];
    __shared__ int s_bad[ND_NW];
    __shared__ int s_infk;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();

    // ---- 1. the node's inputs (pinned host memory, read once)
    const NodeIn* in = N.in;
    const int K = in->K, flags = in->flags, nint = in->nint, max_iter = in->max_iter;
    const double eps = in->eps, rtol = in->ratio_tol, cutoff = in->cutoff, ptol = in->tol;
    const bool skip_fixed = flags & LPX_BDUAL_SKIP_FIXED, long_step = flags & LPX_BDUAL_LONG_STEP, cut = flags & LPX_BDUAL_CUTOFF;
    const double* in_lower = reinterpret_cast<const double*>(in + 1);
    const double* in_upper = in_lower + K;
    const int32_t* in_cols = reinterpret_cast<const int32_t*>(in_upper + K);

    double* tile = nd_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;
    int* list = reinterpret_cast<int*>(buf);

    // the edit staged on the device, in the layout of the other entry points: lower, upper, shift [K] each, save [2K], cols [K]
    double* e_shift = N.edit + 2 * (size_t)K;
    double* e_save = e_shift + K;
    int32_t* e_cols = reinterpret_cast<int32_t*>(e_save + 2 * (size_t)K);

    // ---- 2. the tableau still untouched: +inf on a flipped column, the shifts, the new ub / lo, the count of the flips
    if (t == 0) s_infk = INT_MAX;
    for (int j = t; j < Cm; j += ND_NT) ub_s[j] = N.ub[j];
    __syncthreads();
    for (int k = t; k < K; k += ND_NT)
        if (in_upper[k] == inf && N.flip[in_cols[k]]) atomicMin(&s_infk, k);
    __syncthreads();
    if (s_infk != INT_MAX) { nd_refuse(N, t, 0, 0, s_infk); return; }
    for (int k = t; k < K; k += ND_NT) {                // the columns are distinct (checked on the host)
        const int j = in_cols[k];
        const double lw = in_lower[k], up = in_upper[k];
        const double uj = ub_s[j], lj = N.lo[j];
        e_save[2 * k] = uj; e_save[2 * k + 1] = lj;
        const double l1 = lw - lj;
        const double u1 = up - lj;                      // +inf stays +inf
        e_shift[k] = N.flip[j] ? uj - u1 : l1;
        e_cols[k] = j;
        const double nu = up - lw;
        N.ub[j] = nu; ub_s[j] = nu;
        N.lo[j] = lw;
    }
    __syncthreads();
    int nflips = 0;
    {
        const double* zrow = N.T + (size_t)m * ld;      // left of the RHS: the shift of the edit does not write it
        int n = 0, bad = 0;
        for (int base = 0; base < Cm; base += ND_NT) {  // uniform trip count
            const int j = base + t;
            bool in_l = false, un = false;
            if (j < Cm) {
                const bool neg = zrow[j] < -eps;
                const double u = ub_s[j];
                in_l = neg && u > 0.0 && u < inf;
                un = neg && u == inf;
            }
            n += __popcll(__ballot(in_l)); bad += __popcll(__ballot(un));
        }
        __syncthreads();
        if (lane == 0) { s_tot[wave] = n; s_bad[wave] = bad; }
        __syncthreads();
        n = 0; bad = 0;
        for (int w = 0; w < ND_NW; ++w) { n += s_tot[w]; bad += s_bad[w]; }
        if (bad > 0) {                                  // refused: ub and lo as they were, nothing else has been written
            for (int k = t; k < K; k += ND_NT) { const int j = in_cols[k]; N.ub[j] = e_save[2 * k]; N.lo[j] = e_save[2 * k + 1]; }
            nd_refuse(N, t, 0, bad, -1);
            return;
        }
        nflips = n;
    }

    // ---- 3. the live window into LDS: a wave per row, lanes along it
    for (int i = wave; i < R; i += ND_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    // ---- 4. the RHS shifts of the edit, k in order: a lane per row
    bool dirty = false;                                 // uniform: the tile differs from the tableau in global memory
    if (K > 0) {
        for (int i = t; i < R; i += ND_NT) {
            double* row = tile + (size_t)i * S;
            double b = row[Cm];
            for (int k = 0; k < K; ++k) {
                const double s = e_shift[k];
                if (s == 0.0) continue;
                const double prod = s * row[e_cols[k]];
                b = b - prod;
            }
            row[Cm] = b;
        }
        dirty = true;
        __syncthreads();
    }

    // ---- 5. the dual-feasibility flips, j ascending: the ordered list (a ballot per wave, a prefix over the wave totals), then
    //         a lane per row walks it -- BOUND FLIP arithmetic, objective row included
    if (nflips > 0) {
        const double* zrow = tile + (size_t)m * S;
        int n = 0;
        for (int base = 0; base < Cm; base += ND_NT) {
            const int j = base + t;
            bool in_l = false;
            if (j < Cm) { const double u = ub_s[j]; in_l = zrow[j] < -eps && u > 0.0 && u < inf; }
            const unsigned long long mi = __ballot(in_l);
            const int before = __popcll(mi & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) s_tot[wave] = __popcll(mi);
            __syncthreads();
            int pre = 0, tot = 0;
            for (int w = 0; w < ND_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
            if (in_l) list[n + pre + before] = j;       // n + pre + before < columns tested so far <= Cm
            n += tot;
        }
        __syncthreads();
        for (int k = t; k < n; k += ND_NT) N.flip[list[k]] ^= 1;
        for (int i = t; i < R; i += ND_NT) {
            double* row = tile + (size_t)i * S;
            double b = row[Cm];
            for (int k = 0; k < n; ++k) {
                const int j = list[k];
                const double a = row[j];
                const double prod = ub_s[j] * a;
                b = b - prod;
                row[j] = -a;
            }
            row[Cm] = b;
        }
        dirty = true;
        __syncthreads();
    }

    // ---- 6. the dual loop: every trip ends the loop or makes at least one event
    int iter = 0, k0 = 0, k1 = 0, status = LPX_ITER_LIMIT;
    double* ratios = buf;
    double* pcol = buf;
    double* zrow = tile + (size_t)m * S;
    for (int trip = 0; trip <= max_iter; ++trip) {
        if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
        if (cut && zrow[Cm] <= cutoff) { status = LPX_CUTOFF; break; }

        // leaving row: first strict minimum of the infeasibilities below -eps
        MinIdx mn; mn.v = -eps; mn.i = INT_MAX;
        for (int i = t; i < m; i += ND_NT) {
            const double b = tile[(size_t)i * S + Cm];
            const int pb = N.basis[i];
            const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
            double w = inf;
            if (b < -eps) w = b;
            else if (u < inf) w = u - b;
            if (w < mn.v) { mn.v = w; mn.i = i; }
        }
        mn = block_min_idx<ND_NT>(mn, s_v, s_i);
        if (mn.i == INT_MAX) { status = LPX_OPTIMAL; break; }
        const int r = mn.i;
        double* trow = tile + (size_t)r * S;
        const int kind = trow[Cm] < -eps ? 0 : 1;
        const int p = N.basis[r];

        // kind 1: the complement of row r in place, in front of the ratios
        if (kind) {
            const double up = ub_s[p];
            __syncthreads();                            // every lane has read trow[Cm] before it is rewritten
            for (int j = t; j < C; j += ND_NT) trow[j] = bnd_complement(trow[j], j, p, Cm, up);
            if (t == 0) N.flip[p] ^= 1;
            dirty = true;
        }

        // the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
        for (int j = t; j < Cm; j += ND_NT) {
            const double a = trow[j];
            bool part = a < -eps;
            if (skip_fixed) part = part && ub_s[j] > 0.0;
            ratios[j] = part ? zrow[j] / (-a) : inf;
        }
        __syncthreads();

        int q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
        if (long_step) {
            for (int pass = 0; pass < Cm && q >= 0; ++pass) {       // a column passes at most once: its ratio becomes +inf
                const double uq = ub_s[q];
                if (!(uq < inf)) break;
                const double prod = uq * trow[q];
                const double nb = trow[Cm] - prod;
                if (!(nb < -eps)) break;
                __syncthreads();                        // trow[q] and trow[Cm] read by every lane before the rewrite
                for (int i = t; i < R; i += ND_NT) {
                    double* row = tile + (size_t)i * S;
                    const double a = row[q];
                    const double pr = uq * a;
                    row[Cm] = row[Cm] - pr;
                    row[q] = -a;
                }
                if (t == 0) {
                    N.flip[q] ^= 1;
                    if (iter < N.trace_cap) { N.trace[2 * iter] = -1; N.trace[2 * iter + 1] = q; }
                    ratios[q] = inf;
                }
                ++iter;
                __syncthreads();
                q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
            }
        }
        if (q < 0) { status = LPX_INFEASIBLE; break; } // the complement and the passes stay applied

        // pivot prep: column snapshot, row r normalised in place (it is the pivot row of the update)
        const double piv = trow[q];
        for (int i = t; i < R; i += ND_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
        __syncthreads();
        for (int j = t; j < C; j += ND_NT) trow[j] = trow[j] / piv;
        if (t == 0) {
            N.basis[r] = q;
            if (iter < N.trace_cap) { N.trace[2 * iter] = kind ? -2 - r : r; N.trace[2 * iter + 1] = q; }
        }
        ++iter;
        if (kind) ++k1; else ++k0;
        dirty = true;
        __syncthreads();

        // the rank-1 update with the bits of lpx_update: every row but r, one multiply and one subtract per element
        for (int i = wave; i < R; i += ND_NW) {
            if (i == r) continue;
            const double f = pcol[i];
            double* row = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) {
                const double pr = f * trow[j];
                row[j] = row[j] - pr;
            }
        }
        __syncthreads();
    }
    __syncthreads();                                    // basis and flip as lane 0 left them, for every lane

    // ---- 7. the branch pick, as lpx_branch_pick_kernel
    int var = -1, total = 0;
    double x_var = 0.0;
    if (status == LPX_OPTIMAL) {
        double* vals = buf;
        const bool masked = in->has_mask && nint > 0;
        for (int j = t; j < nint; j += ND_NT) vals[j] = 0.0;
        __syncthreads();
        for (int i = t; i < m; i += ND_NT) {
            const int pb = N.basis[i];
            if ((unsigned)pb < (unsigned)nint) vals[pb] = tile[(size_t)i * S + Cm];
        }
        __syncthreads();
        MinIdx best; best.v = inf; best.i = INT_MAX;
        int nc = 0;
        for (int j = t; j < nint; j += ND_NT) {
            if (masked && !N.mask[j]) continue;
            const double v = vals[j];
            double x = N.flip[j] ? ub_s[j] - v : v;
            if (in->lo_used) x = x + N.lo[j];
            const double f = x - __builtin_floor(x);
            if (f > ptol && (1.0 - f) > ptol) {
                const double d = __builtin_fabs(f - 0.5);
                ++nc;
                if (d < best.v) { best.v = d; best.i = j; }
            }
        }
        best = block_min_idx<ND_NT>(best, s_v, s_i);
        block_excl_scan_sum<ND_NT>(nc, s_i, &total);
        if (best.i != INT_MAX) {
            var = best.i;
            const double v = vals[var];
            x_var = N.flip[var] ? ub_s[var] - v : v;
            if (in->lo_used) x_var = x_var + N.lo[var];
        }
    }

    // ---- 8. back to global memory: the tableau when it changed, the contiguous RHS copy, the state record
    if (dirty)
        for (int i = wave; i < R; i += ND_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += ND_NT) N.rhsbuf[i] = tile[(size_t)i * S + Cm];
    if (t == 0) {
        DevState s;
        s.status = status; s.iter = iter; s.r = -1; s.q = -1; s.phase = 2; s.fdf_count = k0; s.dual_iter = k1; s.primal_count = iter;
        s.forced_k = 0; s.qn = -1; s.c0n = 0; s.qn_valid = 0; s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
        *N.st = s;
        // ---- 9. the node record (pinned host memory)
        NodeOut* o = N.out;
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->flips = nflips; o->unrepairable = 0; o->inf_k = -1;
        o->var = var; o->candidates = total; o->x_var = x_var; o->z = zrow[Cm];
    }
