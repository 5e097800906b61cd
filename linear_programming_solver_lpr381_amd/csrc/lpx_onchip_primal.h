// lpx_onchip_primal.h -- the body of the on-chip bounded PRIMAL loop, included as the text of both of its kernels in
// lpx_bounded_primal.hip: lpx_bounded_primal_onchip (one LP, the record a kernel argument) and lpx_bounded_primals_onchip (the batch,
// workgroup b takes P[b]).  Like lpx_bounded_node_body.h it is a sequence of statements, not a header in the usual sense: it expects
// `const PrimalParams N` in scope, every `return` and every `break` of it is taken by all lanes of the workgroup, and it shares no
// text with the node's step files (whose instruction text is pinned), only the helpers of lpx_onchip.h.
//
// The arithmetic is the contract "bounded-variable primal simplex" of include/lpx.h, steps 1-4, with the bits of the launches form
// (lpx_bounded_select + lpx_update): one event per trip, the iteration limit tested first, so the loop makes at most max_iter + 1
// trips.  A bound flip is bnd_flip_column's text on the tile, the pivot prep is bnd_pivot_prep's (the complement of a kind-1 row
// applied in front of the division, which gives the bits of complementing in place), the update is lpx_update's.
    extern __shared__ double pr_lds[];
    __shared__ double s_v[OC_NW];
    __shared__ int s_i[OC_NW];
    __shared__ int s_out;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int R = N.R, C = N.C, m = R - 1, Cm = C - 1;
    const int S = C | 1;
    const size_t ld = (size_t)N.ld;
    const double inf = __builtin_inf();
    const double eps = N.eps, rtol = N.ratio_tol;
    const int max_iter = N.max_iter, trace_cap = N.trace_cap;
    int32_t* const basis = N.basis; uint8_t* const flip = N.flip; int32_t* const trace = N.trace;

    double* tile = pr_lds;
    double* ub_s = tile + (size_t)R * S;
    double* buf = ub_s + C;

    // ---- 1. the bounds and the live window into LDS: a wave per row, lanes along it
    for (int j = t; j < Cm; j += OC_NT) ub_s[j] = N.ub[j];
    for (int i = wave; i < R; i += OC_NW) {
        const double* src = N.T + (size_t)i * ld;
        double* dst = tile + (size_t)i * S;
        for (int j = lane; j < C; j += 64) dst[j] = src[j];
    }
    __syncthreads();

    // ---- 2. the event loop
    double* zrow = tile + (size_t)m * S;
    double* ratios = buf;
    double* pcol = buf;
    bool dirty = false;                                 // uniform: the tile differs from the tableau in global memory
    int iter = 0, k0 = 0, k1 = 0, nflips = 0, status = LPX_ITER_LIMIT;
    for (int trip = 0; trip <= max_iter; ++trip) {
        if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
        // ChooseEntering: the event before this one ended on a barrier behind its writes of the objective row
        const int q = block_first_min_below<OC_NT>(zrow, 1, Cm, eps, s_v, s_i);
        if (q < 0) { status = LPX_OPTIMAL; break; }

        // the three-way ratios of rows 0..m-1: a column walk of the tile (odd stride: no bank conflict), ub through the basis
        for (int i = t; i < m; i += OC_NT) {
            const double a = tile[(size_t)i * S + q];
            const double b = tile[(size_t)i * S + Cm];
            const int pb = basis[i];
            const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
            double rho = inf;
            if (a > eps) rho = b / a;                                   // basic variable goes to zero
            else if (a < -eps && u < inf) rho = (u - b) / (-a);         // basic variable goes to its upper bound
            ratios[i] = rho;
        }
        __syncthreads();
        const int r = rs_hysteresis(m, rtol, ratios, s_v, s_i, &s_out);
        const double best = r >= 0 ? ratios[r] : inf;
        const double uq = ub_s[q];
        // what the pivot needs of row r as it stands, read by every lane in front of the barrier below
        double* trow = tile + (size_t)(r >= 0 ? r : 0) * S;
        const double a_rq = trow[q];
        const int p = r >= 0 ? basis[r] : -1;
        __syncthreads();                                // every lane is past the ratios and row r before either is rewritten

        if (uq < inf && uq <= best) {                   // BOUND FLIP of column q, ties go to the flip: RHS column and column q, R rows
            for (int i = t; i < R; i += OC_NT) {
                double* row = tile + (size_t)i * S;
                const double a = row[q];
                const double prod = uq * a;             // mul, then sub: contraction is off
                row[Cm] = row[Cm] - prod;
                row[q] = -a;
            }
            if (t == 0) {
                flip[q] ^= 1;
                if (iter < trace_cap) { trace[2 * iter] = -1; trace[2 * iter + 1] = q; }
            }
            ++iter; ++nflips;
            dirty = true;
            __syncthreads();
            continue;
        }
        if (r < 0) { status = LPX_UNBOUNDED; break; }

        // pivot prep: kind 1 (T[r,q] <= eps) leaves at its upper bound, row r complemented in front of the division
        const int kind = a_rq > eps ? 0 : 1;
        const double up = kind ? ub_s[p] : 0.0;
        const double piv = kind ? -a_rq : a_rq;
        for (int i = t; i < R; i += OC_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
        for (int j = t; j < C; j += OC_NT) {            // a lane rewrites the entries of row r that only it reads here
            double v = trow[j];
            if (kind) v = bnd_complement(v, j, p, Cm, up);
            trow[j] = v / piv;
        }
        if (t == 0) {
            if (kind) flip[p] ^= 1;
            basis[r] = q;
            if (iter < trace_cap) { trace[2 * iter] = kind ? -2 - r : r; trace[2 * iter + 1] = q; }
        }
        ++iter;
        if (kind) ++k1; else ++k0;
        dirty = true;
        __syncthreads();

        // the rank-1 update with the bits of lpx_update: every row but r, one multiply and one subtract per element
        for (int i = wave; i < R; i += OC_NW) {
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

    // ---- 3. back to global memory: the tableau when an event wrote it, the contiguous RHS copy, the state record, the result
    if (dirty)
        for (int i = wave; i < R; i += OC_NW) {
            double* dst = N.T + (size_t)i * ld;
            const double* src = tile + (size_t)i * S;
            for (int j = lane; j < C; j += 64) dst[j] = src[j];
        }
    for (int i = t; i < R; i += OC_NT) N.rhsbuf[i] = tile[(size_t)i * S + Cm];
    if (t == 0) {
        DevState s;                                     // as the last lpx_bounded_select launch of the launches form leaves it
        s.status = status; s.iter = iter; s.r = -1; s.q = -1; s.phase = 2; s.fdf_count = k0; s.dual_iter = k1; s.primal_count = iter;
        s.forced_k = 0; s.qn = -1; s.c0n = 0; s.qn_valid = 0; s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
        *N.st = s;
        lpx_primal_record* o = N.out;                   // pinned host memory
        o->status = status; o->events = iter; o->kind0 = k0; o->kind1 = k1; o->flips = nflips; o->z = zrow[Cm];
    }
