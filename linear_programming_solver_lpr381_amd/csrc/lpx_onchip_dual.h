// lpx_onchip_dual.h -- step 6 of an on-chip node as included text: the dual loop.  Every trip ends the loop or makes at least one
// event, and the iteration limit is tested first, so the loop makes at most max_iter + 1 trips.
// Expects in scope: t, lane, wave, R, C, m, Cm, S, eps, rtol, cutoff, inf, skip_fixed, long_step, cut, tile, ub_s, buf,
// s_v / s_i [OC_NW], s_out, and the names by which the kernels differ:
//   zrow               the objective row of the tile
//   basis, flip        what this node reads and writes: the handle's arrays, or a probe's slice of the workspace
//   trace, trace_cap   the handle's event trace, from 0 for every node (trace_cap = 0: none is kept)
//   dirty              set when the tile is written (a dead local where nothing is stored back)
//   max_iter           the event limit
//   GUARD              the file's switch (lpx_onchip.h): the stall guard of include/lpx.h ("stall guard"), with
//   stall_events       its threshold (a constant where GUARD is false).
// Leaves: status, iter, k0, k1 and, for the guard, bland_events and first_bland -- all uniform over the workgroup.
// The guard: z_ref is the objective at the last progress, stall the pivots since; once `stall_events` pivots have brought no
// progress the trip selects by Bland's rule (least index) until the objective moves again.  Its two selections are block_min_idx
// reductions on the scratch the loop has already: the leaving row on the key (basic index, row), the entering column first on
// (ratio, column) for the minimum and then on (0, column) over the columns within ratio_tol of it.
    int iter = 0, k0 = 0, k1 = 0, status = LPX_ITER_LIMIT;
    [[maybe_unused]] int stall = 0, bland_events = 0, first_bland = -1;
    double* ratios = buf;
    double* pcol = buf;
    [[maybe_unused]] double z_ref = zrow[Cm];           // behind the edit and the flips; the next write of it is behind a barrier
    for (int trip = 0; trip <= max_iter; ++trip) {
        if (iter >= max_iter) { status = LPX_ITER_LIMIT; break; }
#if LPX_ONCHIP_GUARD    // the objective read once for both tests.  A preprocessor switch here and nowhere else: either spelling for
        // all kernels moves the code of the others (profiles/r18_onchip_text_isa.md); the rest of the guard hangs on `GUARD`
        const double z_now = zrow[Cm];
        if (cut && z_now <= cutoff) { status = LPX_CUTOFF; break; }
        if (z_now < z_ref - eps) { z_ref = z_now; stall = 0; }
#else
        if (cut && zrow[Cm] <= cutoff) { status = LPX_CUTOFF; break; }
#endif
        const bool bland = GUARD && stall >= stall_events;

        // leaving row: first strict minimum of the infeasibilities below -eps; in Bland mode the least basic index among them
        // (the key is the index as a double, exact; equal keys cannot occur in a basis, and the lowest row would win)
        MinIdx mn; mn.v = bland ? inf : -eps; mn.i = INT_MAX;
        for (int i = t; i < m; i += OC_NT) {
            const double b = tile[(size_t)i * S + Cm];
            const int pb = basis[i];
            const double u = (unsigned)pb < (unsigned)Cm ? ub_s[pb] : inf;
            double w = inf;
            if (b < -eps) w = b;
            else if (u < inf) w = u - b;
            if (bland) { if (w < -eps && (double)pb < mn.v) { mn.v = (double)pb; mn.i = i; } }
            else if (w < mn.v) { mn.v = w; mn.i = i; }
        }
        mn = block_min_idx<OC_NT>(mn, s_v, s_i);
        if (mn.i == INT_MAX) { status = LPX_OPTIMAL; break; }
        const int r = mn.i;
        double* trow = tile + (size_t)r * S;
        const int kind = trow[Cm] < -eps ? 0 : 1;
        const int p = basis[r];

        // kind 1: the complement of row r in place, in front of the ratios
        if (kind) {
            const double up = ub_s[p];
            __syncthreads();                            // every lane has read trow[Cm] before it is rewritten
            for (int j = t; j < C; j += OC_NT) trow[j] = bnd_complement(trow[j], j, p, Cm, up);
            if (t == 0) flip[p] ^= 1;
            dirty = true;
        }

        // the ratios of row r, formed once (a lane reads the entries of trow it wrote itself)
        for (int j = t; j < Cm; j += OC_NT) {
            const double a = trow[j];
            bool part = a < -eps;
            if (skip_fixed) part = part && ub_s[j] > 0.0;
            ratios[j] = part ? zrow[j] / (-a) : inf;
        }
        __syncthreads();

        int q;
        if (bland) {                                    // the lowest column within ratio_tol of the minimum; no hysteresis scan
            MinIdx lo_r; lo_r.v = inf; lo_r.i = INT_MAX;
            for (int j = t; j < Cm; j += OC_NT) { const double v = ratios[j]; if (v < lo_r.v) { lo_r.v = v; lo_r.i = j; } }
            lo_r = block_min_idx<OC_NT>(lo_r, s_v, s_i);
            q = -1;
            if (lo_r.i != INT_MAX) {                    // uniform; a ratio is never NaN where the tableau is finite
                const double band = lo_r.v + rtol;
                MinIdx first; first.v = inf; first.i = INT_MAX;
                for (int j = t; j < Cm; j += OC_NT)
                    if (ratios[j] <= band && first.i == INT_MAX) { first.v = 0.0; first.i = j; }
                first = block_min_idx<OC_NT>(first, s_v, s_i);
                q = first.i != INT_MAX ? first.i : lo_r.i;      // a negative ratio_tol leaves the band empty: the minimum itself
            }
            __syncthreads();                            // as rs_hysteresis ends: every lane is past the ratios and the scratch
        } else q = rs_hysteresis(Cm, rtol, ratios, s_v, s_i, &s_out);
        if (long_step && !bland) {
            for (int pass = 0; pass < Cm && q >= 0; ++pass) {       // a column passes at most once: its ratio becomes +inf
                const double uq = ub_s[q];
                if (!(uq < inf)) break;
                const double prod = uq * trow[q];
                const double nb = trow[Cm] - prod;
                if (!(nb < -eps)) break;
                __syncthreads();                        // trow[q] and trow[Cm] read by every lane before the rewrite
                for (int i = t; i < R; i += OC_NT) {
                    double* row = tile + (size_t)i * S;
                    const double a = row[q];
                    const double pr = uq * a;
                    row[Cm] = row[Cm] - pr;
                    row[q] = -a;
                }
                if (t == 0) {
                    flip[q] ^= 1;
                    if (iter < trace_cap) { trace[2 * iter] = -1; trace[2 * iter + 1] = q; }
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
        for (int i = t; i < R; i += OC_NT) pcol[i] = (i == r) ? 0.0 : tile[(size_t)i * S + q];     // the ratios are dead
        __syncthreads();
        for (int j = t; j < C; j += OC_NT) trow[j] = trow[j] / piv;
        if (t == 0) {
            basis[r] = q;
            if (iter < trace_cap) { trace[2 * iter] = kind ? -2 - r : r; trace[2 * iter + 1] = q; }
        }
        if (bland) { if (bland_events == 0) first_bland = iter; ++bland_events; }
        ++iter; ++stall;
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
