// lpx_onchip_pick.h -- step 7 of an on-chip node as included text: the branch pick, as lpx_branch_pick_kernel.
// Expects in scope: t, m, Cm, S, nint, ptol, inf, tile, ub_s, buf, s_v / s_i [OC_NW], status, N (NodeParams: mask, lo), in (NodeIn:
// has_mask), basis, flip, and
//   lo_used           whether the handle has stored a lower shift (a child inside a chain may have raised it)
//   var, x_var, total preset to -1, 0.0 and 0 by the kernel.
// Leaves: var (the most fractional column, -1 = none), x_var (its value) and total (the count of fractional columns).
    if (status == LPX_OPTIMAL) {
        double* vals = buf;
        const bool masked = in->has_mask && nint > 0;
        for (int j = t; j < nint; j += OC_NT) vals[j] = 0.0;
        __syncthreads();
        for (int i = t; i < m; i += OC_NT) {
            const int pb = basis[i];
            if ((unsigned)pb < (unsigned)nint) vals[pb] = tile[(size_t)i * S + Cm];
        }
        __syncthreads();
        MinIdx best; best.v = inf; best.i = INT_MAX;
        int nc = 0;
        for (int j = t; j < nint; j += OC_NT) {
            if (masked && !N.mask[j]) continue;
            const double v = vals[j];
            double x = flip[j] ? ub_s[j] - v : v;
            if (lo_used) x = x + N.lo[j];
            const double f = x - __builtin_floor(x);
            if (f > ptol && (1.0 - f) > ptol) {
                const double d = __builtin_fabs(f - 0.5);
                ++nc;
                if (d < best.v) { best.v = d; best.i = j; }
            }
        }
        best = block_min_idx<OC_NT>(best, s_v, s_i);
        block_excl_scan_sum<OC_NT>(nc, s_i, &total);
        if (best.i != INT_MAX) {
            var = best.i;
            const double v = vals[var];
            x_var = flip[var] ? ub_s[var] - v : v;
            if (lo_used) x_var = x_var + N.lo[var];
        }
    }
