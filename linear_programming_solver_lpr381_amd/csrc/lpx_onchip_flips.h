// lpx_onchip_flips.h -- step 5 of an on-chip node as included text: the dual-feasibility flips, j ascending -- the ordered list (a
// ballot per wave, a prefix over the wave totals), then a lane per row walks it: BOUND FLIP arithmetic, objective row included.
// Expects in scope: t, lane, wave, R, Cm, S, eps, inf, tile, ub_s, list (int32 view of buf), s_tot [OC_NW], nflips (step 2b's count),
//   zrow   the objective row of the tile
//   flip   the flip marks this node writes (the handle's, or a probe's slice of the workspace)
//   dirty  set when the tile is written (a dead local where nothing is stored back).
    if (nflips > 0) {
        int n = 0;
        for (int base = 0; base < Cm; base += OC_NT) {
            const int j = base + t;
            bool in_l = false;
            if (j < Cm) { const double u = ub_s[j]; in_l = zrow[j] < -eps && u > 0.0 && u < inf; }
            const unsigned long long mi = __ballot(in_l);
            const int before = __popcll(mi & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) s_tot[wave] = __popcll(mi);
            __syncthreads();
            int pre = 0, tot = 0;
            for (int w = 0; w < OC_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
            if (in_l) list[n + pre + before] = j;       // n + pre + before < columns tested so far <= Cm
            n += tot;
        }
        __syncthreads();
        for (int k = t; k < n; k += OC_NT) flip[list[k]] ^= 1;
        for (int i = t; i < R; i += OC_NT) {
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
