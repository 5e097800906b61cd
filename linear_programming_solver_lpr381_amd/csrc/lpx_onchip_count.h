// lpx_onchip_count.h -- step 2b of an on-chip node as included text (lpx_onchip.h says why text): over the columns left of the RHS,
// the count of the dual-feasibility flips that step 5 will make and of the columns no flip can repair.
// Expects in scope: t, lane, wave, Cm, eps, inf, ub_s (the edit of this node applied), s_tot / s_bad [OC_NW], and
//   zrow   the objective row, wherever its bits are the truth: the tableau in global memory while the tile is not loaded
//          (the shift of the edit does not write left of the RHS), the tile afterwards.
// Leaves: n (flips) and bad (unrepairable columns), the same in every lane.  Two barriers; every lane of the workgroup comes here.
        int n = 0, bad = 0;
        for (int base = 0; base < Cm; base += OC_NT) {  // uniform trip count
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
        for (int w = 0; w < OC_NW; ++w) { n += s_tot[w]; bad += s_bad[w]; }
