// lpx_onchip_fix.h -- step 7b of an on-chip node as included text: reduced-cost bound tightening (include/lpx.h, "reduced-cost
// tightening"), behind the pick and in front of the write-back.  The node ended LPX_OPTIMAL, so its objective row is dual feasible:
// a nonbasic integer column j with reduced cost d = T[m,j] > eps cannot rise above t = floor((z - fix_bound) / d) without the
// objective falling to fix_bound, and t < ub[j] tightens its range to [0, t] in the column's own (flipped or unflipped) variable.
// Only ub and lo change: a nonbasic column stands at 0, so the edit has a zero RHS shift and the tile stays as it is.
// Expects in scope: t, lane, wave, m, Cm, S, nint, eps, inf, tile, zrow, ub_s, list (int32 view of buf, free behind the pick), s_tot
// [OC_NW], status, N (NodeParams: ub, lo, mask), in (NodeIn: has_mask), basis, flip, nfix (preset to 0), and from the kernel
//   fix_bound             the bound to beat (-inf: the step does nothing)
//   fcols, flower, fupper the list the host reads: nint entries each (pinned host memory).
// Leaves: nfix, the number of tightened columns, and their triples (col, lower, upper) in ascending column order -- exactly the
// triples a bound edit of the handle would take.  The order is that of lpx_onchip_flips.h: a ballot per wave, a prefix over the
// wave totals, no atomics.  Every loop is bounded by nint or m; status, z and fix_bound are uniform, so every lane meets every barrier.
    if (status == LPX_OPTIMAL && fix_bound > -inf && zrow[Cm] > fix_bound) {       // -inf: an entry of a batch that tightens nothing
        int* mark = list;                               // 1 = the column is basic (through basis, never inferred from a zero)
        __syncthreads();                                // every lane is past the values of the pick
        for (int j = t; j < nint; j += OC_NT) mark[j] = 0;
        __syncthreads();
        for (int i = t; i < m; i += OC_NT) {
            const int pb = basis[i];
            if ((unsigned)pb < (unsigned)nint) mark[pb] = 1;
        }
        __syncthreads();
        const double gap = zrow[Cm] - fix_bound;        // one subtract, the same for every column
        const bool fmasked = in->has_mask && nint > 0;
        for (int base = 0; base < nint; base += OC_NT) {
            const int j = base + t;
            bool hit = false;
            double tt = 0.0;
            if (j < nint && !(fmasked && !N.mask[j]) && !mark[j]) {
                const double d = zrow[j];
                if (d > eps) {
                    const double g = gap / d;           // one IEEE divide
                    tt = __builtin_floor(g);
                    hit = tt < ub_s[j];
                }
            }
            const unsigned long long mi = __ballot(hit);
            const int before = __popcll(mi & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == 0) s_tot[wave] = __popcll(mi);
            __syncthreads();
            int pre = 0, tot = 0;
            for (int w = 0; w < OC_NW; ++w) { const int y = s_tot[w]; if (w < wave) pre += y; tot += y; }
            if (hit) {
                const int k = nfix + pre + before;      // < columns tested so far <= nint
                const double lj = N.lo[j];
                double lw = lj, up = lj + tt;
                if (flip[j]) {                          // the column stands for up - x: its range shrinks from below
                    up = lj + ub_s[j];
                    lw = up - tt;
                    N.lo[j] = lw;
                }
                N.ub[j] = tt;
                fcols[k] = j; flower[k] = lw; fupper[k] = up;
            }
            nfix += tot;
        }
    }
