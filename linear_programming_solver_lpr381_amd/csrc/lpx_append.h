// lpx_append.h -- the in-place append step shared by the GMI cut round (lpx_cuts.hip) and the new-row edit of the
// post-optimal path (lpx_postopt.hip): K rows go in just above the objective row, K slack columns just before the RHS
// column, inside the handle's capacity and without a second buffer.
#pragma once
#include "lpx_internal.h"

namespace lpx {

// One launch of ncb + ceil((m + K) / nt) workgroups of nt lanes.  Workgroups [0, ncb) own one column j < Cm each lane: they
// move the objective row's entry down to row m + K (reading it before new row 0 overwrites it) and write rows m .. m+K-1
// there with rows.body(k, j).  The other workgroups own one old row r < m each lane (its tail: K new zero slack entries
// and the RHS moved from Cm to Cm + K); the lane of r == m writes the tails of the objective row and of the K new rows
// (rows.slack(k, i) in slack column Cm + i, rows.rhs(k) in the RHS column).  Returns the row index r of a tail lane, -1 in
// a column workgroup, so that the caller can write the basis entry of that row afterwards.
template <class NewRows>
__device__ __forceinline__ int append_rows_inplace(double* __restrict__ T, int ld, int m, int Cm, int K, int ncb, int nt,
                                                   const NewRows& rows)
{
    if ((int)blockIdx.x < ncb) {
        const int j = blockIdx.x * nt + threadIdx.x;
        if (j >= Cm) return -1;
        const double obj = T[(size_t)m * ld + j];       // read before new row 0 overwrites it
        T[(size_t)(m + K) * ld + j] = obj;
        for (int k = 0; k < K; ++k) T[(size_t)(m + k) * ld + j] = rows.body(k, j);
        return -1;
    }
    const int r = (blockIdx.x - ncb) * nt + threadIdx.x;
    if (r < m) {
        double* row = T + (size_t)r * ld;
        const double bv = row[Cm];
        for (int k = 0; k < K; ++k) row[Cm + k] = 0.0;
        row[Cm + K] = bv;
    } else if (r == m) {
        const double bv = T[(size_t)m * ld + Cm];
        double* obj = T + (size_t)(m + K) * ld;
        for (int k = 0; k < K; ++k) obj[Cm + k] = 0.0;
        obj[Cm + K] = bv;
        for (int k = 0; k < K; ++k) {
            double* row = T + (size_t)(m + k) * ld;
            for (int i = 0; i < K; ++i) row[Cm + i] = rows.slack(k, i);
            row[Cm + K] = rows.rhs(k);
        }
    }
    return r;
}

}  // namespace lpx
