// Wide rows of the inequality block C in the STAGED engine (hqpkkt_set_dense_rows; StagedPlan::wr_rows): the r rows of a
// stage with many stored entries are the dense block E_k (r rows of ld doubles, zero in the padding), and their share of
// H = Q + C'(Z/W)C is the thin-K MFMA product S'S with S = diag(sqrt(z / w)) E_k (st_add_h_wide, staged_host.hip.h).  With
// the square root in both operands entry (i, j) of the product and its image are the same sum of the same products.
// Included by staged_engine.hip behind staged.hip.h.
#pragma once

namespace stg {

struct RowsScale {
  const double *E;   // r x ld, 16-byte aligned, ld even
  double *S;         // the same shape
  const int *rows;   // the rows of C (indices into wt)
  const double *wt;  // z / w per row of C (k_weights)
  int r;
  long long ld;
};
// S[i][j] = sqrt(wt[rows[i]]) E[i][j]: a thread per pair of doubles
__global__ void __launch_bounds__(256) k_st_rows_scale(RowsScale a) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x, half = a.ld / 2;
  if (q >= a.r * half) return;
  const double s = sqrt(a.wt[a.rows[q / half]]);
  const double2_t v = reinterpret_cast<const double2_t *>(a.E)[q];
  reinterpret_cast<double2_t *>(a.S)[q] = (double2_t){s * v.x, s * v.y};
}

}  // namespace stg
