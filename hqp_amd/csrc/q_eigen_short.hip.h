// gfx950 kernel of hqpkkt_q_eigen_control_short (include/hqpkkt.h): the eigenvalue control of Hqp_HL_BFGS on a plan whose
// blocks are all at most 64 long - the partition of a DOCP, 125 000 blocks of order 8 at n = 10^6 -, in ONE launch.  The
// reference calls symmeig per block (hqp/Hqp_HL_BFGS.C:203-212): Householder's reduction to a tridiagonal T, then T's
// eigenvalues.  So does this kernel, a block per wavefront, where k_qe_* (q_eigen.hip.h) run a Lanczos recurrence of 45
// launches that each pass n-vectors through memory and keep a basis of steps x n doubles:
//   launch    nblocks workgroups of ONE wavefront (the condition of eig::ritz); instances by the plan's longest block,
//             LMAX = 8, 16, 32, 64, so that a plan of order-8 blocks holds 6.4 KB of LDS per wavefront and not 35 KB
//   gather    the block's L x L image A in LDS, cleared, leading dimension LMAX + 1: lane i has row i, and the lanes'
//             reads of one column fall into different banks.  Lane i < L walks row first + i of the symmetric image Qf
//             (what k_qb_rows reads) and stores the entries whose column lies in the block.  An entry across blocks is
//             not loaded; a place nothing is stored at stays +0.0
//   g, theta  offsum_i = sum of |a_ij|, j != i, in ascending j from +0.0, every add rounded on its own; g = min_i (a_ii -
//             offsum_i) by eig::nan_min over a butterfly (min has no order; lane 0's value is the block's); theta, the
//             outcomes 0 and 6 exactly as k_qe_begin forms them.  Such a block is done: its T words are 0
//   reduce    for k = 0 .. L - 3 (tred2's steps on the full image, a lane per row): x = A[k+1 .. L-1][k]; where x[1 ..] is
//             exactly zero no reflector is needed, beta_k = x_0 (a zero sub-column: beta_k = 0, no division); else
//             ss = sum x_i^2, beta_k = -sign(x_0) sqrt(ss), v = x with v_0 = x_0 - beta_k, h = ss - x_0 beta_k = v'v / 2,
//             p = A v / h (lane i: fused multiply-adds over ascending j, one division), c = v'p / 2h, q = p - c v, and
//             a_ij <- fl(a_ij - fl(fl(v_i q_j) + fl(q_i v_j))) on the trailing block - products and sums that commute, so the
//             image stays symmetric bit for bit.  The wavefront's sums are the butterfly of kktdev::wave_sum, lanes
//             past the block adding +0.0: fixed by the lane, which is the index inside the block.  alpha_i = a_ii at the
//             end, beta_{L-2} = a_{L-1,L-2}, beta_{L-1} = 0.  L = 1 and L = 2 need no reflector.  Squares that overflow, and a
//             sub-column whose squares all underflow, end as a T that is not finite (outcome 4, the block left alone)
//   bracket   T out (alpha_0 .. alpha_{L-1}, then beta_0 .. beta_{L-2}, 0; stride 2 cap, words past L 0: every word of the
//             block written once), then eig::ritz on T unchanged, its work arrays in the LDS of the image, which is done
//             with.  beta_{L-1} = 0: rho = 0, lambda_est = lo, outcome 1, 2 or 4, never 3
//   shift     after a barrier lane i < L: q_ii <- fl(q_ii + d_b) through didx, d_b = the report's word 7; d_b == 0: nothing
// So a block's bits depend on its length and its values alone - not on where it lies, on the other blocks or on the
// mode.  Plain loads and stores in the handle's stream: no atomics, nothing polled, nothing read back, no clears ahead
// of the launch.  No contraction; sums that fuse say __fma_rn.
// No MFMA: the work is a matrix-vector product and a symmetric rank-2 update of order <= 64 inside one wavefront, L^2
// multiply-adds per step against operands that change every step - there is no product of two matrices in it to tile.
// Not built: several order-8 blocks per wavefront (8 of 64 lanes work here).
// Included by q_entries.hip behind q_eigen.hip.h.
#pragma once
#include "q_eigen.hip.h"

namespace qv {

template <int LMAX>
struct QesLds {
  union {
    double A[LMAX * (LMAX + 1)];  // the image, then ritz's work arrays
    eig::RitzLds ritz;
  };
  double v[LMAX], q[LMAX], al[LMAX], be[LMAX];
};

template <int LMAX>
__global__ void __launch_bounds__(64) k_qes_block(const int *__restrict__ boff, kktdev::CsrDev Q, const int *__restrict__ didx,
                                                  double *vals, const double *__restrict__ flr, double eps2,
                                                  const double *__restrict__ bfgs, int cap, double *T, double *rep) {
#pragma clang fp contract(off)
  constexpr int LD = LMAX + 1;
  __shared__ QesLds<LMAX> s;
  const long long b = blockIdx.x;
  const int lane = threadIdx.x, first = boff[b], L = boff[b + 1] - first;
  if (L < 1 || L > LMAX || L > cap) return;  // (never: the host picks LMAX and cap from the plan's longest block)
  double *A = s.A, *r = rep + QE_REPORT * b, *Tb = T + 2 * (long long)cap * b;
  for (int k = lane; k < L * LD; k += 64) A[k] = 0.0;
  __syncthreads();
  if (lane < L) {
    const int row = first + lane;
    for (int k = Q.ptr[row], e = Q.ptr[row + 1]; k < e; k++) {
      const int c = Q.col[k] - first;
      if (c >= 0 && c < L) A[lane * LD + c] = Q.val[k];
    }
  }
  __syncthreads();
  double g = __builtin_inf();
  if (lane < L) {
    double off = 0.0;
    for (int j = 0; j < L; j++)
      if (j != lane) off = off + fabs(A[lane * LD + j]);
    g = A[lane * LD + lane] - off;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) g = eig::nan_min(g, __shfl_xor(g, o));
  g = __shfl(g, 0);
  double theta = eps2;
  bool skipped = false;
  if (bfgs) {
    const double sQs = bfgs[QV_REPORT * b + 1];
    if (sQs < theta && sQs >= 0.0) theta = sQs;
    skipped = bfgs[QV_REPORT * b + 7] >= 2.0;
  }
  if (flr) theta = flr[b];
  const int outcome = skipped ? 6 : g >= theta ? 0 : -1;
  if (lane == 0) {
    r[0] = g, r[1] = theta;
    for (int w = 2; w < QE_REPORT - 1; w++) r[w] = 0.0;
    r[QE_REPORT - 1] = (double)outcome;
  }
  if (outcome >= 0) {  // (uniform over the wavefront)
    for (int k = lane; k < 2 * cap; k += 64) Tb[k] = 0.0;
    return;
  }
  for (int k = 0; k + 2 < L; k++) {
    const bool in = lane > k && lane < L;
    const double x = in ? A[lane * LD + k] : 0.0, x0 = __shfl(x, k + 1);
    double tail = lane > k + 1 ? fabs(x) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tail = eig::nan_max(tail, __shfl_xor(tail, o));
    if (__shfl(tail, 0) == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
      if (lane == 0) s.be[k] = x0;
      continue;
    }
    const double ss = kktdev::wave_sum(x * x);
    const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
    const double v = lane == k + 1 ? x - beta : x;
    const double h = ss - x0 * beta;
    if (lane < L) s.v[lane] = v;
    __syncthreads();
    double p = 0.0;
    if (in) {
      for (int j = k + 1; j < L; j++) p = __fma_rn(A[lane * LD + j], s.v[j], p);
      p = p / h;
    }
    const double c = kktdev::wave_sum(v * p) / (h + h);
    const double q = p - c * v;
    if (lane < L) s.q[lane] = q;
    __syncthreads();
    if (in)
      for (int j = k + 1; j < L; j++) A[lane * LD + j] = A[lane * LD + j] - (v * s.q[j] + q * s.v[j]);
    if (lane == 0) s.be[k] = beta;
    __syncthreads();
  }
  if (lane < L) s.al[lane] = A[lane * LD + lane];
  if (lane == L - 1) {
    if (L >= 2) s.be[L - 2] = A[lane * LD + L - 2];
    s.be[L - 1] = 0.0;
  }
  __syncthreads();  // (the image is done with: ritz's arrays take its place)
  for (int k = lane; k < 2 * cap; k += 64) Tb[k] = k < L ? s.al[k] : (k >= cap && k - cap < L) ? s.be[k - cap] : 0.0;
  eig::ritz(s.al, s.be, L, theta, r, s.ritz);
  __syncthreads();
  const double d = r[7];
  if (d != 0.0 && lane < L) {
    const int k = didx[first + lane];
    vals[k] = vals[k] + d;
  }
}

}  // namespace qv
