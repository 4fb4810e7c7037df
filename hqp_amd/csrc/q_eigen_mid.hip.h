// gfx950 kernels of hqpkkt_q_eigen_control_exact (include/hqpkkt.h) for the blocks of a plan that are 65 .. 128 long - a DOCP
// stage of 60 - 120 states and controls -: the mathematics and the contract of k_qes_block (q_eigen_short.hip.h), which
// serves the plan's blocks up to 64 in the same call, on a block that no single wavefront holds.  Two launches over the
// LIST of those blocks (made on the host from the plan's offsets; blockIdx.x indexes the list, not the plan):
// k_qem_block  one workgroup of 256 threads, 4 wavefronts, per block; instances by the list's longest block, LMAX = 96
//              (76.6 KB of LDS, two workgroups per CU) and LMAX = 128 (134 KB, one per CU), dynamic LDS raised by the host
//   split      thread t has row i = t & 127 of the image and column half hf = t >> 7: wavefronts 0, 1 hold rows 0 .. 63 and
//              64 .. 127 with the first half of the trailing columns, wavefronts 2, 3 the same rows with the second half.
//              The trailing columns k + 1 .. L - 1 of step k are cut at mid = k + 1 + ceil((L - k - 1) / 2)
//   LDS        the image A, leading dimension LMAX + 1 (odd: the lanes' reads of one column fall into different banks),
//              then v, q, al, be, ph (the second half's share of p), and 8 words of the wavefronts' partial sums
//   gather     as k_qes_block: the image cleared by all threads, thread i < L (half 0) walks row first + i of Qf
//   g, theta   offsum_i in ascending j from +0.0, every add rounded on its own, by the thread of row i and half 0;
//              g = min_i (a_ii - offsum_i): eig::nan_min over a butterfly per wavefront, lane 0's value to LDS, the four
//              values in ascending wavefront order; theta and the outcomes 0 and 6 as k_qes_block forms them
//   reduce     tred2's steps k = 0 .. L - 3 with k_qes_block's zero-sub-column rule, beta_k, v, h, p = A v / h, q and the
//              commuting rank-2 update a_ij <- fl(a_ij - fl(fl(v_i q_j) + fl(q_i v_j))): the image stays symmetric bit for
//              bit.  Row i's product is two chains of fused multiply-adds, one per half over its columns in ascending j
//              from +0.0; p_i = fl(fl(half0 + half1) / h), the second half's share through LDS.  ss = x'x, v'p and the max
//              that finds a zero tail: kktdev::wave_sum (a butterfly) in the wavefronts of half 0, rows past the block
//              adding +0.0, then fl(wavefront 0's + wavefront 1's) through LDS.  Six barriers per step
//   T out      alpha then beta, stride 2 cap, words past L zero: every word of the block written once
//              So a block's bits depend on its length and its values alone - not on where it lies, on the other blocks
//              or on the mode -, and are equal from call to call
// k_qem_ritz   one workgroup of ONE wavefront per listed block (the condition of eig::ritz, whose barriers and early
//              returns are written for that; it is not called from the 256 threads above): reads the outcome word and
//              T from memory - a block decided by g (0, 6) is skipped -, eig::ritz unchanged on its own LDS, then
//              q_ii <- fl(q_ii + d_b) through didx, two rows per lane, where d_b != 0.  rho = 0, never outcome 3
// Plain loads and stores in the handle's stream: no atomics, nothing polled, nothing read back, no clears ahead of the
// launches.  No contraction; sums that fuse say __fma_rn.
// No MFMA: every step is a matrix-vector product and a symmetric rank-2 update of order <= 128 whose operands change with
// the step - L^2 multiply-adds against a vector, no product of two matrices to tile.
// Not built: several order-8 blocks per wavefront.  (Blocks over 128, whose image leaves LDS: q_eigen_long.hip.h.)
// Included by q_entries.hip behind q_eigen_short.hip.h.
#pragma once
#include "q_eigen_short.hip.h"

namespace qv {

static const int QEM_MIN = 65, QEM_MAX = 128;  // the lengths these kernels serve
template <int LMAX>
constexpr size_t qem_lds_bytes() {
  return sizeof(double) * (LMAX * (LMAX + 1) + 5 * LMAX + 8);
}

template <int LMAX>
__global__ void __launch_bounds__(256) k_qem_block(const int *__restrict__ list, const int *__restrict__ boff, kktdev::CsrDev Q,
                                                   const double *__restrict__ flr, double eps2, const double *__restrict__ bfgs,
                                                   int cap, double *T, double *rep) {
#pragma clang fp contract(off)
  constexpr int LD = LMAX + 1;
  extern __shared__ double qem_lds[];
  double *A = qem_lds, *sv = A + LMAX * LD, *sq = sv + LMAX, *al = sq + LMAX, *be = al + LMAX, *ph = be + LMAX, *red = ph + LMAX;
  const long long b = list[blockIdx.x];
  const int t = threadIdx.x, i = t & 127, hf = t >> 7, lane = t & 63, wf = t >> 6;
  const int first = boff[b], L = boff[b + 1] - first;
  if (L < QEM_MIN || L > LMAX || L > cap) return;  // (never: the host lists these lengths alone and picks LMAX from them)
  double *r = rep + QE_REPORT * b, *Tb = T + 2 * (long long)cap * b;
  const bool mine = hf == 0 && i < L;  // the thread of row i in the sums over the block
  for (int k = t; k < L * LD; k += 256) A[k] = 0.0;
  __syncthreads();
  if (mine) {
    const int row = first + i;
    for (int k = Q.ptr[row], e = Q.ptr[row + 1]; k < e; k++) {
      const int c = Q.col[k] - first;
      if (c >= 0 && c < L) A[i * LD + c] = Q.val[k];
    }
  }
  __syncthreads();
  double g = __builtin_inf();
  if (mine) {
    double off = 0.0;
    for (int j = 0; j < L; j++)
      if (j != i) off = off + fabs(A[i * LD + j]);
    g = A[i * LD + i] - off;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) g = eig::nan_min(g, __shfl_xor(g, o));
  g = __shfl(g, 0);
  if (lane == 0) red[wf] = g;
  __syncthreads();
  g = eig::nan_min(eig::nan_min(eig::nan_min(red[0], red[1]), red[2]), red[3]);
  double theta = eps2;
  bool skipped = false;
  if (bfgs) {
    const double sQs = bfgs[QV_REPORT * b + 1];
    if (sQs < theta && sQs >= 0.0) theta = sQs;
    skipped = bfgs[QV_REPORT * b + 7] >= 2.0;
  }
  if (flr) theta = flr[b];
  const int outcome = skipped ? 6 : g >= theta ? 0 : -1;
  if (t == 0) {
    r[0] = g, r[1] = theta;
    for (int w = 2; w < QE_REPORT - 1; w++) r[w] = 0.0;
    r[QE_REPORT - 1] = (double)outcome;
  }
  if (outcome >= 0) {  // (uniform over the workgroup)
    for (int k = t; k < 2 * cap; k += 256) Tb[k] = 0.0;
    return;
  }
  __syncthreads();  // (red is read: the steps write it again)
  for (int k = 0; k + 2 < L; k++) {
    const bool in = i > k && i < L;
    const double x = in ? A[i * LD + k] : 0.0, x0 = A[(k + 1) * LD + k];
    if (hf == 0) {  // (uniform over a wavefront)
      double tail = i > k + 1 ? fabs(x) : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) tail = eig::nan_max(tail, __shfl_xor(tail, o));
      tail = __shfl(tail, 0);
      const double s = kktdev::wave_sum(x * x);
      if (lane == 0) red[wf] = tail, red[4 + wf] = s;
    }
    __syncthreads();
    if (eig::nan_max(red[0], red[1]) == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
      if (t == 0) be[k] = x0;
      __syncthreads();  // (red is read)
      continue;
    }
    const double ss = red[4] + red[5];
    const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
    const double v = i == k + 1 ? x - beta : x;
    const double h = ss - x0 * beta;
    if (mine) sv[i] = v;
    __syncthreads();
    const int nt = L - k - 1, mid = k + 1 + ((nt + 1) >> 1);
    const int j0 = hf ? mid : k + 1, j1 = hf ? L : mid;
    double p = 0.0;
    if (in) {
      for (int j = j0; j < j1; j++) p = __fma_rn(A[i * LD + j], sv[j], p);
      if (hf) ph[i] = p;
    }
    __syncthreads();
    if (hf == 0) {
      if (in) p = (p + ph[i]) / h;
      const double s = kktdev::wave_sum(v * p);
      if (lane == 0) red[wf] = s;
    }
    __syncthreads();
    const double c = (red[0] + red[1]) / (h + h);
    if (mine) sq[i] = p - c * v;
    __syncthreads();
    if (in) {
      const double vi = sv[i], qi = sq[i];
      for (int j = j0; j < j1; j++) A[i * LD + j] = A[i * LD + j] - (vi * sq[j] + qi * sv[j]);
    }
    if (t == 0) be[k] = beta;
    __syncthreads();
  }
  if (mine) al[i] = A[i * LD + i];
  if (t == 0) be[L - 2] = A[(L - 1) * LD + L - 2], be[L - 1] = 0.0;
  __syncthreads();
  for (int k = t; k < 2 * cap; k += 256) Tb[k] = k < L ? al[k] : (k >= cap && k - cap < L) ? be[k - cap] : 0.0;
}

__global__ void __launch_bounds__(64) k_qem_ritz(const int *__restrict__ list, const int *__restrict__ boff, const int *__restrict__ didx,
                                                 double *vals, int cap, const double *T, double *rep) {
#pragma clang fp contract(off)
  __shared__ eig::RitzLds lds;
  const long long b = list[blockIdx.x];
  const int lane = threadIdx.x, first = boff[b], L = boff[b + 1] - first;
  double *r = rep + QE_REPORT * b;
  if (L < QEM_MIN || L > QEM_MAX || L > cap || r[QE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 6: decided by k_qem_block)
  const double *al = T + 2 * (long long)cap * b;
  eig::ritz(al, al + cap, L, r[1], r, lds);
  __syncthreads();
  const double d = r[7];
  if (d == 0.0) return;
  for (int row = lane; row < L; row += 64) {
    const int k = didx[first + row];
    vals[k] = vals[k] + d;
  }
}

}  // namespace qv
