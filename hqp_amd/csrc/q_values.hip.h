// gfx950 kernels of the entries that read and write the sparse Q of the program where it lies on the device
// (hqpkkt_q_product .. hqpkkt_q_dscale_update, hqpkkt_lagrangian_gradient; include/hqpkkt.h): the Hessian approximations
// of the reference that work on Hqp_Program::Q itself - Hqp_HL::init, Hqp_HL_Gerschgorin, Hqp_HL_DScale - and grd_L of
// Hqp_SqpSolver.  They serve all three modes: the values are the handle's Qx | Ax | Cx (TreeDev::vals), the rows those of
// the symmetric image Qf and of the transposed copies AT, CT.  Of Q only the stored entries with col >= row exist: the
// image is built from them, and the per-entry table `kind` (the row of a diagonal entry, QV_UPPER, QV_LOWER) keeps every
// write away from the others.
// Plain loads and stores in the handle's stream: no polled words, no waits between workgroups, no atomics.  The kernels
// whose operations are promised to be rounded one by one are compiled without contraction and written with the
// operators (staged_hess_bfgs.hip.h says why __dmul_rn is not enough); sums that may fuse say so with __fma_rn.
// Included by q_entries.hip, which has the host code of these entries.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.hip.h"

namespace qv {

static const int QV_UPPER = -1, QV_LOWER = -2;  // `kind` of a stored entry that is no diagonal entry
static const int QV_CHUNK = 4096;               // entries of a block that one unit sums
static const int QV_REPORT = 8;                 // (HQPKKT_DSCALE_REPORT)

// ---------------------------------------------------------------- rows of Qf
// LPR lanes share a row: lane `sub` takes the entries sub, sub + LPR, .. in ascending order, the lanes add up by
// kktdev::row_sum - an order that the row's length and LPR fix.  STATS: the sum of |q_ij|, j != i, and the stored
// diagonal straight from vals (didx: its index there, -1 without one); otherwise y = Q x by fused multiply-adds.
// (No lane leaves before row_sum: a lane past n walks no entry.)
template <int LPR, bool STATS>
__global__ void __launch_bounds__(256) k_qv_rows(int n, kktdev::CsrDev Q, const double *__restrict__ x, double *__restrict__ y,
                                                 const int *__restrict__ didx, const double *__restrict__ vals, double *__restrict__ diag) {
  const int sub = threadIdx.x & (LPR - 1);
  const long long row = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = row < n;
  const int e = live ? Q.ptr[row + 1] : 0;
  double s = 0.0;
  for (int k = live ? Q.ptr[row] + sub : 0; k < e; k += LPR) {
    const int c = Q.col[k];
    const double v = Q.val[k];
    if (STATS) {
      if (c != row) s += fabs(v);
    } else
      s = __fma_rn(v, x[c], s);
  }
  s = kktdev::row_sum<LPR>(s);
  if (!live || sub != 0) return;
  if (y) y[row] = s;
  if (STATS && diag) diag[row] = didx[row] >= 0 ? vals[didx[row]] : 0.0;
}

// ---------------------------------------------------------------- grad L
// out = c - (A'y + C'z) [- minus] (Hqp_SqpSolver::grd_L): a lane's share of row i of AT, then its share of row i of CT,
// one accumulator, fused multiply-adds in ascending order; the lanes by row_sum; the subtractions rounded one by one.
template <int LPR>
__global__ void __launch_bounds__(256) k_qv_grad_l(int n, kktdev::CsrDev AT, kktdev::CsrDev CT, const double *__restrict__ c,
                                                   const double *__restrict__ y, const double *__restrict__ z,
                                                   const double *__restrict__ minus, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int sub = threadIdx.x & (LPR - 1);
  const long long row = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = row < n;
  double t = 0.0;
  if (live) {
    for (int k = AT.ptr[row] + sub, e = AT.ptr[row + 1]; k < e; k += LPR) t = __fma_rn(AT.val[k], y[AT.col[k]], t);
    for (int k = CT.ptr[row] + sub, e = CT.ptr[row + 1]; k < e; k += LPR) t = __fma_rn(CT.val[k], z[CT.col[k]], t);
  }
  t = kktdev::row_sum<LPR>(t);
  if (!live || sub != 0) return;
  double g = c[row] - t;
  if (minus) g = g - minus[row];
  out[row] = g;
}

// ---------------------------------------------------------------- writes by entry
// A thread per stored entry of Q.  setup = 0 (hqpkkt_q_set_diagonal): upper off-diagonals <- +0.0, q_ii <- d_i;
// setup = 1 (Hqp_HL_DScale::setup): upper off-diagonals <- +0.0, q_ii <- max(q_ii, eps), the reference's macro.
__global__ void __launch_bounds__(256) k_qv_reset(int nq, const int *__restrict__ kind, double *__restrict__ vals,
                                                  const double *__restrict__ d, double eps, int setup) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nq) return;
  const int r = kind[k];
  if (r == QV_UPPER)
    vals[k] = 0.0;
  else if (r >= 0) {
    const double q = vals[k];
    vals[k] = setup ? (q > eps ? q : eps) : d[r];
  }
}

// Hqp_HL_Gerschgorin::update behind the row pass: q_ii <- max(q_ii, fl(offsum_i + eps)); the diagonal entries alone
__global__ void __launch_bounds__(256) k_qv_gerschgorin(int n, const int *__restrict__ didx, const double *__restrict__ offsum,
                                                        double eps, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double t = offsum[i] + eps;
  const double q = vals[didx[i]];
  vals[didx[i]] = q > t ? q : t;
}

// ---------------------------------------------------------------- sums of a block
// A block's sums (Hqp_HL_DScale::update, Hqp_HL_BFGS, the eigenvalue control; the passes are in q_bfgs.hip.h and
// q_eigen.hip.h) are made of its chunks of QV_CHUNK entries, counted from its first index: a unit each.  One unit's sum:
// thread t of 256 takes the entries t, t + 256, .. by fused multiply-adds, kktdev::wave_sum, the four wavefronts in order.
// WPU = 4: a workgroup per unit.  WPU = 1 (no block longer than 64): a wavefront per unit, four units a workgroup - the
// entries sit in the lanes they have as the first wavefront of a workgroup, and the three sums that a workgroup's other
// wavefronts would bring are the zeros added here, so the bits are those of WPU = 4.
template <int WPU>
__device__ __forceinline__ double ds_unit_sum(double a, double *red) {
  a = kktdev::wave_sum(a);
  if (WPU == 1) return ((a + 0.0) + 0.0) + 0.0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
// a block's sum: its units' partials added in ascending order
__device__ __forceinline__ double ds_block_sum(long long len, const double *__restrict__ p, int stride) {
  const long long nch = (len + QV_CHUNK - 1) / QV_CHUNK;
  double a = p[0];
  for (long long j = 1; j < nch; j++) a += p[j * stride];
  return a;
}

// ---------------------------------------------------------------- Hqp_HL_DScale::update
// Block b: the variables [b B, min((b + 1) B, n)).  Sums, decision, v and outcome are k_qb_sums .. k_qb_outcome
// (q_bfgs.hip.h) over that partition's plan; rep[8 b ..]: sy, sqs, gamma, theta, sv, first index, length, outcome.
// the update, a thread per variable: q_i <- fl(q_i - fl(fl(sq_i sq_i) / sqs)), then q_i <- fl(q_i + fl(fl(v_i v_i) / sv)),
// v_i formed again by the operations of pass 2.  Divisions, as in the reference.  The damping of a block that is then
// left alone (outcome 2, 3) is the one place theta says more than the outcome: rep[3] != 1 there.  The partition is
// uniform by definition, so a variable finds its block by a division - no table is loaded.
__global__ void __launch_bounds__(256) k_qv_ds_apply(int n, int B, const int *__restrict__ didx, const double *__restrict__ s,
                                                     const double *__restrict__ y, const double *__restrict__ rep, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *r = rep + QV_REPORT * (i / B);
  const int outcome = (int)r[7];
  if (outcome >= 2) return;
  const double sqs = r[1], theta = r[3], sv = r[4];
  double q = vals[didx[i]];
  const double sq = s[i] * q;
  double vi = y[i];
  if (outcome == 1) {
    const double omt = 1.0 - theta;
    vi = theta * y[i] + omt * sq;
  }
  q = q - (sq * sq) / sqs;
  q = q + (vi * vi) / sv;
  vals[didx[i]] = q;
}

}  // namespace qv
