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
// Included by hqpkkt.hip.
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

// ---------------------------------------------------------------- Hqp_HL_DScale::update
// Block b: the variables [b B, min((b + 1) B, n)).  A block's sums are made of its chunks of QV_CHUNK entries, counted
// from its first index; unit u = b cpb + j is chunk j of block b (the last block's units past its end are empty and never
// read).  One unit's sum: thread t of 256 takes the entries t, t + 256, .. by fused multiply-adds, kktdev::wave_sum, the
// four wavefronts in order.  WPU = 4: a workgroup per unit.  WPU = 1 (B <= 64 alone): a wavefront per unit, four units a
// workgroup - the entries sit in the lanes they have as the first wavefront of a workgroup, and the three sums that a
// workgroup's other wavefronts would bring are the zeros added here, so the bits are those of WPU = 4.
struct DsGeom {
  int n, B, cpb, nblocks;
  long long nunits;
};
__device__ __forceinline__ void ds_unit(const DsGeom &g, long long u, long long &first, long long &end) {
  const long long b = u / g.cpb, j = u % g.cpb;
  const long long blk_end = (b + 1) * g.B < g.n ? (b + 1) * g.B : g.n;
  first = b * g.B + j * QV_CHUNK;
  end = first + QV_CHUNK < blk_end ? first + QV_CHUNK : blk_end;
}
template <int WPU>
__device__ __forceinline__ double ds_unit_sum(double a, double *red) {
  a = kktdev::wave_sum(a);
  if (WPU == 1) return ((a + 0.0) + 0.0) + 0.0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// pass 1: part[2 u] = sum s_i y_i, part[2 u + 1] = sum sq_i s_i with sq_i = fl(s_i q_i)
template <int WPU>
__global__ void __launch_bounds__(256) k_qv_ds_sums(DsGeom g, const int *__restrict__ didx, const double *__restrict__ vals,
                                                    const double *__restrict__ s, const double *__restrict__ y, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const long long u = WPU == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  const int t = WPU == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x, stride = WPU == 1 ? 64 : 256;
  double a = 0.0, b = 0.0;
  if (u < g.nunits) {
    long long first, end;
    ds_unit(g, u, first, end);
    for (long long i = first + t; i < end; i += stride) {
      const double si = s[i];
      const double sq = si * vals[didx[i]];
      a = __fma_rn(si, y[i], a);
      b = __fma_rn(sq, si, b);
    }
  }
  a = ds_unit_sum<WPU>(a, red), b = ds_unit_sum<WPU>(b, red);
  if (t == 0 && u < g.nunits) part[2 * u] = a, part[2 * u + 1] = b;
}

// a block's sum: its units' partials added in ascending order
__device__ __forceinline__ double ds_block_sum(long long len, const double *__restrict__ p, int stride) {
  const long long nch = (len + QV_CHUNK - 1) / QV_CHUNK;
  double a = p[0];
  for (long long j = 1; j < nch; j++) a += p[j * stride];
  return a;
}
// the decision, a thread per block: damped where sy < fl(gamma sqs), theta = fl(fl((1 - gamma) sqs) / fl(sqs - sy)).
// rep[8 b ..]: sy, sqs, gamma, theta, sv (sy so far), first index, length, 1 where damped (k_qv_ds_outcome ends 4 and 7)
__global__ void __launch_bounds__(256) k_qv_ds_decide(DsGeom g, const double *__restrict__ part, double gamma, double *__restrict__ rep) {
#pragma clang fp contract(off)
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  const long long first = b * g.B, end = (b + 1) * g.B < g.n ? (b + 1) * g.B : g.n;
  const double *p = part + 2 * b * g.cpb;
  const double sy = ds_block_sum(end - first, p, 2), sqs = ds_block_sum(end - first, p + 1, 2);
  const bool damp = sy < gamma * sqs;  // (false where a sum is NaN)
  double theta = 1.0;
  if (damp) theta = ((1.0 - gamma) * sqs) / (sqs - sy);
  double *r = rep + QV_REPORT * b;
  r[0] = sy, r[1] = sqs, r[2] = gamma, r[3] = theta, r[4] = sy, r[5] = (double)first, r[6] = (double)(end - first), r[7] = damp ? 1.0 : 0.0;
}

// pass 2: on a damped block v_i = fl(fl(theta y_i) + fl((1 - theta) sq_i)) and part2[u] = sum s_i v_i in the order of
// pass 1; v (optional) as applied: y where the block is not damped
template <int WPU>
__global__ void __launch_bounds__(256) k_qv_ds_damped(DsGeom g, const int *__restrict__ didx, const double *__restrict__ vals,
                                                      const double *__restrict__ s, const double *__restrict__ y,
                                                      const double *__restrict__ rep, double *__restrict__ part2, double *__restrict__ v) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const long long u = WPU == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  const int t = WPU == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x, stride = WPU == 1 ? 64 : 256;
  double c = 0.0;
  if (u < g.nunits) {
    long long first, end;
    ds_unit(g, u, first, end);
    const double *r = rep + QV_REPORT * (u / g.cpb);
    const bool damp = r[7] == 1.0;
    const double theta = r[3], omt = 1.0 - theta;
    if (damp)
      for (long long i = first + t; i < end; i += stride) {
        const double si = s[i];
        const double sq = si * vals[didx[i]];
        const double vi = theta * y[i] + omt * sq;
        if (v) v[i] = vi;
        c = __fma_rn(si, vi, c);
      }
    else if (v)
      for (long long i = first + t; i < end; i += stride) v[i] = y[i];
  }
  c = ds_unit_sum<WPU>(c, red);
  if (t == 0 && u < g.nunits) part2[u] = c;
}

// the outcome, a thread per block: sv = the sum of pass 2 on a damped block, sy otherwise; 0 updated, 1 updated with
// damping, 2 left alone (sv or sqs zero), 3 left alone (sv or sqs not finite)
__global__ void __launch_bounds__(256) k_qv_ds_outcome(DsGeom g, const double *__restrict__ part2, double *__restrict__ rep) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  double *r = rep + QV_REPORT * b;
  const bool damp = r[7] == 1.0;
  const double sqs = r[1];
  double sv = r[0];
  if (damp) sv = ds_block_sum((long long)r[6], part2 + b * g.cpb, 1);
  int outcome = damp ? 1 : 0;
  if (!isfinite(sv) || !isfinite(sqs))
    outcome = 3;
  else if (sv == 0.0 || sqs == 0.0)
    outcome = 2;
  r[4] = sv, r[7] = (double)outcome;
}

// the update, a thread per variable: q_i <- fl(q_i - fl(fl(sq_i sq_i) / sqs)), then q_i <- fl(q_i + fl(fl(v_i v_i) / sv)),
// v_i formed again by the operations of pass 2.  Divisions, as in the reference.  The damping of a block that is then
// left alone (outcome 2, 3) is the one place theta says more than the outcome: rep[3] != 1 there.
__global__ void __launch_bounds__(256) k_qv_ds_apply(DsGeom g, const int *__restrict__ didx, const double *__restrict__ s,
                                                     const double *__restrict__ y, const double *__restrict__ rep, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.n) return;
  const double *r = rep + QV_REPORT * (i / g.B);
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
