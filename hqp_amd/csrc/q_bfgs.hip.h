// gfx950 kernels of hqpkkt_q_bfgs_update and of the passes of hqpkkt_q_dscale_update (include/hqpkkt.h): the reference's
// default Hessian approximation Hqp_HL_BFGS - the damped BFGS update of every diagonal block of Hqp_Program::Q - on the
// sparse Q where it lies on the device, and with it the update on the stored entries of a block alone (the operator of
// Hqp_HL_Gangster).  The blocks are a partition of the variables into contiguous ranges of ANY lengths (hqpkkt_q_blocks),
// handed over as tables:
//   blk_of[i]  the block of variable i                      boff[b]   the first index of block b, n behind the last
//   bunit[b]   the first unit of block b, nunits behind     ublk[u]   the block of unit u
//   erow[k], ecol[k]  row and column of stored entry k of Qx (kind[k] as in q_values.hip.h)
// Unit bunit[b] + j is chunk j of block b: QV_CHUNK entries counted from the block's first index.  A unit's sum and a
// block's sum are ds_unit_sum and ds_block_sum (q_values.hip.h), so a block's bits depend on its length alone - not on
// where it lies, on the other blocks, on the grid or on the mode.
// Hqp_HL_DScale::update is the same damped update of a Q that is its diagonal: its sums, decision and outcome are the
// passes here over the plan of its uniform partition, with (Q s)_i = fl(s_i q_ii) formed in registers (DIAG) where the
// BFGS update loads the vector Q s; its own kernel is the write of the diagonal alone (k_qv_ds_apply).
// Plain loads and stores in the handle's stream: no polled words, no waits between workgroups, no atomics.  Operations
// that are promised to be rounded one by one stand in kernels without contraction; sums that may fuse say __fma_rn.
// Included by q_entries.hip behind q_values.hip.h.
#pragma once
#include "q_values.hip.h"

namespace qv {

struct BfgsTables {
  int n, nblocks, nunits;
  const int *blk_of, *boff, *bunit, *ublk;
};
__device__ __forceinline__ void qb_unit(const BfgsTables &g, int u, int &b, int &first, int &end) {
  b = g.ublk[u];
  first = g.boff[b] + (u - g.bunit[b]) * QV_CHUNK;
  const int blk_end = g.boff[b + 1];
  end = blk_end - first > QV_CHUNK ? first + QV_CHUNK : blk_end;
}
// The range of unit u in a unit pass.  DIAG (Hqp_HL_DScale): the partition is uniform by definition - blocks of B, the
// last one shorter - and the plan numbers its units b cpb + j, since only the last block can have fewer than cpb.  So a
// unit finds its range by division, as k_qv_ds_apply finds a variable's block: the chain of table loads (ublk, then boff
// and bunit) that would stand before a unit's first entry costs a block of 10^6 variables 5 % of the call.
template <bool DIAG>
__device__ __forceinline__ void qb_pass_unit(const BfgsTables &g, int B, int u, int &b, int &first, int &end) {
  if (!DIAG) return qb_unit(g, u, b, first, end);
  const int cpb = (B + QV_CHUNK - 1) / QV_CHUNK;
  b = u / cpb;
  const int b0 = b * B;
  first = b0 + (u - b * cpb) * QV_CHUNK;
  const int blk_end = g.n - b0 > B ? b0 + B : g.n;
  end = blk_end - first > QV_CHUNK ? first + QV_CHUNK : blk_end;
}

// y_i = sum of q_ij x_j over the entries of row i of Qf whose column lies in the block of i: the walk, the lanes and the
// order of k_qv_rows - an entry of another block keeps its place in its lane's turn and adds nothing, so where no entry
// crosses a block the bits are those of hqpkkt_q_product.  (No lane leaves before row_sum.)
template <int LPR>
__global__ void __launch_bounds__(256) k_qb_rows(int n, kktdev::CsrDev Q, const int *__restrict__ blk_of, const double *__restrict__ x,
                                                 double *__restrict__ y) {
  const int sub = threadIdx.x & (LPR - 1);
  const long long row = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = row < n;
  const int e = live ? Q.ptr[row + 1] : 0;
  const int b = live ? blk_of[row] : -1;
  double s = 0.0;
  for (int k = live ? Q.ptr[row] + sub : 0; k < e; k += LPR) {
    const int c = Q.col[k];
    if (blk_of[c] == b) s = __fma_rn(Q.val[k], x[c], s);
  }
  s = kktdev::row_sum<LPR>(s);
  if (live && sub == 0) y[row] = s;
}

// (Q s)_i of a pass.  DIAG = false: src is the vector Q s (k_qb_rows).  DIAG = true: Q is its diagonal, src the handle's
// values and didx the diagonals' indices there - fl(s_i q_ii), one rounded product, never stored; B is the block length
// of its uniform partition (not read otherwise).
template <bool DIAG>
__device__ __forceinline__ double qb_qs(const double *__restrict__ src, const int *__restrict__ didx, int i, double si) {
#pragma clang fp contract(off)
  return DIAG ? si * src[didx[i]] : src[i];
}

// pass 1: part[2 u] = sum s_i y_i, part[2 u + 1] = sum s_i (Qs)_i over unit u.  One unit's sum: thread t takes the
// entries t, t + stride, .. by fused multiply-adds, then ds_unit_sum.  WPU = 1 where every block of the plan is at most
// 64 long.
template <int WPU, bool DIAG>
__global__ void __launch_bounds__(256) k_qb_sums(BfgsTables g, const double *__restrict__ s, const double *__restrict__ y,
                                                 const double *__restrict__ src, const int *__restrict__ didx, int B, double *__restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const long long u = WPU == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  const int t = WPU == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x, stride = WPU == 1 ? 64 : 256;
  double a = 0.0, c = 0.0;
  if (u < g.nunits) {
    int b, first, end;
    qb_pass_unit<DIAG>(g, B, (int)u, b, first, end);
    for (int i = first + t; i < end; i += stride) {
      const double si = s[i];
      a = __fma_rn(si, y[i], a);
      c = __fma_rn(si, qb_qs<DIAG>(src, didx, i, si), c);
    }
  }
  a = ds_unit_sum<WPU>(a, red), c = ds_unit_sum<WPU>(c, red);
  if (t == 0 && u < g.nunits) part[2 * u] = a, part[2 * u + 1] = c;
}

// the decision, a thread per block: damped where sy < fl(gamma sQs), theta = fl(fl((1 - gamma) sQs) / fl(sQs - sy)); theta is
// not clamped.  rep[8 b ..]: sy, sQs, gamma_eff, theta, sv (sy so far), first index, length, 1 where damped (k_qb_outcome
// ends 4 and 7)
__global__ void __launch_bounds__(256) k_qb_decide(BfgsTables g, const double *__restrict__ part, double gamma, double *__restrict__ rep) {
#pragma clang fp contract(off)
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  const int first = g.boff[b], len = g.boff[b + 1] - first;
  const double *p = part + 2 * (long long)g.bunit[b];
  const double sy = ds_block_sum(len, p, 2), sqs = ds_block_sum(len, p + 1, 2);
  const bool damp = sy < gamma * sqs;  // (false where a sum is NaN)
  double theta = 1.0;
  if (damp) theta = ((1.0 - gamma) * sqs) / (sqs - sy);
  double *r = rep + QV_REPORT * b;
  r[0] = sy, r[1] = sqs, r[2] = gamma, r[3] = theta, r[4] = sy, r[5] = (double)first, r[6] = (double)len, r[7] = damp ? 1.0 : 0.0;
}

// pass 2: v_i = fl(fl(theta y_i) + fl(fl(1 - theta) (Qs)_i)) on a damped block and part2[u] = sum s_i v_i in the order of
// pass 1; v_i = y_i on the others.  DIAG = false: v is the handle's own vector, k_qb_apply reads it.  DIAG = true: v is
// the caller's and optional - k_qv_ds_apply forms v_i again.
template <int WPU, bool DIAG>
__global__ void __launch_bounds__(256) k_qb_damped(BfgsTables g, const double *__restrict__ s, const double *__restrict__ y,
                                                   const double *__restrict__ src, const int *__restrict__ didx, int B,
                                                   const double *__restrict__ rep, double *__restrict__ part2, double *__restrict__ v) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const long long u = WPU == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  const int t = WPU == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x, stride = WPU == 1 ? 64 : 256;
  double c = 0.0;
  if (u < g.nunits) {
    int b, first, end;
    qb_pass_unit<DIAG>(g, B, (int)u, b, first, end);
    const double *r = rep + QV_REPORT * (long long)b;
    const bool damp = r[7] == 1.0;
    const double theta = r[3], omt = 1.0 - theta;
    if (damp)
      for (int i = first + t; i < end; i += stride) {
        const double si = s[i];
        const double vi = theta * y[i] + omt * qb_qs<DIAG>(src, didx, i, si);
        if (!DIAG || v) v[i] = vi;
        c = __fma_rn(si, vi, c);
      }
    else if (!DIAG || v)
      for (int i = first + t; i < end; i += stride) v[i] = y[i];
  }
  c = ds_unit_sum<WPU>(c, red);
  if (t == 0 && u < g.nunits) part2[u] = c;
}

// the outcome, a thread per block: sv = the sum of pass 2 on a damped block, sy otherwise; 0 updated, 1 updated with
// damping, 2 left alone (sv or sQs zero), 3 left alone (sv or sQs not finite)
__global__ void __launch_bounds__(256) k_qb_outcome(BfgsTables g, const double *__restrict__ part2, double *__restrict__ rep) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  double *r = rep + QV_REPORT * b;
  const bool damp = r[7] == 1.0;
  const double sqs = r[1];
  double sv = r[0];
  if (damp) sv = ds_block_sum(g.boff[b + 1] - g.boff[b], part2 + g.bunit[b], 1);
  int outcome = damp ? 1 : 0;
  if (!isfinite(sv) || !isfinite(sqs))
    outcome = 3;
  else if (sv == 0.0 || sqs == 0.0)
    outcome = 2;
  r[4] = sv, r[7] = (double)outcome;
}

// the update, a thread per stored entry k = (i, j) of Qx: where j >= i and both lie in one block that is updated,
// q <- fl(q - fl(fl((Qs)_i (Qs)_j) / sQs)), then q <- fl(q + fl(fl(v_i v_j) / sv)).  Divisions, as in the reference.  Entries
// with col < row and entries across two blocks are neither read nor written.
__global__ void __launch_bounds__(256) k_qb_apply(int nq, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                  const int *__restrict__ kind, const int *__restrict__ blk_of,
                                                  const double *__restrict__ Qs, const double *__restrict__ v,
                                                  const double *__restrict__ rep, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nq) return;
  if (kind[k] == QV_LOWER) return;
  const int i = erow[k], j = ecol[k];
  const int b = blk_of[i];
  if (blk_of[j] != b) return;
  const double *r = rep + QV_REPORT * (long long)b;
  if ((int)r[7] >= 2) return;
  const double sqs = r[1], sv = r[4];
  double q = vals[k];
  q = q - (Qs[i] * Qs[j]) / sqs;
  q = q + (v[i] * v[j]) / sv;
  vals[k] = q;
}

}  // namespace qv
