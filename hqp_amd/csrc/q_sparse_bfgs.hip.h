// gfx950 kernels of hqpkkt_q_sparse_bfgs_update (include/hqpkkt.h): the reference's Hqp_HL_SparseBFGS - the damped BFGS
// update of every diagonal block of Q after a permutation that makes the blocks contiguous - on the sparse Q where it lies
// on the device.  The blocks are the connected components of Q's graph (hqpkkt_q_components); their variables lie anywhere.
// The plan (the BfgsPlan of key QB_COMPONENTS) puts them in BLOCK ORDER once, on the host:
//   member[p]  the variable at position p: block after block, ascending inside a block
//   pos_of[i]  the position of variable i                   blk_of[i]  the block of variable i
//   boff / bunit / ublk  as in q_bfgs.hip.h, counted in positions
// In positions the partition is one of contiguous ranges, so the unit passes of q_bfgs.hip.h (k_qb_sums, k_qb_damped,
// k_qb_outcome) run unchanged on vectors that lie in block order, and a block's sums are ds_unit_sum / ds_block_sum over its
// own positions: its bits depend on its length, its values and the order of its members alone.  What is new here is the
// way into that order and out of it, each indirection taken once per call and not once per pass:
//   k_qsb_pack     s, y -> block order: a thread per position, one scattered read and one coalesced write each
//   k_qsb_rows     (Q s)_i over row i of the symmetric image, written to position pos_of[i]
//   k_qsb_decide   the decision per block with Hqp_HL_SparseBFGS's clamp of theta to [0, 1]
//   k_qsb_apply    the two steps of every stored entry, Q s and v read through pos_of
//   k_qsb_unpack   v and Q s back into the caller's order where they are asked for
// Plain loads and stores in the handle's stream: no polled words, no waits between workgroups, no atomics.  Operations
// that are promised to be rounded one by one stand in kernels without contraction; sums that may fuse say __fma_rn.
// Included by q_entries.hip behind q_bfgs.hip.h.
#pragma once
#include "q_bfgs.hip.h"

namespace qv {

// a thread per position p: sp[p] = s[member[p]], yp[p] = y[member[p]].  Consecutive positions of a block are ascending
// variables, so a wavefront's reads of an interleaved block are strided and its writes one line.
__global__ void __launch_bounds__(256) k_qsb_pack(int n, const int *__restrict__ member, const double *__restrict__ s,
                                                  const double *__restrict__ y, double *__restrict__ sp, double *__restrict__ yp) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int i = member[p];
  sp[p] = s[i], yp[p] = y[i];
}

// yp[pos_of[i]] = sum of q_ij x_j over row i of Qf: the walk, the lanes and the order of k_qv_rows, x in the caller's order
// (one scattered read an entry either way), the result where the unit passes read it in a line.  No entry is skipped and
// none has to be: Qf is the image of the stored entries with col >= row, and each of them joins its two ends in one
// component - a row of Qf IS its row of the component's block.  (No lane leaves before row_sum.)
template <int LPR>
__global__ void __launch_bounds__(256) k_qsb_rows(int n, kktdev::CsrDev Q, const int *__restrict__ pos_of, const double *__restrict__ x,
                                                  double *__restrict__ yp) {
  const int sub = threadIdx.x & (LPR - 1);
  const long long row = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = row < n;
  const int e = live ? Q.ptr[row + 1] : 0;
  double s = 0.0;
  for (int k = live ? Q.ptr[row] + sub : 0; k < e; k += LPR) s = __fma_rn(Q.val[k], x[Q.col[k]], s);
  s = kktdev::row_sum<LPR>(s);
  if (live && sub == 0) yp[pos_of[row]] = s;
}

// the decision, a thread per block, as k_qb_decide with the reference's clamp (Hqp_HL_SparseBFGS::update_b_Q): damped where
// sy < fl(gamma sQs), theta = fl(fl((1 - gamma) sQs) / fl(sQs - sy)), then theta = 1 unless theta <= 1, then theta = 0 unless
// theta >= 0 - in this order, so a NaN becomes 1.  A block that is damped with theta = 1 is still reported damped.
// rep[8 b ..]: sy, sQs, gamma, theta, sv (sy so far), the block's smallest variable, length, 1 where damped (k_qb_outcome
// ends 4 and 7)
__global__ void __launch_bounds__(256) k_qsb_decide(BfgsTables g, const int *__restrict__ member, const double *__restrict__ part, double gamma,
                                                    double *__restrict__ rep) {
#pragma clang fp contract(off)
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  const int first = g.boff[b], len = g.boff[b + 1] - first;
  const double *p = part + 2 * (long long)g.bunit[b];
  const double sy = ds_block_sum(len, p, 2), sqs = ds_block_sum(len, p + 1, 2);
  const bool damp = sy < gamma * sqs;  // (false where a sum is NaN)
  double theta = 1.0;
  if (damp) {
    theta = ((1.0 - gamma) * sqs) / (sqs - sy);
    if (!(theta <= 1.0)) theta = 1.0;
    if (!(theta >= 0.0)) theta = 0.0;
  }
  double *r = rep + QV_REPORT * b;
  r[0] = sy, r[1] = sqs, r[2] = gamma, r[3] = theta, r[4] = sy, r[5] = (double)member[first], r[6] = (double)len, r[7] = damp ? 1.0 : 0.0;
}

// the update, a thread per stored entry k = (i, j) of Qx with j >= i - both ends lie in one component -: where that block is
// updated, q <- fl(q - fl(fl((Qs)_i (Qs)_j) / sQs)), then q <- fl(q + fl(fl(v_i v_j) / sv)), the operations of k_qb_apply with
// Q s and v read at the positions of i and j.  Entries with col < row are neither read nor written.
__global__ void __launch_bounds__(256) k_qsb_apply(int nq, const int *__restrict__ erow, const int *__restrict__ ecol,
                                                   const int *__restrict__ kind, const int *__restrict__ blk_of,
                                                   const int *__restrict__ pos_of, const double *__restrict__ Qsp,
                                                   const double *__restrict__ vp, const double *__restrict__ rep, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nq) return;
  if (kind[k] == QV_LOWER) return;
  const int i = erow[k];
  const double *r = rep + QV_REPORT * (long long)blk_of[i];
  if ((int)r[7] >= 2) return;
  const int pi = pos_of[i], pj = pos_of[ecol[k]];
  const double sqs = r[1], sv = r[4];
  double q = vals[k];
  q = q - (Qsp[pi] * Qsp[pj]) / sqs;
  q = q + (vp[pi] * vp[pj]) / sv;
  vals[k] = q;
}

// a thread per position: v and Q s of block order into the caller's order, either where it is asked for
__global__ void __launch_bounds__(256) k_qsb_unpack(int n, const int *__restrict__ member, const double *__restrict__ vp,
                                                    const double *__restrict__ Qsp, double *__restrict__ v, double *__restrict__ Qs) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int i = member[p];
  if (v) v[i] = vp[p];
  if (Qs) Qs[i] = Qsp[p];
}

}  // namespace qv
