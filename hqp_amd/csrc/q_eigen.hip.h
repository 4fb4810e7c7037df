// gfx950 kernels of hqpkkt_q_eigen_control (include/hqpkkt.h): the eigenvalue control at the end of Hqp_HL_BFGS::update_b_Q
// (hqp/Hqp_HL_BFGS.C:203-212, on by default there) on the blocks of the sparse Q where it lies on the device - per block
// of hqpkkt_q_blocks(bsize) a Lanczos recurrence for the smallest eigenvalue, all blocks in lockstep, and a shift of the
// block's diagonal up to its floor.  The rules are those of hqpkkt_eigen_control_stage_hessians (staged_hess_guard.hip.h);
// what differs is the geometry: there a workgroup has a whole stage, here a block may be 8 long or 10^6 long and one plan
// may mix both, so every sum of the recurrence is made per UNIT and then per block, as q_bfgs.hip.h makes its sums:
//   unit      QV_CHUNK entries from the block's first index; thread t of the unit takes its entries t, t + stride, .. by fused
//             multiply-adds in ascending order, then ds_unit_sum.  WPU = 1 (every block of the plan at most 64 long): a
//             wavefront per unit; WPU = 4: a workgroup of 256.
//   block     ds_block_sum over the block's units in ascending order.  A workgroup that needs its block's sum forms it
//             itself from the units' partials - one thread adds, the value is handed round (qe_bcast) - so a sum costs no
//             launch of its own, and every unit of a block gets the same bits.
// So a block's bits depend on its length and its values alone - not on where it lies, on the other blocks, on the grid
// or on the mode.  Plain loads and stores in the handle's stream: no polled words, no waits between workgroups, no
// atomics; nothing is read back inside the loop.  Operations that are promised to be rounded one by one stand in kernels
// without contraction; sums that may fuse say __fma_rn.
// The state of a block, QE_STATE doubles - done, steps, beta of the last step, max(|alpha|, beta) so far - is kept twice:
// step j reads copy j & 1 and k_qe_next writes copy (j + 1) & 1 (by the block's first unit alone), so that no unit reads a
// word another unit of its block writes in the same launch.
// Per step, behind the product w = Q v_j by k_qb_rows (unchanged): k_qe_alpha, k_qe_resid, k_qe_ortho, k_qe_next - four
// launches.  A block that is done costs a state test per unit.
// Included by q_entries.hip behind q_bfgs.hip.h.
#pragma once
#include "eigen_ritz.hip.h"
#include "q_bfgs.hip.h"

namespace qv {

static const int QE_STATE = 4;
static const int QE_REPORT = eig::REPORT;

// the unit of this wavefront (WPU = 1) or workgroup (WPU = 4), t the thread's index in it; false: none (WPU = 1 alone -
// a kernel of WPU = 1 has no barrier, its wavefronts are on their own)
template <int WPU>
__device__ __forceinline__ bool qe_unit(const BfgsTables &g, int &u, int &t, int &b, int &first, int &end) {
  const long long uu = WPU == 1 ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
  t = WPU == 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  if (uu >= g.nunits) return false;
  u = (int)uu;
  qb_unit(g, u, b, first, end);
  return true;
}
// thread 0's value to every thread of the unit
template <int WPU>
__device__ __forceinline__ double qe_bcast(double a, double *slot) {
  if (WPU == 1) return __shfl(a, 0);
  __syncthreads();
  if (threadIdx.x == 0) *slot = a;
  __syncthreads();
  return *slot;
}
// the unit's minimum, a NaN kept: a wavefront's butterfly, the four wavefronts in order
template <int WPU>
__device__ __forceinline__ double qe_unit_min(double a, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = eig::nan_min(a, __shfl_xor(a, o));
  if (WPU == 1) return a;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return eig::nan_min(eig::nan_min(eig::nan_min(red[0], red[1]), red[2]), red[3]);
}
static const int QE_STRIDE1 = 64, QE_STRIDE4 = 256;
#define QE_STRIDE (WPU == 1 ? QE_STRIDE1 : QE_STRIDE4)
#define QE_EPT (WPU == 1 ? 1 : QV_CHUNK / QE_STRIDE4)  // entries of a unit per thread

// The block-restricted row pass: offs_i = sum of |q_ij|, j != i, over the entries of row i of Qf whose column lies in the
// block of i - k_qb_rows' walk (hqpkkt_q_row_stats counts the entries across blocks as well).  A NaN stays in its row
// and in its image's row.
template <int LPR>
__global__ void __launch_bounds__(256) k_qe_rows(int n, kktdev::CsrDev Q, const int *__restrict__ blk_of, double *__restrict__ offs) {
  const int sub = threadIdx.x & (LPR - 1);
  const long long row = (long long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  const bool live = row < n;
  const int e = live ? Q.ptr[row + 1] : 0;
  const int b = live ? blk_of[row] : -1;
  double s = 0.0;
  for (int k = live ? Q.ptr[row] + sub : 0; k < e; k += LPR) {
    const int c = Q.col[k];
    if (c != row && blk_of[c] == b) s += fabs(Q.val[k]);
  }
  s = kktdev::row_sum<LPR>(s);
  if (live && sub == 0) offs[row] = s;
}

// per unit: partg[u] = min_i (q_ii - offs_i), a NaN kept; partf[u] = sum f_i^2, f_i = eig::start_entry(i - first index of
// the block)
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_unit0(BfgsTables g, const int *__restrict__ didx, const double *__restrict__ vals,
                                                  const double *__restrict__ offs, double *__restrict__ partg, double *__restrict__ partf) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  const int b0 = g.boff[b];
  double m = __builtin_inf(), a = 0.0;
  for (int i = first + t; i < end; i += QE_STRIDE) {
    m = eig::nan_min(m, vals[didx[i]] - offs[i]);
    const double f = eig::start_entry(i - b0);
    a = __fma_rn(f, f, a);
  }
  m = qe_unit_min<WPU>(m, red), a = ds_unit_sum<WPU>(a, red);
  if (t == 0) partg[u] = m, partf[u] = a;
}

// A thread per block, ahead of the recurrence.  g = min over the block's units in ascending order, Gerschgorin's lower
// bound of the block's spectrum; the floor theta: flr[b] where the host gave floors, else eps2 = fl(eps eps) - lowered to
// sQs where bfgs (the report words of the last k_qb_decide / k_qb_outcome with this plan) holds 0 <= sQs < eps2, the
// reference's rule.  With bfgs a block that update left alone (its outcome 2 or 3) is skipped: outcome 6, the reference's
// early return.  g >= theta: outcome 0, no shift.  Both are done; their share of the basis V stays 0 as the host cleared
// it.  Every other block is pending (-1).  The report and copy 0 of the state are written.
__global__ void __launch_bounds__(256) k_qe_begin(BfgsTables g, const double *__restrict__ partg, const double *__restrict__ flr, double eps2,
                                                  const double *__restrict__ bfgs, double *__restrict__ st, double *__restrict__ rep) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.nblocks) return;
  const int len = g.boff[b + 1] - g.boff[b], nch = (len + QV_CHUNK - 1) / QV_CHUNK;
  const double *p = partg + g.bunit[b];
  double gb = p[0];
  for (int j = 1; j < nch; j++) gb = eig::nan_min(gb, p[j]);
  double theta = eps2;
  bool skipped = false;
  if (bfgs) {
    const double sQs = bfgs[QV_REPORT * b + 1];
    if (sQs < theta && sQs >= 0.0) theta = sQs;
    skipped = bfgs[QV_REPORT * b + 7] >= 2.0;
  }
  if (flr) theta = flr[b];
  const int outcome = skipped ? 6 : gb >= theta ? 0 : -1;
  double *r = rep + QE_REPORT * b;
  r[0] = gb, r[1] = theta;
  for (int q = 2; q < QE_REPORT - 1; q++) r[q] = 0.0;
  r[QE_REPORT - 1] = (double)outcome;
  double *s = st + QE_STATE * b;
  s[0] = outcome < 0 ? 0.0 : 1.0, s[1] = 0.0, s[2] = 0.0, s[3] = 0.0;
}

// v_0 = f / sqrt(sum f_i^2) on the pending blocks
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_v0(BfgsTables g, const double *__restrict__ partf, const double *__restrict__ st, double *__restrict__ V) {
#pragma clang fp contract(off)
  __shared__ double slot;
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  if (st[QE_STATE * (long long)b] != 0.0) return;  // (uniform over the unit)
  const int b0 = g.boff[b];
  double nrm = 0.0;
  if (t == 0) nrm = sqrt(ds_block_sum(g.boff[b + 1] - b0, partf + g.bunit[b], 1));
  nrm = qe_bcast<WPU>(nrm, &slot);
  for (int i = first + t; i < end; i += QE_STRIDE) V[i] = eig::start_entry(i - b0) / nrm;
}

// step j, behind w = Q v_j: parta[u] = sum v_j w over unit u
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_alpha(BfgsTables g, const double *__restrict__ st, const double *__restrict__ vj,
                                                  const double *__restrict__ w, double *__restrict__ parta) {
  __shared__ double red[4];
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  if (st[QE_STATE * (long long)b] != 0.0) return;
  double a = 0.0;
  for (int i = first + t; i < end; i += QE_STRIDE) a = __fma_rn(vj[i], w[i], a);
  a = ds_unit_sum<WPU>(a, red);
  if (t == 0) parta[u] = a;
}

// alpha = v_j'w, the block's sum of parta; w <- fl(fl(w - fl(alpha v_j)) - fl(beta_{j-1} v_{j-1})), every operation rounded on
// its own; then the products of the new w against the whole basis, partc[cap u + q] = sum v_q w over the unit, q = 0 .. j
// (the basis vector q of all blocks lies at V + q n).  A thread keeps its entries of w in registers over the products.
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_resid(BfgsTables g, const double *__restrict__ st, const double *__restrict__ V, long long n, int j,
                                                  int cap, double *__restrict__ w, const double *__restrict__ parta, double *__restrict__ partc) {
#pragma clang fp contract(off)
  __shared__ double red[4], slot;
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  const double *s = st + QE_STATE * (long long)b;
  if (s[0] != 0.0) return;
  const double bprev = s[2];
  double alpha = 0.0;
  if (t == 0) alpha = ds_block_sum(g.boff[b + 1] - g.boff[b], parta + g.bunit[b], 1);
  alpha = qe_bcast<WPU>(alpha, &slot);
  const double *vj = V + (long long)j * n, *vp = V + (long long)(j > 0 ? j - 1 : 0) * n;
  double wr[QE_EPT];
#pragma unroll
  for (int e = 0; e < QE_EPT; e++) {
    const int i = first + t + e * QE_STRIDE;
    wr[e] = 0.0;
    if (i < end) {
      double x = w[i] - alpha * vj[i];
      if (j > 0) x = x - bprev * vp[i];
      w[i] = x, wr[e] = x;
    }
  }
  for (int q = 0; q <= j; q++) {
    const double *vq = V + (long long)q * n;
    double c = 0.0;
#pragma unroll
    for (int e = 0; e < QE_EPT; e++) {
      const int i = first + t + e * QE_STRIDE;
      if (i < end) c = __fma_rn(vq[i], wr[e], c);
    }
    c = ds_unit_sum<WPU>(c, red);
    if (t == 0) partc[(long long)cap * u + q] = c;
  }
}

// w made orthogonal to the whole basis once more: c_q = v_q'w, the block's sums of partc, taken off in ascending q, each
// product and difference rounded on its own; partb[u] = sum w^2 over the unit.  (Without this pass the recurrence grows a
// second copy of an eigenvalue a few steps after it has converged: k_he_step.)
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_ortho(BfgsTables g, const double *__restrict__ st, const double *__restrict__ V, long long n, int j,
                                                  int cap, double *__restrict__ w, const double *__restrict__ partc, double *__restrict__ partb) {
#pragma clang fp contract(off)
  __shared__ double red[4], cf[eig::MAX_STEPS];
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  if (st[QE_STATE * (long long)b] != 0.0) return;
  const double *pc = partc + (long long)cap * g.bunit[b];
  if (WPU != 1) {
    const int len = g.boff[b + 1] - g.boff[b];
    for (int q = t; q <= j; q += QE_STRIDE4) cf[q] = ds_block_sum(len, pc + q, cap);
    __syncthreads();
  }
  double bb = 0.0;
  for (int i = first + t; i < end; i += QE_STRIDE) {
    double x = w[i];
    for (int q = 0; q <= j; q++) x = x - (WPU == 1 ? pc[q] : cf[q]) * V[(long long)q * n + i];  // (WPU = 1: the block is its one unit)
    w[i] = x;
    bb = __fma_rn(x, x, bb);
  }
  bb = ds_unit_sum<WPU>(bb, red);
  if (t == 0) partb[u] = bb;
}

// beta = sqrt(w'w), the block's sum of partb.  The block ends itself where j + 1 equals its length, or where beta >
// EIG_END_REL max(|alpha_0 .. alpha_j|, beta_0 .. beta_{j-1}) does not hold (an invariant subspace - or a value that is not
// finite): it is done, and v_{j+1} stays 0.  Otherwise v_{j+1} = w / beta (not written behind the last step: last).  The
// block's first unit writes T[2 cap b + j] = alpha, T[.. + cap + j] = beta and the state's other copy - of a block that is
// done already a plain copy.
template <int WPU>
__global__ void __launch_bounds__(256) k_qe_next(BfgsTables g, const double *__restrict__ st, double *__restrict__ st_next, double *__restrict__ V,
                                                 long long n, int j, int last, int cap, const double *__restrict__ w,
                                                 const double *__restrict__ parta, const double *__restrict__ partb, double *__restrict__ T) {
#pragma clang fp contract(off)
  __shared__ double slot[2];
  int u, t, b, first, end;
  if (!qe_unit<WPU>(g, u, t, b, first, end)) return;
  const double *s = st + QE_STATE * (long long)b;
  double *sn = st_next + QE_STATE * (long long)b;
  const bool writer = t == 0 && u == g.bunit[b];
  if (s[0] != 0.0) {
    if (writer) sn[0] = s[0], sn[1] = s[1], sn[2] = s[2], sn[3] = s[3];
    return;
  }
  double beta = 0.0, ended = 0.0;
  if (t == 0) {
    const int len = g.boff[b + 1] - g.boff[b];
    const double alpha = ds_block_sum(len, parta + g.bunit[b], 1);
    beta = sqrt(ds_block_sum(len, partb + g.bunit[b], 1));
    const double scale = eig::nan_max(s[3], fabs(alpha));
    const bool end_now = j + 1 >= len || !(beta > EIG_END_REL * scale);
    ended = end_now ? 1.0 : 0.0;
    if (writer) {
      T[(long long)2 * cap * b + j] = alpha, T[(long long)2 * cap * b + cap + j] = beta;
      sn[0] = ended, sn[1] = (double)(j + 1), sn[2] = beta, sn[3] = eig::nan_max(scale, beta);
    }
  }
  beta = qe_bcast<WPU>(beta, &slot[0]), ended = qe_bcast<WPU>(ended, &slot[1]);
  if (ended != 0.0 || last) return;
  double *vn = V + (long long)(j + 1) * n;
  for (int i = first + t; i < end; i += QE_STRIDE) vn[i] = w[i] / beta;
}

// Workgroup b, one wavefront: eig::ritz on block b's T (eigen_ritz.hip.h) - the Sturm bracket, the residual bound, the
// conservative estimate lo - rho and the shift.  rep[QE_REPORT b ..]: g, theta (k_qe_begin), steps, lo, hi, rho, lambda_est,
// d, |T|, outcome.  st: the copy of the state the last step wrote.
__global__ void __launch_bounds__(64) k_qe_ritz(const double *__restrict__ st, const double *__restrict__ T, int cap, double *__restrict__ rep) {
  __shared__ eig::RitzLds lds;
  const long long b = blockIdx.x;
  double *r = rep + QE_REPORT * b;
  if (r[QE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 6: decided by k_qe_begin)
  const int m = min((int)st[QE_STATE * b + 1], cap);
  const double *al = T + 2 * (long long)cap * b;
  eig::ritz(al, al + cap, m, r[1], r, lds);
}

// the shift, a thread per variable: q_ii <- fl(q_ii + d_b), d_b = rep[QE_REPORT b + 7]; a block with d_b == 0 is not touched
__global__ void __launch_bounds__(256) k_qe_shift(int n, const int *__restrict__ blk_of, const int *__restrict__ didx,
                                                  const double *__restrict__ rep, double *__restrict__ vals) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double d = rep[QE_REPORT * (long long)blk_of[i] + 7];
  if (d != 0.0) vals[didx[i]] = vals[didx[i]] + d;
}

#undef QE_STRIDE
#undef QE_EPT

}  // namespace qv
