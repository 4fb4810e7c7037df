// gfx950 kernels of hqpkkt_q_eigen_control_long (include/hqpkkt.h) for the blocks of a plan that are 129 .. 512 long - a DOCP
// stage with up to 512 states and controls -: the mathematics and the contract of k_qes_block and k_qem_block
// (q_eigen_short.hip.h, q_eigen_mid.hip.h), which serve the plan's shorter blocks in the same call, on a block whose image
// no LDS holds (512 x 512 doubles are 2 MB).  The image lives in device memory, in a SLOT of the plan's workspace, and the
// reduction makes ONE pass over the trailing image per step.  Two launches over the LIST of those blocks:
// k_qel_block  persistent workgroups, grid = slots = min(listed blocks, CUs); workgroup w takes the list entries w,
//              w + slots, .. one after the other in slot w (LD x LD doubles, LD = the list's longest block rounded up to
//              16).  Workgroups share nothing: no atomics, nothing polled.  Instances of 512 and of 1024 threads; thread
//              i < 512 is index i of the block wherever a value per index is formed, the pass below is split by wavefront
//   gather     the slot's L x LD image cleared by all threads - the block before left it dense -, then thread i < L walks
//              row first + i of Qf as the other two kernels do; an entry across blocks is not loaded
//   g, theta   offsum_i in ascending j from +0.0, every add rounded on its own, by thread i alone; g = min_i (a_ii -
//              offsum_i): eig::nan_min over a butterfly per wavefront, then the wavefronts' values in ascending order; theta
//              and the outcomes 0 and 6 as k_qes_block forms them.  Such a block's T words are 0
//   reduce     tred2's steps k = 0 .. L - 3 with the rules of k_qes_block - the zero-sub-column rule, beta_k = -sign(x_0)
//              sqrt(sum x^2), v, h, p = A v / h, q = p - (v'p / 2h) v, a_ij <- fl(a_ij - fl(fl(v_i q_j) + fl(q_i v_j))), both
//              triangles equal bit for bit -, but the rank-2 update of a step is applied LAZILY, by the next step that
//              forms a reflector, so that every element of the trailing image is loaded once per step and not twice:
//     pre-pass k   thread j, k <= j < L, loads a_kj (a contiguous row; column k by symmetry), takes the pending update
//                  off it, and keeps it: alpha_k = a_kk, x_j = a_kj.  Row k is final and is not stored again.  The max that
//                  finds a zero tail and sum x^2: a butterfly per wavefront, then the wavefronts' values through LDS in
//                  ascending order.  A step without a reflector ends here and leaves the pending update pending (a
//                  uniform flag says whether there is one)
//     pass k       wavefronts take the rows i > k cyclically; a lane takes the columns k + 1 + lane + 64 c, so a wavefront
//                  reads 512 B of a row at once, and holds v_j and the pending v_j, q_j of ITS columns in registers over
//                  all its rows.  Each element is loaded once, updated, stored (only where an update was pending) and
//                  multiplied into the lane's chain of __fma_rn over ascending c from +0.0; the row's sum is the
//                  wavefront's butterfly, p_i = fl(sum / h)
//     q            v'p as the sums above; q_i = fl(p_i - fl(c v_i)), c = fl(v'p / fl(h + h)); (v, q) is the new pending update
//              After the last step the pending update goes onto the trailing 2 x 2: alpha_{L-2}, alpha_{L-1}, beta_{L-2}.
//              Five barriers per step.  LDS: v, q of two steps, p, alpha, beta, the wavefronts' partials: 28.1 KB,
//              static
//   T out      alpha then beta, stride 2 cap, words past L zero: every word of the block's T and report written once
//              So a block's bits depend on its length and its values alone - not on its slot, on where it lies, on the
//              other blocks, on the instance or on the mode -, and are equal from call to call
// k_qel_ritz   one workgroup of ONE wavefront per listed block, the pattern of k_qem_ritz: eig::ritz, its body unchanged, on
//              work arrays of 512 (RitzLdsT<512>, 24 KB), then q_ii <- fl(q_ii + d_b) through didx, ceil(L / 64) rows per lane
// Plain loads and stores in the handle's stream.  No contraction; sums that fuse say __fma_rn.
// No MFMA: a step is a symmetric matrix-vector product and a rank-2 update whose operands change with the step, bound by
// the 16 B per element and step that move through memory.  A BLOCKED reduction (dsytrd's panels and a rank-2b update of the
// trailing image) would put half of the flops on the matrix pipe - the matrix-vector half stays memory-bound -, but it
// changes the order of the operations that hessian_update.q_tridiag_model restates and every bit of T with it.
// Not built: that blocked reduction; storage of one triangle alone (half the traffic again); blocks over 512; several
// order-8 blocks per wavefront.
// Included by q_entries.hip behind q_eigen_mid.hip.h.
#pragma once
#include "q_eigen_mid.hip.h"

namespace qv {

static const int QEL_MIN = 129, QEL_MAX = 512;  // the lengths these kernels serve (HQPKKT_QEIG_LONG_MAX)
static const int QEL_COLS = QEL_MAX / 64;      // columns of a row per lane

// `a` of the wavefronts 0 .. nw - 1, one value each in red, in ascending order (after a barrier)
__device__ __forceinline__ double qel_sum(const double *red, int nw) {
#pragma clang fp contract(off)
  double s = red[0];
  for (int w = 1; w < nw; w++) s = s + red[w];
  return s;
}

template <int NT>
__global__ void __launch_bounds__(NT) k_qel_block(const int *__restrict__ list, int count, const int *__restrict__ boff, kktdev::CsrDev Q,
                                                  const double *__restrict__ flr, double eps2, const double *__restrict__ bfgs, int cap,
                                                  double *T, double *rep, double *ws, int LD) {
#pragma clang fp contract(off)
  constexpr int NW = NT / 64, NW8 = QEL_MAX / 64;  // wavefronts of the pass; of the threads that stand for an index
  __shared__ double sv[2][QEL_MAX], sq[2][QEL_MAX], sw[QEL_MAX], al[QEL_MAX], be[QEL_MAX], red[2 * (QEL_MAX / 64) + 1];  // (red: 8 maxima, 8 sums, x_0)
  const int t = threadIdx.x, lane = t & 63, wf = t >> 6;
  const bool idx = t < QEL_MAX;  // (uniform over a wavefront) the threads that stand for an index of the block
  double *A = ws + (size_t)blockIdx.x * LD * LD;
  for (int ent = blockIdx.x; ent < count; ent += gridDim.x) {
    const long long b = list[ent];
    const int first = boff[b], L = boff[b + 1] - first;
    if (L < QEL_MIN || L > QEL_MAX || L > LD || L > cap) continue;  // (never: the host lists these lengths alone and sizes LD by them)
    const int nwl = (L + 63) >> 6;  // the wavefronts that hold an index of the block
    for (int k = t; k < L * LD; k += NT) A[k] = 0.0;
    __syncthreads();
    const bool mine = t < L;
    if (mine) {
      const int row = first + t;
      for (int k = Q.ptr[row], e = Q.ptr[row + 1]; k < e; k++) {
        const int c = Q.col[k] - first;
        if (c >= 0 && c < L) A[(size_t)t * LD + c] = Q.val[k];
      }
    }
    __syncthreads();
    double g = __builtin_inf();
    if (mine) {
      const double *row = A + (size_t)t * LD;
      double off = 0.0;
      for (int j = 0; j < L; j++)
        if (j != t) off = off + fabs(row[j]);
      g = row[t] - off;
    }
    if (idx) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) g = eig::nan_min(g, __shfl_xor(g, o));
      if (lane == 0) red[wf] = g;
    }
    __syncthreads();
    g = red[0];
    for (int w = 1; w < nwl; w++) g = eig::nan_min(g, red[w]);
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
      double *r = rep + QE_REPORT * b;
      r[0] = g, r[1] = theta;
      for (int w = 2; w < QE_REPORT - 1; w++) r[w] = 0.0;
      r[QE_REPORT - 1] = (double)outcome;
    }
    __syncthreads();    // (red is read: the next block and the steps write it again)
    double *Tb = T + 2 * (long long)cap * b;
    if (outcome >= 0) {  // (uniform over the workgroup)
      for (int k = t; k < 2 * cap; k += NT) Tb[k] = 0.0;
      continue;
    }
    bool pend = false;  // (uniform) an update (sv[pb], sq[pb]) waits for the trailing image
    int pb = 0;
    for (int k = 0; k + 2 < L; k++) {
      const bool in = t > k && t < L;
      double x = 0.0;
      if (idx) {
        if (t >= k && t < L) {
          double a = A[(size_t)k * LD + t];
          if (pend) a = a - (sv[pb][k] * sq[pb][t] + sq[pb][k] * sv[pb][t]);
          if (t == k) al[k] = a;
          if (t == k + 1) red[2 * NW8] = a;
          if (in) x = a;
        }
        double tail = t > k + 1 ? fabs(x) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tail = eig::nan_max(tail, __shfl_xor(tail, o));
        const double s = kktdev::wave_sum(x * x);
        if (lane == 0) red[wf] = tail, red[NW8 + wf] = s;
      }
      __syncthreads();
      const double x0 = red[2 * NW8];
      double tail = red[0];
      for (int w = 1; w < nwl; w++) tail = eig::nan_max(tail, red[w]);
      if (tail == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
        if (t == 0) be[k] = x0;
        __syncthreads();  // (red is read)
        continue;
      }
      const double ss = qel_sum(red + NW8, nwl);
      const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
      const double v = t == k + 1 ? x - beta : x;
      const double h = ss - x0 * beta;
      const int nb = pb ^ 1;
      if (mine) sv[nb][t] = v;
      if (t == 0) be[k] = beta;
      __syncthreads();
      {  // pass k: the wavefront's rows, the lane's columns
        const int j0 = k + 1 + lane, nfull = (L - k - 1) >> 6;  // chunks of 64 trailing columns that are whole; the next is part
        const bool part = lane < ((L - k - 1) & 63);             // ... and this lane has a column in it
        double vj[QEL_COLS], vpj[QEL_COLS], qpj[QEL_COLS];
#pragma unroll
        for (int c = 0; c < QEL_COLS; c++) {
          const int j = j0 + 64 * c;
          const bool ok = c < nfull || (c == nfull && part);
          vj[c] = ok ? sv[nb][j] : 0.0;
          vpj[c] = ok && pend ? sv[pb][j] : 0.0;
          qpj[c] = ok && pend ? sq[pb][j] : 0.0;
        }
        for (int i = k + 1 + wf; i < L; i += NW) {
          double *row = A + (size_t)i * LD;
          const double vpi = pend ? sv[pb][i] : 0.0, qpi = pend ? sq[pb][i] : 0.0;
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < QEL_COLS; c++) {
            const int j = j0 + 64 * c;
            if (c < nfull || (c == nfull && part)) {
              double a = row[j];
              if (pend) {
                a = a - (vpi * qpj[c] + qpi * vpj[c]);
                row[j] = a;
              }
              s = __fma_rn(a, vj[c], s);
            }
          }
          s = kktdev::wave_sum(s);
          if (lane == 0) sw[i] = s / h;
        }
      }
      __syncthreads();
      const double p = in ? sw[t] : 0.0;
      if (idx) {
        const double s = kktdev::wave_sum(v * p);
        if (lane == 0) red[wf] = s;
      }
      __syncthreads();
      const double c = qel_sum(red, nwl) / (h + h);
      if (mine) sq[nb][t] = p - c * v;
      pb = nb, pend = true;
      __syncthreads();
    }
    if (t == 0) {  // the trailing 2 x 2
      const int i = L - 2, j = L - 1;
      double aii = A[(size_t)i * LD + i], aji = A[(size_t)j * LD + i], ajj = A[(size_t)j * LD + j];
      if (pend) {
        const double vi = sv[pb][i], qi = sq[pb][i], vj = sv[pb][j], qj = sq[pb][j];
        aii = aii - (vi * qi + qi * vi), aji = aji - (vj * qi + qj * vi), ajj = ajj - (vj * qj + qj * vj);
      }
      al[i] = aii, al[j] = ajj, be[i] = aji, be[j] = 0.0;
    }
    __syncthreads();
    for (int k = t; k < 2 * cap; k += NT) Tb[k] = k < L ? al[k] : (k >= cap && k - cap < L) ? be[k - cap] : 0.0;
    __syncthreads();  // (al, be and the image are read: the next block writes them)
  }
}

__global__ void __launch_bounds__(64) k_qel_ritz(const int *__restrict__ list, const int *__restrict__ boff, const int *__restrict__ didx,
                                                 double *vals, int cap, const double *T, double *rep) {
#pragma clang fp contract(off)
  __shared__ eig::RitzLdsT<QEL_MAX> lds;
  const long long b = list[blockIdx.x];
  const int lane = threadIdx.x, first = boff[b], L = boff[b + 1] - first;
  double *r = rep + QE_REPORT * b;
  if (L < QEL_MIN || L > QEL_MAX || L > cap || r[QE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 6: decided by k_qel_block)
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
