// gfx950 kernels of hqpkkt_q_eigen_control_blocked (include/hqpkkt.h) for the blocks of a plan that are 513 .. 2048 long - a
// DOCP stage with up to 2048 states and controls -: the contract of k_qel_block (q_eigen_long.hip.h), which serves the
// plan's blocks of 129 .. 512 in the same call, by a BLOCKED reduction (dlatrd / dsytrd's scheme, lower form): the trailing
// image is read once per step, for the product alone, and written once per PANEL of NB steps, by a rank-2 NB update on
// v_mfma_f64_16x16x4.  Per step the image moves 8 B per element and 16 B / NB more; k_qel_block moves 16 B.
// Two launches over the LIST of those blocks:
// k_qeb_block<NB>  persistent workgroups of 1024 threads, grid = slots; workgroup w takes the list entries w, w + slots, ..
//              one after the other in slot w: the image (LD x LD doubles, LD = the list's longest block rounded up to 16)
//              and behind it the panels V and W (LD x 32 doubles each, a row's NB values side by side).  Workgroups share
//              nothing: no atomics, nothing polled, every loop bounded by the block's length.  Thread t stands for the
//              indices t and t + 1024 of the block wherever a value per index is formed
//   gather     as k_qel_block: the slot's L x LD image cleared, then row first + r of Qf; an entry across blocks is not loaded
//   g, theta   offsum_i in ascending j from +0.0, every add rounded on its own, by one thread, which walks COLUMN i of the
//              image (the same bits: Qf is the image of the stored upper entries; the lanes' reads lie side by side);
//              g = min_i (a_ii - offsum_i): eig::nan_min over a butterfly per wavefront, then the 64-index groups' values
//              in ascending order; theta and the outcomes 0 and 6 as k_qes_block forms them.  Such a block's T words are 0
//   reduce     panels of NB columns, j0 = 0, NB, ..; column k = j0 + i of a panel, for every k < L (the columns L - 2 and
//              L - 1 have no tail and so no reflector: they give alpha_{L-2}, beta_{L-2}, alpha_{L-1} and beta_{L-1} = 0):
//     column   the thread of index r >= k loads a_kr (row k, contiguous; column k by symmetry) and takes the panel's
//              earlier columns off it, c = 0 .. i - 1 ascending: x <- fl(x - fl(fl(V_rc W_kc) + fl(W_rc V_kc))).  alpha_k
//              = x_k.  The max that finds a zero tail and sum x^2: a butterfly per wavefront, then the groups of 64
//              indices through LDS in ascending order.  Zero tail: beta_k = x_0, column i of V and W zero, no more
//     v, h     beta_k = -sign(x_0) sqrt(sum x^2), v = x - beta_k e_0, h = sum x^2 - x_0 beta_k; v to LDS
//     pass     wavefronts take the rows r > k cyclically, four at a time; a lane takes the columns k + 1 + lane + 64 c of
//              the image AS THE LAST PANEL UPDATE LEFT IT, a chain of __fma_rn over ascending c from +0.0 against v in LDS;
//              the row's sum is the wavefront's butterfly, p_r = fl(sum / h).  With its rows the wavefront also sums
//              V'v and W'v of the panel's earlier columns - lane c < NB column c of V, lane NB + c that of W, __fma_rn
//              over its rows ascending - and the 16 wavefronts' parts are added in ascending order
//     correct  p_r <- fl(p_r - fl(s_r / h)), s_r the sum over c ascending from +0.0 of fl(fl(V_rc (W'v)_c) + fl(W_rc (V'v)_c))
//     q        v'p as the sums above; q_r = fl(p_r - fl(c v_r)), c = fl(v'p / fl(h + h)); V_ri <- v_r, W_ri <- q_r
//     update   behind a whole panel that leaves a trailing image, A <- A - (V W' + W V') on the rows and columns >= j0 + NB:
//              wavefronts take the 16 x 16 tiles on and below the diagonal cyclically; a tile's V W' + W V' is 2 NB / 4
//              v_mfma_f64_16x16x4 from +0.0, operands straight from the panels (a row past L enters as +0.0, never as
//              what the slot holds), then a_rs <- fl(a_rs - d_rs) stored at (r, s) AND at (s, r): the image stays
//              symmetric bit for bit.  Of a diagonal tile the lower half counts.  The last panel has no update
//   T out      alpha_k and beta_k as their column forms them, words past L zero: every word of the block's T and report
//              written once.  A block's bits depend on its length and its values alone - not on its slot, on where it
//              lies, on the other blocks or on the mode -, and are equal from call to call.  (They do depend on NB.)
//              LDS: v, p, the wavefronts' parts of the panel sums, the sums: 41.5 KB, static
// k_qeb_ritz   one workgroup of ONE wavefront per listed block, the pattern of k_qel_ritz: eig::ritz, its body unchanged, on
//              work arrays of 2048 (RitzLdsT<2048>, 96 KB of dynamic LDS), then q_ii <- fl(q_ii + d_b) through didx
// Plain loads and stores in the handle's stream.  No contraction; sums that fuse say __fma_rn (and the matrix pipe fuses).
// Not built: storage of one triangle alone; several workgroups per block; blocks over 2048; a numpy model of this order.
// Included by q_entries.hip behind q_eigen_long.hip.h.
#pragma once
#include "q_eigen_long.hip.h"

namespace qv {

static const int QEB_MIN = QEL_MAX + 1, QEB_MAX = 2048;  // the lengths these kernels serve (HQPKKT_QEIG_BLOCKED_MAX)
static const int QEB_NT = 1024, QEB_NW = QEB_NT / 64;    // threads and wavefronts of k_qeb_block
static const int QEB_GROUPS = QEB_MAX / 64;              // groups of 64 indices: the parts of a sum over the block
static const int QEB_PANEL = 32;                         // columns the slot's panels are sized for (the larger NB)

// doubles of one slot: the image and the two panels
__host__ __device__ static inline size_t qeb_slot_doubles(int ld) { return (size_t)ld * ld + 2 * (size_t)ld * QEB_PANEL; }

template <int NB>
__global__ void __launch_bounds__(QEB_NT) k_qeb_block(const int *__restrict__ list, int count, const int *__restrict__ boff, kktdev::CsrDev Q,
                                                      const double *__restrict__ flr, double eps2, const double *__restrict__ bfgs, int cap,
                                                      double *T, double *rep, double *ws, int LD) {
#pragma clang fp contract(off)
  static_assert(NB == 16 || NB == 32, "a panel is one or two tiles wide and fits the slot");
  constexpr int NT = QEB_NT, NW = QEB_NW, G = QEB_GROUPS, X0 = 2 * G;
  __shared__ double sv[QEB_MAX], sp[QEB_MAX], part[NW][64], cf[64], red[2 * G + 1];  // (red: G maxima, G sums, x_0)
  const int t = threadIdx.x, lane = t & 63, wf = t >> 6;
  double *A = ws + (size_t)blockIdx.x * qeb_slot_doubles(LD), *V = A + (size_t)LD * LD, *W = V + (size_t)LD * QEB_PANEL;
  for (int ent = blockIdx.x; ent < count; ent += gridDim.x) {
    const long long b = list[ent];
    const int first = boff[b], L = boff[b + 1] - first;
    if (L < QEB_MIN || L > QEB_MAX || L > LD || L > cap) continue;  // (never: the host lists these lengths alone and sizes LD by them)
    const int ng = (L + 63) >> 6;  // the groups of 64 that hold an index of the block
    for (int k = t; k < L * LD; k += NT) A[k] = 0.0;
    __syncthreads();
    for (int r = t; r < L; r += NT) {
      const int row = first + r;
      for (int k = Q.ptr[row], e = Q.ptr[row + 1]; k < e; k++) {
        const int c = Q.col[k] - first;
        if (c >= 0 && c < L) A[(size_t)r * LD + c] = Q.val[k];
      }
    }
    __syncthreads();
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
      const int r = t + hf * NT;
      double g = __builtin_inf();
      if (r < L) {
        double off = 0.0;
        for (int j = 0; j < L; j++)
          if (j != r) off = off + fabs(A[(size_t)j * LD + r]);
        g = A[(size_t)r * LD + r] - off;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) g = eig::nan_min(g, __shfl_xor(g, o));
      if (lane == 0) red[hf * NW + wf] = g;
    }
    __syncthreads();
    double g = red[0];
    for (int w = 1; w < ng; w++) g = eig::nan_min(g, red[w]);
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
    __syncthreads();  // (red is read: the next block and the columns write it again)
    double *Tb = T + 2 * (long long)cap * b;
    if (outcome >= 0) {  // (uniform over the workgroup)
      for (int k = t; k < 2 * cap; k += NT) Tb[k] = 0.0;
      continue;
    }
    for (int k = L + t; k < cap; k += NT) Tb[k] = Tb[cap + k] = 0.0;  // (the words before them: by the columns below)
    for (int j0 = 0; j0 < L; j0 += NB) {
      const int nb = L - j0 < NB ? L - j0 : NB;
      for (int i = 0; i < nb; i++) {
        const int k = j0 + i;
        const double *Vk = V + (size_t)k * NB, *Wk = W + (size_t)k * NB;
        double x[2], v[2], p[2];
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {  // the column as the panel's earlier columns leave it
          const int r = t + hf * NT;
          x[hf] = 0.0;
          if (r >= k && r < L) {
            const double *Vr = V + (size_t)r * NB, *Wr = W + (size_t)r * NB;
            double a = A[(size_t)k * LD + r];
            for (int c = 0; c < i; c++) a = a - (Vr[c] * Wk[c] + Wr[c] * Vk[c]);
            if (r == k)
              Tb[k] = a;
            else
              x[hf] = a;
            if (r == k + 1) red[X0] = a;
          }
          double tail = r > k + 1 ? fabs(x[hf]) : 0.0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) tail = eig::nan_max(tail, __shfl_xor(tail, o));
          const double s = kktdev::wave_sum(x[hf] * x[hf]);
          if (lane == 0) red[hf * NW + wf] = tail, red[G + hf * NW + wf] = s;
        }
        if (t == 0 && k + 1 >= L) red[X0] = 0.0;  // (the last column has no x_0: beta_{L-1} = 0)
        __syncthreads();
        const double x0 = red[X0];
        double tail = red[0];
        for (int w = 1; w < ng; w++) tail = eig::nan_max(tail, red[w]);
        if (tail == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
          if (t == 0) Tb[cap + k] = x0;
#pragma unroll
          for (int hf = 0; hf < 2; hf++) {
            const int r = t + hf * NT;
            if (r > k && r < L) V[(size_t)r * NB + i] = W[(size_t)r * NB + i] = 0.0;
          }
          __syncthreads();  // (red is read; the panel's column is written)
          continue;
        }
        const double ss = qel_sum(red + G, ng);
        const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
        const double h = ss - x0 * beta;
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
          const int r = t + hf * NT;
          v[hf] = r == k + 1 ? x[hf] - beta : x[hf];
          if (r > k && r < L) sv[r] = v[hf];
        }
        if (t == 0) Tb[cap + k] = beta;
        __syncthreads();
        {  // the pass: the wavefront's rows, four at a time; the lane's columns; and the lane's column of the panels
          const bool pcol = lane < 2 * NB && (lane & (NB - 1)) < i;
          const double *P = (lane < NB ? V : W) + (lane & (NB - 1));
          double acc = 0.0;
          for (int r = k + 1 + wf; r < L; r += 4 * NW) {
            const double *a0 = A + (size_t)r * LD;  // (a row past the block: the block's last row, loaded and not used)
            const double *a1 = A + (size_t)(r + NW < L ? r + NW : L - 1) * LD;
            const double *a2 = A + (size_t)(r + 2 * NW < L ? r + 2 * NW : L - 1) * LD;
            const double *a3 = A + (size_t)(r + 3 * NW < L ? r + 3 * NW : L - 1) * LD;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int j = k + 1 + lane; j < L; j += 64) {
              const double vj = sv[j];
              s0 = __fma_rn(a0[j], vj, s0), s1 = __fma_rn(a1[j], vj, s1), s2 = __fma_rn(a2[j], vj, s2), s3 = __fma_rn(a3[j], vj, s3);
            }
            const double s[4] = {s0, s1, s2, s3};
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int ru = r + u * NW;
              if (ru < L) {  // (uniform over the wavefront)
                const double su = kktdev::wave_sum(s[u]);
                if (lane == 0) sp[ru] = su / h;
                if (pcol) acc = __fma_rn(P[(size_t)ru * NB], sv[ru], acc);
              }
            }
          }
          part[wf][lane] = acc;
        }
        __syncthreads();
        if (t < 2 * NB) {  // cf: V'v of the columns 0 .. NB - 1, then W'v
          double s = part[0][t];
          for (int w = 1; w < NW; w++) s = s + part[w][t];
          cf[t] = s;
        }
        __syncthreads();
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
          const int r = t + hf * NT;
          const bool in = r > k && r < L;
          p[hf] = 0.0;
          if (in) {
            const double *Vr = V + (size_t)r * NB, *Wr = W + (size_t)r * NB;
            double s = 0.0;
            for (int c = 0; c < i; c++) s = s + (Vr[c] * cf[NB + c] + Wr[c] * cf[c]);
            p[hf] = sp[r] - s / h;
          }
          const double s = kktdev::wave_sum(in ? v[hf] * p[hf] : 0.0);
          if (lane == 0) red[hf * NW + wf] = s;
        }
        __syncthreads();
        const double c = qel_sum(red, ng) / (h + h);
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
          const int r = t + hf * NT;
          if (r > k && r < L) V[(size_t)r * NB + i] = v[hf], W[(size_t)r * NB + i] = p[hf] - c * v[hf];
        }
        __syncthreads();
      }
      if (j0 + NB >= L) break;  // (the last panel: nothing trails it)
      // the trailing image: the tiles (I, J), t0 <= J <= I < nt, dealt to the wavefronts in row-major order of the triangle
      const int t0 = (j0 + NB) >> 4, nt = (L + 15) >> 4, lr = lane & 15, lk = lane >> 4;
      for (int I = t0, at = 0; I < nt; at += I - t0 + 1, I++) {
        for (int J = t0 + ((wf - at) & (NW - 1)); J <= I; J += NW) {
          const int ra = 16 * I + lr, rb = 16 * J + lr;  // the operands' rows: of the tile's rows, of its columns
          const bool oka = ra < L, okb = rb < L;
          const double *Va = V + (size_t)(oka ? ra : 0) * NB + lk, *Wa = W + (size_t)(oka ? ra : 0) * NB + lk;
          const double *Vb = V + (size_t)(okb ? rb : 0) * NB + lk, *Wb = W + (size_t)(okb ? rb : 0) * NB + lk;
          kktdev::double4_t d = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kk = 0; kk < NB; kk += 4) {
            const double va = Va[kk], wa = Wa[kk], vb = Vb[kk], wb = Wb[kk];
            d = kktdev::mfma_f64(oka ? va : 0.0, okb ? wb : 0.0, d);
            d = kktdev::mfma_f64(oka ? wa : 0.0, okb ? vb : 0.0, d);
          }
          const int s = 16 * J + lr;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int r = 16 * I + lk + 4 * q;
            if (r < L && s < L && r >= s) {  // (r < s: the upper half of a diagonal tile)
              const double a = A[(size_t)r * LD + s] - d[q];
              A[(size_t)r * LD + s] = a;
              if (r != s) A[(size_t)s * LD + r] = a;
            }
          }
        }
      }
      __syncthreads();
    }
    __syncthreads();  // (the image, the panels and the LDS are read: the next block writes them)
  }
}

__global__ void __launch_bounds__(64) k_qeb_ritz(const int *__restrict__ list, const int *__restrict__ boff, const int *__restrict__ didx,
                                                 double *vals, int cap, const double *T, double *rep) {
#pragma clang fp contract(off)
  extern __shared__ double qeb_lds[];
  eig::RitzLdsT<QEB_MAX> &lds = *reinterpret_cast<eig::RitzLdsT<QEB_MAX> *>(qeb_lds);
  const long long b = list[blockIdx.x];
  const int lane = threadIdx.x, first = boff[b], L = boff[b + 1] - first;
  double *r = rep + QE_REPORT * b;
  if (L < QEB_MIN || L > QEB_MAX || L > cap || r[QE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 6: decided by k_qeb_block)
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
