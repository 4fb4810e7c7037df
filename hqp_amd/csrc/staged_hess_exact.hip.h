// gfx950 kernels of hqpkkt_eigen_control_stage_hessians_exact (include/hqpkkt.h): the eigenvalue control of the dense stage
// Hessians with the EXACT smallest eigenvalue of every block, for stages of order up to HX_MAX = 2048 - the reference's
// symmeig on the block (hqp/Hqp_HL_BFGS.C:203-212), where the Lanczos control (k_he_*, staged_hess_guard.hip.h) estimates
// from below.  Behind the Lanczos entry's own preamble (the floors, the row pass, k_he_start: g_k, theta_k and the outcomes
// 0 and 5 are that entry's bits) two launches:
// k_hx_block<NB, ROWS>  persistent workgroups of 1024 threads, grid = slots; workgroup w takes the stages w, w + slots, ..
//              one after the other in slot w: the image (LD x LD doubles, LD = the largest stage order rounded up to 16) and
//              behind it the panels V and W (LD x 32 doubles each, a row's NB values side by side).  A stage whose report
//              holds outcome 0 or 5 gets its T words cleared and nothing else.  Workgroups share nothing: no atomics, nothing
//              polled, every loop bounded by the stage's order.  Thread t stands for the indices t and t + 1024 of the stage
//              wherever a value per index is formed
//   copy-in    the stage's block read where it lies, every entry (i, j), i, j < L, of the image written once:
//              dense     row i of Q + oQ at ld, the columns below L; a lane takes consecutive columns
//              packed    the stored 128 x 128 tiles (a, b), b <= a, as 2 x 2 subtiles of 64 x 64 through an LDS tile of
//                        64 x 65: a subtile strictly below the diagonal is read once, rows side by side, written at its own
//                        place and - behind a barrier - transposed at its image, both with a row's columns side by side; of a
//                        subtile on the diagonal the lower half is written to both halves; a subtile above the diagonal (of a
//                        diagonal tile) is not read.  Rows and columns past L are neither read nor written
//              The blocks are symmetric bit for bit in both layouts, so both give the same image, symmetric bit for bit.
//              The padding columns of a dense block (ld > L), the ragged rows of a tile and the slot past L x L never enter
//   reduce     blocked, lower form, dlatrd's scheme in the order q_eigen_blocked.hip.h states for k_qeb_block - panels of NB
//              columns; column k = j0 + i less the panel's earlier columns, c ascending, x <- fl(x - fl(fl(V_rc W_kc) +
//              fl(W_rc V_kc))); the zero-sub-column rule (beta_k = x_0, column i of V and W zero); beta_k = -sign(x_0)
//              sqrt(sum x^2), v = x - beta_k e_0, h = sum x^2 - x_0 beta_k; p = A v / h by ONE pass over the trailing image as
//              the last panel update left it; the correction by the panel's earlier columns; q = p - (v'p / 2h) v; behind a
//              whole panel A <- A - (V W' + W V') on v_mfma_f64_16x16x4 over the 16 x 16 tiles on and below the diagonal,
//              each stored with its transposed image.  Sums over the indices: a butterfly per group of 64 indices, the groups
//              in ascending order; sums over a row: a chain of __fma_rn per lane over its columns ascending, then the
//              butterfly.  The orders 1 and 2 and the last two columns of every stage have no tail and form no reflector:
//              alpha_k is the column's head, beta_{L-2} its one sub-entry, beta_{L-1} = 0
//   pass       wavefronts take the rows r > k cyclically, ROWS (4 or 8) of them in flight; a lane the columns k + 1 + lane +
//              64 c.  A row's sum does not depend on ROWS, nor do the wavefront's sums V'v and W'v, which take its rows in
//              ascending order: both instances give the same bits.  ROWS = 4 is the default by the measurement in DESIGN.md
//   T out      alpha_k at Tx[2 cap s + k], beta_k at Tx[2 cap s + cap + k], cap the largest stage order; words past L zero.
//              A stage's bits depend on its order and its values alone - not on its slot, the layout, the other stages or
//              ROWS - and are equal from call to call
// k_hx_ritz    one workgroup of ONE wavefront per stage: eig::ritz, its body unchanged, on work arrays of 2048
//              (RitzLdsT<2048>, 96 KB of dynamic LDS) with m = L; it skips the outcomes 0 and 5 and writes no shift - the
//              entry's k_hg_diag launch adds d_k as the Lanczos entry's does
// gfx950, hipcc -O3, by the compiler's resource remarks: k_hx_block<16, 4> 104 VGPRs, k_hx_block<16, 8> 105, 106 SGPRs
// (11 and 25 SGPRs spilled to VGPR lanes), 41 992 B of static LDS each, no scratch, no VGPR spill; k_hx_ritz 64 VGPRs,
// 96 KB of dynamic LDS, no scratch, no spill.
// Plain loads and stores in the handle's stream.  No contraction; sums that fuse say __fma_rn (and the matrix pipe fuses).
// Stages over 2048 and several workgroups per stage: staged_hess_wide.hip.h.  Not built: the control chained from the
// BFGS update's launch sequence.  Included by staged_hess.hip.h behind staged_hess_guard.hip.h.
#pragma once
#include "staged_hess_guard.hip.h"

namespace stg {

static const int HX_MAX = 2048;                    // the largest order these kernels serve (HQPKKT_EIG_EXACT_MAX)
static const int HX_NT = 1024, HX_NW = HX_NT / 64;  // threads and wavefronts of k_hx_block
static const int HX_GROUPS = HX_MAX / 64;          // groups of 64 indices: the parts of a sum over the stage
static const int HX_PANEL = 32;                    // columns the slot's panels are sized for
static const int HX_SUB = 64;                      // the subtile of the packed copy-in

// doubles of one slot: the image and the two panels
__host__ __device__ static inline size_t hx_slot_doubles(int ld) { return (size_t)ld * ld + 2 * (size_t)ld * HX_PANEL; }

// the values red[0 .. nw - 1] in ascending order (after a barrier): qv::qel_sum's order
__device__ __forceinline__ double hx_sum(const double *red, int nw) {
#pragma clang fp contract(off)
  double s = red[0];
  for (int w = 1; w < nw; w++) s = s + red[w];
  return s;
}

// The image of a packed stage: see copy-in above.  tl: HX_SUB x (HX_SUB + 1) doubles of LDS.  Ends behind a barrier.
__device__ __forceinline__ void hx_copy_packed(const double *__restrict__ Qt, int L, double *A, int LD, double *tl) {
  constexpr int S = HX_SUB, H = HP_T / S;
  const int t = threadIdx.x, c = t & (S - 1), r0 = t >> 6;  // (a thread: column c of the rows r0, r0 + 16, ..)
  const int nt = (L + HP_T - 1) / HP_T;
  for (int a = 0; a < nt; a++)
    for (int b = 0; b <= a; b++) {
      const double *tile = Qt + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T;
      for (int sub = 0; sub < H * H; sub++) {
        const int p = sub / H, q = sub % H;
        const int gi = a * HP_T + p * S, gj = b * HP_T + q * S;  // the subtile's first row and column in the block
        if (gi < gj || gi >= L) continue;                        // (uniform: above the diagonal, or past the stage; gj <= gi)
        const bool diag = gi == gj;
        for (int r = r0; r < S; r += HX_NW) {
          const int i = gi + r, j = gj + c;
          if (i < L && j < L && (!diag || j <= i)) {
            const double v = tile[(p * S + r) * HP_T + q * S + c];
            tl[r * (S + 1) + c] = v;
            A[(size_t)i * LD + j] = v;
          }
        }
        __syncthreads();
        for (int r = r0; r < S; r += HX_NW) {  // entry (gj + r, gi + c) of the block = entry (c, r) of the subtile
          const int i = gj + r, j = gi + c;
          if (i < L && j < L && (!diag || j > i)) A[(size_t)i * LD + j] = tl[c * (S + 1) + r];
        }
        __syncthreads();
      }
    }
}

template <int NB, int ROWS>
__global__ void __launch_bounds__(HX_NT) k_hx_block(const HgDesc *__restrict__ desc, int K1, const double *__restrict__ Q, int cap, double *__restrict__ T,
                                                    const double *__restrict__ rep, double *__restrict__ ws, int LD) {
#pragma clang fp contract(off)
  static_assert(NB == 16 || NB == 32, "a panel is one or two tiles wide and fits the slot");
  static_assert(ROWS == 4 || ROWS == 8, "rows in flight per wavefront");
  constexpr int NT = HX_NT, NW = HX_NW, G = HX_GROUPS, X0 = 2 * G;
  // sv: v; sp: p; part: the wavefronts' parts of the panel sums; cf; red: G maxima, G sums, x_0.  The copy-in's tile lies
  // over sv and sp
  __shared__ double sm[2 * HX_MAX + NW * 64 + 64 + 2 * G + 1];
  static_assert(HX_SUB * (HX_SUB + 1) <= 2 * HX_MAX + NW * 64, "the subtile fits ahead of cf and red");
  double *sv = sm, *sp = sm + HX_MAX, *part = sp + HX_MAX, *cf = part + NW * 64, *red = cf + 64;
  const int t = threadIdx.x, lane = t & 63, wf = t >> 6;
  double *A = ws + (size_t)blockIdx.x * hx_slot_doubles(LD), *V = A + (size_t)LD * LD, *W = V + (size_t)LD * HX_PANEL;
  for (int st = blockIdx.x; st < K1; st += gridDim.x) {
    const HgDesc d = desc[st];
    const int L = d.nz;
    double *Tb = T + 2 * (long long)cap * st;
    if (rep[(long long)HE_REPORT * st + HE_REPORT - 1] >= 0.0 || L < 1 || L > HX_MAX || L > LD || L > cap) {
      // (uniform: outcome 0 or 5 by k_he_start; the other tests never hold - the host sizes LD and cap by the stages)
      for (int k = t; k < 2 * cap; k += NT) Tb[k] = 0.0;
      continue;
    }
    const int ng = (L + 63) >> 6;  // the groups of 64 that hold an index of the stage
    if (d.packed)
      hx_copy_packed(Q + d.oQ, L, A, LD, sm);
    else {
      for (int r = wf; r < L; r += NW) {
        const double *row = Q + d.oQ + (long long)r * d.ld;
        for (int j = lane; j < L; j += 64) A[(size_t)r * LD + j] = row[j];
      }
      __syncthreads();
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
          tail = hg_wave_max(tail);
          const double s = kktdev::wave_sum(x[hf] * x[hf]);
          if (lane == 0) red[hf * NW + wf] = tail, red[G + hf * NW + wf] = s;
        }
        if (t == 0 && k + 1 >= L) red[X0] = 0.0;  // (the last column has no x_0: beta_{L-1} = 0)
        __syncthreads();
        const double x0 = red[X0];
        double tail = red[0];
        for (int w = 1; w < ng; w++) tail = hg_max(tail, red[w]);
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
        const double ss = hx_sum(red + G, ng);
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
        {  // the pass: the wavefront's rows, ROWS at a time; the lane's columns; and the lane's column of the panels
          const bool pcol = lane < 2 * NB && (lane & (NB - 1)) < i;
          const double *P = (lane < NB ? V : W) + (lane & (NB - 1));
          double acc = 0.0;
          for (int r = k + 1 + __builtin_amdgcn_readfirstlane(wf); r < L; r += ROWS * NW) {  // (scalar: the rows' addresses too)
            unsigned a[ROWS];  // the rows' first words in the image (a row past the stage: the stage's last row, loaded and not used)
            double s[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; u++) a[u] = (unsigned)(r + u * NW < L ? r + u * NW : L - 1) * (unsigned)LD, s[u] = 0.0;
            for (int j = k + 1 + lane; j < L; j += 64) {
              const double vj = sv[j];
#pragma unroll
              for (int u = 0; u < ROWS; u++) s[u] = __fma_rn(A[a[u] + (unsigned)j], vj, s[u]);
            }
#pragma unroll
            for (int u = 0; u < ROWS; u++) {
              const int ru = r + u * NW;
              if (ru < L) {  // (uniform over the wavefront)
                const double su = kktdev::wave_sum(s[u]);
                if (lane == 0) sp[ru] = su / h;
                if (pcol) acc = __fma_rn(P[(size_t)ru * NB], sv[ru], acc);
              }
            }
          }
          part[wf * 64 + lane] = acc;
        }
        __syncthreads();
        if (t < 2 * NB) {  // cf: V'v of the columns 0 .. NB - 1, then W'v
          double s = part[t];
          for (int w = 1; w < NW; w++) s = s + part[w * 64 + t];
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
        const double c = hx_sum(red, ng) / (h + h);
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
          kktdev::double4_t dd = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kk = 0; kk < NB; kk += 4) {
            const double va = Va[kk], wa = Wa[kk], vb = Vb[kk], wb = Wb[kk];
            dd = kktdev::mfma_f64(oka ? va : 0.0, okb ? wb : 0.0, dd);
            dd = kktdev::mfma_f64(oka ? wa : 0.0, okb ? vb : 0.0, dd);
          }
          const int s = 16 * J + lr;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int r = 16 * I + lk + 4 * q;
            if (r < L && s < L && r >= s) {  // (r < s: the upper half of a diagonal tile)
              const double a = A[(size_t)r * LD + s] - dd[q];
              A[(size_t)r * LD + s] = a;
              if (r != s) A[(size_t)s * LD + r] = a;
            }
          }
        }
      }
      __syncthreads();
    }
    __syncthreads();  // (the image, the panels and the LDS are read: the next stage writes them)
  }
}

__global__ void __launch_bounds__(64) k_hx_ritz(const HgDesc *__restrict__ desc, int cap, const double *__restrict__ T, double *__restrict__ rep) {
#pragma clang fp contract(off)
  extern __shared__ double hx_lds[];
  eig::RitzLdsT<HX_MAX> &lds = *reinterpret_cast<eig::RitzLdsT<HX_MAX> *>(hx_lds);
  const int k = blockIdx.x, L = desc[k].nz;
  double *r = rep + (long long)HE_REPORT * k;
  if (L < 1 || L > HX_MAX || L > cap || r[HE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 5: decided by k_he_start)
  const double *al = T + 2 * (long long)cap * k;
  eig::ritz(al, al + cap, L, r[1], r, lds);
}

}  // namespace stg
