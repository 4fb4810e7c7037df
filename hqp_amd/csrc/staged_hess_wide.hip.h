// gfx950 kernels of hqpkkt_eigen_control_stage_hessians_wide (include/hqpkkt.h): the exact eigenvalue control of the dense
// stage Hessians for stages of order up to HW_MAX = 8192, the whole chip on a few images at a time where k_hx_block
// (staged_hess_exact.hip.h) gives a stage to one workgroup.  The method is k_hx_block's: the blocked Householder reduction,
// lower form, dlatrd's scheme, panels of NB = 16 columns, both triangles of the image stored, the zero-sub-column rule, no
// reflector for the last two columns.  The wide stages of a call are taken in batches of S slots, longest first; the stage
// of slot s of a batch is wl[s].  A slot (hw_slot) holds the image A (LD x LD, LD the handle's largest order rounded up
// to 16), the panels V and W (LD x NB, a row's NB values side by side), the vectors x (the column, then v) and p, the row
// groups' partial sums pt and two words sc: h, and whether the column formed last has a reflector.  Workgroups never wait
// for each other - no polled words, no grid-wide barriers, no atomics: every launch is a bounded piece of work and the
// handle's stream orders them.  All slots of a batch advance in lockstep, one launch moves every slot by one step; a slot
// whose stage has outcome 0 or 5 by k_he_start, or whose order the step has passed, leaves at once (uniform exits).
//   k_hw_copy    grid (units, slots), 256 threads.  A dense block row by row: unit u the rows 64 u .. 64 u + 63, a wavefront
//                per row, a lane consecutive columns.  A packed stage by the 64 x 64 subtiles (I, J), J <= I, of its stored
//                128 x 128 tiles, unit u = I (I + 1) / 2 + J: read once, rows side by side, written at its own place and -
//                behind a barrier, through an LDS tile of 64 x 65 - transposed at its image, both with a row's columns side
//                by side; of a subtile on the diagonal the lower half is written to both halves.  Rows and columns past L
//                are neither read nor written.  Unit 0 clears the stage's T words past L (all of them where the stage is
//                done already).  The blocks are symmetric bit for bit in both layouts: both give the same image
//   k_hw_column  one workgroup of 1024 threads per slot; thread t stands for the indices t, t + 1024, ..
//     finish kf  (where that column has a reflector) cf = the groups' partial V'v, W'v and v'p summed in ascending group
//                order; p_r <- fl(p_r - fl(sum_c fl(fl(V_rc cf_W c) + fl(W_rc cf_V c)) / h)), c ascending over the panel's earlier
//                columns; v'p of the corrected p is v'p - 2 (V'v)'(W'v) / h, so the factor is fl(fl(v'p - fl(2 dot / h)) / 2h);
//                w = p - factor v; v and w become column i of V and W (rows r > kf)
//     form kn    x_r = A_kr less the panel's earlier columns, c ascending, x <- fl(x - fl(fl(V_rc W_kc) + fl(W_rc V_kc)));
//                alpha_k = x_k to T; the tail's maximum and sum x^2: a butterfly per group of 64 indices, the groups in
//                ascending order; tail zero: beta_k = x_0, column i of V and W zero, no reflector; else beta_k = -sign(x_0)
//                sqrt(sum x^2), v = x - beta_k e_0 into the slot's vector, h = sum x^2 - x_0 beta_k
//                Behind a whole panel the host launches finish, k_hw_update, form; otherwise both in one launch
//   k_hw_pass    grid (row groups, slots), 256 threads, v of the columns k + 1 .. L - 1 staged in dynamic LDS once per
//                workgroup.  Row group g: the rows k + 1 + 64 g ..; a wavefront takes 16 of them, 4 in flight; a lane the
//                columns k + 1 + lane + 64 c in ascending order as a chain of __fma_rn, then the butterfly; p_r = sum / h.
//                The group's parts of V'v and W'v (lane c < 16: column c of V, lane 16 + c: of W, the panel's earlier columns
//                alone) and of v'p (lane 32) - a wavefront's rows ascending by __fma_rn, the four wavefronts in their order -
//                go to pt[64 g ..].  A workgroup walks the groups g = x, x + grid, ..: the grid's width changes no bits
//   k_hw_update  grid (macro-tiles, slots), 256 threads, once per panel: A <- A - (V W' + W V') on v_mfma_f64_16x16x4 over
//                the 64 x 64 macro-tiles (I, J), J <= I, that hold a row at or past lo = the panel's end.  The panels' rows of
//                the tile's rows and of its columns are staged once in LDS (row stride 17); a row past L or before lo enters
//                as +0.0.  A wavefront takes 16 x 64 as four accumulators from +0.0, k ascending, V W' before W V'.  The
//                result is subtracted and stored at (r, s), and - through an LDS tile of 64 x 65 over the panels - at (s, r),
//                both with a row's columns side by side.  Of a diagonal macro-tile the lower half counts
//   k_hw_ritz    one wavefront per wide stage: eig::ritz, its body unchanged, its six work arrays of cap doubles in device
//                memory (HwRitzMem); it skips the outcomes 0 and 5 and writes no shift - k_hg_diag adds d_k
// A stage's bits depend on its order and its values alone - not on its slot, the batch, the layout, the grids or how many
// workgroups the chip ran at once - and are equal from call to call.  They are NOT k_hx_block's: the sums run over other
// groups.  T out as there: alpha_k at Tx[2 cap s + k], beta_k at Tx[2 cap s + cap + k].
// gfx950, hipcc -O3, by the compiler's resource remarks: k_hw_copy 16 VGPRs, 33 280 B of LDS; k_hw_column 58 VGPRs, 2 576 B;
// k_hw_pass 46 VGPRs, dynamic LDS alone (8 (256 + L - k - 1) B per launch, 67 576 B at most); k_hw_update 140 VGPRs, 34 816 B;
// k_hw_ritz 38 VGPRs, no LDS.  No scratch, no VGPR spill and no SGPR spill in any of them.
// No contraction; sums that fuse say __fma_rn (and the matrix pipe fuses).
// Not built: orders over 8192; one triangle stored (half the image traffic of the pass); the control chained from the BFGS
// update's launch sequence.  Included by staged_hess.hip.h behind staged_hess_exact.hip.h.
#pragma once
#include "staged_hess_exact.hip.h"

namespace stg {

static const int HW_MAX = 8192;               // the largest order these kernels serve (HQPKKT_EIG_WIDE_MAX)
static const int HW_NB = 16;                  // columns of a panel
static const int HW_M = 64;                   // rows of a row group, edge of a macro-tile and of a copied subtile
static const int HW_G = HW_MAX / HW_M;        // row groups of the longest stage
static const int HW_NT = 1024, HW_NW = HW_NT / 64;  // threads and wavefronts of k_hw_column
static const int HW_PT = 64;                  // doubles of a row group's partial sums: 2 NB + 1 used
static const int HW_SC = 8;                   // the slot's words: h, reflector
static const int HW_PASS_ROWS = 4;            // rows a wavefront of k_hw_pass keeps in flight

// doubles of one slot, and where its parts lie
__host__ __device__ static inline size_t hw_slot_doubles(int ld) {
  return (size_t)ld * ld + 2 * (size_t)ld * HW_NB + 2 * (size_t)ld + (size_t)HW_G * HW_PT + HW_SC;
}
struct HwSlot {
  double *A, *V, *W, *x, *p, *pt, *sc;
};
__device__ __forceinline__ HwSlot hw_slot(double *ws, int slot, int LD) {
  HwSlot s;
  s.A = ws + (size_t)slot * hw_slot_doubles(LD);
  s.V = s.A + (size_t)LD * LD, s.W = s.V + (size_t)LD * HW_NB;
  s.x = s.W + (size_t)LD * HW_NB, s.p = s.x + LD, s.pt = s.p + LD, s.sc = s.pt + (size_t)HW_G * HW_PT;
  return s;
}
// a stage these kernels pass over: outcome 0 or 5 by k_he_start (the other tests never hold - the host sizes LD and cap)
__device__ __forceinline__ bool hw_skip(const double *rep, int st, int L, int LD, int cap) {
  return rep[(long long)HE_REPORT * st + HE_REPORT - 1] >= 0.0 || L < 1 || L > HW_MAX || L > LD || L > cap;
}

__global__ void __launch_bounds__(256) k_hw_copy(const HgDesc *__restrict__ desc, const int *__restrict__ wl, const double *__restrict__ Q, int cap,
                                                 double *__restrict__ T, const double *__restrict__ rep, double *__restrict__ ws, int LD) {
  constexpr int M = HW_M;
  __shared__ double tl[M * (M + 1)];
  const int st = wl[blockIdx.y];
  const HgDesc d = desc[st];
  const int L = d.nz, t = threadIdx.x, lane = t & 63, wf = t >> 6, u = blockIdx.x;
  const bool skip = hw_skip(rep, st, L, LD, cap);
  if (u == 0) {  // (the words before L: by the columns)
    double *Tb = T + 2 * (long long)cap * st;
    for (int k = t; k < cap; k += 256)
      if (skip || k >= L) Tb[k] = Tb[cap + k] = 0.0;
  }
  if (skip) return;
  double *A = hw_slot(ws, blockIdx.y, LD).A;
  const int nT = (L + M - 1) / M;
  if (!d.packed) {
    if (u >= nT) return;
    const int r1 = min(M * u + M, L);
    for (int r = M * u + wf; r < r1; r += 4) {
      const double *row = Q + d.oQ + (long long)r * d.ld;
      for (int j = lane; j < L; j += 64) A[(size_t)r * LD + j] = row[j];
    }
    return;
  }
  if (u >= nT * (nT + 1) / 2) return;
  int I, J;
  hp_tile_of(u, I, J);
  constexpr int H = HP_T / M;
  static_assert(H * M == HP_T, "a stored tile is H x H subtiles");
  const int a = I / H, b = J / H, p = I % H, q = J % H;  // (J <= I: b <= a, and q <= p in a diagonal tile)
  const double *tile = Q + d.oQ + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T;
  const int gi = M * I, gj = M * J;
  const bool diag = I == J;
  for (int r = wf; r < M; r += 4) {
    const int i = gi + r, j = gj + lane;
    if (i < L && j < L && (!diag || j <= i)) {
      const double v = tile[(p * M + r) * HP_T + q * M + lane];
      tl[r * (M + 1) + lane] = v;
      A[(size_t)i * LD + j] = v;
    }
  }
  __syncthreads();
  for (int r = wf; r < M; r += 4) {  // entry (gj + r, gi + lane) of the block = entry (lane, r) of the subtile
    const int i = gj + r, j = gi + lane;
    if (i < L && j < L && (!diag || j > i)) A[(size_t)i * LD + j] = tl[lane * (M + 1) + r];
  }
}

__global__ void __launch_bounds__(HW_NT) k_hw_column(const HgDesc *__restrict__ desc, const int *__restrict__ wl, int cap, double *__restrict__ T,
                                                     const double *__restrict__ rep, double *__restrict__ ws, int LD, int kf, int kn) {
#pragma clang fp contract(off)
  constexpr int NB = HW_NB, NT = HW_NT, NW = HW_NW, G = HW_G, X0 = 2 * G;
  __shared__ double red[2 * G + 1], cf[HW_PT];  // red: G maxima, G sums, x_0
  const int st = wl[blockIdx.x], L = desc[st].nz;
  if (hw_skip(rep, st, L, LD, cap)) return;
  const int t = threadIdx.x, lane = t & 63, wf = t >> 6;
  const HwSlot s = hw_slot(ws, blockIdx.x, LD);
  double *Tb = T + 2 * (long long)cap * st;
  if (kf >= 0 && kf + 2 < L && s.sc[1] != 0.0) {  // (uniform; sc is written behind this phase's barriers)
    const int i = kf & (NB - 1), ng = (L - kf - 1 + HW_M - 1) / HW_M;
    const double h = s.sc[0];
    if (t <= 2 * NB) {
      double a = s.pt[t];
      for (int g = 1; g < ng; g++) a = a + s.pt[(size_t)g * HW_PT + t];
      cf[t] = a;
    }
    __syncthreads();
    double dot = 0.0;
    for (int c = 0; c < i; c++) dot = dot + cf[c] * cf[NB + c];
    const double cc = (cf[2 * NB] - (dot + dot) / h) / (h + h);
    for (int r = kf + 1 + t; r < L; r += NT) {
      double *Vr = s.V + (size_t)r * NB, *Wr = s.W + (size_t)r * NB;
      double a = 0.0;
      for (int c = 0; c < i; c++) a = a + (Vr[c] * cf[NB + c] + Wr[c] * cf[c]);
      const double v = s.x[r], p = s.p[r] - a / h;
      Vr[i] = v, Wr[i] = p - cc * v;
    }
    __syncthreads();  // (the panel's column is written: form reads row kn of it)
  }
  if (kn < 0 || kn >= L) return;
  const int k = kn, i = k & (NB - 1), nit = (L + NT - 1) / NT, ng = (L + 63) >> 6;
  const double *Vk = s.V + (size_t)k * NB, *Wk = s.W + (size_t)k * NB;
  for (int it = 0; it < nit; it++) {  // the column as the panel's earlier columns leave it
    const int r = t + it * NT;
    double x = 0.0;
    if (r >= k && r < L) {
      const double *Vr = s.V + (size_t)r * NB, *Wr = s.W + (size_t)r * NB;
      double a = s.A[(size_t)k * LD + r];
      for (int c = 0; c < i; c++) a = a - (Vr[c] * Wk[c] + Wr[c] * Vk[c]);
      if (r == k)
        Tb[k] = a;
      else
        x = a;
      if (r == k + 1) red[X0] = a;
    }
    if (r < L) s.x[r] = x;
    const double tail = hg_wave_max(r > k + 1 ? fabs(x) : 0.0);
    const double sq = kktdev::wave_sum(x * x);
    if (lane == 0) red[it * NW + wf] = tail, red[G + it * NW + wf] = sq;
  }
  if (t == 0 && k + 1 >= L) red[X0] = 0.0;  // (the last column has no x_0: beta_{L-1} = 0)
  __syncthreads();
  const double x0 = red[X0];
  double tail = red[0];
  for (int w = 1; w < ng; w++) tail = hg_max(tail, red[w]);
  if (tail == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
    if (t == 0) Tb[cap + k] = x0, s.sc[1] = 0.0;
    for (int r = k + 1 + t; r < L; r += NT) s.V[(size_t)r * NB + i] = s.W[(size_t)r * NB + i] = 0.0;
    return;
  }
  const double ss = hx_sum(red + G, ng);
  const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
  if (t == ((k + 1) & (NT - 1))) s.x[k + 1] = x0 - beta;  // (the thread that wrote x_0 there)
  if (t == 0) Tb[cap + k] = beta, s.sc[0] = ss - x0 * beta, s.sc[1] = 1.0;
}

__global__ void __launch_bounds__(256) k_hw_pass(const HgDesc *__restrict__ desc, const int *__restrict__ wl, const double *__restrict__ rep, int cap,
                                                 double *__restrict__ ws, int LD, int k) {
#pragma clang fp contract(off)
  constexpr int NB = HW_NB, ROWS = HW_PASS_ROWS;
  extern __shared__ double hw_lds[];  // the wavefronts' parts of the panel sums, then v of the columns k + 1 ..
  const int st = wl[blockIdx.y], L = desc[st].nz;
  if (hw_skip(rep, st, L, LD, cap) || k + 2 >= L) return;
  const HwSlot s = hw_slot(ws, blockIdx.y, LD);
  if (s.sc[1] == 0.0) return;  // (uniform: the column has no reflector)
  double *part = hw_lds, *sv = hw_lds + 256;
  const int t = threadIdx.x, lane = t & 63, wf = __builtin_amdgcn_readfirstlane(t >> 6);
  const int m = L - k - 1, ng = (m + HW_M - 1) / HW_M, i = k & (NB - 1);
  for (int j = t; j < m; j += 256) sv[j] = s.x[k + 1 + j];
  __syncthreads();
  const double h = s.sc[0];
  const bool pcol = lane < 2 * NB && (lane & (NB - 1)) < i, vp = lane == 2 * NB;
  const double *P = (lane < NB ? s.V : s.W) + (lane & (NB - 1));
  const double *Ak = s.A + (k + 1);
  for (int g = blockIdx.x; g < ng; g += gridDim.x) {
    const int rw = k + 1 + HW_M * g + 16 * wf;  // the wavefront's first row
    double acc = 0.0;
    for (int u0 = 0; u0 < 16 && rw + u0 < L; u0 += ROWS) {
      unsigned a[ROWS];  // the rows' first words in the image (a row past the stage: the stage's last row, loaded and not used)
      double sm[ROWS];
#pragma unroll
      for (int u = 0; u < ROWS; u++) a[u] = (unsigned)(rw + u0 + u < L ? rw + u0 + u : L - 1) * (unsigned)LD, sm[u] = 0.0;
      for (int j = lane; j < m; j += 64) {
        const double vj = sv[j];
#pragma unroll
        for (int u = 0; u < ROWS; u++) sm[u] = __fma_rn(Ak[a[u] + (unsigned)j], vj, sm[u]);
      }
#pragma unroll
      for (int u = 0; u < ROWS; u++) {
        const int ru = rw + u0 + u;
        if (ru < L) {  // (uniform over the wavefront)
          const double pr = kktdev::wave_sum(sm[u]) / h, vr = sv[ru - k - 1];
          if (lane == 0) s.p[ru] = pr;
          if (pcol) acc = __fma_rn(P[(size_t)ru * NB], vr, acc);
          if (vp) acc = __fma_rn(pr, vr, acc);
        }
      }
    }
    part[wf * 64 + lane] = acc;
    __syncthreads();
    if (t <= 2 * NB) s.pt[(size_t)g * HW_PT + t] = ((part[t] + part[64 + t]) + part[128 + t]) + part[192 + t];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_hw_update(const HgDesc *__restrict__ desc, const int *__restrict__ wl, const double *__restrict__ rep, int cap,
                                                   double *__restrict__ ws, int LD, int lo) {
#pragma clang fp contract(off)
  constexpr int NB = HW_NB, M = HW_M, PS = NB + 1;
  __shared__ double sm[4 * M * PS];  // the panels' rows; behind the products the tile of the transposed store
  static_assert(M * (M + 1) <= 4 * M * PS, "the tile fits over the panels");
  const int st = wl[blockIdx.y], L = desc[st].nz;
  if (hw_skip(rep, st, L, LD, cap) || lo >= L) return;
  int I, J;
  hp_tile_of(blockIdx.x, I, J);
  I += lo / M, J += lo / M;
  if (M * I >= L) return;
  const HwSlot s = hw_slot(ws, blockIdx.y, LD);
  const int t = threadIdx.x, lane = t & 63, wf = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  double *Va = sm, *Wa = Va + M * PS, *Vb = Wa + M * PS, *Wb = Vb + M * PS;
  for (int e = t; e < M * NB; e += 256) {
    const int row = e / NB, c = e % NB, ra = M * I + row, rb = M * J + row;
    const bool oka = ra >= lo && ra < L, okb = rb >= lo && rb < L;
    Va[row * PS + c] = oka ? s.V[(size_t)ra * NB + c] : 0.0, Wa[row * PS + c] = oka ? s.W[(size_t)ra * NB + c] : 0.0;
    Vb[row * PS + c] = okb ? s.V[(size_t)rb * NB + c] : 0.0, Wb[row * PS + c] = okb ? s.W[(size_t)rb * NB + c] : 0.0;
  }
  __syncthreads();
  const int jmax = I == J ? wf : M / 16 - 1;  // (of a diagonal macro-tile the blocks on and below the diagonal)
  kktdev::double4_t dd[M / 16];
#pragma unroll
  for (int jb = 0; jb < M / 16; jb++) dd[jb] = kktdev::double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < NB; kk += 4) {
    const double va = Va[(16 * wf + lr) * PS + lk + kk], wa = Wa[(16 * wf + lr) * PS + lk + kk];
#pragma unroll
    for (int jb = 0; jb < M / 16; jb++)
      if (jb <= jmax) {  // (uniform over the wavefront)
        const double vb = Vb[(16 * jb + lr) * PS + lk + kk], wb = Wb[(16 * jb + lr) * PS + lk + kk];
        dd[jb] = kktdev::mfma_f64(va, wb, dd[jb]);
        dd[jb] = kktdev::mfma_f64(wa, vb, dd[jb]);
      }
  }
  __syncthreads();  // (the panels are read: the tile lies over them)
  double *tl = sm;
#pragma unroll
  for (int jb = 0; jb < M / 16; jb++)
    if (jb <= jmax) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int rl = 16 * wf + lk + 4 * q, sl = 16 * jb + lr, r = M * I + rl, c = M * J + sl;
        if (r < L && c >= lo && r >= c) {  // (r >= c: r >= lo and c < L; r < c: the upper half of a diagonal block)
          const double a = s.A[(size_t)r * LD + c] - dd[jb][q];
          s.A[(size_t)r * LD + c] = a;
          tl[rl * (M + 1) + sl] = a;
        }
      }
    }
  __syncthreads();
  for (int rr = t >> 6; rr < M; rr += 4) {  // entry (M I + lane, M J + rr) of the image, stored at its transposed place
    const int r = M * I + lane, c = M * J + rr;
    if (r < L && c >= lo && r > c) s.A[(size_t)c * LD + r] = tl[lane * (M + 1) + rr];
  }
}

// the work arrays of eig::ritz in device memory: what RitzLdsT holds in LDS
struct HwRitzMem {
  double *al, *be, *b2, *pv, *rv, *z;
};
__global__ void __launch_bounds__(64) k_hw_ritz(const HgDesc *__restrict__ desc, const int *__restrict__ wl, int cap, const double *__restrict__ T,
                                                double *__restrict__ rep, double *__restrict__ work) {
#pragma clang fp contract(off)
  const int k = wl[blockIdx.x], L = desc[k].nz;
  double *r = rep + (long long)HE_REPORT * k;
  if (L < 1 || L > HW_MAX || L > cap || r[HE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 5: decided by k_he_start)
  double *w = work + 6 * (size_t)cap * k;
  HwRitzMem mem{w, w + cap, w + 2 * (size_t)cap, w + 3 * (size_t)cap, w + 4 * (size_t)cap, w + 5 * (size_t)cap};
  const double *al = T + 2 * (long long)cap * k;
  eig::ritz(al, al + cap, L, r[1], r, mem);
}

}  // namespace stg
