// gfx950 kernels of hqpkkt_q_eigen_control_wide (include/hqpkkt.h) for the blocks of a plan that are 2049 .. QEW_MAX = 8192
// long - the diagonal blocks of a DOCP with thousands of states per stage -: the contract of k_qeb_block
// (q_eigen_blocked.hip.h), which serves the plan's blocks of 513 .. 2048 in the same call, with the whole chip on a few
// images at a time and ONE lower triangle of the image stored.  The method is k_qeb_block's: the blocked Householder
// reduction, lower form, dlatrd's scheme, panels of NB = 16 columns, the zero-sub-column rule, no reflector for the last two
// columns.  The execution is that of k_hw_* (staged_hess_wide.hip.h): the listed blocks are taken in batches of S slots,
// longest first, the block of slot s of a batch is wl[s]; all slots advance in lockstep, one launch moves every slot by one
// step; workgroups never wait for each other - no polled words, no grid-wide barriers, no atomics: every launch is a
// bounded piece of work and the handle's stream orders them.  A slot whose block is done (outcome 0 or 6 by k_qew_start) or
// whose length the step has passed leaves at once (uniform exits).
// The image: the 64 x 64 tiles (I, J), J <= I, of the block alone, tile after tile - tile (I, J) is number I (I + 1) / 2 + J,
// so a tile row lies in one piece -, a tile's rows side by side.  The upper half of a diagonal tile mirrors its lower half:
// no kernel masks a triangle inside a tile.  A slot (qew_slot) holds the tiles of LD / 64 tile rows (LD the plan's longest
// block rounded up to 64), the panels V and W (LD x NB, a row's NB values side by side), the vectors x (the column, then v)
// and p, the tile rows' column sums `part` (two rows of LD per tile row), the tile rows' partial sums pt and the words sc: h, and
// whether the column formed last has a reflector.
//   k_qew_gather  grid (tile rows, slots), 256 threads.  The workgroup of tile row I clears its tiles and - behind a barrier -
//                 fills them: a wavefront per row of the block, a lane per entry of row first + r of Qf; the entries with
//                 0 <= column <= r of the block are stored, those of the diagonal tile at their mirrored place too.  An entry
//                 across blocks is not loaded
//   k_qew_offsum  grid (tile rows, slots), 64 threads, lane i of tile row I the index r = 64 I + i: offsum_r in ascending j
//                 from +0.0, every add rounded on its own - row r of the triangle for j < r, column r for j > r: the entries
//                 k_qeb_block walks, in its order; g_r = a_rr - offsum_r, eig::nan_min over the butterfly, to pt[64 I]
//   k_qew_start   a workgroup per slot: g = the tile rows' values in ascending order, theta and the outcomes 0 and 6 as
//                 k_qeb_block forms them, the report's words; the block's T words past L zeroed (all of them where it is done)
//   k_qew_column  one workgroup of 1024 threads per slot; thread t stands for the indices t, t + 1024, ..
//     finish kf   (where that column has a reflector) V'v and W'v = the tile rows' parts in ascending order;
//                 p_r = fl((row part + sum_{I > tile(r)} part[2 I][r] + part[2 I + 1][r], I ascending) / h), then the earlier columns,
//                 c ascending: p_r <- fl(p_r - fl(sum_c fl(fl(V_rc (W'v)_c) + fl(W_rc (V'v)_c)) / h)); v'p of it: a butterfly per
//                 group of 64 indices, the groups in ascending order; w = p - fl(v'p / 2h) v; v and w become column i of V, W
//     form kn     x_r = a_rk out of tile column kn / 64 less the panel's earlier columns, as k_hw_column forms it: alpha_k,
//                 the zero-tail test, beta_k, v, h
//                 Behind a whole panel the host launches finish, k_qew_update, form; otherwise both in one launch
//   k_qew_pass    grid (tile rows, slots), 512 threads.  v of the tile rows that hold an index > k is staged in dynamic LDS
//                 once per workgroup, +0.0 at the indices <= k and past L: no tile needs a mask.  The workgroup of tile row I
//                 takes its tiles J = I0 .. I (I0 the tile of k + 1); wavefront w the half hf = w & 1 (rows 32 hf .. 32 hf + 31)
//                 of the tiles J = I0 + (w >> 1), + 4, ..: it loads its half ONCE, 16 rows in flight, and uses it twice - lane c
//                 keeps 32 row sums (a chain of __fma_rn over its tiles' column c, J ascending) and, for J < I, the sum of
//                 column c against v_I over its 32 rows (a chain over the rows ascending), stored to part[2 I + hf][64 J + c].
//                 Behind the tiles the 32 butterflies (kktdev::wave_sum's tree, run for all rows at once), the four
//                 wavefronts' row sums of a half in ascending order to p (undivided); and the parts of V'v and W'v (lane
//                 c < 16: column c of V, lane 16 + c: of W, the panel's earlier columns alone; wavefront w the rows 8 w ..
//                 8 w + 7 by __fma_rn, the wavefronts in order) to pt[64 I ..].  A workgroup walks the tile rows nT - 1 - x,
//                 - grid, ..: the longest first, and the grid's width changes no bits.  (v'p is the column kernel's: p is
//                 whole only there; 64 row sums per lane spill, so a wavefront takes half a tile)
//   k_qew_update  grid (tiles, slots), 256 threads, once per panel: A <- A - (V W' + W V') on v_mfma_f64_16x16x4 over the
//                 stored tiles that hold a row at or past lo = the panel's end.  The panels' rows of the tile's rows and of
//                 its columns are staged once in LDS (row stride 17); a row past L or before lo enters as +0.0.  A wavefront
//                 takes 16 x 64 as four accumulators from +0.0, k ascending, V W' before W V'.  One load and one store per
//                 element of the tile; of a diagonal tile the blocks on and below the diagonal are computed and every
//                 element below the diagonal is stored at its mirrored place too
//   k_qew_ritz    one wavefront per listed block: eig::ritz, its body unchanged, its six work arrays of cap doubles in device
//                 memory; it passes the outcomes 0 and 6 over and writes no shift - k_qe_shift adds d_b over the block's rows
// A block's bits depend on its length and its values alone - not on its slot, the batch, the grids, the mode or the other
// blocks - and are equal from call to call.  They are NOT k_qeb_block's or k_hw_*'s: the sums run over other groups.
// gfx950, hipcc -O3, by the compiler's resource remarks: k_qew_gather 24 VGPRs, k_qew_offsum 12, k_qew_start 8, no LDS;
// k_qew_column 88 VGPRs, 2 576 B of LDS; k_qew_pass 220 VGPRs, dynamic LDS alone (8 (1024 + 64 tile rows) B per launch, 73 728 B
// at most); k_qew_update 50 VGPRs, 34 816 B; k_qew_ritz 38 VGPRs, no LDS.  No scratch, no VGPR spill and no SGPR spill in any.
// No contraction; sums that fuse say __fma_rn (and the matrix pipe fuses).
// Not built: blocks over 8192; a tile row's tiles split over several workgroups of the pass; the control on the components of
// hqpkkt_q_sparse_bfgs_update.  Included by q_entries.hip behind q_eigen_blocked.hip.h.
#pragma once
#include "q_eigen_blocked.hip.h"

namespace qv {

static const int QEW_MIN = QEB_MAX + 1, QEW_MAX = 8192;  // the lengths these kernels serve (HQPKKT_QEIG_WIDE_MAX)
static const int QEW_NB = 16;                            // columns of a panel
static const int QEW_M = 64, QEW_MM = QEW_M * QEW_M;     // edge and doubles of a tile
static const int QEW_G = QEW_MAX / QEW_M;                // tile rows of the longest block
static const int QEW_NT = 1024, QEW_NW = QEW_NT / 64;    // threads and wavefronts of k_qew_column
static const int QEW_PNT = 512, QEW_PNW = QEW_PNT / 64;  // threads and wavefronts of k_qew_pass
static const int QEW_PT = 64;                            // doubles of a tile row's partial sums: 2 NB used
static const int QEW_SC = 8;                             // the slot's words: h, reflector

// doubles of one slot (ld a multiple of 64), and where its parts lie
__host__ __device__ static inline size_t qew_slot_doubles(int ld) {
  const size_t nt = (size_t)ld / QEW_M;
  return nt * (nt + 1) / 2 * QEW_MM + 2 * (size_t)ld * QEW_NB + 2 * (size_t)ld + 2 * nt * ld + (size_t)QEW_G * QEW_PT + QEW_SC;
}
// doubles of dynamic LDS of k_qew_pass on a block of length len: v, the wavefronts' row sums and panel parts
__host__ __device__ static inline size_t qew_pass_doubles(int len) { return (size_t)((len + QEW_M - 1) / QEW_M) * QEW_M + 2 * QEW_PNT; }
struct QewSlot {
  double *A, *V, *W, *x, *p, *part, *pt, *sc;
};
__device__ __forceinline__ QewSlot qew_slot(double *ws, int slot, int LD) {
  const size_t nt = (size_t)LD / QEW_M;
  QewSlot s;
  s.A = ws + (size_t)slot * qew_slot_doubles(LD);
  s.V = s.A + nt * (nt + 1) / 2 * QEW_MM, s.W = s.V + (size_t)LD * QEW_NB;
  s.x = s.W + (size_t)LD * QEW_NB, s.p = s.x + LD, s.part = s.p + LD, s.pt = s.part + 2 * nt * LD, s.sc = s.pt + (size_t)QEW_G * QEW_PT;
  return s;
}
__device__ __forceinline__ double *qew_tile(double *A, int I, int J) { return A + ((size_t)I * (I + 1) / 2 + J) * QEW_MM; }
// entry (r, c), c <= r, of the image
__device__ __forceinline__ double *qew_at(double *A, int r, int c) { return qew_tile(A, r >> 6, c >> 6) + (r & 63) * QEW_M + (c & 63); }
// the block of a slot; false: a length the host never lists
__device__ __forceinline__ bool qew_block(const int *wl, const int *boff, int LD, int cap, long long &b, int &first, int &L) {
  b = wl[blockIdx.y];
  first = boff[b], L = boff[b + 1] - first;
  return L >= 1 && L <= QEW_MAX && L <= LD && L <= cap;
}
// a block the reduction passes over: outcome 0 or 6 by k_qew_start
__device__ __forceinline__ bool qew_done(const double *rep, long long b) { return rep[QE_REPORT * b + QE_REPORT - 1] >= 0.0; }

__global__ void __launch_bounds__(256) k_qew_gather(const int *__restrict__ wl, const int *__restrict__ boff, kktdev::CsrDev Q, int cap, double *ws, int LD) {
  long long b;
  int first, L;
  const int I = blockIdx.x, t = threadIdx.x, lane = t & 63, wf = t >> 6;
  if (!qew_block(wl, boff, LD, cap, b, first, L) || QEW_M * I >= L) return;
  double *row = qew_tile(qew_slot(ws, blockIdx.y, LD).A, I, 0);  // the tiles (I, 0 .. I)
  for (int e = t; e < (I + 1) * QEW_MM; e += 256) row[e] = 0.0;
  __syncthreads();
  for (int rl = wf; rl < QEW_M && QEW_M * I + rl < L; rl += 4) {
    const int r = QEW_M * I + rl;
    for (int k = Q.ptr[first + r] + lane, e = Q.ptr[first + r + 1]; k < e; k += 64) {
      const int c = Q.col[k] - first;
      if (c < 0 || c > r) continue;
      const double v = Q.val[k];
      row[(size_t)(c >> 6) * QEW_MM + rl * QEW_M + (c & 63)] = v;
      if ((c >> 6) == I) row[(size_t)I * QEW_MM + (c & 63) * QEW_M + rl] = v;
    }
  }
}

__global__ void __launch_bounds__(64) k_qew_offsum(const int *__restrict__ wl, const int *__restrict__ boff, int cap, double *ws, int LD) {
#pragma clang fp contract(off)
  long long b;
  int first, L;
  const int I = blockIdx.x, lane = threadIdx.x, r = QEW_M * I + lane;
  if (!qew_block(wl, boff, LD, cap, b, first, L) || QEW_M * I >= L) return;
  const QewSlot s = qew_slot(ws, blockIdx.y, LD);
  double g = __builtin_inf();
  if (r < L) {
    const double *mine = qew_tile(s.A, I, 0) + lane * QEW_M;
    double off = 0.0;
    for (int j = 0; j < r; j++) off = off + fabs(mine[(size_t)(j >> 6) * QEW_MM + (j & 63)]);
    for (int j = r + 1; j < L; j++) off = off + fabs(qew_tile(s.A, j >> 6, I)[(j & 63) * QEW_M + lane]);
    g = mine[(size_t)I * QEW_MM + lane] - off;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) g = eig::nan_min(g, __shfl_xor(g, o));
  if (lane == 0) s.pt[(size_t)I * QEW_PT] = g;
}

__global__ void __launch_bounds__(256) k_qew_start(const int *__restrict__ wl, const int *__restrict__ boff, const double *__restrict__ flr, double eps2,
                                                   const double *__restrict__ bfgs, int cap, double *T, double *rep, double *ws, int LD) {
#pragma clang fp contract(off)
  const long long b = wl[blockIdx.x];
  const int L = boff[b + 1] - boff[b], t = threadIdx.x;
  double *Tb = T + 2 * (long long)cap * b, *r = rep + QE_REPORT * b;
  if (L < 1 || L > QEW_MAX || L > LD || L > cap) return;  // (never: the host lists these lengths alone and sizes LD by them)
  const QewSlot s = qew_slot(ws, blockIdx.x, LD);
  double g = s.pt[0];
  for (int w = 1; w < (L + 63) >> 6; w++) g = eig::nan_min(g, s.pt[(size_t)w * QEW_PT]);
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
  for (int k = t; k < cap; k += 256)  // (the words before L of a block that goes on: by the columns)
    if (outcome >= 0 || k >= L) Tb[k] = Tb[cap + k] = 0.0;
}

__global__ void __launch_bounds__(QEW_NT) k_qew_column(const int *__restrict__ wl, const int *__restrict__ boff, int cap, double *__restrict__ T,
                                                       const double *__restrict__ rep, double *__restrict__ ws, int LD, int kf, int kn) {
#pragma clang fp contract(off)
  constexpr int NB = QEW_NB, NT = QEW_NT, NW = QEW_NW, G = QEW_G, X0 = 2 * G;
  __shared__ double red[2 * G + 1], cf[QEW_PT];  // red: G maxima, G sums, x_0
  const long long b = wl[blockIdx.x];
  const int L = boff[b + 1] - boff[b];
  if (L < 1 || L > QEW_MAX || L > LD || L > cap || qew_done(rep, b)) return;
  const int t = threadIdx.x, lane = t & 63, wf = t >> 6, nit = (L + NT - 1) / NT, ng = (L + 63) >> 6;
  const QewSlot s = qew_slot(ws, blockIdx.x, LD);
  double *Tb = T + 2 * (long long)cap * b;
  if (kf >= 0 && kf + 2 < L && s.sc[1] != 0.0) {  // (uniform; sc is written behind this phase's barriers)
    const int i = kf & (NB - 1), I0 = (kf + 1) >> 6;
    const double h = s.sc[0];
    if (t < 2 * NB) {
      double a = s.pt[(size_t)I0 * QEW_PT + t];
      for (int I = I0 + 1; I < ng; I++) a = a + s.pt[(size_t)I * QEW_PT + t];
      cf[t] = a;
    }
    __syncthreads();
    for (int it = 0; it < nit; it++) {
      const int r = t + it * NT;
      const bool in = r > kf && r < L;
      double vp = 0.0;
      if (in) {
        const double *Vr = s.V + (size_t)r * NB, *Wr = s.W + (size_t)r * NB;
        double pr = s.p[r];
        for (int I = (r >> 6) + 1; I < ng; I++) pr = (pr + s.part[(size_t)(2 * I) * LD + r]) + s.part[(size_t)(2 * I + 1) * LD + r];
        double a = 0.0;
        for (int c = 0; c < i; c++) a = a + (Vr[c] * cf[NB + c] + Wr[c] * cf[c]);
        const double p = pr / h - a / h;
        s.p[r] = p;  // (this thread reads it again below)
        vp = s.x[r] * p;
      }
      vp = kktdev::wave_sum(vp);
      if (lane == 0) red[it * NW + wf] = vp;
    }
    __syncthreads();
    const double cc = qel_sum(red, ng) / (h + h);
    for (int r = t; r < L; r += NT)
      if (r > kf) {
        const double v = s.x[r];
        s.V[(size_t)r * NB + i] = v, s.W[(size_t)r * NB + i] = s.p[r] - cc * v;
      }
    __syncthreads();  // (red is read; the panel's column is written: form reads row kn of it)
  }
  if (kn < 0 || kn >= L) return;
  const int k = kn, i = k & (NB - 1);
  const double *Vk = s.V + (size_t)k * NB, *Wk = s.W + (size_t)k * NB;
  for (int it = 0; it < nit; it++) {  // the column as the panel's earlier columns leave it
    const int r = t + it * NT;
    double x = 0.0;
    if (r >= k && r < L) {
      const double *Vr = s.V + (size_t)r * NB, *Wr = s.W + (size_t)r * NB;
      double a = *qew_at(s.A, r, k);
      for (int c = 0; c < i; c++) a = a - (Vr[c] * Wk[c] + Wr[c] * Vk[c]);
      if (r == k)
        Tb[k] = a;
      else
        x = a;
      if (r == k + 1) red[X0] = a;
    }
    if (r < L) s.x[r] = x;
    double tail = r > k + 1 ? fabs(x) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tail = eig::nan_max(tail, __shfl_xor(tail, o));
    const double sq = kktdev::wave_sum(x * x);
    if (lane == 0) red[it * NW + wf] = tail, red[G + it * NW + wf] = sq;
  }
  if (t == 0 && k + 1 >= L) red[X0] = 0.0;  // (the last column has no x_0: beta_{L-1} = 0)
  __syncthreads();
  const double x0 = red[X0];
  double tail = red[0];
  for (int w = 1; w < ng; w++) tail = eig::nan_max(tail, red[w]);
  if (tail == 0.0) {  // (a NaN is not zero: it goes through the reflector and stays)
    if (t == 0) Tb[cap + k] = x0, s.sc[1] = 0.0;
    for (int r = k + 1 + t; r < L; r += NT) s.V[(size_t)r * NB + i] = s.W[(size_t)r * NB + i] = 0.0;
    return;
  }
  const double ss = qel_sum(red + G, ng);
  const double nrm = sqrt(ss), beta = x0 > 0.0 ? -nrm : nrm;
  if (t == ((k + 1) & (NT - 1))) s.x[k + 1] = x0 - beta;  // (the thread that wrote x_0 there)
  if (t == 0) Tb[cap + k] = beta, s.sc[0] = ss - x0 * beta, s.sc[1] = 1.0;
}

__global__ void __launch_bounds__(QEW_PNT) k_qew_pass(const int *__restrict__ wl, const int *__restrict__ boff, const double *__restrict__ rep, int cap,
                                                      double *__restrict__ ws, int LD, int k) {
#pragma clang fp contract(off)
  constexpr int NB = QEW_NB, M = QEW_M, MM = QEW_MM, NW = QEW_PNW, NT = QEW_PNT, H = M / 2;
  extern __shared__ double qew_lds[];  // the wavefronts' row sums, their parts of the panel sums, then v of the tile rows I0 ..
  long long b;
  int first, L;
  if (!qew_block(wl, boff, LD, cap, b, first, L) || qew_done(rep, b) || k + 2 >= L) return;
  const QewSlot s = qew_slot(ws, blockIdx.y, LD);
  if (s.sc[1] == 0.0) return;  // (uniform: the column has no reflector)
  double *rr = qew_lds, *pp = qew_lds + NT, *sv = qew_lds + 2 * NT;
  const int t = threadIdx.x, lane = t & 63, wf = __builtin_amdgcn_readfirstlane(t >> 6), hf = wf & 1, jw = wf >> 1;
  const int I0 = (k + 1) >> 6, nT = (L + M - 1) >> 6, base = M * I0, i = k & (NB - 1);
  for (int j = t; j < M * (nT - I0); j += NT) sv[j] = base + j > k && base + j < L ? s.x[base + j] : 0.0;
  __syncthreads();
  const bool pcol = lane < 2 * NB && (lane & (NB - 1)) < i;
  const double *P = (lane < NB ? s.V : s.W) + (lane & (NB - 1));
  for (int I = nT - 1 - (int)blockIdx.x; I >= I0; I -= (int)gridDim.x) {
    const double *trow = qew_tile(s.A, I, 0), *vI = sv + M * (I - I0);
    double sm[H];
#pragma unroll
    for (int u = 0; u < H; u++) sm[u] = 0.0;
    for (int J = I0 + jw; J <= I; J += NW / 2) {
      const double *tp = trow + (size_t)J * MM + H * hf * M;  // (uniform: the lane is the loads' offset)
      const double vj = sv[M * (J - I0) + lane];
      double cs = 0.0;
#pragma unroll
      for (int q = 0; q < H; q += 16) {
        double a[16];
#pragma unroll
        for (int u = 0; u < 16; u++) a[u] = tp[(q + u) * M + lane];
#pragma unroll
        for (int u = 0; u < 16; u++) sm[q + u] = __fma_rn(a[u], vj, sm[q + u]), cs = __fma_rn(a[u], vI[H * hf + q + u], cs);
      }
      if (J < I) s.part[(size_t)(2 * I + hf) * LD + M * J + lane] = cs;  // (uniform over the wavefront)
    }
    // the 32 butterflies at once, kktdev::wave_sum's tree for every row: the distance 32 for all of them, then at distance o
    // a lane keeps the half of its rows that its bit o names and adds what its partner holds of them; lane l ends with
    // the sum of row l & 31
#pragma unroll
    for (int u = 0; u < H; u++) sm[u] = sm[u] + __shfl_xor(sm[u], H);
#pragma unroll
    for (int o = H / 2; o > 0; o >>= 1) {
      const bool up = (lane & o) != 0;
#pragma unroll
      for (int u = 0; u < o; u++) {
        const double keep = up ? sm[u + o] : sm[u], send = up ? sm[u] : sm[u + o];
        sm[u] = keep + __shfl_xor(send, o);
      }
    }
    if (lane < H) rr[jw * M + H * hf + lane] = sm[0];
    double acc = 0.0;
    for (int u = 0; u < M / NW; u++) {
      const int r = M * I + (M / NW) * wf + u;
      if (pcol && r > k && r < L) acc = __fma_rn(P[(size_t)r * NB], vI[(M / NW) * wf + u], acc);
    }
    pp[wf * M + lane] = acc;
    __syncthreads();
    if (t < M) {
      const int r = M * I + t;
      double a = rr[t];
      for (int w = 1; w < NW / 2; w++) a = a + rr[w * M + t];
      if (r > k && r < L) s.p[r] = a;
    } else if (t < M + 2 * NB) {
      const int c = t - M;
      double a = pp[c];
      for (int w = 1; w < NW; w++) a = a + pp[w * M + c];
      s.pt[(size_t)I * QEW_PT + c] = a;
    }
    __syncthreads();
  }
}

// tile (a, b), b <= a, of number u = a (a + 1) / 2 + b
__device__ __forceinline__ void qew_tile_of(int u, int &a, int &b) {
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= u) a++;
  b = u - a * (a + 1) / 2;
}

__global__ void __launch_bounds__(256) k_qew_update(const int *__restrict__ wl, const int *__restrict__ boff, const double *__restrict__ rep, int cap,
                                                    double *__restrict__ ws, int LD, int lo) {
#pragma clang fp contract(off)
  constexpr int NB = QEW_NB, M = QEW_M, PS = NB + 1;
  __shared__ double sm[4 * M * PS];  // the panels' rows of the tile's rows and of its columns
  long long b;
  int first, L;
  if (!qew_block(wl, boff, LD, cap, b, first, L) || qew_done(rep, b) || lo >= L) return;
  int I, J;
  qew_tile_of(blockIdx.x, I, J);
  I += lo / M, J += lo / M;
  if (M * I >= L) return;
  const QewSlot s = qew_slot(ws, blockIdx.y, LD);
  const int t = threadIdx.x, lane = t & 63, wf = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  double *Va = sm, *Wa = Va + M * PS, *Vb = Wa + M * PS, *Wb = Vb + M * PS;
  for (int e = t; e < M * NB; e += 256) {
    const int row = e / NB, c = e % NB, ra = M * I + row, rb = M * J + row;
    const bool oka = ra >= lo && ra < L, okb = rb >= lo && rb < L;
    Va[row * PS + c] = oka ? s.V[(size_t)ra * NB + c] : 0.0, Wa[row * PS + c] = oka ? s.W[(size_t)ra * NB + c] : 0.0;
    Vb[row * PS + c] = okb ? s.V[(size_t)rb * NB + c] : 0.0, Wb[row * PS + c] = okb ? s.W[(size_t)rb * NB + c] : 0.0;
  }
  __syncthreads();
  const bool diag = I == J;
  const int jmax = diag ? wf : M / 16 - 1;  // (of a diagonal tile the blocks on and below the diagonal)
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
  double *tile = qew_tile(s.A, I, J);
#pragma unroll
  for (int jb = 0; jb < M / 16; jb++)
    if (jb <= jmax) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int rl = 16 * wf + lk + 4 * q, sl = 16 * jb + lr, r = M * I + rl, c = M * J + sl;
        if (r < L && c >= lo && r >= c) {  // (r >= c: r >= lo and c < L; r < c: the upper half of a diagonal block)
          const double a = tile[rl * M + sl] - dd[jb][q];
          tile[rl * M + sl] = a;
          if (diag && r != c) tile[sl * M + rl] = a;
        }
      }
    }
}

// the work arrays of eig::ritz in device memory: what RitzLdsT holds in LDS
struct QewRitzMem {
  double *al, *be, *b2, *pv, *rv, *z;
};
__global__ void __launch_bounds__(64) k_qew_ritz(const int *__restrict__ wl, const int *__restrict__ boff, int cap, const double *__restrict__ T,
                                                 double *__restrict__ rep, double *__restrict__ work) {
#pragma clang fp contract(off)
  const long long b = wl[blockIdx.x];
  const int L = boff[b + 1] - boff[b];
  double *r = rep + QE_REPORT * b;
  if (L < 1 || L > QEW_MAX || L > cap || r[QE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 6: decided by k_qew_start)
  double *w = work + 6 * (size_t)cap * blockIdx.x;
  QewRitzMem mem{w, w + cap, w + 2 * (size_t)cap, w + 3 * (size_t)cap, w + 4 * (size_t)cap, w + 5 * (size_t)cap};
  const double *al = T + 2 * (long long)cap * b;
  eig::ritz(al, al + cap, L, r[1], r, mem);
}

}  // namespace qv
