// The dense fp64 product of the STAGED engine, C = A'B on v_mfma_f64_16x16x4 for gfx950: the tile (GemmTile: operand
// staging through registers or by LDS-DMA, the k loops, the epilogue with the mirror image), the plain kernel
// (k_dgemm_tn), a thin product cut in k (k_dgemm_tn_ks), the cut form for tile counts that do not fill the chip evenly
// (k_dgemm_tn_sk) and their launches.  Which form a shape takes: gemm_form.hpp; the cut form's work lists: sk_table.hpp.
// Included by staged.hip.h (staged_engine.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gemm_schedule.hpp"

namespace stg {

using kktdev::double4_t;
using kktdev::mfma_f64;

typedef double double2_t __attribute__((ext_vector_type(2)));

// One system over several ranks (staged_plan.hpp): rank p owns the state columns [cut[p], cut[p+1]) of a stage
// (multiples of 128, so a tile lies inside one strip).  StripTab: where the ranks' local blocks of F lie once they are
// gathered - strip p = n+ rows of cut[p+1] - cut[p] columns (and the control columns behind them), row-major with
// leading dimension ld[p], at fg + off[p].
struct StripTab {
  int nranks;
  int cut[17];
  int ld[17];  // leading dimension of strip p (its width + the control columns, a multiple of 8)
  long long off[17];
};
// ... and where the blocks of G_xx lie after the second: block (a, b), a >= b, = rows of strip a x columns of strip b in
// one part, or in two cut at row rsplit (the pairs half the ring apart, staged_plan.cpp); part t row-major with leading
// dimension cut[b+1] - cut[b] at x + off[t]
struct RectTab {
  int nranks;
  int cut[17];
  struct Block {
    long long off[2];
    int rsplit;  // first row of the second part (a large number: one part)
    int pad;
  } blk[16 * 16];  // [a * 16 + b]
};
static __device__ __forceinline__ int strip_of(const int *cut, int nranks, int j) {
  int p = 0;
  while (p + 1 < nranks && cut[p + 1] <= j) p++;
  return p;
}

// A ranged operand of a product in the profile form that is stored as packed panels (StagedPlan::pk_off): per 128-column
// panel p its rows [16 lo_p, ...) alone, row-major with leading dimension ld.  off: the panel's first element from the
// operand's pointer, less 16 lo_p ld - row k of the product is row k of the panel's addressing, as in a dense block
struct PackPanel {
  long long off, ld;
};
struct GemmArgs {
  const double *A;
  long long lda;  // K x M, row-major (k-major)
  const double *B;
  long long ldb;  // K x N
  const double *Cin;
  long long ldcin;  // M x N, read when beta != 0
  double *C;
  long long ldc;
  int M, N, K;
  double alpha, beta;
  int lower;   // only tiles with tile row >= tile column (M == N)
  int mirror;  // with lower: C[j][i] = C[i][j] as well (exactly symmetric result)
  const int *tile_map;  // 128 x 128 tiles: tile index -> tile row << 16 | tile column.  Lower: in blocks of
                        // 8 x 8 tiles (neighbours in the launch order share operand panels in their XCD's L2);
                        // not lower: the tiles of a launch that computes a part of the product only (the blocks of G_xx
                        // one rank owns, bstrips); null: row by row
  const double *zeros;  // >= 128 zero doubles (16-byte aligned): the source of the operand rows k >= K when the
                        // 128 x 128 kernels stage their operands by LDS-DMA; null: staging through registers
  const RectTab *rects;        // with beta != 0: Cin(i, j), i >= j, is read from the blocks in the exchange buffer `Cin`
                               // (the rank-q update of a sharded stage takes G_xx straight from what the ranks sent)
  const StripTab *bstrips;     // the columns of B come from the ranks' strips in the exchange buffer `B` (128-wide tiles)
  unsigned long long *stamps;  // diagnostic builds of the plain kernel only (hqpkkt_debug_dgemm): 4 constant-clock
                               // (100 MHz) time stamps per workgroup: start, operands of the first slab in LDS, end of
                               // the k loop, end of the epilogue; null in every product of the engine
  // A second k segment (the 128 x 128 LDS-DMA kernels only): C = alpha (A'B + A2'B2) + beta Cin, with the slabs of
  // A2 / B2 (K2 x M / K2 x N) behind the zero-padded slabs of the first pair in the same accumulators - a launch has
  // gemm_slabs(K) + gemm_slabs(K2) slabs, and a cut piece's range may span the boundary.  V_k = F_x'W_x - Y'Rm of a
  // stage comes out of one launch this way, with B2 = -Rm (k_st_rm writes it beside Rm, so the difference is exact)
  const double *A2;
  long long lda2;
  const double *B2;
  long long ldb2;
  int K2;
  // packed panels of A / of B (k_dgemm_tn_sk<.., PACKED = true>, a GEMM_FORM_PROFILE launch alone): the tile at tile row
  // tm / tile column tn takes entry tm / tn; null: the operand is one block
  const PackPanel *apack, *bpack;
  // The control-row segment (k_dgemm_tn_sk<.., AUG = true>, a launch by a list ordered by gemm_ctrl_rows_order alone;
  // gemm_ctrl_rows_ok): Cu = Au'B, mu rows of N columns, out of the free rows of the ragged last tile row's A panels -
  // rows [0, r) of such a panel are A's, rows [r, r + mu) the columns of Au (k-major, K rows; here the columns of C that
  // the last tile column of this launch writes), the rest zero.  ctl: [0] finished tiles of the last tile column,
  // [1] launches whose segment was not ready (the guarded product behind the launch formed Cu), [2] this launch's was
  // not.  guard: a product cut in k (k_dgemm_tn_ks and its finish) returns at once while *guard is 0
  const double *Au;
  long long ldau;
  int mu;
  double *Cu;
  long long ldcu;
  unsigned *ctl;
  const unsigned *guard;
};
// the valid rows of the last tile row
static __host__ __device__ __forceinline__ int gemm_last_rows(int M) { return M - (M - 1) / 128 * 128; }
// k-slabs of a launch (both segments)
static __host__ __device__ __forceinline__ int gemm_slabs_of(const GemmArgs &g) {
  return (g.K + GEMM_BK - 1) / GEMM_BK + (g.K2 > 0 ? (g.K2 + GEMM_BK - 1) / GEMM_BK : 0);
}

static inline size_t gemm_lds_bytes(int bm, int bn, int nbuf = 2) { return sizeof(double) * nbuf * GEMM_BK * (size_t)(bm + 16 + bn + 16); }

// blockIdx -> position in a sequence in which the workgroups of one XCD (blockIdx % 8) are
// neighbours (each XCD has its own L2; neighbouring tiles share operand panels)
__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return x * q + (x < r ? x : r) + (bid >> 3);
}

// One workgroup (256 threads, 2 x 2 wavefronts) per BM x BN tile of C; k-slabs of 16 rows
// of both operands go global -> registers -> LDS (two buffers: the loads of slab t+1 are in
// flight while slab t is multiplied), fragments LDS -> registers with ds_read_b64, conflict
// free because an LDS row is BM + 16 doubles (rows k, k+1 of a fragment: banks 32 apart).
// WGM x WGN wavefronts per workgroup (2 x 2: 64 x 64 per wave, 16 accumulator tiles = 128 registers, two waves
// per SIMD; 2 x 4: 64 x 32 per wave, 8 accumulator tiles, under 128 registers, FOUR waves per SIMD with two
// workgroups per CU - one wave issues a v_mfma_f64_16x16x4 only every ~140 cycles (stamps of the 2 x 2 kernel:
// every workgroup proceeds at that pace whoever its partner is, profiles/r03_dgemm_stamps.txt), the pipe takes
// one per 64, so two waves per SIMD top out near 90 % of the peak and it takes three or four to fill it)
template <int BM, int BN, int WGM = 2, int WGN = 2>
struct GemmTile {
  static constexpr int BK = GEMM_BK;
  static constexpr int NW = WGM * WGN, NT = 64 * NW;
  static constexpr int LDA = BM + 16, LDB = BN + 16;
  static constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 16, TN = WN / 16;
  static constexpr int LA = BK * BM / 2 / 256, LB = BK * BN / 2 / 256;  // 16-byte loads per thread and slab
  static constexpr int RA = 256 / (BM / 2), RB = 256 / (BN / 2);        // slab rows covered by one pass

  // tile index -> (tile row, tile column)
  static __device__ __forceinline__ void tile_of(const GemmArgs &g, int t, int &tm, int &tn) {
    if (g.tile_map && BM == 128) {
      const int e = g.tile_map[t];
      tm = e >> 16, tn = e & 0xffff;
    } else if (g.lower) {
      const int tcols = (g.N + BN - 1) / BN, tri = tcols * (tcols + 1) / 2;
      if (t < tri) {
        tm = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
        while ((tm + 1) * (tm + 2) / 2 <= t) tm++;
        while (tm * (tm + 1) / 2 > t) tm--;
        tn = t - tm * (tm + 1) / 2;
      } else {  // (M > N: the rectangle below the triangle, row by row)
        tm = tcols + (t - tri) / tcols;
        tn = (t - tri) % tcols;
      }
    } else {
      const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
      constexpr int GM = 8;  // tile rows walked together: their A panels stay in L2
      const int grp = t / (GM * tiles_n), first = grp * GM;
      const int rows = min(GM, tiles_m - first);
      const int in = t - grp * GM * tiles_n;
      tm = first + in % rows;
      tn = in / rows;
    }
  }

  // acc += sum over the slabs [s0, s1) of the tile at (i0, j0); ends with a barrier (LDS free again)
  template <bool PACKED = false>
  static __device__ __forceinline__ void accumulate(const GemmArgs &g, int i0, int j0, int s0, int s1,
                                                    double4_t (&acc)[TM][TN], double *As, double *Bs) {
    static_assert(NT == 256, "the register-staged loop is written for 256 threads");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, lk = lane >> 4;
    // global -> register staging: thread covers columns ca, ca+1 of rows ra + p*RA
    const int ca = 2 * (tid % (BM / 2)), ra = tid / (BM / 2);
    const int cb = 2 * (tid % (BN / 2)), rb = tid / (BN / 2);
    // a 16-byte load is inside its row when its first column is < ld (ld even)
    const double *Ap = g.A;
    long long lda = g.lda;
    int ia = i0;  // first column of the tile inside its A block
    const double *Bp = g.B;
    long long ldb = g.ldb;
    int jb = j0;  // first column of the tile inside its B block
    if (g.bstrips) {
      const int q = strip_of(g.bstrips->cut, g.bstrips->nranks, j0);
      Bp = g.B + g.bstrips->off[q], ldb = g.bstrips->ld[q], jb = j0 - g.bstrips->cut[q];
    }
    if constexpr (PACKED) {  // (a panel is a tile wide: the tile starts at its column 0)
      static_assert(BM == 128 && BN == 128, "a packed panel is one 128-wide tile column");
      if (g.apack) Ap = g.A + g.apack[i0 / BM].off, lda = g.apack[i0 / BM].ld, ia = 0;
      if (g.bpack) Bp = g.B + g.bpack[j0 / BN].off, ldb = g.bpack[j0 / BN].ld, jb = 0;
    }
    const long long acol = (ia + ca < lda) ? ia + ca : 0;
    const long long bcol = (jb + cb < ldb) ? jb + cb : 0;
    // D register sets: the loads of slab t + D are issued before the multiplications of slab t and consumed (masked
    // for k >= K, stored to LDS) after those of slab t + D - 1.  With 64 x 64 tiles a slab is 16 multiplications per
    // wavefront (0.4 us) and a load from L2 takes 1.4: one set (round 2) left the loop waiting for its loads - 1.44 us
    // per slab (profiles: 272 tiles of a 1000-state stage in 91 us); the 128 x 128 form of this loop keeps one set
    // (its slab is four times the work, its sets four times the registers).
    constexpr int D = (BM * BN <= 64 * 64) ? 4 : 1;
    double2_t sa[D][LA], sb[D][LB];
    // (no branch anywhere in the loop: rows k >= K are read from row K - 1 and zeroed on their way to LDS, slabs
    // behind the last one are the last one again and go to a buffer nobody reads - with branches between the loads and
    // their use the compiler waits for ALL loads in flight at every join, also those just issued)
    const int last = s1 - 1;
    auto gload = [&](double2_t(&xa)[LA], double2_t(&xb)[LB], int slab) {
      const int k0 = (slab < last ? slab : last) * BK;
#pragma unroll
      for (int p = 0; p < LA; p++) {
        const int k = k0 + ra + p * RA, kc = k < g.K ? k : g.K - 1;
        xa[p] = *(const double2_t *)(Ap + (long long)kc * lda + acol);
      }
#pragma unroll
      for (int p = 0; p < LB; p++) {
        const int k = k0 + rb + p * RB, kc = k < g.K ? k : g.K - 1;
        xb[p] = *(const double2_t *)(Bp + (long long)kc * ldb + bcol);
      }
    };
    auto lstore = [&](int buf, const double2_t(&xa)[LA], const double2_t(&xb)[LB], int slab) {
      const int k0 = (slab < last ? slab : last) * BK;
#pragma unroll
      for (int p = 0; p < LA; p++) {
        double2_t v = xa[p];
        if (k0 + ra + p * RA >= g.K) v = (double2_t){0.0, 0.0};
        *(double2_t *)(As + (buf * BK + ra + p * RA) * LDA + ca) = v;
      }
#pragma unroll
      for (int p = 0; p < LB; p++) {
        double2_t v = xb[p];
        if (k0 + rb + p * RB >= g.K) v = (double2_t){0.0, 0.0};
        *(double2_t *)(Bs + (buf * BK + rb + p * RB) * LDB + cb) = v;
      }
    };
    auto multiply = [&](int buf) {
      const double *Ab = As + buf * BK * LDA + wm * WM + lr;
      const double *Bb = Bs + buf * BK * LDB + wn * WN + lr;
#pragma unroll
      for (int ks = 0; ks < BK / 4; ks++) {
        double af[TM], bf[TN];
#pragma unroll
        for (int x = 0; x < TM; x++) af[x] = Ab[(ks * 4 + lk) * LDA + 16 * x];
#pragma unroll
        for (int y = 0; y < TN; y++) bf[y] = Bb[(ks * 4 + lk) * LDB + 16 * y];
#pragma unroll
        for (int x = 0; x < TM; x++)
#pragma unroll
          for (int y = 0; y < TN; y++) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
      }
    };
    if (s1 <= s0) return;  // (uniform)
#pragma unroll
    for (int d = 0; d < D; d++) gload(sa[d], sb[d], s0 + d);
    lstore(0, sa[0], sb[0], s0);
    __syncthreads();
    // whole groups of D slabs (D even or 1: the LDS buffer of a step is its position in the group, mod 2), straight-line
    int s = s0;
    for (; s + D <= s1; s += D) {
#pragma unroll
      for (int d = 0; d < D; d++) {
        const int buf = d & 1;
        gload(sa[d], sb[d], s + d + D);  // set d: its slab went to LDS one step ago
        multiply(D == 1 ? ((s - s0) & 1) : buf);
        lstore(D == 1 ? (((s - s0) & 1) ^ 1) : (buf ^ 1), sa[(d + 1) % D], sb[(d + 1) % D], s + d + 1);
        __syncthreads();
      }
    }
    // the remaining 0 .. D - 1 slabs one by one (set (s - s0) % D holds slab s + 1 ... the sets rotate as above)
#pragma unroll
    for (int d = 0; d < D - 1; d++) {
      if (s + d < s1) {  // (uniform)
        multiply((D == 1 ? (s + d - s0) : d) & 1);
        if (s + d + 1 < s1) lstore(((D == 1 ? (s + d - s0) : d) & 1) ^ 1, sa[(d + 1) % D], sb[(d + 1) % D], s + d + 1);
        __syncthreads();
      }
    }
  }

  // The same with the operand slabs brought global -> LDS by the DMA path (global_load_lds_dwordx4: no
  // staging registers, no ds_write, no vector ALU work besides the address of a row), 128-wide tiles only: a
  // k-row of a panel is 128 doubles = the 1 KiB one wave-instruction writes (lane l -> bytes 16 l .. 16 l + 15
  // behind a wave-uniform LDS address), so padded LDS rows are no obstacle.  Wave w brings the rows w, w + 4,
  // w + 8, w + 12 of both panels: 8 instructions per wave and slab, issued BETWEEN the first 16 multiplications
  // of the slab before (one per two v_mfma_f64_16x16x4, which take 64 cycles each), into the buffer the
  // barrier at the end of the slab before has released; they have the rest of the slab (~4000 cycles) to land
  // and are waited for (vmcnt(0)) in front of the barrier that ends the slab.  Rows k >= K come from g.zeros,
  // so the last, partial slab needs no masking; behind the last slab of the range the same 8 instructions
  // copy zero rows into the buffer nobody reads any more (no branch in the loop).
  // Per slab a wave is outside its MFMA stream only for the barrier and the latency of its first fragment
  // reads: the register-staged loop above spends ~150 vector instructions per slab on addresses, masks and
  // ds_write_b128 behind the last MFMA, during which the matrix pipe has nothing from this wave (two
  // workgroups per CU that started together stay in step, so the partner wave is in the same phase).
  static __device__ __forceinline__ void glds16(const double *src, double *lds_row) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_row, 16, 0, 0);
  }
  // `skip_upper`: the tile lies on the diagonal of a lower-triangular product - its 16 x 16 blocks strictly above the
  // diagonal are not needed.  Blocks of 16 rows / columns beyond M / N (the ragged last tile row and column: 5000 = 39 x
  // 128 + 8) and those blocks are left out of the multiplications: a wave whose blocks are all wanted runs the plain
  // loop, the others a copy of it with a (wave-uniform, scalar) test in front of every MFMA.  The operands are staged
  // and the barriers kept as always; what is saved is the matrix pipe's time, which the partner workgroup of the CU
  // gets (3.8 % of W's and 5.3 % of G's multiplications at the C4 shapes).
  // The k-rows of one operand of a launch: rows [0, K) from the first segment (leading dimension ld), rows [k0, k1) -
  // k0 = the first segment's slabs x BK - from the second (GemmArgs::K2; row k at offset o2 + k ld2 from the first's
  // origin), every other row from the zero row.  Without a second segment k0 = k1.
  struct Rows {
    int K, k0, k1;
    long long ld, o2, ld2;
  };
  static __device__ __forceinline__ const double *row_of(const Rows &r, const double *p, const double *zr, int k) {
    return k < r.K ? p + (long long)k * r.ld : (k >= r.k0 && k < r.k1) ? p + (r.o2 + (long long)k * r.ld2) : zr;
  }
  template <bool MASKED>
  static __device__ __forceinline__ void slabs_dma(const Rows &ra, const Rows &rb, const double *pa, const double *pb, const double *zr, int wave,
                                                   int wm, int wn, int lr, int lk, int s0, int s1, unsigned mask,
                                                   double4_t (&acc)[TM][TN], double *As, double *Bs) {
    constexpr int RPW = BK / NW;  // rows of each panel per wave and slab
    // piece p of the slab that starts at row k0 -> buffer buf: row wave + NW (p % RPW) of A (p < RPW) or B
    auto dma = [&](int buf, int k0, int p) {
      const int r = wave + NW * (p % RPW), k = k0 + r;
      if (p < RPW)
        glds16(row_of(ra, pa, zr, k), As + (buf * BK + r) * LDA);
      else
        glds16(row_of(rb, pb, zr, k), Bs + (buf * BK + r) * LDB);
    };
    if (s1 > s0) {
#pragma unroll
      for (int p = 0; p < 2 * RPW; p++) dma(0, s0 * BK, p);
    }
    __syncthreads();  // (waits for the DMA: vmcnt(0))
    constexpr int GAP = TM * TN / (2 * RPW);  // multiplications between two pieces
    // (measured and dropped: the waves w and w + 4, which share a SIMD, issuing their pieces two k-steps apart: 8192^3
    // 90.8 -> 88.3 % of peak)
    for (int s = s0; s < s1; s++) {
      const int buf = (s - s0) & 1;
      const int knext = s + 1 < s1 ? (s + 1) * BK : ra.k1;  // behind the last slab: zero rows
      const double *Ab = As + buf * BK * LDA + wm * WM + lr;
      const double *Bb = Bs + buf * BK * LDB + wn * WN + lr;
#pragma unroll
      for (int ks = 0; ks < BK / 4; ks++) {
        double af[TM], bf[TN];
#pragma unroll
        for (int x = 0; x < TM; x++) af[x] = Ab[(ks * 4 + lk) * LDA + 16 * x];
#pragma unroll
        for (int y = 0; y < TN; y++) bf[y] = Bb[(ks * 4 + lk) * LDB + 16 * y];
#pragma unroll
        for (int x = 0; x < TM; x++)
#pragma unroll
          for (int y = 0; y < TN; y++) {
            if (!MASKED || ((mask >> (x * TN + y)) & 1u)) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
            if (ks == 0 && (x * TN + y) % GAP == GAP - 1) dma(buf ^ 1, knext, (x * TN + y) / GAP);
          }
      }
      __syncthreads();
    }
  }
  // The same loop over THREE LDS buffers (110 KB: one workgroup per CU): the DMA of slab s + 2 is issued during slab s
  // and has two slab times to land - with two buffers the DMA of slab s + 1, issued at the start of slab s, is waited
  // for at its end, and under load (every CU streaming its panels out of L2) its 1-2 us do not always fit into the
  // 1.7 us a slab takes a workgroup that has the CU to itself.  Counted wait: vmcnt(2 RPW) leaves the newest slab's
  // pieces in flight across the barrier (raw s_barrier: __syncthreads() would drain them).  As / Bs: 3 BK rows each.
  template <bool MASKED>
  static __device__ __forceinline__ void slabs_dma3(const Rows &ra, const Rows &rb, const double *pa, const double *pb, const double *zr, int wave,
                                                    int wm, int wn, int lr, int lk, int s0, int s1, unsigned mask,
                                                    double4_t (&acc)[TM][TN], double *As, double *Bs) {
    constexpr int RPW = BK / NW;
    static_assert(2 * RPW == 4 || 2 * RPW == 8, "the counted waits below are written for 4 or 8 pieces per wave and slab");
    auto dma = [&](int buf, int k0, int p) {
      const int r = wave + NW * (p % RPW), k = k0 + r;
      if (p < RPW)
        glds16(row_of(ra, pa, zr, k), As + (buf * BK + r) * LDA);
      else
        glds16(row_of(rb, pb, zr, k), Bs + (buf * BK + r) * LDB);
    };
    auto wait_all_but_newest_slab = [&]() {
      if constexpr (2 * RPW == 4)
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    // slabs s0 and s0 + 1 (zero rows where the range is shorter) -> buffers 0 and 1
#pragma unroll
    for (int p = 0; p < 2 * RPW; p++) dma(0, s1 > s0 ? s0 * BK : ra.k1, p);
#pragma unroll
    for (int p = 0; p < 2 * RPW; p++) dma(1, s0 + 1 < s1 ? (s0 + 1) * BK : ra.k1, p);
    wait_all_but_newest_slab();
    constexpr int GAP = TM * TN / (2 * RPW);
    int buf = 0;
    for (int s = s0; s < s1; s++) {
      const int bnext = buf >= 1 ? buf - 1 : 2;  // (buf + 2) % 3
      const int knext = s + 2 < s1 ? (s + 2) * BK : ra.k1;
      const double *Ab = As + buf * BK * LDA + wm * WM + lr;
      const double *Bb = Bs + buf * BK * LDB + wn * WN + lr;
#pragma unroll
      for (int ks = 0; ks < BK / 4; ks++) {
        double af[TM], bf[TN];
#pragma unroll
        for (int x = 0; x < TM; x++) af[x] = Ab[(ks * 4 + lk) * LDA + 16 * x];
#pragma unroll
        for (int y = 0; y < TN; y++) bf[y] = Bb[(ks * 4 + lk) * LDB + 16 * y];
#pragma unroll
        for (int x = 0; x < TM; x++)
#pragma unroll
          for (int y = 0; y < TN; y++) {
            if (!MASKED || ((mask >> (x * TN + y)) & 1u)) acc[x][y] = mfma_f64(af[x], bf[y], acc[x][y]);
            if (ks == 0 && (x * TN + y) % GAP == GAP - 1) dma(bnext, knext, (x * TN + y) / GAP);
          }
      }
      wait_all_but_newest_slab();
      buf = buf == 2 ? 0 : buf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the zero rows behind the range: LDS is reused after this)
    __syncthreads();
  }
  template <bool PACKED = false>
  static __device__ __forceinline__ void accumulate_dma(const GemmArgs &g, int i0, int j0, int s0, int s1,
                                                        double4_t (&acc)[TM][TN], double *As, double *Bs, bool skip_upper = false, int nbuf = 2) {
    static_assert(BM == 128 && BN == 128, "one k-row of a panel must be one 1-KiB wave-instruction");
    static_assert((BK / NW) * NW == BK && TM * TN >= 2 * (BK / NW) && TM * TN <= 32,
                  "pieces are issued behind the multiplications of the first k-step");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, lk = lane >> 4;
    unsigned mask = 0;
#pragma unroll
    for (int x = 0; x < TM; x++)
#pragma unroll
      for (int y = 0; y < TN; y++) {
        const int rb = wm * TM + x, cb = wn * TN + y;  // 16 x 16 block of the tile
        const bool want = i0 + 16 * rb < g.M && j0 + 16 * cb < g.N && !(skip_upper && cb > rb);
        mask |= (want ? 1u : 0u) << (x * TN + y);
      }
    mask = __builtin_amdgcn_readfirstlane(mask);
    const bool all = mask == (TM * TN == 32 ? 0xffffffffu : (1u << (TM * TN)) - 1u);
    // a 16-byte load is inside its row when its first column is < ld (ld even)
    const double *B = g.B;
    long long ldb = g.ldb;  // (B and its leading dimension: the strip of the tile's columns)
    int jb = j0;
    if (g.bstrips) {
      const int q = strip_of(g.bstrips->cut, g.bstrips->nranks, j0);
      B = g.B + g.bstrips->off[q], ldb = g.bstrips->ld[q], jb = j0 - g.bstrips->cut[q];
    }
    const double *A = g.A;
    long long lda = g.lda;
    int ia = i0;
    if constexpr (PACKED) {  // (a panel is a tile wide: the tile starts at its column 0)
      if (g.apack) A = g.A + g.apack[i0 / BM].off, lda = g.apack[i0 / BM].ld, ia = 0;
      if (g.bpack) B = g.B + g.bpack[j0 / BN].off, ldb = g.bpack[j0 / BN].ld, jb = 0;
    }
    const double *pa = A + ((ia + 2 * lane < lda) ? ia + 2 * lane : 0);
    const double *pb = B + ((jb + 2 * lane < ldb) ? jb + 2 * lane : 0);
    const double *zr = g.zeros + 2 * lane;
    // (the second segment's rows are addressed from the first's origin: the same column of the tile in both; not with bstrips)
    const int k0 = (g.K + BK - 1) / BK * BK, k1 = k0 + (g.K2 > 0 ? g.K2 : 0);
    Rows ra{g.K, k0, k1, lda, 0, 0}, rb{g.K, k0, k1, ldb, 0, 0};
    if (g.K2 > 0) {
      ra.ld2 = g.lda2, ra.o2 = (g.A2 - g.A) - (long long)k0 * g.lda2;
      rb.ld2 = g.ldb2, rb.o2 = (g.B2 - g.B) - (long long)k0 * g.ldb2;
    }
    if (nbuf == 3) {
      if (all)
        slabs_dma3<false>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
      else
        slabs_dma3<true>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
    } else if (all)
      slabs_dma<false>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
    else
      slabs_dma<true>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
  }

  // A tile of the ragged last tile row with the control-row segment (GemmArgs::Au): the same loops, with the row of
  // the A panel chosen per LANE - the lanes of the panel columns < r read A as always, those of the columns
  // [r, r + mu) row k of Au (`ready`: the tiles that write it have finished; otherwise the zero row), the others the
  // zero row.  mu odd: the lane of columns r + mu - 1, r + mu brings one value from beyond Au's columns into panel row
  // r + mu, whose products nobody writes.  Always the masked loop: the blocks of the rows [0, r + mu)
  static __device__ __forceinline__ void accumulate_dma_aug(const GemmArgs &g, int i0, int j0, int s0, int s1, bool ready,
                                                            double4_t (&acc)[TM][TN], double *As, double *Bs, int nbuf) {
    static_assert(BM == 128 && BN == 128, "one k-row of a panel must be one 1-KiB wave-instruction");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, lk = lane >> 4;
    const int r = g.M - i0, rows = ready ? r + g.mu : r;
    unsigned mask = 0;
#pragma unroll
    for (int x = 0; x < TM; x++)
#pragma unroll
      for (int y = 0; y < TN; y++) {
        const int rb = wm * TM + x, cb = wn * TN + y;
        mask |= ((16 * rb < rows && j0 + 16 * cb < g.N) ? 1u : 0u) << (x * TN + y);
      }
    mask = __builtin_amdgcn_readfirstlane(mask);
    const double *zr = g.zeros + 2 * lane;
    const int c = 2 * lane;
    const bool mine = c < r, theirs = !mine && c < rows;
    const double *pa = mine ? g.A + ((i0 + c < g.lda) ? i0 + c : 0) : theirs ? g.Au + (c - r) : zr;
    const double *pb = g.B + ((j0 + c < g.ldb) ? j0 + c : 0);
    const int k0 = (g.K + BK - 1) / BK * BK;
    const Rows ra{g.K, k0, k0, mine ? g.lda : theirs ? g.ldau : 0, 0, 0}, rb{g.K, k0, k0, g.ldb, 0, 0};
    if (nbuf == 3)
      slabs_dma3<true>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
    else
      slabs_dma<true>(ra, rb, pa, pb, zr, wave, wm, wn, lr, lk, s0, s1, mask, acc, As, Bs);
  }
  // ... and its epilogue: rows [0, r) of the tile to C (`plain`), rows [r, r + mu) to Cu (`ctrl`), nothing else (alpha
  // alone: a launch with the segment has beta = 0)
  static __device__ __forceinline__ void epilogue_aug(const GemmArgs &g, int tm, int tn, const double4_t (&acc)[TM][TN], bool plain, bool ctrl) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, lk = lane >> 4;
    const int i0 = tm * BM, j0 = tn * BN, r = g.M - i0;
#pragma unroll
    for (int x = 0; x < TM; x++)
#pragma unroll
      for (int y = 0; y < TN; y++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int ii = wm * WM + 16 * x + lk + 4 * rg, j = j0 + wn * WN + 16 * y + lr;
          if (j >= g.N) continue;
          const double v = g.alpha * acc[x][y][rg];
          if (ii < r) {
            if (plain) g.C[(long long)(i0 + ii) * g.ldc + j] = v;
          } else if (ii < r + g.mu && ctrl)
            g.Cu[(long long)(ii - r) * g.ldcu + j] = v;
        }
  }

  // `lds`: the workgroup's LDS (free after accumulate's last barrier), used to write the MIRROR image of an
  // off-diagonal tile in whole rows: the values of 64 tile columns at a time go to LDS transposed ([column][row],
  // leading dimension BM + 2: conflict-free), and every wave then writes rows of the mirrored block in 1-KiB (BM = 128)
  // pieces - written element by element the image costs one 32-byte sector per value (the rank-q update V = G_xx -
  // Y'Rm of a C4 stage, which is nothing but reading G and writing V and its image: 158 us, 1.9 TB/s).  All threads
  // of the workgroup must call (barriers inside when g.mirror is set).
  static __device__ __forceinline__ void epilogue(const GemmArgs &g, int tm, int tn, const double4_t (&acc)[TM][TN], double *lds) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, lk = lane >> 4;
    const int i0 = tm * BM, j0 = tn * BN;
    const bool diag = g.lower && tm == tn;
    const double *cin = g.Cin;
    long long ldcin = g.ldcin;
    if (g.rects && g.beta != 0.0) {  // the block (part) that holds this tile
      const RectTab &R = *g.rects;
      const int a = strip_of(R.cut, R.nranks, i0), b = strip_of(R.cut, R.nranks, j0);
      const RectTab::Block &blk = R.blk[a * 16 + b];
      const int t = i0 >= blk.rsplit ? 1 : 0, r0 = t ? blk.rsplit : R.cut[a], c0 = R.cut[b];
      ldcin = R.cut[b + 1] - c0;
      cin = g.Cin + blk.off[t] - ((long long)r0 * ldcin + c0);
    }
    constexpr int HC = BN < 64 ? BN : 64, LDT = BM + 2;  // columns per pass of the mirrored write
    const bool via_lds = g.mirror && !diag && lds != nullptr;
    double4_t val[TM][TN];
#pragma unroll
    for (int x = 0; x < TM; x++)
#pragma unroll
      for (int y = 0; y < TN; y++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int i = i0 + wm * WM + 16 * x + lk + 4 * rg, j = j0 + wn * WN + 16 * y + lr;
          double v = 0.0;
          if (i < g.M && j < g.N && !(diag && i < j)) {
            v = g.alpha * acc[x][y][rg];
            if (g.beta != 0.0) v += g.beta * cin[(long long)i * ldcin + j];
            g.C[(long long)i * g.ldc + j] = v;
            if (g.mirror && i != j && !via_lds) g.C[(long long)j * g.ldc + i] = v;
          }
          val[x][y][rg] = v;
        }
    if (via_lds) {  // (uniform for the workgroup)
#pragma unroll
      for (int h = 0; h < BN / HC; h++) {
        if ((wn * WN) / HC == h) {
#pragma unroll
          for (int x = 0; x < TM; x++)
#pragma unroll
            for (int y = 0; y < TN; y++)
#pragma unroll
              for (int rg = 0; rg < 4; rg++)
                lds[(wn * WN - h * HC + 16 * y + lr) * LDT + wm * WM + 16 * x + lk + 4 * rg] = val[x][y][rg];
        }
        __syncthreads();
        // row jj of the image = column j0 + h HC + jj of the tile: BM values, two per lane and row
        for (int jj = wave; jj < HC; jj += NW) {
          const int j = j0 + h * HC + jj;
          if (j >= g.N) break;
          for (int ii = 2 * lane; ii < BM; ii += 128) {
            const int i = i0 + ii;
            double *dst = g.C + (long long)j * g.ldc + i;
            if (i + 1 < g.M && (((size_t)dst) & 15) == 0)
              *(double2_t *)dst = *(const double2_t *)(lds + jj * LDT + ii);
            else {
              if (i < g.M) dst[0] = lds[jj * LDT + ii];
              if (i + 1 < g.M) dst[1] = lds[jj * LDT + ii + 1];
            }
          }
        }
        __syncthreads();
      }
    }
  }
};

// wavefronts per SIMD the launch is compiled for: two workgroups per CU (one with three LDS buffers)
// (A 256 x 128 tile on 4 x 4 wavefronts, one workgroup per CU, was written and measured in round 4 - commit 44e8e46,
// profiles/r04_tile256_ab.txt: 88.4 % of the peak at 8192^3 against 89.7 % of the 2 x 4 form, 64 % against 79.5 % on
// the 800 tiles of a C4 stage's W - and taken out again; in the split form (whole rounds + cut remainder) it reaches
// 80.7 % on W against 81.0 % of the form in use: the shape's ceiling - 313 slabs per tile, ragged last tile row and
// column - not the pairing of workgroups, is what holds W at 81 %.)
constexpr int gemm_waves_per_simd(int nw, int nbuf) { return nbuf == 3 ? nw / 4 : nw / 2; }
template <int BM, int BN, bool DMA = false, int WGM = 2, int WGN = 2, int NBUF = 2>
__global__ void __launch_bounds__(64 * WGM * WGN, gemm_waves_per_simd(WGM * WGN, NBUF)) k_dgemm_tn(GemmArgs g) {
  using T = GemmTile<BM, BN, WGM, WGN>;
  extern __shared__ __attribute__((aligned(16))) double lds[];  // NBUF * BK * (LDA + LDB) doubles
  double *As = lds, *Bs = lds + NBUF * T::BK * ((DMA && BM == 64) ? 64 : T::LDA);  // (the 64 x 64 DMA form: unpadded rows)
  int tm, tn;
  const unsigned long long t0 = g.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
  T::tile_of(g, xcd_swizzle(blockIdx.x, gridDim.x), tm, tn);
  double4_t acc[T::TM][T::TN];
#pragma unroll
  for (int x = 0; x < T::TM; x++)
#pragma unroll
    for (int y = 0; y < T::TN; y++) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
  if constexpr (DMA)
    T::accumulate_dma(g, tm * BM, tn * BN, 0, gemm_slabs_of(g), acc, As, Bs, g.lower && tm == tn, NBUF);
  else
    T::accumulate(g, tm * BM, tn * BN, 0, (g.K + T::BK - 1) / T::BK, acc, As, Bs);
  const unsigned long long t2 = g.stamps ? __builtin_amdgcn_s_memrealtime() : 0;
  T::epilogue(g, tm, tn, acc, lds);
  if (g.stamps && threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g.stamps[4 * blockIdx.x + 0] = t0, g.stamps[4 * blockIdx.x + 1] = (unsigned long long)(xcc & 15);
    g.stamps[4 * blockIdx.x + 2] = t2, g.stamps[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
  }
}

// A THIN product - a handful of tiles, thousands of k (the control rows of G: 50 x 690 x 5000; the carried rows) - is a
// chain of 313 slabs in each of its few workgroups: 330 us for 0.3 GFlop.  Cut in k: workgroup (tile, y) sums the slabs
// of piece y into part[y] (M x N, raw sums), k_dgemm_ks_finish adds the pieces in their order (reproducible) and applies
// alpha / beta.  Not lower, not mirrored; register-staged 64-wide tiles.
template <int BM, int BN>
__global__ void __launch_bounds__(256) k_dgemm_tn_ks(GemmArgs g, double *__restrict__ part, int nsplit) {
  using T = GemmTile<BM, BN, 2, 2>;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if (g.guard && *g.guard == 0) return;  // (uniform: a guarded product whose result exists already)
  double *As = lds, *Bs = lds + 2 * T::BK * T::LDA;
  int tm, tn;
  T::tile_of(g, blockIdx.x, tm, tn);
  const int nslab = (g.K + T::BK - 1) / T::BK, L = (nslab + nsplit - 1) / nsplit;
  const int s0 = min(nslab, (int)blockIdx.y * L), s1 = min(nslab, s0 + L);
  double4_t acc[T::TM][T::TN];
#pragma unroll
  for (int x = 0; x < T::TM; x++)
#pragma unroll
    for (int y = 0; y < T::TN; y++) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
  T::accumulate(g, tm * BM, tn * BN, s0, s1, acc, As, Bs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave / 2, wn = wave % 2, lr = lane & 15, lk = lane >> 4;
  double *out = part + (long long)blockIdx.y * g.M * g.N;
#pragma unroll
  for (int x = 0; x < T::TM; x++)
#pragma unroll
    for (int y = 0; y < T::TN; y++)
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const int i = tm * BM + wm * T::WM + 16 * x + lk + 4 * rg, j = tn * BN + wn * T::WN + 16 * y + lr;
        if (i < g.M && j < g.N) out[(long long)i * g.N + j] = acc[x][y][rg];
      }
}
__global__ void k_dgemm_ks_finish(GemmArgs g, const double *__restrict__ part, int nsplit) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x, tot = (long long)g.M * g.N;
  if (e >= tot || (g.guard && *g.guard == 0)) return;
  double s = 0.0;
  for (int y = 0; y < nsplit; y++) s += part[(long long)y * tot + e];
  const int i = (int)(e / g.N), j = (int)(e % g.N);
  double v = g.alpha * s;
  if (g.beta != 0.0) v += g.beta * g.Cin[(long long)i * g.ldcin + j];
  g.C[(long long)i * g.ldc + j] = v;
}

// The same product for tile counts that do not fill the chip evenly (1600 tiles on 512 workgroup
// slots: the last of four rounds would be an eighth full; 100 tiles of a column slice: a fifth of
// the slots busy for a whole tile time).  A fixed grid of G workgroups (two per CU) walks a LIST of units made by
// the host (sk_table.hpp): a unit is a tile's k-slabs [s0, s1) - the whole tile, or piece j of `pieces` of it.  Every
// schedule is such a list: whole tiles with unequal shares for the two workgroups of a CU and the remainder cut, whole
// rounds and cut phases with equal shares, or the k-slabs of all tiles as one sequence (gemm_choose_list).
// The pieces of a tile park their partial sums (plain stores, then an agent-scope release and one
// counter add); the workgroup that arrives last adds all of them in the order of the k ranges (its
// own comes back from memory too: one code path, one order) and writes the tile: the result does not
// depend on the order of arrival, nor on who computes what, and nobody waits for anybody.
struct SplitPlan {
  double *ws;           // parked partial tiles: piece j of a tile -> ws + (slot0 + j) * 128 * 128 (SkUnit::slot0)
  unsigned *cnt;        // arrival counter per tile (zero between launches: the last arriver of a tile resets it)
  const SkUnit *table;  // workgroup b (blockIdx.x) does table[b * stride + i], i = 0 ... until a tile < 0
  int stride;
};
// PACKED: the ranged operand of a profile launch comes from packed panels (GemmArgs::apack / bpack) - instances of
// their own: the others take every operand as one block
// AUG: the launch carries the control-row segment (GemmArgs::Au; the list and tile order of gemm_ctrl_rows_order) -
// instances of their own, so that every other launch runs the code it always has.  A tile of the last tile column adds
// one to ctl[0] behind its epilogue, with the release the parked sums use.  An augmented tile reads ctl[0] ONCE, with the
// matching acquire, before its first operand load: all tiles of the last tile column done - the columns of Au are
// complete and visible, the tile takes them into its A panel and writes their rows of Cu; otherwise it computes its
// plain rows alone and raises ctl[2], and the guarded product behind the launch forms Cu.  Nobody waits.  The pieces of
// a cut augmented tile each decide for themselves and say so in the high half of what they add to the tile's arrival
// counter: the last arriver writes Cu only if every piece was ready.
template <bool DMA, int WGM = 2, int WGN = 2, int NBUF = 2, int BM = 128, int BN = 128, bool PACKED = false, bool AUG = false>
__global__ void __launch_bounds__(64 * WGM * WGN, NBUF == 3 ? WGM * WGN / 4 : WGM * WGN / 2) k_dgemm_tn_sk(GemmArgs g, SplitPlan sk) {
  using T = GemmTile<BM, BN, WGM, WGN>;
  extern __shared__ __attribute__((aligned(16))) double lds[];  // tiles + one word for the arrival order
  double *As = lds, *Bs = lds + NBUF * T::BK * T::LDA;
  unsigned *s_old = (unsigned *)(lds + NBUF * T::BK * (T::LDA + T::LDB));
  constexpr int SLOT = BM * BN;
  unsigned long long *stamp = g.stamps ? g.stamps + 32 * (long long)blockIdx.x : nullptr;  // (diagnostic launches only)
  if (stamp && threadIdx.x == 0) stamp[0] = __builtin_amdgcn_s_memrealtime();
  // (A queue of units was measured in round 3 and does not pay: profiles/NOTES.md.)
  auto unit = [&](const SkUnit u, int r) {
    const int t = u.tile, s0 = u.s0, s1 = u.s1, pieces = u.pieces, j = u.j;
    int tm, tn;
    bool aug = false, ready = false;
    if constexpr (AUG) {
      const int e = g.tile_map[t];
      aug = e < 0, tm = (e >> 16) & 0x7fff, tn = e & 0xffff;
      if (aug) {  // (uniform)
        if (threadIdx.x == 0) {
          const unsigned done = __hip_atomic_load(g.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          *s_old = done;
        }
        __syncthreads();
        ready = *s_old == (unsigned)((g.M + BM - 1) / BM);
        __syncthreads();
      }
    } else
      T::tile_of(g, t, tm, tn);
    double4_t acc[T::TM][T::TN];
#pragma unroll
    for (int x = 0; x < T::TM; x++)
#pragma unroll
      for (int y = 0; y < T::TN; y++) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
    if constexpr (DMA) {
      if (AUG && aug)
        T::accumulate_dma_aug(g, tm * BM, tn * BN, s0, s1, ready, acc, As, Bs, NBUF);
      else
        T::template accumulate_dma<PACKED>(g, tm * BM, tn * BN, s0, s1, acc, As, Bs, g.lower && tm == tn, NBUF);
    } else
      T::template accumulate<PACKED>(g, tm * BM, tn * BN, s0, s1, acc, As, Bs);
    bool finish = true;
    if (stamp && threadIdx.x == 0 && r < 10) stamp[1 + 3 * r] = __builtin_amdgcn_s_memrealtime();
    if (pieces > 1) {
      double *mine = sk.ws + (long long)(u.slot0 + j) * SLOT;
#pragma unroll
      for (int x = 0; x < T::TM; x++)
#pragma unroll
        for (int y = 0; y < T::TN; y++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++) mine[((x * T::TN + y) * 4 + rg) * T::NT + threadIdx.x] = acc[x][y][rg];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *s_old = __hip_atomic_fetch_add(sk.cnt + t, (AUG && aug && !ready) ? 0x10001u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      finish = (AUG ? (*s_old & 0xffffu) : *s_old) == (unsigned)(pieces - 1);
      if (AUG && (*s_old >> 16)) ready = false;
      if (finish) {
        if (threadIdx.x == 0) {
          sk.cnt[t] = 0;  // (every piece of the tile has arrived: the counter is ready for the next launch)
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
#pragma unroll
        for (int x = 0; x < T::TM; x++)
#pragma unroll
          for (int y = 0; y < T::TN; y++) acc[x][y] = (double4_t){0.0, 0.0, 0.0, 0.0};
        for (int jj = 0; jj < pieces; jj++) {  // in the order of the k ranges, whoever arrived last
          const double *theirs = sk.ws + (long long)(u.slot0 + jj) * SLOT;
#pragma unroll
          for (int x = 0; x < T::TM; x++)
#pragma unroll
            for (int y = 0; y < T::TN; y++)
#pragma unroll
              for (int rg = 0; rg < 4; rg++) acc[x][y][rg] += theirs[((x * T::TN + y) * 4 + rg) * T::NT + threadIdx.x];
        }
      }
      __syncthreads();  // s_old is rewritten at the next shared tile
    }
    if (stamp && threadIdx.x == 0 && r < 10) stamp[2 + 3 * r] = __builtin_amdgcn_s_memrealtime();
    if (AUG && aug) {
      // (the corner tile's plain rows were written by its plain form, early in the launch)
      if (finish) T::epilogue_aug(g, tm, tn, acc, tn != (g.N + BN - 1) / BN - 1, ready);
      if (finish && !ready && threadIdx.x == 0) g.ctl[2] = 1u;
    } else if (finish)
      T::epilogue(g, tm, tn, acc, lds);  // (uniform: the whole workgroup)
    if (AUG && finish && !aug && tn == (g.N + BN - 1) / BN - 1) {  // a tile of the last tile column is in memory
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(g.ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (stamp && threadIdx.x == 0 && r < 10) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp[3 + 3 * r] = __builtin_amdgcn_s_memrealtime();
    }
    __syncthreads();
  };
  const SkUnit *tab = sk.table + (long long)blockIdx.x * sk.stride;
  for (int r = 0; r < sk.stride; r++) {
    const SkUnit u = tab[r];
    if (u.tile < 0) break;
    unit(u, r);
  }
}
// (+ 16 bytes: the word for the arrival order, and the size the launches have always had - LDS per workgroup decides how many a CU holds)
static inline size_t gemm_sk_lds_bytes(int nbuf = 2) { return gemm_lds_bytes(128, 128, nbuf) + 16; }

// Host: the variants of the 128 x 128 product (gemm_schedule.hpp)
static inline int gemm_wgs_per_cu(int variant) { return variant == GEMM_DMA8X3 ? 1 : 2; }
// cus > 0: a launch of at most that many tiles takes the three-buffer kernel, whose 110 KB of LDS admit ONE workgroup
// per CU - the dispatcher otherwise puts two workgroups on some CUs and none on others, and a pair takes twice as long
// as a workgroup alone (the column strip 5000 x 640 x 5000 of a system sharded over 8 ranks: 0.75 -> 0.62 ms)
static inline void gemm_launch_plain(int variant, unsigned tiles, hipStream_t s, const GemmArgs &g, int cus = 0) {
  if (variant == GEMM_DMA8 && cus > 0 && (int)tiles <= cus) variant = GEMM_DMA8X3;
  if (variant == GEMM_DMA8X3)
    k_dgemm_tn<128, 128, true, 2, 4, 3><<<tiles, 512, gemm_lds_bytes(128, 128, 3), s>>>(g);
  else if (variant == GEMM_DMA8)
    k_dgemm_tn<128, 128, true, 2, 4><<<tiles, 512, gemm_lds_bytes(128, 128), s>>>(g);
  else if (variant == GEMM_DMA4)
    k_dgemm_tn<128, 128, true><<<tiles, 256, gemm_lds_bytes(128, 128), s>>>(g);
  else
    k_dgemm_tn<128, 128><<<tiles, 256, gemm_lds_bytes(128, 128), s>>>(g);
}
static inline void gemm_launch_split(int variant, int grid, hipStream_t s, const GemmArgs &g, const SplitPlan &sk) {
  if (g.apack || g.bpack) {  // (packed panels: the same kernels with the packed addressing)
    if (variant == GEMM_DMA8X3)
      k_dgemm_tn_sk<true, 2, 4, 3, 128, 128, true><<<grid, 512, gemm_sk_lds_bytes(3), s>>>(g, sk);
    else if (variant == GEMM_DMA8)
      k_dgemm_tn_sk<true, 2, 4, 2, 128, 128, true><<<grid, 512, gemm_sk_lds_bytes(), s>>>(g, sk);
    else if (variant == GEMM_DMA4)
      k_dgemm_tn_sk<true, 2, 2, 2, 128, 128, true><<<grid, 256, gemm_sk_lds_bytes(), s>>>(g, sk);
    else
      k_dgemm_tn_sk<false, 2, 2, 2, 128, 128, true><<<grid, 256, gemm_sk_lds_bytes(), s>>>(g, sk);
    return;
  }
  if (g.Au) {  // (the control-row segment: the 2 x 4 LDS-DMA kernels alone, gemm_ctrl_rows_ok)
    if (variant == GEMM_DMA8X3)
      k_dgemm_tn_sk<true, 2, 4, 3, 128, 128, false, true><<<grid, 512, gemm_sk_lds_bytes(3), s>>>(g, sk);
    else
      k_dgemm_tn_sk<true, 2, 4, 2, 128, 128, false, true><<<grid, 512, gemm_sk_lds_bytes(), s>>>(g, sk);
    return;
  }
  if (variant == GEMM_DMA8X3)
    k_dgemm_tn_sk<true, 2, 4, 3><<<grid, 512, gemm_sk_lds_bytes(3), s>>>(g, sk);
  else if (variant == GEMM_DMA8)
    k_dgemm_tn_sk<true, 2, 4><<<grid, 512, gemm_sk_lds_bytes(), s>>>(g, sk);
  else if (variant == GEMM_DMA4)
    k_dgemm_tn_sk<true><<<grid, 256, gemm_sk_lds_bytes(), s>>>(g, sk);
  else
    k_dgemm_tn_sk<false><<<grid, 256, gemm_sk_lds_bytes(), s>>>(g, sk);
}
// 64 x 64 tiles (register-staged loop) with their k ranges cut: products of a few hundred small tiles, where one
// workgroup per CU leaves the matrix pipe two thirds idle (a stage of ~1000 states: 272 tiles of 63 slabs, 91 us)
static inline hipError_t gemm_set_attributes() {
  hipError_t e = hipSuccess;
  auto set = [&](const void *f, size_t bytes) {
    const hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) e = r;
  };
  set((const void *)k_dgemm_tn<128, 128>, gemm_lds_bytes(128, 128));
  set((const void *)k_dgemm_tn<128, 128, true>, gemm_lds_bytes(128, 128));
  set((const void *)k_dgemm_tn<128, 128, true, 2, 4>, gemm_lds_bytes(128, 128));
  set((const void *)k_dgemm_tn<64, 64>, gemm_lds_bytes(64, 64));
  set((const void *)k_dgemm_tn<64, 32>, gemm_lds_bytes(64, 32));
  set((const void *)k_dgemm_tn_ks<64, 64>, gemm_lds_bytes(64, 64));
  set((const void *)k_dgemm_tn_sk<false>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true, 2, 4>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn<128, 128, true, 2, 4, 3>, gemm_lds_bytes(128, 128, 3));
  set((const void *)k_dgemm_tn_sk<true, 2, 4, 3>, gemm_sk_lds_bytes(3));
  set((const void *)k_dgemm_tn_sk<false, 2, 2, 2, 128, 128, true>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true, 2, 2, 2, 128, 128, true>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true, 2, 4, 2, 128, 128, true>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true, 2, 4, 3, 128, 128, true>, gemm_sk_lds_bytes(3));
  set((const void *)k_dgemm_tn_sk<true, 2, 4, 2, 128, 128, false, true>, gemm_sk_lds_bytes());
  set((const void *)k_dgemm_tn_sk<true, 2, 4, 3, 128, 128, false, true>, gemm_sk_lds_bytes(3));
  return e;
}
// (HQPKKT_SK_TABLE=0: the cut form with equal shares, gemm_equal_table, for same-box comparisons)
static inline bool gemm_sk_table_from_env() {
  const char *r = getenv("HQPKKT_SK_TABLE");
  return !r || atoi(r) != 0;
}
static inline int gemm_variant_from_env() {
  if (getenv("HQPKKT_NO_LDSDMA")) return GEMM_REG4;
  const char *w = getenv("HQPKKT_DGEMM_WAVES");
  if (w && atoi(w) == 4) return GEMM_DMA4;
  return GEMM_DMA8;
}

// What st_gemm (staged_host.hip.h) and the test hooks hqpkkt_debug_dgemm* (staged_engine.hip) share besides the schedule
// of a launch (gemm_schedule.hpp): the request of a GemmArgs, and the launch of a schedule.

// Operands by LDS-DMA (global_load_lds_dwordx4) only from 16-byte aligned rows: an operand that starts at an odd column
// (the control columns F + nn of a stage with an odd number of states) or has an odd leading dimension is staged
// through registers (GemmArgs::zeros stays null)
static inline bool gemm_operands_dma_ok(const GemmArgs &g) {
  return ((((uintptr_t)g.A | (uintptr_t)g.B | (uintptr_t)g.A2 | (uintptr_t)g.B2) & 15) == 0) && (((g.lda | g.ldb | g.lda2 | g.ldb2) & 1) == 0);
}
// The control-row segment of g (GemmArgs::Au) can be taken by a launch of the cut forms: a ragged last tile row with an
// even number r of rows and room for the mu rows, no other special of a launch, and Au = the columns [c0, c0 + mu) of C
// inside the last tile column (so the tiles whose completion the augmented tiles ask for are the ones that write it);
// every 16-byte load of a row of Au lies inside a row of C.  (The kernels it needs - 2 x 4 waves, LDS-DMA - and the list
// are the schedule's to ask for.)
static inline bool gemm_ctrl_rows_ok(const GemmArgs &g) {
  if (!g.Au || !g.Cu || !g.ctl || g.mu <= 0 || g.M <= 0) return false;
  const int r = gemm_last_rows(g.M);
  const long long c0 = g.Au - g.C;
  return !(r & 1) && r + g.mu <= 128 && (((uintptr_t)g.Au) & 15) == 0 && !(g.ldau & 1) && g.ldau == g.ldc && c0 >= (g.N - 1) / 128 * 128LL &&
         c0 + g.mu <= g.N && c0 + g.mu + (g.mu & 1) <= g.ldc && !g.lower && !g.mirror && g.K2 == 0 && g.beta == 0.0 && !g.bstrips && !g.rects && !g.apack &&
         !g.bpack && !g.tile_map && !g.stamps;
}
// the end of a stage's use of the segment: the launch's fall-back counted, its words ready for the next launch
__global__ void k_ctrl_rows_end(unsigned *ctl) {
  if (threadIdx.x == 0) {
    if (ctl[2]) ctl[1]++;
    ctl[0] = 0, ctl[2] = 0;
  }
}
// The request of a launch of g (gemm_schedule.hpp): no pointer or leading dimension of g counts beyond what they admit.
// second: on the second stream; ntiles: the tiles g.tile_map[0 .. ntiles) only; by, panel: the profile form
static inline GemmRequest gemm_request(const GemmArgs &g, bool second = false, int ntiles = 0, int by = 0, const int *panel = nullptr) {
  GemmRequest r;
  r.M = g.M, r.N = g.N, r.K = g.K, r.K2 = g.K2, r.lower = g.lower, r.mirror = g.mirror, r.ntiles = ntiles;
  r.second = second, r.dma = gemm_operands_dma_ok(g);
  if (g.Au && g.mu > 0) r.mu = g.mu, r.seg_ok = gemm_ctrl_rows_ok(g);
  if (by) r.by = by, r.panel.assign(panel, panel + 2 * (((by == 2 ? g.M : g.N) + 127) / 128));
  return r;
}
// Workspace of the thin product cut in k (GEMM_FORM_KS): its pieces' raw sums, M x N each
static inline long long gemm_ks_ws_elems(const GemmArgs &g, const GemmForm &f) { return (long long)f.nsplit * g.M * g.N; }
// What the launch of a form needs besides the product: the 128 x 128 variant, the CUs (plain rounds of at most that many
// tiles take the three-buffer kernel; 0: never), the grid of the cut forms with their list (sk null: a cut form whose
// list's pieces the workspace does not hold runs as a plain round of whole tiles) and the pieces of a product cut in k
struct GemmLaunch {
  int variant, cus, grid;
  const SplitPlan *sk;
  double *ks_ws;
};
// Launches form f of g on stream s.  `around(launch)` runs every kernel launch (st_gemm: inside the handle's profile
// brackets; the test hooks: as it is)
template <class Around>
static inline void gemm_launch_form(const GemmForm &f, const GemmLaunch &L, hipStream_t s, const GemmArgs &g, Around &&around) {
  switch (f.kind) {
    case GEMM_FORM_FRAC:
    case GEMM_FORM_CUT:
      if (L.sk) {
        around([&]() { gemm_launch_split(L.variant, L.grid, s, g, *L.sk); });
        break;
      }
      [[fallthrough]];
    case GEMM_FORM_PLAIN:
      around([&]() { gemm_launch_plain(L.variant, (unsigned)f.tiles, s, g, L.cus); });
      break;
    case GEMM_FORM_PROFILE:  // (only by its list: a round of whole tiles would read what the ranges leave out)
      if (L.sk) around([&]() { gemm_launch_split(L.variant, L.grid, s, g, *L.sk); });
      break;
    case GEMM_FORM_KS:
      around([&]() { k_dgemm_tn_ks<64, 64><<<dim3((unsigned)f.tiles, f.nsplit), 256, gemm_lds_bytes(64, 64), s>>>(g, L.ks_ws, f.nsplit); });
      around([&]() { k_dgemm_ks_finish<<<(unsigned)(((long long)g.M * g.N + 255) / 256), 256, 0, s>>>(g, L.ks_ws, f.nsplit); });
      break;
    case GEMM_FORM_6432:
      around([&]() { k_dgemm_tn<64, 32><<<(unsigned)f.tiles, 256, gemm_lds_bytes(64, 32), s>>>(g); });
      break;
    case GEMM_FORM_6464:
      around([&]() { k_dgemm_tn<64, 64><<<(unsigned)f.tiles, 256, gemm_lds_bytes(64, 64), s>>>(g); });
      break;
    default: break;  // (GEMM_FORM_NONE: nothing to launch)
  }
}
// What a launch by a schedule takes from its holder: the schedule's list and tile order on the device (null: none), the
// parked partial tiles and the arrival counters of the cut forms, the pieces of a product cut in k, the zero row of the
// LDS-DMA staging
struct GemmBufs {
  const SkUnit *units;
  const int *order;
  double *sk_ws;
  unsigned *sk_cnt;
  double *ks_ws;
  const double *zeros;
};
// g as schedule sc of its request launches it: zeros, tile_map; a segment that is not taken is dropped
static inline GemmArgs gemm_complete(const GemmSchedule &sc, const GemmBufs &b, GemmArgs g) {
  if (sc.variant != GEMM_REG4) g.zeros = b.zeros;
  if (b.order) g.tile_map = b.order;
  if (!sc.seg) g.Au = nullptr, g.Cu = nullptr, g.mu = 0, g.ctl = nullptr;
  return g;
}
// Launches g by schedule sc of its request.  `around` as in gemm_launch_form
template <class Around>
static inline void gemm_run(const GemmSchedule &sc, const GemmCaps &c, const GemmBufs &b, hipStream_t s, const GemmArgs &g0, Around &&around) {
  const GemmArgs g = gemm_complete(sc, b, g0);
  // (the arrival counters of the cut forms are zero between launches: the last arriver of a tile resets its)
  const SplitPlan sk{b.sk_ws, b.sk_cnt, b.units, sc.tab.stride};
  const GemmLaunch L{sc.variant, c.cus, c.grid, sc.list != SK_LIST_NONE ? &sk : nullptr, b.ks_ws};
  gemm_launch_form(sc.f, L, s, g, around);
}
}  // namespace stg
