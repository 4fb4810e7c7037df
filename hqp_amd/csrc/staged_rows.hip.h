// Wide rows of the inequality block C in the STAGED engine (hqpkkt_set_dense_rows; StagedPlan::wr_rows): the r rows of a
// stage with many stored entries are the dense block E_k (r rows of ld doubles, zero in the padding), and their share of
// H = Q + C'(Z/W)C is the thin-K MFMA product S'S with S = diag(sqrt(z / w)) E_k (st_add_h_wide, staged_host.hip.h).  With
// the square root in both operands entry (i, j) of the product and its image are the same sum of the same products.
// The vector work of the same rows - the step's q = C'tz - r1, dz and dw, the residual's C dx and C'dz - goes through the
// blocks as well (k_st_rows_gemv, k_st_rows_gemv_t): ONE launch over all stages each, from a table of the blocks
// (RowsBlock) that is uploaded with the plan; the CSR walks of these products see narrow copies of C and C' without the
// wide rows (StagedPlan::cn, ctn).  Fixed order of every sum, no atomics: two runs give the same bits.
// Included by staged_engine.hip behind staged.hip.h.
#pragma once

namespace stg {

struct RowsScale {
  const double *E;   // r x ld, 16-byte aligned, ld even
  double *S;         // the same shape
  const int *rows;   // the rows of C (indices into wt)
  const double *wt;  // z / w per row of C (k_weights)
  int r;
  long long ld;
};
// S[i][j] = sqrt(wt[rows[i]]) E[i][j]: a thread per pair of doubles
__global__ void __launch_bounds__(256) k_st_rows_scale(RowsScale a) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x, half = a.ld / 2;
  if (q >= a.r * half) return;
  const double s = sqrt(a.wt[a.rows[q / half]]);
  const double2_t v = reinterpret_cast<const double2_t *>(a.E)[q];
  reinterpret_cast<double2_t *>(a.S)[q] = (double2_t){s * v.x, s * v.y};
}


// A block E_k as the vector products see it: r rows of ld doubles from E + oE (oE and ld even: 16-byte rows), of which the
// first nz columns count - they meet x[col0 .. col0 + nz); its rows are rows[row0 .. row0 + r) of the row-index list
struct RowsBlock {
  long long oE;
  int ld, nz, col0, row0, r;
};
// Rows form: cdx_j = sum_c E[i][c] x[col0 + c] for the wide row j = rows[row0 + i] of every block; then
//   tz != NULL (the step, k_red_dzdw's expressions): dz_j = tz_j - zw_j cdx_j, dw_j = -1.0 r3_j + cdx_j
//   else (the residual): y_j = cdx_j
// - all vectors indexed by the row of C.  blk_of: per entry of the row-index list its block
struct RowsGemv {
  const RowsBlock *blk;
  const int *blk_of;
  int R;  // rows in the list (all blocks)
  const double *E;
  const int *rows;
  const double *x;
  const double *tz, *zw, *r3;
  double *dz, *dw, *y;
};
// A wavefront per row: lane l takes the pairs of columns l, l + 64, .. with one 16-byte load of E each, four in flight
// (a trip of 512 columns); the sums of the four loads in their order, then the lanes' by wave_sum.  x starts at either
// parity of col0: 16-byte loads where x + col0 is aligned, two scalar loads per pair where not.  The loop ends at nz:
// the last pair of an odd nz takes column nz - 1 alone, by a scalar load - x[col0 + nz] is the next stage's, or behind
// the end of x -, and nothing of the padding of E counts.
__global__ void __launch_bounds__(256) k_st_rows_gemv(RowsGemv a) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= a.R) return;
  const RowsBlock b = a.blk[a.blk_of[j]];
  const double2_t *__restrict__ e = reinterpret_cast<const double2_t *>(a.E + b.oE + (long long)(j - b.row0) * b.ld);
  const double *__restrict__ x = a.x + b.col0;
  const int full = b.nz >> 1;  // whole pairs
  const bool x16 = (reinterpret_cast<size_t>(x) & 15) == 0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  auto pair = [&](int p, double2_t v, double &s) {
    double x0, x1;
    if (x16) {
      const double2_t u = reinterpret_cast<const double2_t *>(x)[p];
      x0 = u.x, x1 = u.y;
    } else
      x0 = x[2 * p], x1 = x[2 * p + 1];
    s += v.x * x0;
    s += v.y * x1;
  };
  int p = lane;
  for (; p + 192 < full; p += 256) {
    const double2_t v0 = e[p], v1 = e[p + 64], v2 = e[p + 128], v3 = e[p + 192];
    pair(p, v0, s0), pair(p + 64, v1, s1), pair(p + 128, v2, s2), pair(p + 192, v3, s3);
  }
  for (; p < full; p += 64) pair(p, e[p], s0);
  if ((b.nz & 1) && lane == (full & 63)) s1 += a.E[b.oE + (long long)(j - b.row0) * b.ld + b.nz - 1] * x[b.nz - 1];
  const double cdx = kktdev::wave_sum((s0 + s1) + (s2 + s3));
  if (lane) return;
  const int row = a.rows[j];
  if (a.tz) {
    a.dz[row] = a.tz[row] - a.zw[row] * cdx;
    a.dw[row] = -1.0 * a.r3[row] + cdx;
  } else
    a.y[row] = cdx;
}

// Columns form: xc[col0 + c] = sum_i E[i][c] t[rows[row0 + i]], i ascending, for every column c < nz of every block; zero
// for a block without rows - the launch writes all of x that the blocks cover (the engine's: the whole n-vector).
struct RowsGemvT {
  const RowsBlock *blk;
  const double *E;
  const int *rows;
  const double *t;
  double *xc;
};
// A thread per pair of columns, a grid row per block (blockIdx.y): the lanes of a wavefront read 1 KB of one row of E with
// 16-byte loads, four rows in flight, and add them in the rows' order - one chain per column, whatever the unrolling.
// (Not cut into chunks of rows: a stage holds tens of wide rows, and a thread's loop over them is r 16-byte loads.)
__global__ void __launch_bounds__(256) k_st_rows_gemv_t(RowsGemvT a) {
  const RowsBlock b = a.blk[blockIdx.y];
  const int p = blockIdx.x * 256 + threadIdx.x, c = 2 * p;
  if (c >= b.nz) return;
  const double2_t *__restrict__ e = reinterpret_cast<const double2_t *>(a.E + b.oE) + p;
  const long long half = b.ld >> 1;
  const int *__restrict__ rows = a.rows + b.row0;
  double s0 = 0.0, s1 = 0.0;
  int i = 0;
  for (; i + 3 < b.r; i += 4) {
    const double2_t v0 = e[i * half], v1 = e[(i + 1) * half], v2 = e[(i + 2) * half], v3 = e[(i + 3) * half];
    const double t0 = a.t[rows[i]], t1 = a.t[rows[i + 1]], t2 = a.t[rows[i + 2]], t3 = a.t[rows[i + 3]];
    s0 += v0.x * t0, s1 += v0.y * t0;
    s0 += v1.x * t1, s1 += v1.y * t1;
    s0 += v2.x * t2, s1 += v2.y * t2;
    s0 += v3.x * t3, s1 += v3.y * t3;
  }
  for (; i < b.r; i++) {
    const double2_t v = e[i * half];
    const double ti = a.t[rows[i]];
    s0 += v.x * ti, s1 += v.y * ti;
  }
  double *__restrict__ xc = a.xc + b.col0;
  xc[c] = s0;
  if (c + 1 < b.nz) xc[c + 1] = s1;
}

// The launches of the two forms as the engine makes them and as hqpkkt_debug_rows_gemv does; `around` as in
// gemv_launch_wide.  nblocks: entries of the table; pairs_max: (nz + 1) / 2 of the block with the most columns
template <class Around>
static inline void rows_launch(const RowsGemv &g, hipStream_t s, Around &&around) {
  if (g.R <= 0) return;
  around([&]() { k_st_rows_gemv<<<(unsigned)((g.R + 3) / 4), 256, 0, s>>>(g); });
}
template <class Around>
static inline void rows_launch_t(const RowsGemvT &g, int nblocks, int pairs_max, hipStream_t s, Around &&around) {
  if (nblocks <= 0 || pairs_max <= 0) return;
  around([&]() { k_st_rows_gemv_t<<<dim3((unsigned)((pairs_max + 255) / 256), (unsigned)nblocks), 256, 0, s>>>(g); });
}

}  // namespace stg
