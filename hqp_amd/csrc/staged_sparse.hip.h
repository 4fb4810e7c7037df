// The sparse form of the STAGED engine's stage products (HQPKKT_DYN_SPARSE; Hqp_IpLQDOCP's mat_a_sparse, FormGxxSp /
// FormGxSp, hqp/Hqp_IpLQDOCP.C:1119-1273): F_k = [fx_k fu_k] is never a dense block.  The kernels walk the CSR arrays of
// A and A' the handle holds anyway (values refreshed by hqpkkt_set_values) over the ranges StagedPlan::sp_arow /
// sp_tcol: per column c of F_k the entries (row j, value F_jc) of that column, per row j its entries without the -1.
//   pass 1   T = F'V+     T[c][i] = sum over the entries (j, F_jc) of column c of V+[i][j] F_jc   (V+ is exactly
//                         symmetric: its ROWS are read)
//   pass 2   G = T F      G[c][d] = sum over the entries (j, F_jd) of column d of T[c][j] F_jd, d <= c, and the mirror
//                         image G[d][c] out of the same register
// Both are ONE kernel (k_sp_gather): a lane owns a column d of F_k, a workgroup SP_RB consecutive rows of the dense operand
// X (V+ or T) times 256 columns.  With a banded F neighbouring lanes read neighbouring X[i][j]: the loads of a wavefront
// are contiguous, every entry of a column re-reads the row segment the entry before it read (L1), the next workgroup of
// the row block the segment's end (L2), so X streams from memory once.  Every sum runs over a column's entries in their
// stored order inside one thread: no atomics, a second factorisation gives the same bits.  The transposed results leave
// a lane as SP_RB consecutive doubles (16-byte stores).
// Included by staged_engine.hip behind staged.hip.h.
#pragma once

namespace stg {

constexpr int SP_RB = 8;  // rows of the dense operand per workgroup (one 64-byte run per lane of a transposed result)

// the entries of the columns [0, ncols) of one stage's F: column c holds ent[2 c] .. ent[2 c + 1] of (row, val), its row
// inside the stage is row[t] - row0
struct SpCols {
  const int *ent;  // (already offset to the stage's first column)
  const int *row;
  const double *val;
  int row0, ncols;
};

// out[i][d] (straight, may be null) and outT[d][i] (transposed, may be null) = sum_t X[i][j_t] a_t over the entries of
// column d, for the rows i < M of X.  lower: only d <= i - both images of an entry below the diagonal, the diagonal once
struct SpGather {
  SpCols f;
  const double *X;
  long long ldx;
  int M;
  double *out;
  long long ldo;
  double *outT;
  long long ldt;
  int lower;
};
__global__ void __launch_bounds__(256) k_sp_gather(SpGather g) {
  const int d = blockIdx.x * 256 + threadIdx.x, i0 = blockIdx.y * SP_RB;
  if (g.lower && blockIdx.x * 256 > i0 + SP_RB - 1) return;  // (the whole workgroup lies above the diagonal)
  if (d >= g.f.ncols) return;
  const int rows = min(SP_RB, g.M - i0);
  const int t0 = g.f.ent[2 * d], t1 = g.f.ent[2 * d + 1];
  double acc[SP_RB];
#pragma unroll
  for (int u = 0; u < SP_RB; u++) acc[u] = 0.0;
  const double *x0 = g.X + (long long)i0 * g.ldx;
  if (rows == SP_RB) {
    for (int t = t0; t < t1; t++) {
      const double a = g.f.val[t];
      const double *x = x0 + (g.f.row[t] - g.f.row0);
      double v[SP_RB];
#pragma unroll
      for (int u = 0; u < SP_RB; u++) v[u] = x[u * g.ldx];
#pragma unroll
      for (int u = 0; u < SP_RB; u++) acc[u] += v[u] * a;
    }
  } else {
    for (int t = t0; t < t1; t++) {
      const double a = g.f.val[t];
      const double *x = x0 + (g.f.row[t] - g.f.row0);
#pragma unroll
      for (int u = 0; u < SP_RB; u++)
        if (u < rows) acc[u] += x[u * g.ldx] * a;
    }
  }
  if (g.out) {
#pragma unroll
    for (int u = 0; u < SP_RB; u++)
      if (u < rows && (!g.lower || d <= i0 + u)) g.out[(long long)(i0 + u) * g.ldo + d] = acc[u];
  }
  if (g.outT) {
    double *o = g.outT + (long long)d * g.ldt + i0;
    // (16-byte stores where the run is whole and aligned: ldt even, i0 a multiple of SP_RB, the block 16-byte aligned)
    if (rows == SP_RB && (!g.lower || d < i0) && ((((size_t)o) & 15) == 0)) {
#pragma unroll
      for (int u = 0; u < SP_RB; u += 2) *(double2_t *)(o + u) = double2_t{acc[u], acc[u + 1]};
    } else {
#pragma unroll
      for (int u = 0; u < SP_RB; u++)
        if (u < rows && (!g.lower || d < i0 + u)) o[u] = acc[u];
    }
  }
}

// carried rows N[r][c] = sum over the entries (j, F_jc) of column c of BT[j][r] F_jc, r < R (BT = B+': n+ rows of ldb >=
// up8(R) doubles): a lane owns a column c and eight rows r, which are one 64-byte run of BT's row j
struct SpCarried {
  SpCols f;
  const double *BT;
  long long ldb;
  int R;
  double *N;
  long long ldn;
};
__global__ void __launch_bounds__(256) k_sp_carried(SpCarried g) {
  const int c = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * 8;
  if (c >= g.f.ncols) return;
  const int t0 = g.f.ent[2 * c], t1 = g.f.ent[2 * c + 1];
  double acc[8];
#pragma unroll
  for (int u = 0; u < 8; u++) acc[u] = 0.0;
  for (int t = t0; t < t1; t++) {
    const double a = g.f.val[t];
    const double2_t *b = (const double2_t *)(g.BT + (long long)(g.f.row[t] - g.f.row0) * g.ldb + r0);  // (ldb a multiple of 8)
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double2_t v = b[u];
      acc[2 * u] += v.x * a, acc[2 * u + 1] += v.y * a;
    }
  }
#pragma unroll
  for (int u = 0; u < 8; u++)
    if (r0 + u < g.R) g.N[(long long)(r0 + u) * g.ldn + c] = acc[u];
}

// the solve's two products with F_k, with the argument lists of k_st_gemv_cols / k_st_gemv_rows:
// y[c] = add[c] + alpha sum over the entries (j, F_jc) of column c of F_jc x[j]; y2 = y + add2 (optional)
struct SpGemvCols {
  SpCols f;
  const double *x;
  const double *add;
  double alpha;
  double *y;
  const double *add2;
  double *y2;
};
__global__ void __launch_bounds__(256) k_sp_gemv_cols(SpGemvCols g) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= g.f.ncols) return;
  double s = 0.0;
  for (int t = g.f.ent[2 * c]; t < g.f.ent[2 * c + 1]; t++) s += g.f.val[t] * g.x[g.f.row[t] - g.f.row0];
  const double r = (g.add ? g.add[c] : 0.0) + g.alpha * s;
  g.y[c] = r;
  if (g.y2) g.y2[c] = r + g.add2[c];
}
// y[i] = scale (add[i] + sum over the entries (c, F_ic) of row i of A, without its -1, of F_ic x[c - col0]), i < M
struct SpGemvRows {
  const int *ent;  // (offset to the stage's first dynamics row: row i holds ent[2 i] .. ent[2 i + 1])
  const int *col;
  const double *val;
  int col0, M;
  const double *x;
  const double *add;
  double *y;
  double scale;
};
__global__ void __launch_bounds__(256) k_sp_gemv_rows(SpGemvRows g) {
  // a quarter wavefront per row: rows of a handful of entries (a band) and dense rows both stay in step
  const int sub = threadIdx.x & 15, i = blockIdx.x * 16 + (threadIdx.x >> 4);
  double s = 0.0;
  if (i < g.M)
    for (int t = g.ent[2 * i] + sub; t < g.ent[2 * i + 1]; t += 16) s += g.val[t] * g.x[g.col[t] - g.col0];
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);  // (a fixed tree: the same bits every run)
  if (i < g.M && sub == 0) g.y[i] = g.scale * ((g.add ? g.add[i] : 0.0) + s);
}

// ---- heavy columns (hqpkkt_set_dense_columns; StagedPlan::hv_cols): the nd columns of F_k with many entries are the
// dense block D (n+ rows of ldd doubles) and go through the MFMA product as thin products - W_h = V+ D, G_hh = D'W_h,
// N_h = B+ D - while the column walks above run over ranges in which those columns are empty.  What is left is moving
// the compact results to where the stage sequence reads them.

// Th[h][j] = Wh[j][h], h < nd, j < np: the rows of T = F'V+ that belong to the heavy columns, for the gather that forms
// their rows of G against the light columns (V+ is exactly symmetric, so D'V+ is the transpose of V+ D)
__global__ void __launch_bounds__(256) k_sp_heavy_transpose(int np, int nd, const double *__restrict__ Wh, long long ldd, double *__restrict__ Th,
                                                            long long ldt) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= np) return;
  const double *w = Wh + (long long)j * ldd;
  for (int h = 0; h < nd; h++) Th[(long long)h * ldt + j] = w[h];
}
// Row and column hv[a] of G, both images from one register, so G stays exactly symmetric: against a light column c the
// gathered Gh[a][c], against the heavy column hv[b] the lower half of Ghh = D'V+D (max(a, b), min(a, b)).  hv_of[c]:
// position of column c among the heavy ones or -1.  The carried rows ride along: N[r][hv[a]] = Nh[r][a], r < R
struct SpHeavyPlace {
  int nz, nd, R;
  const int *hv, *hv_of;
  const double *Gh;
  long long ldgh;
  const double *Ghh;
  long long ldd;
  double *G;
  long long ldg;
  const double *Nh;
  double *N;
  long long ldn;
};
__global__ void __launch_bounds__(256) k_sp_heavy_place(SpHeavyPlace g) {
  const int c = blockIdx.x * 256 + threadIdx.x, a = blockIdx.y;
  const int h = g.hv[a];
  if (c < g.nz) {
    const int b = g.hv_of[c];
    const double v = b < 0 ? g.Gh[(long long)a * g.ldgh + c] : g.Ghh[(long long)max(a, b) * g.ldd + min(a, b)];
    g.G[(long long)h * g.ldg + c] = v;
    g.G[(long long)c * g.ldg + h] = v;
  }
  if (c < g.R) g.N[(long long)c * g.ldn + h] = g.Nh[(long long)c * g.ldd + a];
}
// the solve's gam = q + F'tt for the heavy columns, behind k_sp_gemv_cols on the light ranges (which left y[c] = add[c]
// there): one wavefront per heavy column, the lanes stride over the column's entries in the CSR arrays of A' (coalesced),
// the lanes' sums by a fixed tree.  add, alpha, y2 as in k_sp_gemv_cols
struct SpGemvHeavy {
  SpCols f;       // (the FULL ranges of the stage's columns)
  const int *hv;  // the heavy columns
  int nd;
  const double *x;
  const double *add;
  double alpha;
  double *y;
  const double *add2;
  double *y2;
};
__global__ void __launch_bounds__(256) k_sp_gemv_heavy(SpGemvHeavy g) {
  const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= g.nd) return;  // (whole wavefronts leave)
  const int c = g.hv[a];
  double s = 0.0;
  for (int t = g.f.ent[2 * c] + lane; t < g.f.ent[2 * c + 1]; t += 64) s += g.f.val[t] * g.x[g.f.row[t] - g.f.row0];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) {
    const double r = (g.add ? g.add[c] : 0.0) + g.alpha * s;
    g.y[c] = r;
    if (g.y2) g.y2[c] = r + g.add2[c];
  }
}

}  // namespace stg
