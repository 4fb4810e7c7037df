// The solve's two products with F_k in the profile form of the STAGED engine (HQPKKT_DYN_PROFILE, staged_plan.hpp): F_k
// is the dense block of the dense form, K rows of N = n_k + m_k columns with an even leading dimension, and per 128-column
// panel p the analysis knows the k-slabs [lo_p, hi_p) of 16 rows outside which the panel holds no stored entry.  Both
// kernels stream only that part of the block with 16-byte loads (a panel starts at a multiple of 128 columns and the
// leading dimension is a multiple of 8: every load is aligned and inside its row), sum in a fixed order and use no
// atomics: a second run gives the same bits.  With packed panels (hqpkkt_set_packed_panels, StagedPlan::pk_off) the same
// kernels, same chunks and same order of every sum, take a panel's rows from its own block (PfGemv::pk, the template flag
// PACKED), and the carried rows N = B+ F are formed over the ranges alone (k_pk_carried).
// Included by staged_engine.hip behind staged.hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace stg {

constexpr int PF_RPC = 64;  // rows of a chunk of the columns form (eight rounds of eight rows in flight per lane)

struct PfGemv {
  const double *A;  // K x N, row-major, 16-byte aligned
  long long lda;    // a multiple of 8
  int K, N;
  const int *ranges;  // per panel (lo, hi)
  const double *x;    // columns form: K entries; rows form: N entries
  const double *add;  // may be null
  double alpha;
  double *y;          // columns form: N entries; rows form: K entries
  double *part;       // columns form: chunks x N partial sums (gridDim.y > 1)
  const PackPanel *pk;  // PACKED: per panel its block (A + off: the panel's row 0 as in a dense block, leading dimension ld)
};
// rows [r0, r1) of panel p
static __device__ __forceinline__ void pf_rows(const PfGemv &g, int p, int &r0, int &r1) {
  r0 = 16 * g.ranges[2 * p], r1 = min(g.K, 16 * g.ranges[2 * p + 1]);
}
// columns form, gam = add + alpha A'x: a wavefront per panel and chunk of PF_RPC rows of the panel's range, a lane two
// neighbouring columns.  One chunk per panel at most (gridDim.y == 1): the result is written; otherwise the chunk's sums
// go to part[chunk][column] and k_pf_cols_finish adds a panel's chunks in their order.
template <bool PACKED>
__global__ void __launch_bounds__(256) k_pf_gemv_cols(PfGemv g) {
  const int lane = threadIdx.x & 63, p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int j = 128 * p + 2 * lane;
  if (128 * p >= g.N) return;  // (wave-uniform)
  int r0, r1;
  pf_rows(g, p, r0, r1);
  const int k0 = r0 + (int)blockIdx.y * PF_RPC, k1 = min(r1, k0 + PF_RPC);
  if (gridDim.y > 1 && k0 >= r1) return;  // (no such chunk in this panel: the finish does not read it)
  double s0 = 0.0, s1 = 0.0;
  if (j < g.N && k0 < k1) {  // (j even, j < N <= lda, lda even: the 16-byte load stays inside the row)
    const long long lda = PACKED ? g.pk[p].ld : g.lda;
    const double *a = PACKED ? g.A + g.pk[p].off + (long long)k0 * lda + 2 * lane : g.A + (long long)k0 * lda + j;
    double t0 = 0.0, t1 = 0.0, u0 = 0.0, u1 = 0.0, w0 = 0.0, w1 = 0.0;
    int k = k0;
    for (; k + 7 < k1; k += 8, a += 8 * lda) {
      const double2_t v0 = *(const double2_t *)a, v1 = *(const double2_t *)(a + lda), v2 = *(const double2_t *)(a + 2 * lda),
                      v3 = *(const double2_t *)(a + 3 * lda), v4 = *(const double2_t *)(a + 4 * lda), v5 = *(const double2_t *)(a + 5 * lda),
                      v6 = *(const double2_t *)(a + 6 * lda), v7 = *(const double2_t *)(a + 7 * lda);
      const double x0 = g.x[k], x1 = g.x[k + 1], x2 = g.x[k + 2], x3 = g.x[k + 3], x4 = g.x[k + 4], x5 = g.x[k + 5], x6 = g.x[k + 6],
                   x7 = g.x[k + 7];
      s0 += v0.x * x0, s1 += v0.y * x0, t0 += v1.x * x1, t1 += v1.y * x1;
      u0 += v2.x * x2, u1 += v2.y * x2, w0 += v3.x * x3, w1 += v3.y * x3;
      s0 += v4.x * x4, s1 += v4.y * x4, t0 += v5.x * x5, t1 += v5.y * x5;
      u0 += v6.x * x6, u1 += v6.y * x6, w0 += v7.x * x7, w1 += v7.y * x7;
    }
    for (; k < k1; k++, a += lda) {
      const double2_t v0 = *(const double2_t *)a;
      s0 += v0.x * g.x[k], s1 += v0.y * g.x[k];
    }
    s0 = (s0 + t0) + (u0 + w0), s1 = (s1 + t1) + (u1 + w1);
  }
  if (j >= g.N) return;
  if (gridDim.y == 1) {
    g.y[j] = (g.add ? g.add[j] : 0.0) + g.alpha * s0;
    if (j + 1 < g.N) g.y[j + 1] = (g.add ? g.add[j + 1] : 0.0) + g.alpha * s1;
  } else {
    g.part[(long long)blockIdx.y * g.N + j] = s0;
    if (j + 1 < g.N) g.part[(long long)blockIdx.y * g.N + j + 1] = s1;
  }
}
__global__ void __launch_bounds__(256) k_pf_cols_finish(PfGemv g) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= g.N) return;
  int r0, r1;
  pf_rows(g, j >> 7, r0, r1);
  const int nchunk = r1 > r0 ? (r1 - r0 + PF_RPC - 1) / PF_RPC : 0;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += g.part[(long long)c * g.N + j];
  g.y[j] = (g.add ? g.add[j] : 0.0) + g.alpha * s;
}
// rows form, x+ = add + alpha A x: a wavefront per row; it visits the panels whose range holds the row's slab (a
// wave-uniform test), in ascending order, a lane two neighbouring columns of each
template <bool PACKED>
__global__ void __launch_bounds__(256) k_pf_gemv_rows(PfGemv g) {
  const int lane = threadIdx.x & 63, row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (row >= g.K) return;
  const int slab = row >> 4, np = (g.N + 127) >> 7;
  const double *ar = g.A + (long long)row * g.lda + 2 * lane;
  const double *xr = g.x + 2 * lane;
  double s = 0.0;
  for (int p = 0; p < np; p++) {
    if (slab < g.ranges[2 * p] || slab >= g.ranges[2 * p + 1]) continue;
    const int j = 128 * p + 2 * lane;
    if (j < g.N) {
      const double2_t v = PACKED ? *(const double2_t *)(g.A + g.pk[p].off + (long long)row * g.pk[p].ld + 2 * lane) : *(const double2_t *)(ar + 128 * p);
      s += v.x * xr[128 * p];
      if (j + 1 < g.N) s += v.y * xr[128 * p + 1];
    }
  }
  s = kktdev::wave_sum(s);
  if (lane == 0) g.y[row] = (g.add ? g.add[row] : 0.0) + g.alpha * s;
}

// chunks of the columns form: the longest range of the panels, in chunks of PF_RPC rows (at least one)
static inline int pf_chunks(const int *ranges, int panels, int K) {
  int rows = 0;
  for (int p = 0; p < panels; p++) rows = std::max(rows, std::min(K, 16 * ranges[2 * p + 1]) - 16 * ranges[2 * p]);
  return std::max(1, (rows + PF_RPC - 1) / PF_RPC);
}
// the launches of either product on stream s; `around` as in gemm_launch_form.  g.ranges: the device copy, `ranges`
// the host's; g.part holds pf_chunks x N doubles
template <class Around>
static inline void pf_launch_cols(const PfGemv &g, const int *ranges, hipStream_t s, Around &&around) {
  if (g.N <= 0) return;
  const int np = (g.N + 127) / 128, chunks = pf_chunks(ranges, np, g.K);
  if (g.pk)
    around([&]() { k_pf_gemv_cols<true><<<dim3((np + 3) / 4, chunks), 256, 0, s>>>(g); });
  else
    around([&]() { k_pf_gemv_cols<false><<<dim3((np + 3) / 4, chunks), 256, 0, s>>>(g); });
  if (chunks > 1) around([&]() { k_pf_cols_finish<<<(g.N + 255) / 256, 256, 0, s>>>(g); });
}
template <class Around>
static inline void pf_launch_rows(const PfGemv &g, hipStream_t s, Around &&around) {
  if (g.K <= 0) return;
  if (g.pk)
    around([&]() { k_pf_gemv_rows<true><<<(g.K + 3) / 4, 256, 0, s>>>(g); });
  else
    around([&]() { k_pf_gemv_rows<false><<<(g.K + 3) / 4, 256, 0, s>>>(g); });
}

// The carried rows of a packed stage, N[r][c] = sum over the rows k of panel(c)'s range of BT[k][r] A[k][c] (BT = B+',
// K x R with R <= 256 carried rows; A = F_k in packed panels, N columns): a wavefront per panel, chunk of the panel's
// range and group of PK_RG carried rows; a lane owns two neighbouring columns of the panel (one 16-byte load per row), the
// BT values are the same for all lanes.  The range of the longest panel is cut into at most PK_MAXCH chunks of `rpc` rows
// (pk_chunk_rows); one chunk: the sums are written; otherwise they go to part[chunk][r][c] and k_pk_carried_finish adds a
// panel's chunks in their order.  Plain FMAs in a fixed order, no atomics: a second run gives the same bits.
constexpr int PK_RG = 8, PK_MAXCH = 8;
struct PkCarried {
  const double *BT;
  long long ldb;
  const double *A;
  const PackPanel *pk;
  const int *ranges;
  int K, N, R, rpc;
  double *C;  // R x N
  long long ldc;
  double *part;  // chunks x R x N (gridDim.y > 1)
};
__global__ void __launch_bounds__(256) k_pk_carried(PkCarried g) {
  const int lane = threadIdx.x & 63, p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (128 * p >= g.N) return;  // (wave-uniform)
  const int j = 128 * p + 2 * lane, r0 = blockIdx.z * PK_RG, nr = min(PK_RG, g.R - r0);
  const int lo = 16 * g.ranges[2 * p], hi = min(g.K, 16 * g.ranges[2 * p + 1]);
  const int k0 = lo + (int)blockIdx.y * g.rpc, k1 = min(hi, k0 + g.rpc);
  if (gridDim.y > 1 && k0 >= hi) return;  // (no such chunk in this panel: the finish does not read it)
  double s0[PK_RG], s1[PK_RG];
#pragma unroll
  for (int r = 0; r < PK_RG; r++) s0[r] = s1[r] = 0.0;
  if (j < g.N) {  // (2 lane < the panel's columns <= its leading dimension, a multiple of 8: the load stays inside the row)
    const long long ld = g.pk[p].ld;
    const double *a = g.A + g.pk[p].off + (long long)k0 * ld + 2 * lane;
    const double *b = g.BT + (long long)k0 * g.ldb + r0;
    for (int k = k0; k < k1; k++, a += ld, b += g.ldb) {
      const double2_t v = *(const double2_t *)a;
#pragma unroll
      for (int r = 0; r < PK_RG; r++) {
        const double br = r < nr ? b[r] : 0.0;  // (wave-uniform)
        s0[r] += br * v.x, s1[r] += br * v.y;
      }
    }
  }
  if (j >= g.N) return;
  double *out = gridDim.y == 1 ? g.C : g.part + (long long)blockIdx.y * g.R * g.N;
  const long long ldo = gridDim.y == 1 ? g.ldc : g.N;
#pragma unroll
  for (int r = 0; r < PK_RG; r++)
    if (r < nr) {
      out[(long long)(r0 + r) * ldo + j] = s0[r];
      if (j + 1 < g.N) out[(long long)(r0 + r) * ldo + j + 1] = s1[r];
    }
}
__global__ void __launch_bounds__(256) k_pk_carried_finish(PkCarried g) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (j >= g.N) return;
  const int lo = 16 * g.ranges[2 * (j >> 7)], hi = min(g.K, 16 * g.ranges[2 * (j >> 7) + 1]);
  const int nchunk = hi > lo ? (hi - lo + g.rpc - 1) / g.rpc : 0;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += g.part[((long long)c * g.R + r) * g.N + j];
  g.C[(long long)r * g.ldc + j] = s;
}
// rows of a chunk of the carried rows' k range: a multiple of 64, at most PK_MAXCH chunks over the longest range
static inline int pk_chunk_rows(const int *ranges, int panels, int K) {
  int rows = 0;
  for (int p = 0; p < panels; p++) rows = std::max(rows, std::min(K, 16 * ranges[2 * p + 1]) - 16 * ranges[2 * p]);
  return std::max(64, ((rows + PK_MAXCH - 1) / PK_MAXCH + 63) / 64 * 64);
}
static inline int pk_chunks(const int *ranges, int panels, int K) {
  const int rpc = pk_chunk_rows(ranges, panels, K);
  int rows = 0;
  for (int p = 0; p < panels; p++) rows = std::max(rows, std::min(K, 16 * ranges[2 * p + 1]) - 16 * ranges[2 * p]);
  return std::max(1, (rows + rpc - 1) / rpc);
}
// g.rpc is set here; g.part holds pk_chunks x R x N doubles
template <class Around>
static inline void pk_launch_carried(PkCarried g, const int *ranges, hipStream_t s, Around &&around) {
  if (g.N <= 0 || g.R <= 0) return;
  const int np = (g.N + 127) / 128, chunks = pk_chunks(ranges, np, g.K);
  g.rpc = pk_chunk_rows(ranges, np, g.K);
  around([&]() { k_pk_carried<<<dim3((np + 3) / 4, chunks, (g.R + PK_RG - 1) / PK_RG), 256, 0, s>>>(g); });
  if (chunks > 1) around([&]() { k_pk_carried_finish<<<dim3((g.N + 255) / 256, g.R), 256, 0, s>>>(g); });
}
}  // namespace stg
