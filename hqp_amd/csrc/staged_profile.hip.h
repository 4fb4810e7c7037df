// The solve's two products with F_k in the profile form of the STAGED engine (HQPKKT_DYN_PROFILE, staged_plan.hpp): F_k
// is the dense block of the dense form, K rows of N = n_k + m_k columns with an even leading dimension, and per 128-column
// panel p the analysis knows the k-slabs [lo_p, hi_p) of 16 rows outside which the panel holds no stored entry.  Both
// kernels stream only that part of the block with 16-byte loads (a panel starts at a multiple of 128 columns and the
// leading dimension is a multiple of 8: every load is aligned and inside its row), sum in a fixed order and use no
// atomics: a second run gives the same bits.  Included by staged_engine.hip behind staged.hip.h.
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
};
// rows [r0, r1) of panel p
static __device__ __forceinline__ void pf_rows(const PfGemv &g, int p, int &r0, int &r1) {
  r0 = 16 * g.ranges[2 * p], r1 = min(g.K, 16 * g.ranges[2 * p + 1]);
}
// columns form, gam = add + alpha A'x: a wavefront per panel and chunk of PF_RPC rows of the panel's range, a lane two
// neighbouring columns.  One chunk per panel at most (gridDim.y == 1): the result is written; otherwise the chunk's sums
// go to part[chunk][column] and k_pf_cols_finish adds a panel's chunks in their order.
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
    const double *a = g.A + (long long)k0 * g.lda + j;
    double t0 = 0.0, t1 = 0.0, u0 = 0.0, u1 = 0.0, w0 = 0.0, w1 = 0.0;
    int k = k0;
    for (; k + 7 < k1; k += 8, a += 8 * g.lda) {
      const double2_t v0 = *(const double2_t *)a, v1 = *(const double2_t *)(a + g.lda), v2 = *(const double2_t *)(a + 2 * g.lda),
                      v3 = *(const double2_t *)(a + 3 * g.lda), v4 = *(const double2_t *)(a + 4 * g.lda), v5 = *(const double2_t *)(a + 5 * g.lda),
                      v6 = *(const double2_t *)(a + 6 * g.lda), v7 = *(const double2_t *)(a + 7 * g.lda);
      const double x0 = g.x[k], x1 = g.x[k + 1], x2 = g.x[k + 2], x3 = g.x[k + 3], x4 = g.x[k + 4], x5 = g.x[k + 5], x6 = g.x[k + 6],
                   x7 = g.x[k + 7];
      s0 += v0.x * x0, s1 += v0.y * x0, t0 += v1.x * x1, t1 += v1.y * x1;
      u0 += v2.x * x2, u1 += v2.y * x2, w0 += v3.x * x3, w1 += v3.y * x3;
      s0 += v4.x * x4, s1 += v4.y * x4, t0 += v5.x * x5, t1 += v5.y * x5;
      u0 += v6.x * x6, u1 += v6.y * x6, w0 += v7.x * x7, w1 += v7.y * x7;
    }
    for (; k < k1; k++, a += g.lda) {
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
      const double2_t v = *(const double2_t *)(ar + 128 * p);
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
  around([&]() { k_pf_gemv_cols<<<dim3((np + 3) / 4, chunks), 256, 0, s>>>(g); });
  if (chunks > 1) around([&]() { k_pf_cols_finish<<<(g.N + 255) / 256, 256, 0, s>>>(g); });
}
template <class Around>
static inline void pf_launch_rows(const PfGemv &g, hipStream_t s, Around &&around) {
  if (g.K <= 0) return;
  around([&]() { k_pf_gemv_rows<<<(g.K + 3) / 4, 256, 0, s>>>(g); });
}
}  // namespace stg
