// gfx950 kernel of the in-place update of the dense stage Hessians (hqpkkt_update_stage_hessians): over every stage k
//   Q_k <- beta_k Q_k + diag(d_k) + sum_{j < r} c_kj u_jk u_jk',
// on both layouts of the arena - the dense block (staged_hess.hip.h), both triangles, and the packed lower tiles
// (staged_hess_packed.hip.h), the stored tiles alone.  One launch over all stages, grid (units, K + 1); a workgroup takes one
// HP_T x HP_T tile: of a dense stage tile t = (t / nt, t % nt) of the block, of a packed stage stored tile t = (a, b), b <= a.
// Every stored entry is computed at its own place by hu_entry, whose value does not change when i and j trade places: the
// product u_i u_j is rounded on its own, so a dense block and a diagonal tile stay symmetric bit for bit, and a packed and an
// unpacked handle hold the same bits.  A memory-bound kernel: one read (none with beta = 0) and one write of 16 bytes per lane.
// Plain loads and stores: no polled words, no waits between workgroups, no atomics.  Included by staged_hess.hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace stg {

static const int HU_RANK = 4;  // (HQPKKT_HESS_UPDATE_RANK)

// Per stage what the launch needs.  units: the tiles of the stage, 0 where the call leaves the stage alone.  mode: 0 the
// block is not read (beta = 0), 1 it is taken as it is (beta = 1), 2 it is scaled.  c[j] == 0: term j is skipped, its
// vector is not read.
struct HuDesc {
  long long oQ;
  int ld, nt, nz, col0;
  int packed, units, mode, pad;
  double beta, c[HU_RANK];
};
struct HuVecs {
  const double *u[HU_RANK];
  const double *diag;  // null: none
  int r;
};

// The value of entry (i, j): q scaled, then the diagonal's share, then the terms 0 .. r - 1 in their order; every
// operation rounded on its own (no contraction across the product u_i u_j), ui[j] uj[j] = uj[j] ui[j] bit for bit.
__device__ __forceinline__ double hu_entry(double q, int mode, double beta, bool on_diag, double dd, int r, const double (&c)[HU_RANK],
                                           const double (&ui)[HU_RANK], const double (&uj)[HU_RANK]) {
  double v = mode == 0 ? 0.0 : mode == 1 ? q : __dmul_rn(beta, q);
  if (on_diag) v = __dadd_rn(v, dd);
#pragma unroll
  for (int j = 0; j < HU_RANK; j++)
    if (j < r && c[j] != 0.0) v = __fma_rn(c[j], __dmul_rn(ui[j], uj[j]), v);
  return v;
}

// Workgroup (t, k): tile t of stage k.  The slices of the vectors over the tile's rows (and of the diagonal) go to LDS, those
// over a lane's two columns to registers, both 0 past the stage's order - what lies there belongs to the next stage.
// Wavefront w takes the rows w, w + 4, .. of the tile, a lane the column pair 2 lane, 2 lane + 1, eight rows in flight.
// Only entries with i, j < nz are written, so the padding keeps its +0.0; of a pair that straddles nz the second value is
// written as +0.0.  Leading dimensions are even, blocks and tiles start at 16-byte boundaries.
static const int HU_ROWS = 8;
__global__ void __launch_bounds__(256, 2) k_hu_update(const HuDesc *__restrict__ desc, double *__restrict__ Q, HuVecs V) {
  const HuDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.units) return;
  __shared__ double ur[HU_RANK][HP_T], dr[HP_T];
  int a, b;
  long long stride;
  double *tile;
  if (d.packed) {
    hp_tile_of(blockIdx.x, a, b);
    stride = HP_T;
    tile = Q + d.oQ + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T;
  } else {
    a = blockIdx.x / d.nt, b = blockIdx.x % d.nt;
    stride = d.ld;
    tile = Q + d.oQ + (long long)a * HP_T * d.ld + (long long)b * HP_T;
  }
  const int i0 = a * HP_T, j0 = b * HP_T;
  const bool diag_tile = a == b && V.diag != nullptr;
  double c[HU_RANK];
#pragma unroll
  for (int j = 0; j < HU_RANK; j++) c[j] = j < V.r ? d.c[j] : 0.0;
  if (threadIdx.x < HP_T) {
    const int i = i0 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < HU_RANK; j++) ur[j][threadIdx.x] = (c[j] != 0.0 && i < d.nz) ? V.u[j][d.col0 + i] : 0.0;
    dr[threadIdx.x] = (diag_tile && i < d.nz) ? V.diag[d.col0 + i] : 0.0;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int jc = j0 + 2 * lane;  // the lane's first column
  double uc0[HU_RANK], uc1[HU_RANK];
#pragma unroll
  for (int j = 0; j < HU_RANK; j++) {
    uc0[j] = (c[j] != 0.0 && jc < d.nz) ? V.u[j][d.col0 + jc] : 0.0;
    uc1[j] = (c[j] != 0.0 && jc + 1 < d.nz) ? V.u[j][d.col0 + jc + 1] : 0.0;
  }
  __syncthreads();
  if (jc >= d.nz) return;
  const bool second = jc + 1 < d.nz;
  const int rows = min(HP_T, d.nz - i0);  // (> 0: the tile exists)
  for (int m = 0; m < HP_T / 4; m += HU_ROWS) {
    hs_d2 q[HU_ROWS];
#pragma unroll
    for (int u = 0; u < HU_ROWS; u++) {
      const int r = wave + 4 * (m + u);
      q[u] = hs_d2{0.0, 0.0};
      if (d.mode != 0 && r < rows) q[u] = *(const hs_d2 *)(tile + (long long)r * stride + 2 * lane);
    }
#pragma unroll
    for (int u = 0; u < HU_ROWS; u++) {
      const int r = wave + 4 * (m + u);
      if (r >= rows) continue;
      double ui[HU_RANK];
#pragma unroll
      for (int j = 0; j < HU_RANK; j++) ui[j] = ur[j][r];
      const int i = i0 + r;
      hs_d2 v;
      v.x = hu_entry(q[u].x, d.mode, d.beta, diag_tile && i == jc, dr[r], V.r, c, ui, uc0);
      v.y = second ? hu_entry(q[u].y, d.mode, d.beta, diag_tile && i == jc + 1, dr[r], V.r, c, ui, uc1) : 0.0;
      *(hs_d2 *)(tile + (long long)r * stride + 2 * lane) = v;
    }
  }
}

}  // namespace stg
