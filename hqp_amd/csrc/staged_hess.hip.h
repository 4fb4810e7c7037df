// gfx950 kernels of the dense stage Hessians (hqpkkt_set_hessian_form, StagedPlan::hess_dense): block Q_k of stage
// k = 0 .. K, order nz_k, kept in full and exactly symmetric as nz_k rows of ld = up8(nz_k) doubles, zero padded.
//   store     the caller's block is copied into the arena, then k_hs_mirror writes the strict lower triangle from the
//             upper one (dense hand-over); k_hs_scatter puts the CSR values to both of their places (CSR hand-over)
//   assembly  k_hs_add: a rectangle of Q_k added into the stage's work block G or into V_k, one read of Q and one
//             read-modify-write of the target, 16 bytes per lane
//   products  k_hs_symv: y = Q x over all stages in one launch, a wavefront per row, a fixed order of the sums
//   update    k_hu_update (staged_hess_update.hip.h): Q_k <- beta_k Q_k + diag(d_k) + sum_j c_kj u_j u_j' in place
//             k_hb_terms (staged_hess_bfgs.hip.h): the damped BFGS update's v and coefficients per stage, into that launch's descriptors
//   guards    k_hg_* / k_he_* (staged_hess_guard.hip.h): row maxima and off-diagonal sums of every block, restart_Q, Gerschgorin's
//             diagonal, and the eigenvalue control by a Lanczos recurrence over all stages
// Plain loads and stores: no polled words, no waits between workgroups, no atomics.  Included by staged_engine.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace stg {

typedef double hs_d2 __attribute__((ext_vector_type(2)));

// CSR hand-over: stored entry e of Q to dst[2 e] and to its image dst[2 e + 1] (-1: none)
__global__ void __launch_bounds__(256) k_hs_scatter(long long nent, const long long *__restrict__ dst, const double *__restrict__ vals,
                                                    double *__restrict__ Q) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  const long long d0 = dst[2 * e], d1 = dst[2 * e + 1];
  const double v = vals[e];
  if (d0 >= 0) Q[d0] = v;
  if (d1 >= 0) Q[d1] = v;
}

// The upper triangle of a block mirrored in place, in tiles of HS_TILE x HS_TILE, one workgroup per tile on or above the
// diagonal (T (T + 1) / 2 of them, row by row): workgroup (a, b), a < b, reads tile (a, b) and writes its transpose to tile
// (b, a); a diagonal tile is loaded whole - what it held below the diagonal with it - and rewritten from its upper
// triangle alone, so nothing the block held below the diagonal reaches the result.  The padding columns [nz, ld) of the
// rows a workgroup writes get zeros; those of the rows in the tiles above the diagonal are not written here: they are
// zero because the arena is cleared at upload and the copy ahead of this kernel is nz columns wide.
static const int HS_TILE = 32;
__global__ void __launch_bounds__(256) k_hs_mirror(double *__restrict__ Q, long long ld, int nz, int T) {
  __shared__ double t[HS_TILE][HS_TILE + 1];
  int a = 0, rest = blockIdx.x;  // (tile row a holds T - a tiles)
  while (rest >= T - a) rest -= T - a, a++;
  const int b = a + rest;
  const int r0 = a * HS_TILE, c0 = b * HS_TILE;
  // rows r0 .. of the columns c0 ..: 16 lanes of 16 bytes per row (ld and c0 are even)
  for (int u = threadIdx.x; u < HS_TILE * HS_TILE / 2; u += 256) {
    const int r = u / (HS_TILE / 2), c = 2 * (u % (HS_TILE / 2));
    hs_d2 v{0.0, 0.0};
    if (r0 + r < nz && c0 + c < nz) {
      v = *(const hs_d2 *)&Q[(long long)(r0 + r) * ld + c0 + c];
      if (c0 + c + 1 >= nz) v.y = 0.0;
    }
    t[r][c] = v.x, t[r][c + 1] = v.y;
  }
  __syncthreads();
  // rows c0 .. of the columns r0 ..: the transpose; on the diagonal tile entry (i, j) = t[min][max]
  for (int u = threadIdx.x; u < HS_TILE * HS_TILE / 2; u += 256) {
    const int i = u / (HS_TILE / 2), j = 2 * (u % (HS_TILE / 2));
    if (c0 + i >= nz || r0 + j >= ld) continue;
    hs_d2 v;
    if (a == b)
      v.x = i <= j ? t[i][j] : t[j][i], v.y = i <= j + 1 ? t[i][j + 1] : t[j + 1][i];
    else
      v.x = t[j][i], v.y = t[j + 1][i];
    *(hs_d2 *)&Q[(long long)(c0 + i) * ld + r0 + j] = v;
  }
}

// G[i][j] += Q[i][j] for the rows [r0, r1) and the columns [0, c1) of a block; lower: of row i only the columns up to the
// end of its 128-wide diagonal block.  That covers what a lower-tile product has written fresh, whichever tiles it takes:
// with 64 x 64 tiles the upper 64-tile of a diagonal block is left over from earlier products and gets Q as well - as it
// gets the lists' entries in form 0 - and nobody reads it.  Workgroup (x, y): 256 column pairs of the rows y, y + gridDim.y, ..
// Both leading dimensions are even and both blocks start at a 16-byte boundary.
struct HsAdd {
  const double *Q;
  long long ldq;
  double *G;
  long long ldg;
  int r0, r1, c1, lower;
};
__global__ void __launch_bounds__(256) k_hs_add(HsAdd a) {
  const int j = 2 * (blockIdx.x * 256 + threadIdx.x);
  for (int i = a.r0 + blockIdx.y; i < a.r1; i += gridDim.y) {
    const int lim = a.lower ? min(a.c1, ((i >> 7) + 1) << 7) : a.c1;
    if (j >= lim) continue;
    const double *q = a.Q + (long long)i * a.ldq + j;
    double *g = a.G + (long long)i * a.ldg + j;
    if (j + 1 < lim) {
      const hs_d2 x = *(const hs_d2 *)q;
      hs_d2 y = *(hs_d2 *)g;
      y.x += x.x, y.y += x.y;
      *(hs_d2 *)g = y;
    } else
      g[0] += q[0];
  }
}

// y = Q x over the blocks of all stages: workgroup (.., k) takes rows of stage k, a wavefront per row; a lane sums the
// column pairs lane, lane + 64, .. of the row, even and odd columns apart, and the wavefront's sum is a butterfly: the
// order is fixed by the block's order alone.  Reads the whole block (rows are contiguous)
struct HessDesc {
  long long oQ;
  int ld, nz, col0, pad;
};
__global__ void __launch_bounds__(256) k_hs_symv(const HessDesc *__restrict__ desc, const double *__restrict__ Q, const double *__restrict__ x,
                                                 double *__restrict__ y) {
  const HessDesc d = desc[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *xs = x + d.col0;
  for (int i = blockIdx.x * 4 + wave; i < d.nz; i += gridDim.x * 4) {
    const hs_d2 *row = (const hs_d2 *)(Q + d.oQ + (long long)i * d.ld);
    double s0 = 0.0, s1 = 0.0;
    for (int p = lane; 2 * p < d.nz; p += 64) {
      const hs_d2 q = row[p];
      s0 += q.x * xs[2 * p];
      if (2 * p + 1 < d.nz) s1 += q.y * xs[2 * p + 1];
    }
    const double s = kktdev::wave_sum(s0 + s1);
    if (lane == 0) y[d.col0 + i] = s;
  }
}

}  // namespace stg

#include "staged_hess_packed.hip.h"  // (the same blocks stored as packed lower tiles)
#include "staged_hess_update.hip.h"  // (both layouts updated in place: hqpkkt_update_stage_hessians)
#include "staged_hess_bfgs.hip.h"    // (the damped BFGS terms of that update on the device: hqpkkt_bfgs_update_stage_hessians)
#include "staged_hess_guard.hip.h"   // (row statistics, restart_Q, Gerschgorin and the eigenvalue control: hqpkkt_hessian_row_stats ..)
