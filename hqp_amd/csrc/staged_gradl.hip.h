// gfx950 kernel of hqpkkt_lagrangian_gradient_staged (include/hqpkkt.h): grad L = c - A'y - C'z of Hqp_SqpSolver::grd_L on a
// handle of the dense hand-over, whose dynamics rows are the blocks F_k and not entries of A.  One launch, blockIdx.y =
// stage, over the DynDesc table of the residual's pass (k_st_dyn_both, staged.hip.h): the transposed product alone, so
// the pass keeps that kernel's loads and drops its A x half - the row sums' 48 shuffles per eight rows, the `part`
// buffer and the finish launch - and ends in the walk over the variable's rows of E' and C' and the subtractions.
// Plain loads and stores in the handle's stream: no polled words, no waits between workgroups, no atomics.  Every
// operation is the one the header promises: compiled without contraction, the sums by __fma_rn.
// Included by staged_engine.hip behind staged.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.hip.h"

namespace stg {

// Workgroup (bx, k): the columns 256 bx .. 256 bx + 255 of stage k - of F_k where k < K, of the states x_K where k = K
// (np = 0: no block, and its ncur columns may span several column blocks).  Wavefront w takes the rows w, w + 4, .. of
// the block in ascending order, lane l the columns l, l + 64, l + 128, l + 192 of the workgroup's 256: a wave
// instruction reads 512 contiguous bytes, eight rows' loads (32 per lane) are issued before the first is used.  A
// column's four wavefront sums meet in LDS as (w0 + w1) + (w2 + w3); thread t then finishes column t:
//   t_i = that sum - y[the dynamics row that produces x_k's component]   (k > 0, a state column)
//         + row i of E' times y, then row i of C' times z: one accumulator, fused multiply-adds in ascending order
//   out_i = fl(c_i - t_i), then fl(out_i - minus_i) where minus is given
// So a column's bits depend on its stage's sizes and values alone - not on the grid, not on K.
// Every offset into F is 64 bits wide (5 10^9 doubles at K = 200, nx = 5000).
__global__ void __launch_bounds__(256) k_st_grad_l(const DynDesc *__restrict__ desc, const double *__restrict__ F, kktdev::CsrDev AT,
                                                   kktdev::CsrDev CT, const double *__restrict__ c, const double *__restrict__ y,
                                                   const double *__restrict__ z, const double *__restrict__ minus,
                                                   double *__restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double cs[4][256];
  const DynDesc d = desc[blockIdx.y];
  const int ncols = d.np > 0 ? d.nz : d.ncur;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (uniform: the rows' multipliers come by scalar loads)
  const int c0 = blockIdx.x * 256;
  if (c0 >= ncols) return;  // (uniform)
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (d.np > 0) {  // (uniform; the last stage has no block to sweep)
    // the column guard, once: a lane past the block's last column sweeps column 0 instead, and its sums are never read
    const long long step = 4LL * d.ldf;  // from a row of this wavefront to its next
    long long o[4];  // this lane's four columns in the wavefront's first row, as offsets into F
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int lc = c0 + lane + 64 * g;
      o[g] = d.oF + (long long)wave * d.ldf + (lc < ncols ? lc : 0);
    }
    const double *yw = y + d.row0;
    int li = wave;
    for (; li + 28 < d.np; li += 32) {  // eight rows of this wavefront per trip, all of them inside the block
      double v[8][4], yv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        yv[u] = yw[li + 4 * u];
#pragma unroll
        for (int g = 0; g < 4; g++) v[u][g] = F[o[g] + u * step];
      }
      __builtin_amdgcn_sched_barrier(0);  // all 32 loads of the trip are in flight before the first is used
#pragma unroll
      for (int u = 0; u < 8; u++)
#pragma unroll
        for (int g = 0; g < 4; g++) s[g] = __fma_rn(v[u][g], yv[u], s[g]);
#pragma unroll
      for (int g = 0; g < 4; g++) o[g] += 8 * step;
    }
    for (; li < d.np; li += 4) {  // the row guard, once: the block's last rows (at most seven of a wavefront) one by one
      const double yv = yw[li];
#pragma unroll
      for (int g = 0; g < 4; g++) {
        s[g] = __fma_rn(F[o[g]], yv, s[g]);
        o[g] += step;
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; g++) cs[wave][lane + 64 * g] = s[g];
  __syncthreads();
  const int lc = c0 + tid;
  if (lc >= ncols) return;
  const long long i = (long long)d.col0 + lc;
  double t = (cs[0][tid] + cs[1][tid]) + (cs[2][tid] + cs[3][tid]);
  // x_k is the state the previous stage's dynamics produce: -1.0 in that row
  if (blockIdx.y > 0 && lc < d.ncur) t = t - y[d.row0 - d.ncur + lc];
  for (int k = AT.ptr[i], e = AT.ptr[i + 1]; k < e; k++) t = __fma_rn(AT.val[k], y[AT.col[k]], t);
  for (int k = CT.ptr[i], e = CT.ptr[i + 1]; k < e; k++) t = __fma_rn(CT.val[k], z[CT.col[k]], t);
  double g = c[i] - t;
  if (minus) g = g - minus[i];
  out[i] = g;
}

}  // namespace stg
