// gfx950 kernels of the safeguards of the dense stage Hessians on the device - the parts of the reference's block BFGS that
// READ a block (hqp/Hqp_HL_BFGS.C:125-146 restart_Q, :203-212 the eigenvalue control; hqp/Hqp_HL_Gerschgorin.C:66-106):
//   rows      k_hg_rows (dense blocks) and k_hg_tiles / k_hg_finish (packed lower tiles): per variable i of stage k
//             rowmax_i = max_j |Q_k(i,j)| and offsum_i = sum_{j != i} |Q_k(i,j)| over the stage's order
//             (hqpkkt_hessian_row_stats)
//   restart   k_hg_clip: d_i = min(max(eps, rowmax_i), 1 / eps); k_hu_update applies Q_k <- diag(d_k) (beta = 0)
//   diagonal  k_hg_diag: the diagonal entries alone, set to max(q_ii, fl(offsum_i + eps)) (hqpkkt_gerschgorin_stage_hessians)
//             or shifted to fl(q_ii + d_k), hu_entry's operation with mode 1 (hqpkkt_eigen_control_stage_hessians)
//   Lanczos   k_he_start, k_he_step, k_he_ritz: the smallest eigenvalue of every block, all stages in lockstep, one
//             product staged_hess_symv per step; a conservative estimate lo - rho and the shift d_k = theta_k - (lo - rho)
// Plain loads and stores: no polled words, no waits between workgroups, no atomics.  The blocks are read 16 bytes per lane
// (rows of both layouts start at 16-byte boundaries); the vectors 8 bytes, a stage's first column may be odd.
// Included by staged_hess.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eigen_ritz.hip.h"

namespace stg {

static const int HE_MAX_STEPS = eig::MAX_STEPS;  // (HQPKKT_EIG_MAX_STEPS)
static const int HE_REPORT = eig::REPORT;        // (HQPKKT_EIG_REPORT)
static const int HE_STATE = 4;                   // per stage: done, steps, beta of the last step, max(|alpha|, beta) so far
#define HE_END_REL EIG_END_REL                   // (HQPKKT_EIG_END_REL)

// Per stage what these kernels need.  tiles: the stored tiles of a packed stage (0: the stage keeps its dense block);
// oS: its first slot in the scratch of k_hg_tiles, in doubles.
struct HgDesc {
  long long oQ, oS;
  int ld, nt, nz, col0, packed, tiles;
};

// max and min that keep a NaN once they have met one
__device__ __forceinline__ double hg_max(double m, double a) { return eig::nan_max(m, a); }
__device__ __forceinline__ double hg_min(double m, double a) { return eig::nan_min(m, a); }
__device__ __forceinline__ double hg_wave_max(double m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = hg_max(m, __shfl_xor(m, o));
  return m;
}
__device__ __forceinline__ double hg_wave_min(double m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = hg_min(m, __shfl_xor(m, o));
  return m;
}
// the address of Q_k(i, i): in the dense block, or in diagonal tile (a, a) of a packed stage
__device__ __forceinline__ long long hg_diag_at(const HgDesc &d, int i) {
  if (!d.packed) return d.oQ + (long long)i * d.ld + i;
  const int a = i / HP_T, r = i % HP_T;
  return d.oQ + ((long long)a * (a + 1) / 2 + a) * HP_T * HP_T + (long long)r * HP_T + r;
}

// Dense blocks: workgroup (.., k) takes rows of stage k, a wavefront per row (k_hs_symv's walk); a lane takes the column
// pairs lane, lane + 64, .. and adds |q| of its columns in ascending order, the diagonal entry left out; the wavefront's sum
// is kktdev::wave_sum, its maximum a butterfly.  Columns past nz are loaded with their pair and never enter.
__global__ void __launch_bounds__(256) k_hg_rows(const HgDesc *__restrict__ desc, const double *__restrict__ Q, double *__restrict__ rowmax,
                                                 double *__restrict__ offsum) {
  const HgDesc d = desc[blockIdx.y];
  if (d.packed) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x * 4 + wave; i < d.nz; i += gridDim.x * 4) {
    const hs_d2 *row = (const hs_d2 *)(Q + d.oQ + (long long)i * d.ld);
    double m = 0.0, s = 0.0;
    for (int p = lane; 2 * p < d.nz; p += 64) {
      const hs_d2 q = row[p];
      const int j = 2 * p;
      const double a0 = fabs(q.x);
      m = hg_max(m, a0);
      if (j != i) s += a0;
      if (j + 1 < d.nz) {
        const double a1 = fabs(q.y);
        m = hg_max(m, a1);
        if (j + 1 != i) s += a1;
      }
    }
    m = hg_wave_max(m), s = kktdev::wave_sum(s);
    if (lane == 0) {
      if (rowmax) rowmax[d.col0 + i] = m;
      if (offsum) offsum[d.col0 + i] = s;
    }
  }
}

// Packed stages: workgroup (t, k) takes stored tile t = (a, b) of stage k and loads every element once (the scheme of
// k_hp_symv_tiles).  Wavefront w takes the rows w, w + 4, .., a lane two columns.  Rows: |q| of a row's 128 columns - the
// lane's two first, then the wavefront by wave_sum / a butterfly - is the row's partial over column tile b and goes to slot
// (a, b).  Columns, off the diagonal tile: a lane's two columns over the wavefront's rows in ascending order, the four
// wavefronts in their order through LDS, is row j's partial over column tile a - the transpose's share - and goes to slot
// (b, a).  Slot (r, c) of a stage, HP_T doubles of maxima at smax and as many sums at ssum, lies at oS + (r nt + c) HP_T:
// nt^2 slots, each written by exactly one workgroup; k_hg_finish combines those of a row tile in ascending c.  Rows and
// columns past nz never enter (the tiles hold zeros there, which are not read as values either).
__global__ void __launch_bounds__(256, 2) k_hg_tiles(const HgDesc *__restrict__ desc, const double *__restrict__ Q, double *__restrict__ smax,
                                                     double *__restrict__ ssum) {
  const HgDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.tiles) return;
  __shared__ double pm[4][HP_T], ps[4][HP_T];
  int a, b;
  hp_tile_of(blockIdx.x, a, b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const hs_d2 *tile = (const hs_d2 *)(Q + d.oQ + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T);
  const int i0 = a * HP_T, j0 = b * HP_T + 2 * lane;
  const bool in0 = j0 < d.nz, in1 = j0 + 1 < d.nz;
  const int rows = min(HP_T, d.nz - i0);
  double *rm = smax + d.oS + ((long long)a * d.nt + b) * HP_T, *rs = ssum + d.oS + ((long long)a * d.nt + b) * HP_T;
  double cm0 = 0.0, cm1 = 0.0, cs0 = 0.0, cs1 = 0.0;
  for (int m = 0; m < HP_T / 4; m += 8) {
    hs_d2 v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {  // eight rows in flight per wavefront
      const int r = wave + 4 * (m + u);
      v[u] = hs_d2{0.0, 0.0};
      if (r < rows) v[u] = tile[r * (HP_T / 2) + lane];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int r = wave + 4 * (m + u);
      if (r >= rows) continue;  // (uniform over the wavefront)
      const int i = i0 + r;
      const double a0 = in0 ? fabs(v[u].x) : 0.0, a1 = in1 ? fabs(v[u].y) : 0.0;
      cm0 = hg_max(cm0, a0), cm1 = hg_max(cm1, a1), cs0 += a0, cs1 += a1;
      const double rmx = hg_wave_max(hg_max(a0, a1));
      const double rsm = kktdev::wave_sum((i == j0 ? 0.0 : a0) + (i == j0 + 1 ? 0.0 : a1));
      if (lane == 0) rm[r] = rmx, rs[r] = rsm;
    }
  }
  if (a == b) return;  // (uniform over the workgroup: a diagonal tile holds both triangles and counts by its rows)
  pm[wave][2 * lane] = cm0, pm[wave][2 * lane + 1] = cm1;
  ps[wave][2 * lane] = cs0, ps[wave][2 * lane + 1] = cs1;
  __syncthreads();
  if (threadIdx.x < HP_T) {
    const int t = threadIdx.x;
    const long long at = d.oS + ((long long)b * d.nt + a) * HP_T + t;
    smax[at] = hg_max(hg_max(hg_max(pm[0][t], pm[1][t]), pm[2][t]), pm[3][t]);
    ssum[at] = ((ps[0][t] + ps[1][t]) + ps[2][t]) + ps[3][t];
  }
}
// ... and the slots of a row tile in ascending order of the columns they cover: workgroup (r, k), a lane per row
__global__ void __launch_bounds__(HP_T) k_hg_finish(const HgDesc *__restrict__ desc, const double *__restrict__ smax, const double *__restrict__ ssum,
                                                    double *__restrict__ rowmax, double *__restrict__ offsum) {
  const HgDesc d = desc[blockIdx.y];
  const int r = blockIdx.x, i = r * HP_T + threadIdx.x;
  if (d.tiles == 0 || r >= d.nt || i >= d.nz) return;
  const long long at = d.oS + (long long)r * d.nt * HP_T + threadIdx.x;
  double m = 0.0, s = 0.0;
  for (int c = 0; c < d.nt; c++) m = hg_max(m, smax[at + (long long)c * HP_T]), s += ssum[at + (long long)c * HP_T];
  if (rowmax) rowmax[d.col0 + i] = m;
  if (offsum) offsum[d.col0 + i] = s;
}

// restart_Q's diagonal: d_i = min(max(eps, rowmax_i), 1 / eps), the reference's two comparisons in their order (a NaN row
// maximum ends as 1 / eps); inv = fl(1 / eps) comes from the host
__global__ void __launch_bounds__(256) k_hg_clip(long long n, const double *__restrict__ rowmax, double eps, double inv, double *__restrict__ dvec) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double rm = rowmax[i];
  const double t = eps > rm ? eps : rm;
  dvec[i] = t < inv ? t : inv;
}

// The diagonal entries alone; workgroup (.., k), a thread per variable of stage k.
//   mode 0   set to max: q_ii <- t where t = fl(offsum_i + eps) > q_ii (Hqp_HL_Gerschgorin::update)
//   mode 1   add: q_ii <- fl(q_ii + d_k), d_k = rep[HE_REPORT k + 7]; a stage with d_k == 0 is not touched
__global__ void __launch_bounds__(256) k_hg_diag(const HgDesc *__restrict__ desc, double *__restrict__ Q, const double *__restrict__ offsum, double eps,
                                                 const double *__restrict__ rep, int mode) {
  const HgDesc d = desc[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.nz) return;
  double *q = Q + hg_diag_at(d, i);
  if (mode == 0) {
    const double t = __dadd_rn(offsum[d.col0 + i], eps);
    if (t > *q) *q = t;
  } else {
    const double dk = rep[(long long)HE_REPORT * blockIdx.y + 7];
    if (dk != 0.0) *q = __dadd_rn(*q, dk);
  }
}

// The workgroup's minimum (NaN kept), the same bits in every thread: hb_block_sum's walk
__device__ __forceinline__ double hg_block_min(double a, double *red) {
  a = hg_wave_min(a);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return hg_min(hg_min(hg_min(red[0], red[1]), red[2]), red[3]);
}

// entry i of the start vector before it is normalised
__device__ __forceinline__ double he_start_entry(int i) { return eig::start_entry(i); }

// Workgroup k: stage k ahead of the recurrence.  g = min_i (q_ii - offsum_i), Gerschgorin's lower bound of the spectrum;
// the floor theta: flr[k] where the host gave one (not NaN), else eps2 = fl(eps eps) - lowered to sQs where bfgs (the
// report words of the last k_hb_terms) holds 0 <= sQs < eps2, the reference's rule.  Order 0: outcome 5; g >= theta:
// outcome 0, no shift; both are done, and their share of the basis V stays 0 as the host cleared it.  Every other stage
// starts from v_0 = f / sqrt(sum f_i^2), f_i = he_start_entry(i), the sum as in hb_block_sum.  T, the report and the state of
// the stage are cleared.
__global__ void __launch_bounds__(256) k_he_start(const HgDesc *__restrict__ desc, const double *__restrict__ Q, const double *__restrict__ offsum,
                                                  const double *__restrict__ flr, double eps2, const double *__restrict__ bfgs,
                                                  double *__restrict__ st, double *__restrict__ rep, double *__restrict__ T, double *__restrict__ V) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  __shared__ int pending;
  const int k = blockIdx.x;
  const HgDesc d = desc[k];
  double g = __builtin_inf(), a = 0.0;
  for (int i = threadIdx.x; i < d.nz; i += 256) {
    g = hg_min(g, Q[hg_diag_at(d, i)] - offsum[d.col0 + i]);
    const double f = he_start_entry(i);
    a = __fma_rn(f, f, a);
  }
  g = hg_block_min(g, red);
  const double nrm = sqrt(hb_block_sum(a, red));
  T[(long long)2 * HE_MAX_STEPS * k + threadIdx.x] = 0.0;  // (256 = 2 HE_MAX_STEPS words)
  if (threadIdx.x == 0) {
    double theta = flr[k];
    if (theta != theta) {
      theta = eps2;
      if (bfgs) {
        const double sQs = bfgs[(long long)HB_REPORT * k + 1];
        if (sQs < theta && sQs >= 0.0) theta = sQs;
      }
    }
    const int outcome = d.nz == 0 ? 5 : g >= theta ? 0 : -1;
    double *r = rep + (long long)HE_REPORT * k;
    r[0] = d.nz == 0 ? 0.0 : g, r[1] = theta;
    for (int q = 2; q < HE_REPORT - 1; q++) r[q] = 0.0;
    r[HE_REPORT - 1] = (double)outcome;
    double *s = st + (long long)HE_STATE * k;
    s[0] = outcome < 0 ? 0.0 : 1.0, s[1] = 0.0, s[2] = 0.0, s[3] = 0.0;
    pending = outcome < 0;
  }
  __syncthreads();
  if (!pending) return;
  for (int i = threadIdx.x; i < d.nz; i += 256) V[d.col0 + i] = he_start_entry(i) / nrm;
}

// k_he_step runs a stage on sixteen wavefronts: one workgroup per stage is all the recurrence offers (its sums stay inside
// it), the step is bound by the latency of its loads, and four wavefronts took as long over a step as the product ahead of it
static const int HE_STEP_THREADS = 1024;
// the workgroup's sum of a, the same bits in every thread: hb_block_sum for HE_STEP_THREADS / 64 wavefronts, in their order
__device__ __forceinline__ double he_block_sum(double a, double *red) {
  a = kktdev::wave_sum(a);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int q = 1; q < HE_STEP_THREADS / 64; q++) s += red[q];
  return s;
}

// Workgroup k: step j of stage k, behind w = Q v_j.  The basis vectors v_0 .. v_j of all stages lie in V, vector i at
// V + i n.  alpha = v_j'w; w <- fl(fl(w - fl(alpha v_j)) - fl(beta_{j-1} v_{j-1})), every operation rounded on its own;
// then w is made orthogonal to the whole basis once more, w <- w - sum_i (v_i'w) v_i: without that the recurrence grows
// a second copy of an eigenvalue a few steps after it has converged, and the residual bound of k_he_ritz means nothing
// while the copy is on its way.  Wavefront q forms the products v_i'w, i = q, q + 16, .., a lane's share by fused
// multiply-adds in ascending order, then wave_sum; they are taken off in ascending i, each product and difference
// rounded on its own.  beta = sqrt(w'w); alpha and w'w by he_block_sum.  T[2 HE_MAX_STEPS k + j] = alpha,
// T[.. + HE_MAX_STEPS + j] = beta.  The stage ends itself where j + 1 equals its order, or where beta > HE_END_REL
// max(|alpha_0 .. alpha_j|, beta_0 .. beta_{j-1}) does not hold (an invariant subspace - or a value that is not finite):
// it is done, and v_{j+1} stays 0.  Otherwise v_{j+1} = w / beta (not written behind the last step: last).  A stage that is
// done returns at once.
__global__ void __launch_bounds__(HE_STEP_THREADS) k_he_step(const HgDesc *__restrict__ desc, double *__restrict__ st, double *__restrict__ T, double *__restrict__ V,
                                                 double *__restrict__ w, long long n, int j, int last) {
#pragma clang fp contract(off)
  __shared__ double red[HE_STEP_THREADS / 64], cf[HE_MAX_STEPS];
  __shared__ int ended;
  const int k = blockIdx.x;
  double *s = st + (long long)HE_STATE * k;
  if (s[0] != 0.0) return;  // (uniform over the workgroup; thread 0 writes the state behind the barriers of the sums)
  const double bprev = s[2], scale0 = s[3];
  const int nz = desc[k].nz;
  double *V0 = V + desc[k].col0, *wk = w + desc[k].col0;
  const double *vk = V0 + (long long)j * n, *pk = V0 + (long long)(j > 0 ? j - 1 : 0) * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < nz; i += HE_STEP_THREADS) a = __fma_rn(vk[i], wk[i], a);
  const double alpha = he_block_sum(a, red);
  for (int i = threadIdx.x; i < nz; i += HE_STEP_THREADS) {
    double t = wk[i] - alpha * vk[i];
    if (j > 0) t = t - bprev * pk[i];
    wk[i] = t;
  }
  __syncthreads();  // (w as the workgroup has just written it)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q <= j; q += HE_STEP_THREADS / 64) {
    const double *vq = V0 + (long long)q * n;
    double c = 0.0;
    for (int i = lane; i < nz; i += 64) c = __fma_rn(vq[i], wk[i], c);
    c = kktdev::wave_sum(c);
    if (lane == 0) cf[q] = c;
  }
  __syncthreads();
  double b = 0.0;
  for (int i = threadIdx.x; i < nz; i += HE_STEP_THREADS) {
    double t = wk[i];
    for (int q = 0; q <= j; q++) t = t - cf[q] * V0[(long long)q * n + i];
    wk[i] = t;
    b = __fma_rn(t, t, b);
  }
  const double beta = sqrt(he_block_sum(b, red));
  if (threadIdx.x == 0) {
    const double scale = hg_max(scale0, fabs(alpha));
    const bool end = j + 1 >= nz || !(beta > HE_END_REL * scale);
    T[(long long)2 * HE_MAX_STEPS * k + j] = alpha, T[(long long)2 * HE_MAX_STEPS * k + HE_MAX_STEPS + j] = beta;
    s[0] = end ? 1.0 : 0.0, s[1] = (double)(j + 1), s[2] = beta, s[3] = hg_max(scale, beta);
    ended = end;
  }
  __syncthreads();
  if (ended || last) return;
  double *vn = V0 + (long long)(j + 1) * n;
  for (int i = threadIdx.x; i < nz; i += HE_STEP_THREADS) vn[i] = wk[i] / beta;
}

// Workgroup k, one wavefront: the smallest eigenvalue of stage k's tridiagonal T and the shift - eig::ritz
// (eigen_ritz.hip.h, which says what it does; hqpkkt_q_eigen_control runs the same body on the blocks of the sparse Q).
// rep[HE_REPORT k ..]: g, theta (k_he_start), steps, lo, hi, rho, lambda_est, d, |T|, outcome.
__global__ void __launch_bounds__(64) k_he_ritz(const double *__restrict__ st, const double *__restrict__ T, double *__restrict__ rep) {
  __shared__ eig::RitzLds lds;
  const int k = blockIdx.x;
  double *r = rep + (long long)HE_REPORT * k;
  if (r[HE_REPORT - 1] >= 0.0) return;  // (outcome 0 or 5: decided by k_he_start)
  const int m = min((int)st[(long long)HE_STATE * k + 1], HE_MAX_STEPS);  // (m < 1: the host launches no step for orders of 0 alone)
  const double *al = T + (long long)2 * HE_MAX_STEPS * k;
  eig::ritz(al, al + HE_MAX_STEPS, m, r[1], r, lds);
}

}  // namespace stg
