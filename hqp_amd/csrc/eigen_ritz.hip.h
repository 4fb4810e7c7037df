// What both eigenvalue controls do with the tridiagonal T of one Lanczos recurrence - hqpkkt_eigen_control_stage_hessians
// (k_he_ritz, staged_hess_guard.hip.h) and hqpkkt_q_eigen_control (k_qe_ritz, q_eigen.hip.h): ONE body, so that a T gives
// the same report words in both, and hessian_update.eigen_replay repeats both in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace eig {

static const int MAX_STEPS = 128;  // (HQPKKT_EIG_MAX_STEPS)
static const int REPORT = 10;      // (HQPKKT_EIG_REPORT)
#define EIG_END_REL 0x1p-40        // (HQPKKT_EIG_END_REL)

// max and min that keep a NaN once they have met one (a > m is false for a NaN on either side)
__device__ __forceinline__ double nan_max(double m, double a) { return (a > m || a != a) ? a : m; }
__device__ __forceinline__ double nan_min(double m, double a) { return (a < m || a != a) ? a : m; }

// entry i of the start vector before it is normalised: 1 + ((37 i + 11) mod 64) / 64, in [1, 2), exact
__device__ __forceinline__ double start_entry(int i) { return 1.0 + (double)((37 * i + 11) & 63) * 0.015625; }

// the work arrays of ritz: one set per workgroup of one wavefront
struct RitzLds {
  double al[MAX_STEPS], be[MAX_STEPS], b2[MAX_STEPS], pv[MAX_STEPS], rv[MAX_STEPS], z[MAX_STEPS];
};

// One wavefront, the only one of its workgroup: the smallest eigenvalue of the tridiagonal T (order m = steps, diagonal
// alpha_0 .. alpha_{m-1}, off-diagonal beta_0 .. beta_{m-2}; beta_{m-1} is the norm of the last residual) and the shift
// for the floor theta.  Every operation rounded on its own; hessian_update.eigen_replay repeats them in numpy.
//   norm      |T| = max_i (|alpha_i| + |beta_{i-1}| + |beta_i|), and Gerschgorin's interval [gl, gu] of T; not finite: outcome 4
//   bracket   lo = gl - tol, hi = gu + tol, tol = 2^-50 |T|; while hi - lo > tol (32 rounds at most) lane l counts the
//             eigenvalues below x_l = lo + fl((hi - lo) c_l), c_l = fl((l + 1) / 65), by the Sturm sequence
//             p_0 = alpha_0 - x, p_i = fl(fl(alpha_i - x) - fl(fl(beta_{i-1}^2) / p_{i-1})), a |p| below pivmin = max(2^-104 |T|,
//             2^-1000) replaced by pivmin with its sign; hi becomes the first x_l with a count >= 1 and lo the point before it
//   residual  by lane 0: one step of inverse iteration with T - lo I from a unit vector e_t, by the twisted factorisation -
//             p_i above at x = lo, the same sequence r_i from the last row upwards, t the first index with the smallest
//             |fl(fl(p_i + r_i) - fl(alpha_i - lo))|; z_t = 1, z_i = -fl(fl(beta_i / p_i) z_{i+1}) above t and z_{i+1} =
//             -fl(fl(beta_i / r_{i+1}) z_i) below it: products alone, so that a last component far below the rounding
//             unit keeps its digits; rho = |beta_{m-1}| fl(|z_{m-1}| / sqrt(z'z)), z'z by separate products and sums
//   shift     lambda_est = lo - rho; not finite: outcome 4, left alone; lambda_est < theta: d = theta - lambda_est, outcome 2
//             where rho <= EIG_END_REL |T|, else 3; otherwise d = 0, outcome 1
// r: the REPORT words of the block - of g, theta (the caller's start kernel wrote them), steps, lo, hi, rho, lambda_est, d,
// |T|, outcome this writes 2 .. 9 (of a T that is not finite 2, 8 and 9 alone).  m < 1: no step has run (outcome 4).
__device__ __forceinline__ void ritz(const double *__restrict__ alpha, const double *__restrict__ beta, int m, double theta,
                                     double *__restrict__ r, RitzLds &w) {
#pragma clang fp contract(off)
  double *al = w.al, *be = w.be, *b2 = w.b2, *pv = w.pv, *rv = w.rv, *z = w.z;
  const int lane = threadIdx.x;
  for (int i = lane; i < m; i += 64) {
    const double bi = beta[i];
    al[i] = alpha[i], be[i] = bi, b2[i] = bi * bi;
  }
  __syncthreads();
  double normT = 0.0, gl = __builtin_inf(), gu = -__builtin_inf();
  for (int i = 0; i < m; i++) {
    const double off = (i > 0 ? fabs(be[i - 1]) : 0.0) + (i < m - 1 ? fabs(be[i]) : 0.0);
    normT = nan_max(normT, fabs(al[i]) + off);
    gl = nan_min(gl, al[i] - off), gu = nan_max(gu, al[i] + off);
  }
  if (m < 1 || !isfinite(normT)) {
    if (lane == 0) r[2] = (double)m, r[8] = normT, r[REPORT - 1] = 4.0;
    return;
  }
  const double tol = 0x1p-50 * normT, pivmin = fmax(0x1p-104 * normT, 0x1p-1000);
  double lo = gl - tol, hi = gu + tol;
  const double c = (double)(lane + 1) / 65.0;
  for (int round = 0; round < 32 && hi - lo > tol; round++) {
    const double x = lo + (hi - lo) * c;
    double p = al[0] - x;
    int cnt = p < 0.0;
    for (int i = 1; i < m; i++) {
      if (fabs(p) < pivmin) p = p < 0.0 ? -pivmin : pivmin;
      p = (al[i] - x) - b2[i - 1] / p;
      cnt += p < 0.0;
    }
    const unsigned long long mask = __ballot(cnt >= 1);
    if (mask == 0ull)
      lo = __shfl(x, 63);
    else {
      const int f = __ffsll((long long)mask) - 1;
      hi = __shfl(x, f);
      if (f > 0) lo = __shfl(x, f - 1);
    }
  }
  if (lane != 0) return;
  pv[0] = al[0] - lo;
  for (int i = 1; i <= m; i++) {
    double p = pv[i - 1];
    if (fabs(p) < pivmin) p = p < 0.0 ? -pivmin : pivmin;
    pv[i - 1] = p;
    if (i < m) pv[i] = (al[i] - lo) - b2[i - 1] / p;
  }
  rv[m - 1] = al[m - 1] - lo;
  for (int i = m - 1; i >= 0; i--) {
    double p = rv[i];
    if (fabs(p) < pivmin) p = p < 0.0 ? -pivmin : pivmin;
    rv[i] = p;
    if (i > 0) rv[i - 1] = (al[i - 1] - lo) - b2[i - 1] / p;
  }
  int t = 0;
  double gmin = __builtin_inf();
  for (int i = 0; i < m; i++) {
    const double gam = fabs((pv[i] + rv[i]) - (al[i] - lo));
    if (gam < gmin) gmin = gam, t = i;
  }
  z[t] = 1.0;
  for (int i = t - 1; i >= 0; i--) z[i] = -((be[i] / pv[i]) * z[i + 1]);
  for (int i = t; i < m - 1; i++) z[i + 1] = -((be[i] / rv[i + 1]) * z[i]);
  double zz = 0.0;
  for (int i = 0; i < m; i++) zz = zz + z[i] * z[i];  // (two roundings: no contraction in this body)
  const double rho = fabs(be[m - 1]) * (fabs(z[m - 1]) / sqrt(zz));
  const double lam = lo - rho;
  double dk = 0.0;
  int outcome;
  if (!isfinite(lam))
    outcome = 4;
  else if (lam < theta)
    dk = theta - lam, outcome = rho <= EIG_END_REL * normT ? 2 : 3;
  else
    outcome = 1;
  r[2] = (double)m, r[3] = lo, r[4] = hi, r[5] = rho, r[6] = lam, r[7] = dk, r[8] = normT, r[REPORT - 1] = (double)outcome;
}

}  // namespace eig
