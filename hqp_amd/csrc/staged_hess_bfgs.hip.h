// gfx950 kernel of the damped BFGS update of the dense stage Hessians on the device (hqpkkt_bfgs_update_stage_hessians):
// per stage k the scalars s'y and s'Qs of the reference's Hqp_HL_BFGS::update_b_Q, Powell's test, the vector v and the two
// coefficients of Q+ = Q + c0 v v' + c1 (Qs)(Qs)', written straight into the DEVICE descriptors of the update launch
// (HuDesc::c[0], c[1] and units, staged_hess_update.hip.h) - k_hu_update behind it in the stream applies them unchanged.
// One launch over all stages, one workgroup of 256 threads per stage: a stage's three slices are a few thousand doubles
// each (3 x 40 KB at order 5050), two passes over them are microseconds, and a stage's sums stay inside one workgroup, so
// their order depends on the stage's order alone and no workgroup waits for another.
// Plain loads and stores: no polled words, no waits between workgroups, no atomics.  Loads are 8 bytes wide, a stage's
// first column may be odd.  Included by staged_hess.hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace stg {

static const int HB_REPORT = 8;  // (HQPKKT_BFGS_REPORT)

// The workgroup's sum of a, the same bits in every thread: a wavefront's sum by kktdev::wave_sum, the four wavefronts'
// sums in wavefront order through LDS (red: four doubles, free again at the next call's first barrier).
__device__ __forceinline__ double hb_block_sum(double a, double *red) {
  a = kktdev::wave_sum(a);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Workgroup k: stage k, the entries [col0, col0 + nz) of s, y, Qs and v; thread t takes the entries t, t + 256, .. - what
// lies past nz belongs to the next stage and is never read.
//   pass 1    sy = s'y and sQs = s'Qs, a thread's share by fused multiply-adds in ascending order
//   decision  by thread 0, every operation rounded on its own (hessian_update.bfgs_replay repeats it in numpy; the
//             kernel's body is compiled without contraction and writes these operations with the operators: the
//             toolchain's __dmul_rn / __dadd_rn are the plain operators behind an inline call, a product of one and the
//             sum of the other contract like any others):
//             damp where sy < fl(gamma_eff sQs); theta = fl(fl((1 - gamma_eff) sQs) / fl(sQs - sy)), omt = fl(1 - theta)
//   pass 2    damped: v_i = fl(fl(theta y_i) + fl(omt Qs_i)), no contraction, and sv = s'v in the order of pass 1;
//             otherwise v_i = y_i and sv = sy
//   outcome   sv and sQs finite and nonzero: c0 = 1 / sv, c1 = -1 / sQs (0 updated, 1 updated with damping); otherwise
//             c0 = c1 = 0 and units = 0 - k_hu_update leaves the stage alone - (2: sv or sQs is zero, a stage of order 0
//             included; 3: sv or sQs is not finite).  rep[8 k ..]: sy, sQs, gamma_eff, theta, sv, c0, c1, outcome.
__global__ void __launch_bounds__(256) k_hb_terms(HuDesc *__restrict__ desc, const double *s, const double *y, const double *__restrict__ Qs, double *v,
                                                  double gamma_eff, double *__restrict__ rep) {
#pragma clang fp contract(off)  // (a product and the sum behind it stay two roundings: written with the operators, in this scope)
  __shared__ double red[4], dec[2];
  __shared__ int dec_damp;
  const int k = blockIdx.x;
  const int nz = desc[k].nz;
  const long long col0 = desc[k].col0;
  const double *sk = s + col0, *yk = y + col0, *qk = Qs + col0;
  double *vk = v + col0;
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nz; i += 256) {
    const double si = sk[i];
    a = __fma_rn(si, yk[i], a);
    b = __fma_rn(si, qk[i], b);
  }
  const double sy = hb_block_sum(a, red), sQs = hb_block_sum(b, red);
  if (threadIdx.x == 0) {
    const bool damp = sy < gamma_eff * sQs;  // (false where a scalar is NaN)
    double theta = 1.0, omt = 0.0;
    if (damp) {
      theta = ((1.0 - gamma_eff) * sQs) / (sQs - sy);
      omt = 1.0 - theta;
    }
    dec[0] = theta, dec[1] = omt, dec_damp = damp;
  }
  __syncthreads();
  const bool damp = dec_damp != 0;  // (uniform over the workgroup)
  const double theta = dec[0], omt = dec[1];
  double sv = sy;
  if (damp) {
    double c = 0.0;
    for (int i = threadIdx.x; i < nz; i += 256) {
      const double vi = theta * yk[i] + omt * qk[i];
      vk[i] = vi;
      c = __fma_rn(sk[i], vi, c);
    }
    sv = hb_block_sum(c, red);
  } else {
    for (int i = threadIdx.x; i < nz; i += 256) vk[i] = yk[i];
  }
  if (threadIdx.x != 0) return;
  double c0 = 0.0, c1 = 0.0;
  int outcome;
  if (!isfinite(sv) || !isfinite(sQs))
    outcome = 3;
  else if (sv == 0.0 || sQs == 0.0)
    outcome = 2;
  else {
    outcome = damp ? 1 : 0;
    c0 = 1.0 / sv, c1 = -(1.0 / sQs);
  }
  desc[k].c[0] = c0, desc[k].c[1] = c1;
  if (outcome >= 2) desc[k].units = 0;
  double *r = rep + (long long)HB_REPORT * k;
  r[0] = sy, r[1] = sQs, r[2] = gamma_eff, r[3] = theta, r[4] = sv, r[5] = c0, r[6] = c1, r[7] = (double)outcome;
}

}  // namespace stg
