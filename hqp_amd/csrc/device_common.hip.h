// Device types, constants and wave-level helpers shared by the units of the library (tree.hip,
// staged_engine.hip, ip_loops.hip, q_entries.hip, hqpkkt.hip): declarations and inline functions only, no kernel and no
// device variable, so that every unit may include it.
#pragma once
#include <hip/hip_runtime.h>

namespace kktdev {

typedef double double4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double4_t mfma_f64(double a, double b, double4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

struct DevTree {
  const int *piv_start, *npiv, *nbor, *parent;
  const long long *bptr;
  const int *bidx, *rel;
  const long long *panel_off, *upd_off, *x_off, *cb_off;
  const int *child_ptr, *child_idx;
  const int *pinv;            // per child: parent front index -> child border index (-1: none)
  const long long *pinv_off;
};

// order-preserving max for non-negative doubles through their bit pattern
// (the read-modify-writes of a launch's workgroups on ONE word are served one after the other, ~6 ns each: launches that
// end in this keep their grids at a thousand or two workgroups; a look at the word first - an agent-scope load - cost
// k_assemble_simple more than it saved k_residual)
__device__ __forceinline__ void atomic_max_pos(unsigned long long *addr, double v) {
  atomicMax(addr, (unsigned long long)__double_as_longlong(v));
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// max over the 64 lanes of a non-negative value with DPP row operations (no LDS
// crossbar traffic); the result is broadcast to every lane
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v) {
  const long long b = __double_as_longlong(v);
  int lo = (int)(b & 0xffffffffLL), hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_max_dpp(double v) {
  v = fmax(v, dpp_move<0xb1, 0xf>(v));   // quad_perm [1,0,3,2]
  v = fmax(v, dpp_move<0x4e, 0xf>(v));   // quad_perm [2,3,0,1]
  v = fmax(v, dpp_move<0x124, 0xf>(v));  // row_ror 4
  v = fmax(v, dpp_move<0x128, 0xf>(v));  // row_ror 8
  v = fmax(v, dpp_move<0x142, 0xa>(v));  // row_bcast 15
  v = fmax(v, dpp_move<0x143, 0xc>(v));  // row_bcast 31 -> lane 63 holds the max
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), 63);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// sum over the 64 lanes the same way (lanes a DPP step does not reach contribute zero); broadcast to every lane
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move0(double v) {
  const long long b = __double_as_longlong(v);
  int lo = (int)(b & 0xffffffffLL), hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum_dpp(double v) {
  v += dpp_move0<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_move0<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
  v += dpp_move0<0x124, 0xf>(v);  // row_ror 4
  v += dpp_move0<0x128, 0xf>(v);  // row_ror 8: every lane of a row has the row's sum
  v += dpp_move0<0x142, 0xa>(v);  // row_bcast 15: rows 1 and 3 add the sum of the row before
  v += dpp_move0<0x143, 0xc>(v);  // row_bcast 31: rows 2 and 3 add lane 31 -> lane 63 holds the total
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), 63);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// same for a float (the arg-max search of the pivot column runs in fp32: an fp64
// max costs ~40 cycles of latency per step on gfx950, an fp32 one a few)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL,
                                                    ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_max_dpp_f(float v) {
  v = fmaxf(v, dpp_move_f<0xb1, 0xf>(v));
  v = fmaxf(v, dpp_move_f<0x4e, 0xf>(v));
  v = fmaxf(v, dpp_move_f<0x124, 0xf>(v));
  v = fmaxf(v, dpp_move_f<0x128, 0xf>(v));
  v = fmaxf(v, dpp_move_f<0x142, 0xa>(v));
  v = fmaxf(v, dpp_move_f<0x143, 0xc>(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// 1/d by the hardware estimate and two Newton steps (error ~1 ulp; the pivot is
// bounded away from zero and from overflow by the perturbation test)
__device__ __forceinline__ double fast_rcp(double d) {
  double x = __builtin_amdgcn_rcp(d);
  x = fma(fma(-d, x, 1.0), x, x);
  x = fma(fma(-d, x, 1.0), x, x);
  return x;
}


__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct TermDev {
  int s1, s2, wi;
  double sgn;
};

// the word of the handle's flags buffer that switches the replacement of cancelled pivots on (kernels.hip.h, tiny_replace)
static const int TINY_REPLACE_WORD = 112;
// (the word: 0 off; TINY_REPLACE_ON: cancelled pivots that are not exactly zero; TINY_REPLACE_ZEROS: exactly zero ones as well)
static const int TINY_REPLACE_ON = 0x01010101, TINY_REPLACE_ZEROS = 0x02020202;  // (set by hipMemsetAsync: a byte value)

// the exchange arrays of the polled launches (kernels.hip.h, xw_take)
static const unsigned long long XW_SENTINEL = 0x7ff8dead0badc0deULL;
static const int XW_GAVE_UP = 110;  // index into the handle's flags buffer: a poll gave up (~2^20 tries)

struct CsrDev {
  const int *ptr, *col, *src;
  const double *val;  // the values in CSR order (gathered through src once per update())
};
// sum over the LPR (16 or 4) consecutive lanes that share a CSR row
template <int LPR>
__device__ __forceinline__ double row_sum(double v) {
  v += dpp_move<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
  if (LPR == 16) {
    v += dpp_move<0x124, 0xf>(v);  // row_ror 4
    v += dpp_move<0x128, 0xf>(v);  // row_ror 8 -> every lane of the row holds the sum
  }
  return v;
}
template <int LPR>
__device__ __forceinline__ double row_dot(const CsrDev M, const double *__restrict__ vals,
                                          const double *__restrict__ x, int row, int sub) {
  // (two entries per lane in flight: the loop is a chain of index -> value round trips, 80 - 160 entries per row on
  // the banded systems)
  double s = 0.0, t = 0.0;
  const int e = M.ptr[row + 1];
  int k = M.ptr[row] + sub;
  for (; k + LPR < e; k += 2 * LPR) {
    const int c0 = M.col[k], c1 = M.col[k + LPR];
    const double v0 = M.val[k], v1 = M.val[k + LPR];
    s += v0 * x[c0], t += v1 * x[c1];
  }
  if (k < e) s += M.val[k] * x[M.col[k]];
  return row_sum<LPR>(s + t);
}

// the mapped host words of the read-backs (kernels.hip.h, k_post_words)
#define HPIN_DOUBLES 256
#define HPIN_SEQ 200  // the double of hpin whose first four bytes hold the sequence number
#define HPIN_ZM 208   // two doubles the HOST writes for a kernel to read: zeta and mu of a step of the Franke loop (k_fr_rhs)

struct CopyList {
  const double *src[6];
  double *dst[6];
  int len[6];
};

}  // namespace kktdev
