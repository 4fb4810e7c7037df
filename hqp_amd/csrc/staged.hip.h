// gfx950 kernels of the STAGED engine (HQPKKT_MODE_STAGED): the stage-structured
// solution of the interior-point Newton system for multistage (DOCP) problems, i.e. the
// job of the reference's Hqp_IpLQDOCP (hqp/Hqp_IpLQDOCP.C:796-976; extended Riccati
// recursion ExRiccatiFactorSc :1794-1999, ExRiccatiSolveSc :2007-2182).  Included by
// staged_engine.hip.  The algorithm and its notation: tests/model_staged.py (numpy model).
//
// Layout in HBM: every dense block row-major with an even leading dimension (16-byte
// loads), so that EVERY matrix product of the recursion is of the one form
//     C (M x N) = alpha * sum_k A[k][i] * B[k][j] + beta * Cin        ("TN": both operands k-major; staged_gemm.hip.h)
//   W   = V+ F          A = V+ (symmetric), B = F = [fx fu] (n+ x (n+m))
//   G   = F' W          lower tiles only
//   Nc  = B+ F          A = BT+ (n+ x cap: the carried constraint rows, transposed)
//   Rm  = K^-1 Y        A = K^-1 (symmetric)
//   V   = Gxx - Y' Rm   lower tiles + mirror
// v_mfma_f64_16x16x4 operand layout (hqpkkt_selftest_mfma): A: lane l holds A[l&15][l>>4];
// B: B[l>>4][l&15]; C/D: col = l&15, row = (l>>4) + 4*reg.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "staged_plan.hpp"
#include "staged_gemm.hip.h"

namespace stg {

// ---------------------------------------------------------------------------------------
// H = Q + C'(Z/W)C of one stage added into the dense block (term lists as in the REDUCED
// plugin: value = sum sgn * vals[s1] * vals[s2] * wt[wi]); every entry has one writer
struct HTerm {
  int s1, s2, wi;
};
__global__ void k_st_add_h(int nent, const long long *__restrict__ dst, const int *__restrict__ tptr,
                           const HTerm *__restrict__ terms, const double *__restrict__ vals,
                           const double *__restrict__ wt, double *__restrict__ G, int add) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  double s = 0.0;
  for (int k = tptr[e]; k < tptr[e + 1]; k++) s += vals[terms[k].s1] * vals[terms[k].s2] * wt[terms[k].wi];
  if (add)
    G[dst[e]] += s;
  else
    G[dst[e]] = s;
}

// The state part of H added into V_k where the product's launch has written G_xx - Y'Rm straight into V (lower tiles and
// their mirror image): the entry on or below the diagonal and its image get the identical value, so V stays exactly
// symmetric.  dst: offsets in a block of leading dimension ldg (the plan's list); entries above the diagonal have
// their image in the list and are left to it
__global__ void k_st_add_h_sym(int nent, const long long *__restrict__ dst, const int *__restrict__ tptr,
                               const HTerm *__restrict__ terms, const double *__restrict__ vals,
                               const double *__restrict__ wt, double *__restrict__ V, long long ldg, long long ldv) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  const long long i = dst[e] / ldg, j = dst[e] % ldg;
  if (i < j) return;
  double s = 0.0;
  for (int k = tptr[e]; k < tptr[e + 1]; k++) s += vals[terms[k].s1] * vals[terms[k].s2] * wt[terms[k].wi];
  const double v = V[i * ldv + j] + s;
  V[i * ldv + j] = v;
  if (i != j) V[j * ldv + i] = v;
}

// The same for a system sharded over ranks: a rank computes only ITS tiles of the work block G (the plan's tile list);
// everything else in G is left over from earlier stages.  H is added only into the rank's own tiles (bit
// tr * ntc + tc of `owned`, 128 x 128 tiles): a "+=" on a tile nobody overwrites would grow from stage to stage and
// from factorisation to factorisation.
__global__ void k_st_add_h_owned(int nent, const long long *__restrict__ dst, const int *__restrict__ tptr,
                                 const HTerm *__restrict__ terms, const double *__restrict__ vals,
                                 const double *__restrict__ wt, double *__restrict__ G, long long ld,
                                 const unsigned *__restrict__ owned, int ntc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  const long long d = dst[e];
  const int t = (int)(d / ld >> 7) * ntc + (int)(d % ld >> 7);
  if (!((owned[t >> 5] >> (t & 31)) & 1u)) return;
  double s = 0.0;
  for (int k = tptr[e]; k < tptr[e + 1]; k++) s += vals[terms[k].s1] * vals[terms[k].s2] * wt[terms[k].wi];
  G[d] += s;
}

// values of the A block scattered into dense storage: dst >= 0 offset into the F arena (dynamics
// rows), dst <= -2 offset -(dst + 2) into the misc arena (own equality rows of N), -1 not stored
// (the -1.0 of a dynamics row, the rows that fix x_0)
__global__ void k_st_scatter(long long nent, const long long *__restrict__ dst, const double *__restrict__ vals,
                             double *__restrict__ F, double *__restrict__ misc) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nent) return;
  const long long d = dst[e];
  if (d >= 0)
    F[d] = vals[e];
  else if (d <= -2)
    misc[-(d + 2)] = vals[e];
}
// check of the staircase: the last entry of every dynamics row is -1.0 (Hqp_IpLQDOCP::Get_Dim,
// hqp/Hqp_IpLQDOCP.C:214-215), the entries that fix x_0 are non-zero
__global__ void k_st_check(int nchk, const int *__restrict__ idx, const int *__restrict__ kind,
                           const double *__restrict__ vals, int *__restrict__ status) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nchk) return;
  const double v = vals[idx[e]];
  if (kind[e] == 0 ? v != -1.0 : v == 0.0) atomicExch(status, 6);
}

// ---------------------------------------------------------------------------------------
// block-wide arg-max of |value| with the smallest index winning ties (deterministic)
struct ArgMax {
  double v;
  int i;
};
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ ArgMax block_argmax(ArgMax a, ArgMax *red) {
  // wavefront: the maximum by DPP row operations, then the first lane that holds it (a fixed rule:
  // the thread -> entry map is fixed, so ties always go the same way)
  const double vmax = kktdev::wave_max_dpp(a.v);
  const unsigned long long hit = __ballot(a.v == vmax);
  const int src = hit ? __ffsll((long long)hit) - 1 : 0;
  a.v = vmax;
  a.i = __builtin_amdgcn_readlane(a.i, src);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  ArgMax r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); w++)
    if (red[w].v > r.v) r = red[w];
  return r;
}

// In-place inverse of the q x q matrix a (LDS, leading dimension ld) by Gauss-Jordan
// elimination with complete pivoting.  Returns 0, or 1 when a pivot is exactly zero / NaN.
// ip, ir, ic: int work arrays of q entries; colv, rowv: double work arrays of q entries.
// 256 threads as a 16 x 16 grid: thread (ty, tx) owns the entries (ty + 16 i, tx + 16 j); the
// pivot search of step s+1 rides on the update sweep of step s.
#ifdef HQPKKT_STAMPS
__device__ int g_gj_stamps[32];
#define GSTAMP(slot)                                                                              \
  do {                                                                                            \
    if (threadIdx.x == 0 && s == 10) g_gj_stamps[slot] = (int)__builtin_amdgcn_s_memtime();       \
  } while (0)
#else
#define GSTAMP(slot)
#endif
#ifndef HQPKKT_GJ_RB
#define HQPKKT_GJ_RB 2  // rows per trip of the sweeps whose matrix is in global memory (1024 threads: 128 registers each)
#endif
template <int RB = 1>  // RB rows x 8 columns of loads in flight per thread
__device__ int gj_inverse(double *a, int q, int ld, int *ip, int *ir, int *ic, double *colv, double *rowv,
                          ArgMax *red) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ty = tid >> 4, tx = tid & 15, RS = nt >> 4;  // (ty, tx): rows ty + RS i, columns tx + 16 j
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  const long long ABS = 0x7fffffffffffffffLL, INFB = 0x7ff0000000000000LL;
  for (int j = tid; j < q; j += nt) ip[j] = 0;
  __syncthreads();
  int bad = 0;
  // this thread's largest |entry| among the free rows and columns as its BIT PATTERN: for non-negative doubles the
  // order of the patterns is the order of the values, and a NaN lies above infinity - one integer comparison per
  // entry.  Ties: the first entry in this thread's fixed order, then the first lane, then the first wavefront - the
  // same pivot sequence in every run.
  long long bb = -1;
  int bi = 0x7fffffff;
  for (int r = ty; r < q; r += RS)
    for (int c = tx; c < q; c += 16) {
      const long long bits = __double_as_longlong(a[r * ld + c]) & ABS;
      if (bits > bb) bb = bits, bi = r * q + c;
    }
  for (int s = 0; s < q; s++) {
    GSTAMP(0);
    ArgMax best = block_argmax(ArgMax{bb < 0 ? -1.0 : (bb > INFB ? INF : __longlong_as_double(bb)), bi}, red);
    GSTAMP(1);
    const int irow = best.i / q, icol = best.i - irow * q;
    if (!(best.v > 0.0) || best.v == INF) bad = 1;
    if (irow != icol)
      for (int c = tid; c < q; c += nt) {
        const double x = a[irow * ld + c];
        a[irow * ld + c] = a[icol * ld + c];
        a[icol * ld + c] = x;
      }
    if (tid == 0) ip[icol] = 1, ir[s] = irow, ic[s] = icol;
    __syncthreads();
    GSTAMP(2);
    const double pinv = bad ? 1.0 : 1.0 / a[icol * ld + icol];
    for (int c = tid; c < q; c += nt) {
      colv[c] = (c == icol) ? 0.0 : a[c * ld + icol];
      rowv[c] = (c == icol ? 1.0 : a[icol * ld + c]) * pinv;
    }
    __syncthreads();
    // the pivot column is cleared and the pivot row scaled in place, so that the sweep has no special rows or columns:
    // every entry becomes a - colv[r] rowv[c] (colv is zero in the pivot row)
    for (int c = tid; c < q; c += nt) {
      if (c != icol) a[c * ld + icol] = 0.0;
      a[icol * ld + c] = rowv[c];
    }
    __syncthreads();
    GSTAMP(3);
    bb = -1, bi = 0x7fffffff;
    // RB x 8 entries per trip: what depends on the column alone (pivot row, flags) is read once per trip, the entries'
    // loads are issued together from clamped addresses (no branch between them) - the matrix may live in global memory
    // (stages with hundreds of controls), and in LDS too a wait per entry costs more than the arithmetic
    for (int c0 = tx; c0 < q; c0 += 128) {
      double rv[8];
      int cc[8];
      bool cfree[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int c = c0 + 16 * u;
        cc[u] = c < q ? c : q - 1;
        rv[u] = rowv[cc[u]];
        cfree[u] = c < q && ip[cc[u]] == 0;
      }
      for (int r0 = ty; r0 < q; r0 += RS * RB) {
        double x[RB][8];
#pragma unroll
        for (int k = 0; k < RB; k++) {
          const int r = min(r0 + k * RS, q - 1);
#pragma unroll
          for (int u = 0; u < 8; u++) x[k][u] = a[r * ld + cc[u]];
        }
#pragma unroll
        for (int k = 0; k < RB; k++) {
          const int r = r0 + k * RS, rr = min(r, q - 1);
          const double cr = colv[rr];
          const bool rfree = r < q && ip[rr] == 0;
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int c = c0 + 16 * u;
            const double v = fma(-rv[u], cr, x[k][u]);
            if (r < q && c < q) a[r * ld + c] = v;
            const long long bits = __double_as_longlong(v) & ABS;
            if (rfree && cfree[u] && bits > bb) bb = bits, bi = r * q + c;
          }
        }
      }
    }
    GSTAMP(4);
  }
  __syncthreads();
  for (int s = q - 1; s >= 0; s--) {
    const int r1 = ir[s], c1 = ic[s];
    if (r1 != c1)
      for (int r = tid; r < q; r += nt) {
        const double x = a[r * ld + r1];
        a[r * ld + r1] = a[r * ld + c1];
        a[r * ld + c1] = x;
      }
    __syncthreads();
  }
  return bad;
}

// The same inverse for q <= 16 NB with the matrix in REGISTERS: thread (ty, tx) of the 16 x 16 grid
// holds the entries (ty + 16 i, tx + 16 j) of the augmented matrix [K | I] (NB x 2 NB doubles), so a
// step costs the broadcast of the pivot row and column through LDS and NB x 2 NB multiply-adds; no
// row or column is ever moved: after q steps the left half is a permutation, row r of the right half
// is row pcol(r) of the inverse.  a (LDS, q x q, ld) holds K on entry and the inverse on return.
template <int NB>
__device__ int gj_inverse_reg(double *a, int q, int ld, int *ip, int *pc_of_row, double *colv, double *rowv, ArgMax *red) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  double m[NB][2 * NB];
  int rfree = 0, cfree = 0;  // bit i: own row ty + 16 i / own column tx + 16 i not yet a pivot row / column
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const int r = ty + 16 * i;
    if (r < q) rfree |= 1 << i;
    if (tx + 16 * i < q) cfree |= 1 << i;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int c = tx + 16 * j;
      m[i][j] = (r < q && c < q) ? a[r * ld + c] : 0.0;
      m[i][NB + j] = (r == c && r < q) ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  int bad = 0;
  for (int s = 0; s < q; s++) {
    ArgMax best{-1.0, 0x7fffffff};
#pragma unroll
    for (int i = 0; i < NB; i++)
#pragma unroll
      for (int j = 0; j < NB; j++)
        if ((rfree >> i & 1) && (cfree >> j & 1)) {
          const double v = fabs(m[i][j]);
          best = better(best, ArgMax{v == v ? v : INF, (ty + 16 * i) * q + tx + 16 * j});
        }
    best = block_argmax(best, red);
    const int pr = best.i / q, pc = best.i - pr * q;
    if (!(best.v > 0.0) || best.v == INF) bad = 1;
    // owners publish the pivot row (2 q values) and the pivot column
    if ((pr & 15) == ty) {
      const int i = pr >> 4;
#pragma unroll
      for (int ii = 0; ii < NB; ii++)
        if (ii == i) {
#pragma unroll
          for (int j = 0; j < 2 * NB; j++) rowv[tx + 16 * j] = m[ii][j];
        }
    }
    if ((pc & 15) == tx) {
      const int j = pc >> 4;
#pragma unroll
      for (int jj = 0; jj < NB; jj++)
        if (jj == j) {
#pragma unroll
          for (int i = 0; i < NB; i++) colv[ty + 16 * i] = m[i][jj];
        }
    }
    if (tid == 0) pc_of_row[pr] = pc;
    __syncthreads();
    const double piv = rowv[(pc & 15) + 16 * (pc >> 4)];
    const double pinv = bad ? 1.0 : 1.0 / piv;
    double rv[2 * NB];
#pragma unroll
    for (int j = 0; j < 2 * NB; j++) rv[j] = rowv[tx + 16 * j] * pinv;
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int r = ty + 16 * i;
      const double f = colv[r];
      if (r == pr) {
#pragma unroll
        for (int j = 0; j < 2 * NB; j++) m[i][j] = rv[j];
      } else {
#pragma unroll
        for (int j = 0; j < 2 * NB; j++) m[i][j] -= f * rv[j];
      }
    }
    if ((pr & 15) == ty) rfree &= ~(1 << (pr >> 4));
    if ((pc & 15) == tx) cfree &= ~(1 << (pc >> 4));
    __syncthreads();  // rowv / colv are rewritten in the next step
  }
  // row r of the right half is row pc_of_row[r] of the inverse
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const int r = ty + 16 * i;
    if (r < q) {
      const int dst = pc_of_row[r];
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const int c = tx + 16 * j;
        if (c < q) a[dst * ld + c] = m[i][NB + j];
      }
    }
  }
  __syncthreads();
  (void)ip;
  return bad;
}
// The same for a matrix that is positive definite after its scaling (K = G_uu of a stage without consumed
// constraint rows): pivots in the natural order down the diagonal - no search, two barriers per step instead of
// four.  Elimination without pivoting is backward stable on such a matrix.  Returns 2 without having touched `a`
// when a pivot is not safely positive (G_uu indefinite or nearly singular): the caller then runs the search.
template <int NB>
__device__ int gj_inverse_reg_spd(double *a, int q, int ld, double *colv, double *rowv) {
  // in place (no identity beside the matrix: half the multiply-adds and LDS reads of the form with the search): step s
  // replaces the pivot by 1/p, its row by row/p, its column by -column/p and every other entry by a_ij - a_is a_sj / p
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  double m[NB][NB];
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const int r = ty + 16 * i;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int c = tx + 16 * j;
      m[i][j] = (r < q && c < q) ? a[r * ld + c] : (r == c ? 1.0 : 0.0);
    }
  }
  __syncthreads();
  int bad = 0;
  for (int s = 0; s < q; s++) {
    if ((s & 15) == ty) {
      const int i = s >> 4;
#pragma unroll
      for (int ii = 0; ii < NB; ii++)
        if (ii == i) {
#pragma unroll
          for (int j = 0; j < NB; j++) rowv[tx + 16 * j] = m[ii][j];
        }
    }
    if ((s & 15) == tx) {
      const int j = s >> 4;
#pragma unroll
      for (int jj = 0; jj < NB; jj++)
        if (jj == j) {
#pragma unroll
          for (int i = 0; i < NB; i++) colv[ty + 16 * i] = m[i][jj];
        }
    }
    __syncthreads();
    const double piv = rowv[s];
    if (!(piv > 1e-10)) bad = 2;  // uniform: every thread reads the same value (the matrix is scaled: diagonal <= 1)
    const double pinv = bad ? 1.0 : 1.0 / piv;
    double rv[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) rv[j] = (tx + 16 * j == s ? 1.0 : rowv[tx + 16 * j]) * pinv;
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int r = ty + 16 * i;
      const double f = colv[r];
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const double old = tx + 16 * j == s ? 0.0 : m[i][j];
        m[i][j] = r == s ? rv[j] : fma(-f, rv[j], old);
      }
    }
    __syncthreads();  // rowv / colv are rewritten in the next step
  }
  if (bad) return bad;  // (uniform) `a` still holds the matrix
#pragma unroll
  for (int i = 0; i < NB; i++) {
    const int r = ty + 16 * i;
    if (r < q) {
#pragma unroll
      for (int j = 0; j < NB; j++) {
        const int c = tx + 16 * j;
        if (c < q) a[r * ld + c] = m[i][j];
      }
    }
  }
  __syncthreads();
  return 0;
}
// The inverse of a matrix that is positive definite after its scaling, in place in LDS (order 65 .. 136, sixteen
// wavefronts): pivots down the diagonal, no search - per step one broadcast of the pivot row / column and the sweep.
// Returns 2 at the first pivot that is not safely positive; the matrix is then partly eliminated (the caller builds
// it again and runs the search).
__device__ int gj_inverse_spd(double *a, int q, int ld, double *colv, double *rowv) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ty = tid >> 4, tx = tid & 15, RS = nt >> 4;
  for (int s = 0; s < q; s++) {
    const double piv = a[s * ld + s];
    if (!(piv > 1e-10)) return 2;  // (uniform: every thread reads the same entry)
    const double pinv = 1.0 / piv;
    for (int c = tid; c < q; c += nt) {
      colv[c] = (c == s) ? 0.0 : a[c * ld + s];
      rowv[c] = (c == s ? 1.0 : a[s * ld + c]) * pinv;
    }
    __syncthreads();
    for (int c = tid; c < q; c += nt) {
      if (c != s) a[c * ld + s] = 0.0;
      a[s * ld + c] = rowv[c];
    }
    __syncthreads();
    for (int c0 = tx; c0 < q; c0 += 128) {
      double rv[8];
      int cc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) cc[u] = min(c0 + 16 * u, q - 1), rv[u] = rowv[cc[u]];
      for (int r = ty; r < q; r += RS) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = a[r * ld + cc[u]];
        const double cr = colv[r];
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (c0 + 16 * u < q) a[r * ld + c0 + 16 * u] = fma(-rv[u], cr, x[u]);
      }
    }
    __syncthreads();
  }
  return 0;
}
// dispatch: registers up to order 64 (the register forms are laid out for 256 threads), LDS / global memory above
template <int NT, bool BIG = (NT != 256)>
__device__ int gj_inverse_any(double *a, int q, int ld, int *ip, int *ir, int *ic, double *colv, double *rowv, ArgMax *red,
                              bool spd = false) {
  if constexpr (NT != 256) return gj_inverse<BIG ? HQPKKT_GJ_RB : 1>(a, q, ld, ip, ir, ic, colv, rowv, red);
  if (spd && q <= 64) {
    const int e = q <= 16 ? gj_inverse_reg_spd<1>(a, q, ld, colv, rowv)
                : q <= 32 ? gj_inverse_reg_spd<2>(a, q, ld, colv, rowv) : gj_inverse_reg_spd<4>(a, q, ld, colv, rowv);
    if (e == 0) return 0;
  }
  if (q <= 16) return gj_inverse_reg<1>(a, q, ld, ip, ir, colv, rowv, red);
  if (q <= 32) return gj_inverse_reg<2>(a, q, ld, ip, ir, colv, rowv, red);
  if (q <= 64) return gj_inverse_reg<4>(a, q, ld, ip, ir, colv, rowv, red);
  return gj_inverse(a, q, ld, ip, ir, ic, colv, rowv, red);
}

// LU factors of the q x q matrix a (LDS or global memory, leading dimension ld) in place - unit lower L below the
// diagonal, U on and above it - with complete pivoting; rows and columns are exchanged physically, pr[s] / pc[s]
// record the row / column that came to position s.  Returns 0, or 1 when a pivot is exactly zero / NaN.  The pivot
// search of step s+1 rides on the update sweep of step s (thread grid 16 columns x nt/16 rows, as in gj_inverse).
// Used where the factors are applied by substitution (k_st_x0_free): a solve by factors leaves a residual of
// eps |K| |x| where the product with an explicit inverse leaves cond(K) eps |b|.
template <int RB = 1>
__device__ int lu_complete(double *a, int q, int ld, int *pr, int *pc, double *colv, double *rowv, ArgMax *red) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ty = tid >> 4, tx = tid & 15, RS = nt >> 4;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  int bad = 0;
  ArgMax best{-1.0, 0x7fffffff};
  for (int r = ty; r < q; r += RS)
    for (int c = tx; c < q; c += 16) {
      const double v = fabs(a[r * ld + c]);
      best = better(best, ArgMax{v == v ? v : INF, r * q + c});
    }
  for (int s = 0; s < q; s++) {
    best = block_argmax(best, red);
    const int irow = best.i / q, icol = best.i - irow * q;
    if (!(best.v > 0.0) || best.v == INF) {
      bad = 1;
      break;
    }
    if (irow != s)
      for (int c = tid; c < q; c += nt) {
        const double x = a[irow * ld + c];
        a[irow * ld + c] = a[s * ld + c];
        a[s * ld + c] = x;
      }
    __syncthreads();
    if (icol != s)
      for (int r = tid; r < q; r += nt) {
        const double x = a[r * ld + icol];
        a[r * ld + icol] = a[r * ld + s];
        a[r * ld + s] = x;
      }
    if (tid == 0) pr[s] = irow, pc[s] = icol;
    __syncthreads();
    const double pinv = 1.0 / a[s * ld + s];
    for (int c = s + 1 + tid; c < q; c += nt) {
      colv[c] = a[c * ld + s] * pinv;
      rowv[c] = a[s * ld + c];
    }
    __syncthreads();
    best = ArgMax{-1.0, 0x7fffffff};
    for (int c0 = s + 1 + tx; c0 < q; c0 += 128) {  // (as in gj_inverse: column data once per trip, RB x 8 loads in flight)
      double rv[8];
      int cc[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        cc[u] = min(c0 + 16 * u, q - 1);
        rv[u] = rowv[cc[u]];
      }
      for (int r0 = s + 1 + ty; r0 < q; r0 += RS * RB) {
        double x[RB][8];
#pragma unroll
        for (int k = 0; k < RB; k++) {
          const int r = min(r0 + k * RS, q - 1);
#pragma unroll
          for (int u = 0; u < 8; u++) x[k][u] = a[r * ld + cc[u]];
        }
#pragma unroll
        for (int k = 0; k < RB; k++) {
          const int r = r0 + k * RS;
          const double cr = colv[min(r, q - 1)];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int c = c0 + 16 * u;
            const double v = x[k][u] - cr * rv[u];
            if (r < q && c < q) {
              a[r * ld + c] = v;
              const double av = fabs(v);
              best = better(best, ArgMax{av == av ? av : INF, r * q + c});
            }
          }
        }
      }
    }
    for (int r = s + 1 + tid; r < q; r += nt) a[r * ld + s] = colv[r];  // the multipliers
  }
  __syncthreads();
  return bad;
}

// Per stage, one workgroup: (A) rank-revealing elimination of the control part N_u of the
// stage's constraint rows (own equalities, then the rows carried back from stage k+1) with
// complete pivoting: consumed rows R (they determine controls), leftover rows L (free of u
// after subtracting t times the consumed rows: carried on to stage k-1) - the job of GE_QP
// in the reference (meschach/addon_hqp.c:399-475, QR with column pivoting there);
// (B) K = [G_uu N_uR'; N_uR 0], symmetric scaling, explicit inverse (the reference factors
// Z' G_uu Z by Bunch-Kaufman and forms Z (Z'G_uu Z)^-1 Z' explicitly, :1907-1924).
struct SmallArgs {
  const double *G;
  long long ldg;
  int n, m;             // states, controls of the stage
  const double *N;
  long long ldn;        // constraint rows, capn x (n + m)
  int e;                // own rows
  const int *cnt_next;  // carried rows coming in (device), nullptr: none
  int capn, cap, qmax;
  double ge_tol;
  double *Kinv;
  long long ldq;        // qmax x qmax, zero padded
  double *Kmat;         // K itself (same shape): the products with K^-1 are refined against it
  double *t;
  long long ldt;        // cap x ldt : t[li][s]
  int *dyn;             // [0] r, [1] number of leftover rows, [2..2+capn) R, [2+capn..2+2capn) L
  int *status;          // set to 4 (E_SING) on a singular K
  double *scratch;      // null: the matrices of (A) and (B) live in LDS; else in this global area (stages with hundreds of
                        // controls / carried rows: StagedPlan::big) and LDS holds the flags and vectors only
  int mode;             // (LDS form: 100 = test hook, see k_st_small)  global-memory form:  0: everything; 1: (A) and the scaled K, no inverse (the blocked
                        // elimination k_blk_* follows); 2: the inverse by this kernel only if the blocked one gave up
};
// layout of SmallArgs::scratch in the global-memory form (qmax = SmallArgs::qmax, ldk = up8(qmax)):
// scaled K | its scaling | panel T0 (64 x ldk) | panel R (64 x ldk) | block P (64 x 64) | flags (ints)
struct BigScratch {
  double *Ks, *dsc, *T0, *R, *Pb;
  int *flags;
  long long ldk;
};
__host__ __device__ inline BigScratch big_scratch(double *base, int qmax) {
  BigScratch b;
  b.ldk = (qmax + 7) / 8 * 8;
  b.Ks = base, b.dsc = b.Ks + (long long)qmax * b.ldk, b.T0 = b.dsc + b.ldk, b.R = b.T0 + 64 * b.ldk, b.Pb = b.R + 64 * b.ldk;
  b.flags = (int *)(b.Pb + 64 * 64);
  return b;
}
#ifdef HQPKKT_STAMPS
#define SSTAMP(slot)                                                                          \
  do {                                                                                        \
    if (threadIdx.x == 0) a.status[9 + (slot)] = (int)__builtin_amdgcn_s_memtime();           \
  } while (0)
#else
#define SSTAMP(slot)
#endif
// <256, false>: K of order <= 64, register-resident inverse; <1024, false>: up to what LDS holds (order ~136), sixteen
// wavefronts on the sweeps (measured: the sweep of the LDS inverse is bound by instruction issue, not by LDS);
// <1024, true>: matrices in global memory.
template <int NT, bool BIG = (NT != 256)>
__global__ void __launch_bounds__(NT, NT / 256) k_st_small(SmallArgs a) {  // (one workgroup: no occupancy to protect, all registers)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ ArgMax red[16];
  __shared__ int s_r, s_stop;
  const int tid = threadIdx.x, nt = blockDim.x;
  // BIG: the matrices of (A) and (B) in a.scratch (global memory) instead of LDS
  SSTAMP(0);
  const int m = a.m, n = a.n;
  const int c = a.e + (a.cnt_next ? *a.cnt_next : 0);
  int *Rl = a.dyn + 2, *Ll = a.dyn + 2 + a.capn;
  // ---------------- (A)
  int r = 0;
  if (BIG && a.mode == 2) {
    // (second call for this stage: the ranks stand in dyn, and the area of (A) now holds K's scaling and the flags)
    if (tid == 0) atomicAdd(a.status + 6, 1);
    if (big_scratch(a.scratch, a.qmax).flags[0] == 0) return;  // (uniform)
    if (tid == 0) atomicAdd(a.status + 7, 1);
    r = a.dyn[0];
  } else if (c > 0 && m > 0) {
    const int ld = m + c;
    // (the kind of memory is fixed by the instantiation, so that the accesses are LDS / global instructions and not
    // flat ones: with a pointer chosen at run time every load also waits for the stores in front of it)
    double *aug;
    int *rfree;
    if constexpr (BIG)
      aug = a.scratch, rfree = (int *)sm;
    else
      aug = sm, rfree = (int *)(sm + (size_t)c * ld);
    int *cfree = rfree + c;
    for (int e = tid; e < c * ld; e += nt) {
      const int i = e / ld, j = e - i * ld;
      aug[e] = j < m ? a.N[(long long)i * a.ldn + n + j] : (j - m == i ? 1.0 : 0.0);
    }
    for (int i = tid; i < c; i += nt) rfree[i] = 1;
    for (int j = tid; j < m; j += nt) cfree[j] = 1;
    if (tid == 0) s_r = 0, s_stop = 0;
    __syncthreads();
    const int steps = c < m ? c : m;
    for (int s = 0; s < steps; s++) {
      ArgMax best{-1.0, 0x7fffffff};
      for (int e = tid; e < c * m; e += nt) {
        const int i = e / m, j = e - i * m;
        if (rfree[i] && cfree[j]) {
          const double v = fabs(aug[i * ld + j]);
          best = better(best, ArgMax{v, e});
        }
      }
      best = block_argmax(best, red);
      if (!(best.v > a.ge_tol)) break;  // uniform
      const int pi = best.i / m, pj = best.i - pi * m;
      __syncthreads();
      if (tid == 0) rfree[pi] = 0, cfree[pj] = 0, Rl[s] = pi, s_r = s + 1;
      const double piv = aug[pi * ld + pj];
      // multipliers of the free rows (column pj), then the update
      double *fac = (double *)(cfree + m + ((c + m) & 1));  // c doubles behind the flags, 8-byte aligned
      __syncthreads();
      for (int i = tid; i < c; i += nt) fac[i] = (rfree[i]) ? aug[i * ld + pj] / piv : 0.0;
      __syncthreads();
      {  // (thread grid 16 columns x nt/16 rows; the pivot row's entries once per trip, eight loads in flight)
        const int ty = tid >> 4, tx = tid & 15, RS = nt >> 4;
        for (int j0 = tx; j0 < ld; j0 += 128) {
          double pv[8];
          int jj[8];
#pragma unroll
          for (int u = 0; u < 8; u++) jj[u] = min(j0 + 16 * u, ld - 1), pv[u] = aug[pi * ld + jj[u]];
          for (int i = ty; i < c; i += RS) {
            const double f = fac[i];  // (zero for the rows that are not free)
            if (f != 0.0) {
              double x[8];
#pragma unroll
              for (int u = 0; u < 8; u++) x[u] = aug[i * ld + jj[u]];
#pragma unroll
              for (int u = 0; u < 8; u++) {
                const int j = j0 + 16 * u;
                if (j < ld) aug[i * ld + j] = (j == pj) ? 0.0 : x[u] - f * pv[u];
              }
            }
          }
        }
      }
      __syncthreads();
    }
    __syncthreads();
    r = s_r;
    // leftover rows in increasing order, t = -coef[L, R]
    if (tid == 0) {
      int nl = 0;
      for (int i = 0; i < c; i++)
        if (rfree[i]) Ll[nl++] = i;
      if (nl > a.cap) nl = a.cap, atomicExch(a.status, 1);  // more rows to carry than the plan holds
      a.dyn[0] = r, a.dyn[1] = nl;
    }
    __syncthreads();
    const int nl = min(c - r, a.cap);
    for (int e = tid; e < nl * r; e += nt) {
      const int li = e / r, s = e - li * r;
      a.t[(long long)li * a.ldt + s] = -aug[Ll[li] * ld + m + Rl[s]];
    }
    __syncthreads();
  } else {
    if (tid == 0) {
      int nl = c;
      if (nl > a.cap) nl = a.cap, atomicExch(a.status, 1);
      a.dyn[0] = 0, a.dyn[1] = nl;
      for (int i = 0; i < nl; i++) Ll[i] = i;
    }
    __syncthreads();
  }
  // ---------------- (B)
  SSTAMP(1);
  const int q = m + r;
  if (q > 0) {
    int ld = q | 1;
    double *Km, *dsc, *colv;
    if constexpr (BIG) {
      const BigScratch bs = big_scratch(a.scratch, a.qmax);
      Km = bs.Ks, dsc = bs.dsc, ld = (int)bs.ldk, colv = sm;
    } else
      Km = sm, dsc = sm + (size_t)q * ld, colv = dsc + q;
    double *rowv = colv + (q > 64 ? q : 64);
    int *ip = (int *)(rowv + (q > 128 ? q : 128)), *ir = ip + q, *ic = ir + q;
    if (BIG && a.mode == 2) {
      // the blocked elimination gave up (a diagonal block without a safe pivot, or its result failed the check
      // against K): K is scaled again from its copy and inverted here, with the search over the whole matrix
      const BigScratch bs = big_scratch(a.scratch, a.qmax);
      if (bs.flags[0] == 0) return;  // (uniform)
      for (int e = tid; e < q * q; e += nt) {
        const int i = e / q, j = e - i * q;
        Km[i * ld + j] = a.Kmat[(long long)i * a.ldq + j] * dsc[i] * dsc[j];
      }
      __syncthreads();
    } else {
    for (int e = tid; e < q * q; e += nt) {
      const int i = e / q, j = e - i * q;
      double v;
      if (i < m && j < m) {
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        v = a.G[(long long)(n + hi) * a.ldg + n + lo];
      } else if (i >= m && j >= m)
        v = 0.0;
      else {
        const int s = (i >= m ? i : j) - m, u = i >= m ? j : i;
        v = a.N[(long long)Rl[s] * a.ldn + n + u];
      }
      Km[i * ld + j] = v;
    }
    __syncthreads();
    SSTAMP(2);
    for (int e = tid; e < a.qmax * a.qmax; e += nt) {
      const int i = e / a.qmax, j = e - i * a.qmax;
      a.Kmat[(long long)i * a.ldq + j] = (i < q && j < q) ? Km[i * ld + j] : 0.0;
    }
    SSTAMP(3);
    // scaling: u rows 1/sqrt(K_ii) where K_ii > 1 (hqp/Hqp_IpLQDOCP.C:1851-1858), constraint rows
    // by their largest entry
    for (int i = tid; i < q; i += nt) {
      double d = 1.0;
      if (i < m) {
        const double kii = Km[i * ld + i];
        if (kii > 1.0) d = 1.0 / sqrt(kii);
      } else {
        double mx = 0.0;
        for (int j = 0; j < m; j++) mx = fmax(mx, fabs(Km[i * ld + j]));
        if (mx > 0.0) d = 1.0 / mx;
      }
      dsc[i] = d;
    }
    __syncthreads();
    for (int e = tid; e < q * q; e += nt) {
      const int i = e / q, j = e - i * q;
      Km[i * ld + j] *= dsc[i] * dsc[j];
    }
    __syncthreads();
    if (BIG && a.mode == 1) {
      // identity padding up to qmax (the ranks are decided here, the launches behind this one were sized by the host)
      const BigScratch bs = big_scratch(a.scratch, a.qmax);
      for (int e = tid; e < a.qmax * a.qmax; e += nt) {
        const int i = e / a.qmax, j = e - i * a.qmax;
        if (i >= q || j >= q) Km[i * ld + j] = i == j ? 1.0 : 0.0;
      }
      for (int i = q + tid; i < a.qmax; i += nt) dsc[i] = 0.0;
      if (tid == 0) bs.flags[0] = 0;
      return;
    }
    }
    SSTAMP(4);
    int bad = -1;
    if constexpr (NT == 1024 && !BIG) {
      if (r == 0) {  // no consumed constraint rows: K = G_uu, positive definite unless the problem is not convex in u
        bad = gj_inverse_spd(Km, q, ld, colv, rowv);
        if (a.mode == 100) bad = 2;  // (test hook, HQPKKT_SPD_TEST_FAIL: the way back from a pivot that was refused)
        if (bad) {  // (uniform) scaled again from the copy, then with the search
          __syncthreads();
          for (int e = tid; e < q * q; e += nt) {
            const int i = e / q, j = e - i * q;
            Km[i * ld + j] = a.Kmat[(long long)i * a.ldq + j] * dsc[i] * dsc[j];
          }
          __syncthreads();
          bad = -1;
        }
      }
    }
    if (bad < 0) bad = gj_inverse_any<NT, BIG>(Km, q, ld, ip, ir, ic, colv, rowv, red, r == 0);
    if (bad && tid == 0) atomicExch(a.status, 4);
    __syncthreads();
    SSTAMP(5);
    for (int e = tid; e < a.qmax * a.qmax; e += nt) {
      const int i = e / a.qmax, j = e - i * a.qmax;
      double v = 0.0;
      if (i < q && j < q) v = 0.5 * (Km[i * ld + j] + Km[j * ld + i]) * dsc[i] * dsc[j];
      a.Kinv[(long long)i * a.ldq + j] = v;
    }
    SSTAMP(6);
  } else {
    if (BIG && a.mode == 2) return;
    for (int e = tid; e < a.qmax * a.qmax; e += nt)
      a.Kinv[(long long)(e / a.qmax) * a.ldq + e % a.qmax] = 0.0, a.Kmat[(long long)(e / a.qmax) * a.ldq + e % a.qmax] = 0.0;
    if constexpr (BIG) {
      if (a.mode == 1) {
        const BigScratch bs = big_scratch(a.scratch, a.qmax);
        for (int e = tid; e < a.qmax * a.qmax; e += nt) bs.Ks[(long long)(e / a.qmax) * bs.ldk + e % a.qmax] = e / a.qmax == e % a.qmax ? 1.0 : 0.0;
        for (int i = tid; i < a.qmax; i += nt) bs.dsc[i] = 0.0;
        if (tid == 0) bs.flags[0] = 0;
      }
    }
  }
}

// ---- Blocked elimination of a stage's K where it does not fit the LDS of one CU (order up to 768): the symmetric
// sweep operator with pivot BLOCKS of 64 down the diagonal - per block one workgroup inverts the 64 x 64 diagonal block
// (complete pivoting inside it, registers), two small products on the whole chip form the block row P K_j: and the
// update K - K_:j P K_j:, one kernel puts the block row, its mirror image and -P in place.  After the last block the
// area holds -K^-1.  No pivoting ACROSS blocks: that is safe where the control Hessian of the stage is positive definite
// and the consumed constraint rows come behind it (the quasidefinite order); a diagonal block without a safe pivot, or a
// result that fails the check K K^-1 = I, raises flags[0] and the one-workgroup elimination with the search over the
// whole matrix runs instead (k_st_small mode 2).  200 controls: 3 ms -> ~0.5 ms per stage, 512: 34 -> ~1 ms.
struct BlkArgs {
  double *scratch;
  int qmax, j;
};
__global__ void __launch_bounds__(256) k_blk_pivot(BlkArgs a) {
  __shared__ double A[64 * 65], colv[64], rowv[128];
  __shared__ int ip[64], pcr[64];
  __shared__ ArgMax red[16];
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0]) return;  // (uniform) an earlier block gave up
  const int tid = threadIdx.x, j0 = a.j * 64, b = min(64, a.qmax - j0);
  ArgMax am{0.0, 0};
  for (int e = tid; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;
    const double v = (r < b && c < b) ? bs.Ks[(long long)(j0 + r) * bs.ldk + j0 + c] : 0.0;
    A[r * 65 + c] = v;
    const double av = fabs(v);
    if (!(av <= am.v)) am.v = av == av ? av : __longlong_as_double(0x7ff0000000000000LL);
  }
  for (int e = tid; e < 64 * a.qmax; e += 256) {
    const int r = e / a.qmax, c = e - r * a.qmax;
    bs.T0[(long long)r * bs.ldk + c] = r < b ? bs.Ks[(long long)(j0 + r) * bs.ldk + c] : 0.0;
  }
  am = block_argmax(am, red);
  __syncthreads();
  // (a positive definite block - the control Hessian's blocks and their Schur complements - down its diagonal first;
  // the register form leaves A untouched when it refuses a pivot, the search takes over)
  int bad = gj_inverse_reg_spd<4>(A, b, 65, colv, rowv);
  if (bad) bad = gj_inverse_reg<4>(A, b, 65, ip, pcr, colv, rowv, red);
  ArgMax pm{0.0, 0};
  for (int e = tid; e < 64 * 64; e += 256) {
    const int r = e >> 6, c = e & 63;
    const double v = (r < b && c < b) ? 0.5 * (A[r * 65 + c] + A[c * 65 + r]) : 0.0;
    bs.Pb[e] = v;
    const double av = fabs(v);
    if (!(av <= pm.v)) pm.v = av == av ? av : __longlong_as_double(0x7ff0000000000000LL);
  }
  pm = block_argmax(pm, red);
  // |K_jj| |K_jj^-1| beyond 1e12: no safe pivot inside this block
  if (tid == 0 && (bad || !(am.v * pm.v < 1e12))) {
    bs.flags[0] = 1;
    // (introspection: the block that gave up, and |K_jj|, |K_jj^-1| as floats)
    bs.flags[1] = a.j + 1, bs.flags[2] = __float_as_int((float)am.v), bs.flags[3] = __float_as_int((float)pm.v);
  }
}
__global__ void k_blk_fixup(BlkArgs a) {
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0]) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 64 * a.qmax) return;
  const int r = e / a.qmax, c = e - r * a.qmax, j0 = a.j * 64, b = min(64, a.qmax - j0);
  if (r >= b) return;
  if (c >= j0 && c < j0 + b) {
    bs.Ks[(long long)(j0 + r) * bs.ldk + c] = -bs.Pb[r * 64 + c - j0];
  } else {
    const double v = bs.R[(long long)r * bs.ldk + c];
    bs.Ks[(long long)(j0 + r) * bs.ldk + c] = v;
    bs.Ks[(long long)c * bs.ldk + j0 + r] = v;
  }
}
// Kinv = -(swept area), unscaled, symmetrised, zero beyond the live order q = m + r
__global__ void k_blk_final(SmallArgs a) {
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0]) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.qmax * a.qmax) return;
  const int i = e / a.qmax, l = e - i * a.qmax, q = a.m + a.dyn[0];
  double v = 0.0;
  if (i < q && l < q) v = -0.5 * (bs.Ks[(long long)i * bs.ldk + l] + bs.Ks[(long long)l * bs.ldk + i]) * bs.dsc[i] * bs.dsc[l];
  a.Kinv[(long long)i * a.ldq + l] = v;
}
// E = K Kinv (in the area of the swept matrix) against the identity of order q
__global__ void __launch_bounds__(1024) k_blk_check(SmallArgs a, double tol) {
  __shared__ ArgMax red[16];
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0]) return;
  const int q = a.m + a.dyn[0];
  ArgMax am{0.0, 0};
  for (int e = threadIdx.x; e < a.qmax * a.qmax; e += blockDim.x) {
    const int i = e / a.qmax, l = e - i * a.qmax;
    const double d = fabs(bs.Ks[(long long)i * bs.ldk + l] - ((i == l && i < q) ? 1.0 : 0.0));
    if (!(d <= am.v)) am.v = d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
  }
  am = block_argmax(am, red);
  if (threadIdx.x == 0 && !(am.v <= tol)) bs.flags[0] = 1;
}

static size_t st_small_lds(int m, int capn, bool big = false) {
  const size_t q = (size_t)m + (size_t)(capn < m ? capn : m);
  // big: the matrices are in global memory, LDS holds flags, multipliers, scalings, pivot row / column, index arrays
  const size_t a = (big ? 0 : (size_t)capn * (m + capn) * 8) + (size_t)(capn + m + 2) * 4 + (size_t)capn * 8 + 16;
  const size_t b = big ? (size_t)kktdev::gj_lds_bytes((long long)q) - q * (q | 1) * 8 : (size_t)kktdev::gj_lds_bytes((long long)q);
  return (a > b ? a : b) + 64;
}

// Per stage, one thread per state column j: Y = [G_ux ; N_xR ; 0] and the transposed carried
// rows BT[j][li] = (N_L - t N_R)[li][j] (zero beyond the live count)
struct WideArgs {
  const double *G;
  long long ldg;
  int n, m;
  const double *N;
  long long ldn;
  int capn, cap, qmax;
  const double *t;
  long long ldt;
  const int *dyn;
  double *Y;
  long long ldy;
  double *BT;
  long long ldb;
};
__global__ void k_st_wide(WideArgs a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const int r = a.dyn[0], nl = a.dyn[1];
  const int *Rl = a.dyn + 2, *Ll = a.dyn + 2 + a.capn;
  for (int i = 0; i < a.m; i++) a.Y[(long long)i * a.ldy + j] = a.G[(long long)(a.n + i) * a.ldg + j];
  for (int s = 0; s < a.qmax - a.m; s++)
    a.Y[(long long)(a.m + s) * a.ldy + j] = s < r ? a.N[(long long)Rl[s] * a.ldn + j] : 0.0;
  for (int li = 0; li < a.cap; li++) {
    double v = 0.0;
    if (li < nl) {
      v = a.N[(long long)Ll[li] * a.ldn + j];
      for (int s = 0; s < r; s++) v -= a.t[(long long)li * a.ldt + s] * a.N[(long long)Rl[s] * a.ldn + j];
    }
    a.BT[(long long)j * a.ldb + li] = v;
  }
}
// Rm = K^-1 Y with one round of refinement against K (Rm += K^-1 (Y - K Rm), see staged_run_factor) for stages whose K
// has order <= 64, in ONE launch instead of three products with a 50-deep k loop: a workgroup takes 32 columns of Y;
// K^-1 and K (symmetric, so a row is read as a column: broadcast reads) and the three q x 32 panels live in LDS;
// thread (row group g of 8, column c) computes the rows g, g + 8, ... of its column.
struct RmArgs {
  const double *Kinv, *Kmat;
  long long ldq;
  double *Y;
  double *Rm;
  long long ldy;
  int q, n;
  int wide;  // 1: Y and the carried rows B_k are formed here too, from w (k_st_wide's work: one launch less)
  WideArgs w;
  double *nRm;  // not null: -Rm as well (leading dimension ldy): the second B operand of the launch that forms V_k
};
static const int RM_COLS = 32;
// K^-1 and K zero-padded to a multiple of 16 (rows of QP + 1 doubles), three QP x 32 panels
static inline size_t st_rm_lds(int q) {
  const size_t QP = ((size_t)q + 15) & ~(size_t)15;
  return sizeof(double) * (2 * QP * (QP + 1) + 3 * QP * RM_COLS);
}
#ifdef HQPKKT_STAMPS
#define RSTAMP(slot)                                                                                     \
  do {                                                                                                   \
    if (threadIdx.x == 0 && blockIdx.x == 0) g_gj_stamps[16 + (slot)] = (int)__builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define RSTAMP(slot)
#endif
// The three products are (q x q)' (q x 32) each: on the matrix pipe (v_mfma_f64_16x16x4: wavefront w takes the rows
// 16 w .. 16 w + 15 of the result, both halves of the 32 columns) - as scalar sums out of LDS they had been bound by the
// LDS issue rate (nine reads per eight multiply-adds; 14 us of a 22-us kernel at q = 50, tools/stamps_stsmall.py).
__global__ void __launch_bounds__(256) k_st_rm(RmArgs a) {
  typedef double d4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) double sm[];
  RSTAMP(0);
  const int q = a.q, QP = (q + 15) & ~15, LDK = QP + 1, tid = threadIdx.x, c = tid & (RM_COLS - 1), g = tid / RM_COLS;
  double *Ki = sm, *Km = Ki + (size_t)QP * LDK, *Ys = Km + (size_t)QP * LDK, *Rs = Ys + (size_t)QP * RM_COLS, *Es = Rs + (size_t)QP * RM_COLS;
  const int j = blockIdx.x * RM_COLS + c;
  {  // (lane = column, the wavefronts take the rows in turn; the loads of a thread in flight together)
    const int l = tid & 63;
    double vi[16], vm[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = (tid >> 6) + 4 * u;
      const bool in = i < q && l < q;
      vi[u] = in ? a.Kinv[(long long)i * a.ldq + l] : 0.0;
      vm[u] = in ? a.Kmat[(long long)i * a.ldq + l] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int i = (tid >> 6) + 4 * u;
      if (i < QP && l < QP) Ki[i * LDK + l] = vi[u], Km[i * LDK + l] = vm[u];
    }
  }
  RSTAMP(1);
  if (a.wide) {
    const WideArgs &w = a.w;
    const int r = w.dyn[0], nl = w.dyn[1];
    const int *Rl = w.dyn + 2, *Ll = w.dyn + 2 + w.capn;
    double yv[8];  // (all loads before the first store: Y may alias G and N as far as the compiler knows)
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = g + 8 * u;
      yv[u] = 0.0;
      if (j < a.n && i < q) {
        if (i < w.m)
          yv[u] = w.G[(long long)(w.n + i) * w.ldg + j];
        else if (i - w.m < r)
          yv[u] = w.N[(long long)Rl[i - w.m] * w.ldn + j];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = g + 8 * u;
      if (j < a.n && i < q) a.Y[(long long)i * a.ldy + j] = yv[u];
      if (i < QP) Ys[i * RM_COLS + c] = yv[u];
    }
    if (j < a.n)
      for (int li = g; li < w.cap; li += 8) {
        double v = 0.0;
        if (li < nl) {
          v = w.N[(long long)Ll[li] * w.ldn + j];
          for (int s = 0; s < r; s++) v -= w.t[(long long)li * w.ldt + s] * w.N[(long long)Rl[s] * w.ldn + j];
        }
        w.BT[(long long)j * w.ldb + li] = v;
      }
  } else
    for (int i = g; i < QP; i += 8) Ys[i * RM_COLS + c] = (j < a.n && i < q) ? a.Y[(long long)i * a.ldy + j] : 0.0;
  __syncthreads();
  RSTAMP(2);
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4, m0 = 16 * wave;
  const int kend = (q + 3) & ~3;
  // out = init + sign * Kx' X for this wavefront's 16 rows (operand layout of the instruction: A[m = lr][k = lk],
  // B[k = lk][n = lr], result rows lk + 4 rg)
  auto product = [&](const double *Kx, const double *X, double sign, const double *init, double *out, bool global) {
    if (m0 >= QP) return;  // (wave-uniform)
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    if (init) {
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        acc0[rg] = init[(m0 + lk + 4 * rg) * RM_COLS + lr];
        acc1[rg] = init[(m0 + lk + 4 * rg) * RM_COLS + 16 + lr];
      }
    }
    double av[16], b0[16], b1[16];  // all fragments of the k loop first (QP <= 64: 16 steps at most), then the chain
#pragma unroll
    for (int st = 0; st < 16; st++)
      if (4 * st < kend) {  // (wave-uniform)
        av[st] = Kx[(4 * st + lk) * LDK + m0 + lr];
        b0[st] = sign * X[(4 * st + lk) * RM_COLS + lr], b1[st] = sign * X[(4 * st + lk) * RM_COLS + 16 + lr];
      }
#pragma unroll
    for (int st = 0; st < 16; st++)
      if (4 * st < kend) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b0[st], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b1[st], acc1, 0, 0, 0);
      }
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
      const int m = m0 + lk + 4 * rg;
      if (global) {
        const int jj = blockIdx.x * RM_COLS + lr;
        if (m < q && jj < a.n) out[(long long)m * a.ldy + jj] = acc0[rg];
        if (m < q && jj + 16 < a.n) out[(long long)m * a.ldy + jj + 16] = acc1[rg];
        if (a.nRm && m < q && jj < a.n) a.nRm[(long long)m * a.ldy + jj] = -acc0[rg];
        if (a.nRm && m < q && jj + 16 < a.n) a.nRm[(long long)m * a.ldy + jj + 16] = -acc1[rg];
      } else {
        out[m * RM_COLS + lr] = acc0[rg];
        out[m * RM_COLS + 16 + lr] = acc1[rg];
      }
    }
  };
  product(Ki, Ys, 1.0, nullptr, Rs, false);  // Rs = K^-1 Y
  __syncthreads();
  product(Km, Rs, -1.0, Ys, Es, false);  // Es = Y - K Rs
  __syncthreads();
  product(Ki, Es, 1.0, Rs, a.Rm, true);  // Rm = Rs + K^-1 Es
  RSTAMP(3);
}

// last stage K: all its equality rows are carried (no control): BT_K = E_K', count = e
__global__ void k_st_last(int n, int e, int cap, const double *__restrict__ N, long long ldn, double *__restrict__ BT,
                          long long ldb, int *__restrict__ dyn) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) dyn[0] = 0, dyn[1] = e;
  if (j >= n) return;
  for (int li = 0; li < cap; li++) BT[(long long)j * ldb + li] = li < e ? N[(long long)li * ldn + j] : 0.0;
}
// a fixed initial state must not be left with constraints of its own (the reference cannot
// solve that either, hqp/Hqp_IpLQDOCP.C:2097-2108)
__global__ void k_st_check_fixed(const int *__restrict__ dyn0, int *__restrict__ status) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && dyn0[1] > 0) atomicExch(status, 4);
}

constexpr int X0_BLOCKED = 40, X0_FELL_BACK = 41;  // counters in the status words: blocked inverse of K0 ran / gave up
// free initial state: LU factors (complete pivoting) of the diagonally scaled [V_0 B_0'; B_0 0]; the reference
// factorises the same scaled matrix by Bunch-Kaufman-Parlett (hqp/Hqp_IpLQDOCP.C:1972-1996) and solves by
// substitution.  K0lu: the factors; K0s: 3 q doubles - the scaling, the row and the column exchanges.
template <int NT>
__global__ void __launch_bounds__(NT, NT / 256) k_st_init_factor(int n0, int cap, const double *__restrict__ V, long long ldv,
                                                       const double *__restrict__ BT, long long ldb,
                                                       const int *__restrict__ dyn0, double *__restrict__ K0lu,
                                                       double *__restrict__ K0mat, double *__restrict__ K0s, long long ldq, int qmax,
                                                       int *__restrict__ status, double *scratch, const int *only_if) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ ArgMax red[16];
  const int tid = threadIdx.x, nt = blockDim.x;
  // (only_if: the flag of the blocked inverse, k_x0_*; zero = its result stands, nothing to do here)
  if (only_if) {
    if (*only_if == 0) return;  // (uniform)
    if (tid == 0) atomicAdd(status + X0_FELL_BACK, 1);
  }
  const int c = dyn0[1], q = n0 + c, ld = q | 1;
  constexpr bool BIG = NT != 256;  // (the kind of memory fixed by the instantiation: see k_st_small)
  double *Km, *dsc;
  if constexpr (BIG)
    Km = scratch, dsc = sm;
  else
    Km = sm, dsc = sm + (size_t)q * ld;
  double *colv = dsc + q, *rowv = colv + (q > 64 ? q : 64);
  int *pr = (int *)(rowv + (q > 128 ? q : 128)), *pc = pr + q;
  for (int e = tid; e < q * q; e += nt) {
    const int i = e / q, j = e - i * q;
    double v;
    if (i < n0 && j < n0)
      v = V[(long long)i * ldv + j];
    else if (i >= n0 && j >= n0)
      v = 0.0;
    else
      v = BT[(long long)(i < n0 ? i : j) * ldb + (i < n0 ? j : i) - n0];
    Km[i * ld + j] = v;
  }
  __syncthreads();
  for (int e = tid; e < qmax * qmax; e += nt) {
    const int i = e / qmax, j = e - i * qmax;
    K0mat[(long long)i * ldq + j] = (i < q && j < q) ? Km[i * ld + j] : 0.0;
  }
  for (int i = tid; i < q; i += nt) {
    double d = 1.0;
    if (i < n0) {
      const double kii = Km[i * ld + i];
      if (kii > 1.0) d = 1.0 / sqrt(kii);
    }
    dsc[i] = d;
  }
  __syncthreads();
  for (int e = tid; e < q * q; e += nt) Km[(e / q) * ld + e % q] *= dsc[e / q] * dsc[e % q];
  __syncthreads();
  const int bad = lu_complete<BIG ? HQPKKT_GJ_RB : 1>(Km, q, ld, pr, pc, colv, rowv, red);
  if (bad && tid == 0) atomicExch(status, 4);
  __syncthreads();
  for (int e = tid; e < qmax * qmax; e += nt) {
    const int i = e / qmax, j = e - i * qmax;
    K0lu[(long long)i * ldq + j] = (i < q && j < q) ? Km[i * ld + j] : 0.0;
  }
  for (int i = tid; i < q; i += nt) K0s[i] = dsc[i], K0s[qmax + i] = (double)pr[i], K0s[2 * qmax + i] = (double)pc[i];
  if (tid == 0) K0s[3 * qmax] = 0.0;  // the area K0lu holds LU factors
}

// The same matrix of a free initial state with hundreds of components, inverted by the blocked sweep on the whole chip
// (k_blk_pivot / two products / k_blk_fixup per block of 64, as for a stage's K): k_x0_prepare writes the scaled matrix
// (identity beyond the live order n0 + carried rows), k_x0_final the inverse, unscaled and symmetrised, into the area
// of the factors, k_x0_check compares K0 K0^-1 with the identity and leaves the verdict in K0s[3 qmax] (1: the area
// holds the inverse; 0: LU factors - written by k_st_init_factor behind it, which runs only where the sweep gave up or
// failed the check).  1000 components: 99 ms -> a few ms.  hqp/Hqp_IpLQDOCP.C:1972-1996 factorises the same matrix.
struct X0Args {
  int n0, qmax;
  const double *V;
  long long ldv;
  const double *BT;
  long long ldb;
  const int *dyn0;
  double *K0inv, *K0mat, *K0s;
  long long ldq;
  double *scratch;
  int *status;
};
__global__ void k_x0_prepare(X0Args a) {
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)a.qmax * a.qmax) return;
  const int i = (int)(e / a.qmax), j = (int)(e - (long long)i * a.qmax), q = a.n0 + a.dyn0[1];
  double v = 0.0, sc = 1.0;
  if (i < q && j < q) {
    if (i < a.n0 && j < a.n0)
      v = a.V[(long long)i * a.ldv + j];
    else if (i < a.n0 || j < a.n0)
      v = a.BT[(long long)(i < a.n0 ? i : j) * a.ldb + (i < a.n0 ? j : i) - a.n0];
    if (i < a.n0) {
      const double kii = a.V[(long long)i * a.ldv + i];
      if (kii > 1.0) sc = 1.0 / sqrt(kii);
    }
    if (j < a.n0) {
      const double kjj = a.V[(long long)j * a.ldv + j];
      if (kjj > 1.0) sc *= 1.0 / sqrt(kjj);
    }
  }
  a.K0mat[(long long)i * a.ldq + j] = v;
  bs.Ks[(long long)i * bs.ldk + j] = (i < q && j < q) ? v * sc : (i == j ? 1.0 : 0.0);
  if (j == 0) {
    double d = 0.0;
    if (i < q) {
      d = 1.0;
      if (i < a.n0) {
        const double kii = a.V[(long long)i * a.ldv + i];
        if (kii > 1.0) d = 1.0 / sqrt(kii);
      }
    }
    bs.dsc[i] = d;
  }
  if (e == 0) bs.flags[0] = bs.flags[1] = bs.flags[2] = bs.flags[3] = bs.flags[4] = 0, atomicAdd(a.status + X0_BLOCKED, 1);
}
__global__ void k_x0_final(X0Args a) {
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0]) return;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)a.qmax * a.qmax) return;
  const int i = (int)(e / a.qmax), l = (int)(e - (long long)i * a.qmax), q = a.n0 + a.dyn0[1];
  double v = 0.0;
  if (i < q && l < q) v = -0.5 * (bs.Ks[(long long)i * bs.ldk + l] + bs.Ks[(long long)l * bs.ldk + i]) * bs.dsc[i] * bs.dsc[l];
  a.K0inv[(long long)i * a.ldq + l] = v;
}
// E = K0 K0inv (in the area of the swept matrix) against the identity of the live order; the verdict
__global__ void __launch_bounds__(1024) k_x0_check(X0Args a, double tol) {
  __shared__ ArgMax red[16];
  const BigScratch bs = big_scratch(a.scratch, a.qmax);
  if (bs.flags[0] == 0) {
    const int q = a.n0 + a.dyn0[1];
    ArgMax am{0.0, 0};
    for (long long e = threadIdx.x; e < (long long)a.qmax * a.qmax; e += blockDim.x) {
      const int i = (int)(e / a.qmax), l = (int)(e - (long long)i * a.qmax);
      const double d = fabs(bs.Ks[(long long)i * bs.ldk + l] - ((i == l && i < q) ? 1.0 : 0.0));
      if (!(d <= am.v)) am.v = d == d ? d : __longlong_as_double(0x7ff0000000000000LL);
    }
    am = block_argmax(am, red);
    if (threadIdx.x == 0) {
      bs.flags[4] = __float_as_int((float)am.v);  // (introspection: max |K0 K0^-1 - I|)
      if (!(am.v <= tol)) bs.flags[0] = 1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) a.K0s[3 * a.qmax] = bs.flags[0] ? 0.0 : 1.0;
}
// the solve with the inverse: rhs (nb = -b, pb = b with b = [v_0 ; beta_0], zero beyond the live order), three products
// by k_st_gemv_rows (y = K0inv nb; r = -(pb + K0 y); z = y + K0inv r: one round of refinement against K0), the result
struct X0Vec {
  int n0, cap0, qmax;
  const int *dyn0;
  const double *K0s;
  const double *v0, *beta0;
  double *nb, *pb;
  const double *z;
  double *x0, *eta0;
};
__global__ void k_x0_rhs(X0Vec a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.qmax) return;
  const int q = a.n0 + a.dyn0[1];
  const double b = i < q ? (i < a.n0 ? a.v0[i] : a.beta0[i - a.n0]) : 0.0;
  a.nb[i] = -b, a.pb[i] = b;
}
__global__ void k_x0_out(X0Vec a) {
  if (a.K0s[3 * a.qmax] != 1.0) return;  // (the factors are in use: k_st_x0_free writes the result)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n0 + a.cap0) return;
  const int q = a.n0 + a.dyn0[1];
  const double s = i < q ? a.z[i] : 0.0;
  if (i < a.n0)
    a.x0[i] = s;
  else
    a.eta0[i - a.n0] = s;
}

// ---------------------------------------------------------------------------------------
// dense matrix-vector products of the two sweeps (HBM-bound: a stage block is read once)
// rows form: y[i] = add[i] + sum_j A[i][j] x[j] (+ sum_l A2[i][l] x2[l]), one wavefront per row
struct GemvRows {
  const double *A;
  long long lda;
  int M, N;
  const double *x;
  const double *add;  // may be null
  const double *A2;   // optional second block (the carried rows: BT eta)
  long long lda2;
  const int *n2;      // live columns of A2 (device)
  const double *x2;
  double *y;
  double scale;       // y = scale * (...)
};
__global__ void __launch_bounds__(256) k_st_gemv_rows(GemvRows g) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= g.M) return;
  const double *ar = g.A + (long long)row * g.lda;
  double s = 0.0;
  if ((((size_t)ar) & 15) == 0) {
    // 16-byte loads of the matrix row (it is what streams from HBM), four in flight per lane
    const double2_t *a2 = (const double2_t *)ar;
    const int n2 = g.N >> 1;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = lane;
    for (; j + 192 < n2; j += 256) {
      const double2_t v0 = a2[j], v1 = a2[j + 64], v2 = a2[j + 128], v3 = a2[j + 192];
      s0 += v0.x * g.x[2 * j] + v0.y * g.x[2 * j + 1];
      s1 += v1.x * g.x[2 * (j + 64)] + v1.y * g.x[2 * (j + 64) + 1];
      s2 += v2.x * g.x[2 * (j + 128)] + v2.y * g.x[2 * (j + 128) + 1];
      s3 += v3.x * g.x[2 * (j + 192)] + v3.y * g.x[2 * (j + 192) + 1];
    }
    for (; j < n2; j += 64) {
      const double2_t v0 = a2[j];
      s0 += v0.x * g.x[2 * j] + v0.y * g.x[2 * j + 1];
    }
    if ((g.N & 1) && lane == 0) s0 += ar[g.N - 1] * g.x[g.N - 1];
    s = (s0 + s1) + (s2 + s3);
  } else
    for (int j = lane; j < g.N; j += 64) s += ar[j] * g.x[j];
  if (g.A2) {
    const int k2 = *g.n2;
    const double *br = g.A2 + (long long)row * g.lda2;
    for (int j = lane; j < k2; j += 64) s += br[j] * g.x2[j];
  }
  s = kktdev::wave_sum(s);
  if (lane == 0) g.y[row] = g.scale * ((g.add ? g.add[row] : 0.0) + s);
}
// The same product with a SYMMETRIC matrix stored in full (V of a stage: the lower tiles and their mirror images, exactly
// symmetric), reading only the tiles on and below the diagonal: a tile of SV_R rows x SV_C columns gives the partial dot
// products of its rows (rowpart[column tile][row]) and, from the same registers, the partial products of the mirrored
// elements (colpart[row tile][column]: sum over the tile's rows i of V[i][j] x[i], elements strictly below the
// diagonal).  k_st_symv_finish adds the partials of a row in a fixed order (reproducible from run to run), the carried
// rows' term and `add`.  HBM traffic: half the matrix plus (N / SV_R + N / SV_C) N / 2 doubles of partials, twice.
constexpr int SV_R = 64, SV_P = 4, SV_C = 128 * SV_P, SV_U = 4;  // rows, 16-byte loads per lane and row, columns of a tile; rows in flight
struct SymvArgs {
  const double *V;
  long long ldv;
  int N;
  const double *x;
  double *rowpart;  // [ceil(N / SV_C)][N]
  double *colpart;  // [ceil(N / SV_R)][N]
};
// (measured on the 5000 x 5000 V of the headline, tools/symv_probe.hip: 22.8 us for the 113 MB of the triangle's tiles
// against 37.1 us for the rows form over the whole matrix; tiles of 64 x 256, 32 x 512, 96 x 512, 128 x 512 and 2 / 8
// rows in flight: 22.2 - 32 us; the row sums by DPP, 1 us less than by ds_bpermute)
// tile number -> (row tile bi, column tile bj) over the tiles on and below the diagonal: the RT = SV_C / SV_R row tiles
// RT g .. RT g + RT - 1 have g + 1 column tiles each, RT g (g + 1) / 2 tiles stand before them (the host evaluates the
// same code: hqpkkt_debug_symv_map)
__host__ __device__ __forceinline__ void symv_tile_pair(const int t, int &bi, int &bj) {
  constexpr int RT = SV_C / SV_R;
  int gq = (int)((sqrt(1.0 + 8.0 * t / RT) - 1.0) * 0.5);
  while (RT * gq * (gq + 1) / 2 > t) gq--;
  while (RT * (gq + 1) * (gq + 2) / 2 <= t) gq++;
  const int rem = t - RT * gq * (gq + 1) / 2;
  bi = RT * gq + rem / (gq + 1), bj = rem % (gq + 1);
}
__device__ __forceinline__ void symv_tile(const SymvArgs &g, const int t, double (*red)[SV_C]) {
  int bi, bj;
  symv_tile_pair(t, bi, bj);
  const int r0 = bi * SV_R, c0 = bj * SV_C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool diag = c0 + SV_C - 1 >= r0;  // the tile meets the diagonal: element masks
  int jj[SV_P];                           // this lane's column pairs (jj, jj + 1)
  double xa[SV_P], xb[SV_P], ca[SV_P], cb[SV_P];
#pragma unroll
  for (int p = 0; p < SV_P; p++) {
    jj[p] = c0 + 2 * lane + 128 * p;
    xa[p] = jj[p] < g.N ? g.x[jj[p]] : 0.0, xb[p] = jj[p] + 1 < g.N ? g.x[jj[p] + 1] : 0.0;
    ca[p] = cb[p] = 0.0;
  }
  const int ra = r0 + wave * (SV_R / 4), rb = min(g.N, ra + SV_R / 4);
  const double *row = g.V + (long long)ra * g.ldv;
  double *rp = g.rowpart + (long long)bj * g.N;
  for (int i = ra; i < rb; i += SV_U) {
    double2_t v[SV_U][SV_P];
    double xi[SV_U];
#pragma unroll
    for (int u = 0; u < SV_U; u++) {
      const bool live = i + u < rb;
#pragma unroll
      for (int p = 0; p < SV_P; p++)
        v[u][p] = (live && jj[p] < g.N) ? *(const double2_t *)(row + (long long)u * g.ldv + jj[p]) : double2_t{0.0, 0.0};
      xi[u] = live ? g.x[i + u] : 0.0;
    }
    row += SV_U * g.ldv;
#pragma unroll
    for (int u = 0; u < SV_U; u++) {
      const int ii = i + u;
      double s = 0.0;
#pragma unroll
      for (int p = 0; p < SV_P; p++) {
        double a = v[u][p].x, b = jj[p] + 1 < g.N ? v[u][p].y : 0.0;
        if (diag) {  // row part: columns <= ii
          if (jj[p] > ii) a = 0.0;
          if (jj[p] + 1 > ii) b = 0.0;
        }
        s += a * xa[p] + b * xb[p];
        if (diag) {  // mirrored part: columns < ii
          if (jj[p] == ii) a = 0.0;
          if (jj[p] + 1 == ii) b = 0.0;
        }
        ca[p] += a * xi[u], cb[p] += b * xi[u];
      }
      s = kktdev::wave_sum_dpp(s);
      if (lane == 0 && ii < rb) rp[ii] = s;
    }
  }
#pragma unroll
  for (int p = 0; p < SV_P; p++) red[wave][128 * p + 2 * lane] = ca[p], red[wave][128 * p + 2 * lane + 1] = cb[p];
  __syncthreads();
  for (int c = threadIdx.x; c < SV_C; c += 256)
    if (c0 + c < g.N) g.colpart[(long long)bi * g.N + c0 + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}
__global__ void __launch_bounds__(256) k_st_symv_tiles(SymvArgs g) {
  __shared__ double red[4][SV_C];
  symv_tile(g, blockIdx.x, red);
}
struct SymvFinish {
  int N;
  const double *rowpart, *colpart;
  const double *add;  // may be null
  const double *A2;   // optional block of carried rows (as GemvRows)
  long long lda2;
  const int *n2;
  const double *x2;
  double *y;
  double scale;
};
__device__ __forceinline__ void symv_finish_blk(const SymvFinish &g, const int blk, double (*red)[64]) {
  // 64 columns per workgroup, four threads per column: thread group q adds every fourth partial of the mirrored part
  // (eight loads in flight), group 0 the row parts and the carried rows' term; fixed order throughout
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, j = blk * 64 + cl;
  double s = 0.0;
  if (j < g.N) {
    const int bi = j / SV_R, nrt = (g.N + SV_R - 1) / SV_R, ct = (bi * SV_R + SV_R - 1) / SV_C;
    int b = bi + q;
    for (; b + 28 < nrt; b += 32) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = g.colpart[(long long)(b + 4 * u) * g.N + j];
#pragma unroll
      for (int u = 0; u < 8; u++) s += v[u];
    }
    for (; b < nrt; b += 4) s += g.colpart[(long long)b * g.N + j];
    {  // the row parts: every fourth one per group, up to eight loads in flight
      double v[8];
      for (int t0 = q; t0 <= ct; t0 += 32) {
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = t0 + 4 * u <= ct ? g.rowpart[(long long)(t0 + 4 * u) * g.N + j] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) s += v[u];
      }
    }
    if (q == 0) {
      if (g.A2) {
        const int k2 = *g.n2;
        const double *br = g.A2 + (long long)j * g.lda2;
        for (int l = 0; l < k2; l++) s += br[l] * g.x2[l];
      }
    }
  }
  red[q][cl] = s;
  __syncthreads();
  if (q == 0 && j < g.N) g.y[j] = g.scale * ((g.add ? g.add[j] : 0.0) + ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])));
}
__global__ void __launch_bounds__(256) k_st_symv_finish(SymvFinish g) {
  __shared__ double red[4][64];
  symv_finish_blk(g, blockIdx.x, red);
}
// The products with V that stand outside the chains of the two sweeps - g_k = V+ f_k with the dynamics' right-hand side
// (known before the backward sweep starts), the dynamics rows' multipliers V+ x+ + v+ + B+' eta+ (wanted by nobody before
// the sweep is over) - for MANY stages per launch: item i holds the tiles tile0 .. (next item's tile0) of the launch and
// the finishing blocks fin0 ..; partial sums of its own.  The vectors of the caller (right-hand side, multipliers) are
// addressed relative to a base, so that one table serves every set of vectors the solve runs on.
struct SymvItem {
  SymvArgs a;
  SymvFinish f;
  int tile0, fin0;      // first tile / finishing block inside the launch
  int xrel, yrel;       // a.x = xbase + xoff / f.y = ybase + yoff
  long long xoff, yoff;
};
__device__ __forceinline__ int symv_item_of(const SymvItem *items, int cnt, int blk, bool fin) {
  int lo = 0, hi = cnt - 1;  // the last item whose first block is <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((fin ? items[mid].fin0 : items[mid].tile0) <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// (a grid smaller than the number of tiles / blocks: every workgroup takes several, in a stride)
__global__ void __launch_bounds__(256) k_st_symv_tiles_batch(const SymvItem *__restrict__ items, int cnt, int tiles, const double *xbase) {
  __shared__ double red[4][SV_C];
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const SymvItem &it = items[symv_item_of(items, cnt, t, false)];
    SymvArgs a = it.a;
    if (it.xrel) a.x = xbase + it.xoff;
    symv_tile(a, t - it.tile0, red);
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_st_symv_finish_batch(const SymvItem *__restrict__ items, int cnt, int fins, double *ybase) {
  __shared__ double red[4][64];
  for (int t = blockIdx.x; t < fins; t += gridDim.x) {
    const SymvItem &it = items[symv_item_of(items, cnt, t, true)];
    SymvFinish f = it.f;
    if (it.yrel) f.y = ybase + it.yoff;
    symv_finish_blk(f, t - it.fin0, red);
    __syncthreads();
  }
}
// the same for few, long rows (Rm x with a handful of controls and thousands of states): one
// workgroup per row, so that a row's bytes are in flight from 256 threads
__global__ void __launch_bounds__(256) k_st_gemv_wide(GemvRows g) {
  __shared__ double red[4];
  const int row = blockIdx.x;
  const double *ar = g.A + (long long)row * g.lda;
  double s = 0.0;
  if ((((size_t)ar) & 15) == 0) {
    // 16-byte loads, four in flight per thread (a row of 5000 states: 10 loads per thread, three batches instead of
    // twenty dependent round trips: 10.7 -> ~4 us)
    const double2_t *a2 = (const double2_t *)ar;
    const int n2 = g.N >> 1;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = threadIdx.x;
    for (; j + 768 < n2; j += 1024) {
      const double2_t v0 = a2[j], v1 = a2[j + 256], v2 = a2[j + 512], v3 = a2[j + 768];
      s += v0.x * g.x[2 * j] + v0.y * g.x[2 * j + 1];
      s1 += v1.x * g.x[2 * (j + 256)] + v1.y * g.x[2 * (j + 256) + 1];
      s2 += v2.x * g.x[2 * (j + 512)] + v2.y * g.x[2 * (j + 512) + 1];
      s3 += v3.x * g.x[2 * (j + 768)] + v3.y * g.x[2 * (j + 768) + 1];
    }
    for (; j < n2; j += 256) {
      const double2_t v0 = a2[j];
      s += v0.x * g.x[2 * j] + v0.y * g.x[2 * j + 1];
    }
    if ((g.N & 1) && threadIdx.x == 0) s += ar[g.N - 1] * g.x[g.N - 1];
    s = (s + s1) + (s2 + s3);
  } else
    for (int j = threadIdx.x; j < g.N; j += 256) s += ar[j] * g.x[j];
  s = kktdev::wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) g.y[row] = g.scale * ((g.add ? g.add[row] : 0.0) + ((red[0] + red[1]) + (red[2] + red[3])));
}
// columns form: part[s][j] = sum over the rows k of chunk s of A[k][j] x[k]; with one chunk the
// result y[j] = add[j] + alpha * sum is written directly
struct GemvCols {
  const double *A;
  long long lda;
  int K, N;
  const double *x;
  const double *add;
  double alpha;
  double *y;
  double *part;  // nchunk x N
  int rows_per_chunk;
  const double *add2 = nullptr;  // optional second result y2 = y + add2 (the backward sweep: v_k and, with the product
  double *y2 = nullptr;          // V_k f_{k-1} computed ahead of the sweep, v_k + V_k f_{k-1})
};
__global__ void __launch_bounds__(256) k_st_gemv_cols(GemvCols g) {
  // two neighbouring columns per thread (one 16-byte load per row; rows 16-byte aligned when lda is even and the
  // block starts aligned), four rows in flight
  const int j = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= g.N) return;
  const int k0 = blockIdx.y * g.rows_per_chunk, k1 = min(g.K, k0 + g.rows_per_chunk);
  double s0 = 0.0, s1 = 0.0;
  const double *a = g.A + (long long)k0 * g.lda + j;
  if (j + 1 < g.N && (((size_t)a) & 15) == 0 && (g.lda & 1) == 0) {
    double t0 = 0.0, t1 = 0.0, u0 = 0.0, u1 = 0.0, w0 = 0.0, w1 = 0.0;
    int k = k0;
    // (eight rows in flight first: with few rows and one chunk - Y' rho, a few dozen rows - the loop is a chain of
    // memory round trips; the sums are added in the order of the four-row form)
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
    for (; k + 3 < k1; k += 4, a += 4 * g.lda) {
      const double2_t v0 = *(const double2_t *)a, v1 = *(const double2_t *)(a + g.lda), v2 = *(const double2_t *)(a + 2 * g.lda),
                      v3 = *(const double2_t *)(a + 3 * g.lda);
      const double x0 = g.x[k], x1 = g.x[k + 1], x2 = g.x[k + 2], x3 = g.x[k + 3];
      s0 += v0.x * x0, s1 += v0.y * x0, t0 += v1.x * x1, t1 += v1.y * x1;
      u0 += v2.x * x2, u1 += v2.y * x2, w0 += v3.x * x3, w1 += v3.y * x3;
    }
    for (; k < k1; k++, a += g.lda) {
      const double2_t v0 = *(const double2_t *)a;
      s0 += v0.x * g.x[k], s1 += v0.y * g.x[k];
    }
    s0 = (s0 + t0) + (u0 + w0), s1 = (s1 + t1) + (u1 + w1);
  } else {
    for (int k = k0; k < k1; k++, a += g.lda) {
      s0 += a[0] * g.x[k];
      if (j + 1 < g.N) s1 += a[1] * g.x[k];
    }
  }
  if (gridDim.y == 1) {
    const double r0 = (g.add ? g.add[j] : 0.0) + g.alpha * s0;
    g.y[j] = r0;
    if (g.y2) g.y2[j] = r0 + g.add2[j];
    if (j + 1 < g.N) {
      const double r1 = (g.add ? g.add[j + 1] : 0.0) + g.alpha * s1;
      g.y[j + 1] = r1;
      if (g.y2) g.y2[j + 1] = r1 + g.add2[j + 1];
    }
  } else {
    g.part[(long long)blockIdx.y * g.N + j] = s0;
    if (j + 1 < g.N) g.part[(long long)blockIdx.y * g.N + j + 1] = s1;
  }
}
__global__ void k_st_cols_finish(int N, int nchunk, const double *__restrict__ part, const double *__restrict__ add,
                                 double alpha, double *__restrict__ y, const double *__restrict__ add2 = nullptr,
                                 double *__restrict__ y2 = nullptr) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N) return;
  double s = 0.0;
  int c = 0;
  for (; c + 8 <= nchunk; c += 8) {  // (eight loads in flight; the order of the sum as before)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = part[(long long)(c + u) * N + j];
#pragma unroll
    for (int u = 0; u < 8; u++) s += v[u];
  }
  for (; c < nchunk; c++) s += part[(long long)c * N + j];
  const double r = (add ? add[j] : 0.0) + alpha * s;
  y[j] = r;
  if (y2) y2[j] = r + add2[j];
}

// The launches of these products on stream s, for the engine (staged_host.hip.h) and for the test hooks
// (hqpkkt_debug_gemv_dense, hqpkkt_debug_symv, hqpkkt_debug_symv_batch); `around` as in pf_launch_rows.
template <class Around>
static inline void gemv_launch_rows(const GemvRows &g, hipStream_t s, Around &&around) {
  if (g.M <= 0) return;
  around([&]() { k_st_gemv_rows<<<(g.M + 3) / 4, 256, 0, s>>>(g); });
}
// (k_st_gemv_wide has no guard `row >= M`: exactly M workgroups)
template <class Around>
static inline void gemv_launch_wide(const GemvRows &g, hipStream_t s, Around &&around) {
  if (g.M <= 0) return;
  around([&]() { k_st_gemv_wide<<<g.M, 256, 0, s>>>(g); });
}
// chunks of the columns form: at least 64 rows each, at most the plan's part_chunks; g.part holds part_chunks x N
// doubles, g.rows_per_chunk is set here.  Returns the chunks launched.
static inline int gemv_cols_chunks(int part_chunks, int K) { return std::max(1, std::min(part_chunks, K / 64)); }
template <class Around>
static inline int gemv_launch_cols(GemvCols g, int part_chunks, hipStream_t s, Around &&around) {
  if (g.N <= 0) return 0;
  const int chunks = gemv_cols_chunks(part_chunks, g.K);
  g.rows_per_chunk = (g.K + chunks - 1) / chunks;
  around([&]() { k_st_gemv_cols<<<dim3((g.N + 511) / 512, chunks), 256, 0, s>>>(g); });
  if (chunks > 1) around([&]() { k_st_cols_finish<<<(g.N + 255) / 256, 256, 0, s>>>(g.N, chunks, g.part, g.add, g.alpha, g.y, g.add2, g.y2); });
  return chunks;
}
// triangle form: tiles on and below the diagonal of an N x N matrix, and where the partial sums of one product lie in
// a scratch area of StagedPlan::symv_need(N) doubles (the row parts first, the mirrored parts behind ceil(N / SV_C) N)
static inline long long symv_tiles(int N) {
  const int nrt = (N + SV_R - 1) / SV_R;
  long long tiles = 0;
  for (int bi = 0; bi < nrt; bi++) tiles += bi / (SV_C / SV_R) + 1;
  return tiles;
}
static inline void symv_parts(double *scratch, int N, double *&rowpart, double *&colpart) {
  static_assert(SV_R == 64 && SV_C == 512, "StagedPlan::symv_need is sized for these tiles");
  rowpart = scratch, colpart = scratch + (long long)((N + SV_C - 1) / SV_C) * N;
}
// y = scale (add + V x + A2 x2), g as for the rows form with M = N, an even lda and a 16-byte aligned A
template <class Around>
static inline void symv_launch(const GemvRows &g, double *scratch, hipStream_t s, Around &&around) {
  const int N = g.N;
  if (N <= 0) return;
  double *rowpart, *colpart;
  symv_parts(scratch, N, rowpart, colpart);
  const long long tiles = symv_tiles(N);
  around([&]() { k_st_symv_tiles<<<(unsigned)tiles, 256, 0, s>>>(SymvArgs{g.A, g.lda, N, g.x, rowpart, colpart}); });
  around([&]() { k_st_symv_finish<<<(N + 63) / 64, 256, 0, s>>>(SymvFinish{N, rowpart, colpart, g.add, g.A2, g.lda2, g.n2, g.x2, g.y, g.scale}); });
}
// many products per launch: `count` items (device) of `tiles` tiles and `fins` finishing blocks in all, on grid_tiles /
// grid_fins workgroups (0: one per tile / per block)
template <class Around>
static inline void symv_launch_batch(const SymvItem *items, int count, int tiles, int fins, int grid_tiles, int grid_fins, const double *xbase,
                                     double *ybase, hipStream_t s, Around &&around) {
  if (count <= 0 || tiles <= 0 || fins <= 0) return;
  around([&]() { k_st_symv_tiles_batch<<<(unsigned)(grid_tiles > 0 ? grid_tiles : tiles), 256, 0, s>>>(items, count, tiles, xbase); });
  around([&]() { k_st_symv_finish_batch<<<(unsigned)(grid_fins > 0 ? grid_fins : fins), 256, 0, s>>>(items, count, fins, ybase); });
}

// q = -(r1 - C' tz)   (the reference's gx, gu: hqp/Hqp_IpLQDOCP.C:884-918)
// xc (or NULL): the share of the wide rows of C, which the arrays of C' then do not hold (k_st_rows_gemv_t)
__global__ void k_st_q(int n, const int *__restrict__ CTp, const int *__restrict__ CTc, const int *__restrict__ CTs,
                       const double *__restrict__ vals, const double *__restrict__ tz, const double *__restrict__ r1,
                       double *__restrict__ q, const double *__restrict__ xc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = CTp[i]; k < CTp[i + 1]; k++) s += vals[CTs[k]] * tz[CTc[k]];
  if (xc) s += xc[i];
  q[i] = s - r1[i];
}

// backward sweep, the small part of a stage (one workgroup):
//   nu = [a_k ; beta+ + B+ f],  y0 = [gam_u ; nu_R],  rho = K^-1 y0 (+ one round of refinement against K:
//   the product with an explicit inverse alone has a residual of cond(K) eps, a solve by factors has not),
//   beta = nu_L - t nu_R
struct BwdSmall {
  int n, m, np, e, capn, cap, qmax;
  const int *eq_rows;        // QP row index of the own equality rows
  const double *r2;
  const int *cnt_next;       // live carried rows coming in (nullptr: none)
  const double *beta_next;
  const double *BT_next;     // np x ldbn
  long long ldbn;
  const double *f;           // r2 + first dynamics row of the stage
  const double *gam;         // n + m
  const double *Kinv;
  const double *Kmat;
  long long ldq;
  const double *t;
  long long ldt;
  const int *dyn;
  double *rho;               // qmax
  double *beta;              // cap
};
__global__ void __launch_bounds__(256) k_st_bwd_small(BwdSmall a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int cn = a.cnt_next ? *a.cnt_next : 0;
  const int r = a.dyn[0], nl = a.dyn[1];
  const int *Rl = a.dyn + 2, *Ll = a.dyn + 2 + a.capn;
  double *nu = sm, *y0 = sm + a.capn + 1;
  // K of order <= 64: this thread's 16 entries of column (tid & 63) of K^-1 and of K are requested before anything else
  // (they come from HBM: the factorisation wrote them long ago) and the three products below run out of registers,
  // four partial sums per entry meeting in LDS.  (Both are stored zero-padded to qmax and symmetric.)
  const bool fastq = a.qmax <= 64 && nt == 256;
  const int ci = tid & 63, part = tid >> 6;
  double ki[16], km[16];
  if (fastq) {
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int j = part * 16 + u;
      const bool ok = j < a.qmax && ci < a.qmax;
      ki[u] = ok ? a.Kinv[(long long)j * a.ldq + ci] : 0.0;
      km[u] = ok ? a.Kmat[(long long)j * a.ldq + ci] : 0.0;
    }
  }
  for (int i = tid; i < a.e; i += nt) nu[i] = a.r2[a.eq_rows[i]];
  // carried rows: beta+ + B+ f, one wavefront per row
  for (int li = tid >> 6; li < cn; li += nt >> 6) {
    double s = 0.0;
    for (int k = tid & 63; k < a.np; k += 64) s += a.BT_next[(long long)k * a.ldbn + li] * a.f[k];
    s = kktdev::wave_sum(s);
    if ((tid & 63) == 0) nu[a.e + li] = a.beta_next[li] + s;
  }
  __syncthreads();
  const int q = a.m + r;
  for (int i = tid; i < q; i += nt) y0[i] = i < a.m ? a.gam[a.n + i] : nu[Rl[i - a.m]];
  __syncthreads();
  double *rh = y0 + a.qmax, *rs = rh + a.qmax;
  if (fastq) {
    double *P = rs + a.qmax;  // 4 x 64 partial sums
    auto col_times = [&](const double(&kk)[16], const double *x) {
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < 16; u++) {
        const int j = part * 16 + u;
        s = fma(kk[u], j < q ? x[j] : 0.0, s);
      }
      P[part * 64 + ci] = s;
    };
    col_times(ki, y0);
    __syncthreads();
    if (tid < q) rh[tid] = (P[tid] + P[64 + tid]) + (P[128 + tid] + P[192 + tid]);
    __syncthreads();
    col_times(km, rh);
    __syncthreads();
    if (tid < q) rs[tid] = y0[tid] - ((P[tid] + P[64 + tid]) + (P[128 + tid] + P[192 + tid]));
    __syncthreads();
    col_times(ki, rs);
    __syncthreads();
    if (tid < a.qmax) a.rho[tid] = tid < q ? rh[tid] + ((P[tid] + P[64 + tid]) + (P[128 + tid] + P[192 + tid])) : 0.0;
  } else {
  for (int i = tid; i < q; i += nt) {
    double s = 0.0;  // K^-1 and K are stored symmetric: column i, so that neighbouring threads read neighbouring words
    for (int j = 0; j < q; j++) s += a.Kinv[(long long)j * a.ldq + i] * y0[j];
    rh[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < q; i += nt) {
    double s = y0[i];
    for (int j = 0; j < q; j++) s -= a.Kmat[(long long)j * a.ldq + i] * rh[j];
    rs[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < a.qmax; i += nt) {
    double s = 0.0;
    if (i < q) {
      for (int j = 0; j < q; j++) s += a.Kinv[(long long)j * a.ldq + i] * rs[j];
      s += rh[i];
    }
    a.rho[i] = s;
  }
  }
  for (int li = tid; li < a.cap; li += nt) {
    double s = 0.0;
    if (li < nl) {
      s = nu[Ll[li]];
      for (int k = 0; k < r; k++) s -= a.t[(long long)li * a.ldt + k] * nu[Rl[k]];
    }
    a.beta[li] = s;
  }
}

// forward sweep, the small part of a stage (one workgroup):
//   [u ; yhat] = -(Rm x + rho);  multipliers of the rows of N: consumed yhat - t' eta, leftover eta;
//   own rows -> dy, carried rows -> eta of stage k+1
struct FwdSmall {
  int n, m, e, capn, cap, qmax;
  const double *uy;    // -(Rm x_k + rho), qmax entries (k_st_gemv_wide)
  const double *t;
  long long ldt;
  const int *dyn;
  const double *eta;   // multipliers of this stage's leftover rows (cap)
  const int *eq_rows;
  double *u;           // m (inside the s vector)
  double *dy;
  double *eta_next;    // capn - e entries at most
  int cap_next;
};
__global__ void __launch_bounds__(256) k_st_fwd_small(FwdSmall a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int r = a.dyn[0], nl = a.dyn[1];
  const int *Rl = a.dyn + 2, *Ll = a.dyn + 2 + a.capn;
  const double *uy = a.uy;
  double *yN = sm;
  for (int i = tid; i < a.m; i += nt) a.u[i] = uy[i];
  for (int s = tid; s < r; s += nt) {
    double v = uy[a.m + s];
    for (int li = 0; li < nl; li++) v -= a.t[(long long)li * a.ldt + s] * a.eta[li];
    yN[Rl[s]] = v;
  }
  for (int li = tid; li < nl; li += nt) yN[Ll[li]] = a.eta[li];
  __syncthreads();
  const int c = r + nl;
  for (int i = tid; i < a.e; i += nt) a.dy[a.eq_rows[i]] = yN[i];
  for (int i = tid; i < a.cap_next; i += nt) a.eta_next[i] = (a.e + i < c) ? yN[a.e + i] : 0.0;
}

// initial state.  Fixed: x_0 = -r2[fix] / val, eta_0 = 0.  Free: [x_0 ; eta_0] = -K0^-1 [v_0 ; beta_0]
__global__ void k_st_x0_fixed(int n0, const int *__restrict__ fix_rows, const int *__restrict__ fix_src,
                              const double *__restrict__ vals, const double *__restrict__ r2, double *__restrict__ x0,
                              double *__restrict__ eta0, int cap0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n0) x0[i] = -r2[fix_rows[i]] / vals[fix_src[i]];
  if (i < cap0) eta0[i] = 0.0;
}
// multipliers of the rows that fix x_0: -(V_0 x_0 + v_0) / val   (tmp = v_0 + V_0 x_0)
__global__ void k_st_y_fixed(int n0, const int *__restrict__ fix_rows, const int *__restrict__ fix_src,
                             const double *__restrict__ vals, const double *__restrict__ tmp, double *__restrict__ dy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n0) dy[fix_rows[i]] = -tmp[i] / vals[fix_src[i]];
}
// t <- (D K D)^-1 t by the factors of k_st_init_factor (t in LDS, already scaled by D): row exchanges, L, U, column
// exchanges.  Blocks of 64 unknowns: the part of a block's rows outside its diagonal block is one dot product per
// row (a wavefront per row, coalesced), the diagonal block is solved by one wavefront out of LDS.
__device__ void x0_lu_solve(const double *__restrict__ LU, long long ldq, const double *__restrict__ perm, int qmax, int q,
                            double *t, double *T) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  if (tid == 0)
    for (int s = 0; s < q; s++) {
      const int r = (int)perm[qmax + s];
      const double x = t[s];
      t[s] = t[r], t[r] = x;
    }
  __syncthreads();
  for (int b0 = 0; b0 < q; b0 += 64) {  // L y = t
    const int nb = min(64, q - b0);
    for (int i = wave; i < nb; i += nw) {
      double sum = 0.0;
      for (int j = lane; j < b0; j += 64) sum += LU[(long long)(b0 + i) * ldq + j] * t[j];
      sum = kktdev::wave_sum(sum);
      if (lane == 0) t[b0 + i] -= sum;
    }
    for (int e = tid; e < nb * nb; e += blockDim.x) T[(e / nb) * 65 + e % nb] = LU[(long long)(b0 + e / nb) * ldq + b0 + e % nb];
    __syncthreads();
    if (wave == 0) {
      double y = lane < nb ? t[b0 + lane] : 0.0;
      for (int s = 0; s < nb; s++) {
        const double ys = __shfl(y, s);
        if (lane > s && lane < nb) y -= T[lane * 65 + s] * ys;
      }
      if (lane < nb) t[b0 + lane] = y;
    }
    __syncthreads();
  }
  for (int b0 = ((q - 1) / 64) * 64; b0 >= 0; b0 -= 64) {  // U z = y
    const int nb = min(64, q - b0);
    for (int i = wave; i < nb; i += nw) {
      double sum = 0.0;
      for (int j = b0 + nb + lane; j < q; j += 64) sum += LU[(long long)(b0 + i) * ldq + j] * t[j];
      sum = kktdev::wave_sum(sum);
      if (lane == 0) t[b0 + i] -= sum;
    }
    for (int e = tid; e < nb * nb; e += blockDim.x) T[(e / nb) * 65 + e % nb] = LU[(long long)(b0 + e / nb) * ldq + b0 + e % nb];
    __syncthreads();
    if (wave == 0) {
      double y = lane < nb ? t[b0 + lane] : 0.0;
      for (int s = nb - 1; s >= 0; s--) {
        if (lane == s) y /= T[s * 65 + s];
        const double ys = __shfl(y, s);
        if (lane < s) y -= T[lane * 65 + s] * ys;
      }
      if (lane < nb) t[b0 + lane] = y;
    }
    __syncthreads();
  }
  if (tid == 0)
    for (int s = q - 1; s >= 0; s--) {
      const int r = (int)perm[2 * qmax + s];
      const double x = t[s];
      t[s] = t[r], t[r] = x;
    }
  __syncthreads();
}
__global__ void __launch_bounds__(256) k_st_x0_free(int n0, int cap0, int qmax, const double *__restrict__ K0lu,
                                                    const double *__restrict__ K0mat, const double *__restrict__ K0s, long long ldq,
                                                    const int *__restrict__ dyn0, const double *__restrict__ v0,
                                                    const double *__restrict__ beta0, double *__restrict__ x0,
                                                    double *__restrict__ eta0) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  if (K0s[3 * qmax] == 1.0) return;  // (uniform) the area holds the inverse: k_x0_rhs ... k_x0_out have done it
  const int c = dyn0[1], q = n0 + c, tid = threadIdx.x, nt = blockDim.x;
  double *b = sm, *y = sm + qmax, *t = y + qmax, *T = t + qmax;
  for (int i = tid; i < q; i += nt) {
    b[i] = i < n0 ? v0[i] : beta0[i - n0];
    t[i] = K0s[i] * b[i];
  }
  __syncthreads();
  x0_lu_solve(K0lu, ldq, K0s, qmax, q, t, T);
  for (int i = tid; i < q; i += nt) y[i] = K0s[i] * t[i];
  __syncthreads();
  for (int i = tid; i < q; i += nt) {  // one round of refinement against K0 itself (symmetric: column i read as row i)
    double s = b[i];
    for (int j = 0; j < q; j++) s -= K0mat[(long long)j * ldq + i] * y[j];
    t[i] = K0s[i] * s;
  }
  __syncthreads();
  x0_lu_solve(K0lu, ldq, K0s, qmax, q, t, T);
  for (int i = tid; i < n0 + cap0; i += nt) {
    const double s = i < q ? y[i] + K0s[i] * t[i] : 0.0;
    if (i < n0)
      x0[i] = -s;
    else
      eta0[i - n0] = -s;
  }
}
// last stage: multipliers of its equality rows = eta_K
__global__ void k_st_y_last(int e, const int *__restrict__ eq_rows, const double *__restrict__ eta, double *__restrict__ dy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < e) dy[eq_rows[i]] = eta[i];
}
__global__ void k_st_gather(int e, const int *__restrict__ rows, const double *__restrict__ src, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < e) out[i] = src[rows[i]];
}
__global__ void k_st_negate(int n, const double *__restrict__ s, double *__restrict__ dx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dx[i] = -s[i];
}
// d = s, d2 = s + a2
__global__ void k_st_copy_add(int n, const double *__restrict__ s, double *__restrict__ d, const double *__restrict__ a2,
                              double *__restrict__ d2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = s[i], d2[i] = s[i] + a2[i];
}
__global__ void k_st_copy(int n, const double *__restrict__ s, double *__restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = s[i];
}

// ---------------------------------------------------------------------------------------
// One system over several ranks (staged_plan.hpp).  The blocks of G_xx this rank has computed in its row strip of the
// work block G go into its slot of the second exchange buffer in LOWER orientation: a block of its own rows as it is,
// a block it computed for the partner's rows (rows = its own columns) transposed.  blockIdx.y = block.
struct PackRect {
  int r0, c0, rows, cols;  // where the block lies in G (work orientation) and its size there
  int transpose;           // the slot holds it transposed: cols x rows, leading dimension rows
  int pad;
  long long off;           // into this rank's slot
};
__global__ void __launch_bounds__(256) k_st_pack_rects(const PackRect *__restrict__ rects, const double *__restrict__ G, long long ldg,
                                                       double *__restrict__ slot) {
  __shared__ double t[32][33];
  const PackRect r = rects[blockIdx.y];
  double *dst = slot + r.off;
  if (!r.transpose) {
    for (int i = blockIdx.x; i < r.rows; i += gridDim.x) {
      const double *src = G + (long long)(r.r0 + i) * ldg + r.c0;
      for (int j = threadIdx.x; j < r.cols; j += blockDim.x) dst[(long long)i * r.cols + j] = src[j];
    }
    return;
  }
  // 32 x 32 tiles through LDS: rows of G are read, rows of the transposed block written
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int tr = (r.rows + 31) / 32, tc = (r.cols + 31) / 32;
  for (int tile = blockIdx.x; tile < tr * tc; tile += gridDim.x) {
    const int i0 = (tile / tc) * 32, j0 = (tile % tc) * 32;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + ty + 8 * u, j = j0 + tx;
      t[ty + 8 * u][tx] = (i < r.rows && j < r.cols) ? G[(long long)(r.r0 + i) * ldg + r.c0 + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = j0 + ty + 8 * u, i = i0 + tx;
      if (i < r.rows && j < r.cols) dst[(long long)j * r.rows + i] = t[tx][ty + 8 * u];
    }
    __syncthreads();
  }
}
// rows x cols block copy (the own row strip of V_k out of the transient full block)
__global__ void __launch_bounds__(256) k_st_copy2d(const double *__restrict__ src, long long lds_, double *__restrict__ dst, long long ldd, int rows,
                                                   int cols) {
  for (int i = blockIdx.x; i < rows; i += gridDim.x)
    for (int j = threadIdx.x; j < cols; j += blockDim.x) dst[(long long)i * ldd + j] = src[(long long)i * lds_ + j];
}
// y = add + the ranks' partial vectors in their order (x+ = F s + f over the column strips)
__global__ void k_st_sum_slots(int n, int nslots, const double *__restrict__ slots, long long stride, const double *__restrict__ add,
                               double *__restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = add ? add[i] : 0.0;
  for (int p = 0; p < nslots; p++) s += slots[(long long)p * stride + i];
  y[i] = s;
}
__global__ void k_st_zero(long long n, double *__restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = 0.0;
}
// ---------------------------------------------------------------------------------------
// Dense dynamics (hqpkkt_set_values_staged): the products with the dynamics rows of A that
// residuum() needs, all stages in one launch (blockIdx.y = stage)
struct DynDesc {
  long long oF;
  int ldf, np, nz, col0, row0, ncur;  // F block, its sizes, first column / dynamics row, states of the stage
};
// out2[row0 + li] = F_k[li][:] dx_k - dx_{k+1}[li]
// out1[c] = sum_li F_k[li][lc] dy[row0 + li] - dy[row of x_k's dynamics equation]   (c in stage k;
// the last stage has no F: np = 0)
// Both products of residuum() with the dense dynamics rows in ONE pass over the F blocks (two passes: 80 GB at the
// headline size, 14.5 ms): workgroup (bx, k) takes 256 columns of stage k's block, thread = column.  Down the rows it
// accumulates its column of A_dyn' dy; the row sums of A_dyn dx over the workgroup's 256 columns go, 64 rows at a time,
// through a wavefront sum and LDS into `part` (one value per row and column block); k_st_dyn_ax_finish adds the
// column blocks in their order and the -x_{k+1} of the dynamics rows.
__global__ void __launch_bounds__(256) k_st_dyn_both(const DynDesc *__restrict__ desc, const double *__restrict__ F,
                                                     const double *__restrict__ dx, const double *__restrict__ dy,
                                                     double *__restrict__ out1, double *__restrict__ part, int nblk_cols) {
  // wavefront w takes the rows w, w + 4, ... of the block; lane l the columns l, l + 64, l + 128, l + 192 of the
  // workgroup's 256: a row's sum over those columns is ONE wavefront sum (eight rows' sums side by side), a column's
  // sum over the rows meets the other three wavefronts' in LDS at the end
  __shared__ double cs[4][256];
  const DynDesc d = desc[blockIdx.y];
  const int ncols = d.np > 0 ? d.nz : d.ncur;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 256;
  if (c0 >= ncols) return;  // (uniform)
  bool in[4];
  double xj[4], s[4];
  const double *fc[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int lc = c0 + lane + 64 * g;
    in[g] = lc < ncols;
    xj[g] = (in[g] && lc < d.nz) ? dx[d.col0 + lc] : 0.0;
    fc[g] = F + d.oF + (in[g] ? lc : 0);
    s[g] = 0.0;
  }
  for (int li0 = wave; li0 < d.np; li0 += 32) {  // eight rows of this wavefront per trip: li0, li0 + 4, ...
    double v[8][4], p[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int li = li0 + 4 * u;
#pragma unroll
      for (int g = 0; g < 4; g++) v[u][g] = (in[g] && li < d.np) ? fc[g][(long long)li * d.ldf] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int li = li0 + 4 * u;
      const double yv = li < d.np ? dy[d.row0 + li] : 0.0;
      p[u] = 0.0;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        s[g] = fma(v[u][g], yv, s[g]);
        p[u] = fma(v[u][g], xj[g], p[u]);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int u = 0; u < 8; u++) p[u] += __shfl_xor(p[u], o);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (li0 + 4 * u < d.np) part[(long long)(d.row0 + li0 + 4 * u) * nblk_cols + blockIdx.x] = p[u];
    }
  }
#pragma unroll
  for (int g = 0; g < 4; g++) cs[wave][lane + 64 * g] = s[g];
  __syncthreads();
  const int lc = c0 + tid;
  if (lc < ncols) {
    double t = (cs[0][tid] + cs[1][tid]) + (cs[2][tid] + cs[3][tid]);
    // x_k is the state the previous stage's dynamics produce: -1.0 in that row
    if (blockIdx.y > 0 && lc < d.ncur) t -= dy[d.row0 - d.ncur + lc];
    out1[d.col0 + lc] = t;
  }
}
__global__ void k_st_dyn_ax_finish(const DynDesc *__restrict__ desc, const double *__restrict__ part, int nblk_cols,
                                   const double *__restrict__ dx, double *__restrict__ out2) {
  const DynDesc d = desc[blockIdx.y];
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= d.np) return;
  const int nb = (d.nz + 255) / 256;
  double s = 0.0;
  for (int b = 0; b < nb; b++) s += part[(long long)(d.row0 + li) * nblk_cols + b];
  out2[d.row0 + li] = s - dx[d.col0 + d.nz + li];
}

// The same two products when the F blocks are the LOCAL ones of a rank (Floc_k = [F_p | F_u], staged_plan.hpp): the rank
// adds what its state columns contribute; the control columns, the -x_{k+1} of the dynamics rows and the -dy of the
// rows that produce x_k are added once, by the rank that owns them (control columns: rank 0).  Both outputs start at
// zero and are summed over the ranks afterwards.
struct DynLoc {
  long long oF;
  int ldf, np, nz, col0, row0, ncur;  // as DynDesc (nz, ncur: of the whole stage)
  int c0, wd, m;                      // own state columns [c0, c0 + wd), controls of the stage
  int with_controls;                  // this rank adds the control columns' share
};
__global__ void __launch_bounds__(256) k_st_dynloc_ax(const DynLoc *__restrict__ desc, const double *__restrict__ F,
                                                      const double *__restrict__ dx, double *__restrict__ out2) {
  const DynLoc d = desc[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int nloc = d.wd + (d.with_controls ? d.m : 0);
  for (int li = blockIdx.x * 4 + (threadIdx.x >> 6); li < d.np; li += gridDim.x * 4) {
    const double *fr = F + d.oF + (long long)li * d.ldf;
    double s = 0.0;
    for (int j = lane; j < nloc; j += 64) s += fr[j] * dx[d.col0 + (j < d.wd ? d.c0 + j : d.ncur + (j - d.wd))];
    s = kktdev::wave_sum(s);
    // -x_{k+1}[li]: by the rank that owns row li of the next stage's states ... which only the host knows: rank 0 here
    if (lane == 0) out2[d.row0 + li] = s - (d.with_controls ? dx[d.col0 + d.nz + li] : 0.0);
  }
}
__global__ void __launch_bounds__(256) k_st_dynloc_aty(const DynLoc *__restrict__ desc, const double *__restrict__ F,
                                                       const double *__restrict__ dy, double *__restrict__ out1) {
  const DynLoc d = desc[blockIdx.y];
  const int nloc = d.wd + (d.with_controls && d.np > 0 ? d.m : 0);
  for (int lc = blockIdx.x * blockDim.x + threadIdx.x; lc < nloc; lc += gridDim.x * blockDim.x) {
    const int gc = lc < d.wd ? d.c0 + lc : d.ncur + (lc - d.wd);
    double s = 0.0;
    const double *fc = F + d.oF + lc;
    for (int li = 0; li < d.np; li++) s += fc[(long long)li * d.ldf] * dy[d.row0 + li];
    // x_k is the state the previous stage's dynamics produce: -1.0 in that row
    if (blockIdx.y > 0 && gc < d.ncur) s -= dy[d.row0 - d.ncur + gc];
    out1[d.col0 + gc] = s;
  }
}

}  // namespace stg
