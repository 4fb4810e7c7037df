// Sizes the tree engine's kernels and its launch rule (tree_plan.hpp) share: LDS bytes of a launch, the limits of the
// instances.  Plain C++: the kernel headers include it under hipcc, tree_plan.hpp and the host tests under g++.
#pragma once
#include <cstddef>

#if defined(__HIP__) || defined(__HIPCC__)
#define HQP_HD __host__ __device__
#else
#define HQP_HD
#endif

namespace kktdev {

// ---- k_factor_blk (factor_blk.hip.h)
// leading dimension of the 16-row LDS images: = 16 mod 32 doubles, so that the four
// k-rows a wavefront reads with one ds_read_b64 fall into different halves of the banks
// (a compile-time constant of the two instantiations: 144 for blocks of up to 128 pivots, 208 up to 192 - the
// k-rows of an operand are immediate offsets of one address then)
HQP_HD inline int fb_ld_of(int p) { return p <= 128 ? 144 : 208; }
// an image takes 16 ld + 8 doubles (the skew of FBROW, factor_blk.hip.h)
HQP_HD inline int fb_img_of(int ld) { return 16 * ld + 8; }
HQP_HD inline size_t fb_lds_bytes(int p) {
  const int pp = ((p + 15) / 16) * 16, ld = fb_ld_of(p);
  // Op, Lb, Yb, Xq | Tb, Ld (two each), Gb | Ab, G2 | dvals, dinvs, cmaxf, flags (two each) | rm0 | dv | lp, pt (ints)
  return sizeof(double) * ((size_t)4 * fb_img_of(ld) + 5 * 272 + 512 + 96 + (size_t)pp + 2 * (size_t)pp + (size_t)pp + 16);
}

// ---- k_factor_diag_small (kernels.hip.h)
// LDS bytes of one front for the leading dimensions of a launch: ldp odd and >= the largest p,
// ldb >= the largest b of the fronts in the launch (a level of a narrow-band tree has
// fronts of 5..20 pivots, a quarter of the room the limits would need)
HQP_HD inline size_t fs_lds_bytes(bool front, int ldp, int ldb) {
  const size_t d = (size_t)ldp * ldp + 2 * (size_t)ldp + (front ? 2 * (size_t)ldb * ldp + (size_t)ldb * ldb : 0);
  return 8 * d + 8 * (size_t)ldp;
}

// ---- k_panel_solve (kernels.hip.h)
static const int PS_LD = 33;  // doubles per column of the RESULT slab in LDS (what the launch sizes its LDS by)

// ---- k_solve_top (solve_top.hip.h)
static const int ST_THREADS = 1024, ST_MAXFRONTS = 128, ST_MAXSPLIT = 1 << 15;  // fronts of one fused launch / of the split form
static const int ST_XS = 192, ST_CS = 256;  // words per front in the exchange arrays: solution (pivots), contribution (border rows)
// the two instances: <3, 11> fronts of up to 176 pivots and 192 border rows, <4, 10> up to 160 pivots and 256 border rows
static inline bool st_top_fits(int p, int b, int ns, int nu) { return p <= 16 * nu && b <= 64 * ns; }
static inline size_t st_top_lds_bytes(int maxp, int ns) {
  const size_t mlen = ((size_t)maxp * (maxp + 1) / 2 + 1) & ~(size_t)1;
  return sizeof(double) * (mlen + 8 * 64 * ns + 16 * 64 * ns);
}

}  // namespace kktdev
