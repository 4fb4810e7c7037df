"""The thin-K shapes the wide rows of C bring to the STAGED engine's fp64 product (st_add_h_wide: G += S'S in place over
the lower tiles, depth = the number of wide rows of a stage): one launch per shape through hqpkkt_debug_dgemm_full - the
engine's launch rule and launch code - on operands laid out as the engine's (both operands the same K rows of up8(M)
doubles, 16-byte aligned), the whole C buffer compared on the host.

K in {1, 15, 16, 17, 33} (around the 16-row k-slab), M = N in {73, 154, 300} (narrower than a tile and odd, two tiles,
three), lower with and without the mirror image, beta = 1 with Cin in place.
  exact     integer operands of magnitude <= 2^15, Cin integers below 2^40: every partial sum is an integer below 2^53, the
            result is exact whatever the order of summation, and the buffer must hold it bit for bit;
  rounding  full-mantissa operands against a numpy.longdouble product: |C - ref| <= 1e-14 sum |a||b| for every entry, the
            entry of Cin that beta = 1 adds counted as one more term of the sum (an image above the diagonal: its source's
            terms, Cin[j][i] - nothing above the diagonal is read);
  canaries  one quiet-NaN pattern fills every element outside the block and, without the mirror, strictly above its
            diagonal: afterwards it is still there; the operands carry NaN in 16 rows behind row K and in the columns
            between M and the leading dimension, and no result may depend on them."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

pytestmark = pytest.mark.gpu

CANARY = np.uint64(0x7FF8C0DE5EEDBEEF)  # a quiet NaN no arithmetic produces
R0, C0 = 3, 4


def _run(M, K, mirror, values, cin_values, seed):
    rng = np.random.default_rng([seed, M, K, mirror])
    ld = (M + 7) // 8 * 8
    S = np.full((K + 17, ld), np.nan)
    s = values(rng, (K, M))
    S[:K, :M] = s
    cin = cin_values(rng, (M, M))
    ldc = (C0 + M + 4) // 2 * 2
    Cb = np.empty((R0 + M + 2, ldc))
    Cb.view(np.uint64)[...] = CANARY
    low = np.tril(np.ones((M, M), bool))
    blk = Cb[R0:R0 + M, C0:C0 + M]
    blk[low] = cin[low]  # in place: what the product may not read stays a canary
    want = Cb.copy()
    ran = ipmatrix.dgemm_full(M, M, K, Cb, R0, C0, A=S, B=S.copy(), alpha=1.0, beta=1.0, cin_is_c=True, lower=True, mirror=bool(mirror))
    return Cb, want, s, cin, low, ran


def _ints(rng, shape):
    return rng.integers(-2 ** 15, 2 ** 15, size=shape, endpoint=True).astype(np.float64)


def _big_ints(rng, shape):
    return rng.integers(-2 ** 40 + 1, 2 ** 40, size=shape).astype(np.float64)


def _uniform(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape)


@pytest.mark.parametrize("mirror", [0, 1])
@pytest.mark.parametrize("M", [73, 154, 300])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 33])
def test_thin_k_in_place_lower(K, M, mirror):
    # ---- exact
    got, want, s, cin, low, ran = _run(M, K, mirror, _ints, _big_ints, 0)
    print("M = N = %d K = %d mirror %d: form %s, %d tiles, LDS-DMA %d" % (M, K, mirror, ran[0], ran[1], ran[3]))
    ref = s.T @ s + cin
    wb = want[R0:R0 + M, C0:C0 + M]
    wb[low] = ref[low]
    if mirror:
        wb[~low] = ref.T[~low]
    g, w = got.view(np.uint64), want.view(np.uint64)
    guard = w == CANARY
    assert not (guard & (g != CANARY)).any(), ("written outside", np.argwhere(guard & (g != CANARY))[:8].tolist())
    assert not (~guard & (g == CANARY)).any(), ("not written", np.argwhere(~guard & (g == CANARY))[:8].tolist())
    assert np.array_equal(g, w), ("wrong entries", np.argwhere(g != w)[:8].tolist())
    # ---- full-mantissa operands
    got, want, s, cin, low, _ = _run(M, K, mirror, _uniform, _uniform, 1)
    g, w = got.view(np.uint64), want.view(np.uint64)
    guard = w == CANARY
    guard[R0:R0 + M, C0:C0 + M] &= ~low if not mirror else False
    assert np.array_equal(g[guard], w[guard])
    blk = got[R0:R0 + M, C0:C0 + M]
    ref = s.astype(np.longdouble).T @ s.astype(np.longdouble) + cin
    bound = 1e-14 * (np.abs(s).T @ np.abs(s) + np.abs(cin))
    sel = np.ones((M, M), bool) if mirror else low
    # an image above the diagonal is the sum of its source's terms: s_j s_i + cin[j][i]; cin[i][j] is never read
    full, bound = np.where(low, ref, ref.T), np.where(low, bound, bound.T)
    assert not np.isnan(blk[sel]).any()
    err = np.abs(blk.astype(np.longdouble) - full)
    assert (err[sel] <= bound[sel]).all(), float((err[sel] / bound[sel]).max())
    if mirror:
        assert np.array_equal(blk, blk.T)
