"""The fp64 product with a second k segment (GemmArgs::K2, hqpkkt_debug_dgemm2): C = A'B - A2'B2 out of ONE launch of the
128 x 128 LDS-DMA kernels - the slabs of the second operand pair behind the zero-padded slabs of the first in the same
accumulators, a cut piece's slab range free to span the boundary.  This is the launch that forms V_k = F_x'W_x - Y'Rm
of a stage.  Criterion of test_large_dgemm_kernels_against_exact_products (tests/test_gpu_staged.py): 4096 sample
entries against exactly accumulated sums, |C_ij - exact| <= 1e-14 sum_k |a_ki b_kj|; and a mirrored result is exactly
symmetric, bit for bit."""
import pytest
import torch

from hqp_amd import ipmatrix

pytestmark = pytest.mark.gpu

# M = N, K1, K2 (all lower + mirror)
SHAPES = [
    (5000, 5000, 50),   # the C4 stage: 820 lower tiles of 313 + 4 slabs, cut form by a work table
    (5000, 5000, 1),
    (5000, 5000, 16),
    (5000, 5000, 64),
    (3000, 1000, 64),   # 300 lower tiles of 63 + 4 slabs: the fractional form, shares of 40 slabs - most pieces span the boundary
    (4097, 37, 50),     # 561 tiles of 3 + 4 slabs, K1 not a multiple of the slab, ragged edge of one row: plain rounds
    (3700, 300, 7),     # 435 tiles of 19 + 1 slabs: plain rounds
]


def _spanning_pieces(n, k1, k2):
    """Cut pieces of the launch's work table whose slab range holds slabs of both segments."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (n + 127) // 128
    tiles = tiles * (tiles + 1) // 2
    n1, n2 = (k1 + 15) // 16, (k2 + 15) // 16
    got = ipmatrix.sk_table(tiles, n1 + n2, 2 * cus)
    assert got is not None
    units = got[0].reshape(-1, 6)
    return int(((units[:, 0] >= 0) & (units[:, 4] > 1) & (units[:, 1] < n1) & (units[:, 2] > n1)).sum())


@pytest.mark.parametrize("n,k1,k2", SHAPES)
def test_two_segment_product_exact_and_symmetric(n, k1, k2):
    ms, err, asym = ipmatrix.bench_dgemm2(n, n, k1, k2, lower=True, mirror=True, reps=1)
    print(f"dgemm2 {n} x {n}, K1 {k1}, K2 {k2}: {ms:.3f} ms, err {err:.2e}, asymmetric entries {asym}")
    assert err <= 1e-14, (n, k1, k2, err)
    assert asym == 0, (n, k1, k2, asym)


def test_c4_shape_has_pieces_across_the_boundary():
    """... so that the first case above is one whose cut pieces span the segment boundary (the last piece of every cut
    tile: slabs of F_x'W_x and all of Y'Rm's)."""
    assert _spanning_pieces(5000, 5000, 50) > 0


def test_not_lower_and_not_mirrored():
    for (m, n, k1, k2, lower, mirror) in [(5000, 5050, 1000, 50, 0, 0), (5050, 5050, 500, 33, 1, 0)]:
        ms, err, asym = ipmatrix.bench_dgemm2(m, n, k1, k2, lower=bool(lower), mirror=bool(mirror), reps=1)  # (raises unless the status is 0)
        assert err <= 1e-14, (m, n, k1, k2, err)
