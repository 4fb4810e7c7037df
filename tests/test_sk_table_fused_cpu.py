"""The work table of the launch that forms V_k of a stage (F_x'W_x and - Y'Rm as two k segments of one product, host
code): its tiles have gemm_slabs(n+) + gemm_slabs(q) k-slabs, and every slab of every tile - of both segments - is
computed exactly once, whatever the shares; cut pieces may hold slabs of both."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

# states n, states of the next stage n+, order q of the control-sized matrix, grid
CASES = [(5000, 5000, 50, 512), (5000, 5000, 1, 512), (5000, 5000, 64, 512), (4096, 5000, 17, 512), (5000, 3000, 50, 512),
         (3600, 3600, 7, 512), (5000, 5000, 50, 208), (6000, 2000, 64, 608)]


def _slabs(k):
    return (k + 15) // 16


@pytest.mark.parametrize("n,np_,q,grid", CASES)
def test_every_slab_of_both_segments_once(n, np_, q, grid):
    T = (n + 127) // 128
    tiles = T * (T + 1) // 2
    n1, n2 = _slabs(np_), _slabs(q)
    nslab = n1 + n2
    # the launch rule sees a product of that depth: the cut form (a table) or whole rounds on 128 x 128 tiles
    form, ftiles, table, _, _ = ipmatrix.gemm_form(n, n, 16 * nslab, lower=True, mirror=True, cus=grid // 2, grid=grid)
    assert form in ("cut", "plain", "frac") and ftiles == tiles, (form, ftiles)
    got = ipmatrix.sk_table(tiles, nslab, grid)
    assert got is not None
    units = got[0]
    seen = np.zeros((tiles, nslab), dtype=int)
    spanning = 0
    for b in range(grid):
        for (t, s0, s1, slot0, pieces, j) in units[b]:
            if t < 0:
                break
            assert 0 <= s0 < s1 <= nslab
            seen[t, s0:s1] += 1
            spanning += pieces > 1 and s0 < n1 < s1
    assert (seen[:, :n1] == 1).all(), "a slab of the first segment missing or twice"
    assert (seen[:, n1:] == 1).all(), "a slab of the second segment missing or twice"
    if form == "cut" and got[1] > 0:
        assert spanning > 0  # (the last piece of a cut tile holds the end of the first segment and the second)
