"""The work list and tile order of a launch with the control-row segment (gemm_ctrl_rows_order, sk_table.hpp; host code):
tiles + 1 logical tiles - the corner tile twice - in the list the chooser gives that count, with
  - the tiles of the last tile column at the START of their workgroups' lists (with fewer of them than workgroups: the
    first unit),
  - the augmented tiles of the last tile row at the END of theirs (the last unit),
  - every tile and every k-slab covered exactly once, the corner tile once in each form.
The headline's W (40 x 40 tiles of 313 k-slabs; G_xx's launch has 317, the depth of both of its segments) on 512
workgroups, and two small grids, on which a workgroup holds several tiles of a kind."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

CASES = [(40, 40, 313, 512), (40, 40, 317, 512), (3, 3, 17, 2), (2, 2, 13, 1), (33, 33, 257, 512), (5, 7, 40, 6)]


def _lists(units):
    return [[tuple(u) for u in row if u[0] >= 0] for row in units]


@pytest.mark.parametrize("tm,tn,nslab,grid", CASES)
def test_order_and_cover(tm, tn, nslab, grid):
    got = ipmatrix.sk_ctrl_rows(tm, tn, nslab, grid)
    assert got is not None
    units, tmap, pieces = got
    T = tm * tn + 1
    assert len(tmap) == T
    aug = tmap < 0
    row, col = (tmap >> 16) & 0x7FFF, tmap & 0xFFFF
    last_col = ~aug & (col == tn - 1)
    assert aug.sum() == tn and (row[aug] == tm - 1).all() and sorted(col[aug]) == list(range(tn))
    assert last_col.sum() == tm and sorted(row[last_col]) == list(range(tm))
    # every tile once, the corner in both forms
    count = np.zeros((tm, tn), dtype=int)
    np.add.at(count, (row, col), 1)
    want = np.ones((tm, tn), dtype=int)
    want[tm - 1, tn - 1] = 2
    assert (count == want).all()
    # every k-slab of every logical tile once, pieces in the order of k
    seen = np.zeros((T, nslab), dtype=int)
    lists = _lists(units)
    for lst in lists:
        for (t, s0, s1, slot0, npc, j) in lst:
            assert 0 <= s0 < s1 <= nslab and 0 <= j < npc
            seen[t, s0:s1] += 1
    assert (seen == 1).all()
    # the order inside every workgroup's list
    few = tm <= grid and tn <= grid
    for lst in lists:
        kinds = [1 if last_col[t] else 2 if aug[t] else 0 for (t, *_rest) in lst]
        n1, n2 = kinds.count(1), kinds.count(2)
        assert kinds[:n1] == [1] * n1, kinds
        assert kinds[len(kinds) - n2:] == [2] * n2, kinds
        if few and grid >= 512:
            assert n1 <= 1 and n2 <= 1


def test_the_headline_keeps_its_shares():
    """Nothing else about the list changes: 1601 logical tiles take the unequal shares 1600 take - whole tiles first, the
    remainder cut - and the augmented tiles are units of the cut remainder."""
    base = ipmatrix.sk_table(1600, 313, 512)
    got = ipmatrix.sk_table(1601, 313, 512)
    assert base is not None and got is not None and (base[2], base[3]) == (got[2], got[3])
    units, tmap, pieces = ipmatrix.sk_ctrl_rows(40, 40, 313, 512)
    assert np.array_equal(units, got[0]) and pieces == got[1]
