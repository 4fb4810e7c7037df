"""The work lists of the cut forms of the STAGED engine's fp64 product (hqp_amd/csrc/sk_table.hpp, host code): whatever
shares a list gives the workgroups, every k-slab of every tile is computed exactly once, a tile's pieces park in
slots of their own in the order of their k ranges, and nobody's list is longer than the stride says.  The equal-share
and the fractional list are the schedules k_dgemm_tn_sk computed in the kernel until commit 4a7e31d: unit by unit what
its two loops gave every workgroup, in their order (the sums of a tile's pieces depend on nothing else)."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

CASES = [(1600, 313, 512), (820, 313, 512), (780, 313, 512), (321, 313, 512), (511, 40, 512), (513, 64, 512), (1000, 200, 512),
         (2000, 313, 512), (700, 100, 512), (330, 313, 512), (5000, 70, 512), (600, 33, 512), (257, 1000, 512), (150, 128, 208),
         (104, 313, 208), (1600, 313, 256)]
# tiles, k-slabs, grid: headline and stage shapes, odd grids (no half round), small ones
EQUAL_CASES = [(1600, 313, 512), (820, 313, 512), (780, 313, 512), (321, 313, 512), (513, 64, 512), (700, 100, 512), (600, 33, 512),
               (200, 313, 256), (104, 313, 208), (1600, 313, 511), (37, 40, 13), (45, 32, 16), (23, 64, 16), (16, 100, 16), (17, 16, 16),
               (7, 35, 12)]
FRAC_CASES = [(272, 125, 512), (300, 188, 512), (200, 313, 512), (160, 64, 512), (320, 313, 512), (7, 64, 16), (9, 70, 12), (10, 64, 13),
              (5, 200, 16)]
# (the unequal cases keep the ids they have always had)
ALL = ([pytest.param("unequal", *c, id="-".join(map(str, c))) for c in CASES] + [pytest.param("equal", *c, id="equal-" + "-".join(map(str, c))) for c in EQUAL_CASES] +
       [pytest.param("frac", *c, id="frac-" + "-".join(map(str, c))) for c in FRAC_CASES])


def swz(bid, nwg):
    """xcd_swizzle: blockIdx.x -> the workgroup's position"""
    q, r, x = nwg >> 3, nwg & 7, bid & 7
    return x * q + min(x, r) + (bid >> 3)


def split_plan(tiles, nslab, grid):
    """gemm_split_plan of 4a7e31d: (whole tiles, [(begin, count, split)])"""
    smax = max(1, min(16, nslab // 16))
    whole = tiles // grid * grid
    R, begin, ph = tiles - whole, whole, []
    while R > 0 and len(ph) < 2:
        s, r = min(smax, grid // R), R
        if s <= 1:
            s = 1
            if len(ph) == 0 and smax >= 2 and R > grid // 2 and grid % 2 == 0:
                s, r = 2, grid // 2
        ph.append((begin, r, s))
        begin += r
        R -= r
    return whole, ph


def kernel_equal(tiles, nslab, grid):
    """The rounds-and-phases loop of k_dgemm_tn_sk at 4a7e31d: per blockIdx.x its units (tile, s0, s1, pieces, j)."""
    whole, ph = split_plan(tiles, nslab, grid)
    n_units = whole + sum(c * s for _, c, s in ph)
    out = []
    for b in range(grid):
        v = swz(b, grid)
        u, mine = v, []
        while u < n_units:
            q, pbase, cnt, pieces = -1, 0, grid, 1
            if u < whole:
                mine.append((u, 0, nslab, 1, 0))
            else:
                rel, q = u - whole, 0
                while q + 1 < len(ph) and rel >= ph[q][1] * ph[q][2]:
                    rel -= ph[q][1] * ph[q][2]
                    pbase += ph[q][1] * ph[q][2]
                    q += 1
                cnt, pieces = ph[q][1], ph[q][2]
                ti, j, L = rel % cnt, rel // cnt, (nslab + pieces - 1) // pieces
                s0 = min(nslab, j * L)
                mine.append((ph[q][0] + ti, s0, min(nslab, s0 + L), pieces, j))
            nu = n_units
            if u + grid < whole:
                nu = u + grid
            else:
                base, qq = whole, 0
                if u >= whole:
                    base, qq = base + pbase + cnt * pieces, q + 1
                while qq < len(ph) and nu == n_units:
                    if v < ph[qq][1] * ph[qq][2]:
                        nu = base + v
                    base += ph[qq][1] * ph[qq][2]
                    qq += 1
            u = nu
        out.append(mine)
    # (parked pieces: the units of the cut phases.  gemm_split_plan_pieces of 4a7e31d also counted the units of a phase
    # that cuts nothing - split 1, as with the odd grids here -, which park nothing and take no slot)
    return out, sum(c * s for _, c, s in ph if s > 1)


def kernel_frac(tiles, nslab, grid):
    """The sk.frac loop of k_dgemm_tn_sk at 4a7e31d (gemm_split_plan_frac: per = ceil(tiles nslab / grid))."""
    U = tiles * nslab
    per = (U + grid - 1) // grid
    out = []
    for b in range(grid):
        v = swz(b, grid)
        lo = min(U, v * per)
        hi = min(U, lo + per)
        x, mine = lo, []
        while x < hi:
            t = x // nslab
            s0 = x - t * nslab
            s1 = min(nslab, s0 + (hi - x))
            w_first, w_last = (t * nslab) // per, ((t + 1) * nslab - 1) // per
            mine.append((t, s0, s1, w_last - w_first + 1, v - w_first))
            x += s1 - s0
        out.append(mine)
    return out


@pytest.mark.parametrize("tiles,nslab,grid", EQUAL_CASES)
def test_equal_list_is_the_kernel_loop(tiles, nslab, grid):
    want, pieces = kernel_equal(tiles, nslab, grid)
    units, got_pieces, _, _ = ipmatrix.sk_table(tiles, nslab, grid, kind="equal")
    got = [[(t, s0, s1, n, j) for (t, s0, s1, _, n, j) in units[b] if t >= 0] for b in range(grid)]
    assert got == want
    assert got_pieces == pieces  # (gemm_split_plan_pieces: what the handle's workspace is sized by)


@pytest.mark.parametrize("tiles,nslab,grid", FRAC_CASES)
def test_frac_list_is_the_kernel_loop(tiles, nslab, grid):
    want = kernel_frac(tiles, nslab, grid)
    units, pieces, _, _ = ipmatrix.sk_table(tiles, nslab, grid, kind="frac")
    got = [[(t, s0, s1, n, j) for (t, s0, s1, _, n, j) in units[b] if t >= 0] for b in range(grid)]
    assert got == want
    assert pieces <= 2 * grid  # (the bound the launch rule checks against the workspace)
    assert units.shape[1] <= 5 and max(sum(1 for u in row if u[0] >= 0 and u[4] > 1) for row in units) <= 2


def test_lists_refuse_k_slabs_beyond_16_bits():
    for kind in ipmatrix.SK_KINDS:
        assert ipmatrix.sk_table(600, 65535, 512, kind=kind) is not None
        assert ipmatrix.sk_table(600, 65536, 512, kind=kind) is None


@pytest.mark.parametrize("kind,tiles,nslab,grid", ALL)
def test_every_slab_of_every_tile_once(kind, tiles, nslab, grid):
    got = ipmatrix.sk_table(tiles, nslab, grid, kind=kind)
    assert got is not None
    units, pieces, wa, wb = got
    assert units.shape[0] == grid and wa >= wb >= 0
    cover = [[] for _ in range(tiles)]
    slots = {}
    for b in range(grid):
        ended = False
        for (t, s0, s1, slot0, np_, j) in units[b]:
            if t < 0:
                ended = True
                continue
            assert not ended, "a unit behind the end mark"
            assert 0 <= t < tiles and 0 <= s0 < s1 <= nslab and 0 <= j < np_
            cover[t].append((s0, s1, j))
            if np_ > 1:
                assert 0 <= slot0 and slot0 + np_ <= pieces
                assert slots.setdefault(t, (slot0, np_)) == (slot0, np_)
            else:
                assert (s0, s1) == (0, nslab)
        assert ended, "no end mark"
    used = np.zeros(pieces, dtype=int)
    for t in range(tiles):
        c = sorted(cover[t])
        at = 0
        for q, (s0, s1, j) in enumerate(c):
            assert s0 == at and j == q, (t, c)
            at = s1
        assert at == nslab, (t, c)
        if t in slots:
            assert slots[t][1] == len(c)
            used[slots[t][0]:slots[t][0] + slots[t][1]] += 1
        else:
            assert len(c) == 1
    assert (used == 1).all()
    if kind == "frac":
        assert pieces <= 2 * grid
    if kind == "equal":
        assert pieces == kernel_equal(tiles, nslab, grid)[1]
    if kind != "unequal":
        return
    # whole tiles first: the first workgroup of a CU (blockIdx < grid / 2) gets at least as many as the second
    work = np.array([[(u[2] - u[1]) for u in units[b] if u[0] >= 0] for b in range(grid)], dtype=object)
    tot = np.array([sum(w) for w in work])
    assert tot[:grid // 2].min() >= wa * nslab and tot[grid // 2:].min() >= wb * nslab
    assert tot.sum() == tiles * nslab


def test_headline_shapes_take_whole_tiles():
    # W of the headline (40 x 40 tiles): four whole tiles for the first workgroup of a CU, two and a quarter for the second;
    # G (820 lower tiles): two, and one and a quarter for 208 of the second ones
    u, pieces, wa, wb = ipmatrix.sk_table(1600, 313, 512)
    assert (wa, wb, pieces) == (4, 2, 256)
    u, pieces, wa, wb = ipmatrix.sk_table(820, 313, 512)
    assert (wa, wb, pieces) == (2, 1, 208)
