"""GPU tests of the STAGED solve's dense vector products, one launch at a time on chosen operands: k_st_gemv_rows,
k_st_gemv_wide, k_st_gemv_cols with k_st_cols_finish, the triangle form k_st_symv_tiles with k_st_symv_finish and the
many-products-per-launch pair k_st_symv_*_batch (staged.hip.h), through the hooks hqpkkt_debug_gemv_dense,
hqpkkt_debug_symv and hqpkkt_debug_symv_batch, which launch by the functions the engine's sweeps call.  A whole solve ends in
iterative refinement, which forgives a product that is slightly wrong; these tests do not.

Two kinds of operands for every case.
  ints:  entries of the matrices and vectors from -8 .. 8, scale from +-1, +-2: every partial sum is an integer that a
         double holds exactly, so every order of summation gives the same bits, and the result must EQUAL the int64 product
         of numpy.  A missing, doubled or misplaced term cannot hide.
  reals: uniform(-1, 1) against a longdouble product.  Row i: |y_i - ref_i| <= (T_i + 4) 2^-53 |scale| (|add_i| + sum |a||x|)
         with T_i products in the row - the bound of a dot product of T terms in any order, with or without fused
         multiply-adds (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), and four more roundings for
         add and scale.  Derived, not measured.  A second launch gives the same bits.
Whatever a result may not depend on is NaN: the columns of a row outside the block, the rows behind it, the columns of the
carried rows' block behind its live count, x behind its length and, for the triangle form, every element of V strictly
above the diagonal - the kernel masks those instead of multiplying, so this is the test that it reads one triangle.  The
hooks put NaN into the partial sums' scratch and marks behind every result: a partial sum that is read but never written
shows as NaN in y, a write past a result as HQPKKT_E_INTERN.

The shapes are the smallest that reach each branch: 16-byte against scalar loads (even / odd leading dimension, odd first
column), odd tails, the unrolled loops with their remainders, one and several workgroups, the chunked columns form with
its finish, diagonal tiles, one to three column tiles of the triangle form and 30 row tiles (the finish's 8-deep loop).
More than 32 column tiles of the triangle form (N >= 16 385, the second round of the finish's loop over the row parts) is
not tested: the matrix alone is 2 GB.

Largest err / bound seen on one MI355X, reals: rows form 0.21, wide form 0.16, columns form 0.19, triangle form
0.068, batch 0.0086 (each case prints its own)."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

pytestmark = pytest.mark.gpu

NAN = np.nan
KINDS = ("ints", "reals")
U = 2.0 ** -53


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _vals(rng, kind, *shape):
    if kind == "ints":
        return rng.integers(-8, 9, shape).astype(np.float64)
    return rng.uniform(-1.0, 1.0, shape)


def _scale(rng, kind, sign):
    """ints: one of +-1, +-2 (sign 0: positive); reals: +-1, so that |scale| = 1 in the bound"""
    s = -1.0 if sign else 1.0
    return s * float(rng.choice([1.0, 2.0])) if kind == "ints" else s


def _block(vals, ld, col0, live_cols=None):
    """A buffer of one row more than vals and ld columns, NaN but for vals at column col0 (of which the columns behind
    live_cols are NaN too)."""
    r, c = vals.shape
    buf = np.full((r + 1, ld), NAN)
    buf[:r, col0: col0 + c] = vals
    if live_cols is not None:
        buf[:r, col0 + live_cols: col0 + c] = NAN
    return buf


def _tail(v, extra=5):
    return np.concatenate([v, np.full(extra, NAN)])


def _ld(width, col0, how):
    even = (width + col0 + 1) // 2 * 2
    return {"even": even, "odd": even + 1}[how]


def _verify(kind, label, y, terms, add, scale, after_scale=False):
    """y against scale (add + sum of a x over the terms (a, x)) - after_scale: add + scale sum, the columns form.  ints:
    equal; reals: the bound of the module's docstring.  Returns err / bound (reals)."""
    assert not np.isnan(y).any(), label
    n = len(y)
    if kind == "ints":
        s = np.zeros(n, dtype=np.int64)
        for a, x in terms:
            s += a.astype(np.int64) @ x.astype(np.int64)
        a0 = np.zeros(n, dtype=np.int64) if add is None else add.astype(np.int64)
        ref = a0 + int(scale) * s if after_scale else int(scale) * (a0 + s)
        assert np.array_equal(y, ref.astype(np.float64)), (label, np.flatnonzero(y != ref)[:8])
        return 0.0
    s, mag, T = np.zeros(n, dtype=np.longdouble), np.zeros(n), 0
    for a, x in terms:
        s += a.astype(np.longdouble) @ x.astype(np.longdouble)
        mag += np.abs(a) @ np.abs(x)
        T += a.shape[1]
    a0 = np.zeros(n) if add is None else add
    ref = a0 + np.longdouble(scale) * s if after_scale else np.longdouble(scale) * (a0 + s)
    bound = (T + 4) * U * abs(scale) * (np.abs(a0) + mag)
    err = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{label}: largest err / bound {ratio:.3g}")
    assert (err <= bound).all(), (label, ratio)
    return ratio


# ---- rows form and wide form: y (M) = scale (add + A x + A2 x2)

ROWS = [(1, 1), (3, 2), (5, 127), (4, 128), (7, 129), (6, 511), (6, 513), (9, 1030), (8, 66)]
WIDE = [(1, 1), (2, 511), (3, 2047), (3, 2048), (2, 2049), (4, 5003)]
LAYOUTS = [("even", 0), ("odd", 0), ("even", 1)]


def _rows_case(kind, form, M, N, how, col0, full, n2=None):
    """full: add, scale < 0 (and, with n2, the carried rows' block of 72 stored columns, odd ld2, n2 of them live)"""
    rng = _rng(11, form == "wide", M, N, how == "odd", col0, full, 0 if n2 is None else n2 + 1, kind == "ints")
    a, x = _vals(rng, kind, M, N), _vals(rng, kind, N)
    add = _vals(rng, kind, M) if full else None
    scale = _scale(rng, kind, full)
    ld = _ld(N, col0, how)
    kw, terms = {}, [(a, x)]
    if n2 is not None:
        a2, x2 = _vals(rng, kind, M, 72), _vals(rng, kind, n2)
        kw = dict(A2=_block(a2, 73, 0, live_cols=n2), n2=n2, x2=_tail(x2))
        terms.append((a2[:, :n2], x2))
    A = _block(a, ld, col0)
    args = dict(col0=col0, add=add, scale=scale, **kw)
    y, _, chunks, vec16 = ipmatrix.gemv_dense(form, A, M, N, _tail(x), **args)
    label = f"{form} {M}x{N} ld {ld} col0 {col0} n2 {n2} {kind}"
    # the rows whose first element is 16-byte aligned take the 16-byte loads (the device buffer itself is aligned)
    want16 = sum((col0 + i * ld) % 2 == 0 for i in range(M))
    print(f"{label}: 16-byte rows {vec16} of {M}")
    assert chunks == 1 and vec16 == want16
    ratio = _verify(kind, label, y, terms, add, scale)
    y_again = ipmatrix.gemv_dense(form, A, M, N, _tail(x), **args)[0]
    assert np.array_equal(y, y_again)  # run to run
    return ratio


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("how,col0", LAYOUTS)
@pytest.mark.parametrize("M,N", ROWS)
def test_rows_form(M, N, how, col0, full, kind):
    """Odd tails, one 4-deep round of 256 pairs plus remainder (511, 513), two rounds (1030), a partly filled and a full
    last workgroup of four rows (M = 5, 8); even ld with col0 0: every row by 16-byte loads, odd ld: every other row,
    col0 1 with an even ld: none."""
    _rows_case(kind, "rows", M, N, how, col0, full)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n2", [0, 1, 64, 70])
@pytest.mark.parametrize("M,N,how", [(5, 127, "even"), (8, 129, "odd")])
def test_rows_form_carried_rows(M, N, how, n2, kind):
    """The second block with its live-column count on the device: none, one, one per lane, more than a wavefront; the
    columns behind the count are NaN."""
    _rows_case(kind, "rows", M, N, how, 0, True, n2=n2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("how,col0", LAYOUTS)
@pytest.mark.parametrize("M,N", WIDE)
def test_wide_form(M, N, how, col0, full, kind):
    """One workgroup per row: a 4-deep round of 1024 pairs on either side (2047, 2048, 2049), two rounds plus remainder and
    an odd tail (5003)."""
    _rows_case(kind, "wide", M, N, how, col0, full)


# ---- columns form: y (N) = add + alpha A'x over K rows, y2 = y + add2

COLS = [(1, 1, 1), (3, 2, 1), (7, 513, 1), (8, 512, 1), (13, 1025, 1), (130, 70, 64), (581, 131, 64), (581, 131, 4), (64, 30, 64)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("how,col0", LAYOUTS)
@pytest.mark.parametrize("K,N,part_chunks", COLS)
def test_columns_form(K, N, part_chunks, how, col0, full, kind):
    """The 8-, 4- and 1-row loops with N on both sides of a workgroup's 512 columns, a last column alone (odd N), one
    chunk written directly, 2 chunks of 65 rows, 9 chunks (the finish's 8-deep loop plus one), chunks capped by the plan's
    count.  full: add, alpha < 0 and the second result y2 = y + add2."""
    rng = _rng(13, K, N, part_chunks, how == "odd", col0, full, kind == "ints")
    a, x = _vals(rng, kind, K, N), _vals(rng, kind, K)
    add, add2 = (_vals(rng, kind, N), _vals(rng, kind, N)) if full else (None, None)
    alpha = _scale(rng, kind, full)
    ld = _ld(N, col0, how)
    A = _block(a, ld, col0)
    args = dict(col0=col0, add=add, scale=alpha, add2=add2, part_chunks=part_chunks)
    y, y2, chunks, vec16 = ipmatrix.gemv_dense("cols", A, K, N, _tail(x), **args)
    label = f"cols {K}x{N} ld {ld} col0 {col0} part_chunks {part_chunks} {kind}"
    print(f"{label}: chunks {chunks} 16-byte loads {vec16}")
    assert chunks == max(1, min(part_chunks, K // 64))
    assert vec16 == (ld % 2 == 0 and col0 % 2 == 0)
    _verify(kind, label, y, [(a.T, x)], add, alpha, after_scale=True)
    if full:
        assert np.array_equal(y2, y + add2)  # (one IEEE addition of the value that went to y)
    else:
        assert y2 is None
    again = ipmatrix.gemv_dense("cols", A, K, N, _tail(x), **args)
    assert np.array_equal(y, again[0]) and (not full or np.array_equal(y2, again[1]))


# ---- triangle form: y (N) = scale (add + V x + A2 x2), V symmetric, only its lower triangle given

SYMV_N = [1, 5, 63, 64, 65, 127, 511, 512, 513, 577, 1025, 1090, 1857]


def _sym_operands(rng, kind, N, ld, col0):
    """(lower triangle L, the full symmetric matrix, V's buffer with NaN strictly above the diagonal and all around)"""
    L = np.tril(_vals(rng, kind, N, N))
    full = L + L.T - np.diag(np.diag(L))
    V = _block(np.where(np.tri(N, dtype=bool), L, NAN), ld, col0)
    return full, V


def _symv_item(kind, N, how, full_args, n2, key):
    """One product's operands: (keywords of ipmatrix.symv, terms of the reference, add, scale, the full matrix)"""
    rng = _rng(17, N, how == "even+6", full_args, 0 if n2 is None else n2 + 1, kind == "ints", key)
    col0 = 2 if how == "even+6" else 0
    ld = (N + 1) // 2 * 2 + (6 if how == "even+6" else 0)
    S, V = _sym_operands(rng, kind, N, ld, col0)
    x = _vals(rng, kind, N)
    add = _vals(rng, kind, N) if full_args else None
    scale = _scale(rng, kind, full_args)
    kw, terms = dict(V=V, N=N, x=_tail(x), col0=col0, add=add, scale=scale), [(S, x)]
    if n2 is not None:
        a2, x2 = _vals(rng, kind, N, 72), _vals(rng, kind, n2)
        kw.update(A2=_block(a2, 73, 0, live_cols=n2), n2=n2, x2=_tail(x2))
        terms.append((a2[:, :n2], x2))
    return kw, terms, add, scale, S


def _symv_case(kind, N, how, full_args, n2=None):
    kw, terms, add, scale, S = _symv_item(kind, N, how, full_args, n2, 0)
    args = dict(kw)
    V, x = args.pop("V"), args.pop("x")
    args.pop("N")
    y, tiles = ipmatrix.symv(V, N, x, **args)
    label = f"symv {N} ld {V.shape[1]} col0 {args['col0']} n2 {n2} {kind}"
    assert tiles == sum(bi // 8 + 1 for bi in range((N + 63) // 64))
    _verify(kind, label, y, terms, add, scale)
    assert np.array_equal(y, ipmatrix.symv(V, N, x, **args)[0])  # run to run
    # the rows form on the same matrix stored in full: the same reference and bound; the two within the sum of their bounds
    ldr = _ld(N, 0, "even")
    yr = ipmatrix.gemv_dense("rows", _block(S, ldr, 0), N, N, x, **dict(args, col0=0))[0]
    _verify(kind, label + " (rows form)", yr, terms, add, scale)
    if kind == "ints":
        assert np.array_equal(y, yr)
    else:
        mag = sum(np.abs(a) @ np.abs(v) for a, v in terms) + (0.0 if add is None else np.abs(add))
        assert (np.abs(y - yr) <= 2 * (sum(a.shape[1] for a, _ in terms) + 4) * U * abs(scale) * mag).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how,full_args", [("even", False), ("even+6", True)])
@pytest.mark.parametrize("N", SYMV_N)
def test_triangle_form(N, how, full_args, kind):
    """One row tile and a partial one, the diagonal inside the first and the second tile of 512 columns, one to three
    column tiles (the correction loops of the tile number's square root), 30 row tiles with an odd N (1857: the finish's
    8-deep loop over the mirrored partials); ld = N rounded up to even at column 0, and that + 6 from column 2 with add,
    scale < 0 and carried rows.  Every element above the diagonal is NaN."""
    _symv_case(kind, N, how, full_args, n2=70 if full_args else None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n2", [0, 1, 64, 70])
@pytest.mark.parametrize("N", [65, 577])
def test_triangle_form_carried_rows(N, n2, kind):
    _symv_case(kind, N, "even", True, n2=n2)


# ---- many products per launch

BATCH_N = (70, 513, 130, 1025)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grid", [(0, 0), (3, 2)])
@pytest.mark.parametrize("direction", ["x_relative", "y_relative"])
def test_triangle_form_batch(direction, grid, kind):
    """Four products of different orders in one launch pair, as the solve uses it before the backward sweep (x relative to
    a base vector, y per item) and behind the forward sweep (y relative, with add, carried rows and their live counts, one
    of them 0); one workgroup per tile / finishing block as the engine launches, and 3 / 2 workgroups that stride over the
    tiles / blocks of several items.  Bit-equal to hqpkkt_debug_symv item by item, and to the reference as there."""
    yrel = direction == "y_relative"
    items, refs = [], []
    for i, N in enumerate(BATCH_N):
        kw, terms, add, scale, _S = _symv_item(kind, N, "even+6" if i % 2 else "even", yrel, ((70, 0, 1, 64)[i] if yrel else None), 1 + i)
        items.append(kw)
        refs.append((terms, add, scale))
    offs = np.concatenate([[3], 3 + np.cumsum([n + 7 for n in BATCH_N])])  # (odd offsets, gaps between the items)
    xbase = ybase = None
    batch_items = [dict(it) for it in items]
    if yrel:
        ybase = np.full(int(offs[-1]), 777.0)
        for it, o in zip(batch_items, offs):
            it["yoff"] = int(o)
    else:
        xbase = np.full(int(offs[-1]), NAN)
        for it, o, N in zip(batch_items, offs, BATCH_N):
            xbase[o: o + N] = it.pop("x")[:N]
            it["xoff"] = int(o)
    ys, tiles = ipmatrix.symv_batch(batch_items, xbase=xbase, ybase=ybase, grid_tiles=grid[0], grid_fins=grid[1])
    assert tiles == sum(sum(bi // 8 + 1 for bi in range((N + 63) // 64)) for N in BATCH_N)
    for i, (it, (terms, add, scale), N) in enumerate(zip(items, refs, BATCH_N)):
        label = f"batch {direction} grid {grid} item {i} order {N} {kind}"
        _verify(kind, label, ys[i], terms, add, scale)
        one = dict(it)
        V, x = one.pop("V"), one.pop("x")
        one.pop("N")
        assert np.array_equal(ys[i], ipmatrix.symv(V, N, x, **one)[0]), label
    if yrel:  # nothing written between the items
        keep = np.ones(len(ybase), dtype=bool)
        for o, N in zip(offs, BATCH_N):
            keep[o: o + N] = False
        assert (ybase[keep] == 777.0).all()
