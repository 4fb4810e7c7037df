"""The control-row segment of the fp64 product (k_dgemm_tn_sk<.., AUG>, GemmArgs::Au): one launch of C = A'B (M = K) whose
ragged last tile row also forms Cu = C[:, N - mu:]'B from the columns its last tile column writes, with the guarded thin
product behind it, on operands of the test's own through hqpkkt_debug_dgemm_ctrl_rows, entry by entry against numpy.

Criterion, as tests/test_gpu_dgemm_full.py (a): integer operands, here of magnitude <= 2^7, so that C (< 2^23) and
Cu = C_u'B (at most 264 products of at most 2^30) and every partial sum are integers below 2^53: the fp64 results are
exact whatever the order of summation or the cut in k, and both WHOLE buffers are compared bit for bit with what they
must hold.  One quiet-NaN pattern fills the rows of C at and beyond M (they are the rows >= K of Au as well: no result
may depend on them), its columns at and beyond N (mu odd: the 16-byte load of Au's last column reaches one of them),
the rows of Cu at and beyond mu, and the operands' rows behind K.  Afterwards every such element still holds the pattern.
And (b) for the base shape: uniform operands, |got - ref| <= 1e-14 |A|'|B| against a numpy.longdouble product.

Every shape runs twice.  Small forced grid (grid 2 for 3 x 3 tiles - ten units on two workgroups, at least four each, the
last tile column in their first two, the augmented tiles in the fourth and later: every augmented tile starts at least
one whole tile time after the last tile column is written; grid 1 for 2 x 2 tiles, one workgroup in program order):
the augmented tiles find the columns finished, fallbacks == 0.  Grid 64 >= tiles: every workgroup has one unit, the
augmented tiles start with the tiles they ask for, raise the flag, and the guarded product delivers Cu: fallbacks == 1."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

pytestmark = pytest.mark.gpu

CANARY = np.uint64(0x7FF8C0DE5EEDBEEF)
# M = K, mu, N, segment taken
CASES = {
    "base": (264, 50, 314, True),
    "mu1": (264, 1, 265, True),
    "mu64": (264, 64, 328, True),
    "exactly_full_row": (206, 50, 256, True),
    "too_many_rows": (208, 50, 258, False),
    "no_ragged_row": (256, 50, 306, False),
}


def _ints(rng, shape):
    return rng.integers(-2 ** 7, 2 ** 7, size=shape, endpoint=True).astype(np.float64)


def _uniform(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape)


def _operand(rng, k, w, col0, values):
    ld = col0 + w + 3
    ld += ld & 1
    buf = np.full((k + 17, ld), np.nan)
    blk = values(rng, (k, w))
    buf[:k, col0:col0 + w] = blk
    return buf, blk


def _run(M, mu, N, grid, values=_ints, seed=0):
    rng = np.random.default_rng([seed, M, mu, N])
    A, a = _operand(rng, M, M, 2, values)
    B, b = _operand(rng, M, N, 4, values)
    ldc = N + 5 + ((N + 5) & 1)
    Cb = np.empty((M + 3, ldc))
    Cb.view(np.uint64)[...] = CANARY
    Cu = np.empty((mu + 2, N + 2 + (N & 1)))
    Cu.view(np.uint64)[...] = CANARY
    taken, fallbacks, form, tiles = ipmatrix.dgemm_ctrl_rows(M, N, mu, A, B, Cb, Cu, grid=grid, a_col0=2, b_col0=4)
    return a, b, Cb, Cu, taken, fallbacks, form, tiles


def _check_exact(name, grid, a, b, Cb, Cu, M, mu, N):
    c = a.T @ b
    want_c = np.empty_like(Cb)
    want_c.view(np.uint64)[...] = CANARY
    want_c[:M, :N] = c
    want_u = np.empty_like(Cu)
    want_u.view(np.uint64)[...] = CANARY
    want_u[:mu, :N] = c[:, N - mu:].T @ b
    bad = np.argwhere(Cb.view(np.uint64) != want_c.view(np.uint64))
    assert bad.size == 0, (name, grid, "C", len(bad), bad[:5].tolist())
    bad = np.argwhere(Cu.view(np.uint64) != want_u.view(np.uint64))
    assert bad.size == 0, (name, grid, "Cu", len(bad), bad[:5].tolist())


@pytest.mark.parametrize("name", sorted(CASES))
def test_ready_path_on_a_small_grid(name):
    M, mu, N, want_taken = CASES[name]
    grid = 2 if (M + 127) // 128 >= 3 else 1
    a, b, Cb, Cu, taken, fallbacks, form, tiles = _run(M, mu, N, grid)
    assert form == "cut" and tiles == ((M + 127) // 128) * ((N + 127) // 128)
    assert taken == want_taken and fallbacks == 0, (name, taken, fallbacks)
    _check_exact(name, grid, a, b, Cb, Cu, M, mu, N)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fallback_delivers_the_rows_when_every_workgroup_has_one_unit(name):
    M, mu, N, want_taken = CASES[name]
    a, b, Cb, Cu, taken, fallbacks, form, tiles = _run(M, mu, N, 64)
    assert taken == want_taken and fallbacks == (1 if want_taken else 0), (name, taken, fallbacks)
    _check_exact(name, 64, a, b, Cb, Cu, M, mu, N)


def test_rounding_of_the_base_shape():
    M, mu, N, _ = CASES["base"]
    a, b, Cb, Cu, taken, fallbacks, _, _ = _run(M, mu, N, 2, values=_uniform, seed=1)
    assert taken and fallbacks == 0
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    c = al.T @ bl
    assert (np.abs(Cb[:M, :N] - c) <= 1e-14 * (np.abs(al).T @ np.abs(bl))).all()
    # (Cu is formed from the C the launch wrote: the exact product of that fp64 block with B is its reference)
    wu = Cb[:M, N - mu:N].astype(np.longdouble)
    assert (np.abs(Cu[:mu, :N] - wu.T @ bl) <= 1e-14 * (np.abs(wu).T @ np.abs(bl))).all()


def test_a_launch_without_the_segment_is_the_launch_it_always_was():
    """mu = 0: the hook launches the cut form without the segment - the list, the kernel and so the bits of
    hqpkkt_debug_dgemm_full with the cut form forced, on full-mantissa operands (pieces of k summed in the same order)."""
    M, N = 264, 314
    rng = np.random.default_rng(5)
    A, a = _operand(rng, M, M, 2, _uniform)
    B, b = _operand(rng, M, N, 4, _uniform)
    ldc = N + 6
    C1, C2, Cu = np.zeros((M + 3, ldc)), np.zeros((M + 3, ldc)), np.zeros((1, N + 2))
    taken, fallbacks, form, _ = ipmatrix.dgemm_ctrl_rows(M, N, 0, A, B, C1, Cu, a_col0=2, b_col0=4)
    assert not taken and fallbacks == 0 and form == "cut"
    assert ipmatrix.dgemm_full(M, N, M, C2, 0, 0, A=A, a_col0=2, B=B, b_col0=4, no_ks=True, force_split=True)[0] == "cut"
    assert np.array_equal(C1.view(np.uint64), C2.view(np.uint64))
