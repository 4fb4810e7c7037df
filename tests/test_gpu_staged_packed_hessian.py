"""GPU tests of the dense stage Hessians stored as packed lower tiles (hqpkkt_set_packed_hessians;
hqp_amd/csrc/staged_hess_packed.hip.h) against the unpacked dense form of the same library: the store of every hand-over,
factor and step bit for bit, the product Q x against sums accumulated exactly on the host, residual and solve, the
interior-point loop, and the time of the product.

Shapes at the edges of the 128-wide tile: stage orders 313 (the first of three tile rows that packs; odd, a ragged last tile
of 57 rows), 384 (whole tiles), 402 with 17 controls (the control rows [385, 402) cross the tile edge at 384), and three
stages of orders 313, 311, 320 of which the middle one keeps its dense block."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import packed_hessian_cases as P
from common import new_d
from dense_hessian_cases import kkt_row_bound, padded, up8
from hqp_amd import ipmatrix, problems

pytestmark = pytest.mark.gpu

H = problems.with_dense_hessian
CASES = {
    "order_313": lambda: H(problems.sparse_docp(2, 310, 3, band=5, seed=31, low_rank=False)),
    "order_384": lambda: H(problems.sparse_docp(2, 380, 4, band=5, seed=32, low_rank=False)),
    "order_402_17_controls": lambda: H(problems.sparse_docp(2, 385, 17, band=5, seed=33, low_rank=False)),
    "middle_stage_unpacked": lambda: H(problems.sparse_docp(2, [310, 310, 320], [3, 1], band=5, seed=34, low_rank=False)),
}
PACKED = {"order_313": [1, 1, 0], "order_384": [1, 1, 1], "order_402_17_controls": [1, 1, 0], "middle_stage_unpacked": [1, 0, 1]}
# the dynamics forms the dense-Hessian cases run under, and the dense hand-over of the dynamics
FORMS = {"dense": {}, "sparse": dict(a_sparse=True, dense_columns=8), "profile": dict(a_profile=True), "packed_panels": dict(a_profile=True, a_packed=True)}


@functools.lru_cache(maxsize=None)
def _prog(case):
    return CASES[case]()


@functools.lru_cache(maxsize=None)
def _wide():
    """order_402_17_controls with wide rows of C over states and controls (hqpkkt_set_dense_rows)."""
    return H(problems.with_wide_rows(_prog("order_402_17_controls"), [(0, 300, True), (1, 200, True), (2, 120, False)] * 3, seed=35))


def _pair(**opts):
    return ipmatrix.IpLQDOCP(q_dense=True, q_packed=True, **opts), ipmatrix.IpLQDOCP(q_dense=True, **opts)


def _init(M, prog, how):
    if how == "csr":
        M.init(prog)
    else:
        M.init_dense(problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True))
    return M


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _poisoned(blocks, ld_extra=3):
    """The blocks as a caller may hand them over: NaN in the strict lower triangle and in the columns behind the block."""
    out = []
    for B in blocks:
        G = np.full((B.shape[0], B.shape[0] + ld_extra), np.nan)
        iu = np.triu_indices(B.shape[0])
        G[iu] = B[iu]
        out.append(G)
    return out


def _sym(rng, nz):
    U = rng.standard_normal((nz, nz)) * 10.0 ** rng.uniform(-3, 3, (nz, nz))
    return np.triu(U) + np.triu(U, 1).T


def _block_docp(nz, blocks, seed=1):
    """A dense hand-over of K = 2 stages with Q_k of the given orders (stage k < 2: order - 1 states and one control)."""
    nx, nu = [nz[0] - 1, nz[1] - 1, nz[2]], [1, 1]
    rng = np.random.default_rng(seed)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    F = [0.1 * rng.uniform(-1, 1, (nx[k + 1], nx[k] + nu[k])) for k in range(2)]
    return problems.DenseDocp(nx, nu, empty(sum(nz)), empty(0), empty(0), F, 0, 0, Qd=blocks)


BLOCK_ORDERS = [(313, 384, 220), (402, 311, 320), (256, 129, 640)]


def test_layout_on_the_device_is_the_rule():
    for case, want in PACKED.items():
        M = _init(ipmatrix.IpLQDOCP(q_dense=True, q_packed=True), _prog(case), "csr")
        assert [int(t > 0) for t in M.hessian_packing()[:, 0]] == want, case


@pytest.mark.parametrize("nz", BLOCK_ORDERS)
@pytest.mark.parametrize("how", ["host", "device", "staging"])
def test_store_of_the_dense_hand_over(nz, how):
    """stage_hessian(k) of the packed handle - the unpacked view - is bit for bit that of the unpacked dense handle and the
    symmetrised block itself, with the caller's lower triangle and the columns behind nz poisoned with NaN: host pointers,
    device pointers, and host blocks out of the hqpkkt_stage_staging buffers.  A second hand-over of other values leaves
    nothing of the first."""
    rng = np.random.default_rng(sum(nz))
    dev = how == "device"
    Mp, Md = _pair(device_vectors=dev)
    for round_ in range(2):
        blocks = [_sym(rng, v) for v in nz]
        given = _poisoned(blocks)
        for M in (Mp, Md):
            if dev:
                import torch
                dq = _block_docp(nz, [torch.as_tensor(G).cuda() for G in given])
                dq.F = [torch.as_tensor(f).cuda() for f in dq.F]
            else:
                dq = _block_docp(nz, given)
            if how != "staging":
                M.init_dense(dq) if round_ == 0 else M.update_dense(dq)
                continue
            L = M._L
            vp = lambda a: C.c_void_p(a.ctypes.data)
            nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
            if round_ == 0:
                assert L.hqpkkt_analyze_staged(M._h, 2, vp(nx), vp(nu), dq.n, 0, 0, None, None, None, None, None, None) == 0
                M.n, M.me, M.m = dq.dims
            for k, B in enumerate(blocks):
                buf, elems = C.c_void_p(), C.c_longlong()
                assert L.hqpkkt_stage_staging(M._h, k & 1, C.byref(buf), C.byref(elems)) == 0
                assert elems.value == max(max(nz) ** 2, max(f.size for f in dq.F))  # (its size and meaning stay)
                view = np.ctypeslib.as_array((C.c_double * elems.value).from_address(buf.value))
                view[:] = np.nan
                view = view[: B.size].reshape(B.shape)
                iu = np.triu_indices(B.shape[0])
                view[iu] = B[iu]
                assert L.hqpkkt_set_stage_hessian(M._h, k, buf, B.shape[0]) == 0
            F = [np.ascontiguousarray(b) for b in dq.F]
            fp = (C.c_void_p * dq.K)(*[b.ctypes.data for b in F])
            ld = (C.c_longlong * dq.K)(*[b.shape[1] for b in F])
            assert L.hqpkkt_set_values_staged(M._h, None, fp, ld, None, None) == 0
        assert [int(t > 0) for t in Mp.hessian_packing()[:, 0]] == [int(P.packs(v)) for v in nz]
        assert np.array_equal(Mp.hessian_layout(), Md.hessian_layout())
        for k, want in enumerate(padded(blocks)):
            got, dense = Mp.stage_hessian(k), Md.stage_hessian(k)
            assert _bits(got, dense), (round_, k, nz[k])
            assert _bits(got, want), (round_, k, nz[k])


@pytest.mark.parametrize("case", sorted(CASES))
def test_store_of_the_csr_hand_over(case):
    """The scatter to the packed places: the unpacked view is the unpacked handle's block bit for bit; new values on the
    same pattern replace every entry."""
    prog = _prog(case)
    Mp, Md = _pair()
    _init(Mp, prog, "csr"), _init(Md, prog, "csr")
    for round_ in range(2):
        if round_:
            other = H(prog, seed=56)
            Mp.update(other), Md.update(other)
            prog = other
        for k, want in enumerate(padded(problems.stage_hessians(prog.Q, prog.nx, prog.nu))):
            got = Mp.stage_hessian(k)
            assert _bits(got, Md.stage_hessian(k)) and _bits(got, want), (round_, k)


def _factor_and_step(M, prog, st):
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    M.step(prog, *st, *d)
    return d + [M.stage_block(k) for k in range(len(prog.nx))]


def _assert_same_factor_and_step(prog, how, **opts):
    st = problems.ip_state(prog, 3, 1.0)
    Mp, Md = _pair(**opts)
    outs = [_factor_and_step(_init(M, prog, how), prog, st) for M in (Mp, Md)]
    assert any(Mp.hessian_packing()[:, 0] > 0)
    for q, (a, b) in enumerate(zip(*outs)):
        assert np.isfinite(a).all() and _bits(a, b), q  # (q < 4: dx, dy, dz, dw; then V_0 ..)
    assert np.abs(outs[0][0]).max() > 0.0


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_factor_and_step_are_those_of_the_unpacked_form(case, form):
    """Every V_k and every output of step, bit for bit: the adds are the same values into the same entries."""
    _assert_same_factor_and_step(_prog(case), "csr", **FORMS[form])


@pytest.mark.parametrize("case", sorted(CASES))
def test_factor_and_step_on_the_dense_hand_over(case):
    _assert_same_factor_and_step(_prog(case), "dense")


@pytest.mark.parametrize("how", ["csr", "dense"])
def test_factor_and_step_with_dense_rows(how):
    _assert_same_factor_and_step(_wide(), how, dense_rows=32)


def _exact_rows(B, x):
    """(sum_j q_ij x_j rounded once, sum_j |q_ij x_j|) per row: every product split exactly into two doubles (Veltkamp /
    Dekker; no operand here is near overflow or underflow), the 2 nz terms of a row summed by math.fsum."""
    def split(a):
        c = a * 134217729.0
        hi = c - (c - a)
        return hi, a - hi
    p = B * x[None, :]
    bh, bl = split(B)
    xh, xl = split(np.broadcast_to(x[None, :], B.shape))
    e = ((bh * xh - p) + bh * xl + bl * xh) + bl * xl
    exact = np.array([math.fsum(np.concatenate([p[i], e[i]]).tolist()) for i in range(B.shape[0])])
    return exact, np.abs(p).sum(axis=1)


def _check_product(M, blocks, x, label):
    nz = [B.shape[0] for B in blocks]
    off = np.concatenate([[0], np.cumsum(nz)])
    n = int(off[-1])
    y = np.full(n + 64, -7.25)  # (64 marked doubles behind y)
    assert M._L.hqpkkt_debug_hess_symv(M._h, C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)) == 0
    assert (y[n:] == -7.25).all()
    assert np.array_equal(M.hess_symv(x).view(np.int64), y[:n].view(np.int64))  # (two runs: the same bits)
    for k, B in enumerate(blocks):
        xk, yk = x[off[k]: off[k + 1]], y[off[k]: off[k + 1]]
        exact, sabs = _exact_rows(B, xk)
        # |y_i - exact_i| <= (nz + 1) 2^-52 sum_j |q_ij x_j|, less the one rounding of the host's sum
        bound = ((nz[k] + 1) * 2.0 ** -52 - 2.0 ** -53) * sabs
        err = np.abs(yk - exact)
        worst = (err / np.where(bound > 0, bound, 1.0)).max()
        print(f"{label}, order {nz[k]}: largest error {worst:.3e} of the bound")
        assert (err <= bound).all(), (label, k, nz[k], worst)


@pytest.mark.parametrize("nz", BLOCK_ORDERS)
def test_product_against_exact_sums(nz):
    """y = Q x by the kernels of the handle's residual against sums accumulated exactly on the host, entry by entry, within
    the bound of any summation order of nz products; x of mixed signs and magnitudes, a single nonzero of x at every block's
    last index (the last column of every row, the whole last row's column sums), and blocks with a single stored nonzero
    in the last column (0, nz - 1) - the last row of the stored tiles - and in the last row (nz - 1, nz - 1)."""
    rng = np.random.default_rng(sum(nz) + 1)
    n = sum(nz)
    blocks = [_sym(rng, v) for v in nz]
    M = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True)
    dq = _block_docp(nz, _poisoned(blocks))
    M.init_dense(dq)
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    _check_product(M, blocks, x, "mixed x")
    e = np.zeros(n)
    e[np.cumsum(nz) - 1] = [1.5, -0.75, 3.0]
    _check_product(M, blocks, e, "x = e_last")
    for label, at in (("last column", lambda v: (0, v - 1)), ("last row", lambda v: (v - 1, v - 1))):
        single = []
        for v in nz:
            B = np.zeros((v, v))
            i, j = at(v)
            B[i, j] = B[j, i] = 1.0 + rng.uniform()
            single.append(B)
        dq.Qd = [np.triu(B) for B in single]
        M.update_dense(dq)
        _check_product(M, single, x, f"single nonzero in the {label}")
        y = M.hess_symv(x)
        assert np.count_nonzero(y) == (6 if label == "last column" else 3)


@pytest.mark.parametrize("case,how", [("order_313", "csr"), ("order_402_17_controls", "dense"), ("middle_stage_unpacked", "csr")])
def test_residual_and_solve_against_the_unpacked_form(case, how):
    """hqpkkt_residual on vectors that solve nothing, packed against unpacked: to 1e-12 relative, and within the criterion
    of test_gpu_staged_dense_hessian.py for the same comparison against the CSR form, 1e-14 of the largest row sum sum_j |K_ij|
    |d_j| of the Newton system.  The res of hqpkkt_solve - the residual of a refined solution, a few roundings of those row
    sums in either form - agrees to 1e-12 of the largest row sum at the solution, and the solutions to 1e-8 (the
    sibling tests' bar)."""
    prog = _prog(case)
    st = problems.ip_state(prog, 3, 1.0)
    rng = np.random.default_rng(3)
    d = [rng.uniform(-1, 1, k) for k in (prog.n, prog.me, prog.m, prog.m)]
    Mp, Md = _pair()
    _init(Mp, prog, how), _init(Md, prog, how)
    rp, rd = Mp.residuum(prog, *st, *d), Md.residuum(prog, *st, *d)
    bound = kkt_row_bound(prog, st, d)
    print(f"{case} ({how}): residuum packed {rp!r} unpacked {rd!r}; difference {abs(rp - rd):.2e}, row sum {bound:.3e}")
    assert rd > 1.0 and abs(rp - rd) <= 1e-12 * rd and abs(rp - rd) <= 1e-14 * bound
    sol, res = [], []
    for M in (Mp, Md):
        M.factor(prog, st[0], st[1])
        s = new_d(prog)
        res.append(M.solve(prog, *st, *s))
        sol.append(s)
    scale = kkt_row_bound(prog, st, sol[1])
    print(f"{case} ({how}): res of solve packed {res[0]:.3e} unpacked {res[1]:.3e}, row sum at the solution {scale:.3e}")
    assert abs(res[0] - res[1]) <= 1e-12 * scale
    for a, b in zip(*sol):
        assert np.abs(a - b).max() <= 1e-8 * max(1.0, np.abs(b).max())


def test_mehrotra_is_that_of_the_unpacked_form():
    """hqpkkt_mehrotra: the same result code and iteration count as the unpacked dense handle, the same point to 1e-8."""
    prog = _prog("order_402_17_controls")
    Mp, Md = _pair()
    Mp.init(prog), Md.init(prog)
    xp, yp, zp, wp, ip_ = Mp.mehrotra(prog)
    xd, yd, zd, wd, id_ = Md.mehrotra(prog)
    print(f"mehrotra: iterations packed / unpacked {ip_['iters']} / {id_['iters']}, result {ip_['result']} / {id_['result']}")
    assert ip_["result"] == id_["result"] and ip_["iters"] == id_["iters"], (ip_, id_)
    assert np.abs(xp - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xp - xd).max()


# The product's time.  Blocks of order 3000 (2992 states, 8 controls; the terminal block 2992): 9 000 000 doubles, 72 MB
# each.  The last-level cache of the device is 256 MB; the smallest stage count whose unpacked arena exceeds twice that, 512
# MB, is K = 7: 7 x 72.0 + 71.6 = 575.7 MB (K = 6: 503.7 MB).
TIME_K, TIME_NX, TIME_NU = 7, 2992, 8


def time_handles():
    """(packed, unpacked, n): two handles with the same blocks, handed over from host memory."""
    nx, nu = [TIME_NX] * (TIME_K + 1), [TIME_NU] * TIME_K
    nz = [TIME_NX + TIME_NU] * TIME_K + [TIME_NX]
    assert 8 * sum(v * up8(v) for v in nz) > 2 * 256e6 >= 8 * sum(v * up8(v) for v in nz[1:])
    rng = np.random.default_rng(5)
    U = rng.standard_normal((nz[0], nz[0]))
    blocks = [U] * TIME_K + [U[:TIME_NX, :TIME_NX]]  # (the upper triangle is read; the same values in every stage)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    F = [np.zeros((TIME_NX, TIME_NX + TIME_NU))] * TIME_K
    dq = problems.DenseDocp(nx, nu, empty(sum(nz)), empty(0), empty(0), F, 0, 0, Qd=blocks)
    Mp, Md = _pair()
    Mp.init_dense(dq), Md.init_dense(dq)
    return Mp, Md, dq


def test_the_packed_product_is_not_slower():
    """hess_symv_timed with reps = 20, the handles taking turns, three rounds each: the best of the packed handle is not
    above the worst of the unpacked one - the margin is the unpacked form's own spread; reading half the bytes must not cost
    more than that.  The reference is the unpacked form on the same device in the same process.  Measured on one MI355X
    when the test was written: packed 0.0752, 0.0780, 0.0751 ms, unpacked 0.1062, 0.1063, 0.1055 ms, ratio 0.706."""
    Mp, Md, dq = time_handles()
    assert (Mp.hessian_packing()[:, 0] == P.T).all()
    x = np.random.default_rng(6).standard_normal(dq.n)
    ms = {"packed": [], "unpacked": []}
    y = {}
    for _ in range(3):
        for name, M in (("packed", Mp), ("unpacked", Md)):
            y[name], t = M.hess_symv_timed(x, 20)
            ms[name].append(t)
    scale = np.abs(y["unpacked"]).max()
    assert np.abs(y["packed"] - y["unpacked"]).max() <= 1e-12 * scale
    best, worst = min(ms["packed"]), max(ms["unpacked"])
    print(f"Q x at order {TIME_NX + TIME_NU}, {TIME_K + 1} stages: packed {ms['packed']} ms, unpacked {ms['unpacked']} ms; "
          f"best packed / worst unpacked {best:.4f} / {worst:.4f} = {best / worst:.3f}")
    assert best <= worst, (ms,)
