"""The GPU checks of hqpkkt_q_eigen_control / hqpkkt_q_eigen_report (tests/test_gpu_q_eigen.py starts this once, as a child
process): every check of CHECKS runs on the device and the outcomes go to stdout as one JSON line, {name: "ok" |
traceback}.  A check that ends in a device error ends the run: nothing more is started on the GPU.

The programs, the allowance and the bound on T are those of tests/q_eigen_cases.py.  Per block, the checks (i) - (v) of
test_gpu_staged_hessian_guard._check_stage (check_block below):
  (i)   the reported bracket is honest for the reported T, by the exact Sturm count (every block here has at most 64 steps
        unless a check asks for more; those that end early by the invariant-subspace rule are among them)
  (ii)  eigen_replay of the reported T gives the same outcome and bit for bit lo, hi, rho, lambda_est, d, |T|
  (iii) |lambda_est - eigvalsh| <= rho + 8 ALLOWANCE unit on the block as q_values() gave it before the call,
        unit = 2^-53 L |B|_inf
  (iv)  q_values() after the call is bit for bit what a twin handle holds after hqpkkt_set_values with fl(q_ii + d_b) on the
        diagonals of the touched blocks: every off-diagonal entry and every untouched block unchanged
  (v)   after a shift eigvalsh >= theta - 8 ALLOWANCE unit, and on outcome 2 the shift is not wasteful:
        d - (theta - lambda) <= 2 rho + 8 ALLOWANCE unit."""
import ctypes as C
import json
import sys
import time
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu
import hessian_guard_cases as G
import q_eigen_cases as E
from q_eigen_cases import DK, GK, HI, LAM, LO, NORMT, OUTCOME, RHO, STEPS, THETA
from q_values_worker import Vecs, bits, handle, rows_of, with_lower_nan, with_q


def csr_with(prog, x):
    return (prog.Q[0], prog.Q[1], np.asarray(x, dtype=np.float64))


def shifted(prog, first, x, d):
    """x with fl(q_ii + d_b) on the stored diagonals of the blocks with d_b != 0"""
    r, ix = rows_of(prog.Q), np.asarray(prog.Q[1])
    of = np.repeat(np.arange(first.size - 1), np.diff(first))
    out = np.array(x, dtype=np.float64)
    k = np.flatnonzero((ix == r) & (d[of[r]] != 0.0))
    out[k] = out[k] + d[of[r[k]]]
    return out


def run(M, V, **ctl):
    """one control: (q_values before, report, T, q_values after) as numpy"""
    before = V.np(M.q_values()).copy()
    M.q_eigen_control(E.EPS, **ctl)
    rep, T = M.q_eigen_report(with_T=True)
    return before, rep, T, V.np(M.q_values())


def check_block(case, b, before, after, r, T, want=None, mod=None):
    """(i) - (v) of one block, and T against the model's where one is given; returns the outcome"""
    prog = case["prog"]
    tag = (case["name"], b)
    outcome = int(r[OUTCOME])
    lam, N, ln = E.block_facts(csr_with(prog, before), case, b)
    unit = E.U * ln * N
    slack = 8 * E.ALLOWANCE * unit
    if want is not None:
        assert outcome in want, (tag, outcome, want)
    steps = int(r[STEPS])
    if outcome == 6:  # (skipped ahead of everything: the replay has nothing to say)
        assert (r[2:9] == 0.0).all(), tag
    else:  # (ii)
        m = hu.eigen_replay(ln, r[GK], r[THETA], steps if outcome != 0 else 0, T)
        assert m["outcome"] == outcome, (tag, m["outcome"], outcome)
    assert (T[:, steps:] == 0.0).all(), tag
    if outcome in (1, 2, 3):
        for word, key in ((LO, "lo"), (HI, "hi"), (RHO, "rho"), (LAM, "lam"), (DK, "d"), (NORMT, "normT")):
            assert bits(r[word], m[key]), (tag, key, r[word], m[key])
        assert 1 <= steps <= min(ln, T.shape[1]), tag
        al, be, gg = T[0][:steps], T[1][:steps], 8 * E.U * r[NORMT]  # (i)
        assert G.sturm_count(al, be, r[LO] - gg) == 0 and G.sturm_count(al, be, r[HI] + gg) >= 1, tag
        assert r[HI] - r[LO] <= 2.0 ** -50 * r[NORMT], tag
        assert abs(r[LAM] - lam) <= r[RHO] + slack, (tag, r[LAM], lam, r[RHO])  # (iii)
    if outcome == 0:
        assert r[GK] >= r[THETA] and lam >= r[GK] - slack, tag
    if r[DK] != 0.0:  # (v)
        assert outcome in (2, 3) and r[DK] > 0.0, tag
        lam_new = E.block_facts(csr_with(prog, after), case, b)[0]
        assert lam_new >= r[THETA] - slack, (tag, lam_new)
        if outcome == 2:
            assert r[DK] - (r[THETA] - lam) <= 2 * r[RHO] + slack, (tag, r[DK], r[THETA] - lam)
    else:
        assert outcome in (0, 1, 4, 6), tag
    if mod is not None and outcome not in (0, 6):
        assert mod["steps"] >= 1, tag
        k, worst = E.t_compare(ln, N, T, mod["T"], min(steps, mod["steps"]))
        assert k >= 1 and worst <= 1.0, (tag, k, worst)
    return outcome


def check_all(case, cls, res, want=True, mod=None, twin=True):
    """every block of one control, and (iv) for the whole of Q; returns the outcomes"""
    before, rep, T, after = res
    prog, first = case["prog"], case["first"]
    nb = first.size - 1
    assert rep.shape == (nb, 10) and T.shape[:2] == (nb, 2), case["name"]
    outs = [check_block(case, b, before, after, rep[b], T[b], case["want"][b] if want else None, None if mod is None else mod[b]) for b in range(nb)]
    expect = shifted(prog, first, before, rep[:, DK])
    assert bits(after, expect), case["name"]
    if twin:  # (iv)
        R = handle(cls, with_q(prog, expect))
        assert bits(R.q_values(), after), case["name"]
    return outs


# ------------------------------------------------------------------------------------------------ the checks
def check_cases():
    """Every case of q_eigen_cases.cases() on its plugins, the short ones with host and device vectors: (i) - (v) per block,
    the outcomes the case allows, theta = eps^2, T against q_lanczos_model within t_bound, hqpkkt_q_blocks the partition."""
    seen = set()
    for case in E.cases():
        prog, first = case["prog"], case["first"]
        mod = E.model(prog.Q, case)
        cap = int(min(64, np.diff(first).max()))
        for cls in case["classes"]:
            for device in ((False, True) if prog.n < 1000 else (False,)):
                t0 = time.time()
                V = Vecs(device)
                M = handle(cls, prog, device)
                assert (M.q_blocks(case["bsize"])[0] == first).all()
                res = run(M, V, bsize=case["bsize"])
                assert res[2].shape[2] == cap and (res[1][:, THETA] == E.EPS ** 2).all(), case["name"]
                outs = check_all(case, cls, res, mod=mod, twin=not device)
                seen |= set(outs)
                print(f"{case['name']} {cls.__name__} device={device}: outcomes {sorted(set(outs))} max steps {int(res[1][:, STEPS].max())} "
                      f"{time.time() - t0:.2f} s", file=sys.stderr)
    assert seen >= {0, 1, 2}, seen


def _aligned_case():
    rng = np.random.default_rng(41)
    blocks = [[G.aligned_block(rng, 220)], [G.dominant_block(rng, 65)], [G.aligned_block(rng, 40)]]
    prog, first, fine = E.program_of(blocks, 41)
    assert (hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, -1)[0] == first).all()
    return dict(name="aligned", prog=prog, bsize=-1, first=first, fine=fine, want=None), blocks


def check_every_outcome():
    """max_steps = 1 on blocks whose smallest eigenvector is nearly the start vector (outcome 3: not converged, yet
    conservative; T has stride 1), floors per block with the cap of 128 steps (outcomes 1 and 2; T has stride 128), a NaN on
    a diagonal (outcome 4: left alone bit for bit, its neighbours not touched by it), and - under from_bfgs - a block with
    s = 0 (outcome 6).  With outcome 0 of the dominant block: 0, 1, 2, 3, 4, 6."""
    case, blocks = _aligned_case()
    prog = case["prog"]
    seen = set()
    for cls in E.SP:
        V = Vecs(False)
        M = handle(cls, prog)
        case["want"] = [(3,), (0,), (3,)]
        res = run(M, V, max_steps=1)
        assert res[2].shape == (3, 2, 1) and res[1][0, STEPS] == 1 and res[1][0, RHO] > 2.0 ** -40 * res[1][0, NORMT]
        seen |= set(check_all(case, cls, res))
        # block 0 below its spectrum, whose end is near -47, but above its Gerschgorin bound; block 1 above its own
        lam1 = float(np.linalg.eigvalsh(blocks[1][0])[0])
        floors = [-55.0, 2.0 * lam1, 1.0]
        M.update(prog)
        case["want"] = [(1,), (2,), (2,)]
        res = run(M, V, floor=floors, max_steps=128)
        assert res[2].shape == (3, 2, 128) and res[1][:, THETA].tolist() == floors
        seen |= set(check_all(case, cls, res))
        # a NaN on a diagonal of block 1
        x = np.array(prog.Q[2])
        k = int(np.flatnonzero((rows_of(prog.Q) == 227) & (np.asarray(prog.Q[1]) == 227))[0])
        x[k] = np.nan
        bad = with_q(prog, x)
        M = handle(cls, bad)
        before, rep, T, after = run(M, V)
        assert rep[:, OUTCOME].tolist() == [2.0, 4.0, 2.0] and rep[1, DK] == 0.0, rep[:, OUTCOME]
        assert bits(after, shifted(bad, case["first"], before, rep[:, DK])) and np.isfinite(np.delete(after, k)).all()
        ref = run(handle(cls, prog), V)
        assert bits(np.delete(rep, 1, 0), np.delete(ref[1], 1, 0)) and bits(np.delete(T, 1, 0), np.delete(ref[2], 1, 0))
        seen.add(4)
    seen |= _from_bfgs(E.SP[0], skip=True)
    assert seen >= {0, 1, 2, 3, 4, 6}, seen


def _bfgs_case():
    rng = np.random.default_rng(51)
    orders = (63, 64, 65, 8)
    blocks = [[G.rank2_block(rng, v, 0.0)] for v in orders]
    prog, first, fine = E.program_of(blocks, 51)
    return dict(name="bfgs", prog=prog, bsize=-1, first=first, fine=fine, want=None)


def _from_bfgs(cls, skip):
    """q_bfgs_update(eigen_control=eps) against the update followed by q_eigen_control(from_bfgs=True); returns the outcomes"""
    case = _bfgs_case()
    prog, first = case["prog"], case["first"]
    rng = np.random.default_rng(52)
    s, y = rng.uniform(-1, 1, prog.n), rng.uniform(-1, 1, prog.n)
    s[first[1]: first[2]] *= 2.0 ** -16  # s'Qs of block 1 about 3 |s|^2 2^-32, some 2^-27: below eps^2 = 2^-20
    y[first[2]: first[3]] = -y[first[2]: first[3]] - 3.0 * s[first[2]: first[3]]  # (an indefinite pair on block 2)
    if skip:
        s[first[3]:] = 0.0
    V = Vecs(False)
    M = handle(cls, prog)
    M.q_bfgs_update(s, y, eigen_control=E.EPS)
    brep = M.q_bfgs_report()
    rep, T = M.q_eigen_report(with_T=True)
    want = [b[1] if 0.0 <= b[1] < E.EPS ** 2 else E.EPS ** 2 for b in brep]
    assert rep[:, THETA].tolist() == want and 0.0 < want[1] < E.EPS ** 2 == want[0], want
    R = handle(cls, prog)
    R.q_bfgs_update(s, y)
    mid = R.q_values().copy()
    R.q_eigen_control(E.EPS, from_bfgs=True)
    r2, T2 = R.q_eigen_report(with_T=True)
    assert bits(r2, rep) and bits(T2, T) and bits(R.q_values(), M.q_values())
    outs = check_all(case, cls, (mid, rep, T, V.np(M.q_values())), want=False)
    skipped = brep[:, 7] >= 2
    assert ((rep[:, OUTCOME] == 6.0) == skipped).all() and skipped[3] == skip, (rep[:, OUTCOME], brep[:, 7])
    # without from_bfgs the floor is eps^2 and nothing is skipped; with it after an update of another bsize: refused
    R.q_eigen_control(E.EPS)
    r3 = R.q_eigen_report()
    assert (r3[:, THETA] == E.EPS ** 2).all() and (r3[:, OUTCOME] != 6.0).all()
    R.q_bfgs_update(s, y, bsize=0, pattern=True)
    try:
        R.q_eigen_control(E.EPS, from_bfgs=True)
        raise AssertionError("accepted")
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_INTERN
    R.q_eigen_control(E.EPS, bsize=0, from_bfgs=True)
    assert R.q_eigen_report().shape == (1, 10)
    return set(outs)


def check_from_bfgs():
    """from_bfgs lowers theta to the reported s'Qs on a block built so that 0 <= s'Qs < eps^2, on every plugin; the pair
    q_bfgs_update(eigen_control=eps) is the update followed by q_eigen_control(from_bfgs=True), bit for bit; HQPKKT_E_INTERN
    where the last update was of another bsize."""
    for cls in E.SP:
        _from_bfgs(cls, skip=False)
    _from_bfgs(E.SP[1], skip=True)


def check_untouched():
    """NaN below the diagonal is never read or written; NaN in the entries that cross two blocks stays there and reaches
    nothing."""
    V = Vecs(False)
    for case, cls in ((E.band_case(7), E.SP[0]), (E.band_case(100), E.SP[1]), (E.dense_case("mixed", E.MIXED_ORDERS, 2), E.SP[0])):
        base, first = case["prog"], case["first"]
        ref = run(handle(cls, base), V, bsize=case["bsize"])
        prog, low = with_lower_nan(base)
        assert (hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, case["bsize"])[0] == first).all()
        got = run(handle(cls, prog), V, bsize=case["bsize"])
        assert np.isnan(got[3][low]).all() and bits(got[3][~low], ref[3]) and bits(got[1], ref[1]) and bits(got[2], ref[2]), case["name"]
        r, ix = rows_of(base.Q), np.asarray(base.Q[1])
        of = np.repeat(np.arange(first.size - 1), np.diff(first))
        cross = of[r] != of[ix]
        assert cross.any() == case["name"].startswith("band")
        if cross.any():
            x = np.array(base.Q[2], dtype=np.float64)
            x[cross] = np.nan
            got = run(handle(cls, with_q(base, x)), V, bsize=case["bsize"])
            assert np.isnan(got[3][cross]).all() and bits(got[3][~cross], ref[3][~cross]), case["name"]
            assert bits(got[1], ref[1]) and bits(got[2], ref[2]), case["name"]


def _perm_case(orders):
    blocks = [[E.dense_block("indefinite", v, np.random.default_rng(700 + 11 * v))] for v in orders]
    prog, first, fine = E.program_of(blocks, 0)
    return dict(name="perm", prog=prog, bsize=-1, first=first, fine=fine, want=None)


def check_reproducible():
    """Equal bits from call to call, over the plugins and over host and device vectors; and for a block of 257 wherever it
    lies: the blocks of `mixed` permuted."""
    for case in E.cases():
        if case["prog"].n > 1000 and case["name"] != "long4097":
            continue
        ref = None
        for cls in case["classes"]:
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, case["prog"], device)
                for _ in range(2):
                    M.update(case["prog"])
                    res = run(M, V, bsize=case["bsize"])
                    ref = ref or res
                    assert all(bits(a, b) for a, b in zip(res, ref)), (case["name"], cls.__name__, device)
    ref = None
    for orders in (E.MIXED_ORDERS, (257, 1, 2, 3, 63, 64, 65), (64, 65, 257, 63, 1, 2, 3)):
        case = _perm_case(orders)
        at = orders.index(257)
        first = case["first"]
        before, rep, T, after = run(handle(E.SP[at % 2], case["prog"]), Vecs(False))
        r = rows_of(case["prog"].Q)
        d = (r >= first[at]) & (r < first[at + 1])
        got = (rep[at], T[at], before[d], after[d])
        assert rep[at, OUTCOME] == 2.0 and rep[at, STEPS] > 3
        ref = ref or got
        assert all(bits(a, b) for a, b in zip(got, ref)), orders


def check_handle_afterwards():
    """After the control the handle is not factored; then factor, step, residuum, solve and hqpkkt_mehrotra are bit-identical
    to a FRESH handle of the same class given the new q_values() through hqpkkt_set_values.  Once more under zd_policy -1
    with a Q so small that its diagonals are weak before and after."""
    from common import new_d
    from q_values_worker import _state_bits
    todo = [("random", problems.random_sparse_qp(150, 40, 90, row_nnz=3), E.SP, 0, (False, True)),
            ("grid", problems.grid_sparse_qp(14, 11), E.SP, 0, (False,)),
            ("docp", problems.with_dense_hessian(problems.lq_docp(4, 3, 2)), E.SP + (ipmatrix.IpLQDOCP,), -1, (False,))]
    for name, base, classes, bsize, weaks in todo:
        st = problems.ip_state(base, seed=12, spread=1.0)
        for cls in classes:
            for weak in weaks:
                prog = with_q(base, 1e-6 * np.asarray(base.Q[2])) if weak else base
                nb = len(hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, bsize)[0]) - 1
                scale = float(np.abs(prog.Q[2]).max())
                tag = (name, cls.__name__, weak)
                M = handle(cls, prog, zd_policy=-1)
                M.factor(prog, st[0], st[1])  # (factored - and not any more after the control)
                M.q_eigen_control(E.EPS, bsize=bsize, floor=np.full(nb, 2.0 * scale))  # (a floor above every diagonal entry: every block shifted)
                rep = M.q_eigen_report()
                assert (rep[:, DK] > 0.0).all(), tag
                if weak:
                    assert M.debug(30)[1] == 1, tag
                with np.testing.assert_raises(ipmatrix.KktError) as e:
                    M.solve(prog, *st, *new_d(prog))
                assert e.exception.code == _lib.E_INTERN, tag
                qx = M.q_values()
                assert not bits(qx, prog.Q[2]) and np.isfinite(qx).all(), tag
                prog2 = with_q(prog, qx)
                F = handle(cls, prog2, zd_policy=-1)
                assert (F.debug(30) == M.debug(30)).all(), tag
                a, b = _state_bits(M, prog2, st), _state_bits(F, prog2, st)
                assert len(a) == len(b) and all(bits(p, q) for p, q in zip(a, b)), tag
                if not weak:
                    assert a[0] == 0.0 and np.isfinite(a[1]).all(), tag  # (the factorisation went through)


def check_refused_and_report():
    """HQPKKT_E_INTERN on dense stage Hessians and before values; HQPKKT_E_RANGE for a floor that is not finite, then
    HQPKKT_E_FORMAT on a missing diagonal with nothing changed; hqpkkt_q_eigen_report: HQPKKT_E_INTERN before a control,
    HQPKKT_E_RANGE with *n_blocks and *t_steps set on a short cap, and the report of the LAST control."""
    L = _lib.lib()
    prog = E.docp_program()
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.init(prog)
    N = ipmatrix.IpSpBKP()
    N.analyze(prog)
    for H in (D, N):
        for call in (lambda: H.q_eigen_control(E.EPS), lambda: H.q_eigen_control(E.EPS, bsize=0, max_steps=3), H.q_eigen_report):
            try:
                call()
                raise AssertionError("accepted")
            except ipmatrix.KktError as e:
                assert e.code == _lib.E_INTERN
    G_ = handle(ipmatrix.IpSpBKP, prog)
    k, ts = C.c_longlong(-1), C.c_int(-1)
    out = np.zeros(10)

    def report(cap):
        return L.hqpkkt_q_eigen_report(G_._h, C.c_void_p(out.ctypes.data), None, cap, C.byref(k), C.byref(ts))

    assert report(1) == _lib.E_INTERN
    G_.q_bfgs_update(np.ones(prog.n), np.ones(prog.n))  # (another entry's report is not this one's)
    assert report(1) == _lib.E_INTERN
    G_.update(prog)
    G_.q_eigen_control(E.EPS)
    assert report(1) == _lib.E_RANGE and (k.value, ts.value) == (5, 5)
    assert (out == 0.0).all()
    rep, T = G_.q_eigen_report(with_T=True)
    assert rep.shape == (5, 10) and T.shape == (5, 2, 5)
    G_.q_eigen_control(E.EPS, bsize=4, max_steps=3)
    rep, T = G_.q_eigen_report(with_T=True)
    assert rep.shape == (6, 10) and T.shape == (6, 2, 3) and rep[:, STEPS].max() == 3
    G_.q_eigen_control(E.EPS, bsize=0, max_steps=128)
    rep, T = G_.q_eigen_report(with_T=True)
    assert rep.shape == (1, 10) and T.shape == (1, 2, 23)
    # a floor that is not finite, then the diagonal rule; nothing is written
    base = E.band_program(40)
    p, ix, x = (np.array(a) for a in base.Q)
    kd = int(p[7])
    assert ix[kd] == 7
    p[8:] -= 1
    bad = problems.Program(base.n, base.me, base.m, (p, np.delete(ix, kd), np.delete(x, kd)), base.A, base.C, base.c, base.b, base.d)
    for cls in E.SP:
        M = handle(cls, bad)
        fl = np.ones(6)
        fl[2] = np.nan
        for kw, code in ((dict(floor=fl), _lib.E_RANGE), (dict(floor=np.ones(6)), _lib.E_FORMAT), (dict(), _lib.E_FORMAT), (dict(from_bfgs=True), _lib.E_INTERN)):
            try:
                M.q_eigen_control(E.EPS, bsize=7, **kw)
                raise AssertionError("accepted")
            except ipmatrix.KktError as e:
                assert e.code == code, (kw, e.code)
        assert bits(M.q_values(), bad.Q[2])
        try:
            M.q_eigen_report()
            raise AssertionError("accepted")
        except ipmatrix.KktError as e:
            assert e.code == _lib.E_INTERN


def check_steps_stay_above_the_floor():
    """Twenty damped BFGS updates with pairs (s, y) of negative curvature, the control behind every one
    (q_bfgs_update(eigen_control = 1)): every block keeps its smallest eigenvalue at or above the floor the control reports
    (1, or the s'Qs that lowered it), less the allowance; the twin without the control ends below 1."""
    rng = np.random.default_rng(61)
    orders = (63, 64, 65)
    blocks = [[G.rank2_block(rng, v, 0.0)] for v in orders]
    prog, first, fine = E.program_of(blocks, 61)
    case = dict(name="steps", prog=prog, bsize=-1, first=first, fine=fine)
    for cls in E.SP:
        M, R = handle(cls, prog), handle(cls, prog)
        for it in range(20):
            s = rng.uniform(-1, 1, prog.n)
            y = -3.0 * s + 0.1 * rng.uniform(-1, 1, prog.n)
            M.q_bfgs_update(s, y, eigen_control=1.0)
            R.q_bfgs_update(s, y)
            rep = M.q_eigen_report()
            assert set(rep[:, OUTCOME].tolist()) <= {0.0, 1.0, 2.0}, (it, rep[:, OUTCOME])
            qx = M.q_values()
            for b, v in enumerate(orders):
                lam, N, ln = E.block_facts(csr_with(prog, qx), case, b)
                assert 0.0 < rep[b, THETA] <= 1.0 and lam >= rep[b, THETA] - 8 * E.ALLOWANCE * E.U * ln * N, (it, b, lam, rep[b, THETA])
        low = [E.block_facts(csr_with(prog, R.q_values()), case, b)[0] for b in range(3)]
        assert min(low) < 1.0, low
        print(f"{cls.__name__}: floors at the end {rep[:, THETA].tolist()}, without the control {low}", file=sys.stderr)


CHECKS = {f.__name__[6:]: f for f in (check_cases, check_every_outcome, check_from_bfgs, check_untouched, check_reproducible,
                                       check_handle_afterwards, check_refused_and_report, check_steps_stay_above_the_floor)}


def main():
    results = {}
    dead = False
    for name, fn in CHECKS.items():
        if dead:
            results[name] = "not run: an earlier check ended in a device error"
            continue
        t0 = time.time()
        try:
            fn()
            results[name] = "ok"
        except ipmatrix.KktError as e:
            results[name] = traceback.format_exc()
            dead = e.code == _lib.E_DEVICE
        except Exception:
            results[name] = traceback.format_exc()
        print(f"check {name}: {time.time() - t0:.2f} s", file=sys.stderr)
    print("Q_EIGEN_RESULTS " + json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
