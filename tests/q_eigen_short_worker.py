"""The GPU checks of hqpkkt_q_eigen_control_short (test_gpu_q_eigen_short.py runs this once, in a child process; the outcomes go
to stdout as one JSON line).  Plans: `detected` - fully stored blocks of the LENGTHS, per length one of every KIND (full with one
eigenvalue pushed to about -5; a diagonal of integers, zeros stored beside it; a full block whose first sub-column is zero; a
dominant one) and the full block of order 8 once more - and `band` - a band of 10 cut by bsize 63 into blocks of 63, 63, 4 that
are not fully stored, with entries across blocks -, on a FULL and a REDUCED handle.
The bound: A_SHORT L 2^-53 |B|_inf + 2^-50 |T| (the bracket's width).  A_SHORT is twice - the device sums in another order - the
largest distance between the eigenvalues of hessian_update.q_tridiag_model's T and eigvalsh of the block in units of L 2^-53
|B|_inf over these blocks: 1.02, measured and held by test_q_eigen_short_cpu.py, no device code in it.  B is the block eigvalsh
is given: for the shifted block against its floor that is the block with d_b on its diagonal, whose entries fl(q_ii + d_b) and
whose eigvalsh round in units of ITS norm (a floor of 40 on a block of norm 10: theta - 4.3e-14 seen, 2.8e-14 by the norm before)."""
import json
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu
import hessian_guard_cases as G
import q_eigen_cases as E
from q_eigen_worker import csr_with, shifted
from q_values_worker import bits, handle, rows_of, with_lower_nan, with_q

A_SHORT = 2.1
LENGTHS = (1, 2, 3, 8, 63, 64)
KINDS = ("full", "integers", "zero_column", "dominant")


def block(kind, L):
    rng = np.random.default_rng(8000 + 7 * L + KINDS.index(kind))
    if kind == "integers":
        return np.diag(rng.integers(-5, 6, L).astype(np.float64))
    R, u = np.triu(rng.uniform(-1.0, 1.0, (L, L))) / np.sqrt(L), rng.uniform(-1.0, 1.0, L)
    if kind == "dominant":  # (a_ii > 2 + sqrt(L), offsum_i < sqrt(L))
        return (3.0 + np.sqrt(L)) * np.eye(L) + R + np.triu(R, 1).T
    B = 3.0 * np.eye(L) + R + np.triu(R, 1).T - (8.0 / (u @ u)) * np.outer(u, u)
    if kind == "zero_column":
        B[1:, 0] = B[0, 1:] = 0.0
    return B


def plans():
    kinds = [(k, L) for L in LENGTHS for k in KINDS] + [("full", 8)]
    prog, first, _fine = E.program_of([[block(k, L)] for k, L in kinds])
    band = E.band_program(130)
    return [dict(name="detected", prog=prog, bsize=-1, first=first, kinds=kinds),
            dict(name="band", prog=band, bsize=63, first=hu.q_blocks_model(band.Q[0], band.Q[1], band.n, 63)[0], kinds=[("band", 63), ("band", 63), ("band", 4)])]


def tri_eigs(al, be):
    return np.linalg.eigvalsh(np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1))


def run(M, plan, **kw):  # one short control: (q_values before, report, T, q_values after)
    before = np.array(M.q_values())
    M.q_eigen_control_short(E.EPS, bsize=plan["bsize"], **kw)
    rep, T = M.q_eigen_report(with_T=True)
    return before, rep, T, np.array(M.q_values())


def check_plan(plan, res, want=()):
    """the issue's checks 1 - 6 of every block, and Q as a whole: the diagonals fl(q_ii + d_b), every other entry bit-unchanged"""
    before, rep, T, after = res
    prog, first = plan["prog"], plan["first"]
    assert T.shape == (first.size - 1, 2, np.diff(first).max()) and bits(after, shifted(prog, first, before, rep[:, E.DK]))
    for b, (kind, L) in enumerate(plan["kinds"]):
        r, tag = rep[b], (plan["name"], b, kind, L)
        B, Ba = (hu.q_block_dense(csr_with(prog, x), first, b) for x in (before, after))
        assert bits(r[E.GK], hu.q_block_gerschgorin_model(B)) and dict(want).get(b, r[E.OUTCOME]) == r[E.OUTCOME], (tag, r)
        if r[E.OUTCOME] in (0.0, 6.0):
            assert (r[2:9] == 0.0).all() and (T[b] == 0.0).all(), tag
            continue
        m = hu.eigen_replay(L, r[E.GK], r[E.THETA], L, T[b])
        assert r[E.STEPS] == L and bits(r[3:], [m[k] for k in ("lo", "hi", "rho", "lam", "d", "normT", "outcome")]), (tag, r, m)  # 2
        assert r[E.RHO] == 0.0 and bits(r[E.LAM], r[E.LO]) and r[E.OUTCOME] in (1.0, 2.0) and (T[b][:, L:] == 0.0).all() and T[b][1, L - 1] == 0.0, tag  # 3
        bound = [A_SHORT * L * E.U * G.norm_inf(X) + 2.0 ** -50 * r[E.NORMT] for X in (B, Ba)]
        err = np.abs(tri_eigs(T[b][0, :L], T[b][1, :L]) - np.linalg.eigvalsh(B)).max()
        assert err <= bound[0], (tag, err, bound)  # 1
        assert r[E.DK] == 0.0 or (r[E.OUTCOME] == 2.0 and np.linalg.eigvalsh(Ba)[0] >= r[E.THETA] - max(bound)), (tag, bound)  # 5
        assert kind != "integers" or bits(T[b][0, :L], np.diag(B)), tag  # 6


def check_blocks():
    """every block of both plans, theta = eps^2: checks 1 - 6; FULL and REDUCED, a second call and the block placed twice: equal bits"""
    for plan in plans():
        ref = None
        for cls in E.SP:
            M = handle(cls, plan["prog"])
            for _ in range(2):
                M.update(plan["prog"])
                res = run(M, plan)
                ref = ref or res
                assert all(bits(a, c) for a, c in zip(res, ref)), (plan["name"], cls.__name__)
        want = {"full": 2.0, "dominant": 0.0}
        check_plan(plan, ref, [(b, want[k]) for b, (k, _L) in enumerate(plan["kinds"]) if k in want])
        assert (ref[1][:, E.THETA] == E.EPS ** 2).all()
        if plan["name"] == "detected":
            at = plan["kinds"].index(("full", 8))
            assert bits(ref[1][at], ref[1][-1]) and bits(ref[2][at], ref[2][-1])


def check_untouched_and_nan():
    """NaN below the diagonal and across blocks changes no bits anywhere; a NaN inside one block: outcome 4 there, the block
    untouched, every other block's words unchanged."""
    plan = plans()[1]
    base, first = plan["prog"], plan["first"]
    ref = run(handle(E.SP[0], base), plan)
    prog, low = with_lower_nan(base)
    got = run(handle(E.SP[1], prog), plan)
    assert np.isnan(got[3][low]).all() and bits(got[3][~low], ref[3]) and bits(got[1], ref[1]) and bits(got[2], ref[2])
    r, ix = rows_of(base.Q), np.asarray(base.Q[1])
    of = np.repeat(np.arange(first.size - 1), np.diff(first))
    cross, one = of[r] != of[ix], of[r] == 1
    got = run(handle(E.SP[0], with_q(base, np.where(cross, np.nan, base.Q[2]))), plan)
    assert cross.any() and bits(got[3][~cross], ref[3][~cross]) and bits(got[1], ref[1]) and bits(got[2], ref[2])
    before, rep, T, after = run(handle(E.SP[0], with_q(base, np.where((r == 70) & (ix == 72), np.nan, base.Q[2]))), plan)  # (inside block 1)
    assert rep[1, E.OUTCOME] == 4.0 and rep[1, E.DK] == 0.0 and bits(after[one], before[one]) and bits(after[~one], ref[3][~one])
    assert bits(np.delete(rep, 1, 0), np.delete(ref[1], 1, 0)) and bits(np.delete(T, 1, 0), np.delete(ref[2], 1, 0))


def check_floors_sizes_and_sequence():
    """floor_from_bfgs behind a q_bfgs_update: one block with its floor lowered to s'Qs, one left alone (outcome 6); host floors;
    a block of 65: HQPKKT_E_SIZES, Qx bit-unchanged; q_eigen_control behind the short control on one plan: a fresh handle's bits."""
    rng = np.random.default_rng(51)
    prog, first, _f = E.program_of([[G.rank2_block(rng, v, 0.0)] for v in (63, 64, 8)], 51)
    plan = dict(name="bfgs", prog=prog, bsize=-1, first=first, kinds=[("spd", 63), ("spd", 64), ("spd", 8)])
    s, y = rng.uniform(-1, 1, prog.n), rng.uniform(-1, 1, prog.n)
    s[first[1]: first[2]] *= 2.0 ** -16  # (s'Qs of block 1 about 2^-27, below eps^2 = 2^-20)
    s[first[2]:] = 0.0
    for cls in E.SP:
        M = handle(cls, prog)
        M.q_bfgs_update(s, y)
        brep = M.q_bfgs_report()
        res = run(M, plan, floor_from_bfgs=True)
        theta = [sqs if 0.0 <= sqs < E.EPS ** 2 else E.EPS ** 2 for sqs in brep[:, 1]]  # (the block with s = 0: s'Qs = 0)
        assert res[1][:, E.THETA].tolist() == theta and theta[0] == E.EPS ** 2 > theta[1] > 0.0 == theta[2] and brep[2, 7] >= 2.0
        check_plan(plan, res, [(2, 6.0)])
        res = run(M, plan, floor=[50.0, -50.0, 40.0])
        assert res[1][:, E.THETA].tolist() == [50.0, -50.0, 40.0]
        check_plan(plan, res, [(0, 2.0), (2, 2.0)])
        F = handle(cls, with_q(prog, res[3]))
        for H in (M, F):
            H.q_eigen_control(E.EPS, floor=[60.0, 60.0, 60.0])
        a, c = M.q_eigen_report(with_T=True), F.q_eigen_report(with_T=True)
        assert bits(a[0], c[0]) and bits(a[1], c[1]) and bits(M.q_values(), F.q_values()) and (a[0][:, E.DK] > 0.0).all()
    long_ = E.program_of([[block("full", 65)], [block("full", 8)]])[0]
    M = handle(E.SP[0], long_)
    try:
        M.q_eigen_control_short(E.EPS)
        raise AssertionError("accepted")
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_SIZES and bits(M.q_values(), long_.Q[2])


CHECKS = {f.__name__[6:]: f for f in (check_blocks, check_untouched_and_nan, check_floors_sizes_and_sequence)}

if __name__ == "__main__":
    results = {}
    for name, fn in CHECKS.items():
        try:
            fn()
            results[name] = "ok"
        except Exception as e:
            results[name] = traceback.format_exc()
            if getattr(e, "code", None) == _lib.E_DEVICE:  # (nothing more is started on the GPU)
                break
    print("Q_EIGEN_SHORT_RESULTS " + json.dumps(results))
