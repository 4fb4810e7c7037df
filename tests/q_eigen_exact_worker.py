"""The GPU checks of hqpkkt_q_eigen_control_exact (test_gpu_q_eigen_exact.py runs this once, in a child process).  Blocks, check_plan
and the bound are q_eigen_short_worker's.  Plans: `detected` - full blocks of the LENGTHS, one of every kind, so that every launch
sees blocks of both classes - and `band` - a band of 10 over n = 230 cut by bsize 100 into 100, 100, 30, entries across blocks."""
import json
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu
import hessian_guard_cases as G
import q_eigen_cases as E
import q_eigen_short_worker as W
from q_values_worker import bits, handle, rows_of, with_q

LENGTHS = (8, 64, 65, 96, 97, 127, 128)


def plans():
    kinds = [(k, L) for L in LENGTHS for k in W.KINDS]
    prog, first, _fine = E.program_of([[W.block(k, L)] for k, L in kinds])
    band = E.band_program(230)
    return [dict(name="detected", prog=prog, bsize=-1, first=first, kinds=kinds),
            dict(name="band", prog=band, bsize=100, first=hu.q_blocks_model(band.Q[0], band.Q[1], band.n, 100)[0], kinds=[("band", 100), ("band", 100), ("band", 30)])]


def run(M, plan, entry="q_eigen_control_exact", **kw):  # one control: (q_values before, report, T, q_values after)
    before = np.array(M.q_values())
    getattr(M, entry)(E.EPS, bsize=plan["bsize"], **kw)
    rep, T = M.q_eigen_report(with_T=True)
    return before, rep, T, np.array(M.q_values())


def check_blocks():  # every block of both plans, theta = eps^2; FULL and REDUCED, a second call: equal bits
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
        W.check_plan(plan, ref, [(b, want[k]) for b, (k, _L) in enumerate(plan["kinds"]) if k in want])


def check_same_as_short():  # no block over 64: the short entry's report, T and values bit for bit
    plan = W.plans()[0]
    a, c = (run(handle(E.SP[0], plan["prog"]), plan, entry) for entry in ("q_eigen_control_short", "q_eigen_control_exact"))
    assert all(bits(x, y) for x, y in zip(a, c)) and (a[1][:, E.DK] > 0.0).any()


def check_nan_floors_sizes():
    plan = plans()[1]  # a NaN inside block 1: outcome 4 there, the block untouched, every other block's words unchanged
    base, first = plan["prog"], plan["first"]
    ref = run(handle(E.SP[0], base), plan)
    r, ix = rows_of(base.Q), np.asarray(base.Q[1])
    one = (r >= first[1]) & (r < first[2])
    before, rep, T, after = run(handle(E.SP[0], with_q(base, np.where((r == 150) & (ix == 152), np.nan, base.Q[2]))), plan)
    assert rep[1, E.OUTCOME] == 4.0 and rep[1, E.DK] == 0.0 and bits(after[one], before[one]) and bits(after[~one], ref[3][~one])
    assert bits(np.delete(rep, 1, 0), np.delete(ref[1], 1, 0)) and bits(np.delete(T, 1, 0), np.delete(ref[2], 1, 0))
    rng = np.random.default_rng(52)  # host floors on blocks of 100, 128 and 8
    prog, first, _f = E.program_of([[G.rank2_block(rng, v, 0.0)] for v in (100, 128, 8)], 52)
    plan = dict(name="floors", prog=prog, bsize=-1, first=first, kinds=[("spd", 100), ("spd", 128), ("spd", 8)])
    for cls in E.SP:
        res = run(handle(cls, prog), plan, floor=[50.0, -50.0, 40.0])
        assert res[1][:, E.THETA].tolist() == [50.0, -50.0, 40.0] and res[1][1, E.OUTCOME] in (0.0, 1.0)
        W.check_plan(plan, res, [(0, 2.0), (2, 2.0)])
    long_ = E.program_of([[W.block("full", 129)], [W.block("full", 8)]])[0]  # a block of 129: refused, Qx bit-unchanged
    M = handle(E.SP[0], long_)
    try:
        M.q_eigen_control_exact(E.EPS)
        raise AssertionError("accepted")
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_SIZES and bits(M.q_values(), long_.Q[2])


if __name__ == "__main__":
    results = {}
    for fn in (check_blocks, check_same_as_short, check_nan_floors_sizes):
        try:
            fn()
            results[fn.__name__[6:]] = "ok"
        except Exception as e:
            results[fn.__name__[6:]] = traceback.format_exc()
            if getattr(e, "code", None) == _lib.E_DEVICE:  # (nothing more is started on the GPU)
                break
    print("Q_EIGEN_EXACT_RESULTS " + json.dumps(results))
