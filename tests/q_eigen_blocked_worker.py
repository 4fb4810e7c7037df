"""The GPU checks of hqpkkt_q_eigen_control_blocked (test_gpu_q_eigen_blocked.py runs this once, in a child process).  Blocks,
check_plan and the bound are q_eigen_short_worker's.  Plans: `detected` - every kind at 513 (one over the long entry's limit), 527 (a
ragged tile and a ragged panel), 544 (whole panels) and 1025 (a thread's second row), "full" alone at 1024 and 2048, and one "full"
each of 8, 128 and 512, so that all four classes of block meet in one call - and `band` - a band of 10 over n = 1500 cut by bsize
600 into 600, 600, 300, entries across blocks, the blocks not fully stored: with one slot the second block's image lies where the
first left a dense one."""
import functools
import json
import os
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu
import hessian_guard_cases as G
import q_eigen_cases as E
import q_eigen_exact_worker as X
import q_eigen_long_worker as LW
import q_eigen_short_worker as W
from q_values_worker import bits, handle, rows_of, with_q

LENGTHS = (513, 527, 544, 1025)


def plans():
    kinds = [(k, L) for L in LENGTHS for k in W.KINDS] + [("full", L) for L in (1024, 2048, 8, 128, 512)]
    prog, first, _fine = E.program_of([[W.block(k, L)] for k, L in kinds])
    band = E.band_program(1500)
    return [dict(name="detected", prog=prog, bsize=-1, first=first, kinds=kinds),
            dict(name="band", prog=band, bsize=600, first=hu.q_blocks_model(band.Q[0], band.Q[1], band.n, 600)[0], kinds=[("band", 600), ("band", 600), ("band", 300)])]


run = functools.partial(X.run, entry="q_eigen_control_blocked")
PLANS, REF = [], []  # the plans and their default runs, made by check_blocks and shared


def same(a, c):
    return all(bits(x, y) for x, y in zip(a, c))


def check_blocks():  # every block of both plans, theta = eps^2; FULL and REDUCED, a second call: equal bits
    for plan in plans():
        ref = None
        for cls in E.SP:
            M = handle(cls, plan["prog"])
            for _ in range(2):
                M.update(plan["prog"])
                res = run(M, plan)
                ref = ref or res
                assert same(res, ref), (plan["name"], cls.__name__)
        PLANS.append(plan), REF.append(ref)
        W.check_plan(plan, ref, [(b, {"full": 2.0, "dominant": 0.0}[k]) for b, (k, _L) in enumerate(plan["kinds"]) if k in ("full", "dominant")])


def check_slots():  # handles made under a cap of one and of two slots: the default run's bits
    assert len(REF) == 2, "check_blocks gives the default runs"
    try:
        for slots, (plan, ref) in ((s, pr) for s in ("1", "2") for pr in zip(PLANS, REF)):
            os.environ["HQPKKT_QEB_SLOTS"] = slots
            assert same(run(handle(E.SP[0], plan["prog"]), plan), ref), (slots, plan["name"])
    finally:
        os.environ.pop("HQPKKT_QEB_SLOTS", None)


def check_same_as_long():  # no block over 512: the long entry's report, T and values bit for bit
    shifts = 0
    for plan in LW.plans():
        a, c = (X.run(handle(E.SP[0], plan["prog"]), plan, entry) for entry in ("q_eigen_control_long", "q_eigen_control_blocked"))
        assert same(a, c), plan["name"]
        shifts += int((a[1][:, E.DK] > 0.0).sum())
    assert shifts > 0


def check_nan_floors_sizes():
    plan, ref = PLANS[1], REF[1]  # a NaN inside block 1: outcome 4 there, the block untouched, every other block's words unchanged
    base, first = plan["prog"], plan["first"]
    r, ix = rows_of(base.Q), np.asarray(base.Q[1])
    one = (r >= first[1]) & (r < first[2])
    before, rep, T, after = run(handle(E.SP[0], with_q(base, np.where((r == 900) & (ix == 902), np.nan, base.Q[2]))), plan)
    assert rep[1, E.OUTCOME] == 4.0 and rep[1, E.DK] == 0.0 and bits(after[one], before[one]) and bits(after[~one], ref[3][~one])
    assert bits(np.delete(rep, 1, 0), np.delete(ref[1], 1, 0)) and bits(np.delete(T, 1, 0), np.delete(ref[2], 1, 0))
    rng = np.random.default_rng(54)  # host floors on blocks of 600, 1024 and 8
    prog, first, _f = E.program_of([[G.rank2_block(rng, v, 0.0)] for v in (600, 1024, 8)], 54)
    plan = dict(name="floors", prog=prog, bsize=-1, first=first, kinds=[("spd", 600), ("spd", 1024), ("spd", 8)])
    for cls in E.SP:
        res = run(handle(cls, prog), plan, floor=[50.0, -50.0, 40.0])
        assert res[1][:, E.THETA].tolist() == [50.0, -50.0, 40.0] and res[1][1, E.OUTCOME] in (0.0, 1.0)
        W.check_plan(plan, res, [(0, 2.0), (2, 2.0)])
    over = E.program_of([[W.block("full", 2049)], [W.block("full", 8)]])[0]  # a block of 2049: refused, Qx bit-unchanged
    M = handle(E.SP[0], over)
    try:
        M.q_eigen_control_blocked(E.EPS)
        raise AssertionError("accepted")
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_SIZES and bits(M.q_values(), over.Q[2])


if __name__ == "__main__":
    results = {}
    for fn in (check_blocks, check_slots, check_same_as_long, check_nan_floors_sizes):
        try:
            fn()
            results[fn.__name__[6:]] = "ok"
        except Exception as e:
            results[fn.__name__[6:]] = traceback.format_exc()
            if getattr(e, "code", None) == _lib.E_DEVICE:  # (nothing more is started on the GPU)
                break
    print("Q_EIGEN_BLOCKED_RESULTS " + json.dumps(results))
