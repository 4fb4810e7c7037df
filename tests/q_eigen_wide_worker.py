"""The GPU checks of hqpkkt_q_eigen_control_wide (test_gpu_q_eigen_wide.py runs this once, in a child process).  Blocks, check_plan
and the bound (A_SHORT L 2^-53 |B|_inf + 2^-50 |T|) are q_eigen_short_worker's.  Plans, the first two under HQPKKT_QEW_FROM=1, which
sends every block through k_qew_*: `detected` - every kind at 1, 2, 3, 17 (one tile), 63, 64, 65 (a tile's edge), 127, 129, 193 and 257
(a ragged last tile, 2 to 5 tile rows: the tile indexing, the column sums of the tile rows below and the mirror of a diagonal tile) -,
`band` - a band of 10 over n = 600 cut by bsize 257 into 257, 257, 86, entries across blocks, the blocks not fully stored - and `big`,
at the default threshold: "full" blocks of 2049 and 2100 beside blocks of 8, 128 and 600 for the other kernels.  The control takes the
partitions of hqpkkt_q_blocks(bsize) alone: the components of hqpkkt_q_sparse_bfgs_update have no eigenvalue control on any rung."""
import functools
import json
import os
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu
import hessian_guard_cases as G
import q_eigen_blocked_worker as BW
import q_eigen_cases as E
import q_eigen_exact_worker as X
import q_eigen_long_worker as LW
import q_eigen_short_worker as W
from q_eigen_worker import csr_with
from q_values_worker import bits, handle, rows_of, with_q

LENGTHS = (1, 2, 3, 17, 63, 64, 65, 127, 129, 193, 257)
run = functools.partial(X.run, entry="q_eigen_control_wide")
PLANS, REF = [], []  # the plans and their default runs, made by check_blocks and shared


def plans():
    kinds = [(k, L) for L in LENGTHS for k in W.KINDS]
    prog, first, _fine = E.program_of([[W.block(k, L)] for k, L in kinds])
    band = E.band_program(600)
    big = [("full", 8), ("full", 2049), ("full", 128), ("zero_column", 2100), ("full", 600)]
    bprog, bfirst, _fine = E.program_of([[W.block(k, L)] for k, L in big])
    return [dict(name="detected", prog=prog, bsize=-1, first=first, kinds=kinds, env="1"),
            dict(name="band", prog=band, bsize=257, first=hu.q_blocks_model(band.Q[0], band.Q[1], band.n, 257)[0], kinds=[("band", 257), ("band", 257), ("band", 86)], env="1"),
            dict(name="big", prog=bprog, bsize=-1, first=bfirst, kinds=big, env=None)]


def run_env(M, plan, **env):  # a control under the plan's threshold and the given hooks
    env = dict(env, **({"HQPKKT_QEW_FROM": plan["env"]} if plan["env"] else {}))
    os.environ.update(env)
    try:
        return run(M, plan)
    finally:
        for k in env:
            os.environ.pop(k, None)


def same(a, c):
    return all(bits(x, y) for x, y in zip(a, c))


def ratios(plan, res):  # err / bound of every reduced block, as check_plan forms both
    before, rep, T, _after = res
    out = []
    for b, (kind, L) in enumerate(plan["kinds"]):
        if rep[b, E.OUTCOME] in (0.0, 6.0):
            continue
        B = hu.q_block_dense(csr_with(plan["prog"], before), plan["first"], b)
        err = np.abs(W.tri_eigs(T[b][0, :L], T[b][1, :L]) - np.linalg.eigvalsh(B)).max()
        out.append(err / (W.A_SHORT * L * E.U * G.norm_inf(B) + 2.0 ** -50 * rep[b, E.NORMT]))
        print("err/bound %-8s block %2d %-11s L %4d: %.3f" % (plan["name"], b, kind, L, out[-1]), flush=True)
    return max(out)


def check_blocks():  # every block of the plans, theta = eps^2; FULL and REDUCED, a second call: equal bits
    worst = 0.0
    for plan in plans():
        ref = None
        for cls in E.SP[:1] if plan["name"] == "big" else E.SP:
            M = handle(cls, plan["prog"])
            for _ in range(2):
                M.update(plan["prog"])
                res = run_env(M, plan)
                ref = ref or res
                assert same(res, ref), (plan["name"], cls.__name__)
        PLANS.append(plan), REF.append(ref)
        worst = max(worst, ratios(plan, ref))
        W.check_plan(plan, ref, [(b, {"full": 2.0, "dominant": 0.0}[k]) for b, (k, _L) in enumerate(plan["kinds"]) if k in ("full", "dominant")])
    print("err/bound, the largest: %.3f" % worst, flush=True)


def check_slots_and_grids():  # handles made under a cap of one slot, and one workgroup per slot in the pass: the default run's bits
    assert len(REF) == 3, "check_blocks gives the default runs"
    for env, (plan, ref) in ((e, pr) for e in ({"HQPKKT_QEW_SLOTS": "1"}, {"HQPKKT_QEW_GROUPS": "1"}, {"HQPKKT_QEW_GROUPS": "3"}) for pr in zip(PLANS, REF)):
        assert same(run_env(handle(E.SP[0], plan["prog"]), plan, **env), ref), (env, plan["name"])


def check_same_as_blocked():  # no block over 2048, the default threshold: the blocked entry's report, T and values bit for bit
    shifts = 0
    for plan in [BW.plans()[1]] + LW.plans():
        a, c = (X.run(handle(E.SP[0], plan["prog"]), plan, entry) for entry in ("q_eigen_control_blocked", "q_eigen_control_wide"))
        assert same(a, c), plan["name"]
        shifts += int((a[1][:, E.DK] > 0.0).sum())
    assert shifts > 0


def check_nan_floors_sizes():
    plan, ref = PLANS[1], REF[1]  # a NaN inside block 1: outcome 4 there, the block untouched, every other block's words unchanged
    base, first = plan["prog"], plan["first"]
    r, ix = rows_of(base.Q), np.asarray(base.Q[1])
    one = (r >= first[1]) & (r < first[2])
    before, rep, T, after = run_env(handle(E.SP[0], with_q(base, np.where((r == 400) & (ix == 402), np.nan, base.Q[2]))), plan)
    assert rep[1, E.OUTCOME] == 4.0 and rep[1, E.DK] == 0.0 and bits(after[one], before[one]) and bits(after[~one], ref[3][~one])
    assert bits(np.delete(rep, 1, 0), np.delete(ref[1], 1, 0)) and bits(np.delete(T, 1, 0), np.delete(ref[2], 1, 0))
    rng = np.random.default_rng(55)  # floor_from_bfgs behind an update that left block 2 alone (outcome 6), then host floors
    prog, first, _f = E.program_of([[G.rank2_block(rng, v, 0.0)] for v in (129, 200, 65)], 55)
    plan = dict(name="floors", prog=prog, bsize=-1, first=first, kinds=[("spd", 129), ("spd", 200), ("spd", 65)], env="1")
    s, y = rng.uniform(-1, 1, prog.n), rng.uniform(-1, 1, prog.n)
    s[first[1]: first[2]] *= 2.0 ** -16  # (s'Qs of block 1 about 2^-27, below eps^2 = 2^-20)
    s[first[2]:] = 0.0
    for cls in E.SP:
        M = handle(cls, prog)
        M.q_bfgs_update(s, y)
        brep = M.q_bfgs_report()
        os.environ["HQPKKT_QEW_FROM"] = "1"
        try:
            res = run(M, plan, floor_from_bfgs=True)
            theta = [sqs if 0.0 <= sqs < E.EPS ** 2 else E.EPS ** 2 for sqs in brep[:, 1]]
            assert res[1][:, E.THETA].tolist() == theta and theta[0] == E.EPS ** 2 > theta[1] > 0.0 == theta[2] and brep[2, 7] >= 2.0
            W.check_plan(plan, res, [(2, 6.0)])
            res = run(M, plan, floor=[50.0, -50.0, 40.0])
        finally:
            os.environ.pop("HQPKKT_QEW_FROM", None)
        assert res[1][:, E.THETA].tolist() == [50.0, -50.0, 40.0] and res[1][1, E.OUTCOME] in (0.0, 1.0)
        W.check_plan(plan, res, [(0, 2.0), (2, 2.0)])
    over = over_program()  # a block of 8193: refused, Qx bit-unchanged
    M = handle(E.SP[0], over)
    try:
        M.q_eigen_control_wide(E.EPS)
        raise AssertionError("accepted")
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_SIZES and bits(M.q_values(), over.Q[2])


def over_program(L=8193, tail=8):
    """detected blocks of L and of `tail`: a diagonal, and the first row of each block stored whole"""
    n = L + tail
    r = np.concatenate([np.arange(n), np.zeros(L - 1, dtype=np.int64), np.full(tail - 1, L)])
    c = np.concatenate([np.arange(n), np.arange(1, L), np.arange(L + 1, n)])
    return E._program(n, problems._csr(r, c, np.where(r == c, 4.0, 0.5 ** 8), n), 0)


if __name__ == "__main__":
    results = {}
    for fn in (check_blocks, check_slots_and_grids, check_same_as_blocked, check_nan_floors_sizes):
        try:
            fn()
            results[fn.__name__[6:]] = "ok"
        except Exception as e:
            results[fn.__name__[6:]] = traceback.format_exc()
            if getattr(e, "code", None) == _lib.E_DEVICE:  # (nothing more is started on the GPU)
                break
    print("Q_EIGEN_WIDE_RESULTS " + json.dumps(results))
