"""GPU (-m gpu): the launch plan a handle reports (hqpkkt_debug_get 48, hqp_amd/csrc/tree_plan.hpp) against what runs.
Over the table of tests/tree_cases.py, one factor() and one step() with the profile on launch, per kernel class,
exactly what the plan's records say; and the solve meets the tolerances of tests/test_gpu_ordering.py against the CPU
oracle (residual within 1e-10 * scale of the oracle's, solution to 1e-8 * scale)."""
import numpy as np
import pytest

import tree_cases as tc
from hqp_amd import problems
from oracle import oracleapi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [c for c in tc.CASES if c.gpu], ids=lambda c: c.name)
def test_launches_are_the_plan_and_the_solve_is_the_oracles(case, monkeypatch):
    for k in tc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    prog = case.prog()
    st = problems.ip_state(prog, 3, 1.0)
    M = case.cls(**case.kw)
    M.init(prog)
    P = M.launch_plan()
    want = tc.launches(P)
    M.set_profile(True)
    M.factor(prog, st[0], st[1])
    d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
    M.step(prog, *st, *d)  # (one step() is one run_step; a solve() adds refinement rounds)
    got = {k: n for k, (_ms, n) in M.profile().items() if k in want}
    print(case.name, "kinds", sorted(tc.kinds(P)), "launches", got)
    assert got == want
    assert M.launch_plan() == P  # (no polled launch gave up)
    M.set_profile(False)
    res = M.solve(prog, *st, *d)
    O = oracleapi.OracleIpMatrix("SpBKP" if case.cls is tc.FULL else "RedSpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    osol, ores = O.solve(*st)
    scale = max(1.0, max(np.abs(v).max() for v in osol))
    err = max(np.abs(a - b).max() for a, b in zip(d, osol))
    print(case.name, "res", res, "oracle", ores, "err", err, "scale", scale)
    assert res <= ores + 1e-10 * scale
    assert err <= 1e-8 * scale
