"""GPU (-m gpu): every front of the tree factorisation entry by entry (tests/frontcheck.py), and one unrefined step
against the sweeps in longdouble on the device's own blocks.

Over the table of tests/tree_cases.py (the systems that together reach every launch kind of hqp_amd/csrc/tree_plan.hpp) at
problems.ip_state(prog, 3, 1.0): after factor() the identities a (pivot block), b (panel solve), c (L21), d (update
block), e (triangles) and the scale vector over EVERY front; then a second factorisation on the same handle with another
(z, w) and the identities again (a whole-tree factorisation alternates between two exchange copies of the update blocks);
then step() under the case's own environment and under each of tree_cases.SWITCHES, each on a handle made with the switch
set, against the reference sweeps on that handle's blocks.  Bounds: the docstring of tests/frontcheck.py; nothing here is
fitted to what the device gives.  n_perturbed == 0 everywhere (a perturbed pivot breaks a by design).

Beside the table: pivoting inside a tree (2x2 pivots and interchanges on general fronts and on small fronts, the counters
and the pivot types and orders read from the device asserted) and the integer twin - small-integer Q, A, C, dyadic z and w with z >= w, so that every scale is 1 and every
entry of a leaf front is exact: the first pivot's column of X of every leaf is the host's column bit for bit (the panel
itself holds L after the factorisation, so that column is what is left of the assembled entries untouched), and a to d
hold on it like everywhere else.

Seen on an MI355X (7 149 fronts, none through the float64 path): largest err/bound a 0.74, b 0.25, c 0.59, d 0.20, sweeps
0.004, scale vector 0."""
import time

import numpy as np
import pytest

import frontcheck as fc
import tree_cases as tc
from hqp_amd import problems

pytestmark = pytest.mark.gpu

GPU_CASES = [c for c in tc.CASES if c.gpu]
_kinds = {}


def _env(monkeypatch, env):
    for k in set(tc.SWITCHES) | {k for c in tc.CASES for k in c.env}:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _mode(cls):
    return 0 if cls is tc.FULL else 1


def sweep_blocks(src):
    """the blocks the reference sweeps need, of every front"""
    s = src.structure()
    out = {}
    for k in range(len(s["npiv"])):
        p, b = int(s["npiv"][k]), int(s["nborder"][k])
        panel = src.read_block(0, k).reshape(p, p + b).T
        out[k] = (panel[p:].copy(), np.tril(src.read_block(1, k).reshape(p, p).T), src.read_block(4, k),
                  src.read_block(5, k).astype(int), src.read_block(6, k).astype(int))
    return out


def step_check(M, rep, prog, st, mode, where):
    """one step() (one run_step, no refinement) against the reference sweeps on rep.blocks"""
    s = M.structure()
    d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
    M.step(prog, *st, *d)
    x_e = fc.solution_e(prog, mode, rep.sc, s["elim"], d[0], d[1], d[2])
    fc.check_sweeps(rep, s, prog, mode, st, x_e, where=where)


def full_check(cls, kw, prog, st, name, st2=None, switches=True, monkeypatch=None, env=None, exact_leaves=False):
    """the whole check of one system; returns (report of the first factorisation, handle, plan)"""
    mode = _mode(cls)
    t0 = time.time()
    M = cls(**kw)
    M.init(prog)
    plan = M.launch_plan()
    M.factor(prog, st[0], st[1])
    src = fc.DeviceSource(M, plan)
    rep = fc.check_fronts(src, prog, st[0], st[1], mode, name, exact_leaves=exact_leaves)
    step_check(M, rep, prog, st, mode, "sweeps, the case's environment")
    stats = M.stats()
    print(rep.text())
    print(name, "kinds", sorted(tc.kinds(plan)), "n_2x2", stats["n_2x2"], "n_slow_pivots", stats["n_slow_pivots"],
          "seconds %.1f" % (time.time() - t0))
    assert stats["n_perturbed"] == 0
    assert rep.fronts == len(src.structure()["npiv"])
    assert not rep.failed(), rep.text()
    if st2 is not None:  # the same handle again with other weights: the other exchange copy, nothing stale
        M.factor(prog, st2[0], st2[1])
        rep2 = fc.check_fronts(src, prog, st2[0], st2[1], mode, name + " (second factorisation)", keep_blocks=False)
        print(rep2.text())
        assert M.stats()["n_perturbed"] == 0
        assert not rep2.failed(), rep2.text()
    if switches:
        for sw in tc.SWITCHES:
            _env(monkeypatch, dict(env or {}, **{sw: "1"}))
            M2 = cls(**kw)
            M2.init(prog)
            M2.factor(prog, st[0], st[1])
            r2 = fc.Report(name + " " + sw)
            r2.sc = M2.read_block(7, 0)
            r2.blocks = sweep_blocks(fc.DeviceSource(M2))
            step_check(M2, r2, prog, st, mode, "sweeps, " + sw)
            print("  %s: sweep err/bound %.4g kinds %s" % (sw, r2.worst["sweep"][0], sorted(tc.kinds(M2.launch_plan()))))
            assert not r2.failed(), r2.text()
        _env(monkeypatch, env or {})
    return rep, M, plan


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.name)
def test_every_front_and_the_sweeps(case, monkeypatch):
    _env(monkeypatch, case.env)
    prog = case.prog()
    st = problems.ip_state(prog, 3, 1.0)
    st2 = problems.ip_state(prog, 4, 1.0)
    _rep, _M, plan = full_check(case.cls, case.kw, prog, st, case.name, st2=st2, monkeypatch=monkeypatch, env=case.env)
    _kinds[case.name] = tc.kinds(plan)


def test_the_cases_reach_every_launch_kind(monkeypatch):
    """a later change of the launch rule cannot quietly leave a kernel form unchecked: the plans of the cases above (as
    they ran; a case that did not run in this session is analysed here) hold every launch kind but the sharded one"""
    got = set()
    for case in GPU_CASES:
        if case.name not in _kinds:
            _env(monkeypatch, case.env)
            M = case.cls(**case.kw)
            M.analyze(case.prog())
            _kinds[case.name] = tc.kinds(M.launch_plan())
        got |= _kinds[case.name]
    assert got == tc.ALL_KINDS - {"schedule1"}, (sorted(tc.ALL_KINDS - got), sorted(got - tc.ALL_KINDS))


def _pivoting(M, kinds_wanted, src):
    """(2x2 pivots, fronts whose pivot order is not the identity) among the fronts of the given launch kinds, as read
    from the device"""
    s = M.structure()
    n2 = swapped = 0
    for k in range(len(s["npiv"])):
        if src.kind(k).startswith(kinds_wanted):
            n2 += int((M.read_block(5, k) == 1).sum())
            swapped += int((M.read_block(6, k) != np.arange(s["npiv"][k])).any())
    return n2, swapped


def test_slow_steps_on_general_fronts(monkeypatch):
    """interchanges (slow steps) inside k_factor_blk fronts of a tree: the slack rows in the order that needs them
    (slack_policy 0, tests/test_gpu_parity.py::test_slack_order_policies_agree).  Q of this family is strongly diagonal:
    its interchanges end in 1x1 pivots, the 2x2 pivots of general fronts are the next test's."""
    _env(monkeypatch, {})
    prog = problems.banded_qp(3000, 24, 4)
    st = problems.ip_state(prog, 3, 1.0)
    _rep, M, plan = full_check(tc.FULL, dict(slack_policy=0), prog, st, "banded3000_24_slack0", switches=False)
    assert M.stats()["n_slow_pivots"] > 0
    n2, swapped = _pivoting(M, "blk", fc.DeviceSource(M, plan))
    assert swapped > 0


def test_2x2_pivots_on_general_fronts(monkeypatch):
    """2x2 pivots and slow steps inside k_factor_blk fronts (D^-1 of a pair in k_panel_solve, in the sweeps): the
    double-integrator structure in leaves of up to 128 variables, weights over eight decades"""
    _env(monkeypatch, {})
    prog = problems.did_like_qp(400)
    st = problems.ip_state(prog, 3, 4.0)
    _rep, M, plan = full_check(tc.FULL, dict(leaf_size=128), prog, st, "did400_full_leaf128_spread4", switches=False)
    stats = M.stats()
    assert stats["n_2x2"] > 0 and stats["n_slow_pivots"] > 0, stats
    n2, swapped = _pivoting(M, "blk", fc.DeviceSource(M, plan))
    assert n2 > 0 and swapped > 0


def test_2x2_pivots_on_small_fronts(monkeypatch):
    """... and inside the one-wavefront kernel of the small fronts (here all levels in one launch).  That kernel counts
    its 2x2 pivots and not its slow steps (n_slow_pivots is k_factor_blk's): the interchanges are read off the pivot
    order it leaves."""
    _env(monkeypatch, {})
    prog = problems.did_like_qp(400)
    st = problems.ip_state(prog, 3, 4.0)
    _rep, M, plan = full_check(tc.FULL, {}, prog, st, "did400_full_spread4", switches=False)
    assert M.stats()["n_2x2"] > 0
    n2, swapped = _pivoting(M, fc.FUSED_KINDS, fc.DeviceSource(M, plan))
    assert n2 > 0 and swapped > 0


def integer_twin(n=240, seed=5):
    """small-integer Q (diagonal 8, a band of -1 / 0 / 1), A (entries -2 .. 2) and C = I; z a power of two >= w = 1: every
    scale of the FULL system is 1 and every entry of the matrix an integer or a power of two"""
    rng = np.random.default_rng(seed)
    me, m = n // 3, n
    i = np.repeat(np.arange(n), 2)
    j = i + np.tile(np.arange(1, 3), n)
    keep = j < n
    i, j = i[keep], j[keep]
    Q = problems._csr(np.concatenate([np.arange(n), i]), np.concatenate([np.arange(n), j]),
                      np.concatenate([np.full(n, 8.0), rng.integers(-1, 2, i.size).astype(float)]), n)
    ai = np.repeat(np.arange(me), 3)
    aj = 3 * ai + np.tile(np.arange(3), me)
    A = problems._csr(ai, aj, rng.choice([-2.0, -1.0, 1.0, 2.0], ai.size), me)
    C = problems._csr(np.arange(m), np.arange(m), np.ones(m), m)
    prog = problems.Program(n, me, m, Q, A, C)
    z = 2.0 ** rng.integers(0, 4, m)
    w = np.ones(m)
    r = [np.round(rng.uniform(-4, 4, k)) / 8.0 for k in (n, me, m, m)]
    return prog, (z, w, r[0], r[1], r[2], r[3])


def test_integer_twin_leaves_bit_for_bit(monkeypatch):
    _env(monkeypatch, {})
    prog, st = integer_twin()
    rep, M, _plan = full_check(tc.FULL, dict(leaf_size=8), prog, st, "integer_twin", switches=False, exact_leaves=True)
    assert np.array_equal(rep.sc, np.ones(rep.sc.size))
    s = M.structure()
    leaves = set(range(len(s["npiv"]))) - set(int(p) for p in s["parent"] if p >= 0)
    with_border = [k for k in leaves if s["nborder"][k] > 0]
    assert rep.exact_leaves == len(with_border) > 4
