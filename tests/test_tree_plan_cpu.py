"""CPU: what a handle of the tree engine launches (hqp_amd/csrc/tree_plan.hpp through hqpkkt_debug_get 48), read after
hqpkkt_analyze alone - no device is touched.  Over the table of tests/tree_cases.py: every front is launched exactly once
per factorisation and per sweep, the pivot-block instance is the smallest that holds a level, the fused top's fronts fit
its instance, no launch asks for more LDS than the chip has, item 31 is the plan's header, the three switches change the
plan as they say and nothing else, and the table reaches every launch kind of the rule."""
import copy

import numpy as np
import pytest

import tree_cases as tc
from hqp_amd import ipmatrix

M_ = ipmatrix.Hqp_IpMatrix
_made = {}


def analyzed(case, monkeypatch):
    """(handle after hqpkkt_analyze, its structure): one per case; what the plan reads from the environment is read at
    every launch_plan() of such a handle"""
    for k in tc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    if case.name not in _made:
        M = case.cls(**case.kw)
        M.analyze(case.prog())
        _made[case.name] = (M, M.structure())
    return _made[case.name]


def nodes_of(case, s):
    """per schedule the supernodes it holds"""
    owner, ids = s["node_owner"], np.arange(len(s["npiv"]))
    if "shard" not in case.kw:
        return [ids, ids[:0]]
    return [ids[owner == case.kw["shard"][0]], ids[owner == -1]]


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_every_front_is_launched_once_and_fits_its_launch(case, monkeypatch):
    M, s = analyzed(case, monkeypatch)
    P = M.launch_plan()
    assert list(M.debug(31)) == [P[k] for k in M.PLAN_HEADER[:7]]
    npiv, nbor, level = s["npiv"], s["nborder"], s["level"]
    sched = nodes_of(case, s)
    assert [P["nnodes0"], P["nnodes1"]] == [len(v) for v in sched]
    for k in ("top_lds", "lds_panel", "lds_bwdb", "lds_blk"):
        assert 0 <= P[k] <= tc.LDS_LIMIT, k
    in_top = in_tree = 0
    for w in range(2):
        off = 0
        for l, R in enumerate(P["levels"][w]):
            here = sched[w][level[sched[w]] == l]
            assert R["n"] == len(here) and (R["n"] == 0 or R["nodes_off"] == off), (w, l)
            off += R["n"]
            # factorisation: one of the three launches of the level, or the whole-tree launch
            if w == 0 and P["tree_factor"]:
                assert R["fs_n"] + R["sm_n"] + R["blk_n"] + R["ps_grid"] + R["su_variant"] + R["big_n"] == 0
            else:
                assert R["fs_n"] + R["sm_n"] + R["blk_n"] == R["n"], (w, l)
            for k in ("fs_lds", "sm_lds", "blk_lds"):
                assert 0 <= R[k] <= tc.LDS_LIMIT
            if R["blk_n"]:
                # (fronts outside the pivot-block launch have at most 32 pivots: a larger maximum is a pivot-block front's)
                maxp = int(npiv[here].max())
                want = min(i for i, cap in enumerate(tc.FB_MAXP) if cap >= maxp) if maxp > 32 else 0
                assert R["blk_inst"] == want and R["blk_threads"] == (512 if want == 0 else 768), (w, l, maxp)
            assert (R["su_variant"] == 0) == (R["su_n"] == 0) and R["su_grid"] == (2 * R["su_n"] if R["su_variant"] == 1 else R["su_n"])
            # the sweeps of the solve
            if R["fwd_form"] in (M_.FWD_TOP, M_.FWD_TREE):
                assert w == 0 and R["fwd_small_n"] + R["fwd_grid"] + R["bwd_small_n"] + R["bwd_a_grid"] + R["bwd_b_grid"] == 0
                in_top += R["n"] * (R["fwd_form"] == M_.FWD_TOP)
                in_tree += R["n"] * (R["fwd_form"] == M_.FWD_TREE)
                if R["fwd_form"] == M_.FWD_TOP:
                    ns, nu = (3, 11) if P["top_ns"] == 3 else (4, 10)
                    assert l >= P["top_lt"] and (npiv[here] <= 16 * nu).all() and (nbor[here] <= 64 * ns).all()
                continue
            rest = R["n"] - R["fwd_small_n"]
            assert (R["fwd_form"] == M_.FWD_NONE) == (rest == 0), (w, l)
            assert R["fwd_a_grid"] == (rest if R["fwd_form"] == M_.FWD_AB else 0)
            assert (R["fwd_form"] == M_.FWD_AB) == (R["fwd_grid"] > 1024) and (rest == 0 or R["fwd_grid"] >= rest)
            assert R["bwd_small_n"] + R["bwd_a_grid"] == R["n"] and (R["bwd_b_grid"] > 0) == (R["bwd_a_grid"] > 0)
    assert in_top == P["top_n"] and in_tree == (P["nnodes0"] if P["small_tree"] else 0)
    assert not (P["top_n"] and P["small_tree"]) and P["tree_factor"] <= P["small_tree"]
    if P["top_n"]:
        assert P["top_ns"] in (3, 4) and (P["top_split"] == 1 or P["top_n"] <= 128)


def without(P, *keys):
    Q = copy.deepcopy(P)
    for k in keys:
        Q.pop(k, None)
    return Q


FACTOR_KEYS = M_.PLAN_RECORD[:M_.PLAN_RECORD.index("fwd_form")]


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_the_switches_change_the_plan_as_they_say(case, monkeypatch):
    M, _s = analyzed(case, monkeypatch)
    base = M.launch_plan()
    # HQPKKT_SOLVE_TOP_FUSED: the top in one launch where one launch may hold its fronts; nothing else
    monkeypatch.setenv("HQPKKT_SOLVE_TOP_FUSED", "1")
    P = M.launch_plan()
    assert without(P, "top_split") == without(base, "top_split")
    assert P["top_split"] == (1 if P["top_n"] > 128 else 0)
    if "HQPKKT_SOLVE_TOP_FUSED" not in case.env:
        monkeypatch.delenv("HQPKKT_SOLVE_TOP_FUSED")
        assert base["top_split"] == (1 if base["top_n"] else 0)
    # HQPKKT_NO_SOLVE_TOP: no fused top, its levels launch by themselves; the factorisation and the levels below as before
    monkeypatch.setenv("HQPKKT_NO_SOLVE_TOP", "1")
    P = M.launch_plan()
    assert [P["top_n"], P["top_lds"], P["top_split"]] == [0, 0, 0] and P["top_lt"] == P["nlevels"]
    for (w, l, R), (_w, _l, B) in zip(tc.records(P), tc.records(base)):
        assert R["fwd_form"] != M_.FWD_TOP
        if B["fwd_form"] == M_.FWD_TOP:
            assert {k: R[k] for k in FACTOR_KEYS} == {k: B[k] for k in FACTOR_KEYS} and R["bwd_a_grid"] == R["n"]
        else:
            assert R == B, (w, l)
    assert without(P, "levels", "top_n", "top_lt", "top_lds", "top_ns", "top_split") == \
        without(base, "levels", "top_n", "top_lt", "top_lds", "top_ns", "top_split")
    monkeypatch.delenv("HQPKKT_NO_SOLVE_TOP")
    # HQPKKT_NO_TREE_SWEEPS: no whole-tree launch, every level launches by itself; a tree that had none is untouched
    monkeypatch.setenv("HQPKKT_NO_TREE_SWEEPS", "1")
    P = M.launch_plan()
    assert [P["small_tree"], P["tree_factor"]] == [0, 0]
    if not base["small_tree"]:
        assert P == base
    else:
        for _w, _l, R in tc.records(P):
            assert R["fwd_form"] == M_.FWD_NONE and R["fs_n"] == R["fwd_small_n"] == R["bwd_small_n"] == R["n"]


def test_the_table_reaches_every_launch_kind(monkeypatch):
    seen = set()
    for case in tc.CASES:
        M, _s = analyzed(case, monkeypatch)
        seen |= tc.kinds(M.launch_plan())
    assert seen == tc.ALL_KINDS, (tc.ALL_KINDS - seen, seen - tc.ALL_KINDS)
