"""GPU (-m gpu): paths of the device-resident loops (hqp_amd/csrc/ip_loops.hip) that the switch-against-switch tests of
test_gpu_franke.py do not reach - hot starts, a QP without inequalities, qp_init_method 3 - with the segment graphs
against the loops launch by launch (HQPKKT_NO_IP_SEGMENTS): the same calls on the same values, so the same iterates."""
import numpy as np
import pytest

from hqp_amd import ipmatrix, problems
from test_reference_host import _without_inequalities

pytestmark = pytest.mark.gpu

PROGS = {"did400": lambda: problems.did_like_qp(400), "banded": lambda: problems.banded_qp(300, 8, 5),
         "noineq": lambda: _without_inequalities(problems.banded_qp(400, 10, 6))}


def _both_ways(prog, calls, monkeypatch):
    """[(with segment graphs, launch by launch)] of `calls` = [(loop, keyword arguments)], made on one handle each way"""
    runs = []
    for env in ({}, {"HQPKKT_NO_IP_SEGMENTS": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        M = ipmatrix.IpRedSpBKP()
        M.init(prog)
        runs.append([getattr(M, loop)(prog, **kw) for loop, kw in calls])
    return list(zip(*runs))


def _same(a, b, what):
    assert (a[4]["result"], a[4]["iters"], a[4]["n_solve"]) == (b[4]["result"], b[4]["iters"], b[4]["n_solve"]), (what, a[4], b[4])
    for vec, u, v in zip("xyzw", a[:4], b[:4]):
        assert np.array_equal(u, v), (what, vec, float(np.abs(u - v).max()), a[4], b[4])


@pytest.mark.parametrize("case", ["did400", "banded"])
@pytest.mark.parametrize("loop", ["mehrotra", "franke"])
def test_hot_start_with_and_without_segment_graphs(loop, case, monkeypatch):
    """hot_start 2 (cold, keeping what a hot start needs), then hot_start 1 on the same handle"""
    kw = dict(max_iters=300) if loop == "franke" else {}
    pairs = _both_ways(PROGS[case](), [(loop, dict(hot_start=2, **kw)), (loop, dict(hot_start=1, **kw))], monkeypatch)
    for name, (a, b) in zip(("hot_start 2", "hot_start 1"), pairs):
        _same(a, b, name)


@pytest.mark.parametrize("loop", ["mehrotra", "franke"])
def test_equality_constrained_qp_with_and_without_segment_graphs(loop, monkeypatch):
    """m == 0: one Newton step in hqpkkt_mehrotra; hqpkkt_franke's steps with mu = 0 and no step-length reduction"""
    (a, b), = _both_ways(PROGS["noineq"](), [(loop, dict(max_iters=300) if loop == "franke" else {})], monkeypatch)
    _same(a, b, loop)
    assert a[2].size == 0


@pytest.mark.parametrize("case", ["did400", "banded"])
def test_init_method_3_with_and_without_segment_graphs(case, monkeypatch):
    (a, b), = _both_ways(PROGS[case](), [("mehrotra", dict(init_method=3))], monkeypatch)
    _same(a, b, "init_method 3")
