"""V_k out of the G_xx launch (HQPKKT_FUSED_V=1: F_x'W_x and - Y'Rm as two k segments of one product, the control-sized
chain ahead of it on the control rows of G alone, H_xx added into V and its mirror image) against the sequence with the
separate rank-q update (HQPKKT_FUSED_V=0), each in a fresh child process (tests/fused_v_worker.py), on multistage QPs
of 3600 states - wide enough for the 128 x 128 tiles - with 1, 7, 50 and 64 controls, stage equalities that consume
controls, carried rows, a fixed and a free initial state.  Both runs are compared with the numpy model of the recursion
(tests/model_staged.py) by one unrefined step():

    distance(fused, model) <= 2 distance(separate, model) + FLOOR

2: the changed order of summation (Y'Rm inside the long sums of F_x'W_x; H_xx added last instead of first);
FLOOR = n_x eps = 8.0e-13: the worst-case rounding of ONE accumulation of n_x terms, which both sequences and the model
carry out in different orders - below it the distances say nothing about either.

Measured distances (MI355X; fused, separate):
    u1_free_x0_final2  see profiles/r08_stage_order.txt
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import rel_err
from hqp_amd import ipmatrix

import fused_v_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = W.NX * np.finfo(float).eps


def test_the_widths_take_the_128_tile_form():
    """(host code) The launch that forms V_k of a stage of NX states gets 128 x 128 tiles from the rule, for every depth
    of the second segment the cases have; a stage of 1000 states does not, and keeps the separate update."""
    for q in (1, 3, 9, 12, 51, 64):
        nslab = (W.NX + 15) // 16 + (q + 15) // 16
        form, tiles, _, _, _ = ipmatrix.gemm_form(W.NX, W.NX, 16 * nslab, lower=True, mirror=True)
        assert form in ("cut", "plain", "frac") and tiles == 29 * 30 // 2, (q, form, tiles)
    assert ipmatrix.gemm_form(1000, 1000, 16 * (63 + 4), lower=True, mirror=True)[0] == "6464"


def _child(case, fused, tmp_path):
    out = str(tmp_path / f"{case}_{fused}.npz")
    env = dict(os.environ, HQPKKT_FUSED_V=str(fused))
    subprocess.run([sys.executable, os.path.join(HERE, "fused_v_worker.py"), case, out], env=env, check=True, timeout=900)
    return np.load(out)


def _d(g):
    return [g[k] for k in ("dx", "dy", "dz", "dw")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in sorted(W.CASES) if not c.startswith("mixed")])
def test_fused_sequence_is_as_close_to_the_model_as_the_separate_update(case, tmp_path):
    from model_staged import StagedModel
    K = len(W.CASES[case]["nu"])
    new, old = _child(case, 1, tmp_path), _child(case, 0, tmp_path)
    assert list(new["fused"][:K]) == [1] * K and list(old["fused"][:K]) == [0] * K, (new["fused"], old["fused"])
    assert (new["ranks"] == old["ranks"]).all()
    assert new["asym"].max() == 0.0 and old["asym"].max() == 0.0  # V_k exactly symmetric, both ways
    prog = W.make(case)
    st = W.state(prog)
    R = StagedModel(prog)
    R.factor(st[0], st[1])
    md = R.step(*st[2:])
    for k in range(K):
        assert new["ranks"][k, 0] == len(R.st[k]["R"]) and new["ranks"][k, 1] == len(R.st[k]["L"]), (k, new["ranks"][k])
    dn, do = rel_err(_d(new), md), rel_err(_d(old), md)
    print(f"fused-V {case}: distance to the model fused {dn:.3e}, separate {do:.3e}, floor {FLOOR:.1e}")
    assert dn <= 2.0 * do + FLOOR, (case, dn, do)


@pytest.mark.gpu
def test_ineligible_stage_keeps_the_separate_update_and_its_bits(tmp_path):
    """Three stages, the last one with 70 controls (K of order 70 > 64).  It is the first stage of the backward
    recursion: under HQPKKT_FUSED_V=1 it takes the old sequence - its V is the old V bit for bit - and the two stages
    behind it take the new one."""
    case = "mixed_u50_u70"
    new, old = _child(case, 1, tmp_path), _child(case, 0, tmp_path)
    assert list(new["fused"][:3]) == [1, 1, 0] and list(old["fused"][:3]) == [0, 0, 0]
    assert np.array_equal(new["v_last"].view(np.int64), old["v_last"].view(np.int64))
    assert new["asym"].max() == 0.0
    dn = rel_err(_d(new), _d(old))
    print(f"fused-V {case}: fused against separate {dn:.3e}")
    assert dn <= 1e-9  # (the same system solved by both: the bound test_staged_step_equals_the_model uses against the model)
