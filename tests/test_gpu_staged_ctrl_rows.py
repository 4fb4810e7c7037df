"""The fused stage with the control rows of G out of W's ragged last tile row (the control-row segment, staged_stage_fused
with StagedDev::ctrl_rows) against the sequence with the separate rank-q update (HQPKKT_FUSED_V=0), each in a fresh child
process (tests/ctrl_rows_worker.py), by the criterion of tests/test_gpu_staged_fused_v.py: both runs are compared with
the numpy model of the recursion (tests/model_staged.py) by one unrefined step(),

    distance(fused, model) <= 2 distance(separate, model) + n_x eps.

Width: the smallest for which the stage takes the new sequence unasked - W = V+ F gets the cut form on 128 x 128 tiles,
the ragged last tile row has an even number r of rows with r + n_u <= 128, and the width is not one of those whose chain
runs beside G_xx (1280 .. 4096 states).  It is found on the host (4098: 33 x 33 tiles, r = 2).  Three stages, 7 and 50
controls.  The case whose row condition fails runs at 2300 states (r = 124) under HQPKKT_FUSED_V=1: the fused sequence
with the thin product, as before the segment existed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import rel_err
from hqp_amd import ipmatrix

import ctrl_rows_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(float).eps


def _takes_segment_unasked(n, nu):
    r = n - (n - 1) // 128 * 128
    if n % 2 or r + nu > 128 or 1280 <= n <= 4096:
        return False
    form, tiles, _, _, _ = ipmatrix.gemm_form(n, n + nu, n)
    return form == "cut" and tiles == ((n + 127) // 128) * ((n + nu + 127) // 128)


def _smallest_width(nu):
    return next(n for n in range(2, 1 << 14) if _takes_segment_unasked(n, nu))


NX = _smallest_width(50)
NX_ROWS_FAIL = 2300


def test_the_width_is_the_smallest_that_takes_the_segment_unasked():
    assert NX == 4098 and _smallest_width(7) == NX and _smallest_width(70) == NX
    # the launch that forms V_k gets 128 x 128 tiles at both widths
    for n, q in ((NX, 7), (NX, 9), (NX, 50), (NX, 51), (NX_ROWS_FAIL, 50), (NX_ROWS_FAIL, 51)):
        nslab = (n + 15) // 16 + (q + 15) // 16
        assert ipmatrix.gemm_form(n, n, 16 * nslab, lower=True, mirror=True)[0] in ("cut", "plain", "frac")
    # 2300 states: W in the cut form on 128 x 128 tiles, 124 rows in its last tile row - no room for 50 more
    assert ipmatrix.gemm_form(NX_ROWS_FAIL, NX_ROWS_FAIL + 50, NX_ROWS_FAIL)[:2] == ("cut", 18 * 19)


def _child(case, nx, fused, tmp_path):
    out = str(tmp_path / f"{case}_{nx}_{fused}.npz")
    env = dict(os.environ)
    env.pop("HQPKKT_FUSED_V", None)
    if fused is not None:
        env["HQPKKT_FUSED_V"] = str(fused)
    subprocess.run([sys.executable, os.path.join(HERE, "ctrl_rows_worker.py"), case, str(nx), out], env=env, check=True, timeout=900)
    return np.load(out)


def _d(g):
    return [g[k] for k in ("dx", "dy", "dz", "dw")]


def _against_the_model(case, nx, new, old):
    from model_staged import StagedModel
    K = len(W.CASES[case]["nu"])
    assert (new["ranks"] == old["ranks"]).all()
    assert new["asym"].max() == 0.0 and old["asym"].max() == 0.0
    prog = W.make(case, nx)
    st = W.W.state(prog)
    R = StagedModel(prog)
    R.factor(st[0], st[1])
    md = R.step(*st[2:])
    for k in range(K):
        assert new["ranks"][k, 0] == len(R.st[k]["R"]) and new["ranks"][k, 1] == len(R.st[k]["L"]), (k, new["ranks"][k])
    dn, do = rel_err(_d(new), md), rel_err(_d(old), md)
    print(f"control rows {case} at {nx}: distance to the model fused {dn:.3e}, separate {do:.3e}, floor {nx * EPS:.1e}")
    assert dn <= 2.0 * do + nx * EPS, (case, dn, do)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["u7_path2_final3", "u50_path1_xb"])
def test_default_takes_the_segment_and_is_as_close_to_the_model(case, tmp_path):
    new, old = _child(case, NX, None, tmp_path), _child(case, NX, 0, tmp_path)
    assert list(new["fused"][:3]) == [1, 1, 1] and list(new["seg"][:3]) == [1, 1, 1] and int(new["fallbacks"]) == 0, (new["fused"], new["seg"], new["fallbacks"])
    assert list(old["fused"][:3]) == [0, 0, 0] and list(old["seg"][:3]) == [0, 0, 0]
    _against_the_model(case, NX, new, old)


@pytest.mark.gpu
def test_row_condition_fails_the_thin_product_forms_the_rows(tmp_path):
    case = "u50_path1_xb"
    new, old = _child(case, NX_ROWS_FAIL, 1, tmp_path), _child(case, NX_ROWS_FAIL, 0, tmp_path)
    assert list(new["fused"][:3]) == [1, 1, 1] and list(new["seg"][:3]) == [0, 0, 0] and int(new["fallbacks"]) == 0
    _against_the_model(case, NX_ROWS_FAIL, new, old)


@pytest.mark.gpu
def test_ineligible_stage_keeps_the_separate_update_and_its_bits(tmp_path):
    """The last stage has 70 controls (K of order 70 > 64): it is the first of the backward recursion and keeps the
    separate update - its V is the old V bit for bit - and the two stages behind it take the segment unasked."""
    case = "mixed_u50_u70"
    new, old = _child(case, NX, None, tmp_path), _child(case, NX, 0, tmp_path)
    assert list(new["fused"][:3]) == [1, 1, 0] and list(new["seg"][:3]) == [1, 1, 0] and int(new["fallbacks"]) == 0
    assert list(old["fused"][:3]) == [0, 0, 0]
    assert np.array_equal(new["v_last"].view(np.int64), old["v_last"].view(np.int64))
    assert new["asym"].max() == 0.0
    dn = rel_err(_d(new), _d(old))
    print(f"control rows {case}: fused against separate {dn:.3e}")
    assert dn <= 1e-9
