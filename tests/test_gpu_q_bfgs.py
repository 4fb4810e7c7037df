"""GPU tests of hqpkkt_q_blocks / hqpkkt_q_bfgs_update / hqpkkt_q_bfgs_report (hqp_amd/csrc/q_bfgs.hip.h).  The checks themselves
are tests/q_bfgs_worker.py - its docstring has the programs and the bounds; it runs once, in a child process, and every
test here reads its own outcome."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = ["integers", "reals", "product_bits", "secant", "untouched_and_skips", "reproducible", "handle_afterwards", "refused_handles"]


@pytest.fixture(scope="module")
def outcomes():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "q_bfgs_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Q_BFGS_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("Q_BFGS_RESULTS "):])


@pytest.mark.parametrize("check", CHECKS)
def test_q_bfgs(outcomes, check):
    """integers: Qs, sy and sQs exact against int64.  reals: Qs and the reported sums against longdouble, everything behind
    them bit for bit hessian_update.q_bfgs_replay.  product_bits: without entries across blocks Qs has the bits of
    q_product(s).  secant: Q+ s = v on every updated block within the derived bound.  untouched_and_skips: NaN below the
    diagonal and across blocks is never read or written; blocks with s = 0 (outcome 2) and with a NaN in y (outcome 3) are
    left alone and reach no other block; HQPKKT_E_FORMAT under FULL where one entry is missing.  reproducible: equal bits
    from call to call, over the plugins, host and device vectors, and for a block of 257 wherever it lies.
    handle_afterwards: not factored after the update; factor, step, residuum, solve and hqpkkt_mehrotra bit-identical to a
    fresh handle given q_values by hqpkkt_set_values, also under zd_policy -1 with weak diagonals.  refused_handles:
    HQPKKT_E_INTERN on dense stage Hessians, before values and for the report before an update; HQPKKT_E_RANGE on a short cap."""
    assert outcomes[check] == "ok", outcomes[check]
