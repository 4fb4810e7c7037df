"""GPU tests of the entries on the sparse Q (hqpkkt_q_values .. hqpkkt_q_dscale_report, hqpkkt_lagrangian_gradient;
hqp_amd/csrc/q_entries.hip, q_values.hip.h).  The checks themselves are tests/q_values_worker.py - its docstring has the shapes and the
bounds; it runs once, in a child process, and every test here reads its own outcome."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def outcomes():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "q_values_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Q_VALUES_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("Q_VALUES_RESULTS "):])


@pytest.mark.parametrize("check", ["integers", "reals", "lower_entries_and_skips", "reproducible", "handle_afterwards", "refused_handles", "shared_plans"])
def test_q_values(outcomes, check):
    """integers: exact against int64.  reals: products and reported sums against longdouble, the DScale update bit for bit
    hessian_update.dscale_replay.  lower_entries_and_skips: NaN below the diagonal is never read or written; blocks with
    s = 0 (outcome 2) and with a NaN in y (outcome 3) are left alone and reach no other block.  reproducible: equal bits
    from call to call, over the three plugins, host and device vectors, and for a block wherever it lies.
    handle_afterwards: factor, step, residuum, solve and hqpkkt_mehrotra bit-identical to a fresh handle given q_values
    by hqpkkt_set_values; not factored after a write; zd_policy -1 with diagonals made weak.  refused_handles:
    HQPKKT_E_INTERN on the dense hand-over and on dense stage Hessians, HQPKKT_E_FORMAT by the diagonal rule.
    shared_plans: a DScale and a BFGS update with one bsize share a partition and keep their reports apart; the DScale
    update's bits are those of a handle that never made a BFGS update."""
    assert outcomes[check] == "ok", outcomes[check]
