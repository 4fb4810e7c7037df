"""GPU tests of hqpkkt_q_eigen_control / hqpkkt_q_eigen_report (hqp_amd/csrc/q_eigen.hip.h).  The checks themselves are
tests/q_eigen_worker.py - its docstring has the per-block checks, tests/q_eigen_cases.py the programs and the bounds; the
worker runs once, in a child process, and every test here reads its own outcome."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHECKS = ["cases", "every_outcome", "from_bfgs", "untouched", "reproducible", "handle_afterwards", "refused_and_report",
          "steps_stay_above_the_floor"]


@pytest.fixture(scope="module")
def outcomes():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "q_eigen_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Q_EIGEN_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("Q_EIGEN_RESULTS "):])


@pytest.mark.parametrize("check", CHECKS)
def test_q_eigen(outcomes, check):
    """cases: every block length 1 .. 8193, a plan of blocks of at most 64 and a mixed one, bsize -1, 0 and > 0, the three
    plugins, host and device vectors - per block the bracket honest for the reported T (exact Sturm count), eigen_replay of
    the reported T bit for bit, lambda_est against eigvalsh within rho and the allowance, Q afterwards bit for bit a twin
    handle's given fl(q_ii + d_b), the shifted block not below its floor and the shift not wasteful; T against
    q_lanczos_model within the derived bound.  every_outcome: 0, 1, 2, 3, 4 and 6 - max_steps = 1 on aligned blocks, floors
    per block, a NaN on a diagonal, s = 0 under from_bfgs.  from_bfgs: theta lowered to the reported s'Qs; the pair
    q_bfgs_update(eigen_control=eps).  untouched: NaN below the diagonal and across blocks is never read or written.
    reproducible: equal bits from call to call, over plugins and kinds of vector, and for a block of 257 wherever it lies.
    handle_afterwards: not factored; factor, step, residuum, solve and hqpkkt_mehrotra bit-identical to a fresh handle, also
    under zd_policy -1 with weak diagonals.  refused_and_report: the refused handles, HQPKKT_E_RANGE for a floor, then
    HQPKKT_E_FORMAT on a missing diagonal, the report's protocol.  steps_stay_above_the_floor: 20 updates with the control
    behind each keep every block at or above its floor."""
    assert outcomes[check] == "ok", outcomes[check]
