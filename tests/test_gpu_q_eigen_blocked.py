"""GPU tests of hqpkkt_q_eigen_control_blocked (hqp_amd/csrc/q_eigen_blocked.hip.h).  The checks are tests/q_eigen_blocked_worker.py,
whose docstrings have the plans and what each check covers; the worker runs once, in a child process."""
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
    r = subprocess.run([sys.executable, os.path.join(HERE, "q_eigen_blocked_worker.py")], capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Q_EIGEN_BLOCKED_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("Q_EIGEN_BLOCKED_RESULTS "):])


@pytest.mark.parametrize("check", ["blocks", "slots", "same_as_long", "nan_floors_sizes"])
def test_q_eigen_blocked(outcomes, check):
    assert outcomes.get(check) == "ok", outcomes.get(check, "not run: an earlier check ended in a device error")
