"""GPU tests of hqpkkt_q_eigen_control_wide (hqp_amd/csrc/q_eigen_wide.hip.h).  The checks are tests/q_eigen_wide_worker.py, whose
docstrings have the plans and what each check covers; the worker runs once, in a child process, and prints err / bound of every
reduced block against the bound A_SHORT L 2^-53 |B|_inf + 2^-50 |T| (the largest on an MI355X: 0.194, a "full" block of order 3;
0.094 at most from order 63 on, 0.004 at 2049 and 0.003 at 2100)."""
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
    r = subprocess.run([sys.executable, os.path.join(HERE, "q_eigen_wide_worker.py")], capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Q_EIGEN_WIDE_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout)
    return json.loads(lines[-1][len("Q_EIGEN_WIDE_RESULTS "):])


@pytest.mark.parametrize("check", ["blocks", "slots_and_grids", "same_as_blocked", "nan_floors_sizes"])
def test_q_eigen_wide(outcomes, check):
    assert outcomes.get(check) == "ok", outcomes.get(check, "not run: an earlier check ended in a device error")
