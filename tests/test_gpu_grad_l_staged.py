"""GPU tests of hqpkkt_lagrangian_gradient_staged (grad L on a handle of the dense hand-over; hqp_amd/csrc/staged_gradl.hip.h).
The checks themselves are tests/grad_l_staged_worker.py - its docstring has the shapes and the bounds; it runs once, in a
child process, and every test here reads its own outcome."""
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
    r = subprocess.run([sys.executable, os.path.join(HERE, "grad_l_staged_worker.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("GRAD_L_STAGED_RESULTS ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[-1][len("GRAD_L_STAGED_RESULTS "):])


@pytest.mark.parametrize("check", ["integers", "reals", "both_hand_overs", "repeatable", "no_side_effects", "refusals", "end_to_end"])
def test_grad_l_staged(outcomes, check):
    """Five shapes x (me_rest = 0, > 0) x (m = 0, > 0) x four handles (caller's ldF, host / device vectors, sparse Q /
    q_dense).  integers: bit-equal to int64 arithmetic, with and without minus.  reals: within
    (L_i + 3) 2^-53 (sum |terms|_i + |c_i|) of hessian_update.grad_l_dense_model in longdouble; with minus bit-equal to
    fl(g - minus).  both_hand_overs: the CSR hand-over's lagrangian_gradient of the same program within the sum of the two
    bounds, bit for bit on the integer data.  repeatable: two calls, and the four handles, give equal bits.
    no_side_effects: a factor + solve made before the calls gives the same bits after them, from the same factorisation and
    from a new one.  refusals: HQPKKT_E_INTERN from the new entry on handles of the CSR hand-over (STAGED, FULL, REDUCED), from
    the old entry on the dense handle.  end_to_end: g_old, new blocks, y = g_new with minus = g_old into bfgs_update_device;
    the updated blocks bit for bit those of the update replayed from the reported sums on that y."""
    assert outcomes[check] == "ok", outcomes[check]
