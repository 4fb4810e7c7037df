"""Child process of tests/test_gpu_staged_ctrl_rows.py: one factorisation and one unrefined step() of a wide multistage QP
(tests/fused_v_worker.py's problems at a width of the caller's) by the STAGED engine under the environment the parent
has set - HQPKKT_FUSED_V is read at the upload, so every setting gets a fresh process.
python ctrl_rows_worker.py <case> <states> <out.npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import fused_v_worker as W  # noqa: E402

CASES = {
    "u7_path2_final3": W.CASES["u7_path2_final3"],
    "u50_path1_xb": dict(W.CASES["u50_path1_xb"], nu=[50, 50, 50]),
    "mixed_u50_u70": W.CASES["mixed_u50_u70"],
}


def make(case, nx):
    """fused_v_worker.make with this module's cases; that module's own table is left as it is (its test imports it in the
    same process)."""
    theirs = W.CASES
    W.CASES = dict(theirs, **CASES)
    try:
        return W.make(case, nx=nx)
    finally:
        W.CASES = theirs


if __name__ == "__main__":
    from hqp_amd import ipmatrix
    case, nx, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    prog = make(case, nx)
    st = W.state(prog)
    M = ipmatrix.IpLQDOCP()
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
    M.step(prog, *st, *d)
    K = len(CASES[case]["nu"])
    fallbacks, seg = M.ctrl_rows()
    asym = [float(np.abs(V - V.T).max()) for V in (M.stage_block(k) for k in range(K))]
    np.savez(out, dx=d[0], dy=d[1], dz=d[2], dw=d[3], fused=np.asarray(M.stages_fused()), seg=np.asarray(seg), fallbacks=fallbacks,
             asym=np.asarray(asym), v_last=M.stage_block(K - 1), ranks=M.stage_ranks())
