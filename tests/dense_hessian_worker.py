"""Child process of tests/test_gpu_staged_dense_hessian.py, for the runs that need a switch in the environment before the
library reads it (HQPKKT_FUSED_V at the upload, HQPKKT_NO_IP_SEGMENTS in the loops): the parent puts the switch into the
environment.  python dense_hessian_worker.py step <case> <out.npz>: one factorisation and one unrefined step() with the
stage Hessians as term lists (form 0) and as dense blocks (form 1); ... ip <case> <out.npz>: hqpkkt_mehrotra and
hqpkkt_franke in form 1."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FUSED_NX = 2304  # 18 tile rows: the narrowest stage whose V_k launch the rule gives 128 x 128 tiles (test in the parent)


def make(case):
    from hqp_amd import problems
    from dense_hessian_cases import CASES
    if case == "fused_width":  # (a stage wide enough to form V_k in the G_xx launch; Q_k of order 2312, and 2304)
        return problems.with_dense_hessian(problems.sparse_docp(1, FUSED_NX, 8, band=5, seed=13, low_rank=False))
    return CASES[case]()


def state(prog):
    from hqp_amd import problems
    return problems.ip_state(prog, 3, 1.0)


def step_run(M, prog, st):
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
    M.step(prog, *st, *d)
    return d


if __name__ == "__main__":
    from hqp_amd import ipmatrix
    what, case, out = sys.argv[1], sys.argv[2], sys.argv[3]
    prog = make(case)
    if what == "step":
        st = state(prog)
        K1 = len(prog.nx)
        res = {}
        for form, M in enumerate((ipmatrix.IpLQDOCP(), ipmatrix.IpLQDOCP(q_dense=True))):
            d = step_run(M, prog, st)
            V = [M.stage_block(k) for k in range(K1)]
            for nm, v in zip(("dx", "dy", "dz", "dw"), d):
                res[f"{nm}{form}"] = v
            res[f"fused{form}"] = np.asarray(M.stages_fused())
            res[f"asym{form}"] = np.asarray([float(np.abs(v - v.T).max()) for v in V])
            res[f"vmax{form}"] = np.asarray([float(np.abs(v).max()) for v in V])
            if form == 0:
                V0 = V
            else:
                res["vdiff"] = np.asarray([float(np.abs(a - b).max()) for a, b in zip(V, V0)])
        np.savez(out, **res)
    else:
        M = ipmatrix.IpLQDOCP(q_dense=True)
        M.init(prog)
        res = {}
        for nm, run in (("mehrotra", M.mehrotra), ("franke", M.franke)):
            x, y, z, w, info = run(prog)
            res.update({f"{nm}_x": x, f"{nm}_y": y, f"{nm}_z": z, f"{nm}_w": w, f"{nm}_info": np.asarray([info["result"], info["iters"]])})
        np.savez(out, **res)
