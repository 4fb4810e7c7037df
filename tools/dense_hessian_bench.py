"""The structure of BASELINE configs[3] (multistage LQ DOCP, K stages of nx states and nu controls, dense dynamics, x_0
fixed, box bounds on the controls) with DENSE stage Hessians (hqpkkt_set_hessian_form): Q_k = M M' / nz + diag(U(0.5, 1.5)),
M ~ U(-1, 1), generated on the device block by block and handed over through hqpkkt_set_stage_hessian.  Prints factor +
solve per second, the time of one residual and hqpkkt_stats.bytes_panels.
python tools/dense_hessian_bench.py K nx nu [reps]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hqp_amd import ipmatrix
import c4_bench


class Blocks:
    """K + 1 stage Hessians, made one at a time: the block before has been read by the engine when the next one is made."""

    def __init__(self, K, nx, nu, seed=55):
        self.K, self.nx, self.nu = K, nx, nu
        self.g = torch.Generator(device="cuda").manual_seed(seed)

    def __len__(self):
        return self.K + 1

    def __iter__(self):
        for k in range(self.K + 1):
            torch.cuda.synchronize()
            nz = self.nx + (self.nu if k < self.K else 0)
            M = torch.empty((nz, nz), dtype=torch.float64, device="cuda").uniform_(-1.0, 1.0, generator=self.g)
            B = M @ M.T
            B /= nz
            del M
            B.diagonal().add_(torch.empty(nz, dtype=torch.float64, device="cuda").uniform_(0.5, 1.5, generator=self.g))
            torch.cuda.synchronize()  # (the engine copies in its own stream)
            yield B


def run(K, nx, nu, reps=3):
    t0 = time.time()
    dq = c4_bench.make(K, nx, nu)
    dq.Qd = Blocks(K, nx, nu)
    torch.cuda.synchronize()
    t1 = time.time()
    M = ipmatrix.IpLQDOCP(device_vectors=True, q_dense=True)
    M.init_dense(dq)
    dq.F = None  # the engine holds its own copies
    torch.cuda.empty_cache()
    t2 = time.time()
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda k, lo, hi: torch.empty(k, dtype=torch.float64, device="cuda").uniform_(lo, hi, generator=g)
    n, me, m = dq.dims
    z, w = rnd(m, 0.1, 1.1), rnd(m, 0.1, 1.1)
    r = [rnd(k, -0.5, 0.5) for k in (n, me, m, m)]
    d = [torch.zeros(k, dtype=torch.float64, device="cuda") for k in (n, me, m, m)]
    out = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        ta = time.time()
        M.factor(None, z, w)
        tb = time.time()
        res = M.solve(None, z, w, *r, *d)
        tc = time.time()
        s = M.stats()
        M.residuum(None, z, w, *r, *d)
        torch.cuda.synchronize()
        td = time.time()
        if it:
            out.append((tb - ta, tc - tb, s["ms_factor"], s["ms_solve"], res, s["refine_rounds"], td - tc, M.stats()["ms_residual"]))
    med = lambda i: float(np.median([o[i] for o in out]))
    s = M.stats()
    return {"K": K, "nx": nx, "nu": nu, "n": n, "me": me, "m": m, "gen_s": round(t1 - t0, 2), "init_s": round(t2 - t1, 2),
            "factor_s": med(0), "solve_s": med(1), "factor_solve_per_s": 1.0 / (med(0) + med(1)), "ms_factor_dev": med(2), "ms_solve_dev": med(3),
            "res": out[-1][4], "refine_rounds": out[-1][5], "residual_s": med(6), "ms_residual_dev": med(7),
            "bytes_panels": s["bytes_panels"], "hessian_gb": sum((nx + (nu if k < K else 0)) * ((nx + (nu if k < K else 0) + 7) // 8 * 8) for k in range(K + 1)) * 8 / 1e9,
            "hbm_gb": (s["bytes_panels"] + s["bytes_updates"]) / 1e9}


if __name__ == "__main__":
    K, nx, nu = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    print(json.dumps(run(K, nx, nu, reps)), flush=True)
