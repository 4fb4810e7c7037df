"""Child process of tests/test_gpu_staged_fused_v.py: one factorisation and one unrefined step() of a wide multistage QP
by the STAGED engine under the HQPKKT_FUSED_V the parent has put into the environment (the switch is read at the
upload, so every setting gets a fresh process).  python fused_v_worker.py <case> <out.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NX = 3600  # 29 tile rows, 435 lower tiles of 128 x 128: the launch rule gives G_xx the 128-tile form (test below)

# controls per stage, fixed initial state, rows that fix components of x_K (carried back through the stages), random
# equality rows on (x_k, u_k) of every stage (they consume controls), upper bounds on the first states of every stage
CASES = {
    "u1_free_x0_final2": dict(nu=[1, 1, 1], x0_fixed=False, final_eq=2, path_eq=0, x_bounds=3),
    "u7_path2_final3": dict(nu=[7, 7, 7], x0_fixed=True, final_eq=3, path_eq=2, x_bounds=0),
    "u50_path1_xb": dict(nu=[50, 50, 50, 50], x0_fixed=True, final_eq=0, path_eq=1, x_bounds=40),
    "u64": dict(nu=[64, 64, 64], x0_fixed=True, final_eq=0, path_eq=0, x_bounds=0),
    # the last stage (the first of the recursion) has K of order 70 > 64: it keeps the separate update
    "mixed_u50_u70": dict(nu=[50, 50, 70], x0_fixed=True, final_eq=0, path_eq=0, x_bounds=5),
}


def make(case, nx=NX, seed=17):
    """x = [x_0, u_0, x_1, ..., x_K]; dynamics rows fx_k x_k + fu_k u_k - x_{k+1} (dense, different for every stage,
    spectral radius about 0.9), then the other equality rows; Q = 1 on states, 0.1 on controls, and couplings between
    neighbouring states and between x_k[0] and u_k[0] (entries of H off the diagonal, inside and across the tiles);
    box bounds on every control."""
    from hqp_amd import problems
    c = CASES[case]
    nu, K = c["nu"], len(c["nu"])
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([nx + m for m in nu])])  # first variable of stage k
    n = int(off[K]) + nx
    qr, qc, qv = [np.arange(n)], [np.arange(n)], [np.ones(n)]
    for k in range(K + 1):
        i = off[k] + np.arange(0, nx - 1, 7)
        qr.append(i), qc.append(i + 1), qv.append(np.full(i.size, 0.05))
        i = off[k] + np.arange(0, nx - 300, 11)
        qr.append(i), qc.append(i + 300), qv.append(np.full(i.size, -0.02))
        if k < K:
            u = off[k] + nx + np.arange(nu[k])
            qv[0][u] = 0.1
            qr.append([off[k]]), qc.append([off[k] + nx]), qv.append([0.01])
    Q = problems._csr(np.concatenate(qr), np.concatenate(qc), np.concatenate(qv), n)
    ar, ac, av = [], [], []
    rows = np.arange(nx)
    for k in range(K):
        nz = nx + nu[k]
        F = rng.uniform(-1.0, 1.0, (nx, nz))
        F[:, :nx] *= 0.9 / np.sqrt(nx / 3.0)
        ar.append(np.repeat(k * nx + rows, nz)), ac.append(off[k] + np.tile(np.arange(nz), nx)), av.append(F.ravel())
        ar.append(k * nx + rows), ac.append(off[k + 1] + rows), av.append(np.full(nx, -1.0))
    me = K * nx
    if c["x0_fixed"]:
        ar.append(me + rows), ac.append(rows), av.append(np.ones(nx))
        me += nx
    for k in range(K):
        for _ in range(c["path_eq"]):
            nz = nx + nu[k]
            ar.append(np.full(nz, me)), ac.append(off[k] + np.arange(nz)), av.append(rng.uniform(-1, 1, nz))
            me += 1
    if c["final_eq"]:
        fr = np.arange(c["final_eq"])
        ar.append(me + fr), ac.append(off[K] + fr), av.append(np.ones(fr.size))
        me += fr.size
    A = problems._csr(np.concatenate(ar), np.concatenate(ac), np.concatenate(av), me)
    ucols = np.concatenate([off[k] + nx + np.arange(nu[k]) for k in range(K)])
    cols = np.concatenate([ucols, ucols])
    vals = np.concatenate([np.ones(ucols.size), -np.ones(ucols.size)])
    if c["x_bounds"]:
        xb = np.concatenate([off[k] + np.arange(c["x_bounds"]) for k in range(1, K + 1)])
        cols, vals = np.concatenate([cols, xb]), np.concatenate([vals, -np.ones(xb.size)])
    m = cols.size
    C = problems._csr(np.arange(m), cols, vals, m)
    return problems.Program(n, me, m, Q, A, C, c=rng.uniform(-0.1, 0.1, n), b=rng.uniform(-0.1, 0.1, me), d=np.ones(m))


def state(prog):
    from hqp_amd import problems
    return problems.ip_state(prog, 4, 1.0)


if __name__ == "__main__":
    from hqp_amd import ipmatrix
    case, out = sys.argv[1], sys.argv[2]
    prog = make(case)
    st = state(prog)
    M = ipmatrix.IpLQDOCP()
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
    M.step(prog, *st, *d)
    K = len(CASES[case]["nu"])
    fused = np.asarray(M.stages_fused())
    asym = [float(np.abs(V - V.T).max()) for V in (M.stage_block(k) for k in range(K))]
    np.savez(out, dx=d[0], dy=d[1], dz=d[2], dw=d[3], fused=fused, asym=np.asarray(asym), v_last=M.stage_block(K - 1),
             ranks=M.stage_ranks())
