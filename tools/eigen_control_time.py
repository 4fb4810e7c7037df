"""The eigenvalue control behind a damped BFGS update of the dense stage Hessians, on the device against the only route
before hqpkkt_eigen_control_stage_hessians: reading every block back and numpy's eigvalsh.
K = 8 stages of order 5050 (5000 states, 50 controls; the last block of order 5000), dense hand-over, device_vectors=True, a
packed and an unpacked handle - tools/bfgs_time.py's shape.  Per call, each timed by wall clock from the call to a
synchronisation of the device:
  (u) bfgs_update_device alone
  (a) bfgs_update_device(eigen_control=eps): the update, then the row pass, 64 Lanczos steps over all stages (one product
      Q v and one k_he_step each), k_he_ritz and the shift, nothing on the host
  (b) bfgs_update_device, then stage_hessian(k) of every block (the read-back) and numpy.linalg.eigvalsh of each; the two
      parts are timed apart
Mean, median and least of REPS calls after WARM untimed ones for (u) and (a), ROUNDS rounds, the paths and the handles
taking turns; (b) once per handle: it takes seconds.
python tools/eigen_control_time.py [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hqp_amd import ipmatrix, problems

K, NX, NU, WARM, REPS, ROUNDS = 8, 5000, 50, 3, 20, 2
NZ = [NX + NU] * K + [NX]
EPS = 2.0 ** -10


def handle(packed, Ud):
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    Fd = torch.zeros((NX, NX + NU), dtype=torch.float64, device="cuda")
    fix = (np.arange(NX + 1, dtype=np.int32), np.arange(NX, dtype=np.int32), np.ones(NX))  # (x_0 fixed: a singleton row per component)
    dq = problems.DenseDocp([NX] * (K + 1), [NU] * K, empty(sum(NZ)), fix, empty(0), [Fd] * K, NX, 0, Qd=[Ud] * K + [Ud[:NX, :NX]])
    D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed, device_vectors=True)
    D.init_dense(dq)
    return D


def timed(call, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def read_back_route(D, st, yt):
    """(ms of the read-back, ms of eigvalsh, the smallest eigenvalue per block)"""
    D.bfgs_update_device(st, yt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    blocks = [D.stage_hessian(k)[:, :v] for k, v in enumerate(NZ)]
    t1 = time.perf_counter()
    low = [float(np.linalg.eigvalsh(B)[0]) for B in blocks]
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, low


def main(out_path):
    rng = np.random.default_rng(5)
    U = rng.standard_normal((NZ[0], NZ[0]))  # (the upper triangle is read: a symmetric matrix with eigenvalues within +-2 sqrt(order))
    U[np.diag_indices(NZ[0])] += 200.0
    Ud = torch.as_tensor(U).cuda()
    n = sum(NZ)
    s = rng.standard_normal(n)
    y = 300.0 * s + rng.standard_normal(n)
    st, yt = torch.as_tensor(s).cuda(), torch.as_tensor(y).cuda()
    sets = {name: handle(packed, Ud) for name, packed in (("packed", True), ("unpacked", False))}
    paths = {"u": lambda D: D.bfgs_update_device(st, yt), "a": lambda D: D.bfgs_update_device(st, yt, eigen_control=EPS)}
    t = {name: {p: [] for p in paths} for name in sets}
    for _ in range(ROUNDS):
        for name, D in sets.items():
            for p, call in paths.items():
                timed(lambda: call(D), WARM)
                t[name][p].append(timed(lambda: call(D), REPS))
    lines = [f"eigen_control_time: {K + 1} blocks, {K} of order {NZ[0]} and one of order {NX} (K = {K}, {NX} states, {NU} controls), n = {n}, {torch.cuda.get_device_name(0)}",
             f"(u) bfgs_update_device; (a) bfgs_update_device(eigen_control=2^-10): the control on the device, 64 Lanczos steps; (b) the update, "
             f"every block read back, numpy eigvalsh; device vectors; per call by wall clock to a synchronisation, {REPS} calls after {WARM}; "
             f"{ROUNDS} rounds, paths and handles taking turns; (b) once per handle; ms"]
    for name, D in sets.items():
        rep = D.eigen_report()
        lines.append(f"{name}: outcomes {rep[:, 9].astype(int).tolist()}, steps {rep[:, 2].astype(int).tolist()}, lambda_est of block 0 {rep[0, 6]:.6g}, rho {rep[0, 5]:.3g}")
        best = {}
        for p in paths:
            for r, v in enumerate(t[name][p]):
                lines.append(f"  ({p}) round {r}: mean {np.mean(v):.4f}  median {np.median(v):.4f}  least {min(v):.4f}  most {max(v):.4f}")
            best[p] = min(np.mean(v) for v in t[name][p])
        back, eig, low = read_back_route(D, st, yt)
        lines.append(f"  (b) read-back of {K + 1} blocks {back:.1f}, eigvalsh {eig:.1f}; smallest eigenvalue of block 0 {low[0]:.6g}")
        ctl = best["a"] - best["u"]
        lines.append(f"  least mean (u) {best['u']:.4f}, (a) {best['a']:.4f}: the control {ctl:.4f}; read-back alone / control = {back / ctl:.1f}, "
                     f"read-back + eigvalsh / control = {(back + eig) / ctl:.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_eigen_control.txt"))
