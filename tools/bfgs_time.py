"""One damped BFGS update of the dense stage Hessians, its terms formed on the host against formed on the device.
K = 8 stages of order 5050 (5000 states, 50 controls; the last block of order 5000), dense hand-over, device_vectors=True, a
packed and an unpacked handle.  Per call, each timed by wall clock from the call to a synchronisation of the device:
  (a) bfgs_update: s to the device, Q s back, hessian_update.bfgs_terms in numpy block by block, v and Q s to the device,
      the coefficients through a host array, the rank-2 update (the only path before hqpkkt_bfgs_update_stage_hessians)
  (b) bfgs_update_device: the product, k_hb_terms and the same rank-2 update, nothing on the host
Mean, median and least of REPS calls after WARM untimed ones; ROUNDS rounds, the paths and the handles taking turns.  Every
stage takes the branch without damping (y = 300 s + noise against blocks with eigenvalues of about 60 .. 340).
python tools/bfgs_time.py [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hqp_amd import ipmatrix, problems

K, NX, NU, WARM, REPS, ROUNDS = 8, 5000, 50, 3, 20, 2
NZ = [NX + NU] * K + [NX]


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
    paths = {"a": lambda D: D.bfgs_update(s, y), "b": lambda D: D.bfgs_update_device(st, yt)}
    t = {name: {p: [] for p in paths} for name in sets}
    for _ in range(ROUNDS):
        for name, D in sets.items():
            for p, call in paths.items():
                timed(lambda: call(D), WARM)
                t[name][p].append(timed(lambda: call(D), REPS))
    lines = [f"bfgs_time: {K + 1} blocks, {K} of order {NZ[0]} and one of order {NX} (K = {K}, {NX} states, {NU} controls), n = {n}, {torch.cuda.get_device_name(0)}",
             f"(a) bfgs_update: terms on the host; (b) bfgs_update_device: terms on the device; device vectors; per call by wall clock to a "
             f"synchronisation, {REPS} calls after {WARM}; {ROUNDS} rounds, paths and handles taking turns; ms"]
    for name, D in sets.items():
        assert (D.bfgs_report()[:, 7] == 0.0).all()
        lines.append(f"{name}:")
        best = {}
        for p in paths:
            for r, v in enumerate(t[name][p]):
                lines.append(f"  ({p}) round {r}: mean {np.mean(v):.4f}  median {np.median(v):.4f}  least {min(v):.4f}  most {max(v):.4f}")
            best[p] = min(np.mean(v) for v in t[name][p])
        lines.append(f"  least mean (a) {best['a']:.4f}, (b) {best['b']:.4f}; (a) / (b) = {best['a'] / best['b']:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_bfgs_device.txt"))
