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
python tools/eigen_control_time.py [out.txt]

--exact: the exact control (hqpkkt_eigen_control_stage_hessians_exact) beside the Lanczos control (64 steps) on the same
handles - 201 stages of order 1024, 21 of order 2048, 201 of order 200, no controls, one symmetric random block (eigenvalues
within +-2 sqrt(order)) on every stage; packed and unpacked; HQPKKT_HX_ROWS 4 and 8 (read per call).  Per call by wall clock
to a synchronisation, EXACT_REPS calls after one; the outcome counts of both entries.
python tools/eigen_control_time.py --exact [out.txt]

--wide: the wide control (hqpkkt_eigen_control_stage_hessians_wide) on 21 stages of order 5050 (packed and unpacked), 8 of
order 8192, 201 of order 5050, x_0 fixed; and on 21 stages of order 2048 with HQPKKT_HW_FROM=1025 beside the exact and the
Lanczos control.  EIGEN_TIME_ONLY=201x5050 (or 21x5050, 8x8192, 21x2048) runs that shape alone.  Appends to the file.
python tools/eigen_control_time.py --wide [out.txt]

--qwide: the sparse Q's wide control (hqpkkt_q_eigen_control_wide) on plain programs (IpSpBKP) whose Q is 21 dense blocks of
order 5050, 8 of order 8192 - beside the dense stage entry (eigen_control_wide, unpacked) on the same block in the same run -
and 21 of order 2048 with HQPKKT_QEW_FROM=1 beside hqpkkt_q_eigen_control_blocked.  EIGEN_TIME_ONLY as for --wide.  Every call
by wall clock to a synchronisation and listed (the first makes the workspace).  Appends to the file.
python tools/eigen_control_time.py --qwide [out.txt]"""
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


EXACT_SHAPES, EXACT_REPS = ((201, 1024), (21, 2048), (201, 200)), 3


def main_exact(out_path):
    rng = np.random.default_rng(5)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    lines = [f"eigen_control_time --exact: eigen_control_exact beside eigen_control (64 Lanczos steps) on the same handles, {torch.cuda.get_device_name(0)}; "
             f"per call by wall clock to a synchronisation, {EXACT_REPS} calls after one; ms: mean (least)"]
    counts = lambda rep: {int(o): int((rep[:, 9] == o).sum()) for o in np.unique(rep[:, 9])}
    for stages, v in EXACT_SHAPES:
        Ud = torch.as_tensor(rng.standard_normal((v, v))).cuda()
        Fd = torch.zeros((v, v), dtype=torch.float64, device="cuda")
        for name, packed in (("packed", True), ("unpacked", False)):
            dq = problems.DenseDocp([v] * stages, [0] * (stages - 1), empty(stages * v), empty(0), empty(0), [Fd] * (stages - 1), 0, 0, Qd=[Ud] * stages)
            D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed, device_vectors=True)
            D.init_dense(dq)
            row = f"{stages} stages of order {v}, {name}:"
            for rows in (4, 8):
                os.environ["HQPKKT_HX_ROWS"] = str(rows)
                t = timed(lambda: D.eigen_control_exact(EPS), 1 + EXACT_REPS)[1:]
                row += f"  exact ROWS={rows} {np.mean(t):.2f} ({min(t):.2f})"
            del os.environ["HQPKKT_HX_ROWS"]
            out_x = counts(D.eigen_report_exact())
            t = timed(lambda: D.eigen_control(EPS), 1 + EXACT_REPS)[1:]
            lines.append(row + f"  Lanczos {np.mean(t):.2f} ({min(t):.2f});  outcomes exact {out_x}, Lanczos {counts(D.eigen_report())}")
            print(lines[-1], flush=True)
            del D
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


WIDE_SHAPES = ((21, 5050, (True, False)), (8, 8192, (False,)), (201, 5050, (True,)))


def main_wide(out_path):
    """every call timed by wall clock to a synchronisation and listed: the first makes the workspace"""
    rng = np.random.default_rng(5)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    counts = lambda rep: {int(o): int((rep[:, 9] == o).sum()) for o in np.unique(rep[:, 9])}
    ms = lambda t: " ".join(f"{x:.1f}" for x in t)

    def handle_of(stages, v, packed):
        Ud = torch.as_tensor(rng.standard_normal((v, v))).cuda()
        Fd = torch.zeros((v, v), dtype=torch.float64, device="cuda")
        fix = (np.arange(v + 1, dtype=np.int32), np.arange(v, dtype=np.int32), np.ones(v))  # (x_0 fixed: the analysis holds a free one to 4096)
        dq = problems.DenseDocp([v] * stages, [0] * (stages - 1), empty(stages * v), fix, empty(0), [Fd] * (stages - 1), v, 0, Qd=[Ud] * stages)
        D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed, device_vectors=True)
        D.init_dense(dq)
        return D

    lines = [f"eigen_control_time --wide: eigen_control_wide, {torch.cuda.get_device_name(0)}; per call by wall clock to a synchronisation, "
             f"every call listed (the first makes the workspace); ms"]
    only = os.environ.get("EIGEN_TIME_ONLY")  # (a run's time limit: one shape per run, e.g. 201x5050)
    for stages, v, layouts in WIDE_SHAPES:
        if only and only != f"{stages}x{v}":
            continue
        for packed in layouts:
            D = handle_of(stages, v, packed)
            t = timed(lambda: D.eigen_control_wide(EPS), 1 if stages > 100 else 3)
            lines.append(f"{stages} stages of order {v}, {'packed' if packed else 'unpacked'}: wide {ms(t)};  outcomes {counts(D.eigen_report_exact())}")
            print(lines[-1], flush=True)
            del D
    if not only or only == "21x2048":
        D = handle_of(21, 2048, True)
        os.environ["HQPKKT_HW_FROM"] = "1025"
        t = timed(lambda: D.eigen_control_wide(EPS), 3)
        del os.environ["HQPKKT_HW_FROM"]
        out_w = counts(D.eigen_report_exact())
        tx = timed(lambda: D.eigen_control_exact(EPS), 3)
        out_x = counts(D.eigen_report_exact())
        tl = timed(lambda: D.eigen_control(EPS), 3)
        lines.append(f"21 stages of order 2048, packed: wide (HQPKKT_HW_FROM=1025) {ms(t)};  exact {ms(tx)};  Lanczos, 64 steps {ms(tl)};  outcomes wide {out_w}, "
                     f"exact {out_x}, Lanczos {counts(D.eigen_report())}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:  # (behind the --exact lines of the same file)
        f.write(text)


QWIDE_SHAPES = ((21, 2048), (21, 5050), (8, 8192))


def block_program(stages, v, U):
    """a plain program whose Q is `stages` copies of the upper triangle of U (order v), rows ascending; two equalities, no bounds"""
    i, j = np.triu_indices(v)
    ptr = np.concatenate([[0], np.cumsum(np.tile(np.arange(v, 0, -1), stages))]).astype(np.int64)
    idx = np.concatenate([(j + b * v).astype(np.int32) for b in range(stages)])
    n = stages * v
    A = problems._csr(np.array([0, 1]), np.array([0, n - 1]), np.ones(2), 2)
    Cm = (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    return problems.Program(n, 2, 0, (ptr, idx, np.tile(U[i, j], stages)), A, Cm, c=np.zeros(n), b=np.zeros(2), d=np.zeros(0))


def main_qwide(out_path):
    rng = np.random.default_rng(5)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    counts = lambda rep: {int(o): int((rep[:, 9] == o).sum()) for o in np.unique(rep[:, 9])}
    ms = lambda t: " ".join(f"{x:.1f}" for x in t)
    lines = [f"eigen_control_time --qwide: q_eigen_control_wide on a plain program of dense blocks, {torch.cuda.get_device_name(0)}; per call by wall "
             f"clock to a synchronisation, every call listed (the first makes the workspace); ms"]
    only = os.environ.get("EIGEN_TIME_ONLY")
    for stages, v in QWIDE_SHAPES:
        if only and only != f"{stages}x{v}":
            continue
        U = rng.standard_normal((v, v))
        t0 = time.perf_counter()
        M = ipmatrix.IpSpBKP(device_vectors=True)
        M.init(block_program(stages, v, U))
        row = f"{stages} blocks of order {v} (hand-over and analysis {time.perf_counter() - t0:.0f} s):"
        if v <= 2048:
            os.environ["HQPKKT_QEW_FROM"] = "1"
        t = timed(lambda: M.q_eigen_control_wide(EPS, bsize=v), 4)
        os.environ.pop("HQPKKT_QEW_FROM", None)
        row += f"  q wide{' (HQPKKT_QEW_FROM=1)' if v <= 2048 else ''} {ms(t)}, outcomes {counts(M.q_eigen_report())}"
        if v <= 2048:
            t = timed(lambda: M.q_eigen_control_blocked(EPS, bsize=v), 4)
            row += f";  q blocked {ms(t)}, outcomes {counts(M.q_eigen_report())}"
        del M
        if v > 2048:
            Ud, Fd = torch.as_tensor(U).cuda(), torch.zeros((v, v), dtype=torch.float64, device="cuda")
            fix = (np.arange(v + 1, dtype=np.int32), np.arange(v, dtype=np.int32), np.ones(v))
            dq = problems.DenseDocp([v] * stages, [0] * (stages - 1), empty(stages * v), fix, empty(0), [Fd] * (stages - 1), v, 0, Qd=[Ud] * stages)
            D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=False, device_vectors=True)
            D.init_dense(dq)
            t = timed(lambda: D.eigen_control_wide(EPS), 3)
            row += f";  stage wide, unpacked {ms(t)}, outcomes {counts(D.eigen_report_exact())}"
            del D
        lines.append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")


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
    if "--qwide" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--qwide"]
        main_qwide(rest[0] if rest else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigen_control_time.txt"))
        sys.exit(0)
    if "--wide" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--wide"]
        main_wide(rest[0] if rest else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigen_control_time.txt"))
        sys.exit(0)
    if "--exact" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--exact"]
        main_exact(rest[0] if rest else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigen_control_time.txt"))
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_eigen_control.txt"))
