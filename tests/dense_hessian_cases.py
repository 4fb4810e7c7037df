"""The multistage QPs of the dense-Hessian tests (hqpkkt_set_hessian_form; test_staged_dense_hessian_cpu.py,
test_gpu_staged_dense_hessian.py): every stage block of Q a dense SPD matrix (problems.with_dense_hessian), the handle's
options of every case, and what numpy counts as layout and as H terms left in the lists."""
import numpy as np

from hqp_amd import problems

H = problems.with_dense_hessian


def _banded():
    return H(problems.sparse_docp(3, 300, 4, band=5, seed=21))


# every case is factored by the reference's Hqp_IpLQDOCP without E_SING on ip_state(prog, 3, 1.0); the reference and the CPU
# oracle of the full system agree to 8e-14 relative there, both residuals <= 1e-11 (checked on the CPU when the cases were
# written)
CASES = {
    "nx70": lambda: H(problems.lq_docp(3, 70, 3, seed=4)),
    "nx150": lambda: H(problems.lq_docp(4, 150, 4, seed=5)),
    "order_128": lambda: H(problems.lq_docp(3, 124, 4, seed=6)),
    "order_129": lambda: H(problems.lq_docp(2, 126, 3, seed=7)),
    "stages_differ": lambda: H(problems.sparse_docp(3, [60, 60, 131, 90], [3, 2, 4], band=6, seed=9)),
    "with_carried_rows": lambda: H(problems.lq_docp(4, 50, 4, seed=10, path_eq=1, final_eq=3)),
    "free_x0": lambda: H(problems.lq_docp(3, 40, 3, seed=11, x0_fixed=False)),
    "x_bounds": lambda: H(problems.lq_docp(3, 64, 4, seed=12, x_bounds=5)),
    "wide_rows": lambda: H(problems.with_wide_rows(problems.lq_docp(3, 150, 4, seed=6), [(3, 150, False)] * 17 + [(1, 60, True)], seed=33)),
    "banded_sparse_form": _banded,
    "banded_profile_form": _banded,
    "banded_packed_panels": _banded,
}
# the handle's other options
OPTIONS = {name: {} for name in CASES}
OPTIONS["wide_rows"] = dict(dense_rows=32)
OPTIONS["banded_sparse_form"] = dict(a_sparse=True, dense_columns=8)
OPTIONS["banded_profile_form"] = dict(a_profile=True)
OPTIONS["banded_packed_panels"] = dict(a_profile=True, a_packed=True)
# the cases the dense hand-over of the dynamics takes (the sparse and the profile form walk the CSR rows)
DENSE_HANDOVER = [name for name in CASES if not name.startswith("banded")]

up8 = lambda v: (v + 7) // 8 * 8


def orders(prog):
    """Order of Q_k per stage 0 .. K."""
    return [prog.nx[k] + prog.nu[k] for k in range(len(prog.nu))] + [prog.nx[-1]]


def arena_bytes(prog):
    return 8 * sum(nz * up8(nz) for nz in orders(prog))


def terms_left(prog, min_entries=0):
    """H terms per stage 0 .. K that stay in the lists with dense Hessians: L^2 per row of C of L entries that is not wide."""
    K1 = len(prog.nx)
    off = np.concatenate([[0], np.cumsum(orders(prog))])
    p, i, _x = (np.asarray(a) for a in prog.C)
    stage = np.searchsorted(off, i[p[:-1]], side="right") - 1
    cnt = np.diff(p).astype(np.int64)
    light = ~((cnt >= min_entries) & (min_entries > 0))
    return np.bincount(stage[light], weights=(cnt * cnt)[light], minlength=K1).astype(np.int64)


def padded(blocks):
    """The blocks as they lie in the arena: order x up8(order), zero padded."""
    out = []
    for B in blocks:
        P = np.zeros((B.shape[0], up8(B.shape[0])))
        P[:, : B.shape[0]] = B
        out.append(P)
    return out


def kkt_row_bound(prog, st, d):
    """max_i sum_j |K_ij| |d_j| over the rows of the Newton system [Q -A' -C'; A; C -I; Z W] at the vectors d = (dx, dy,
    dz, dw): what one rounding of every product in a row of the residual is measured against."""
    z, w = st[0], st[1]
    dx, dy, dz, dw = (np.abs(v) for v in d)

    def rows_of(csr):
        p, i, x = (np.asarray(a) for a in csr)
        return np.repeat(np.arange(len(p) - 1), np.diff(p)), i, np.abs(np.asarray(x, dtype=float))

    qr, qc, qv = rows_of(prog.Q)
    up = qc >= qr
    qr, qc, qv = qr[up], qc[up], qv[up]
    off = qc > qr
    r1 = np.bincount(qr, weights=qv * dx[qc], minlength=prog.n) + np.bincount(qc[off], weights=qv[off] * dx[qr[off]], minlength=prog.n)
    ar, ac, av = rows_of(prog.A)
    r1 += np.bincount(ac, weights=av * dy[ar], minlength=prog.n)
    r2 = np.bincount(ar, weights=av * dx[ac], minlength=prog.me)
    cr, cc, cv = rows_of(prog.C)
    r1 += np.bincount(cc, weights=cv * dz[cr], minlength=prog.n)
    r3 = np.bincount(cr, weights=cv * dx[cc], minlength=prog.m) + dw
    r4 = np.abs(z) * dw + np.abs(w) * dz
    return max(float(v.max(initial=0.0)) for v in (r1, r2, r3, r4))
