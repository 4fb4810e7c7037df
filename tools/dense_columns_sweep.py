"""From how many entries on does a column of F_k pay as a heavy column (hqpkkt_set_dense_columns)?  One MI355X.

sweep: problems.sparse_docp(K, nx, 20, band=5, low_rank=False) with sixteen state columns per stage, evenly spread, filled to
e entries each (rows from a seeded permutation, values 0.05 U(-1, 1)); hqpkkt_stats.ms_factor of a replayed factorisation
with min_entries = 0 against min_entries = e, the two handles alternating, three times each: best and worst.
headline: problems.sparse_docp(4, 5000, 50, band=5, fu_nnz=10**9, seed=2, low_rank=False) - dense control columns at the
headline width - in the three forms, ms per stage.

    python tools/dense_columns_sweep.py sweep 2000 8
    python tools/dense_columns_sweep.py sweep 5000 4
    python tools/dense_columns_sweep.py headline
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hqp_amd import ipmatrix, problems

ENTRIES = (16, 32, 64, 128, 256, 512, 1024, 2000)


def fill_columns(prog, ncols, entries, seed=99, scale=0.05):
    """`ncols` state columns of every stage, evenly spread, filled to `entries` stored entries."""
    rng = np.random.default_rng(seed)
    nxs, nus = prog.nx, prog.nu
    K = len(nus)
    off = np.concatenate([[0], np.cumsum([nxs[k] + nus[k] for k in range(K)])]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum(nxs[1:])]).astype(np.int64)
    p, i, x = (np.asarray(a) for a in prog.A)
    rows = np.repeat(np.arange(prog.me), np.diff(p))
    ar, ac, av = [rows], [i], [np.asarray(x, dtype=float)]
    for k in range(K):
        for j in (np.arange(ncols) * nxs[k] // ncols + nxs[k] // (2 * ncols)):
            col = int(off[k] + j)
            stage = np.arange(int(roff[k]), int(roff[k + 1]))
            have = rows[(i == col) & (rows >= stage[0]) & (rows <= stage[-1])]
            add = rng.permutation(np.setdiff1d(stage, have))[: max(0, min(entries, stage.size) - have.size)]
            ar.append(add), ac.append(np.full(add.size, col)), av.append(scale * rng.uniform(-1, 1, add.size))
    A = problems._csr(np.concatenate(ar), np.concatenate(ac), np.concatenate(av), prog.me)
    out = problems.Program(prog.n, prog.me, prog.m, prog.Q, A, prog.C, c=prog.c, b=prog.b, d=prog.d)
    out.nx, out.nu = nxs, nus
    return out


def time_forms(prog, handles, rounds=3):
    """{name: [ms_factor of `rounds` replayed factorisations]}, the handles alternating; and each one's residuum()."""
    st = problems.ip_state(prog, 3, 1.0)
    res = {}
    for name, M in handles.items():
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
        res[name] = M.solve(prog, *st, *d)
        M.factor(prog, st[0], st[1])
    ms = {name: [] for name in handles}
    for _ in range(rounds):
        for name, M in handles.items():
            M.factor(prog, st[0], st[1])
            if M.stats()["ms_factor"] > 0:  # (-1: the events gave no time)
                ms[name].append(M.stats()["ms_factor"])
    return ms, res


def sweep(nx, K):
    base = problems.sparse_docp(K, nx, 20, band=5, seed=2, low_rank=False)
    print(f"nx {nx}, K {K}, band 5, sixteen state columns per stage filled to e entries; ms_factor / K, best (worst) of three")
    print("      e |  min_entries = 0   |  min_entries = e   | split / unsplit")
    for e in ENTRIES + ((nx,) if nx > ENTRIES[-1] else ()):
        prog = fill_columns(base, 16, e)
        H = {"unsplit": ipmatrix.IpLQDOCP(a_sparse=True), "split": ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=e)}
        ms, res = time_forms(prog, H)
        assert all(len(h) == 16 for h in H["split"].dense_columns()), H["split"].dense_columns()
        u, s = ms["unsplit"], ms["split"]
        print(f"  {e:5d} | {min(u) / K:8.3f} ({max(u) / K:7.3f}) | {min(s) / K:8.3f} ({max(s) / K:7.3f}) | {min(s) / min(u):6.3f}"
              f"   res {res['unsplit']:.1e} {res['split']:.1e}", flush=True)
        del H


def headline():
    K = 4
    prog = problems.sparse_docp(K, 5000, 50, band=5, fu_nnz=10**9, seed=2, low_rank=False)
    H = {"dense": ipmatrix.IpLQDOCP(), "sparse": ipmatrix.IpLQDOCP(a_sparse=True), "split": ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=-1)}
    ms, res = time_forms(prog, H)
    print("nx 5000, nu 50 dense control columns, K 4, band 5; ms_factor / K, best (worst) of three; bytes_panels")
    for name, M in H.items():
        print(f"  {name:7s} {min(ms[name]) / K:8.3f} ({max(ms[name]) / K:7.3f}) ms per stage   res {res[name]:.1e}   "
              f"{M.stats()['bytes_panels'] / 1e9:.2f} GB", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "sweep":
        sweep(int(sys.argv[2]), int(sys.argv[3]))
    else:
        headline()
