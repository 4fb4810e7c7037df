"""From how many entries on does a row of C pay as a wide row (hqpkkt_set_dense_rows)?  One MI355X.

sweep: problems.sparse_docp(K, nx, 8, band=5, low_rank=False) with sixteen inequality rows of L entries in every stage
k < K (problems.with_wide_rows: random state columns, values 0.05 U(-1, 1)); hqpkkt_stats.ms_factor of a replayed
factorisation with dense_rows = 0 against dense_rows = L, the two handles taking turns, three times each: best and worst,
per stage; the seconds of init() (analysis + upload + first values) of both, and the device bytes of the H term lists
(12 per term, 12 per entry of H: the terms' indices, the entry's place and its offset into the terms).
row: the same program with ONE row over all states of stage 1 against the program without it, both with dense_rows = 32:
hqpkkt_stats.ms_solve of one solve - the vector kernels that walk a row of C with one lane (k_red_dzdw, the residual,
k_st_q's columns) see the whole row whatever the setting.

    python tools/wide_rows_sweep.py sweep 1000 2
    python tools/wide_rows_sweep.py sweep 2000 2
    python tools/wide_rows_sweep.py row 2000 2
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hqp_amd import ipmatrix, problems

ENTRIES = (8, 16, 32, 64, 128, 256, 512, 1024, 2000)
MAX_TERMS = 2 ** 31 - 1


def time_handles(prog, handles, rounds=3):
    """{name: [ms_factor of `rounds` replayed factorisations]}, the handles taking turns; each one's residuum() and the
    seconds its init() took; {name: {"step" / "residuum": [ms of `rounds` calls], "classes": {class: ms of one profiled
    step + residuum}}}."""
    st = problems.ip_state(prog, 3, 1.0)
    res, init_s = {}, {}
    for name, M in handles.items():
        t0 = time.perf_counter()
        M.init(prog)
        init_s[name] = time.perf_counter() - t0
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
    vec = {name: {"step": [], "residuum": [], "classes": {}} for name in handles}
    d = {name: [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)] for name in handles}
    for name, M in handles.items():  # (the first call captures the sequence)
        M.step(prog, *st, *d[name])
        M.residuum(prog, *st, *d[name])
    for _ in range(rounds):
        for name, M in handles.items():
            M.step(prog, *st, *d[name])
            vec[name]["step"].append(M.stats()["ms_step"])
            M.residuum(prog, *st, *d[name])
            vec[name]["residuum"].append(M.stats()["ms_residual"])
    for name, M in handles.items():
        M.set_profile(True)
        M.step(prog, *st, *d[name])
        M.residuum(prog, *st, *d[name])
        prof = M.profile()
        M.set_profile(False)
        vec[name]["classes"] = {c: prof.get(c, (0.0, 0))[0] for c in ("vector", "residual", "staged_rows_gemv")}
    return ms, res, init_s, vec


def sweep(nx, K, entries=ENTRIES):
    base = problems.sparse_docp(K, nx, 8, band=5, seed=2, low_rank=False)
    print(f"nx {nx}, K {K}, band 5, sixteen rows of L entries in every stage k < K; ms_factor / K, best (worst) of three")
    print("      L |  dense_rows = 0    |  dense_rows = L    | split / unsplit | init() s unsplit, split | term lists MB unsplit, split")
    for L in entries:
        if L > nx:
            continue
        prog = problems.with_wide_rows(base, [(k, L, False) for k in range(K) for _ in range(16)])
        terms = 16 * K * L * L
        if terms > MAX_TERMS:
            print(f"  {L:5d} | the lists would hold {terms:.2e} terms: HQPKKT_E_SIZES without the split")
            continue
        H = {"unsplit": ipmatrix.IpLQDOCP(), "split": ipmatrix.IpLQDOCP(dense_rows=L)}
        ms, res, init_s, vec = time_handles(prog, H)
        assert [len(r) for r in H["split"].dense_rows()] == [16] * K + [0], H["split"].dense_rows()
        kept = int(H["split"].h_terms()[0].sum())
        entries_h = K * min(16 * L, nx) ** 2  # (at most: the rows' columns overlap)
        u, s = ms["unsplit"], ms["split"]
        print(f"  {L:5d} | {min(u) / K:8.3f} ({max(u) / K:7.3f}) | {min(s) / K:8.3f} ({max(s) / K:7.3f}) | {min(s) / min(u):6.3f}"
              f"          | {init_s['unsplit']:7.2f} {init_s['split']:7.2f}        | <= {(12 * (kept + terms) + 12 * entries_h) / 1e6:9.1f} {12 * kept / 1e6:7.1f}"
              f"   res {res['unsplit']:.1e} {res['split']:.1e}", flush=True)
        for name in ("unsplit", "split"):
            v = vec[name]
            print(f"        {name:8s} ms: step {min(v['step']):8.3f} residuum {min(v['residuum']):8.3f} | profiled once, device ms by class: "
                  + " ".join(f"{c} {t:.3f}" for c, t in v["classes"].items()), flush=True)
        del H


def one_row(nx, K):
    base = problems.sparse_docp(K, nx, 8, band=5, seed=2, low_rank=False)
    st_of = lambda prog: problems.ip_state(prog, 3, 1.0)
    print(f"nx {nx}, K {K}: hqpkkt_stats.ms_solve of one solve, dense_rows = 32, best of three")
    for name, prog in (("without", base), ("one row over all states of stage 1", problems.with_wide_rows(base, [(1, nx, False)]))):
        M = ipmatrix.IpLQDOCP(dense_rows=32)
        M.init(prog)
        st = st_of(prog)
        M.factor(prog, st[0], st[1])
        ms = []
        for _ in range(4):
            d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
            res = M.solve(prog, *st, *d)
            ms.append(M.stats()["ms_solve"])
        print(f"  {name:36s} {min(ms[1:]):8.3f} ms   res {res:.1e}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "sweep":
        sweep(int(sys.argv[2]), int(sys.argv[3]), tuple(int(v) for v in sys.argv[4:]) or ENTRIES)
    else:
        one_row(int(sys.argv[2]), int(sys.argv[3]))
