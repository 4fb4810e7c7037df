"""Where does each of the three forms of the STAGED engine's stage products win on banded dynamics?  One MI355X.

problems.sparse_docp(K, nx, 20, band=b, low_rank=False) with 3 entries per control column, or with dense control columns
(fu_nnz = 10**6), on four handles: the profile form (HQPKKT_DYN_PROFILE), the same with packed panels
(hqpkkt_set_packed_panels; MB: hqpkkt_stats.bytes_panels of the two), the dense form, and the sparse form with the
library's heavy-column threshold (dense_columns=-1).  After one factor + solve and one more factorisation per handle the
handles take turns, three times: hqpkkt_stats.ms_factor of a replayed factorisation / K, and ms_step of the solve; best
(worst) of three.  share: the k-slabs inside the panels' ranges over all (panel, slab) pairs.

    python tools/profile_form_sweep.py            # states 1000, 2000, 5000; bands 1, 5, 50, 150
    python tools/profile_form_sweep.py 2000 50    # one width and band
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hqp_amd import ipmatrix, problems

STATES, BANDS, K = (1000, 2000, 5000), (1, 5, 50, 150), 4
FORMS = ("profile", "packed", "dense", "sparse")


def handles():
    return {"profile": ipmatrix.IpLQDOCP(a_profile=True), "packed": ipmatrix.IpLQDOCP(a_profile=True, a_packed=True), "dense": ipmatrix.IpLQDOCP(),
            "sparse": ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=-1)}


def time_forms(prog, H, rounds=3):
    st = problems.ip_state(prog, 3, 1.0)
    res, fac, stp = {}, {f: [] for f in H}, {f: [] for f in H}
    for name, M in H.items():
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
        res[name] = M.solve(prog, *st, *d)
        M.factor(prog, st[0], st[1])
        M.step(prog, *st, *d)
    for _ in range(rounds):
        for name, M in H.items():
            M.factor(prog, st[0], st[1])
            fac[name].append(M.stats()["ms_factor"])
            d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
            M.step(prog, *st, *d)
            stp[name].append(M.stats()["ms_step"])
    return fac, stp, res


def row(nx, band, dense_controls):
    prog = problems.sparse_docp(K, nx, 20, band=band, seed=2, low_rank=False, fu_nnz=10**6 if dense_controls else 3)
    H = handles()
    fac, stp, res = time_forms(prog, H)
    rng = H["profile"].profile_ranges()
    share = sum(int((r[:, 1] - r[:, 0]).sum()) for r in rng) / sum(len(r) * ((nx + 15) // 16) for r in rng)
    ran = int((H["profile"].dynamics_entries()[:, 1] == 2).sum())
    cells = " | ".join(f"{min(fac[f]) / K:7.3f} ({max(fac[f]) / K:7.3f}) {min(stp[f]) / K:6.3f}" for f in FORMS)
    mb = "%7.1f %7.1f" % tuple(H[f].stats()["bytes_panels"] / 2.0**20 for f in ("profile", "packed"))
    print(f"{nx:5d} {band:4d} {'dense' if dense_controls else '3/col':>6s} {share:6.3f} {ran}/{K} | {cells} | {mb} | " +
          " ".join(f"{res[f]:.0e}" for f in FORMS), flush=True)


if __name__ == "__main__":
    todo = [(int(sys.argv[1]), int(sys.argv[2]))] if len(sys.argv) > 2 else [(nx, b) for nx in STATES for b in BANDS]
    print(f"K {K}, nu 20; per form: ms_factor / K best (worst) of three, ms_step / K best; residuum() of the three forms")
    print("   nx band  fu_nnz  share  ran |        profile            |     packed panels         |         dense             |   sparse, dense_columns=-1 | MB profile, packed | res")
    for nx, band in todo:
        for dense_controls in (False, True):
            row(nx, band, dense_controls)
