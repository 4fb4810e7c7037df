"""The multistage QPs of the heavy-column tests (hqpkkt_set_dense_columns; test_staged_dense_columns_cpu.py,
test_gpu_staged_dense_columns.py): sparse state coupling with a few full columns, and what numpy counts as heavy."""
import numpy as np

from hqp_amd import problems

BIG = 10**9  # fu_nnz: every control column full

# every case is factored by the reference's Hqp_IpLQDOCP without E_SING (checked on the CPU when the cases were written)
CASES = {
    "dense_fu_nx40": lambda: problems.sparse_docp(6, 40, 3, band=5, fu_nnz=BIG),
    "dense_fu_nx130": lambda: problems.sparse_docp(4, 130, 4, band=5, fu_nnz=BIG, seed=5),
    "dense_fu_odd_nx": lambda: problems.sparse_docp(5, 43, 3, band=3, fu_nnz=BIG, seed=7),  # (odd leading dimensions: the 16-byte stores)
    "dense_fu_stages_differ": lambda: problems.sparse_docp(5, [40, 40, 37, 52, 45, 31], [3, 2, 4, 1, 3], band=4, fu_nnz=BIG, seed=6),
    "dense_fu_final_eq": lambda: problems.sparse_docp(7, 40, 3, band=4, final_eq=7, fu_nnz=BIG, seed=8),  # (carried rows x heavy columns)
    "dense_fu_path_eq_free_x0": lambda: problems.sparse_docp(6, 40, 4, band=3, path_eq=2, x_bounds=5, x0_fixed=False, fu_nnz=BIG, seed=9),
    "state_cols_first_mid_last": lambda: problems.with_dense_columns(
        problems.sparse_docp(6, 40, 3, band=2, seed=14), [(k, j) for k in range(6) for j in (0, 17, 39)]),
    # (stages with and without heavy columns of their own; a state and a control column)
    "state_cols_some_stages": lambda: problems.with_dense_columns(
        problems.sparse_docp(6, 48, 4, band=5, path_eq=1, path_eq_every=2, final_eq=3, x_bounds=4, seed=10), [(1, 5), (1, 6), (4, 47), (4, 50)]),
    # (nd = 9: not a multiple of 8; runs, singles, the boundary between states and controls)
    "nine_cols_nx130": lambda: problems.with_dense_columns(
        problems.sparse_docp(4, 130, 4, band=1, seed=4), [(k, j) for k in range(4) for j in (3, 4, 5, 64, 65, 129, 130, 131, 133)]),
    "all_dense": lambda: problems.sparse_docp(4, 40, 3, dense=True, seed=11),  # (no light column at all)
}
MIN_ENTRIES = {name: 8 for name in CASES}
MIN_ENTRIES["all_dense"] = 1


def expected_heavy(prog, min_entries):
    """Per stage the columns of F_k (local: states, then controls) with at least min_entries stored entries in the
    stage's dynamics rows, from the CSR arrays of A alone."""
    nxs, nus = prog.nx, prog.nu
    K = len(nus)
    off = np.concatenate([[0], np.cumsum([nxs[k] + nus[k] for k in range(K)])])
    roff = np.concatenate([[0], np.cumsum(nxs[1:])])
    p, i, _x = (np.asarray(a) for a in prog.A)
    rows = np.repeat(np.arange(prog.me), np.diff(p))
    out = []
    for k in range(K):
        nz = nxs[k] + nus[k]
        sel = (rows >= roff[k]) & (rows < roff[k + 1]) & (i >= off[k]) & (i < off[k] + nz)
        cnt = np.bincount(i[sel] - off[k], minlength=nz)
        out.append(np.flatnonzero(cnt >= min_entries).tolist() if min_entries > 0 else [])
    return out
