"""The multistage QPs of the wide-row tests (hqpkkt_set_dense_rows; test_staged_wide_rows_cpu.py,
test_gpu_staged_wide_rows.py): inequality rows with many entries inside a stage, the threshold of every case, the
handle's options, and what numpy counts as wide rows and as H terms."""
import numpy as np

from hqp_amd import problems

W = problems.with_wide_rows


def _banded():
    return W(problems.sparse_docp(3, 300, 4, band=5, seed=21), [(0, 200, True), (1, 300, False), (1, 64, True), (3, 300, False)], seed=31)


# every case is factored by the reference's Hqp_IpLQDOCP without E_SING, and the reference and the CPU oracle of the full
# system agree within the GPU tests' bars on ip_state(prog, 3, 1.0) (checked on the CPU when the cases were written)
CASES = {
    # (one block narrower than a tile and odd; one row over states and controls)
    "one_row_nx70": lambda: W(problems.lq_docp(3, 70, 3, seed=4), [(1, 40, True)]),
    # (two tiles; 1, 15, 16 and 17 wide rows in the four stages: around the depth of a k-slab)
    "slab_edges": lambda: W(problems.lq_docp(4, 150, 4, seed=5),
                            [(0, 60, True)] + [(1, 40 + i, i % 2 == 0) for i in range(15)] + [(2, 150 - i, False) for i in range(16)] +
                            [(3, 50 + 3 * i, i % 3 == 0) for i in range(17)], seed=32),
    # (a polytopic terminal set: the mirrored product into V_K)
    "terminal_set": lambda: W(problems.lq_docp(3, 150, 4, seed=6), [(3, 150, False)] * 17, seed=33),
    # (threshold 1: the one-entry bounds are wide too; stage K has no inequality row at all)
    "every_row_wide": lambda: W(problems.lq_docp(4, 40, 3, seed=7), [(1, 25, True), (2, 40, False)], seed=34),
    "at_the_threshold": lambda: W(problems.lq_docp(3, 60, 3, seed=8), [(1, 32, False), (1, 31, False), (2, 31, True), (2, 32, True)], seed=35),
    "stages_differ": lambda: W(problems.sparse_docp(3, [60, 60, 131, 90], [3, 2, 4], band=6, seed=9),
                               [(0, 50, True), (1, 60, False), (2, 131, False), (2, 100, True), (3, 90, False), (3, 33, False)], seed=36),
    # (own and carried equality rows with wide rows that touch the controls: G_uu in the elimination)
    "with_carried_rows": lambda: W(problems.lq_docp(4, 50, 4, seed=10, path_eq=1, final_eq=3),
                                   [(k, 40 + k, True) for k in range(4)] + [(k, 54, True) for k in range(4)] + [(4, 50, False)], seed=37),
    # (the width that otherwise runs the control-sized chain on the second stream)
    "overlap_width": lambda: W(problems.sparse_docp(2, 1280, 8, band=5, seed=11, low_rank=False), [(1, 600, i % 4 == 0) for i in range(20)], seed=38),
    "banded_sparse_form": _banded,
    "banded_profile_form": _banded,
    "banded_packed_panels": _banded,
}
MIN_ENTRIES = {name: 32 for name in CASES}
MIN_ENTRIES["every_row_wide"] = 1
# the handle's other options
OPTIONS = {name: {} for name in CASES}
OPTIONS["banded_sparse_form"] = dict(a_sparse=True, dense_columns=8)
OPTIONS["banded_profile_form"] = dict(a_profile=True)
OPTIONS["banded_packed_panels"] = dict(a_profile=True, a_packed=True)
SMALL = [name for name in CASES if name != "overlap_width"]


def stage_of_rows(prog):
    """The stage (0 .. K) of every row of C, from its first column."""
    nxs, nus = prog.nx, prog.nu
    off = np.concatenate([[0], np.cumsum([nxs[k] + nus[k] for k in range(len(nus))])])
    p, i, _x = (np.asarray(a) for a in prog.C)
    return np.searchsorted(off, i[p[:-1]], side="right") - 1


def expected_wide(prog, min_entries):
    """Per stage 0 .. K the rows of C with at least min_entries stored entries, ascending."""
    stage, cnt = stage_of_rows(prog), np.diff(np.asarray(prog.C[0]))
    return [np.flatnonzero((stage == k) & (cnt >= min_entries) & (min_entries > 0)).tolist() for k in range(len(prog.nx))]


def expected_terms(prog, min_entries):
    """(kept, removed) per stage 0 .. K: the stored upper entries of Q twice, its diagonal once, and L^2 per row of C
    of L entries - in the lists for a light row, removed for a wide one."""
    K1 = len(prog.nx)
    stage, cnt = stage_of_rows(prog), np.diff(np.asarray(prog.C[0])).astype(np.int64)
    wide = (cnt >= min_entries) & (min_entries > 0)
    nxs, nus = prog.nx, prog.nu
    off = np.concatenate([[0], np.cumsum([nxs[k] + nus[k] for k in range(len(nus))])])
    qp, qi, _x = (np.asarray(a) for a in prog.Q)
    qrow = np.repeat(np.arange(prog.n), np.diff(qp))
    qstage = np.searchsorted(off, qrow, side="right") - 1
    kept = np.bincount(qstage[qi > qrow], minlength=K1) * 2 + np.bincount(qstage[qi == qrow], minlength=K1)
    kept = kept + np.bincount(stage[~wide], weights=(cnt * cnt)[~wide], minlength=K1).astype(np.int64)
    removed = np.bincount(stage[wide], weights=(cnt * cnt)[wide], minlength=K1).astype(np.int64)
    return kept.astype(np.int64), removed
