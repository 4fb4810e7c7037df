"""The systems that together reach every launch kind of the tree engine's launch rule (hqp_amd/csrc/tree_plan.hpp),
shared by tests/test_tree_plan_cpu.py (the plan alone, no device), tests/test_gpu_tree_plan.py (the plan against what runs)
and tools/tree_bits.py; and the reading of a plan (IpMatrix.launch_plan()) those three need."""
from hqp_amd import ipmatrix, problems

RED, FULL = ipmatrix.IpRedSpBKP, ipmatrix.IpSpBKP


class Case:
    def __init__(self, name, cls, prog, kw=None, env=None, gpu=True):
        self.name, self.cls, self.prog, self.kw, self.env, self.gpu = name, cls, prog, kw or {}, env or {}, gpu


# (env: set before the handle is made - HQPKKT_SCHUR_BIG_B is read by the analysis, HQPKKT_SOLVE_TOP_FUSED by the upload, or
# by hqpkkt_debug_get 48 on a handle without a device; gpu=False: the plan alone - a rank of a sharded system solves nothing
# on its own)
CASES = [
    Case("banded400", RED, lambda: problems.banded_qp(400, 10, 11)),
    Case("did400_red", RED, lambda: problems.did_like_qp(400)),
    Case("did400_full", FULL, lambda: problems.did_like_qp(400)),
    # (a tree of small fronts whose update blocks pass 1 MB: they ping-pong, so the factorisation goes level by level)
    Case("banded6000_5_pingpong", RED, lambda: problems.banded_qp(6000, 5, 3), dict(leaf_size=8, upd_pingpong_mb=1)),
    Case("banded2000_full", FULL, lambda: problems.banded_qp(2000, 20, 3)),
    Case("banded2000_full_fused", FULL, lambda: problems.banded_qp(2000, 20, 3), env={"HQPKKT_SOLVE_TOP_FUSED": "1"}),
    Case("banded3000_60", RED, lambda: problems.banded_qp(3000, 60, 3)),
    Case("banded3000_60_fused", RED, lambda: problems.banded_qp(3000, 60, 3), env={"HQPKKT_SOLVE_TOP_FUSED": "1"}),
    Case("banded3000_60_big_tiles", RED, lambda: problems.banded_qp(3000, 60, 3), env={"HQPKKT_SCHUR_BIG_B": "1"}),
    Case("banded3000_70_p176", RED, lambda: problems.banded_qp(3000, 70, 3), dict(max_pivots=176)),
    Case("banded3000_80_p192", RED, lambda: problems.banded_qp(3000, 80, 3), dict(max_pivots=192)),
    Case("banded20000_8", RED, lambda: problems.banded_qp(20000, 8, 3)),
    Case("grid60x50_far", RED, lambda: problems.grid_sparse_qp(60, 50, seed=2, long_range=40), dict(ordering=1)),
    # (a level of 1028 solve slabs: the smallest banded system found with more than 1024 - n = 40000 has 2055)
    Case("banded20000_12_full", FULL, lambda: problems.banded_qp(20000, 12, 3)),
    Case("banded2000_rank1of3", RED, lambda: problems.banded_qp(2000, 20, 3), dict(shard=(1, 3, lambda *a: None)), gpu=False),
]
SWITCHES = ("HQPKKT_NO_TREE_SWEEPS", "HQPKKT_NO_SOLVE_TOP", "HQPKKT_SOLVE_TOP_FUSED")
FB_MAXP = (128, 160, 176, 192)  # pivots the instances of k_factor_blk hold
LDS_LIMIT = 160 * 1024
# every launch kind of the rule: kinds() names them
ALL_KINDS = {"small_fronts", "small_blocks", "blk0", "blk1", "blk2", "blk3", "panel_solve", "update1", "update2", "update_big",
             "fwd_small", "fwd_one", "fwd_ab", "fwd_top", "fwd_tree", "bwd_small", "bwd_ab", "tree_factor", "tree_solve_only",
             "top_ns3", "top_ns4", "top_split", "top_fused", "schedule1"}


def records(P):
    return [(w, l, R) for w in range(2) for l, R in enumerate(P["levels"][w])]


def kinds(P):
    """the launch kinds a plan holds"""
    M = ipmatrix.Hqp_IpMatrix
    k = set()
    if P["tree_factor"]:
        k.add("tree_factor")
    if P["small_tree"]:
        k.add("fwd_tree" if P["tree_factor"] else "tree_solve_only")
    if P["top_n"]:
        k |= {"top_ns%d" % P["top_ns"], "top_split" if P["top_split"] else "top_fused"}
    for w, _l, R in records(P):
        for name, on in (("small_fronts", R["fs_n"]), ("small_blocks", R["sm_n"]), ("blk%d" % R["blk_inst"], R["blk_n"]),
                         ("panel_solve", R["ps_grid"]), ("update%d" % R["su_variant"], R["su_variant"]), ("update_big", R["big_n"]),
                         ("fwd_small", R["fwd_small_n"]), ("fwd_one", R["fwd_form"] == M.FWD_ONE), ("fwd_ab", R["fwd_form"] == M.FWD_AB),
                         ("fwd_top", R["fwd_form"] == M.FWD_TOP), ("fwd_tree", R["fwd_form"] == M.FWD_TREE),
                         ("bwd_small", R["bwd_small_n"]), ("bwd_ab", R["bwd_a_grid"]), ("schedule1", w == 1 and R["n"])):
            if on:
                k.add(name)
    return k


def launches(P):
    """{kernel class of profile(): launches} of one factor() and one step() as the plan has them"""
    M = ipmatrix.Hqp_IpMatrix
    n = {"factor_diag": P["tree_factor"], "panel_solve": 0, "schur_update": 0, "solve_fwd": P["small_tree"], "solve_bwd": P["small_tree"],
         "solve_top": 0 if not P["top_n"] else 2 if P["top_split"] else 1}
    for _w, _l, R in records(P):
        n["factor_diag"] += (R["fs_n"] > 0) + (R["sm_n"] > 0) + (R["blk_n"] > 0)
        n["panel_solve"] += R["ps_grid"] > 0
        n["schur_update"] += (R["su_variant"] > 0) + (R["big_n"] > 0)
        n["solve_fwd"] += (R["fwd_small_n"] > 0) + {M.FWD_ONE: 1, M.FWD_AB: 2}.get(R["fwd_form"], 0)
        n["solve_bwd"] += (R["bwd_small_n"] > 0) + 2 * (R["bwd_a_grid"] > 0)
    return n
