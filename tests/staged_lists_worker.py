"""One factorisation and one solve() of a multistage QP of wide stages by the STAGED engine through the dense hand-over,
with the work lists its upload prepared (hqpkkt_debug_get 38: rows of tiles, k-slabs, form, list, hits).
tests/test_gpu_staged.py calls make() and run() in its own process, and starts this file as a fresh child process where
a switch that is read at the upload (HQPKKT_FUSED_V) has to differ; the child gets the QP its parent has made:
python staged_lists_worker.py <pickle of (dense form, state)> <out.npz>"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=1)  # (a case of 2304 states holds 200 MB; the tests that share one follow each other)
def make(nx, nu, K):
    """The QP of test_staged_mid_size_stages_against_the_tree_engine, its interior-point state and its dense form;
    nobody writes to them."""
    from hqp_amd import problems
    prog = problems.lq_docp(K, nx, nu, final_eq=2, seed=21)
    return prog, problems.ip_state(prog, 8, 1.0), problems.dense_docp_from_program(prog, [nx] * (K + 1), [nu] * K)


def run(dq, st, profile=False):
    """profile: per-class timing on, i.e. the launches go out one by one instead of as a captured graph."""
    from hqp_amd import ipmatrix
    M = ipmatrix.IpLQDOCP()
    if profile:
        M.set_profile(True)
    M.init_dense(dq)
    M.factor(None, st[0], st[1])
    d = [np.zeros(k) for k in (dq.n, dq.me, dq.m, dq.m)]
    res = M.solve(None, *st, *d)
    return dict(dx=d[0], dy=d[1], dz=d[2], dw=d[3], res=res, lists=M.debug(38).reshape(-1, 5), fused=np.asarray(M.stages_fused()))


if __name__ == "__main__":
    import pickle
    with open(sys.argv[1], "rb") as f:
        np.savez(sys.argv[2], **run(*pickle.load(f)))
