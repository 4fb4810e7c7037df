#!/usr/bin/env python3
"""The bits of what the entries on the dense stage Hessians (hqpkkt_set_stage_hessian .. hqpkkt_eigen_report, 13 of them)
and on the sparse Q (hqpkkt_q_values .. hqpkkt_lagrangian_gradient, 16) return and leave behind, for comparing two builds
of the library whose kernels are the same (a change of the entries' host code): run it once per library (HQPKKT_LIB
selects one, hqp_amd/_lib.py) and compare the two outputs line for line - there is no tolerance.

    python tools/hess_entry_bits.py --out bits.jsonl

One JSON line per handle: "case" (kind/shape/storage form or plugin/kind of vectors), "calls", "sha256" - over the bytes
of every vector and report every call returned and, behind every call, of every stage block as hqpkkt_debug_stage_hessian
shows it (or of hqpkkt_q_values), in the order of the calls, the code of a call that must fail in its place -, and
"entries": per entry point the first 16 digits of the sha256 over its own calls alone, which tells where two runs part,
then the codes of its calls that must fail.  The shapes are those of the GPU tests: tests/hessian_guard_cases.ORDERS on
packed and unpacked handles, the programs and plugins of tests/q_values_worker.py, host and device vectors each; for
hqpkkt_q_blocks, the BFGS update and the eigenvalue control on the sparse Q the cases of tests/q_bfgs_worker.cases() - per
program and plugin, a fresh handle for every bsize of that program - and of tests/q_eigen_cases.cases(); and DScale and
BFGS updates taking turns on one handle with one bsize.  Every line runs in a child process of its own, one at a time; a
child that fails ends the run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def to_np(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a))


def flat(out):
    if out is None:
        return []
    return list(out) if isinstance(out, (tuple, list)) else [out]


class Run:
    """The calls of one handle, each under the entry point it belongs to; the state is read behind each call (which waits
    for the handle's stream, so a device caller's results are complete when they are hashed).  done() prints the line."""

    def __init__(self, tag, device, state):
        self.tag, self.device, self.state, self.k = tag, device, state, 0
        self.all, self.per, self.codes = hashlib.sha256(), {}, {}

    def vec(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not self.device:
            return a
        import torch
        return torch.as_tensor(a).cuda()

    def call(self, entry, name, fn, fails=False):
        from hqp_amd import ipmatrix
        self.k += 1
        try:
            out = fn()
            if fails:
                raise AssertionError(f"{self.tag} {name}: accepted")
            state = list(self.state())  # (first: it waits for the handle's stream)
            arrays = [to_np(a) for a in flat(out)] + state
            data = name.encode() + b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays if a is not None)
        except ipmatrix.KktError as e:
            if not fails:
                sys.stderr.write(f"{self.tag} {name}: status {e.code}\n")
                raise
            data = f"{name} error {e.code}".encode()
            self.codes.setdefault(entry, []).append(e.code)
        self.all.update(data)
        self.per.setdefault(entry, hashlib.sha256()).update(data)

    def done(self):
        entries = {e: [h.hexdigest()[:16]] + self.codes.get(e, []) for e, h in self.per.items()}
        print(json.dumps({"case": self.tag, "calls": self.k, "sha256": self.all.hexdigest(), "entries": entries}, separators=(",", ":")), flush=True)


def dense_child(shape, packed, device):
    import hessian_guard_cases as G
    import hessian_update_cases as H
    nz = G.ORDERS[shape]
    rng = np.random.default_rng(100 + shape)
    n, off = int(sum(nz)), H.offsets(nz)
    blocks = [G.rank2_block(rng, v, 0.0) for v in nz]
    M = H.handle(packed, device_vectors=device)
    dq = H.block_docp(nz, blocks)
    if device:
        import torch
        dq.Qd = [torch.as_tensor(Q).cuda() for Q in dq.Qd]
        dq.F = [torch.as_tensor(f).cuda() for f in dq.F]
    R = Run(f"dense/{'x'.join(map(str, nz))}/{'packed' if packed else 'blocks'}/{'device' if device else 'host'}", device,
            lambda: [M.stage_hessian(k) for k in range(3)])
    v = R.vec
    x, s, y, s2 = (rng.standard_normal(n) for _ in range(4))
    y2 = -0.5 * s2 + 0.1 * rng.standard_normal(n)
    y[off[1]: off[2]] = 0.0  # (a stage that damps)
    U = [rng.uniform(-1, 1, n) for _ in range(5)]
    coef = rng.uniform(0.5, 2.0, (3, 4))
    coef[1, 2] = 0.0
    diag = rng.uniform(0.0, 1.0, n)
    R.call("set_stage_hessian", "set_stage_hessian x3", lambda: M.init_dense(dq))
    R.call("debug_stage_hessian", "stage_hessian 1", lambda: M.stage_hessian(1))
    # (the debug entries take host arrays on every handle)
    R.call("debug_hess_symv", "debug_hess_symv", lambda: M.hess_symv(x))
    R.call("debug_hess_symv_timed", "debug_hess_symv_timed", lambda: M.hess_symv_timed(x, 2)[0])
    R.call("hessian_product", "hessian_product", lambda: M.hessian_product(v(x)))
    R.call("update_stage_hessians", "update r=4 diag beta", lambda: M.update_stage_hessians([v(u) for u in U[:4]], coef, beta=[1.0, 0.5, 1.0], diag=v(diag)))
    R.call("update_stage_hessians", "update r=1", lambda: M.update_stage_hessians([v(U[4])], coef[:, :1]))
    R.call("update_stage_hessians", "update r=0 beta=0 diag", lambda: M.update_stage_hessians([], np.zeros((3, 0)), beta=[1.0, 1.0, 0.0], diag=v(1.0 + diag)))
    R.call("update_stage_hessians", "update r=5", lambda: M.update_stage_hessians([v(u) for u in U], np.ones((3, 5))), fails=True)
    R.call("update_stage_hessians", "update beta=nan", lambda: M.update_stage_hessians([], np.zeros((3, 0)), beta=[1.0, np.nan, 1.0]), fails=True)
    R.call("bfgs_report", "bfgs_report early", lambda: M.bfgs_report(), fails=True)
    R.call("eigen_control_stage_hessians", "eigen_control from_bfgs early", lambda: M.eigen_control(G.EPS, from_bfgs=True), fails=True)
    R.call("bfgs_update_stage_hessians", "bfgs want_v gamma<0", lambda: M.bfgs_update_device(v(s), v(y), gamma=-0.5, alpha=0.7, want_v=True))
    R.call("bfgs_report", "bfgs_report", lambda: M.bfgs_report())
    R.call("bfgs_update_stage_hessians", "bfgs", lambda: M.bfgs_update_device(v(s2), v(y2)))
    R.call("bfgs_report", "bfgs_report", lambda: M.bfgs_report())
    R.call("bfgs_update_stage_hessians", "bfgs gamma=nan", lambda: M.bfgs_update_device(v(s), v(y), gamma=np.nan), fails=True)
    R.call("hessian_row_stats", "row_stats", lambda: M.hessian_row_stats())
    R.call("hessian_row_stats", "row_stats sum alone", lambda: M.hessian_row_stats(want_max=False)[1])
    R.call("eigen_report", "eigen_report early", lambda: M.eigen_report(), fails=True)
    R.call("eigen_control_stage_hessians", "eigen_control from_bfgs", lambda: M.eigen_control(1.0, from_bfgs=True))
    R.call("eigen_report", "eigen_report", lambda: M.eigen_report(with_T=True))
    R.call("gerschgorin_stage_hessians", "gerschgorin", lambda: M.gerschgorin_hessians(3.0))
    R.call("gerschgorin_stage_hessians", "gerschgorin eps=0", lambda: M.gerschgorin_hessians(0.0), fails=True)
    R.call("eigen_control_stage_hessians", "eigen_control floors 5 steps", lambda: M.eigen_control(G.EPS, floor=[1e3, 2.0, 1e4], max_steps=5))
    R.call("eigen_report", "eigen_report", lambda: M.eigen_report(with_T=True))
    R.call("eigen_control_stage_hessians", "eigen_control 129 steps", lambda: M.eigen_control(G.EPS, max_steps=129), fails=True)
    R.call("eigen_control_stage_hessians", "eigen_control floor=inf", lambda: M.eigen_control(G.EPS, floor=[1.0, np.inf, 1.0]), fails=True)
    R.call("restart_stage_hessians", "restart 1,0,1", lambda: M.restart_hessians(2.0 ** -3, stages=[1, 0, 1]))
    R.call("restart_stage_hessians", "restart eps<0", lambda: M.restart_hessians(-1.0), fails=True)
    R.call("restart_stage_hessians", "restart all", lambda: M.restart_hessians(2.0 ** -12))
    blk = v(blocks[1])  # (a device block is the caller's to keep until the stream has read it)
    R.call("set_stage_hessian", "set_stage_hessian 1", lambda: M.set_stage_hessian(1, blk))
    R.call("set_stage_hessian", "set_stage_hessian 3", lambda: M.set_stage_hessian(3, blk), fails=True)
    R.call("hessian_product", "hessian_product", lambda: M.hessian_product(v(x)))
    R.done()


def dense_refused_child(packed):
    """An analysed handle no block has arrived on, and a handle of the CSR form."""
    import hessian_guard_cases as G
    import hessian_update_cases as H
    from hqp_amd import ipmatrix, problems
    nz = G.ORDERS[0]
    n = int(sum(nz))
    M = H.handle(packed)
    assert H.analyze_only(M, nz) == 0
    R = Run(f"dense-refused/{'packed' if packed else 'blocks'}", False, lambda: [])
    one = np.ones(n)
    R.call("update_stage_hessians", "update beta=1 before arrival", lambda: M.update_stage_hessians([one], np.ones((3, 1))), fails=True)
    R.call("bfgs_update_stage_hessians", "bfgs before arrival", lambda: M.bfgs_update_device(one, one), fails=True)
    R.call("hessian_row_stats", "row_stats before arrival", lambda: M.hessian_row_stats(), fails=True)
    R.call("restart_stage_hessians", "restart before arrival", lambda: M.restart_hessians(1e-3), fails=True)
    R.call("gerschgorin_stage_hessians", "gerschgorin before arrival", lambda: M.gerschgorin_hessians(1e-3), fails=True)
    R.call("eigen_control_stage_hessians", "eigen_control before arrival", lambda: M.eigen_control(1e-3), fails=True)
    R.call("hessian_product", "hessian_product before upload", lambda: M.hessian_product(one), fails=True)
    prog = problems.lq_docp(4, 3, 2)
    S = ipmatrix.IpLQDOCP()
    S.init(prog)
    one = np.ones(prog.n)
    R.call("hessian_product", "csr form: hessian_product", lambda: S.hessian_product(one), fails=True)
    R.call("update_stage_hessians", "csr form: update", lambda: S.update_stage_hessians([one], np.ones((5, 1))), fails=True)
    R.call("bfgs_update_stage_hessians", "csr form: bfgs", lambda: S.bfgs_update_device(one, one), fails=True)
    R.call("restart_stage_hessians", "csr form: restart", lambda: S.restart_hessians(1e-3), fails=True)
    R.done()


def sparse_child(problem, cls, device):
    import q_values_worker as W
    name, prog = W.programs()[problem]
    C = W.classes(name)[cls]
    n, me, m = prog.dims
    M = W.handle(C, prog, device)
    R = Run(f"sparse/{name}/{C.__name__}/{'device' if device else 'host'}", device, lambda: [to_np(M.q_values())])
    v = R.vec
    rng = np.random.default_rng(200 + problem)
    x, c, mi, d = (rng.standard_normal(n) for _ in range(4))
    y, z = rng.standard_normal(me), rng.standard_normal(m)
    s, yy, _q = W._dscale_case(prog, 5)
    R.call("q_values", "q_values", lambda: M.q_values())
    R.call("q_product", "q_product", lambda: M.q_product(v(x)))
    R.call("q_row_stats", "q_row_stats", lambda: M.q_row_stats())
    R.call("q_row_stats", "q_row_stats offsum alone", lambda: M.q_row_stats(want_diag=False)[1])
    R.call("lagrangian_gradient", "lagrangian_gradient", lambda: M.lagrangian_gradient(v(c), v(y), v(z)))
    R.call("lagrangian_gradient", "lagrangian_gradient minus", lambda: M.lagrangian_gradient(v(c), v(y), v(z), minus=v(mi)))
    R.call("q_dscale_report", "q_dscale_report early", lambda: M.q_dscale_report(), fails=True)
    for bsize in (0, 7, 64, 4096):
        R.call("q_dscale_update", f"q_dscale_update bsize={bsize}", lambda: M.q_dscale_update(v(s), v(yy), gamma=0.2, bsize=bsize, want_v=True))
        R.call("q_dscale_report", "q_dscale_report", lambda: M.q_dscale_report())
    R.call("q_dscale_update", "q_dscale_update no v", lambda: M.q_dscale_update(v(yy), v(s), bsize=7))
    R.call("q_dscale_update", "q_dscale_update gamma<0", lambda: M.q_dscale_update(v(s), v(yy), gamma=-1.0), fails=True)
    R.call("q_gerschgorin", "q_gerschgorin", lambda: M.q_gerschgorin(0.5))
    R.call("q_gerschgorin", "q_gerschgorin eps=0", lambda: M.q_gerschgorin(0.0), fails=True)
    R.call("q_dscale_setup", "q_dscale_setup", lambda: M.q_dscale_setup(1e-8))
    R.call("q_dscale_setup", "q_dscale_setup eps=nan", lambda: M.q_dscale_setup(np.nan), fails=True)
    R.call("q_set_diagonal", "q_set_diagonal", lambda: M.q_set_diagonal(v(d)))
    R.call("q_product", "q_product", lambda: M.q_product(v(x)))
    R.done()


def bfgs_groups():
    """q_bfgs_worker.cases() by program and plugin: [(name, class, [(program, bsize, pattern), ..])], a program's cases together"""
    import q_bfgs_worker as B
    out = {}
    for name, prog, classes, bsize, pattern in B.cases():
        for cls in classes:
            out.setdefault((name, cls), []).append((prog, bsize, pattern))
    return [(name, cls, runs) for (name, cls), runs in out.items()]


def sparse_bfgs_child(group, device):
    import q_bfgs_worker as B
    import q_values_worker as W
    name, cls, runs = bfgs_groups()[group]
    cur = {}
    R = Run(f"sparse-bfgs/{name}/{cls.__name__}/{'device' if device else 'host'}", device, lambda: [to_np(cur["M"].q_values())])
    v = R.vec
    for k, (prog, bsize, pattern) in enumerate(runs):
        M = cur["M"] = W.handle(cls, prog, device)
        first = B.blocks_of(prog, bsize)
        s, y = B.mixed_inputs(prog, first, 40 + k)
        s2, y2 = B.secant_inputs(prog, first, 60 + k)
        tag = f" bsize={bsize}"
        R.call("q_blocks", "q_blocks" + tag, lambda: M.q_blocks(bsize))
        R.call("q_bfgs_report", "q_bfgs_report early", lambda: M.q_bfgs_report(), fails=True)
        R.call("q_eigen_control", "q_eigen_control from_bfgs early", lambda: M.q_eigen_control(1e-3, bsize=bsize, from_bfgs=True), fails=True)
        R.call("q_bfgs_update", "q_bfgs_update" + tag, lambda: M.q_bfgs_update(v(s), v(y), bsize=bsize, pattern=pattern, want_v=True, want_Qs=True))
        R.call("q_bfgs_report", "q_bfgs_report", lambda: M.q_bfgs_report())
        R.call("q_bfgs_update", "q_bfgs_update gamma<0" + tag, lambda: M.q_bfgs_update(v(s2), v(y2), gamma=-0.5, alpha=0.7, bsize=bsize, pattern=pattern))
        R.call("q_bfgs_report", "q_bfgs_report", lambda: M.q_bfgs_report())
        R.call("q_bfgs_update", "q_bfgs_update gamma=nan", lambda: M.q_bfgs_update(v(s), v(y), gamma=np.nan, bsize=bsize, pattern=pattern), fails=True)
        R.call("q_eigen_control", "q_eigen_control from_bfgs" + tag, lambda: M.q_eigen_control(1.0, bsize=bsize, from_bfgs=True, max_steps=6))
        R.call("q_eigen_report", "q_eigen_report", lambda: M.q_eigen_report(with_T=True))
    R.done()


def eigen_groups():
    import q_eigen_cases as E
    return [(c, cls) for c in E.cases() for cls in c["classes"]]


def sparse_eigen_child(group, device):
    import q_eigen_cases as E
    import q_values_worker as W
    case, cls = eigen_groups()[group]
    prog, bsize = case["prog"], case["bsize"]
    M = W.handle(cls, prog, device)
    R = Run(f"sparse-eigen/{case['name']}/{cls.__name__}/{'device' if device else 'host'}", device, lambda: [to_np(M.q_values())])
    nb = len(case["first"]) - 1
    R.call("q_eigen_report", "q_eigen_report early", lambda: M.q_eigen_report(), fails=True)
    R.call("q_eigen_control", "q_eigen_control", lambda: M.q_eigen_control(E.EPS, bsize=bsize))
    R.call("q_eigen_report", "q_eigen_report", lambda: M.q_eigen_report(with_T=True))
    R.call("q_eigen_control", "q_eigen_control floors 5 steps", lambda: M.q_eigen_control(E.EPS, bsize=bsize, floor=np.linspace(1.0, 1e3, nb), max_steps=5))
    R.call("q_eigen_report", "q_eigen_report", lambda: M.q_eigen_report(with_T=True))
    R.call("q_eigen_report", "q_eigen_report without T", lambda: M.q_eigen_report())
    R.call("q_eigen_control", "q_eigen_control 129 steps", lambda: M.q_eigen_control(E.EPS, bsize=bsize, max_steps=129), fails=True)
    R.call("q_eigen_control", "q_eigen_control floor=inf", lambda: M.q_eigen_control(E.EPS, bsize=bsize, floor=np.full(nb, np.inf)), fails=True)
    R.call("q_eigen_control", "q_eigen_control eps=0", lambda: M.q_eigen_control(0.0, bsize=bsize), fails=True)
    R.done()


INTERLEAVED = ((65, 64), (4097, 0), (300, 7))


def sparse_interleaved_child(which, device):
    """DScale and BFGS (PATTERN) updates with one bsize taking turns on one handle, each report read behind the other's update"""
    import q_values_worker as W
    from hqp_amd import ipmatrix
    n, bsize = INTERLEAVED[which]
    prog = W.band_qp(n)
    M = W.handle(ipmatrix.IpRedSpBKP, prog, device)
    R = Run(f"sparse-interleaved/band{n}/bsize{bsize}/{'device' if device else 'host'}", device, lambda: [to_np(M.q_values())])
    v = R.vec
    for k in range(2):
        s, y, _q = W._dscale_case(prog, 70 + k)
        R.call("q_dscale_update", "q_dscale_update", lambda: M.q_dscale_update(v(s), v(y), bsize=bsize, want_v=True))
        R.call("q_bfgs_report", "q_bfgs_report", lambda: M.q_bfgs_report(), fails=k == 0)
        R.call("q_bfgs_update", "q_bfgs_update", lambda: M.q_bfgs_update(v(y), v(s), bsize=bsize, pattern=True, want_v=True, want_Qs=True))
        R.call("q_dscale_report", "q_dscale_report", lambda: M.q_dscale_report())
        R.call("q_bfgs_report", "q_bfgs_report", lambda: M.q_bfgs_report())
        R.call("q_eigen_control", "q_eigen_control from_bfgs", lambda: M.q_eigen_control(1.0, bsize=bsize, from_bfgs=True, max_steps=4))
        R.call("q_dscale_report", "q_dscale_report", lambda: M.q_dscale_report())
        R.call("q_eigen_report", "q_eigen_report", lambda: M.q_eigen_report(with_T=True))
    R.done()


def sparse_refused_child():
    """Dense stage Hessians refuse the entries on Q, the dense hand-over the gradient, a row without a diagonal the writers."""
    import q_values_worker as W
    from hqp_amd import ipmatrix, problems
    prog = problems.lq_docp(4, 3, 2)
    x = np.ones(prog.n)
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.init(prog)
    R = Run("sparse-refused", False, lambda: [])
    for name, fn in (("q_values", D.q_values), ("q_product", lambda: D.q_product(x)), ("q_row_stats", D.q_row_stats),
                     ("q_set_diagonal", lambda: D.q_set_diagonal(x)), ("q_gerschgorin", lambda: D.q_gerschgorin(1.0)),
                     ("q_dscale_setup", lambda: D.q_dscale_setup(1.0)), ("q_dscale_update", lambda: D.q_dscale_update(x, x)),
                     ("q_dscale_report", D.q_dscale_report)):
        R.call(name, "dense Hessians: " + name, fn, fails=True)
    M = ipmatrix.IpLQDOCP()
    M.init_dense(problems.dense_docp_from_program(prog, [3] * 5, [2] * 4))
    R.call("lagrangian_gradient", "dense hand-over: lagrangian_gradient", lambda: M.lagrangian_gradient(x, np.ones(prog.me), np.ones(prog.m)), fails=True)
    base = problems.banded_qp(40, 3)
    p, ix, val = (np.array(a) for a in base.Q)
    k = int(p[7])
    p[8:] -= 1
    bad = problems.Program(base.n, base.me, base.m, (p, np.delete(ix, k), np.delete(val, k)), base.A, base.C, base.c, base.b, base.d)
    B = W.handle(ipmatrix.IpRedSpBKP, bad)
    one = np.ones(bad.n)
    for name, fn in (("q_set_diagonal", lambda: B.q_set_diagonal(one)), ("q_gerschgorin", lambda: B.q_gerschgorin(1.0)),
                     ("q_dscale_setup", lambda: B.q_dscale_setup(1.0)), ("q_dscale_update", lambda: B.q_dscale_update(one, one))):
        R.call(name, "no diagonal: " + name, fn, fails=True)
    R.done()


def jobs():
    import hessian_guard_cases as G
    import q_values_worker as W
    out = [["dense", str(sh), str(int(pk)), str(int(dev))] for sh in range(len(G.ORDERS)) for pk in (1, 0) for dev in (0, 1)]
    out += [["dense-refused", str(pk)] for pk in (1, 0)]
    for q, (name, _prog) in enumerate(W.programs()):
        out += [["sparse", str(q), str(c), str(dev)] for c in range(len(W.classes(name))) for dev in (0, 1)]
    out += [["sparse-refused"]]
    out += [["sparse-bfgs", str(g), str(dev)] for g in range(len(bfgs_groups())) for dev in (0, 1)]
    out += [["sparse-eigen", str(g), str(dev)] for g in range(len(eigen_groups())) for dev in (0, 1)]
    return out + [["sparse-interleaved", str(w), str(dev)] for w in range(len(INTERLEAVED)) for dev in (0, 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=120, help="seconds a child may take")
    args = ap.parse_args()
    if args.child:
        kind, rest = args.child[0], [int(a) for a in args.child[1:]]
        return {"dense": dense_child, "dense-refused": dense_refused_child, "sparse": sparse_child, "sparse-refused": sparse_refused_child,
                "sparse-bfgs": sparse_bfgs_child, "sparse-eigen": sparse_eigen_child, "sparse-interleaved": sparse_interleaved_child}[kind](*rest)
    out = open(args.out, "w") if args.out else None
    for extra in jobs():  # a fresh process each, one at a time; the first that fails ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + extra, cwd=ROOT, stdout=subprocess.PIPE, text=True,
                           timeout=args.timeout)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out:
            out.write(r.stdout)
            out.flush()
        if r.returncode != 0:
            sys.exit(f"hess_entry_bits: {' '.join(extra)} ended with status {r.returncode}")


if __name__ == "__main__":
    main()
