#!/usr/bin/env python3
"""The bits of what hqpkkt_mehrotra and hqpkkt_franke return, for comparing two builds of the library whose kernels are
the same (a change of the loops' host code): run it once per library (HQPKKT_LIB selects one, hqp_amd/_lib.py) and
compare the two outputs line for line - there is no tolerance.

    python tools/ip_loop_bits.py --out bits.jsonl

One short JSON line per call: "case" (setting/problem/number of the call, the handle, the loop and its arguments), "xyzw"
(sha256 of the bytes of x, y, z, w, in this order), "r" (result, iters, n_factor, n_solve, attempts) and "bits" (the bit
patterns of gap, mu, phi, alpha, pcost, in this order).  Every (switch setting, problem) pair runs in a child process of its own, one at a time:
HQPKKT_TINY_IN_LOOP is read once per process, and the calls on one problem share handles on purpose (replayed graphs,
hot starts).  A last child prints the launches per kernel class of one call of each loop with the profile on (which
turns the segment graphs off: the launch-by-launch path), and of the one residuum() call behind it that makes the handle
sum its events up.  A child that fails ends the run."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = {"none": {}, "no_ip_small": {"HQPKKT_NO_IP_SMALL": "1"}, "no_ip_segments": {"HQPKKT_NO_IP_SEGMENTS": "1"},
            "franke_two_reads": {"HQPKKT_FRANKE_TWO_READS": "1"}, "tiny_in_loop_1": {"HQPKKT_TINY_IN_LOOP": "1"},
            "tiny_in_loop_0": {"HQPKKT_TINY_IN_LOOP": "0"}}
SWITCHES = sorted({k for env in SETTINGS.values() for k in env})
PROBLEMS = ["banded300", "did400", "lq40", "banded2000_full", "docp_csr", "docp_dense", "docp_dense_hessian", "no_inequalities",
            "duplicated_equality"]
DOCP = dict(K=8, nx=40, nu=5)


def handle(problem):
    """(a fresh, initialised handle; the QP)"""
    from hqp_amd import ipmatrix, problems
    from test_reference_host import _duplicated_equality, _without_inequalities
    if problem.startswith("docp"):
        prog = problems.lq_docp(DOCP["K"], DOCP["nx"], DOCP["nu"], final_eq=3)
        M = ipmatrix.IpLQDOCP(q_dense=problem == "docp_dense_hessian")
        if problem == "docp_csr":
            M.init(prog)
        else:
            M.init_dense(problems.dense_docp_from_program(prog, [DOCP["nx"]] * (DOCP["K"] + 1), [DOCP["nu"]] * DOCP["K"],
                                                          dense_hessian=problem == "docp_dense_hessian"))
        return M, prog
    prog = {"banded300": lambda: problems.banded_qp(300, 8, 5), "did400": lambda: problems.did_like_qp(400),
            "lq40": lambda: problems.lq_docp(40, 6, 2, final_eq=2), "banded2000_full": lambda: problems.banded_qp(2000, 20, 3),
            "no_inequalities": lambda: _without_inequalities(problems.banded_qp(400, 10, 6)),
            "duplicated_equality": lambda: _duplicated_equality(problems.banded_qp(60, 6, 5))}[problem]()
    M = (ipmatrix.IpSpBKP if problem == "banded2000_full" else ipmatrix.IpRedSpBKP)()
    M.init(prog)
    return M, prog


def calls(problem):
    """[(name of the handle, loop, keyword arguments)]: calls with the same handle name share a handle, in this order"""
    plain = [("a", "mehrotra", {}), ("a", "franke", dict(max_iters=300))]
    if problem in ("no_inequalities", "duplicated_equality"):
        return plain
    return plain + [("a", "mehrotra", {}), ("a", "franke", dict(max_iters=300))] + \
        [("a", "mehrotra", dict(init_method=k)) for k in (1, 2, 3)] + [("a", "franke", dict(max_iters=300, qp_mu0=1e-3))] + \
        [("hot", loop, dict(hot_start=hs, **kw)) for loop, kw in (("mehrotra", {}), ("franke", dict(max_iters=300))) for hs in (2, 1)] + \
        [("cap", "mehrotra", dict(max_iters=3)), ("cap", "franke", dict(max_iters=3))]


def bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def child(setting, problem):
    from hqp_amd import ipmatrix
    handles = {}
    for k, (name, loop, kw) in enumerate(calls(problem)):
        args = " ".join(f"{a}={v}" for a, v in sorted(kw.items()))
        line = {"case": f"{setting}/{problem}/{k:02d} {name} {loop} {args}".rstrip()}
        try:
            if name not in handles:
                handles[name] = handle(problem)
            M, prog = handles[name]
            x, y, z, w, info = getattr(M, loop)(prog, **kw)
            line["xyzw"] = hashlib.sha256(b"".join(a.tobytes() for a in (x, y, z, w))).hexdigest()
            line["r"] = [info[k2] for k2 in ("result", "iters", "n_factor", "n_solve", "attempts")]
            line["bits"] = " ".join(bits(info[k2]) for k2 in ("gap", "mu", "phi", "alpha", "pcost"))
        except ipmatrix.KktError as e:
            line["error"] = e.code
        print(json.dumps(line, separators=(",", ":")), flush=True)


def launch_counts():
    from hqp_amd import ipmatrix, problems
    prog = problems.did_like_qp(400)
    for loop, kw in (("mehrotra", {}), ("franke", dict(max_iters=300))):
        M = ipmatrix.IpRedSpBKP()
        M.init(prog)
        M.set_profile(True)
        x, y, z, w, info = getattr(M, loop)(prog, **kw)
        # (the loops leave their events with the handle; the next plain call sums them up: one residual launch more)
        M.residuum(prog, *problems.ip_state(prog, seed=1), x, y, z, w)
        print(json.dumps({"launch_counts": loop, "problem": "did400", "iters": info["iters"], "result": info["result"],
                          "launches": {k: n for k, (_ms, n) in sorted(M.profile().items()) if n}}, separators=(",", ":")), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--child", nargs=2, metavar=("SETTING", "PROBLEM"), help=argparse.SUPPRESS)
    ap.add_argument("--launch-counts", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=120, help="seconds a child may take")
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if args.launch_counts:
        return launch_counts()
    out = open(args.out, "w") if args.out else None
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    jobs = [(dict(base, **env), ["--child", s, p]) for s, env in SETTINGS.items() for p in PROBLEMS] + [(base, ["--launch-counts"])]
    for env, extra in jobs:  # a fresh process each, one at a time; the first that fails ends the run
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                           text=True, timeout=args.timeout)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if out:
            out.write(r.stdout)
            out.flush()
        if r.returncode != 0:
            sys.exit(f"ip_loop_bits: {' '.join(extra)} ended with status {r.returncode}")


if __name__ == "__main__":
    main()
