#!/usr/bin/env python3
"""The bits of what the tree engine computes, for comparing two builds of the library whose kernels and launches are the
same (a change of tree.hip's host code): run it once per library (HQPKKT_LIB selects one, hqp_amd/_lib.py) and compare
the two outputs line for line - there is no tolerance.

    python tools/tree_bits.py --out bits.jsonl

Over the table of tests/tree_cases.py x {host vectors, device vectors} x the switches below: factor + solve twice in a
row on one handle (the second pair replays the captured graphs), one JSON line after each pair: "case", "d" (sha256 of
the bytes of dx, dy, dz, dw, in this order), "res" (the bit pattern of the residual), "st" (n_2x2, n_perturbed,
refine_rounds) and "root" (sha256 of the root front's panel and M, hqpkkt_debug_read 0 and 1).  Every (switch, case) pair
runs in a child process of its own, one at a time, under a time limit; a child that fails ends the run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ip_loop_bits import bits  # noqa: E402

SETTINGS = {"none": {}, **{k.lower()[7:]: {k: "1"} for k in (
    "HQPKKT_NO_SOLVE_TOP", "HQPKKT_NO_TREE_SWEEPS", "HQPKKT_SOLVE_TOP_FUSED", "HQPKKT_NO_FUSED_VECTORS", "HQPKKT_NO_DIRECT_VECTORS",
    "HQPKKT_NO_HOST_GRAPHS")}}
SWITCHES = sorted({k for env in SETTINGS.values() for k in env})


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


def child(setting, name):
    import tree_cases as tc
    from hqp_amd import problems
    case = next(c for c in tc.CASES if c.name == name)
    prog = case.prog()
    st = problems.ip_state(prog, 3, 1.0)
    for vectors in ("host", "device"):
        M = case.cls(device_vectors=vectors == "device", **case.kw)
        M.init(prog)
        root = int(np.flatnonzero(M.structure()["parent"] < 0)[-1])
        if vectors == "device":
            import torch
            vin = [torch.as_tensor(v).cuda() for v in st]
            d = [torch.zeros(k, dtype=torch.float64, device="cuda") for k in (prog.n, prog.me, prog.m, prog.m)]
        else:
            vin, d = st, [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
        for rep in range(2):
            M.factor(prog, vin[0], vin[1])
            res = M.solve(prog, *vin, *d)
            s = M.stats()
            out = [v.cpu().numpy() if vectors == "device" else v for v in d]
            print(json.dumps({"case": f"{setting}/{name}/{vectors}/{rep}", "d": sha(*out), "res": bits(res),
                              "st": [s["n_2x2"], s["n_perturbed"], s["refine_rounds"]],
                              "root": sha(M.read_block(0, root), M.read_block(1, root))}, separators=(",", ":")), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the lines to this file")
    ap.add_argument("--child", nargs=2, metavar=("SETTING", "CASE"), help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=int, default=120, help="seconds a child may take")
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    import tree_cases as tc
    out = open(args.out, "w") if args.out else None
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for setting, env in SETTINGS.items():  # a fresh process each, one at a time; the first that fails ends the run
        for case in tc.CASES:
            if not case.gpu:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", setting, case.name], env={**base, **case.env, **env},
                               cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if out:
                out.write(r.stdout)
                out.flush()
            if r.returncode != 0:
                sys.exit(f"tree_bits: {setting} {case.name} ended with status {r.returncode}")


if __name__ == "__main__":
    main()
