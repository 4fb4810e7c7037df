"""The in-place update of the dense stage Hessians (hqpkkt_update_stage_hessians) against the only other way to make the
same change, a new hand-over of every block.  The shape of DESIGN.md section 3's measurement: 8 blocks of order 3000 (K = 7,
2992 states, 8 controls; the unpacked arena of 575.7 MB is the smallest over twice the 256 MB last-level cache), packed and
unpacked.  In one process, the handles taking turns, best of three:
  (a) 20 rank-2 updates with coefficients of alternating sign, device vectors, by wall clock between two synchronisations
  (b) one full dense hand-over of the eight Hessian blocks out of the pinned hqpkkt_stage_staging buffers (host handle)
  (c) hess_symv_timed, 20 products: the read rate of the same arena
Writes the three times, (a) / (b) and the effective rate 2 * arena bytes / (a).
python tools/hessian_update_bench.py [out.txt]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hqp_amd import _lib, ipmatrix, problems

K, NX, NU, REPS, ROUNDS = 7, 2992, 8, 20, 3
NZ = [NX + NU] * K + [NX]
up8 = lambda v: (v + 7) // 8 * 8


def docp(blocks, device):
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    F = [np.zeros((NX, NX + NU))] * K
    if device:
        Fd = torch.zeros((NX, NX + NU), dtype=torch.float64, device="cuda")
        F = [Fd] * K
    return problems.DenseDocp([NX] * (K + 1), [NU] * K, empty(sum(NZ)), empty(0), empty(0), F, 0, 0, Qd=blocks)


def handles(packed):
    """(device-vector handle for (a) and (c), host handle for (b)) with the same blocks."""
    rng = np.random.default_rng(5)
    U = rng.standard_normal((NZ[0], NZ[0]))
    host = [U] * K + [U[:NX, :NX]]  # (the upper triangle is read; the same values in every stage)
    Ud = torch.as_tensor(U).cuda()
    D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed, device_vectors=True)
    D.init_dense(docp([Ud] * K + [Ud[:NX, :NX]], True))
    Hh = ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed)
    Hh.init_dense(docp(host, False))
    return D, Hh, U


def arena_bytes(M):
    lay = M.hessian_packing()
    return 8 * int(lay[:, 2].sum()) if len(lay) else 8 * sum(v * up8(v) for v in NZ)


def time_updates(D, vecs):
    """ms per update: REPS rank-2 updates, the sign of both coefficients flipping from one to the next."""
    up = (C.c_void_p * 2)(vecs[0].data_ptr(), vecs[1].data_ptr())
    coefs = [np.ascontiguousarray(np.tile([s * 0.5, -s * 0.25], (K + 1, 1))) for s in (1.0, -1.0)]
    us = []
    for c in coefs:
        u = _lib.HessUpdate()
        u.r, u.U, u.coef = 2, C.cast(up, C.POINTER(C.c_void_p)), c.ctypes.data
        us.append(u)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(REPS):
        code = D._L.hqpkkt_update_stage_hessians(D._h, C.byref(us[i & 1]))
        assert code == 0, code
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / REPS


def time_hand_over(Hh):
    """ms of one hand-over of the K + 1 blocks out of the staging buffers (filled ahead of the clock)."""
    L = Hh._L
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, nz in enumerate(NZ):
        buf, elems = C.c_void_p(), C.c_longlong()
        code = L.hqpkkt_stage_staging(Hh._h, k & 1, C.byref(buf), C.byref(elems))
        assert code == 0 and elems.value >= nz * nz, (code, elems.value)
        code = L.hqpkkt_set_stage_hessian(Hh._h, k, buf, nz)
        assert code == 0, code
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def fill_staging(Hh, U):
    for which in (0, 1):
        buf, elems = C.c_void_p(), C.c_longlong()
        assert Hh._L.hqpkkt_stage_staging(Hh._h, which, C.byref(buf), C.byref(elems)) == 0
        view = np.ctypeslib.as_array((C.c_double * (NZ[0] * NZ[0])).from_address(buf.value))
        view[:] = U.ravel()  # (stage K reads its order's rows and columns of the same buffer with ld = its order: other values, the same bytes)


def main(out_path):
    sets = {name: handles(packed) for name, packed in (("packed", True), ("unpacked", False))}
    n = sum(NZ)
    g = torch.Generator(device="cuda").manual_seed(1)
    vecs = [torch.empty(n, dtype=torch.float64, device="cuda").uniform_(-1.0, 1.0, generator=g) for _ in range(2)]
    x = np.random.default_rng(6).standard_normal(n)
    for D, Hh, U in sets.values():
        fill_staging(Hh, U)
        time_updates(D, vecs), time_hand_over(Hh)  # (one untimed round: buffers made, code loaded)
    t = {name: {"a": [], "b": [], "c": []} for name in sets}
    for _ in range(ROUNDS):
        for name, (D, Hh, _U) in sets.items():
            t[name]["a"].append(time_updates(D, vecs))
            t[name]["b"].append(time_hand_over(Hh))
            t[name]["c"].append(D.hess_symv_timed(x, REPS)[1])
    lines = [f"hessian_update_bench: {K + 1} blocks of order {NZ[0]} (K = {K}, {NX} states, {NU} controls), {torch.cuda.get_device_name(0)}",
             f"(a) one rank-2 update in place, mean of {REPS} by wall clock; (b) one dense hand-over of the {K + 1} blocks out of the staging buffers; "
             f"(c) one product Q x, mean of {REPS} by events; {ROUNDS} rounds, the handles taking turns; ms"]
    for name, (D, _Hh, _U) in sets.items():
        a, b, c = (min(t[name][q]) for q in "abc")
        by = arena_bytes(D)
        fmt = lambda v: ", ".join(f"{q:.4f}" for q in v)
        lines += [f"{name}: arena {by / 1e6:.1f} MB",
                  f"  (a) update     {fmt(t[name]['a'])}  best {a:.4f}",
                  f"  (b) hand-over  {fmt(t[name]['b'])}  best {b:.4f}",
                  f"  (c) product    {fmt(t[name]['c'])}  best {c:.4f}",
                  f"  (a) / (b) = {a / b:.4f}; update rate 2 x arena / (a) = {2 * by / a / 1e9:.2f} TB/s; read rate arena / (c) = {by / c / 1e9:.2f} TB/s; "
                  f"update rate / read rate = {2 * c / a:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r18_hessian_update.txt"))
