"""CPU: what tests/test_gpu_ip_kernels.py needs before it may launch - the references of tests/ip_kernel_refs.py agree with
hand-made cases, the reference's margin to every threshold exceeds its error bound for every seeded case of the GPU test,
the CSR programs have the row lengths the walks branch on and analyse, and the hooks refuse bad cases without a device."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix

import ip_kernel_refs as R

GAMMA, GAMMAF = 1.0e-4 ** 0.25, 0.01
MS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 65537, 70001)


def test_blocking_by_hand():
    z, w = np.array([1.0, 2.0, 1.0, 4.0]), np.array([3.0, 1.0, 5.0, 2.0])
    dz, dw = np.array([-2.0, -4.0, 1.0, 0.0]), np.array([1.0, -0.0, -10.0, -4.0])
    B = R.blocking(z, w, dz, dw)
    assert list(B) == [0.5, 0, 1.0, -2.0, 3.0, 1.0, 0.5, 2, 1.0, 1.0, 5.0, -10.0]  # equal ratios: the first index
    assert list(R.blocking(z, w, np.abs(dz), np.abs(dw))) == [1e300, -1, 0, 0, 0, 0] * 2
    assert R.ratio_stats(z, w, dz, dw) == (0.5, 0.0) and R.ratio_stats(z, w, -np.abs(dz) - 1, -np.abs(dw) - 1)[1] == 11 * 2 / 1 / 5


def test_tracked_bound_covers_double_arithmetic():
    r = R.rng_of(1)
    for _ in range(200):
        a, b, c, d = r.uniform(0.1, 2.0, 4)
        t = (R.Tr(a) * b - c) / (R.Tr(d) + a)
        assert t.close((a * b - c) / (d + a)) and t.err < 1e-14


@pytest.mark.parametrize("m", MS)
def test_margins_of_every_seeded_step_case(m):
    for kind in ("ints", "reals"):
        for seed, block in ((2, "both"), (3, "none"), (3, "z"), (3, "w"), (3, "both")):
            mm = m if seed == 2 else 777
            o = R.step_operands(kind, mm, seed, block)
            ref = R.step_ref(o, mm, GAMMA, GAMMAF, 0.5)
            assert all(v > 0.0 for v in ref["margins"].values()), (kind, mm, seed, block, ref["margins"])
            assert ref["alpha"].err < 1e-9   # (a bound that says something)
            if kind == "ints" and ref["damp"]:
                assert np.log2(ref["alpha_pre"]) % 1 == 0
                exact = float(np.sum((o["z"] + ref["alpha_pre"] * o["dz"]) * (o["w"] + ref["alpha_pre"] * o["dw"])))
                assert ref["alpha"].close(R.step_rule_f64(ref["Bk"], exact, mm, GAMMAF)[1])


def test_rows_programs_have_the_lengths_and_analyse():
    for dims in ((70, 55, 60), (70, 55, 0), (70, 0, 60)):
        prog, qlen = R.rows_program("ints", *dims, seed=15)
        n, me, m = dims
        Q = R.dense_of(prog.Q, n, n, True)
        assert np.array_equal((Q != 0).sum(1), qlen) and all(L in qlen for L in R.ROW_LENGTHS)
        mat = ipmatrix.IpSpBKP()
        mat.analyze(prog)
    prog, _ = R.rows_program("ints", 70, 55, 60, seed=15)
    for blk, rows in ((prog.A, 55), (prog.C, 60)):
        D = R.dense_of(blk, rows, 70)
        for L in R.ROW_LENGTHS:
            assert L in (D != 0).sum(1) and L in (D != 0).sum(0)


def test_hooks_refuse_before_the_device():
    L = _lib.lib()
    assert L.hqpkkt_debug_ip_vec(0, None) == _lib.E_NULL and L.hqpkkt_debug_ip_rows(None, 0, None) == _lib.E_NULL
    c = _lib.IpCase()
    for op, form, m in ((16, 0, 1), (-1, 0, 1), (2, 1, 1), (0, 1, 8193), (0, 0, 0), (9, 0, 0), (6, 0, 0)):
        c.op, c.form, c.m = op, form, m
        assert L.hqpkkt_debug_ip_vec(0, C.byref(c)) == _lib.E_RANGE, (op, form, m)
    c.op, c.form, c.m = 0, 0, 5
    assert L.hqpkkt_debug_ip_vec(0, C.byref(c)) == _lib.E_NULL
    mat = ipmatrix.IpSpBKP()
    assert L.hqpkkt_debug_ip_rows(mat._h, 0, C.byref(c)) == _lib.E_INTERN   # not analysed
    # the host's copy of the step rule needs no device
    B = np.array([0.5, 0, 1.0, -2.0, 3.0, 1.0, 1e300, -1, 0, 0, 0, 0])
    got = ipmatrix.ip_vec("host_step_rule", 0, 0, 4, Bk_in=B, sum=8.0, gammaf=GAMMAF)
    assert (got["S"][2], got["S"][5]) == R.step_rule_f64(B, 8.0, 4, GAMMAF)
