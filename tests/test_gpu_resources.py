"""GPU (-m gpu): every device buffer and pinned host buffer a handle allocates is freed by its owner.  The live counts
of hqpkkt_debug_get item 40 rise while handles live and are back at their baseline once the handles are destroyed."""
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_destroyed_handles_leave_no_buffers_behind():
    """In a fresh process, so that other tests' handles do not count.  A STAGED handle with a stage of 2100 states
    (from 2048 states on the solve batches its products with V: StagedDev::symv_items); a tree handle through
    hqpkkt_mehrotra (ipv, the pinned read-back words, the graphs captured on the loop's vectors) and the pinned value
    staging, analysed twice: the second analysis of the same pattern holds no more than the first."""
    code = textwrap.dedent("""
        import sys; sys.path.insert(0, %r)
        import ctypes as C, gc
        import numpy as np
        from hqp_amd import ipmatrix, problems
        probe = ipmatrix.IpRedSpBKP()  # (never analysed: item 40 is answered on any handle)
        live = lambda: tuple(int(v) for v in probe.debug(40))
        base = live()

        prog = problems.lq_docp(3, 2100, 6, final_eq=2, seed=3)
        st = problems.ip_state(prog, 6, 1.0)
        S = ipmatrix.IpLQDOCP()
        S.init(prog)
        S.factor(prog, st[0], st[1])
        d = [np.zeros(k) for k in (prog.n, prog.me, prog.m, prog.m)]
        assert S.solve(prog, *st, *d) <= 1e-10
        held = live()
        assert held[0] > base[0] and held[1] > base[1], (base, held)
        del S
        gc.collect()
        assert live() == base, ("STAGED", base, live())

        qp = problems.banded_qp(300, 8, 5)
        T = ipmatrix.IpRedSpBKP()
        counts = []
        for _ in range(2):
            T.init(qp)
            assert T.mehrotra(qp)[-1]["result"] == 0
            q, a, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert T._L.hqpkkt_values_staging(T._h, C.byref(q), C.byref(a), C.byref(c)) == 0
            counts.append(live())
        assert counts[0][0] > base[0] and counts[0][1] > base[1], (base, counts)
        assert counts[1] == counts[0], counts
        del T
        gc.collect()
        assert live() == base, ("tree", base, live())
        print("OK")
    """) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
