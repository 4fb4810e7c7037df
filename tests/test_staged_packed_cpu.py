"""CPU tests of the packed panels of the profile form (hqpkkt_set_packed_panels): the symbols, the setter's return codes
and call order, the layout the analysis plans (hqpkkt_debug_get 42) against numpy on the patterns of the profile form's
CPU test, and hqpkkt_stats.bytes_panels against the dense and the unpacked handle.  hqpkkt_analyze is host-only: no GPU
needed."""
import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems
from test_staged_profile_cpu import CASES, _analyze, expected_ranges


def up(x, m):
    return (x + m - 1) // m * m


def runs_profile(rng, np1):
    """a stage runs the profile sequence: at least two panels, a range shorter than all slabs of n_{k+1}"""
    return len(rng) >= 2 and bool(((rng[:, 1] - rng[:, 0]) < (np1 + 15) // 16).any())


def expected_layout(prog):
    """Per stage ((offset, ld) per panel, packed elements, dense elements) from the ranges, by the rule of the layout:
    panel p holds the rows [16 lo, min(16 hi, n+)) with ld 128, the last panel up8 of its columns, back to back; an
    empty panel takes no room; the stage's total is rounded up to 16 doubles."""
    out = []
    for k, rng in enumerate(expected_ranges(prog)):
        nz, np1 = prog.nx[k] + prog.nu[k], prog.nx[k + 1]
        dense = up(np1 * up(nz, 8), 16)
        if not runs_profile(rng, np1):
            out.append((np.tile([-1, 0], (len(rng), 1)), dense, dense))
            continue
        pan, off = [], 0
        for p, (lo, hi) in enumerate(rng):
            ld = 128 if p + 1 < len(rng) else up(nz - 128 * p, 8)
            pan.append((off, ld))
            off += (min(16 * hi, np1) - 16 * lo) * ld
        out.append((np.array(pan), up(off, 16), dense))
    return out


def test_symbols():
    L = _lib.lib()
    for sym in ("hqpkkt_set_packed_panels", "hqpkkt_debug_dgemm_packed", "hqpkkt_debug_gemv_packed", "hqpkkt_debug_carried_packed"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
    for fn in ("dgemm_packed", "gemv_packed", "carried_packed"):
        assert hasattr(ipmatrix, fn)


def test_return_codes_and_call_order():
    L = _lib.lib()
    prog = CASES["band5"]()
    assert L.hqpkkt_set_packed_panels(None, 1) == _lib.E_NULL
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):  # not a STAGED handle
        assert L.hqpkkt_set_packed_panels(cls()._h, 1) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP()
    for bad in (-1, 2, 7):
        assert L.hqpkkt_set_packed_panels(M._h, bad) == _lib.E_RANGE
    for unknown in (2, 4):  # (no new value of the dynamics form)
        assert L.hqpkkt_set_dynamics_form(M._h, unknown) == _lib.E_RANGE
    # accepted and ignored on the dense and the sparse form
    D = ipmatrix.IpLQDOCP()
    assert _analyze(D, prog) == 0
    for form in ("dense", "sparse"):
        assert L.hqpkkt_set_packed_panels(M._h, 1) == 0
        M.set_dynamics_form(form)
        assert _analyze(M, prog) == 0
        assert M.packed_panels() == [] and M.debug(42).size == 0
        if form == "dense":
            assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"]
    # it held: the profile form of the next analysis picks it up
    M.set_dynamics_form("profile")
    assert _analyze(M, prog) == 0
    assert all((p[:, 0] >= 0).all() for p in M.packed_panels())
    assert _analyze(M, prog) == 0  # (and over analyses)
    assert all((p[:, 0] >= 0).all() for p in M.packed_panels())
    M.set_packed_panels(0)
    assert _analyze(M, prog) == 0
    assert all((p == (-1, 0)).all() for p in M.packed_panels())
    assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"]
    # the profile form's other rules stand
    M.set_packed_panels(1)
    dq = problems.dense_docp_from_program(prog, list(prog.nx), list(prog.nu))
    with pytest.raises(ipmatrix.KktError) as err:
        M.init_dense(dq)
    assert err.value.code == _lib.E_INTERN
    R = ipmatrix.IpLQDOCP(a_profile=True, a_packed=True, shard=(0, 2, lambda *a: None))
    assert _analyze(R, prog) == _lib.E_RANGE


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_against_numpy(case):
    prog = CASES[case]()
    K = len(prog.nu)
    D, U, M = ipmatrix.IpLQDOCP(), ipmatrix.IpLQDOCP(a_profile=True), ipmatrix.IpLQDOCP(a_profile=True, a_packed=True)
    for h in (D, U, M):
        assert _analyze(h, prog) == 0
    want, got = expected_layout(prog), M.packed_panels()
    assert len(got) == K
    for k in range(K):
        assert np.array_equal(got[k], want[k][0]), (k, got[k], want[k][0])
        assert want[k][1] <= want[k][2]  # (never larger than the dense block)
    d = M.debug(42)
    assert np.array_equal(d[: K + 1], M.debug(41)[: K + 1])
    # the ranges and the sequences are the unpacked profile form's (item 36 keeps reporting 2)
    assert all(np.array_equal(a, b) for a, b in zip(M.profile_ranges(), U.profile_ranges()))
    assert np.array_equal(M.dynamics_entries(), U.dynamics_entries())
    # the arena: the dense handle's less the difference, exactly
    saved = sum(w[2] - w[1] for w in want)
    assert U.stats()["bytes_panels"] == D.stats()["bytes_panels"]
    assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"] - 8 * saved
    if case in ("dense", "one_panel"):
        assert saved == 0 and all((g == (-1, 0)).all() for g in got)
    if case in ("band5", "band20_odd", "stages_differ"):
        assert saved > 0
    if case == "empty_panel":  # (takes no room: the next panel would start where it does)
        assert tuple(M.profile_ranges()[1][2]) == (0, 0) and want[1][1] == up(int(got[1][2][0]), 16)
    # the unpacked profile handle reports no layout
    assert all((p == (-1, 0)).all() for p in U.packed_panels())


def test_arena_sizes_of_the_record():
    """The F arena in elements, dense -> packed, as computed from the patterns when the layout was decided."""
    table = {"band5": (280800, 164448), "band20_odd": (818928, 296048), "stages_differ": (715440, 305328)}
    for case, (dense, packed) in table.items():
        want = expected_layout(CASES[case]())
        assert (sum(w[2] for w in want), sum(w[1] for w in want)) == (dense, packed), case
    prog = problems.sparse_docp(4, 200, 3, band=5, seed=38)  # (two narrow panels)
    want = expected_layout(prog)
    assert (sum(w[2] for w in want), sum(w[1] for w in want)) == (166400, 133888)
    D, M = ipmatrix.IpLQDOCP(), ipmatrix.IpLQDOCP(a_profile=True, a_packed=True)
    assert _analyze(D, prog) == 0 and _analyze(M, prog) == 0
    assert D.stats()["bytes_panels"] - M.stats()["bytes_panels"] == 8 * (166400 - 133888)
