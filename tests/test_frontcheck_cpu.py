"""CPU: the checker of tests/frontcheck.py on its own - no GPU.

The host analysis runs without a device (as in tests/test_host_abi.py); the factors come from frontcheck.ModelSource, a
float64 front-by-front factorisation with the pivoting of tests/model.py in the device's layout.  Clean factors must stay
inside every bound (the reference alone: what the bounds ask of float64 arithmetic), and each injected defect - put in
the way a wrong kernel would, with everything computed afterwards following from it - must break exactly the identity it
belongs to.  The derivation of the scaled right-hand side and of the map back to (dx, dy, dz, dw) that the sweep check
uses is pinned against the oracle's step on goldens."""
import numpy as np
import pytest

import frontcheck as fc
import model
from common import KINDS, load_golden
from hqp_amd import _lib, ipmatrix
from oracle import oracleapi

CLS = {"SpBKP": ipmatrix.IpSpBKP, "RedSpBKP": ipmatrix.IpRedSpBKP}
NAMES = ["banded_n300_b10", "did_K50_spread4", "random_n200", "noineq_n120"]
SMALL = dict(leaf_size=24, max_pivots=12)
_cache = {}


def analyzed(name, kind, small):
    """(prog, state, structure, mode) of a golden: the host analysis alone"""
    key = (name, kind, small)
    if key not in _cache:
        prog, st, _g = load_golden(name)
        M = CLS[kind](**(SMALL if small else {}))
        try:
            M.init(prog)
        except ipmatrix.KktError as e:
            assert e.code == _lib.E_DEVICE
        _cache[key] = (prog, st, M.structure(), 0 if kind == "SpBKP" else 1)
    return _cache[key]


def run(name, kind, small, with_sweeps=True, **kw):
    prog, st, s, mode = analyzed(name, kind, small)
    src = fc.model_source(prog, st[0], st[1], mode, s, **kw)
    rep = fc.check_fronts(src, prog, st[0], st[1], mode, "%s %s" % (name, kind))
    if with_sweeps:
        t, _ta = fc.scaled_rhs(prog, mode, st, rep.sc)
        te = np.zeros(t.size)
        te[np.asarray(s["elim"])] = t.astype(float)
        fc.check_sweeps(rep, s, prog, mode, st, src.step(te))
    return rep, src, s


@pytest.mark.parametrize("fused", [False, True], ids=["product", "substitution"])
@pytest.mark.parametrize("small", [False, True], ids=["default", "small"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_clean_factors_pass(name, kind, small, fused):
    """Every err/bound <= 1 on float64 factors, X as a product with M (k_panel_solve) and by substitution (the fused small
    fronts).  Largest ratios over the 32 systems: a 0.096, b 0.237, c 0.440, d 0.214, sweeps 0.008, scale 0; e holds
    exactly.  No bound had to be widened."""
    rep, src, _s = run(name, kind, small, fused=fused)
    print(rep.text())
    assert src.npert == 0
    assert not rep.failed(), rep.text()
    r = rep.ratios()
    assert 0 < r["a"] and 0 < r["c"] and 0 < r["sweep"]  # (the identities were evaluated)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_host_matrix_and_scale_are_the_models(name, kind):
    """the sparse longdouble matrix and the scale vector against model.scaled_kkt (dense, float64)"""
    prog, st, s, mode = analyzed(name, kind, False)
    K, sc = model.scaled_kkt(prog, st[0], st[1], mode)
    hs = fc.host_scale(prog, st[0], st[1], mode)
    assert np.abs(hs - sc).max() <= 2 * np.spacing(1.0)
    H = fc.HostMatrix(prog, st[0], st[1], sc, mode, s["elim"])
    e = np.asarray(s["elim"])
    Ke = np.zeros_like(K)
    Ke[np.ix_(e, e)] = K
    Hd = H.csc.toarray()
    Hd = Hd + np.tril(Hd, -1).T
    assert np.abs(Hd - Ke).max() <= 4 * np.spacing(np.abs(Ke).max())
    assert (H.mag >= np.abs(H.val)).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["banded_n300_b10", "random_n200"])
def test_rhs_and_unpack_are_the_oracles_step(name, kind):
    """t of scaled_rhs through a dense solve of the scaled system and unpack() is the oracle's step (one unrefined solve
    of its own factorisation): the same (dx, dy, dz, dw) to 1e-9 of the largest component."""
    prog, st, s, mode = analyzed(name, kind, False)
    K, sc = model.scaled_kkt(prog, st[0], st[1], mode)
    t, ta = fc.scaled_rhs(prog, mode, st, sc)
    assert (ta >= np.abs(t)).all()
    xq = np.linalg.solve(K, t.astype(float))
    got = fc.unpack(prog, mode, st, sc, xq)
    O = oracleapi.OracleIpMatrix(kind)
    O.init(prog)
    O.factor(st[0], st[1])
    want = O.step(*st)
    scale = max(np.abs(v).max() for v in want if v.size)
    for g, w in zip(got, want):
        assert np.abs(g - w).max(initial=0.0) <= 1e-9 * scale
    # and back: the elimination-order solution the sweep check compares is the inverse of unpack
    xe = fc.solution_e(prog, mode, sc, s["elim"], *got[:3])
    assert np.abs(xe[np.asarray(s["elim"])].astype(float) - xq).max() <= 4 * np.spacing(np.abs(xq).max())


def _pick(src, s, want):
    """the first front (smallest pivot count first) that `want(node, blocks)` accepts"""
    order = sorted(range(len(s["npiv"])), key=lambda k: (int(s["npiv"][k]), k))
    for k in order:
        if want(k, src.blk[k]):
            return k
    raise AssertionError("no front for this defect")


def _is_leaf(s, k):
    return not (np.asarray(s["parent"]) == k).any()


DEFECTS = ["x_entry", "drop_last_column", "diag_twice", "child_shift", "dinv_swap", "m_entry", "entry_border", "entry_pivot"]


@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defects_fail_their_identity(defect):
    """One defect at one front; 64 ulp where a value is moved.  The fronts are chosen small (p + nch + 6 and 2 (2p + 8)
    below 64, or there is nothing to see at 64 ulp) and, for the moved entries, in the first pivot's column, where the
    entry is the whole term."""
    name, kind = ("did_K50_spread4", "SpBKP") if defect == "dinv_swap" else ("banded_n300_b10", "SpBKP")
    clean, src, s = run(name, kind, True, with_sweeps=False)
    assert not clean.failed()
    nb = s["nborder"]
    leaf = lambda k: _is_leaf(s, k)
    if defect == "x_entry":  # one entry of X, first pivot's column of a leaf
        k = _pick(src, s, lambda k, B: leaf(k) and nb[k] >= 2 and np.abs(B["X"][:, 0]).max() > 0)
        spec, want = ("x_entry", k, int(np.abs(src.blk[k]["X"][:, 0]).argmax()), 0), {"b"}
    elif defect == "drop_last_column":  # the last pivot column left out of L21 X'
        k = _pick(src, s, lambda k, B: nb[k] >= 2 and np.abs(B["X"][:, -1]).max() > 0 and np.abs(B["panel"][s["npiv"][k]:, -1]).max() > 0)
        spec, want = ("drop_last_column", k), {"d"}
    elif defect == "diag_twice":  # the diagonal term of U counted twice
        k = _pick(src, s, lambda k, B: nb[k] >= 2 and np.abs(B["X"][0]).max() > 0)
        spec, want = ("diag_twice", k, 0), {"d"}
    elif defect == "child_shift":  # one child's part of the update block one border position off
        def ok(k, B):
            ch = [c for c in range(len(nb)) if s["parent"][c] == k]
            return nb[k] >= 3 and ch and np.abs(src.blk[ch[0]]["U"]).max() > 0 and \
                np.isin(fc._front_index(s, ch[0])[1], fc._front_index(s, k)[1]).sum() >= 2
        k = _pick(src, s, ok)
        spec, want = ("child_shift", k, 0), {"d"}
    elif defect == "dinv_swap":  # D^-1 of a 2x2 pair: i11 and i22 exchanged
        k = _pick(src, s, lambda k, B: (B["ptype"] == 1).any())
        spec, want = ("dinv_swap", k), {"a"}
    elif defect == "m_entry":  # one entry of M below the diagonal
        k = _pick(src, s, lambda k, B: leaf(k) and s["npiv"][k] >= 2 and nb[k] >= 2 and B["M"][1, 0] != 0 and np.abs(B["X"][:, 0]).max() > 0)
        spec, want = ("m_entry", k, 1, 0, 64), {"b"}
    elif defect == "entry_border":  # one scaled entry of the matrix, border row, first pivot's column of a leaf
        def ok(k, B):
            return leaf(k) and nb[k] >= 2 and (B["lperm"] == np.arange(s["npiv"][k])).all() and np.abs(B["X"][:, 0]).max() > 0
        k = _pick(src, s, ok)
        spec, want = ("entry", k, int(s["npiv"][k]) + int(np.abs(src.blk[k]["X"][:, 0]).argmax()), 0), {"b"}
    else:  # ... and the first pivot itself
        k = _pick(src, s, lambda k, B: leaf(k) and (B["lperm"] == np.arange(s["npiv"][k])).all() and B["ptype"][0] == 0)
        assert 2 * (2 * int(s["npiv"][k]) + 8) < 64
        spec, want = ("entry", k, 0, 0), {"a"}
    rep, _src, _s = run(name, kind, True, with_sweeps=False, defect=spec)
    print(rep.text())
    assert set(rep.failed()) == want, rep.text()
    # the report names the front and the entries
    where, entries = rep.worst[next(iter(want))][1], rep.offenders[next(iter(want))]
    assert "node %d " % k in where and entries


def test_a_moved_entry_of_m_in_the_sweeps():
    """The sweep bound (2 levels + 2)(F_max + 4) u mu is some hundred u of the magnitudes: an entry of M moved by 64 ulp
    stays below it by construction (b sees it, above), and mu holds every term of the row, not this one alone.  Moved by
    4096 times the bound's constant, in ulp - a relative 1e-10 or so, two decades below what the parity tests of the
    solve see - in the root's M, the sweeps fail and nothing else does (the root has no border: b has nothing to say)."""
    name, kind = "banded_n300_b10", "SpBKP"
    _rep, src, s = run(name, kind, True)
    root = len(s["npiv"]) - 1
    assert s["nborder"][root] == 0 and s["npiv"][root] >= 2
    row = int(np.abs(src.blk[root]["M"][1:, 0]).argmax()) + 1
    rep, _src, _s = run(name, kind, True, defect=("m_entry", root, row, 0, 4096 * fc.sweep_constant(s)))
    print(rep.text())
    assert set(rep.failed()) == {"sweep"}, rep.text()


def test_update_blocks_the_source_no_longer_holds():
    """Update blocks that alternate between two half-arenas are gone when the factorisation ends, all but the last
    levels': the parents are then assembled from the reference blocks with d's allowance added to their bounds.  Clean
    factors pass; a front that leaves the last pivot column out of its (lost) update block is found in the fronts above it."""
    name, kind = "banded_n300_b10", "RedSpBKP"
    _clean, src0, s = run(name, kind, True, with_sweeps=False)
    top = int(np.max(s["level"]))
    lost = [k for k in range(len(s["npiv"])) if s["level"][k] < top - 1 and s["nborder"][k] > 0]
    assert len(lost) > 10
    rep, _src, _s = run(name, kind, True, with_sweeps=False, lost_u=lost)
    assert sorted(rep.derived_u) == lost and not rep.failed(), rep.text()
    k = _pick(src0, s, lambda k, B: k in lost and np.abs(B["X"][:, -1]).max() > 0 and np.abs(B["panel"][s["npiv"][k]:, -1]).max() > 0)
    rep, _src, _s = run(name, kind, True, with_sweeps=False, lost_u=lost, defect=("drop_last_column", k))
    print(rep.text())
    assert rep.failed() and set(rep.failed()) <= {"a", "b", "d"}
    anc, a = [], int(s["parent"][k])
    while a >= 0:
        anc.append(a)
        a = int(s["parent"][a])
    assert all(int(rep.worst[i][1].split()[1]) in anc for i in rep.failed())


def test_blocked_pivot_kernel_allowance_only_widens():
    """the extra term of identity a for k_factor_blk's products with the inverse of a diagonal block: evaluated on a
    source that calls its fronts blk0, clean factors pass as before"""
    prog, st, s, mode = analyzed("banded_n300_b10", "RedSpBKP", False)
    src = fc.model_source(prog, st[0], st[1], mode, s)
    src.kind = lambda node: "blk0"
    assert int(np.max(s["npiv"])) > 32
    rep = fc.check_fronts(src, prog, st[0], st[1], mode, "blk0")
    assert not rep.failed(), rep.text()
