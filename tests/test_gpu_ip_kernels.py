"""GPU tests of the vector kernels of the device-resident loops (hqp_amd/csrc/ipdriver.hip.h), one launch group at a time on
chosen operands, through hqpkkt_debug_ip_vec / hqpkkt_debug_ip_rows, which call the launch functions the loops call.
The references and the derivation of every bound are in tests/ip_kernel_refs.py: ratios, minima, maxima, indices and
branch flags must be numpy float64's bits; elementwise results, sums and the step's scalars carry derived bounds; ints
operands (entries -8 .. 8, power-of-two step lengths) must give EQUAL results whatever the order of summation.

Whatever a result may not depend on is NaN: every vector behind its length (the hooks' marks are NaN), the partials, out,
Bk and S before the launch.  A mark that changed comes back as HQPKKT_E_INTERN.  Every case is launched twice and must
give the same bits.

Shapes: m = 1, 63 .. 65, 255 .. 257, 1023 .. 1025, 8191, 8192 (the wave and workgroup edges, the eight element slots of a
thread of the one-workgroup kernels, IP_SMALL_M itself) on both forms; 8193, 65 537 and 70 001 (the second trip of the
256 x 256 grid-stride loops) on the separate launches.  "No blocking component" leaves Bk = (1e300, -1, 0, 0, 0, 0) per
vector: the ratio slot is the kernels' own "none" value, the four components are zero.

Not covered here: k_ip_rhs with the STAGED engine's xq, x1, x2 (a STAGED handle per case; tests/test_gpu_staged*.py run
them in whole solves).

Largest err / bound seen on one MI355X, reals: predictor statistics 0.58, step 0.33, corr_rhs / mupl / updates 0.33, cold
kernels 6.3e-4, k_fr_rhs 0.33, k_ip_rhs 0.49, k_fr_cold 0.16 (each case prints its own)."""
import numpy as np
import pytest

from hqp_amd import ipmatrix

import ip_kernel_refs as R

pytestmark = pytest.mark.gpu

NAN = np.nan
KINDS = ("ints", "reals")
GAMMA = 1.0e-4 ** 0.25  # the loops' values
GAMMAF = 0.01
M_BOTH = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192)
M_SEPARATE = (8193, 65537, 70001)


def _same(a, b):
    """equal bits, NaN included"""
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in a)


def _twice(op, n, me, m, **kw):
    a = ipmatrix.ip_vec(op, n, me, m, **kw)
    b = ipmatrix.ip_vec(op, n, me, m, **kw)
    assert _same(a, b), (op, "a second launch gives other bits")
    return a


# ---- predictor statistics: k_ip_ratio + k_ip_final + ip_sigma + k_ip_corr_rhs, k_ip_pred_small

def _pred(kind, m, seed, small, block="both", scale=1.0):
    o = R.step_operands(kind, m, seed, block)
    o["dz"], o["dw"] = o["dz"] * scale, o["dw"] * scale
    zw = float(o["z"] @ o["w"]) if kind == "ints" else float(np.sum(o["z"] * o["w"]))
    got = _twice("pred", 0, 0, m, small=small, sum=zw, gamma=GAMMA, **{k: o[k] for k in ("z", "w", "dz", "dw")})
    a, t = R.ratio_stats(o["z"], o["w"], o["dz"], o["dw"])
    ref = R.sigma_ref(a, t, zw, m, GAMMA)
    S = got["S"]
    if not small:
        assert got["out"][0] == a and got["out"][1] == t, (got["out"][:2], a, t)
    assert S[0] == ref["alpha_aff"], (S[0], ref["alpha_aff"])
    assert ref["sigma"].close(S[6]) and ref["smm"].close(S[1]), (S, ref["sigma"].v, ref["smm"].v)
    assert np.isnan(S[[2, 3, 4, 5, 7]]).all()  # nothing else is written
    # r4 = -(z w + (dza dwa - sigma mu)) with the sigma mu the device has stored: 4 operations
    ratio = R.elem_check(got["r4"], [R.prod(-1.0, o["z"], o["w"]), R.prod(-1.0, o["dz"], o["dw"]), (R.LD(S[1]), abs(S[1]))], 4, "r4")
    if kind == "ints" and float(S[1]) == round(S[1] * 2 ** 20) / 2 ** 20 and abs(S[1]) < 2 ** 20:
        assert np.array_equal(got["r4"], -(o["z"] * o["w"] + (o["dz"] * o["dw"] - S[1])))
    return got, ref, max(ratio, ref["sigma"].ratio(S[6]), ref["smm"].ratio(S[1]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", M_BOTH + M_SEPARATE)
def test_predictor_statistics(kind, m):
    sep, ref, r0 = _pred(kind, m, 1, False)
    worst = r0
    if m <= 8192:
        small, _ref, r1 = _pred(kind, m, 1, True)
        worst = max(worst, r1)
        assert _same({k: sep[k] for k in ("S", "r4")}, {k: small[k] for k in ("S", "r4")}), "small form against separate launches"
    print(f"pred {kind} m {m}: largest err / bound {worst:.3g}, alpha_aff {ref['alpha_aff']:.3g}")


@pytest.mark.parametrize("m", (1, 64, 257, 1025, 8192, 65537, 70001))
def test_predictor_last_element_decides(m):
    """the smallest ratio (1/64, below every other: ints have none under 1, reals none under 0.05) and the largest t
    (64 * 64, above 64 and 1 / 0.05^2) sit on the last element - beyond 65 536 that is the second trip of the loop"""
    for kind in KINDS:
        o = R.step_operands(kind, m, 1)
        o["z"][m - 1], o["w"][m - 1], o["dz"][m - 1], o["dw"][m - 1] = 1.0, 1.0, -64.0, -64.0
        four = {k: o[k] for k in ("z", "w", "dz", "dw")}
        for small in (False, True) if m <= 8192 else (False,):
            got = _twice("pred", 0, 0, m, small=small, sum=float(np.sum(o["z"] * o["w"])), gamma=GAMMA, **four)
            assert got["S"][0] == 1.0 / 64.0 and (small or (got["out"][0] == 1.0 / 64.0 and got["out"][1] == 4096.0)), got["out"][:2]
            assert R.sigma_ref(1.0 / 64.0, 4096.0, 1.0, m, GAMMA)["sigma"].close(got["S"][6])   # (the safe sigma: no t in it)
        if kind == "reals":   # (t = 1 / (ratio of z * ratio of w): no larger t with alpha_aff >= 0.1 among ratios near 0.05)
            continue
        o["dz"][m - 1] = -2.0   # alpha_aff 1/2: Terlaky's sigma with t = 2 * 64 from the last element (ints: t <= 64 elsewhere)
        four["dz"] = o["dz"]
        for small in (False, True) if m <= 8192 else (False,):
            got = _twice("pred", 0, 0, m, small=small, sum=float(np.sum(o["z"] * o["w"])), gamma=GAMMA, **four)
            a, t = R.ratio_stats(*(o[k] for k in ("z", "w", "dz", "dw")))
            assert t == 128.0 and got["S"][0] == R.clip01(a) and R.sigma_ref(a, t, 1.0, m, GAMMA)["sigma"].close(got["S"][6])


@pytest.mark.parametrize("small", (False, True))
def test_sigma_branches(small):
    """alpha_aff below and above 0.1 (a short step takes the safe sigma), exactly 0.1 as the double nearest 0.1 (z = 0.1,
    dz = -1: the quotient is that double, and 0.1 >= 0.1 takes Terlaky's branch), a ratio exactly 1, t from a single
    element and from none (dz dw <= 0 everywhere)."""
    m = 300
    base = dict(z=np.full(m, 2.0), w=np.full(m, 2.0), dz=np.full(m, 1.0), dw=np.full(m, -1.0))  # dz dw < 0: t = 0, ratio 2
    def run(**ch):
        o = {k: v.copy() for k, v in base.items()}
        for k, (i, v) in ch.items():
            o[k][i] = v
        got = _twice("pred", 0, 0, m, small=small, sum=float(o["z"] @ o["w"]), gamma=GAMMA, **o)
        a, t = R.ratio_stats(o["z"], o["w"], o["dz"], o["dw"])
        ref = R.sigma_ref(a, t, float(o["z"] @ o["w"]), m, GAMMA)
        assert got["S"][0] == ref["alpha_aff"] and ref["sigma"].close(got["S"][6]) and ref["smm"].close(got["S"][1]), (ch, got["S"])
        return got["S"], ref, t
    S, ref, t = run()
    assert S[0] == 1.0 and t == 0.0 and not ref["safe"]
    S, ref, t = run(z=(299, 0.1), dz=(299, -1.0), dw=(299, 1.0))   # 0.1 / 1 on the last element
    assert S[0] == 0.1 and not ref["safe"]
    S, ref, t = run(w=(7, 0.05), dw=(7, -1.0))
    assert S[0] == 0.05 and ref["safe"] and S[6] == pytest.approx(GAMMA / (1 - GAMMA), rel=1e-15)
    S, ref, t = run(w=(64, 2.0), dw=(64, -2.0))                    # a ratio exactly 1
    assert S[0] == 1.0
    S, ref, t = run(dz=(200, -4.0), dw=(200, -4.0))                # t from one element: 16 / 2 / 2, ratio 1/2
    assert t == 4.0 and S[0] == 0.5


# ---- the step: k_ip_minratio_part / _final + ip_alpha_pre + k_ip_mupl + k_ip_final + ip_alpha_fin + k_ip_update, k_ip_step_small

def _step(kind, m, seed, small, block="both", n=5, me=3, alpha_aff=0.5, plant=None, gammaf=GAMMAF):
    o = R.step_operands(kind, m, seed, block, n, me)
    if plant:
        plant(o)
    S_in = np.full(8, NAN)
    S_in[0] = alpha_aff
    got = _twice("step", n, me, m, small=small, gamma=GAMMA, gammaf=gammaf, S_in=S_in, **o)
    ref = R.step_ref(o, m, GAMMA, gammaf, alpha_aff)
    for name, mg in ref["margins"].items():
        assert mg > 0.0, ("the reference's margin to a threshold is below its error bound", name, mg)
    S, Bk = got["S"], got["Bk"]
    assert np.array_equal(Bk, ref["Bk"]), (Bk, ref["Bk"])
    assert S[0] == alpha_aff and S[4] == float(ref["need2"]) and S[3] == float(ref["damp"]) and S[2] == ref["alpha_pre"], (S, ref)
    assert ref["alpha"].close(S[5]), (S[5], ref["alpha"].v, ref["alpha"].err)
    worst = ref["alpha"].ratio(S[5])
    if ref["sum"] is not None and not small:
        assert ref["sum"].close(got["out"][0])
        worst = max(worst, ref["sum"].ratio(got["out"][0]))
    if kind == "ints":
        exact = float(np.sum((o["z"] + S[2] * o["dz"]) * (o["w"] + S[2] * o["dw"])))
        pre, fin = R.step_rule_f64(ref["Bk"], exact, m, gammaf)
        assert S[2] == pre and S[5] == (0.0 if ref["need2"] else fin), (S, pre, fin)
        if ref["damp"] and not small:
            assert got["out"][0] == exact
    al = S[5]
    for res, v, dv in (("ox", "x", "dx"), ("oy", "y", "dy"), ("oz", "z", "dz"), ("ow", "w", "dw")):
        if o[v].size:
            worst = max(worst, R.axpy_check(got[res], o[v], al, o[dv], res))
    return got, ref, worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", M_BOTH + M_SEPARATE)
def test_step(kind, m):
    n, me = (1025, 1) if m % 2 else (0, 1025)
    sep, ref, worst = _step(kind, m, 2, False, n=n, me=me)
    if m <= 8192:
        small, _r, r1 = _step(kind, m, 2, True, n=n, me=me)
        worst = max(worst, r1)
        keys = ("S", "Bk", "ox", "oy", "oz", "ow")
        assert _same({k: sep[k] for k in keys}, {k: small[k] for k in keys}), "small form against separate launches"
    print(f"step {kind} m {m}: largest err / bound {worst:.3g}, branch {ref['branch']}, alpha {sep['S'][5]:.3g}")


@pytest.mark.parametrize("small", (False, True))
@pytest.mark.parametrize("block", ("none", "z", "w", "both"))
def test_step_blocking_sides(block, small):
    for kind in KINDS:
        got, ref, _ = _step(kind, 777, 3, small, block=block)
        assert ref["damp"] == (block != "none")
        if block == "none":
            assert np.array_equal(got["Bk"], [1e300, -1, 0, 0, 0, 0] * 2) and got["S"][2] == 1.0 and got["S"][5] == 1.0


def test_step_small_largest_total():
    """n + me + m = 4 * 8192 on the one-workgroup form, and one more is refused"""
    _step("ints", 8192, 4, True, n=3 * 8192 - 1025, me=1025)
    o = R.step_operands("ints", 8192, 4, "both", 3 * 8192 - 1024, 1025)
    with pytest.raises(ipmatrix.KktError):
        ipmatrix.ip_vec("step", 3 * 8192 - 1024, 1025, 8192, small=True, gamma=GAMMA, gammaf=GAMMAF, S_in=np.zeros(8), **o)
    with pytest.raises(ipmatrix.KktError):
        o = R.step_operands("ints", 8193, 4, "both")
        ipmatrix.ip_vec("step", 0, 0, 8193, small=True, gamma=GAMMA, gammaf=GAMMAF, S_in=np.zeros(8), **o)


# equal smallest ratios at several indices: the smallest index wins.  (first index, second index, m)
TIES = [((3, 40), 64, "one wavefront"), ((10, 100), 256, "two wavefronts"), ((300, 900), 1025, "two blocks"),
        ((5, 5 + 1024), 2100, "two slots of one small-form thread"), ((2000, 8191), 8192, "the last element"),
        ((70000, 4000), 70001, "second trip against first"), ((65536, 65537), 65538, "inside the second trip")]


@pytest.mark.parametrize("tie", TIES, ids=[t[2] for t in TIES])
@pytest.mark.parametrize("vec", ("z", "w", "zw"))
def test_ties_take_the_smallest_index(tie, vec):
    (i, j), m, _ = tie
    first = min(i, j)
    def plant(o):
        for v in vec:
            dv = "d" + v
            for k in (j, i):   # ratio 1/8, below every other (>= 1), with different components at the two indices
                o[v][k], o[dv][k] = (1.0, -8.0) if k == first else (0.5, -4.0)
    forms = (False, True) if m <= 8192 else (False,)
    for small in forms:
        got, ref, _ = _step("ints", m, 5, small, plant=plant, n=0, me=0)
        for p, v in enumerate("zw"):
            if v in vec:
                assert got["Bk"][6 * p] == 0.125 and got["Bk"][6 * p + 1] == first, (got["Bk"], first)
        b = ipmatrix.ip_vec("blocking", 0, 0, m, **_planted(m, plant))
        assert np.array_equal(b["Bk"], ref["Bk"])


def _planted(m, plant):
    o = R.step_operands("ints", m, 5, "both", 0, 0)
    plant(o)
    return {k: o[k] for k in ("z", "w", "dz", "dw")}


@pytest.mark.parametrize("small", (False, True))
def test_step_thresholds_and_zeros(small):
    """dz = +0.0 and -0.0 block nothing; alpha == zmin == wmin takes the w branch first (the rule asks w first)."""
    m = 130
    def zeros(o):
        o["dz"][:] = 0.0
        o["dz"][1::2] = -0.0
        o["dw"][:] = np.abs(o["dw"])
    got, ref, _ = _step("ints", m, 6, small, plant=zeros)
    assert got["Bk"][1] == -1 and got["Bk"][7] == -1 and got["S"][3] == 0.0 and got["S"][5] == 1.0
    def both_equal(o):
        o["z"][17], o["dz"][17], o["w"][17], o["dw"][17] = 1.0, -4.0, 8.0, 1.0
        o["w"][90], o["dw"][90], o["z"][90], o["dz"][90] = 2.0, -8.0, 8.0, 1.0
    got, ref, _ = _step("ints", m, 6, small, plant=both_equal)
    assert got["Bk"][0] == 0.25 and got["Bk"][6] == 0.25 and ref["branch"] == 1
    # the second corrector's switch: alpha_aff >= 0.1 and a tiny corrector step
    def tiny(o):
        o["z"][3], o["dz"][3] = 2.0 ** -40, -8.0
    got, ref, _ = _step("ints", m, 6, small, plant=tiny)
    assert ref["need2"] and got["S"][4] == 1.0 and got["S"][5] == 0.0
    got, ref, _ = _step("ints", m, 6, small, plant=tiny, alpha_aff=0.05)
    assert not ref["need2"] and got["S"][4] == 0.0 and got["S"][5] > 0.0


# ---- the host's copy of the step rule against the device's

@pytest.mark.parametrize("block", ("none", "z", "w", "both"))
def test_host_step_rule_equals_device(block):
    m = 500
    o = R.step_operands("ints", m, 7, block)
    B = R.blocking(o["z"], o["w"], o["dz"], o["dw"])
    pre = 1.0 if block == "none" else min(B[0], B[6])
    s = float(np.sum((o["z"] + pre * o["dz"]) * (o["w"] + pre * o["dw"])))
    host = ipmatrix.ip_vec("host_step_rule", 0, 0, m, Bk_in=B, sum=s, gammaf=GAMMAF)
    S_in = np.full(8, NAN)
    S_in[0] = 0.05
    dev = ipmatrix.ip_vec("step", 0, 0, m, gamma=GAMMA, gammaf=GAMMAF, S_in=S_in, **{k: o[k] for k in ("z", "w", "dz", "dw")})
    assert host["S"][2] == dev["S"][2] and host["S"][5] == dev["S"][5] and host["S"][3] == dev["S"][3], (host["S"], dev["S"])
    assert (host["S"][2], host["S"][5]) == R.step_rule_f64(B, s, m, GAMMAF)


# ---- k_ip_final on a hand-made 256 x 8 table of distinct integers

@pytest.mark.parametrize("ops", ipmatrix.IP_FINAL_OPS)
def test_final_patterns(ops):
    part = R.rng_of(8).permutation(4096)[:2048].astype(float) - 1000.0
    P = part.reshape(256, 8)
    pat = {"OPS_SUM": "ssssssss", "OPS_HEAD": "sssxnnss", "OPS_COLD": "nnxxssss", "OPS_MIN_MAX": "nxssssss", "OPS_MIN": "nsssssss",
           "OPS_SUM_MAX": "sxssssss"}[ops]
    want = [{"s": P[:, k].sum(), "x": P[:, k].max(), "n": P[:, k].min()}[c] for k, c in enumerate(pat)]
    got = _twice("final", 0, 0, 0, part_in=part, ops=ops, epi=0)
    assert np.array_equal(got["out"], want), (got["out"], want)
    assert np.isnan(got["S"]).all()


def test_final_epilogues():
    part = np.zeros((256, 8))
    # epi 1: sigma from slots 0 (ratio) and 1 (t)
    part[:, 0], part[:, 1] = 1e300, 0.0
    part[77, 0], part[200, 1] = 0.75, 3.0
    got = _twice("final", 0, 0, 10, part_in=part.ravel(), ops="OPS_MIN_MAX", epi=1, mu=0.5, gamma=GAMMA)
    ref = R.sigma_ref(0.75, 3.0, 5.0, 10, GAMMA)
    assert got["S"][0] == 0.75 and ref["sigma"].close(got["S"][6]) and ref["smm"].close(got["S"][1])
    # epi 3: min(1, beta v) on both sides of 1
    for v, want in ((0.5, 0.995 * 0.5), (1.0, 0.995), (1.25, 1.0), (2.0, 1.0)):
        part[:, 0] = 2.0
        part[255, 0] = v
        got = _twice("final", 0, 0, 10, part_in=part.ravel(), ops="OPS_MIN", epi=3, gammaf=0.995)
        assert got["out"][0] == v and got["S"][5] == want
    # epi 2: the damped step from Bk and S, the sum spread over the table
    o = R.step_operands("ints", 200, 9)
    B = R.blocking(o["z"], o["w"], o["dz"], o["dw"])
    pre = min(B[0], B[6])
    terms = (o["z"] + pre * o["dz"]) * (o["w"] + pre * o["dw"])
    part[:] = 0.0
    part[:200, 0] = terms
    S_in = np.array([0.05, NAN, pre, 1.0, 0.0, NAN, NAN, NAN])
    got = _twice("final", 0, 0, 200, part_in=part.ravel(), ops="OPS_SUM", epi=2, gammaf=GAMMAF, Bk_in=B, S_in=S_in)
    assert got["out"][0] == terms.sum() and got["S"][5] == R.step_rule_f64(B, terms.sum(), 200, GAMMAF)[1]


# ---- single kernels with the host's scalars

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", (1, 255, 256, 257, 70001))
def test_corr_rhs_mupl_update(kind, m):
    o = R.step_operands(kind, m, 10, "both", 257, 255)
    four = {k: o[k] for k in ("z", "w", "dz", "dw")}
    smm = 0.25 if kind == "ints" else 0.123456789
    got = _twice("corr_rhs", 0, 0, m, smm=smm, **four)
    worst = R.elem_check(got["r4"], [R.prod(-1.0, o["z"], o["w"]), R.prod(-1.0, o["dz"], o["dw"]), (R.LD(smm), smm)], 4, "corr r4")
    alpha = 0.5 if kind == "ints" else 0.7071
    got = _twice("mupl", 0, 0, m, alpha=alpha, **four)
    ref = R.mupl_sum(o["z"], o["w"], o["dz"], o["dw"], alpha)
    assert ref.close(got["out"][0]) and (kind == "reals" or got["out"][0] == float(ref.v))
    worst = max(worst, ref.ratio(got["out"][0]))
    for op, sign in (("update", 1.0), ("fr_update", -1.0)):
        S_in = np.full(8, NAN)
        S_in[5] = alpha
        got = _twice(op, 257, 255, m, alpha=alpha, S_in=S_in, **o)
        for res, v, dv in (("ox", "x", "dx"), ("oy", "y", "dy"), ("oz", "z", "dz"), ("ow", "w", "dw")):
            worst = max(worst, R.axpy_check(got[res], o[v], alpha, o[dv], op + res, sign))
        zn, wn = got["oz"], got["ow"]   # slot 0 sums the products of the stored values: one operation per term
        worst = max(worst, R.sum_check(got["out"][0], zn * wn if kind == "ints" else zn.astype(R.LD) * wn.astype(R.LD), np.abs(zn * wn), 1, op))
        assert got["out"][1] == np.abs(got["ox"]).max()
        if kind == "ints":
            assert got["out"][0] == float(zn @ wn)
    print(f"corr_rhs / mupl / updates {kind} m {m}: largest err / bound {worst:.3g}")


@pytest.mark.parametrize("op", ("update", "fr_update"))
def test_update_nan_in_x_gives_inf(op):
    o = R.step_operands("ints", 10, 11, "both", 70001, 0)
    o["x"][65540] = NAN
    S_in = np.full(8, NAN)
    S_in[5] = 0.5
    got = ipmatrix.ip_vec(op, 70001, 0, 10, alpha=0.5, S_in=S_in, **o)
    assert got["out"][1] == np.inf
    got = ipmatrix.ip_vec(op, 70001, 0, 0, alpha=0.5, x=o["x"], dx=o["dx"])   # m = 0: the host's alpha
    assert got["out"][1] == np.inf and got["out"][0] == 0.0


# ---- cold starts

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", (1, 255, 256, 257, 70001))
def test_cold_start_kernels(kind, m):
    r = R.rng_of(12, m, kind == "ints")
    v = (lambda k: r.integers(-8, 9, k).astype(float)) if kind == "ints" else (lambda k: r.uniform(-1, 1, k))
    n, me = 257, 1
    c, b, d, dz, dw = v(n), v(me), v(m), v(m), v(m)
    got = _twice("cold_rhs", n, me, m, c=c, b=b, d=d, p0=0.375, p1=-0.375)
    assert np.array_equal(got["r1"], c) and np.array_equal(got["r2"], -b) and np.array_equal(got["r3"], -d)
    assert (got["oz"] == 1.0).all() and (got["ow"] == 0.375).all() and (got["r4"] == -0.375).all()
    got = _twice("cold_stats", 0, 0, m, dz=dz, dw=dw)
    out = got["out"]
    assert out[0] == dz.min() and out[1] == dw.min() and out[2] == np.abs(dz).max() and out[3] == np.abs(dw).max()
    worst = max(R.sum_check(out[4], dz, np.abs(dz), 0, "sum dz"), R.sum_check(out[5], dw, np.abs(dw), 0, "sum dw"))
    assert kind == "reals" or (out[4] == dz.sum() and out[5] == dw.sum())
    for inplace in (False, True):   # one addition: correctly rounded, numpy's bits
        got = _twice("shift", 0, 0, m, dz=dz, dw=dw, p0=1.5, p1=0.1, inplace=inplace)
        assert np.array_equal(got["oz"], dz + 1.5) and np.array_equal(got["ow"], dw + 0.1)
    got = _twice("fill", 0, 0, m, p0=1e-10)
    assert (got["oz"] == 1e-10).all()
    got = _twice("fr_dstats", 0, 0, m, d=d)
    assert got["out"][0] == d.min() and got["out"][1] == np.abs(d).max() and (kind == "reals" or got["out"][2] == d.sum())
    worst = max(worst, R.sum_check(got["out"][2], d, np.abs(d), 0, "sum d"))
    print(f"cold kernels {kind} m {m}: largest err / bound {worst:.3g}")


# ---- Franke's ratio test, right-hand sides

@pytest.mark.parametrize("m", (1, 64, 257, 8193, 70001))
def test_franke_ratio(m):
    beta = 0.995
    for kind in KINDS:
        o = R.step_operands(kind, m, 13)
        z, w, dz, dw = (o[k] for k in ("z", "w", "dz", "dw"))
        q = np.concatenate([(z / np.where(dz > 0, dz, 1.0))[dz > 0], (w / np.where(dw > 0, dw, 1.0))[dw > 0], [2.0]])
        got = _twice("fr_ratio", 0, 0, m, gammaf=beta, z=z, w=w, dz=dz, dw=dw)
        assert got["out"][0] == q.min() and got["S"][5] == min(1.0, beta * q.min()), (got["out"][0], q.min())
    # steps <= 0 everywhere (zeros of both signs among them): the cap 2; a step of exactly 0 is no blocking component
    dz = -np.abs(dz)
    dz[::3] = 0.0
    dz[1::3] = -0.0
    got = _twice("fr_ratio", 0, 0, m, gammaf=beta, z=z, w=w, dz=dz, dw=dz)
    assert got["out"][0] == 2.0 and got["S"][5] == 1.0
    dz[m - 1] = 4.0 * z[m - 1]   # the last element alone blocks: 1/4
    got = _twice("fr_ratio", 0, 0, m, gammaf=beta, z=z, w=w, dz=dz, dw=-np.abs(dw))
    assert got["out"][0] == z[m - 1] / dz[m - 1] and got["S"][5] == beta * got["out"][0]


@pytest.mark.parametrize("dims", ((1, 0, 0), (0, 1, 1), (255, 1, 1), (1025, 1025, 257), (1, 0, 70001)))
def test_franke_rhs(dims):
    n, me, m = dims
    for kind in KINDS:
        r = R.rng_of(14, n, me, m, kind == "ints")
        v = (lambda k: r.integers(-8, 9, k).astype(float)) if kind == "ints" else (lambda k: r.uniform(-1, 1, k))
        a1, a2, a3, z, w = v(n), v(me), v(m), np.abs(v(m)) + 1, np.abs(v(m)) + 1
        zeta, mu = (0.5, 3.0) if kind == "ints" else (0.3, 0.017)
        got = _twice("fr_rhs", n, me, m, c=a1, b=a2, d=a3, z=z, w=w, p0=zeta, p1=mu)
        # one product each: correctly rounded; r4 = z w - mu: 2 operations
        assert np.array_equal(got["r1"], -zeta * a1) and np.array_equal(got["r2"], -zeta * a2) and np.array_equal(got["r3"], -zeta * a3)
        ratio = R.elem_check(got["r4"], [R.prod(z, w), (R.LD(-mu), mu)], 2, "fr r4") if m else 0.0
        assert kind == "reals" or np.array_equal(got["r4"], z * w - mu)
    print(f"fr_rhs {dims}: largest err / bound {ratio:.3g}")


# ---- the kernels that walk the CSR blocks: k_ip_rhs, k_fr_cold

ROWS_DIMS = ((70, 55, 60), (70, 55, 0), (70, 0, 60), (385, 8000, 8000))  # the last: 16 385 rows, the second trip at 4 lanes per row
_mats = {}


def _matrix(kind, dims):
    if (kind, dims) not in _mats:
        prog, qlen = R.rows_program(kind, *dims, seed=15)
        mat = ipmatrix.IpSpBKP()
        mat.init(prog)
        _mats[kind, dims] = (prog, mat, qlen)
    return _mats[kind, dims]


@pytest.mark.parametrize("lpr", (4, 16))
@pytest.mark.parametrize("dims", ROWS_DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_rhs_rows(kind, dims, lpr):
    prog, mat, qlen = _matrix(kind, dims)
    n, me, m = dims
    if dims == ROWS_DIMS[0]:
        for L in R.ROW_LENGTHS:   # the lengths the walk has branches for are there, in every block and transpose
            assert L in qlen
            for blk, rows in ((prog.A, me), (prog.C, m)):
                D = R.dense_of(blk, rows, n)
                assert L in (D != 0).sum(1) and L in (D != 0).sum(0), (L, rows)
    r = R.rng_of(16, n, me, m, kind == "ints")
    v = (lambda k: r.integers(-8, 9, k).astype(float)) if kind == "ints" else (lambda k: r.uniform(-1, 1, k))
    x, y, z, w = v(n), v(me), np.abs(v(m)) + 1.0, np.abs(v(m)) + 1.0
    kw = dict(c=prog.c, b=prog.b, d=prog.d, x=x, y=y, z=z, w=w)
    got = ipmatrix.ip_rows(mat, "rhs", lpr, **kw)
    assert _same(got, ipmatrix.ip_rows(mat, "rhs", lpr, **kw)), "a second launch gives other bits"
    ref = R.rhs_ref(kind, prog, x, y, z, w)
    worst = 0.0
    for name in ("r1", "r2", "r3", "r4"):
        val, bound = ref[name]
        if kind == "ints":
            assert np.array_equal(got[name], val.astype(float)), (name, np.flatnonzero(got[name] != val)[:8])
        else:
            err = np.abs(got[name].astype(R.LD) - val).astype(float)
            assert (err <= bound).all(), (name, np.flatnonzero(err > bound)[:8])
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max(initial=0.0)))
    out = got["out"]
    for k, name in enumerate(("gap", "pcost", "zw")):
        val, bound = ref[name]
        if kind == "ints":
            assert out[k] == float(val), (name, out[k], val)
        else:
            err = float(abs(R.LD(out[k]) - val))
            assert err <= bound, (name, err, bound)
            worst = max(worst, err / max(bound, 1e-300))
    rmax = max([float(np.abs(got[k]).max(initial=0.0)) for k in ("r1", "r2", "r3")])
    assert out[3] == rmax and out[4] == (z.min() if m else 1e300) and out[5] == (w.min() if m else 1e300)
    print(f"k_ip_rhs {kind} {dims} lpr {lpr}: largest err / bound {worst:.3g}")
    if dims == ROWS_DIMS[0] and kind == "ints":   # NaN in a residual row makes slot 3 inf
        kw["x"] = x.copy()
        kw["x"][prog.A[1][0]] = NAN
        assert ipmatrix.ip_rows(mat, "rhs", lpr, **kw)["out"][3] == np.inf


@pytest.mark.parametrize("lpr", (4, 16))
@pytest.mark.parametrize("dims", ROWS_DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_franke_cold_rows(kind, dims, lpr):
    prog, mat, _ = _matrix(kind, dims)
    n, me, m = dims
    Lt = 64.0 if kind == "ints" else 37.3
    got = ipmatrix.ip_rows(mat, "fr_cold", lpr, c=prog.c, b=prog.b, d=prog.d, p0=Lt)
    assert _same(got, ipmatrix.ip_rows(mat, "fr_cold", lpr, c=prog.c, b=prog.b, d=prog.d, p0=Lt))
    z0 = Lt / (float(m) * m) if m else 0.0   # one product and one division, as the kernel: these bits
    assert (got["ox"] == 0).all() and (got["oy"] == 0).all() and np.array_equal(got["r2"], -prog.b)
    Cd = R.dense_of(prog.C, m, n)
    if m:
        wj = Lt + prog.d + 1e-10
        assert (got["oz"] == z0).all() and np.array_equal(got["ow"], wj) and (got["r3"] == Lt).all()
        # a1 = c - (sum of the column of C) z0: T entries, then 2 operations
        col = Cd.astype(R.LD).sum(0)
        T = (Cd != 0).sum(0)
        ref = prog.c - col * R.LD(z0)
        bound = (T + 3) * R.U * (np.abs(prog.c) + np.abs(Cd).sum(0) * z0)
        err = np.abs(got["r1"].astype(R.LD) - ref).astype(float)
        assert (err <= bound).all(), np.flatnonzero(err > bound)[:8]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, R.sum_check(got["out"][0], R.LD(z0) * wj.astype(R.LD), np.abs(z0 * wj), 1, "z'w"))
    else:
        assert np.array_equal(got["r1"], prog.c)
        worst = 0.0
    print(f"k_fr_cold {kind} {dims} lpr {lpr}: largest err / bound {worst:.3g}")
