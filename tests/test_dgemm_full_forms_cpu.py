"""The shapes of tests/test_gpu_dgemm_full.py (tests/dgemm_full_cases.py) get the forms they are named for: the launch
rule (hqp_amd/csrc/gemm_form.hpp, host code) through hqpkkt_debug_gemm_form, for a device of 256 CUs with a grid of 512
workgroups and the workspace hqpkkt_debug_dgemm_full states.  On another device the GPU test skips a case whose shape
the rule gives another form; here a change of the rule that moves a case is seen without a GPU."""
import pytest

from dgemm_full_cases import CASES, ROUNDING, rule_kwargs
from hqp_amd import ipmatrix


@pytest.mark.parametrize("case", CASES + ROUNDING, ids=lambda c: c.name)
def test_case_gets_the_form_it_names(case):
    form, tiles, table, tile_map, nsplit = ipmatrix.gemm_form(**rule_kwargs(case))
    assert form == case.form, (case.name, form)
    assert tile_map == bool(case.layout.get("tile_map")), case.name
    assert table == (form == "cut"), case.name
    if form == "ks":
        assert nsplit > 1, (case.name, nsplit)
    if case.name.startswith("plain3"):
        assert tiles <= 256, (case.name, tiles)  # one workgroup per CU: the three-buffer kernel (gemm_launch_plain)


def test_every_form_and_both_tile_orders_are_covered():
    assert {c.form for c in CASES} == set(ipmatrix.GEMM_FORMS)
    assert {c.form for c in ROUNDING} == set(ipmatrix.GEMM_FORMS) - {"frac"}
    assert any(c.layout.get("tile_map") for c in CASES) and any(c.form == "plain" and not c.layout.get("tile_map") for c in CASES)


def test_lists_of_the_cut_cases_park_partial_tiles():
    """Among the cut and frac cases every kind of work list - unequal shares, equal shares, fractional - occurs with
    tiles cut in k, so the sum over parked pieces runs; the list of the small forced-cut rounding case holds whole tiles
    only, as dgemm_full_cases.py says."""
    parked = {}
    for case in CASES + ROUNDING:
        if case.form not in ("cut", "frac"):
            continue
        kw = rule_kwargs(case)
        tiles = ipmatrix.gemm_form(**kw)[1]
        kind = "frac" if case.form == "frac" else "equal" if case.env.get("HQPKKT_SK_TABLE") == "0" else "unequal"
        got = ipmatrix.sk_table(tiles, -(-kw["K"] // 16), 512, kind)
        assert got is not None, (case.name, kind)
        if case.layout.get("force_split"):
            assert got[1] == 0, (case.name, got[1])
        else:
            parked[kind] = max(parked.get(kind, 0), got[1])
    assert set(parked) == {"unequal", "equal", "frac"} and min(parked.values()) > 0, parked
