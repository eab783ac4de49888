"""
Conditions on the INPUTS of tests/test_gpu_f_pass_model_tables.py, checked without a GPU: what the NumPy restatement of the
rule of decided edges (tests/f_sure_ref.py) says of every table of tests/f_pass_table_cases.py.  A GPU case asserts from the
context's counters which form of the f pass ran; these conditions are why that form is the one the case is about, so that
none passes on a table that never reaches it.  They are conditions, not measurements: a seed that misses one is replaced,
the condition stays.
"""
import numpy as np
import pytest

import f_pass_table_cases as FC
import f_sure_ref as R

NAMES = list(FC.CASES)


def kind(name):
    return FC.CASES[name][2]


def of_kind(*kinds):
    return [n for n in NAMES if kind(n) in kinds]


@pytest.mark.parametrize("name", NAMES)
def test_tables_are_well_formed(name):
    (S_B, lM, N, U, p) = FC.build(name)
    assert S_B.shape == (N * (N - 1) // 2, 3) and lM.shape == (S_B.shape[0], U, 3, 3) and 1 <= U <= 64
    assert np.isfinite(S_B).all() and not np.isnan(lM).any() and not (lM == np.inf).any()
    assert np.isfinite(lM).all() == (kind(name) != "ninf")
    assert p["tiles"] == sum(len(t) > 0 for t in R.tiles(N)) and p["decided_hint"] >= p["decided_T"]


def test_shapes_cover_the_geometry():
    assert {FC.build(n)[2] for n in NAMES} == {5, 13, 18, 34}
    assert {FC.CASES[n][3] for n in NAMES} == {65, 1100}
    assert {FC.build(n)[3] for n in NAMES} >= {1, 3, 64}
    # every family has a table that takes the run form and one that takes the per-tile kernel
    for family in ("shared", "grouped", "grouped64", "sessions", "noise"):
        kinds = {kind(n) for n in NAMES if n.split("-")[0] == family}
        assert kinds == {"all", "mixed"}, (family, kinds)


@pytest.mark.parametrize("name", of_kind("all"))
def test_decided_cases_have_every_tile_decided_at_the_hint(name):
    p = FC.build(name)[4]
    assert p["all"] and p["decided_hint"] == p["tiles"] and p["decided_T"] > 0, (name, p["decided_T"], p["decided_hint"], p["tiles"])


@pytest.mark.parametrize("name", of_kind("mixed"))
def test_mixed_cases_have_tiles_of_both_kinds(name):
    p = FC.build(name)[4]
    assert 0 < p["decided_hint"] < p["tiles"] and not p["all"], (name, p["decided_hint"], p["tiles"])
    assert 0 < p["decided_T"], name                  # (... and the passes at this gamma skip some)


@pytest.mark.parametrize("name", [n for n in NAMES if n.split("-")[0] in ("sessions", "noise")])
def test_sessions_tables_hold_an_item_whose_linear_product_underflows(name):
    (_S, lM, _N, _U, p) = FC.build(name)
    assert len(p["underflow"]) >= 1 and np.isfinite(lM).all()
    if name.startswith("noise"):
        assert len(set(np.round(p["var_b"], 12))) > 1 and len(set(np.round(p["var_bt"].ravel(), 12))) > 1


@pytest.mark.parametrize("name", of_kind("scaled"))
def test_scaled_table_has_an_edge_over_the_cap_inside_a_live_tile(name):
    (_S, _L, N, _U, p) = FC.build(name)
    assert FC.scaled_premise_holds(N, p)
    assert len(p["capped"]) >= 1 and (p["mode_T"][p["capped"]] == -1).all() and p["decided_T"] >= 1
    lone = [c for c in p["capped"] if (p["mode_T"][FC.tile_of(N, c)] < 0).sum() == 1]
    assert len(lone) >= 1
    assert not p["all"]                              # (the auto choice keeps the per-tile kernel; f_runs = 2 meets the cap in the run kernel)


@pytest.mark.parametrize("name", of_kind("missing"))
def test_missing_tables_hold_the_exact_zero_rows_and_leave_them_open(name):
    (S_B, lM, N, U, p) = FC.build(name)
    (z_lM, z_SB) = (p["zero_lM"], p["zero_SB"])
    assert U % 2 == 1 and (lM[:, U - 1] == 0.0).all()
    assert (lM[z_lM] == 0.0).all() and (S_B[z_lM] != 0.0).all()
    assert (S_B[z_SB] == 0.0).all() and (lM[z_SB] != 0.0).any()
    assert (lM[p["dead_edges"]] == 0.0).all() and len(p["dead_edges"]) == N - 1
    for mode in (p["mode_T"], p["mode_hint"]):
        assert mode[z_lM] == -1 and mode[z_SB] == -1
    assert (p["mode_T"][p["dead_edges"]] >= 0).all()        # (a decided edge whose records are all zero)
    assert p["decided_T"] >= 1 and p["any"] and not p["all"]
    assert 0.2 <= p["nan_fraction"] <= 0.5


def test_weighted_tables_are_a_finite_one_and_one_with_minus_inf():
    (fin, inf) = (FC.build("weighted-finite-13"), FC.build("weighted-ninf-13"))
    c0 = inf[4]["ninf_edge"]
    assert np.array_equal(fin[0], inf[0]) and fin[3] == inf[3] == 1
    assert np.isfinite(fin[1]).all() and not fin[4]["ninf"].any() and len(fin[4]["nan_bounds"]) == 0
    assert np.isneginf(inf[1][c0]).all() and np.isfinite(np.delete(inf[1], c0, axis=0)).all()
    assert inf[4]["nan_bounds"].tolist() == [c0] and inf[4]["mode_T"][c0] == -1 and inf[4]["mode_hint"][c0] == -1
    assert inf[4]["decided_T"] >= 1 and inf[4]["any"]
    # the tile around the -inf edge is live: its other edges are decided
    t = FC.tile_of(13, c0)
    assert (inf[4]["mode_T"][t[t != c0]] >= 0).all() and len(t) > 1


def test_ladder_walks_the_four_hint_states_in_order():
    steps = FC.build_ladder()
    assert tuple(FC.hint_state(s[4]) for s in steps) == FC.LADDER_STATES == ("all", "none", "some", "all")
    assert len({s[2] for s in steps}) == 1 and len({s[3] for s in steps}) == 1
    assert steps[1][4]["decided_T"] == 0 and 0 < steps[2][4]["decided_T"] < steps[2][4]["tiles"]
    assert [s[4]["beta"] for s in steps][0::3] == [1.0, 1.0] and steps[1][4]["beta"] < steps[2][4]["beta"] < 1.0
