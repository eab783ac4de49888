"""
The options of the permutation baselines (missing_data=True, variance="welch") without a GPU: the reference
(baseline_missing_ref.py) against values worked by hand on three regions with one missing value, the loop-level reference
against its exact form, the host-side refusals (they run before any context exists), and that header, binding and library
agree on the two entry points with options.
"""
import math
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_missing_ref as MR
import baseline_ref as BR
from conftest import ROOT
from fcdiff_amd import _lib, baseline

NAN = math.nan


def hand_case():
    """Three regions, H = 3, U = 2; control 2 of connection 0 is missing.  Row 0 of the labels is the observed labelling, row 1
    labels subjects 2 and 3: on connection 0 that leaves n1 = 1 (the value 5) against 0, 2, 7."""
    b = np.array([[0.0, 2.0, NAN], [0.0, 2.0, 4.0], [1.0, 4.0, 1.0]])
    bt = np.array([[5.0, 7.0], [5.0, 7.0], [2.0, 3.0]])
    labels = np.array([[0, 0, 0, 1, 1], [0, 0, 1, 1, 0]], dtype=np.uint8)
    return b, bt, labels


def test_reference_against_values_worked_by_hand():
    (b, bt, labels) = hand_case()
    t2 = 0.5 / math.sqrt(6.5 / 3.0 * (1.0 / 3.0 + 1.0 / 2.0))           # (1, 4, 1) against (2, 3): SS 6 and 0.5
    pooled = MR.group_test(b, bt, labels, "pooled")
    # connection 0: (0, 2) against (5, 7), the textbook 5 / sqrt 2; connection 1: (0, 2, 4) against (5, 7), SS 8 and 2,
    # pooled variance 10/3, t = 4 / sqrt(10/3 * 5/6) = 2.4
    nptest.assert_allclose(pooled["t"], [5.0 / math.sqrt(2.0), 2.4, t2], rtol=1e-14)
    nptest.assert_array_equal(pooled["null_t"][0], pooled["t"])
    # row 1 on connection 0: 5 against (0, 2, 7), mean 3, SS 26, t = 2 / sqrt(26/2 * 4/3)
    nptest.assert_allclose(pooled["null_t"][1, 0], 2.0 / math.sqrt(52.0 / 3.0), rtol=1e-14)
    assert pooled["n_controls"].tolist() == [2, 3, 3] and pooled["n_patients"].tolist() == [2, 2, 2]
    assert pooled["count_t"][0] == 1
    t = pooled["t"]
    nptest.assert_allclose(pooled["region"], [t[0] ** 2 + t[1] ** 2, t[0] ** 2 + t[2] ** 2, t[1] ** 2 + t[2] ** 2], rtol=1e-14)
    welch = MR.group_test(b, bt, labels, "welch")
    # equal sizes and spreads on connection 0: Welch's t is Student's; connection 1: v = (8/2)/3 + (2/1)/2 = 7/3
    w2 = 0.5 / math.sqrt(3.0 / 3.0 + 0.5 / 2.0)
    nptest.assert_allclose(welch["t"], [5.0 / math.sqrt(2.0), 4.0 / math.sqrt(7.0 / 3.0), w2], rtol=1e-14)
    # row 1 leaves one labelled value on connection 0: undefined, an exceedance, and 0 to the sums of regions 0 and 1
    assert math.isnan(welch["null_t"][1, 0]) and welch["count_t"][0] == 2
    tw = welch["null_t"][1]
    nptest.assert_allclose(welch["null_region"][1], [tw[1] ** 2, tw[2] ** 2, tw[1] ** 2 + tw[2] ** 2], rtol=1e-14)
    nptest.assert_allclose(welch["null_max_t"][1], max(abs(tw[1]), abs(tw[2])), rtol=0)
    nptest.assert_array_equal(welch["p_t"], (1.0 + welch["count_t"]) / 3.0)


def test_reference_dead_connections():
    """Missing in every patient, n = 2, and equal observed values: dead, NaN, and no part in the regions."""
    (b, bt, labels) = hand_case()
    for (c, (rb, rt)) in enumerate([([1.0, 2.0, 3.0], [NAN, NAN]), ([1.0, NAN, NAN], [2.0, NAN]), ([4.0, NAN, 4.0], [4.0, NAN])]):
        (b2, bt2) = (b.copy(), bt.copy())
        (b2[c], bt2[c]) = (rb, rt)
        for variance in MR.VARIANCES:
            full = MR.group_test(b, bt, labels, variance)
            ref = MR.group_test(b2, bt2, labels, variance)
            assert math.isnan(ref["t"][c]) and ref["count_t"][c] == 0 and math.isnan(ref["p_t"][c]) and math.isnan(ref["p_fwe_t"][c])
            for n in range(3):
                lost = full["t"][c] ** 2 if c in BR.edges_of(3)[n] else 0.0
                nptest.assert_allclose(ref["region"][n], full["region"][n] - lost, rtol=1e-13)
            net = MR.network_test(b2, bt2, labels, 1.0, "both", variance)
            assert not net["edge_mask"][c] and math.isnan(net["t"][c])


@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_loop_reference_against_the_exact_form(variance):
    # integer rows with missing values: t and the sums; real rows (no ties): the counts and the p-values too
    rng = np.random.default_rng(21)
    (N, H, U, P) = (7, 5, 5, 30)
    X = MR.integer_rows_missing(21, H + U, rng, 0.15)
    labels = BR.make_data(N, H, U, P, 3)[2]
    (b, bt) = (np.ascontiguousarray(X[:, :H]), np.ascontiguousarray(X[:, H:]))
    ex = MR.Exact(b, bt, labels, variance)
    assert all(ex.integer) and np.isnan(X).sum() > 10
    ref = MR.group_test(b, bt, labels, variance)
    got = ex.group_test()
    for k in ("t", "region", "null_max_t", "null_max_region"):
        nptest.assert_allclose(ref[k], got[k], rtol=1e-12, err_msg=k)
    for k in ("n_controls", "n_patients"):
        nptest.assert_array_equal(ref[k], got[k])
    (b, bt, labels) = MR.make_missing(BR.SHAPES[1], 0.1)
    ex = MR.Exact(b, bt, labels, variance)
    ex.check_conditions(thresholds=(1.5,))
    ref = MR.group_test(b, bt, labels, variance)
    got = ex.group_test()
    assert set(got) == set(ref) - {"null_t", "null_region"}
    for k in ("t", "region", "null_max_t", "null_max_region"):
        nptest.assert_allclose(ref[k], got[k], rtol=1e-11, err_msg=k)
    for k in ("count_t", "count_region", "p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(ref[k], got[k], err_msg=k)
    assert (ref["count_t"] > 0).any() and np.isnan(ref["null_t"][:, ~np.isnan(ref["t"])]).any() == (variance == "welch")
    net = MR.network_test(b, bt, labels, 1.5, "greater", variance)
    netx = ex.network_test(1.5, "greater")
    for k in netx:
        if k == "t":
            nptest.assert_allclose(net[k], netx[k], rtol=1e-11)
        elif k not in ("threshold", "tail"):
            nptest.assert_array_equal(net[k], netx[k], err_msg=k)
    assert net["edge_mask"].sum() > 3


def test_exact_form_on_engineered_rows():
    """t^2 exactly 4 with a missing control, and complete separation under Welch: +/-inf with the sign of A."""
    rng = np.random.default_rng(5)
    (H, U) = (5, 4)
    X = MR.integer_rows_missing(6, H + U, rng, 0.1)
    X[0] = [-3, -1, 0, 0, NAN, 3, 1, 0, 0]
    X[1] = [3, 1, 0, 0, NAN, -3, -1, 0, 0]
    X[2] = [0, 0, 0, 0, 0, 8, 8, 8, NAN]                # 5 at 0 and 3 at 8: sum 24, n = 8, mean 3
    X[3] = [7, 7, 7, NAN, NAN, 0, 0, 0, 0]              # 3 at 7 and 4 at 0: sum 21, n = 7, mean 3; the patients are the lower
    labels = BR.make_data(4, H, U, 8, 1)[2]
    for variance in MR.VARIANCES:
        ex = MR.Exact(X[:, :H], X[:, H:], labels, variance)
        assert ex.t2[0][0] == 4 and ex.t2[0][1] == 4 and ex.A[0][0] == 4 and ex.A[0][1] == -4
        assert ex.t2[0][2] == math.inf and ex.t2[0][3] == math.inf and all(ex.integer[:4])
        t = ex.t()
        assert t[0] == 2.0 and t[1] == -2.0 and t[2] == math.inf and t[3] == -math.inf
        bits = ex.bits(2.0, "both")
        assert not bits[0, 0] and not bits[0, 1] and bits[0, 2] and bits[0, 3]
        below = ex.bits(math.nextafter(2.0, 0.0), "greater")
        assert below[0, 0] and not below[0, 1] and below[0, 2] and not below[0, 3]
        ref = MR.group_test(X[:, :H], X[:, H:], labels, variance)
        assert ref["t"][2] == math.inf and ref["t"][3] == -math.inf
        nptest.assert_allclose(ref["t"][:2], [2.0, -2.0], rtol=1e-14)


def test_host_refusals_run_before_any_context():
    rng = np.random.default_rng(0)
    (b, bt) = (rng.normal(size=(6, 5)), rng.normal(size=(6, 4)))
    nan_b = b.copy()
    nan_b[2, 1] = np.nan
    inf_b = b.copy()
    inf_b[2, 1] = -np.inf
    for (fn, args) in ((baseline.group_test, ()), (baseline.network_test, (2.0,))):
        for kw in ({}, {"missing_data": True}):
            with pytest.raises(ValueError, match="variance"):
                fn(b, bt, *args, variance="student", **kw)
            with pytest.raises(ValueError, match="variance"):
                fn(b, bt, *args, variance=None, **kw)
            with pytest.raises(ValueError, match="welch"):
                fn(b, bt[:, :1], *args, variance="welch", **kw)
            with pytest.raises(ValueError, match="welch"):
                fn(b[:, :1], bt, *args, variance="welch", **kw)
            with pytest.raises(ValueError, match="infinite"):
                fn(inf_b, bt, *args, **kw)
            with pytest.raises(ValueError, match="infinite"):
                fn(b, inf_b[:, :4], *args, variance="welch", **kw)
            with pytest.raises(NotImplementedError, match="sessions"):
                fn(b, rng.normal(size=(6, 4, 2)), *args, **kw)
            with pytest.raises(ValueError, match="triangular"):
                fn(b[:5], bt[:5], *args, **kw)
            with pytest.raises(NotImplementedError, match="1024"):
                fn(np.zeros((3, 1000)), np.zeros((3, 25)), *args, **kw)
            with pytest.raises(ValueError, match="n_perm"):
                fn(b, bt, *args, n_perm=0, **kw)
            with pytest.raises(ValueError, match="labels"):
                fn(b, bt, *args, labels=1 - baseline.draw_labels(3, 5, 4, seed=1), **kw)
        # without missing_data a NaN stays refused, whatever the variance
        with pytest.raises(ValueError, match="NaN"):
            fn(nan_b, bt, *args, variance="welch")
        with pytest.raises(ValueError, match="complete"):
            fn(nan_b, bt, *args)
    with pytest.raises(NotImplementedError, match="1024"):
        baseline.network_test(np.zeros((1025 * 1024 // 2, 2)), np.zeros((1025 * 1024 // 2, 2)), 2.0, missing_data=True)
    with pytest.raises(ValueError, match="needs 3"):
        baseline.group_test(np.zeros((3, 1)), np.zeros((3, 1)), missing_data=True)
    with pytest.raises(ValueError, match="tail"):
        baseline.network_test(b, bt, 2.0, tail="up", missing_data=True)


def test_options_reach_the_device():
    """With an option set the call passes the host checks and reaches for the device (and fails here without one)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(0)
    (b, bt) = (rng.normal(size=(6, 5)), rng.normal(size=(6, 4)))
    nan_b = b.copy()
    nan_b[2, 1] = np.nan
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.group_test(nan_b, bt, missing_data=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.network_test(b, bt, 2.0, variance="welch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.network_test(nan_b, bt, 2.0, missing_data=True, variance="welch")


def test_header_binding_and_library_agree():
    names = ("fcd_baseline_group_perm_opt", "fcd_baseline_network_bits_opt")
    text = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES[names[0]][1]) == len(_lib.SIGNATURES["fcd_baseline_group_perm"][1]) + 3
    assert len(_lib.SIGNATURES[names[1]][1]) == len(_lib.SIGNATURES["fcd_baseline_network_bits"][1]) + 1
    assert re.search(r"#define\s+FCD_BASELINE_MISSING\s+1\b", header) and re.search(r"#define\s+FCD_BASELINE_WELCH\s+2\b", header)
    assert (baseline.FLAG_MISSING, baseline.FLAG_WELCH) == (1, 2)
    assert lib.fcd_abi_version() == 4


def test_docstrings_state_the_rules():
    for fn in (baseline.group_test, baseline.network_test):
        assert "missing_data" in fn.__doc__ and "welch" in fn.__doc__
    assert "exceedance" in baseline.group_test.__doc__ and "conservative" in baseline.group_test.__doc__
    assert "Welch's t" not in baseline.group_test.__doc__.split("Not provided:")[1]
    assert "missing data" not in baseline.network_test.__doc__.split("Not provided:")[1]
