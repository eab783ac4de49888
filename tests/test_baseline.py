"""
The classical baselines without a GPU: the reference (baseline_ref.py) against closed forms on a 3-region case worked by hand,
the host-side refusals of fcdiff_amd.baseline (they run before any context exists, so they raise here, where there is no
device), the label draw, and that header, binding and Makefile agree on the two entry points.
"""
import math
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_ref as BR
import fcdiff_amd
from conftest import ROOT
from fcdiff_amd import _lib, baseline


def test_reference_normative_closed_forms():
    """Controls 1, 2, 3, 4 (+ a shift per connection) and one patient: mean 2.5, s^2 = 5/3; deleting a control by hand."""
    base = np.array([1.0, 2.0, 3.0, 4.0])
    b = np.stack([base, base + 10.0, 2.0 * base])              # connections (1,0), (2,0), (2,1)
    bt = np.array([[6.0], [12.5], [np.nan]])
    ref = BR.normative(b, bt, z_threshold=2.0)
    s = math.sqrt(5.0 / 3.0)
    z_want = np.array([[3.5 / (s * math.sqrt(1.25))], [0.0], [np.nan]])
    nptest.assert_allclose(ref["z"], z_want, rtol=1e-14, atol=1e-15)
    # control 4 deleted: the others 1, 2, 3 have mean 2 and deviation 1; control 2 deleted: mean 8/3, variance 7/3
    z0_row = np.array([-math.sqrt(3.0), -1.0 / math.sqrt(7.0), 1.0 / math.sqrt(7.0), math.sqrt(3.0)])
    nptest.assert_allclose(ref["z0"], np.stack([z0_row, z0_row, z0_row]), rtol=1e-13)
    assert ref["n_controls"].tolist() == [4, 4, 4]
    # regions: E(0) = {0, 1}, E(1) = {0, 2}, E(2) = {1, 2}
    z = z_want[0, 0]
    nptest.assert_allclose(ref["msq"][:, 0], [z * z / 2.0, z * z, 0.0], rtol=1e-13)
    assert ref["n_edges"][:, 0].tolist() == [2, 1, 1] and ref["n_over"][:, 0].tolist() == [1, 1, 0]
    m0 = np.array([3.0, 1.0 / 7.0, 1.0 / 7.0, 3.0])
    nptest.assert_allclose(ref["msq0"], np.stack([m0, m0, m0]), rtol=1e-13)
    assert (ref["n_edges0"] == 2).all() and (ref["n_over0"] == 0).all()
    nptest.assert_allclose(ref["max0"], ref["msq0"].max(axis=0), rtol=0)
    # msq = 2.94, 5.88, 0 against a null of {3, 1/7, 1/7, 3}, and against the maxima, which are the same values
    assert ref["p_region"][:, 0].tolist() == [3.0 / 5.0, 1.0 / 5.0, 1.0]
    assert ref["p_fwe"][:, 0].tolist() == [3.0 / 5.0, 1.0 / 5.0, 1.0]


def test_reference_normative_undefined_scores():
    b = np.array([[1.0, 2.0, np.nan, np.nan], [5.0, 5.0, 5.0, 5.0], [1.0, 2.0, 4.0, np.nan]])
    bt = np.array([[1.0], [2.0], [3.0]])
    ref = BR.normative(b, bt)
    assert np.isnan(ref["z"][:2]).all() and np.isnan(ref["z0"][:2]).all()       # n_c < 3; deviation 0
    assert not np.isnan(ref["z"][2, 0]) and np.isnan(ref["z0"][2, 3]) and not np.isnan(ref["z0"][2, :3]).any()
    assert ref["n_controls"].tolist() == [2, 4, 3]
    assert ref["n_edges"][:, 0].tolist() == [0, 1, 1] and np.isnan(ref["msq"][0, 0])
    assert np.isnan(ref["max0"][3]) and math.isnan(ref["p_region"][0, 0])


def test_reference_group_closed_forms():
    """Two against two: the textbook t of (0, 2) against (5, 7) is 5 / sqrt 2; the swapped labelling gives -t."""
    row = np.array([0.0, 2.0, 5.0, 7.0])
    b = np.stack([row[:2], row[:2] * 2.0, np.array([1.0, 4.0])])
    bt = np.stack([row[2:], row[2:] * 2.0, np.array([2.0, 3.0])])
    labels = np.array([[1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0]], dtype=np.uint8)
    ref = BR.group_test(b, bt, labels)
    t0 = 5.0 / math.sqrt(2.0)
    nptest.assert_allclose(ref["t"], [t0, t0, 0.0], rtol=1e-14, atol=1e-15)
    nptest.assert_allclose(ref["region"], [2 * t0 * t0, t0 * t0, t0 * t0], rtol=1e-14)
    nptest.assert_allclose(ref["null_t"][0], -ref["t"], rtol=1e-14, atol=1e-15)
    nptest.assert_array_equal(ref["null_t"][1], ref["t"])
    # row 2 compares (0, 5) with (2, 7): difference 2, pooled variance 12.5
    nptest.assert_allclose(ref["null_t"][2, 0], -2.0 / math.sqrt(12.5), rtol=1e-14)
    assert ref["count_t"].tolist() == [2, 2, 3] and ref["count_region"].tolist() == [2, 2, 2]
    nptest.assert_array_equal(ref["p_t"], np.array([3.0, 3.0, 4.0]) / 4.0)
    nptest.assert_array_equal(ref["p_fwe_region"], np.array([3.0, 3.0, 3.0]) / 4.0)
    nptest.assert_allclose(ref["null_max_t"][:2], [t0, t0], rtol=1e-14)


def test_data_recipe_is_seeded():
    (b, bt, labels) = BR.make_data(*BR.SHAPES[0])
    (b2, bt2, labels2) = BR.make_data(*BR.SHAPES[0])
    assert np.array_equal(b, b2) and np.array_equal(bt, bt2) and np.array_equal(labels, labels2)
    assert b.shape == (21, 5) and bt.shape == (21, 4) and labels.shape == (50, 9) and (labels.sum(axis=1) == 4).all()
    assert bt[:6].mean() - bt[6:].mean() > 0.1
    (bn, btn, _l) = BR.make_data(*BR.SHAPES[1], f=0.1)
    assert np.isnan(bn).any() and np.isnan(btn).any()


def test_host_refusals_run_before_any_context():
    rng = np.random.default_rng(0)
    (b, bt) = (rng.normal(size=(6, 5)), rng.normal(size=(6, 4)))
    nan_b = b.copy()
    nan_b[2, 1] = np.nan
    for fn in (baseline.normative, baseline.group_test):
        with pytest.raises(NotImplementedError, match="sessions"):
            fn(b, rng.normal(size=(6, 4, 2)))
        with pytest.raises(ValueError, match="triangular"):
            fn(b[:5], bt[:5])
        with pytest.raises(ValueError, match="connections"):
            fn(b, bt[:3])
        with pytest.raises(ValueError, match="NaN"):
            fn(nan_b, bt)
        with pytest.raises(ValueError, match="NaN"):
            fn(bt, nan_b)
    with pytest.raises(ValueError, match="complete"):
        baseline.group_test(nan_b, bt)
    with pytest.raises(NotImplementedError, match="1024"):
        baseline.normative(np.zeros((3, 1025)), np.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match="1024"):
        baseline.group_test(np.zeros((3, 1000)), np.zeros((3, 25)))
    with pytest.raises(ValueError, match="n_perm"):
        baseline.group_test(b, bt, n_perm=0)
    good = baseline.draw_labels(3, 5, 4, seed=1)
    for bad in (good[:, :8], good.astype(np.int64) * 2, good[0], 1 - good, np.zeros((0, 9), dtype=np.uint8)):
        with pytest.raises(ValueError, match="labels"):
            baseline.group_test(b, bt, labels=bad)
    assert baseline.MAX_CONTROLS == 1024 and baseline.MAX_SUBJECTS == 1024


def test_missing_data_flag_is_what_admits_nan():
    """With missing_data=True the NaN check is skipped: the call then reaches for the device (and fails here without one)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    b = np.arange(12.0).reshape(3, 4)
    b[0, 0] = np.nan
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        baseline.normative(b, np.ones((3, 2)), missing_data=True)


def test_label_draw_is_reproducible():
    lab = baseline.draw_labels(40, 7, 5, seed=11)
    assert lab.dtype == np.uint8 and lab.shape == (40, 12)
    assert (lab.sum(axis=1) == 5).all() and set(np.unique(lab)) == {0, 1}
    assert np.array_equal(lab, baseline.draw_labels(40, 7, 5, seed=11))
    assert not np.array_equal(lab, baseline.draw_labels(40, 7, 5, seed=12))
    rng = np.random.default_rng(11)
    for p in range(40):
        assert sorted(np.flatnonzero(lab[p])) == sorted(rng.permutation(12)[:5])


def test_host_pvalues_match_the_reference():
    """The host half of both functions on the reference's own arrays."""
    (b, bt, labels) = BR.make_data(*BR.SHAPES[4], f=0.2)
    ref = BR.normative(b, bt)
    (max0, p_region, p_fwe) = baseline.normative_pvalues(ref["msq"], ref["msq0"])
    nptest.assert_array_equal(max0, ref["max0"])
    nptest.assert_array_equal(p_region, ref["p_region"])
    nptest.assert_array_equal(p_fwe, ref["p_fwe"])
    (b, bt, labels) = BR.make_data(*BR.SHAPES[0])
    g = BR.group_test(b, bt, labels)
    pv = baseline.group_pvalues(g["t"], g["region"], g["null_max_t"], g["null_max_region"], g["count_t"], g["count_region"])
    for k in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(pv[k], g[k])


def test_header_binding_and_makefile_agree():
    names = ("fcd_baseline_normative", "fcd_baseline_group_perm")
    header = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    make = open(os.path.join(ROOT, "fcdiff_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "fcd_baseline.hip" in srcs and os.path.exists(os.path.join(ROOT, "fcdiff_amd", "csrc", "fcd_baseline.hip"))
    assert re.search(r"fcd_baseline\$\(SUF\).*-amdgpu-mfma-vgpr-form=1", make)
    lib = _lib.load()
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name)
    assert lib.fcd_abi_version() == 4


def test_package_exports_the_module():
    assert "baseline" in fcdiff_amd.__all__ and fcdiff_amd.baseline is baseline
    assert "one degree of freedom fewer" in baseline.normative.__doc__ and "conservative" in baseline.normative.__doc__
