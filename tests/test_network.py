"""
The network-based statistic without a GPU: the reference (network_ref.py) on graphs worked by hand and on the two-against-two
case of test_baseline.py, the host half (network_pvalues), the host-side refusals of baseline.network_test and
baseline.graph_components (they run before any context exists), and that header, binding and Makefile agree on the two entry
points.
"""
import math
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_ref as BR
import network_ref as NR
from conftest import ROOT
from fcdiff_amd import _lib, baseline, util


def mask_of(N, edges):
    m = np.zeros(util.N_to_C(N), dtype=bool)
    for (n, k) in edges:
        m[util.nm_to_c(max(n, k), min(n, k))] = True
    return m


def test_reference_components_by_hand():
    ref = NR.components(mask_of(5, [(1, 0), (2, 1), (4, 3)]), 5)
    assert ref["component"].tolist() == [0, 0, 0, 3, 3]
    assert ref["component_label"].tolist() == [0, 3]
    assert ref["component_edges"].tolist() == [2, 1] and ref["component_regions"].tolist() == [3, 2]
    assert (ref["n_edges"], ref["max_extent"], ref["max_regions"]) == (3, 2, 3)
    # a triangle has more connections than a path over as many regions; equal extents are ordered by label
    ref = NR.components(mask_of(7, [(6, 5), (5, 4), (2, 1), (2, 0), (1, 0)]), 7)
    assert ref["component"].tolist() == [0, 0, 0, -1, 4, 4, 4]
    assert ref["component_label"].tolist() == [0, 4] and ref["component_edges"].tolist() == [3, 2]
    ref = NR.components(mask_of(6, [(5, 4), (1, 0), (3, 2)]), 6)
    assert ref["component_label"].tolist() == [0, 2, 4] and ref["component_edges"].tolist() == [1, 1, 1]
    # labels travel against the index order: 0 - 4 - 1 - 3
    ref = NR.components(mask_of(5, [(4, 0), (4, 1), (3, 1)]), 5)
    assert ref["component"].tolist() == [0, 0, -1, 0, 0] and ref["max_regions"] == 4
    ref = NR.components(np.zeros(10, dtype=bool), 5)
    assert (ref["component"] == -1).all() and ref["component_label"].shape == (0,)
    assert (ref["n_edges"], ref["max_extent"], ref["max_regions"]) == (0, 0, 0)


def two_against_two():
    row = np.array([0.0, 2.0, 5.0, 7.0])
    b = np.stack([row[:2], row[:2] * 2.0, np.array([1.0, 4.0])])
    bt = np.stack([row[2:], row[2:] * 2.0, np.array([2.0, 3.0])])
    labels = np.array([[1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0]], dtype=np.uint8)
    return b, bt, labels


@pytest.mark.parametrize("tail", ["both", "greater", "less"])
def test_reference_on_the_two_against_two_case(tail):
    """t = (5/sqrt 2, 5/sqrt 2, 0) on connections (1,0), (2,0), (2,1); row 0 is the swapped labelling (-t), row 1 the observed."""
    (b, bt, labels) = two_against_two()
    ref = NR.network_test(b, bt, labels, 3.0, tail)
    nptest.assert_allclose(ref["t"], [5.0 / math.sqrt(2.0)] * 2 + [0.0], rtol=1e-14, atol=1e-15)
    if tail == "less":            # only the swapped labelling has t < -3
        assert not ref["edge_mask"].any() and ref["component"].tolist() == [-1, -1, -1]
        assert ref["component_label"].shape == ref["p_fwe"].shape == (0,) and np.isnan(ref["p_fwe_region"]).all()
        assert ref["null_max_extent"].tolist() == [2, 0, 0]
    else:
        assert ref["edge_mask"].tolist() == [True, True, False] and ref["component"].tolist() == [0, 0, 0]
        assert ref["component_label"].tolist() == [0] and ref["component_edges"].tolist() == [2]
        assert ref["component_regions"].tolist() == [3]
        # "both": the swapped and the observed row reach extent 2; "greater": the observed row alone
        (want_null, count) = (([2, 2, 0], 2) if tail == "both" else ([0, 2, 0], 1))
        assert ref["null_max_extent"].tolist() == want_null and ref["null_n_edges"].tolist() == want_null
        assert ref["null_max_regions"].tolist() == [3 if v else 0 for v in want_null]
        assert ref["p_fwe"].tolist() == [(1.0 + count) / 4.0] and ref["p_fwe_region"].tolist() == [(1.0 + count) / 4.0] * 3
    above = NR.network_test(b, bt, labels, 4.0, tail)         # 3.54 < 4: nothing anywhere
    assert not above["edge_mask"].any() and above["null_max_extent"].tolist() == [0, 0, 0]
    assert above["p_fwe"].shape == (0,) and np.isnan(above["p_fwe_region"]).all() and above["p_fwe_region"].shape == (3,)


def test_host_pvalues_match_the_reference():
    assert baseline.network_pvalues(np.array([3, 1]), np.array([0, 1, 3, 5])).tolist() == [3.0 / 5.0, 4.0 / 5.0]     # >=
    assert baseline.network_pvalues(np.zeros(0, dtype=np.int64), np.array([1, 2])).shape == (0,)
    seen = 0
    for (shape, thr) in ((BR.SHAPES[1], 2.0), (BR.SHAPES[4], 2.5), (BR.SHAPES[0], 1.5)):
        (_b, _bt, _labels, ref) = NR.case(shape, thr)
        nptest.assert_array_equal(baseline.network_pvalues(ref["component_edges"], ref["null_max_extent"]), ref["p_fwe"])
        seen += ref["p_fwe"].shape[0]
    assert seen >= 4


def test_host_tables_match_the_reference():
    """What network_test and graph_components derive on the host from `component` and the mask."""
    for (shape, thr) in ((BR.SHAPES[1], 2.5), (BR.SHAPES[4], 2.0)):
        (_b, _bt, _labels, ref) = NR.case(shape, thr)
        (label, edges, regions) = baseline._component_tables(ref["component"], ref["edge_mask"])
        for (got, key) in ((label, "component_label"), (edges, "component_edges"), (regions, "component_regions")):
            assert got.dtype == np.int64 and np.array_equal(got, ref[key]), key
    (label, edges, regions) = baseline._component_tables(np.full(5, -1, dtype=np.int64), np.zeros(10, dtype=bool))
    assert label.shape == edges.shape == regions.shape == (0,)


def test_host_refusals_run_before_any_context():
    rng = np.random.default_rng(0)
    (b, bt) = (rng.normal(size=(6, 5)), rng.normal(size=(6, 4)))
    nan_b = b.copy()
    nan_b[2, 1] = np.nan
    fn = baseline.network_test
    with pytest.raises(NotImplementedError, match="sessions"):
        fn(b, rng.normal(size=(6, 4, 2)), 2.0)
    with pytest.raises(ValueError, match="triangular"):
        fn(b[:5], bt[:5], 2.0)
    with pytest.raises(ValueError, match="connections"):
        fn(b, bt[:3], 2.0)
    with pytest.raises(ValueError, match="complete"):
        fn(nan_b, bt, 2.0)
    with pytest.raises(ValueError, match="NaN"):
        fn(bt, nan_b, 2.0)
    with pytest.raises(NotImplementedError, match="1024"):
        fn(np.zeros((3, 1000)), np.zeros((3, 25)), 2.0)
    with pytest.raises(ValueError, match="needs 3"):
        fn(np.zeros((3, 1)), np.zeros((3, 1)), 2.0)
    with pytest.raises(ValueError, match="n_perm"):
        fn(b, bt, 2.0, n_perm=0)
    good = baseline.draw_labels(3, 5, 4, seed=1)
    for bad in (good[:, :8], good.astype(np.int64) * 2, good[0], 1 - good, np.zeros((0, 9), dtype=np.uint8)):
        with pytest.raises(ValueError, match="labels"):
            fn(b, bt, 2.0, labels=bad)
    for bad in (0.0, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="threshold"):
            fn(b, bt, bad)
    for bad in ("two-sided", "", None, 0):
        with pytest.raises(ValueError, match="tail"):
            fn(b, bt, 2.0, tail=bad)
    C = util.N_to_C(1025)
    with pytest.raises(NotImplementedError, match="1024"):
        fn(np.zeros((C, 2)), np.zeros((C, 2)), 2.0)
    with pytest.raises(NotImplementedError, match="1024"):
        baseline.graph_components(np.zeros(C, dtype=bool))
    with pytest.raises(ValueError, match="triangular"):
        baseline.graph_components(np.zeros((2, 5), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        baseline.graph_components(np.zeros((2, 2, 3), dtype=bool))
    assert baseline.MAX_REGIONS == 1024


def test_header_binding_and_makefile_agree():
    names = ("fcd_baseline_network_bits", "fcd_graph_components")
    header = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    make = open(os.path.join(ROOT, "fcdiff_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    source = open(os.path.join(ROOT, "fcdiff_amd", "csrc", "fcd_baseline.hip")).read()
    assert "fcd_baseline.hip" in srcs and re.search(r"fcd_baseline\$\(SUF\).*-amdgpu-mfma-vgpr-form=1", make)
    lib = _lib.load()
    for (name, n_args) in zip(names, (13, 9)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]) == n_args
        assert re.search(r'extern "C" int %s\(' % name, source) and hasattr(lib, name)
    assert lib.fcd_abi_version() == 4 == _lib.ABI_VERSION


def test_docstrings_say_where_the_statistic_lives():
    assert "network_test()" in baseline.group_test.__doc__
    for word in ("intensity", "TFCE", "1024 regions"):
        assert word in baseline.network_test.__doc__
