"""
Component intensity of the network-based statistic without a GPU: the reference (network_intensity_ref.py) on a graph worked by
hand, what the device test's case list covers (asserted on the reference), the host half (network_intensity_pvalues), the
host-side refusals (they run before any context exists), and that header, binding and Makefile agree on the two entry points.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import network_intensity_ref as IR
import network_ref as NR
from conftest import ROOT
from fcdiff_amd import _lib, baseline

THRESHOLDS = (1.5, 2.0, 2.5)
CASES = [(shape, thr, "both") for shape in NR.SHAPES for thr in THRESHOLDS] + \
        [(shape, 2.0, tail) for shape in (NR.SHAPES[1], NR.SHAPES[8]) for tail in ("greater", "less")]


def test_reference_by_hand():
    """Four regions, connections (1,0) (2,0) (2,1) (3,0) (3,1) (3,2); connection 4 is dead (NaN under the observed labelling)."""
    nan = math.nan
    t = np.array([2.5, 1.0, -2.25, 0.5, nan, 9.0])
    tp = np.array([[0.1, -0.2, 0.3, 0.0, 1.0, 1.9],            # nothing above 2: an empty graph, 0.0
                   [math.inf, 0.0, 0.0, 0.0, 0.0, 3.0],        # a separated connection: inf, and 1.0 beside it
                   [0.0, 0.0, 0.0, 0.0, 5.0, 2.5]])            # the dead connection's 5.0 adds nothing: 0.5
    ref = IR.from_t(t, tp, 2.0, "both")                          # edges (1,0) (2,1) (3,2): one path over all four regions
    assert ref["component"].tolist() == [0, 0, 0, 0] and ref["component_edges"].tolist() == [3]
    assert ref["component_intensity"].tolist() == [0.5 + 0.25 + 7.0]
    assert ref["null_max_intensity"].tolist() == [0.0, math.inf, 0.5] and ref["null_max_extent"].tolist() == [0, 1, 1]
    assert ref["p_fwe"].tolist() == [2.0 / 4.0] and ref["p_fwe_extent"].tolist() == [1.0 / 4.0]
    assert ref["p_fwe_region"].tolist() == [0.5] * 4 and ref["statistic"] == "intensity"
    assert ref["null_arg_extent"].tolist() == [0, 1, 1] and ref["null_extent_of_max"].tolist() == [True, True, True]
    ref = IR.from_t(t, tp, 2.0, "greater")                       # (1,0) and (3,2): two components of one connection each
    assert ref["component_label"].tolist() == [0, 2] and ref["component_edges"].tolist() == [1, 1]
    assert ref["component_intensity"].tolist() == [0.5, 7.0]     # ordered by extent, then label: not by intensity
    assert ref["p_fwe"].tolist() == [3.0 / 4.0, 2.0 / 4.0] and ref["p_fwe_extent"].tolist() == [3.0 / 4.0, 3.0 / 4.0]
    ref = IR.from_t(t, tp, 2.0, "less")                          # (2,1) alone
    assert ref["component"].tolist() == [-1, 1, 1, -1] and ref["component_intensity"].tolist() == [0.25]
    assert ref["null_max_intensity"].tolist() == [0.0, 0.0, 0.0] and ref["p_fwe"].tolist() == [0.25]
    assert np.isnan(ref["p_fwe_region"][[0, 3]]).all() and ref["p_fwe_region"][1] == 0.25
    # an observed +inf is met only by a null +inf
    ref = IR.from_t(np.array([math.inf, 0, 0, 0, 0, 0.0]), tp, 2.0, "both")
    assert ref["component_intensity"].tolist() == [math.inf] and ref["p_fwe"].tolist() == [2.0 / 4.0]
    # weights are read only where the mask is set; the sum is fsum's
    w = np.array([nan, 0.1, -1.0, 0.2, 1e16, 1.0])
    out = IR.weighted_components(np.array([0, 1, 0, 1, 1, 1], dtype=bool), w, 4)
    assert out["component_weight"].tolist() == [math.fsum([0.1, 0.2, 1e16, 1.0])] and out["max_weight"] == out["component_weight"][0]
    assert IR.weighted_components(np.zeros(6, dtype=bool), w, 4)["max_weight"] == 0.0


def test_host_pvalues():
    p = baseline.network_intensity_pvalues([0.5, 7.0, math.inf, 0.0], [0.0, math.inf, 0.5])
    assert p.tolist() == [3.0 / 4.0, 2.0 / 4.0, 2.0 / 4.0, 1.0]
    assert baseline.network_intensity_pvalues([], [1.0]).shape == (0,)


def test_reference_cases_cover_the_ground():
    """Asserted on the reference: the device test's cases separate intensity from extent, and no comparison is a near tie."""
    (differ, gap) = (0, math.inf)
    for (shape, thr, tail) in CASES:
        ref = IR.case(shape, thr, tail)[3]
        assert NR.threshold_gap(ref["t"], ref["null_t"], thr) > 1e-9
        if tail == "both":
            differ += int((~ref["null_extent_of_max"]).sum())
        gap = min(gap, IR.intensity_gap(ref))
    print("labellings whose largest-intensity component is not a largest-extent one: %d; smallest relative gap: %.3g" % (differ, gap))
    assert differ >= 20
    assert gap >= 1e-6


def test_host_refusals_come_before_any_context(monkeypatch):
    def no_context():
        raise AssertionError("a context was made")
    monkeypatch.setattr(_lib, "Context", no_context)
    (b, bt) = (np.zeros((6, 3)), np.ones((6, 3)))
    for bad in ("size", "", None, "Intensity"):
        with pytest.raises(ValueError, match="statistic"):
            baseline.network_test(b, bt, 2.0, n_perm=4, statistic=bad)
    mask = np.array([1, 0, 1, 0, 0, 1], dtype=bool)
    good = np.array([1.0, np.nan, 0.0, -3.0, np.nan, math.inf])    # (NaN and negative only where the mask is not set)
    with pytest.raises(ValueError, match="shape"):
        baseline.graph_components(mask, good[:5])
    with pytest.raises(ValueError, match="shape"):
        baseline.graph_components(mask, np.stack([good, good]))
    with pytest.raises(ValueError, match="shape"):
        baseline.graph_components(np.stack([mask, mask]), good)
    with pytest.raises(ValueError, match="float64"):
        baseline.graph_components(mask, good.astype(np.float32))
    with pytest.raises(ValueError, match="float64"):
        baseline.graph_components(mask, np.ones(6, dtype=np.int64))
    for (at, value) in ((0, np.nan), (2, -1e-300), (5, -math.inf)):
        w = good.copy()
        w[at] = value
        with pytest.raises(ValueError, match=">= 0 and not NaN"):
            baseline.graph_components(mask, w)
    with pytest.raises(AssertionError, match="a context was made"):  # the good weights pass every host check
        baseline.graph_components(mask, good)
    assert baseline.STATISTICS == ("extent", "intensity")
    assert baseline._excess_chunk(1) == (256 << 20) // 256 and baseline._excess_chunk(16368) == 64 and baseline._excess_chunk(1 << 40) == 1


def test_header_binding_and_makefile_agree():
    names = {"fcd_baseline_network_excess": ("fcd_network_excess_desc", _lib.NetworkExcessDesc),
             "fcd_graph_components_weighted": ("fcd_components_desc", _lib.ComponentsDesc)}
    header = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    make = open(os.path.join(ROOT, "fcdiff_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    source = open(os.path.join(ROOT, "fcdiff_amd", "csrc", "fcd_baseline.hip")).read()
    assert "fcd_baseline.hip" in srcs
    lib = _lib.load()
    for (name, (struct, binding)) in names.items():
        assert re.search(r"\bint\s+%s\s*\(\s*fcd_ctx \*ctx,\s*const %s \*d\s*\)\s*;" % (name, struct), header), name
        assert _lib.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
        assert re.search(r'extern "C" int %s\(' % name, source) and hasattr(lib, name)
        # the members of the header's struct, in its order, are the binding's fields
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
        members = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                members += [m.strip().lstrip("*") for m in re.sub(r"^.*?(\**\w+(\s*,\s*\**\w+)*)$", r"\1", decl).split(",")]
        assert members == [f[0] for f in binding._fields_], (name, members)
        assert lib and getattr(lib, name)(None, None) == _lib.FCD_ERR_ARG
    assert ctypes.sizeof(_lib.NetworkExcessDesc) == 8 + 4 * 8 + 8 + 8 + 9 * 8 and ctypes.sizeof(_lib.ComponentsDesc) == 8 + 16 + 9 * 8
    assert lib.fcd_abi_version() == 4 == _lib.ABI_VERSION
    # the flat entry points keep their parameters
    assert len(_lib.SIGNATURES["fcd_baseline_network_bits"][1]) == 13 and len(_lib.SIGNATURES["fcd_graph_components"][1]) == 9


def test_docstrings():
    for word in ("intensity", "TFCE", "1024 regions", "statistic=\"intensity\"", "null_max_intensity", "p_fwe_extent"):
        assert word in baseline.network_test.__doc__, word
    for word in ("weights", "max_weight", "component_weight"):
        assert word in baseline.graph_components.__doc__, word
