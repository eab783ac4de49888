"""
The registry of tests/caller_stream_cases.py against the header: every prototype of include/fcdiff_hip.h that takes an
fcd_stream is called by some case or is exempt with a reason, so an entry point added later fails here until it has a
case -- and with it runs on a caller's stream (tests/test_gpu_caller_stream.py) and on a context that other families have
used (tests/test_gpu_context_reuse.py).  CPU only: the cases are built, none is run.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fcdiff_hip.h")


def stream_prototypes(text):
    """the names of the functions declared with an fcd_stream among their parameters"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(fcd_\w+)\s*\(([^;{}]*?)\)\s*;", text) if re.search(r"\bfcd_stream\b", m.group(2)))


def uncovered(prototypes, cases, exempt):
    named = set(e for c in cases for e in c.entry_points)
    return sorted(set(prototypes) - named - set(exempt))


def header_prototypes():
    with open(HEADER) as fh:
        return stream_prototypes(fh.read())


def test_the_parser_finds_the_prototypes():
    text = "/* int fcd_not(fcd_stream s); */ int fcd_a(fcd_ctx *c,\n fcd_stream stream);\nint fcd_b(fcd_ctx *c);\ntypedef void *fcd_stream;"
    assert stream_prototypes(text) == ["fcd_a"]
    protos = header_prototypes()
    assert len(protos) > 70 and "fcd_gibbs_run" in protos and "fcd_corr_partial" in protos and "fcd_ctx_create" not in protos


def test_every_stream_entry_point_has_a_case_or_an_exemption():
    protos = header_prototypes()
    missing = uncovered(protos, R.CASES, R.EXEMPT)
    assert not missing, "no case of tests/caller_stream_cases.py calls: %s" % ", ".join(missing)
    # nothing stale either: every name a case or the exemption list gives is a prototype with a stream
    named = set(e for c in R.CASES for e in c.entry_points) | set(R.EXEMPT)
    assert not named - set(protos), sorted(named - set(protos))
    assert not set(R.EXEMPT) & set(e for c in R.CASES for e in c.entry_points)
    for (name, reason) in R.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 5, name


def test_an_emptied_registry_names_what_it_leaves_uncovered():
    protos = header_prototypes()
    assert uncovered(protos, [], R.EXEMPT) == sorted(set(protos) - set(R.EXEMPT))
    lone = [e for e in R.BY_NAME["hyper_set"].entry_points]
    assert uncovered(protos, [c for c in R.CASES if c.name != "hyper_set"], R.EXEMPT) == lone


def test_every_entry_point_of_a_case_is_bound():
    from fcdiff_amd import _lib
    for c in R.CASES:
        for e in c.entry_points:
            assert e in _lib.SIGNATURES, (c.name, e)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_inputs(case):
    """deterministic, within what the family's reference asks of its inputs, and larger at "large" """
    for size in R.SIZES:
        (a, b) = (case.make(size), case.make(size))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (case.name, size, k)
            assert a[k].flags["C_CONTIGUOUS"] and a[k] is not b[k]
        spec = case.spec(size)
        assert set(spec["inout"]) <= set(a), (case.name, size)
        assert not set(spec["outputs"]) & set(a), (case.name, size)
        for (k, (shape, _dt)) in spec["outputs"].items():
            assert all(int(n) >= 1 for n in shape), (case.name, size, k, shape)
        case.conditions(size)
    # a fresh build of the same case gives the same bytes (nothing depends on what was built before it)
    again = R.Case(case.name, case.entry_points, case._build, case._call)
    for (k, v) in again.make("small").items():
        assert v.tobytes() == case.make("small")[k].tobytes(), (case.name, k)
    (small, large) = (case.extents("small"), case.extents("large"))
    assert sorted(small) == sorted(large)
    if case.name in R.ONE_SHAPE:
        assert small == large
        (hs, hl) = (case.host("small"), case.host("large"))
        assert any(not np.array_equal(hs[k], hl[k]) for k in hs), case.name
    else:
        assert small != large, case.name
        grown = [k for k in small if np.prod(large[k]) > np.prod(small[k])]
        assert grown and not [k for k in small if np.prod(large[k]) < np.prod(small[k])], (case.name, small, large)


def test_shapes_are_the_small_ones():
    """the registry's shapes stay at the tile and word edges they were chosen for"""
    (s, l) = (R.DIMS["small"], R.DIMS["large"])
    assert (s["N"], s["H"], s["U"], s["G"], s["T"], s["Q"]) == (17, 3, 3, 64, 40, 2)
    assert (l["N"], l["H"], l["U"], l["G"], l["T"], l["Q"]) == (33, 5, 7, 128, 100, 9)
    assert R.BY_NAME["corr_edges_subject"].host("large")["T"] >= 128          # several time slices per subject
    assert R.BY_NAME["corr_edges_block"].host("small")["N"] > 208             # the block form
    assert R.BY_NAME["corr_partial_chunked"].knobs == {"partial_chunk": 2} and R.BY_NAME["corr_partial_chunked"].host("small")["S"] > 2
