"""
tests/guard_arena.py on the CPU: what carve() hands a case is what Case.alloc hands it, at the start asked for and no better
one, between guards that overlap nothing, and check() sees a byte changed at either edge of a payload and at the far end of a
guard -- so that an empty check() in tests/test_gpu_guard_bands.py means what it says.  Every case of the three registries at
both sizes and both starts; no GPU.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402
import guard_arena as GA  # noqa: E402
from test_gpu_harmonize import HARM_CASES  # noqa: E402
from test_gpu_tangent import TG_CASES  # noqa: E402

ALL_CASES = R.CASES + HARM_CASES + TG_CASES


def test_the_constants_and_the_case_count():
    assert GA.GUARD == 4096 and GA.GUARD >= 512 * 8 and GA.BOUNDARY == 256
    assert len(R.CASES) == 77 and len(ALL_CASES) == 81 and len(set(c.name for c in ALL_CASES)) == 81
    assert GA.start_offset("sixteen", 8) == 16 and GA.start_offset("sixteen", 1) == 16
    assert [GA.start_offset("element", k) for k in (1, 2, 4, 8)] == [1, 2, 4, 8]


def tensors(din, dout):
    return dict(list(R.Case.tensors(din).items()) + list(dout.items()))


@pytest.mark.parametrize("start", GA.STARTS)
@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_carve(case, size, start):
    import torch
    (din0, dout0) = case.alloc(size, "cpu")
    (din, dout, arena) = GA.carve(case, size, "cpu", start, 0xFF)
    # the contract of Case.alloc
    assert sorted(din) == sorted(din0) and sorted(dout) == sorted(dout0)
    assert din["_host"] is din0["_host"] and din["_inout"] == din0["_inout"]
    (got, want) = (tensors(din, dout), tensors(din0, dout0))
    assert sorted(arena.bands) == sorted(want)
    for (k, t) in got.items():
        assert t.shape == want[k].shape and t.dtype == want[k].dtype and t.is_contiguous() and t.device.type == "cpu", k
        # the start asked for, and no better alignment
        size_of = t.element_size()
        if start == "sixteen":
            assert t.data_ptr() % 256 == 16 and t.data_ptr() % 32 == 16, k
        else:
            assert t.data_ptr() % 256 == size_of and t.data_ptr() % (2 * size_of) == size_of, k
            if size_of == 8:
                assert t.data_ptr() % 16 == 8, k
        b = arena.bands[k]
        (base, lo, hi, end) = b.extent()
        assert lo == t.data_ptr() and hi - lo == t.numel() * size_of and lo - base >= GA.GUARD and end - hi == GA.GUARD, k
    assert arena.names_start_at(16 if start == "sixteen" else 8) == sorted(
        k for (k, t) in got.items() if start == "sixteen" or t.element_size() == 8)
    # no two allocations (guards and payloads) overlap
    spans = sorted(arena.bands[k].extent()[::3] for k in got)
    assert all(a[1] <= b[0] for (a, b) in zip(spans, spans[1:]))
    assert arena.check() == []
    # every payload byte written: no guard changes, under either fill's opposite
    for t in got.values():
        R.as_bytes(t).fill_(0x00)
    assert arena.check() == []
    # a changed byte is found, with its tensor, side and offset: each on its own
    for k in sorted(got):
        b = arena.bands[k]
        for (index, side, offset) in ((b.lo - 1, "front", -1), (b.hi, "back", 0), (b.hi + GA.GUARD - 1, "back", GA.GUARD - 1),
                                      (0, "front", -b.lo)):
            assert int(b.raw[index]) == 0xFF
            b.raw[index] = 0x5A
            assert arena.check() == [(k, side, offset)], (k, side, offset)
            b.raw[index] = 0xFF
            assert arena.check() == []
    # the helpers of the registry work on the views unchanged
    R.fill_outputs(dout)
    R.feed(case, din, dict((k, torch.from_numpy(v)) for (k, v) in case.make(size).items()))
    for (k, v) in case.make(size).items():
        assert R.as_bytes(din[k]).numpy().tobytes() == v.tobytes(), k
    for t in dout.values():
        assert bool((R.as_bytes(t) == R.SENTINEL).all())
    assert arena.check() == []


def test_the_zero_fill_and_a_start_per_tensor():
    case = R.BY_NAME["gibbs_steps_blocked_pipelined"]
    (din, dout, arena) = GA.carve(case, "small", "cpu", {"*": "sixteen", "lMf": "element", "f_state": "element"}, 0x00)
    assert dout["lMf"].data_ptr() % 16 == 8 and din["f_state"].data_ptr() % 256 == 1
    assert sorted(arena.names_start_at(16)) == sorted(set(arena.bands) - set(("lMf", "f_state")))
    b = arena.bands["lMf"]
    assert int(b.raw[:b.lo].max()) == 0 and int(b.raw[b.hi:].max()) == 0 and arena.check() == []
    b.raw[b.lo - 3] = 1
    b.raw[b.lo - 2] = 1
    b.raw[b.hi + 5] = 1
    assert arena.check() == [("lMf", "front", -3), ("lMf", "back", 5)]
    with pytest.raises(AssertionError):
        GA.carve(case, "small", "cpu", "page", 0xFF)
    with pytest.raises(AssertionError):
        GA.carve(case, "small", "cpu", "sixteen", 0x5A)
