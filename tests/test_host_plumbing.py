"""
The host plumbing every fit and query shares, without a GPU: which library call a table build issues (tables.build, through
UnsharedRegionFit / SharedRegionFit._update_lps and score.lik_tables), with which flags, counter and buffers, and the pooling
of the sampler's uint32 tallies (gibbs.pool_u32).  The context is a stand-in that records its calls; tensors live on the CPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fcdiff_amd
from fcdiff_amd import _lib, gibbs, score, tables

# argument positions after the entry point's name (include/fcdiff_hip.h, without the context)
EX = {"S_B": 6, "lM": 7, "lpB": 8, "pBt": 9, "flags": 10, "n_missing": 11, "n_args": 13}       # fcd_lik_tables_ex
SH = {"S_B": 6, "lM": 7, "flags": 8, "n_missing": 9, "n_args": 11}                              # fcd_lik_shared_tables


class Recorder(object):
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))

    def take(self):
        (calls, self.calls) = (self.calls, [])
        return calls


@pytest.fixture(autouse=True)
def no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "stream_ptr", lambda: C.c_void_p(0))


def address(arg):
    return arg.value or 0


def data(N=5, H=3, U=4, nan=False):
    (_r, _t, _f, _ft, b, bt) = fcdiff_amd.UnsharedRegionModel().sample_fast(N, H, U, seed=3)
    if nan:
        (b[1, 0], bt[2, 1], bt[0, 3]) = (np.nan, np.nan, np.nan)
    return b, bt


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_one_library_call_per_table_build(shared, missing):
    (N, H, U) = (5, 3, 4)
    fit = (fcdiff_amd.fit.SharedRegionFit if shared else fcdiff_amd.fit.UnsharedRegionFit)()
    rec = fit._ctx = Recorder()
    fit.model = fcdiff_amd.SharedRegionModel() if shared else fcdiff_amd.UnsharedRegionModel()
    (fit.b, fit.bt) = data(N, H, U, nan=missing)
    fit.missing_data = missing
    fit._init_lps(N, H, U)
    assert rec.take() == []
    assert tuple(fit._d["lM"].shape) == ((10, 1, 3, 3) if shared else (10, U, 3, 3))
    assert tuple(fit._d["lq_R"].shape) == ((N, 1, 2) if shared else (N, U, 2))
    assert float(fit._d["lM"].flatten()[0]) == (0.0 if shared else 1.0)
    (name, pos) = ("fcd_lik_shared_tables", SH) if shared else ("fcd_lik_tables_ex", EX)
    flags = _lib.FCD_DATA_NAN_MISSING if missing else 0
    kept = (fit._d["S_B"].data_ptr(), fit._d["lM"].data_ptr())
    # first build (the data is uploaded: a counting build under missing_data), second build, a build after invalidate_data()
    for (step, counts) in (("first", missing), ("second", False), ("invalidated", missing)):
        if step == "invalidated":
            fit.invalidate_data()
        fit._update_lps()
        calls = rec.take()
        assert [c[0] for c in calls] == [name], step
        args = calls[0][1]
        assert len(args) == pos["n_args"] and args[2:5] == (10, H, U)
        assert args[pos["flags"]] == flags, step
        assert (address(args[pos["n_missing"]]) != 0) == counts, step
        if counts:
            assert address(args[pos["n_missing"]]) == fit._d["n_missing"].data_ptr()
        assert (fit._d["S_B"].data_ptr(), fit._d["lM"].data_ptr()) == kept, step
        assert (address(args[pos["S_B"]]), address(args[pos["lM"]])) == kept, step
        if not shared:
            assert address(args[EX["lpB"]]) == 0 and address(args[EX["pBt"]]) == 0
        assert fit._d["n_missing_valid"] is missing
    # the per-item tables: still one call; the shared model has none
    fit._tables(full=True)
    calls = rec.take()
    assert [c[0] for c in calls] == [name]
    if shared:
        assert fit._d["lpB"] is None and fit._d["pBt"] is None
    else:
        assert tuple(fit._d["lpB"].shape) == (10, H, 3) and tuple(fit._d["pBt"].shape) == (10, U, 3)
        assert address(calls[0][1][EX["lpB"]]) == fit._d["lpB"].data_ptr()
        assert address(calls[0][1][EX["pBt"]]) == fit._d["pBt"].data_ptr()
    assert (fit._d["S_B"].data_ptr(), fit._d["lM"].data_ptr()) == kept
    # a table of another shape is replaced, not written over
    fit._d["lM"] = torch.zeros((10, U + 1, 3, 3), dtype=torch.float64)
    fit._update_lps()
    assert tuple(fit._d["lM"].shape) == ((10, 1, 3, 3) if shared else (10, U, 3, 3)) and len(rec.take()) == 1


@pytest.mark.parametrize("shared", [False, True])
def test_build_allocates_only_what_it_is_not_given(shared):
    rec = Recorder()
    (b, bt) = (torch.as_tensor(a) for a in data(5, 3, 4))
    theta = fcdiff_amd.UnsharedRegionModel().theta()
    (S_B, lM) = tables.build(rec, b, bt, theta, 0, shared=shared)
    assert tuple(S_B.shape) == (10, 3) and tuple(lM.shape) == (10, 1 if shared else 4, 3, 3)
    assert S_B.dtype == lM.dtype == torch.float64 and len(rec.take()) == 1
    (S2, lM2) = tables.build(rec, b, bt, theta, 0, shared=shared, S_B=S_B, lM=lM)
    assert S2 is S_B and lM2 is lM
    ((name, args),) = rec.take()
    pos = SH if shared else EX
    assert (address(args[pos["S_B"]]), address(args[pos["lM"]])) == (S_B.data_ptr(), lM.data_ptr())
    assert [float(x) for x in args[5][0:12]] == [float(x) for x in theta]


@pytest.mark.parametrize("missing", [False, True])
def test_score_lik_tables_is_the_same_call(missing):
    rec = Recorder()
    (b, bt) = (torch.as_tensor(a) for a in data(5, 3, 2))
    (S_B, lM) = score.lik_tables(rec, b, bt, fcdiff_amd.UnsharedRegionModel().theta(), missing)
    assert tuple(S_B.shape) == (10, 3) and tuple(lM.shape) == (10, 2, 3, 3)
    ((name, args),) = rec.take()
    assert name == "fcd_lik_tables_ex" and args[EX["flags"]] == (_lib.FCD_DATA_NAN_MISSING if missing else 0)
    assert [address(args[EX[k]]) for k in ("lpB", "pBt", "n_missing")] == [0, 0, 0]


def test_one_writer_of_the_hyper_block():
    rec = Recorder()
    m = fcdiff_amd.UnsharedRegionModel()
    hyper = score.hyper_block(rec, m.gamma, m.pi2(), "cpu")
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit._ctx, fit.model) = (rec, m)
    block = fit._hyper()
    fit._hyper()                                       # unchanged values: not written again
    eng = gibbs.GibbsEngine.__new__(gibbs.GibbsEngine)
    (eng.ctx, eng.hyper) = (rec, torch.zeros(8, dtype=torch.float64))
    eng.set_hyper(m.gamma, m.pi2())
    calls = rec.take()
    assert [c[0] for c in calls] == ["fcd_hyper_set"] * 3
    assert [address(c[1][0]) for c in calls] == [hyper.data_ptr(), block.data_ptr(), eng.hyper.data_ptr()]
    for (_name, args) in calls:
        assert list(args[1][0:3]) == list(np.asarray(m.gamma, dtype=np.float64)) and list(args[2][0:2]) == list(m.pi2())
    with pytest.raises(ValueError):
        tables.write_hyper(rec, hyper, [0.5, 0.5], m.pi2())


def test_pool_u32_reads_int32_storage_as_uint32():
    want = np.array([[0, 1, 2 ** 31 - 1], [2 ** 31, 2 ** 31 + 5, 2 ** 32 - 1]], dtype=np.uint32)
    held = torch.as_tensor(want.view(np.int32).copy())
    assert held.dtype == torch.int32 and int(held.min()) < 0
    got = gibbs.pool_u32(held)
    assert got.dtype == torch.int64 and tuple(got.shape) == (2, 3)
    assert np.array_equal(got.numpy(), want.astype(np.int64))
    assert np.array_equal(held.numpy().view(np.uint32), want)          # the tally itself is left as it was
