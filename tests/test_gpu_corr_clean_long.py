"""
The cleaning front-end on scans longer than one block of 256 frames (fcd_corr_clean behind fcdiff_amd.corr.clean and
correlations(confounds=, frame_mask=)) against the long-double oracle of tests/corr_clean_ref.py, under the bounds of
tests/test_gpu_corr_clean.py: corr_ref.BOUND for correlations, RESID for residuals, info exactly equal.

What runs here and in no shorter scan (inputs: corr_clean_ref.GPU_LONG_INPUTS, on which tests/test_corr_clean.py finds the
fp64 restatement of the kernels' pipeline inside the same bound):
  clean_index_kernel   walks the mask in chunks of 256 frames and carries the count of kept frames from chunk to chunk:
                       a first chunk with nothing kept, nothing kept behind the first chunk, a whole middle chunk dropped,
                       a dropped run across frame 256 (corr_clean_ref.chunk_masks);
  clean_resid_kernel   blockIdx.x > 0: one lane in the second block (T = 257), the trailing waves' early return there,
                       n_kept exactly 256 with blocks of nothing but zero fill behind it, n_kept = 200 at T = 513 and 700;
                       the instantiations QP = 32, 48 and 56 (Q = 25, 32, 41, 48, 49, 56);
  K_corr               behind them on zero-padded rows of T > 96: its subject kernel slices the time axis, and the slices
                       behind n_kept hold nothing but padding.
"""
import functools

import numpy as np
import numpy.testing as nptest
import pytest

import corr_clean_ref as CR
import corr_ref as R
from test_gpu_corr_clean import RESID, check  # noqa: E402  (the bounds and the comparison of the shorter scans)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd import corr
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib, e.O, e.corr) = (torch, fcdiff_amd, _lib, O, corr)
    e.ctx = _lib.Context()
    return e


@functools.lru_cache(maxsize=None)
def case(i):
    """(ts, confounds, mask, clean_ld result) of GPU_LONG_INPUTS[i]: made once, shared; the tests write to copies only."""
    return CR.gpu_case(CR.GPU_LONG_INPUTS[i])


LONG = list(range(len(CR.GPU_LONG_INPUTS)))
CHUNK = [i for i in LONG if CR.GPU_LONG_INPUTS[i].get("mask") == "chunk"]


def long_id(i):
    return CR.input_id(CR.GPU_LONG_INPUTS[i])


@pytest.mark.parametrize("i", LONG, ids=long_id)
def test_correlations(env, i):
    (ts, cf, mask, cleaned) = case(i)
    (exp, info_exp) = CR.corr_clean_ld(ts, cf, mask, cleaned=cleaned)
    assert np.isfinite(exp).all()
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert np.array_equal(info, info_exp)
    check(got, exp, long_id(i))


@pytest.mark.parametrize("i", LONG, ids=long_id)
def test_residuals(env, i):
    (ts, cf, mask, cleaned) = case(i)
    kw = CR.GPU_LONG_INPUTS[i]
    (resid, info) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    assert resid.shape == ts.shape and resid.dtype == np.float64
    assert np.array_equal(info, cleaned["info"])
    assert np.array_equal(info[:, 0], mask.sum(axis=1)) and (info[:, 1] == kw["Q"]).all()
    exp = cleaned["resid"].astype(np.float64)
    print("%s: worst |diff| of a residual %.3g, %.3g of the bound" % (long_id(i), np.abs(resid - exp).max(),
                                                                     np.abs(resid - exp).max() / RESID["atol"]))
    nptest.assert_allclose(resid, exp, **RESID)
    for s in range(kw["S"]):
        nk = int(info[s, 0])
        tail = resid[s, :, nk:]
        assert (tail == 0.0).all() and not np.signbit(tail).any(), "subject %d: not exact zeros behind n_kept = %d" % (s, nk)
        assert (np.abs(resid[s, :, :nk]).max(axis=1) > 0.0).all() and (resid[s, :, nk - 1] != 0.0).all()


def test_chunk_cases_are_there():
    assert len(CHUNK) == 3 and sorted(CR.GPU_LONG_INPUTS[i]["T"] for i in CHUNK) == [513, 700, 700]


@pytest.mark.parametrize("i", CHUNK, ids=long_id)
def test_no_bit_of_the_batch(env, i):
    """No sum of these kernels crosses a subject and none is ordered by S: a subject's residuals are the same bits alone and
    in the batch, and two calls agree."""
    (ts, cf, mask, _cleaned) = case(i)
    (a, ia) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    (b, ib) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(a, b) and np.array_equal(ia, ib)
    for s in range(ts.shape[0]):
        (one, io) = env.corr.clean(ts[s:s + 1], confounds=None if cf is None else cf[s:s + 1], frame_mask=mask[s:s + 1], ctx=env.ctx)
        assert np.array_equal(io[0], ia[s]), s
        assert np.array_equal(one[0], a[s]), "subject %d alone and in the batch differ" % s
    (c, ic) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    (d, id_) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert np.array_equal(c, d) and np.array_equal(ic, id_) and np.isfinite(c).all()


def test_nonfinite_in_dropped_frames_past_frame_256(env):
    """A dropped frame is never read, in any chunk: NaN, 1e300 and -inf there give the bits that finite junk gives."""
    i = [k for k in CHUNK if CR.GPU_LONG_INPUTS[k]["Q"] == 9][0]
    (ts, cf, mask, cleaned) = case(i)
    (S, N, T) = ts.shape
    Q = cf.shape[1]
    assert T == 700
    rs = np.random.RandomState(45)
    (tsa, cfa, tsn, cfn) = (ts.copy(), cf.copy(), ts.copy(), cf.copy())
    bad = np.array([np.nan, 1e300, -np.inf])
    for s in range(S):
        dropped = np.flatnonzero(~mask[s])
        assert dropped.size > 0 and dropped.max() > 256
        tsa[s][:, dropped] = 50.0 * rs.standard_normal((N, dropped.size))
        cfa[s][:, dropped] = 50.0 * rs.standard_normal((Q, dropped.size))
        tsn[s][:, dropped] = bad[(np.arange(N)[:, None] + np.arange(dropped.size)[None, :]) % 3]
        cfn[s][:, dropped] = bad[(np.arange(Q)[:, None] + np.arange(dropped.size)[None, :] + 1) % 3]
    a = env.corr.correlations(tsa, ctx=env.ctx, confounds=cfa, frame_mask=mask)
    b = env.corr.correlations(tsn, ctx=env.ctx, confounds=cfn, frame_mask=mask)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    (ra, ia) = env.corr.clean(tsa, confounds=cfa, frame_mask=mask, ctx=env.ctx)
    (rb, ib) = env.corr.clean(tsn, confounds=cfn, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(ra, rb) and np.array_equal(ia, ib) and np.array_equal(ia, cleaned["info"])
    (exp, _i) = CR.corr_clean_ld(ts, cf, mask, cleaned=cleaned)
    check(b, exp, "NaN, 1e300 and -inf in dropped frames, T 700")


def block_masks(S, T, seed):
    """Subject 0 drops the first frame and a run across position 256 (as far as T reaches), subject 1 the last frame and a
    run across frame 64, the others random frames and runs."""
    m = CR.random_mask(np.random.RandomState(seed), S, T, 0.2)
    m[0] = True
    m[0, 0] = False
    m[0, 254:258] = False
    m[1] = True
    m[1, T - 1] = False
    m[1, 62:67] = False
    return m


@pytest.mark.parametrize("T", [257, 513])
@pytest.mark.parametrize("N", [5, 70])
def test_mask_only(env, N, T):
    S = 3
    (ts, _cf, _m) = CR.make_input(100 + N + T, S, N, T, 0, level=2.0)
    mask = block_masks(S, T, N * T)
    (exp, info_exp) = CR.corr_clean_ld(ts, None, mask)
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, frame_mask=mask, return_info=True)
    check(got, exp, "mask only N %d T %d" % (N, T))
    assert np.array_equal(info, info_exp) and info.shape == (S, 3)
    for s in range(S):      # the correlation of the kept columns, by the reference of the plain path
        check(got[:, s:s + 1], R.corr_edges_ld(ts[s:s + 1][:, :, mask[s]]), "kept columns of subject %d" % s)
    full = env.corr.correlations(ts, ctx=env.ctx, frame_mask=np.ones((S, T), dtype=bool))
    check(full, env.corr.correlations(ts, ctx=env.ctx), "full mask against the plain path")
    check(full, R.corr_edges_ld(ts), "full mask")
