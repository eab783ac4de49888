"""
The cleaning front-end on the device (fcd_corr_clean behind fcdiff_amd.corr.clean and correlations(confounds=,
frame_mask=)) against the long-double oracle of tests/corr_clean_ref.py.

Every comparison of correlations uses corr_ref.BOUND (rtol 1e-11, atol 1e-13), Fisher z the rtol 1e-10 of
tests/test_gpu_corr_edges.py.  The inputs meet two conditions, asserted on the oracle side (corr_clean_ref.gpu_case /
assert_conditions): every row that has a residual keeps at least 1e-6 of its centred variance -- the error grows as the
inverse root of that fraction -- and every confound set that is not deliberately collinear has a unit-scaled Gram
condition number below 1e3.  tests/test_corr_clean.py runs the fp64 restatement of the kernels' pipeline over the same
inputs (corr_clean_ref.GPU_INPUTS) on the CPU and finds it inside the same bound.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import corr_clean_ref as CR
import corr_ref as R

pytestmark = pytest.mark.gpu

FISHER = dict(rtol=1e-10, atol=1e-13)
# residuals against the oracle's: the rows are O(1) to O(10) and each value is a difference of Q + 1 products of that size
RESID = dict(rtol=0, atol=1e-10)


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


def check(got, exp, what, bound=R.BOUND):
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    ok = ~np.isnan(exp)
    (d, excess) = R.worst_excess(got, exp, **bound)
    print("%s: worst |diff| %.3g, %.3g of the bound" % (what, d, excess))
    nptest.assert_allclose(got[ok], exp[ok], err_msg=what, **bound)
    assert got[ok].min() >= -1.0 and got[ok].max() <= 1.0, what


def seam_masks(S, T, seed):
    """Subject 0 drops the first frame and a run across the 16-sample step, subject 1 the last frame and a run across the
    32-sample step, the others random frames and runs."""
    m = CR.random_mask(np.random.RandomState(seed), S, T, 0.2)
    m[0] = True
    m[0, 0] = False
    m[0, 14:19] = False
    if S > 1:
        m[1] = True
        m[1, T - 1] = False
        m[1, 30:35] = False
    return m


# ---------------------------------------------------------------------------------------------------------------------
# mask only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [37, 64, 65])
@pytest.mark.parametrize("N", [5, 16, 17, 33])
def test_mask_only(env, N, T):
    S = 3
    (ts, _cf, _m) = CR.make_input(100 + N + T, S, N, T, 0, level=2.0)
    mask = seam_masks(S, T, N * T)
    (exp, info_exp) = CR.corr_clean_ld(ts, None, mask)
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, frame_mask=mask, return_info=True)
    check(got, exp, "mask only N %d T %d" % (N, T))
    assert np.array_equal(info, info_exp) and info.shape == (S, 3)
    for s in range(S):      # the correlation of the kept columns, by the reference of the plain path
        check(got[:, s:s + 1], R.corr_edges_ld(ts[s:s + 1][:, :, mask[s]]), "kept columns of subject %d" % s)
    full = env.corr.correlations(ts, ctx=env.ctx, frame_mask=np.ones((S, T), dtype=bool))
    check(full, env.corr.correlations(ts, ctx=env.ctx), "full mask against the plain path")
    check(full, R.corr_edges_ld(ts), "full mask")
    # anything that casts to bool is a mask
    again = env.corr.correlations(ts, ctx=env.ctx, frame_mask=mask.astype(np.float64) * 3.0)
    assert np.array_equal(again, got)


# ---------------------------------------------------------------------------------------------------------------------
# confounds: Q at the tile edges of the normal equations, S in {1, 3, 9}, level and scale, the block kernel of K_corr
# ---------------------------------------------------------------------------------------------------------------------
CONFOUND_INPUTS = [kw for kw in CR.GPU_INPUTS if kw["Q"] > 0]


@pytest.mark.parametrize("kw", CONFOUND_INPUTS, ids=CR.input_id)
def test_confounds(env, kw):
    (ts, cf, mask, cleaned) = CR.gpu_case(kw)
    (exp, info_exp) = CR.corr_clean_ld(ts, cf, mask, cleaned=cleaned)
    assert np.isfinite(exp).all()
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert np.array_equal(info, info_exp)
    check(got, exp, CR.input_id(kw))


def test_block_kernel_of_corr_edges_is_reached():
    assert any(kw["Nreg"] > 208 and kw["Q"] > 0 for kw in CONFOUND_INPUTS)      # (208: the last shape of the subject kernel)


def test_fisher_z(env):
    (ts, cf, mask) = CR.make_input(31, 2, 17, 70, 3, drop=0.2)
    (exp, _i) = CR.corr_clean_ld(ts, cf, mask, fisher_z=True)
    got = env.corr.correlations(ts, fisher_z=True, ctx=env.ctx, confounds=cf, frame_mask=mask)
    assert np.isfinite(exp).all()
    nptest.assert_allclose(got, exp, **FISHER)


# ---------------------------------------------------------------------------------------------------------------------
# a dropped frame is never read
# ---------------------------------------------------------------------------------------------------------------------
def test_nonfinite_in_dropped_frames(env):
    (S, N, T, Q) = (3, 17, 70, 5)
    (ts, cf, _m) = CR.make_input(41, S, N, T, Q, level=1.0)
    mask = seam_masks(S, T, 41)
    (ts0, cf0) = (ts.copy(), cf.copy())
    ts0[~mask[:, None, :].repeat(N, axis=1)] = 0.0
    cf0[~mask[:, None, :].repeat(Q, axis=1)] = 0.0
    (tsn, cfn) = (ts0.copy(), cf0.copy())
    bad = np.array([np.nan, np.inf, -np.inf])
    for s in range(S):
        dropped = np.flatnonzero(~mask[s])
        tsn[s][:, dropped] = bad[(np.arange(N)[:, None] + np.arange(dropped.size)[None, :]) % 3]
        cfn[s][:, dropped] = bad[(np.arange(Q)[:, None] + np.arange(dropped.size)[None, :] + 1) % 3]
    a = env.corr.correlations(ts0, ctx=env.ctx, confounds=cf0, frame_mask=mask)
    b = env.corr.correlations(tsn, ctx=env.ctx, confounds=cfn, frame_mask=mask)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    (ra, ia) = env.corr.clean(ts0, confounds=cf0, frame_mask=mask, ctx=env.ctx)
    (rb, ib) = env.corr.clean(tsn, confounds=cfn, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(ra, rb) and np.array_equal(ia, ib)
    (exp, _i) = CR.corr_clean_ld(tsn, cfn, mask)
    check(b, exp, "NaN and inf in dropped frames")


def test_nonfinite_in_kept_frames(env):
    (S, N, T, Q) = (3, 6, 50, 2)
    (ts, cf, mask) = CR.make_input(43, S, N, T, Q, drop=0.2)
    ts[0, 2, np.flatnonzero(mask[0])[3]] = np.nan            # a region: its edges
    ts[0, 4, np.flatnonzero(mask[0])[0]] = np.inf
    cf[1, 1, np.flatnonzero(mask[1])[5]] = np.inf            # a confound: the subject
    (exp, info_exp) = CR.corr_clean_ld(ts, cf, mask)
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    ends = env.O.edge_endpoints(N)
    touched = (ends == 2).any(axis=1) | (ends == 4).any(axis=1)
    assert np.isnan(got[touched, 0]).all() and np.isfinite(got[~touched, 0]).all()
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, 2]).all()
    assert np.array_equal(info, info_exp)
    check(got, exp, "non-finite kept values")


# ---------------------------------------------------------------------------------------------------------------------
# rank
# ---------------------------------------------------------------------------------------------------------------------
def test_rank_deficient_confounds(env):
    (S, N, T, Q) = (2, 17, 70, 5)
    (ts, cf, mask) = CR.make_input(51, S, N, T, Q, drop=0.2, level=3.0)
    CR.assert_conditions(CR.clean_ld(ts, cf, mask))
    (base_exp, _i) = CR.corr_clean_ld(ts, cf, mask)
    base = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask)
    check(base, base_exp, "full rank")
    dup = np.concatenate([cf, -2.5 * cf[:, 1:2]], axis=1)
    zero = np.concatenate([cf[:, :2], np.zeros((S, 1, T)), cf[:, 2:]], axis=1)
    const = np.concatenate([np.full((S, 1, T), 7.25), cf], axis=1)
    const[:, 0][~mask] = -1.0                  # constant over the kept frames only
    allthree = np.concatenate([const, zero[:, 2:3], dup[:, -1:]], axis=1)
    for (name, other) in (("duplicate", dup), ("zero", zero), ("constant", const), ("all three", allthree)):
        (exp, info_exp) = CR.corr_clean_ld(ts, other, mask)
        (got, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=other, frame_mask=mask, return_info=True)
        assert np.array_equal(info, info_exp) and (info[:, 1] == Q).all(), name
        check(got, exp, name)
        check(got, base_exp, name + " against the set without the column")


# ---------------------------------------------------------------------------------------------------------------------
# rows and subjects with no residual
# ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_rows_and_subjects(env):
    (S, N, T, Q) = (7, 6, 40, 3)
    (ts, cf, mask) = CR.make_input(61, S, N, T, Q, drop=0.2)
    ts[0, 1][mask[0]] = 3.0                                        # constant over the kept frames, not over the dropped
    assert ts[0, 1].min() != ts[0, 1].max()
    ts[0, 3] = 2.0 * cf[0, 0] - 0.5 * cf[0, 2] + 4.0               # a combination of confounds (and the intercept)
    for (s, nk) in ((1, Q + 3), (2, Q + 2), (3, 1), (4, 0)):       # dof 2, dof 1, one frame, none
        mask[s] = False
        mask[s, np.arange(T)[5::2][:nk]] = True
    cf[5, 2] = cf[5, 0] * 2.0                                      # rank Q - 1: n_kept = rank + 3 below
    mask[5] = False
    mask[5, 3:3 + Q - 1 + 3] = True
    ts_in, cf_in, mask_in = ts.copy(), cf.copy(), mask.copy()
    (exp, info_exp) = CR.corr_clean_ld(ts, cf, mask)
    (got, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert np.array_equal(ts, ts_in) and np.array_equal(cf, cf_in) and np.array_equal(mask, mask_in)
    assert np.array_equal(info, info_exp)
    assert info[1:6].tolist() == [[Q + 3, Q, 2], [Q + 2, Q, 1], [1, 0, 0], [0, 0, -1], [Q + 2, Q - 1, 2]]
    ends = env.O.edge_endpoints(N)
    touched = (ends == 1).any(axis=1) | (ends == 3).any(axis=1)
    assert np.isnan(got[touched, 0]).all() and np.isfinite(got[~touched, 0]).all()
    assert np.isfinite(got[:, 1]).all() and np.isfinite(got[:, 5]).all() and np.isfinite(got[:, 6]).all()
    assert np.isnan(got[:, 2]).all() and np.isnan(got[:, 3]).all() and np.isnan(got[:, 4]).all()
    # the neighbours in the batch are untouched: subject 6 alone gives the same bits
    alone = env.corr.correlations(ts[6:7], ctx=env.ctx, confounds=cf[6:7], frame_mask=mask[6:7])
    assert np.array_equal(alone[:, 0], got[:, 6])
    # (two degrees of freedom leave a plane: subjects 1 and 5 are only asked to be finite) the others against the oracle
    CR.assert_conditions(CR.clean_ld(ts[[0, 6]], cf[[0, 6]], mask[[0, 6]]))
    check(got[:, [0, 6]], exp[:, [0, 6]], "well-conditioned subjects of the degenerate batch")


# ---------------------------------------------------------------------------------------------------------------------
# clean() on its own
# ---------------------------------------------------------------------------------------------------------------------
def test_clean_residuals(env):
    torch = env.torch
    (S, N, T, Q) = (3, 33, 131, 17)
    (ts, cf, _m) = CR.make_input(71, S, N, T, Q, level=3.0)
    mask = seam_masks(S, T, 71)
    ts[2, 4][mask[2]] = -1.0                   # a row with no residual
    cleaned = CR.clean_ld(ts, cf, mask)
    CR.assert_conditions(cleaned)
    (ts_in, cf_in, mask_in) = (ts.copy(), cf.copy(), mask.copy())
    (resid, info) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(ts, ts_in) and np.array_equal(cf, cf_in) and np.array_equal(mask, mask_in)
    assert resid.shape == (S, N, T) and resid.dtype == np.float64 and info.shape == (S, 3)
    assert np.array_equal(info, cleaned["info"])
    assert np.array_equal(info[:, 0], mask.sum(axis=1)) and (info[:, 1] == Q).all()
    assert np.array_equal(info[:, 2], info[:, 0] - 1 - info[:, 1])
    nptest.assert_allclose(resid, cleaned["resid"].astype(np.float64), **RESID)
    for s in range(S):
        assert (resid[s, :, info[s, 0]:] == 0.0).all() and not np.signbit(resid[s, :, info[s, 0]:]).any()
    assert (resid[2, 4] == 0.0).all() and np.abs(resid[2, 3]).max() > 0.1
    # device tensors in, device tensors out; the inputs are not written
    (dts, dcf, dm) = (torch.as_tensor(ts, device=env.ctx.device), torch.as_tensor(cf, device=env.ctx.device),
                      torch.as_tensor(mask, device=env.ctx.device))
    (dts0, dcf0, dm0) = (dts.clone(), dcf.clone(), dm.clone())
    (dres, dinfo) = env.corr.clean(dts, confounds=dcf, frame_mask=dm, ctx=env.ctx, as_numpy=False)
    assert isinstance(dres, torch.Tensor) and dres.is_cuda and isinstance(dinfo, torch.Tensor) and dinfo.is_cuda
    assert torch.equal(dts, dts0) and torch.equal(dcf, dcf0) and torch.equal(dm, dm0)
    assert np.array_equal(dres.cpu().numpy(), resid) and np.array_equal(dinfo.cpu().numpy(), info)
    (out, oinfo) = env.corr.correlations(dts, ctx=env.ctx, as_numpy=False, confounds=dcf, frame_mask=dm, return_info=True)
    assert out.is_cuda and oinfo.is_cuda
    # no confounds, no mask: centring alone
    (r0, i0) = env.corr.clean(ts, ctx=env.ctx)
    c0 = CR.clean_ld(ts)
    nptest.assert_allclose(r0, c0["resid"].astype(np.float64), **RESID)
    assert np.array_equal(i0, c0["info"]) and i0[0].tolist() == [T, 0, T - 1]


def test_deterministic(env):
    (ts, cf, mask) = CR.make_input(81, 9, 33, 131, 36, drop=0.15, level=2.0)
    (a, ia) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    (b, ib) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert np.array_equal(a, b) and np.array_equal(ia, ib) and np.isfinite(a).all()
    (ra, _i) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    (rb, _i) = env.corr.clean(ts, confounds=cf, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(ra, rb)


# ---------------------------------------------------------------------------------------------------------------------
# refusals through the C ABI, the old path
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(env):
    torch = env.torch
    (S, N, T) = (2, 5, 30)
    dev = env.ctx.device
    ts = torch.ones((S, N, T), dtype=torch.float64, device=dev)
    cf = torch.ones((S, 65, T), dtype=torch.float64, device=dev)
    resid = torch.full((S, N, T), -7.0, dtype=torch.float64, device=dev)
    info = torch.full((S, 3), -7, dtype=torch.int32, device=dev)
    (p, st) = (env.lib.dptr, env.lib.stream_ptr())
    with pytest.raises(NotImplementedError):
        env.ctx.call("fcd_corr_clean", p(ts), p(cf), p(None), S, N, 65, T, p(resid), p(info), st)
    with pytest.raises(NotImplementedError):
        env.ctx.call("fcd_corr_clean", p(ts), p(None), p(None), 65536, N, 0, T, p(resid), p(info), st)
    with pytest.raises(ValueError):
        env.ctx.call("fcd_corr_clean", p(ts), p(None), p(None), S, N, 2, T, p(resid), p(info), st)      # Q > 0 needs confounds
    with pytest.raises(ValueError):
        env.ctx.call("fcd_corr_clean", p(None), p(None), p(None), S, N, 0, T, p(resid), p(info), st)
    with pytest.raises(ValueError):
        env.ctx.call("fcd_corr_clean", p(ts), p(None), p(None), S, N, 0, T, p(None), p(info), st)
    with pytest.raises(ValueError):
        env.ctx.call("fcd_corr_clean", p(ts), p(None), p(None), S, N, 0, T, p(resid), p(None), st)
    with pytest.raises(ValueError):
        env.ctx.call("fcd_corr_clean", p(ts), p(None), p(None), S, 1, 0, T, p(resid), p(info), st)         # Nreg < 2
    torch.cuda.synchronize()
    assert bool((resid == -7.0).all()) and bool((info == -7).all())
    assert env.lib.load().fcd_abi_version() == 4


def test_old_path_is_one_corr_edges_call(env):
    torch = env.torch
    (S, N, T) = (3, 17, 65)
    (ts, _cf, _m) = CR.make_input(91, S, N, T, 0, level=2.0)
    t = torch.as_tensor(ts, device=env.ctx.device)
    for fz in (False, True):
        out = torch.empty((N * (N - 1) // 2, S), dtype=torch.float64, device=env.ctx.device)
        env.ctx.call("fcd_corr_edges", env.lib.dptr(t), S, N, T, 1 if fz else 0, env.lib.dptr(out), env.lib.stream_ptr())
        got = env.corr.correlations(ts, fisher_z=fz, ctx=env.ctx)
        assert np.array_equal(got, out.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# end to end: cleaned correlations into a fit with missing data
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_into_a_fit(env):
    (N, H, U, T, Q) = (5, 3, 3, 40, 2)
    (ts, cf, mask) = CR.make_input(95, H + U, N, T, Q, drop=0.2)
    mask[H + 1] = False
    mask[H + 1, :Q + 2] = True                 # one patient with dof 1
    (out, info) = env.corr.correlations(ts, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
    assert info[H + 1].tolist() == [Q + 2, Q, 1]
    (b, bt) = (out[:, :H].copy(), out[:, H:].copy())
    Cn = N * (N - 1) // 2
    assert np.isnan(bt[:, 1]).all() and np.isnan(out).sum() == Cn
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt, fit.missing_data) = (env.pkg.UnsharedRegionModel(), b, bt, True)
    (fit.max_iters, fit.rel_tol) = (2, -np.inf)
    fit.run()
    assert len(fit.energy) == 3 and all(np.isfinite(fit.energy))
    assert fit.missing_counts() == (0, Cn)
