"""
Covariate adjustment on the device (fcd_edge_cov_fit, fcd_edge_cov_apply, fcdiff_amd.covariates) against
tests/covariates_ref.py.

Tolerances (covariates_ref.BETA, RESID_VAR): under the conditions covariates_ref.assert_conditions checks on the oracle's
side -- design condition below 1e2, no drop decision near the threshold, the residual keeps 1e-6 of the row -- the normal
equations lose at most about Q cond^2 2^-53 = 2e-11 of a fitted part whose norm is at most the row's centred norm, about 0.7
here.  So beta in scaled units (times the norm of the centred column) and adjusted values are compared with atol 1e-10,
rtol 0; resid_var with rtol 1e-9; info exactly.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import covariates_ref as CV
import noise_ref as NR
from conftest import theta_dict
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu

FIT = dict(rtol=1e-10, atol=1e-12)         # the FIT tolerance of tests/test_gpu_noise.py
CS = (3, 10, 2016)                         # 3, 5 and 64 regions: the last crosses workgroups


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, covariates

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.cov = torch, fcdiff_amd, _lib, covariates
    e.ctx = _lib.Context()
    return e


def up(env, a, dtype=None):
    return None if a is None else env.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def dev_fit(env, b, z, flags=0, tensors=None):
    """fcd_edge_cov_fit on host arrays -> (beta, resid_var, info) as NumPy; tensors: a list that receives the input tensors."""
    t = env.torch
    (C, H) = b.shape
    Q = z.shape[1]
    (bd, zd) = (up(env, b, np.float64), up(env, z, np.float64) if Q else None)
    beta = t.full((C, Q), 7.0, dtype=t.float64, device="cuda")
    rv = t.full((C,), 7.0, dtype=t.float64, device="cuda")
    info = t.full((C, 4), -7, dtype=t.int32, device="cuda")
    p = env.lib.dptr
    env.ctx.call("fcd_edge_cov_fit", p(bd), C, H, p(zd), Q, flags, p(beta) if Q else p(None), p(rv), p(info), env.lib.stream_ptr())
    if tensors is not None:
        tensors.extend([bd, zd])
    return beta.cpu().numpy(), rv.cpu().numpy(), info.cpu().numpy()


def dev_apply(env, x, z, z_ref, beta):
    t = env.torch
    (C, S) = x.shape
    Q = z.shape[1]
    xd = up(env, x, np.float64)
    out = t.full((C, S), 7.0, dtype=t.float64, device="cuda")
    p = env.lib.dptr
    (zd, rd, bd) = [up(env, a, np.float64) if Q else None for a in (z, z_ref, beta)]      # (held until the result is read)
    env.ctx.call("fcd_edge_cov_apply", p(xd), C, S, p(zd), Q, p(rd), p(bd), p(out), env.lib.stream_ptr())
    return out.cpu().numpy()


def compare(env, got, ref, b, z, rows=None, tol_rows=None):
    """The device's (beta, resid_var, info) of the rows `rows` of the reference (default: the first len(beta)); tol_rows: the
    fitted rows whose conditions were asserted (default: all fitted ones)."""
    (beta, rv, info) = got
    C = beta.shape[0]
    rows = np.arange(C) if rows is None else np.asarray(rows)
    assert np.array_equal(info, ref["info"][rows]), "info"
    fitted = ref["fitted"][rows]
    assert np.all(beta[~fitted] == 0.0) and np.isnan(rv[~fitted]).all()
    norm = ref["norm"][rows]
    assert np.all(beta[norm == 0.0] == 0.0), "a column not used has a slope"
    tol = fitted if tol_rows is None else np.isin(rows, tol_rows) & fitted
    d = np.abs(beta * norm - ref["beta"][rows] * norm)[tol]
    rel = np.abs(rv[tol] / ref["resid_var"][rows][tol] - 1.0)
    print("C=%d: %d rows to tolerance, max |d beta| (scaled) %.3g, max rel d resid_var %.3g"
          % (C, int(tol.sum()), d.max() if d.size else 0.0, rel.max() if rel.size else 0.0))
    nptest.assert_allclose((beta * norm)[tol], (ref["beta"][rows] * norm)[tol], **CV.BETA)
    nptest.assert_allclose(rv[tol], ref["resid_var"][rows][tol], **CV.RESID_VAR)
    if z.shape[1] and tol.any():
        z_ref = CV.default_z_ref(z)
        x = b[rows][tol]
        nptest.assert_allclose(dev_apply(env, x, z, z_ref, beta[tol]), CV.apply_ld(x, z, z_ref, ref["beta"][rows][tol]), **CV.BETA)


# ------------------------------------------------------------------------------------------------
# 1. the fit against the reference
# ------------------------------------------------------------------------------------------------
def fit_cases():
    out = []
    for Q in (0, 1, 3, 16):
        for H in (Q + 2, 17, 64, 65, 130):
            for nan in (0.0, 0.06):
                out.append((H, Q, nan))
    return out


@pytest.mark.parametrize("H,Q,nan", fit_cases())
def test_fit_against_the_reference(env, H, Q, nan):
    """One set of 2016 rows per case and one run of the reference; the device at C = 3, 10 and 2016 on its first rows.
    (H = 17 with Q = 16 has dof 0: every row is left unadjusted, exactly.)"""
    rng = np.random.default_rng(1000 * H + 10 * Q + (1 if nan else 0))
    z = CV.make_design(rng, H, Q)
    b = CV.make_rows(rng, CS[-1], CV.make_design(rng, H, min(Q, H - 2)) if H - 1 - Q < 1 else z, nan)
    ref = CV.fit_ld(b, z, missing=nan > 0)
    CV.assert_conditions(ref)
    assert ref["fitted"].any() == (H - 1 - Q >= 1)
    for C in CS:
        compare(env, dev_fit(env, b[:C], z, env.lib.FCD_DATA_NAN_MISSING if nan else 0), ref, b, z)


@pytest.mark.parametrize("nan", [0.0, 0.02])
def test_fit_walks_a_long_design_in_pieces(env, nan):
    (H, Q, C) = (1500, 16, 3)
    rng = np.random.default_rng(77)
    z = CV.make_design(rng, H, Q)
    b = CV.make_rows(rng, C, z, nan)
    ref = CV.fit_ld(b, z, missing=nan > 0)
    assert len(CV.assert_conditions(ref)) == C
    compare(env, dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING if nan else 0), ref, b, z)


# ------------------------------------------------------------------------------------------------
# 2. degenerate rows beside well-conditioned ones
# ------------------------------------------------------------------------------------------------
def degenerate_design(rng, H):
    """Columns: 0, 1 continuous; 2 = column 0 again; 3, 4, 5 a full set of dummies (5, 8 and H - 13 controls); 6 varies on
    controls 0-2 only."""
    z = np.zeros((H, 7))
    z[:, :2] = CV.make_design(rng, H, 2)
    z[:, 2] = z[:, 0]
    site = np.repeat([0, 1, 2], [5, 8, H - 13])
    rng.shuffle(site[3:])
    for k in range(3):
        z[:, 3 + k] = site == k
    z[:, 6] = 2.0
    z[:3, 6] = [1.0, 2.5, 4.0]
    return z


def test_degenerate_rows_beside_well_conditioned_ones(env):
    H = 24
    rng = np.random.default_rng(11)
    z = degenerate_design(rng, H)
    b = CV.make_rows(rng, 14, z)
    good = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13]      # complete rows, and rows 11-13 with scattered NaN
    b[11, [4, 9]] = np.nan
    b[12, 20] = np.nan
    b[13, [5, 6, 7, 15]] = np.nan
    b[4, :] = np.nan                                 # all controls missing
    b[5, :3] = np.nan                                # column 6 is constant over the controls left
    b[6, 1:] = np.nan                                # one control
    # n_obs = rank + 1: the longest run of leading controls that leaves dof 0
    k0 = max(k for k in range(2, H) if CV.design_of(z, np.arange(H) < k)["rank"] == k - 1)
    b[7, k0:] = np.nan
    ref = CV.fit_ld(b, z, missing=True)
    CV.assert_conditions(ref, good + [5])
    assert np.all(ref["gap"][good + [5]] > 1e-6)      # which columns are used is not a rounding matter
    info = ref["info"]
    assert info[4].tolist() == [0, 0, -1, 0] and info[6].tolist() == [1, 0, 0, 0]
    assert k0 > 2 and info[7].tolist() == [k0, 0, 0, 0]
    # complete rows: column 0 used and its copy not, two of the three dummies, column 6
    assert info[0, 1] == 5 and info[0, 3] & 0b0000101 == 0b0000001 and bin(info[0, 3] & 0b0111000).count("1") == 2
    assert info[0, 3] & 0b1000000
    assert info[5, 1] == 4 and not info[5, 3] & 0b1000000 and info[5, 3] & 0b0000101 == 0b0000001
    compare(env, dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING), ref, b, z, tol_rows=good + [5])
    # the same rows without the flag: rows with a NaN become NaN, the others are fitted on all controls
    plain = CV.fit_ld(b, z)
    (beta, rv, info_d) = dev_fit(env, b, z, 0)
    assert np.array_equal(info_d, plain["info"]) and info_d[4].tolist() == [H, 5, H - 6, info[0, 3]]
    holes = np.isnan(b).any(axis=1)
    assert np.isnan(beta[holes]).all() and np.isnan(rv[holes]).all() and np.isfinite(beta[~holes]).all()
    nptest.assert_allclose((beta * plain["norm"])[~holes], (plain["beta"] * plain["norm"])[~holes], **CV.BETA)
    nptest.assert_allclose(rv[~holes], plain["resid_var"][~holes], **CV.RESID_VAR)


@pytest.mark.parametrize("Q", [0, 2])
def test_one_control(env, Q):
    rng = np.random.default_rng(3)
    b = rng.standard_normal((5, 1))
    b[2, 0] = np.nan
    z = rng.standard_normal((1, Q))
    (beta, rv, info) = dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING)
    assert np.all(beta == 0.0) and np.isnan(rv).all()
    assert info.tolist() == [[1, 0, 0, 0]] * 2 + [[0, 0, -1, 0]] + [[1, 0, 0, 0]] * 2


# ------------------------------------------------------------------------------------------------
# 3. the two paths, determinism, inputs
# ------------------------------------------------------------------------------------------------
def test_complete_and_missing_path_agree(env):
    """A row without NaN is a complete row with or without the flag: bit for bit.  One more control that is NaN in every row
    sends every row down the path of rows with missing controls, which fits the same H controls: to the tolerance."""
    (H, Q, C) = (65, 16, 130)
    rng = np.random.default_rng(21)
    z = CV.make_design(rng, H, Q)
    b = CV.make_rows(rng, C, z)
    ref = CV.fit_ld(b, z)
    CV.assert_conditions(ref)
    plain = dev_fit(env, b, z, 0)
    flagged = dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING)
    for (a, c) in zip(plain, flagged):
        assert np.array_equal(a, c)
    b1 = np.concatenate([b[:, :30], np.full((C, 1), np.nan), b[:, 30:]], axis=1)
    z1 = np.concatenate([z[:30], 5.0 * np.ones((1, Q)), z[30:]], axis=0)
    own = dev_fit(env, b1, z1, env.lib.FCD_DATA_NAN_MISSING)
    assert np.array_equal(own[2], plain[2])
    d = np.abs((own[0] - plain[0]) * ref["norm"]).max()
    print("paths: max |d beta| (scaled) %.3g, max rel d resid_var %.3g" % (d, np.abs(own[1] / plain[1] - 1).max()))
    nptest.assert_allclose(own[0] * ref["norm"], plain[0] * ref["norm"], **CV.BETA)
    nptest.assert_allclose(own[1], plain[1], **CV.RESID_VAR)
    compare(env, own, ref, b, z)


def test_deterministic_and_inputs_unchanged(env):
    (H, Q, C) = (130, 16, 2016)
    rng = np.random.default_rng(31)
    z = CV.make_design(rng, H, Q)
    b = CV.make_rows(rng, C, z, 0.05)
    b[:40] = CV.make_rows(rng, 40, z)                # complete rows among them: both paths
    held = []
    first = dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING, tensors=held)
    second = dev_fit(env, b, z, env.lib.FCD_DATA_NAN_MISSING)
    for (a, c) in zip(first, second):
        assert a.tobytes() == c.tobytes()
    assert held[0].cpu().numpy().tobytes() == b.tobytes() and held[1].cpu().numpy().tobytes() == z.tobytes()


# ------------------------------------------------------------------------------------------------
# 4. apply
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 258])
@pytest.mark.parametrize("Q", [0, 3, 16])
def test_apply_is_the_numpy_loop_bit_for_bit(env, S, Q):
    """S odd: 8 bytes per lane; S even: 16; 257 / 258: two blocks of columns.  37 rows: two blocks of rows."""
    C = 37
    rng = np.random.default_rng(100 * S + Q)
    x = rng.standard_normal((C, S))
    x[rng.random((C, S)) < 0.1] = np.nan
    z = rng.standard_normal((S, Q)) * 3.0 + 1.0
    z_ref = rng.standard_normal(Q)
    beta = rng.standard_normal((C, Q)) * 0.1
    beta[3] = 0.0
    out = dev_apply(env, x, z, z_ref, beta)
    want = CV.apply_loop(x, z, z_ref, beta)
    assert np.array_equal(np.isnan(out), np.isnan(x))
    assert out.tobytes() == want.tobytes()
    assert out[3].tobytes() == x[3].tobytes()


def test_apply_takes_sessions(env):
    (C, U, K, Q) = (10, 3, 2, 3)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((C, U, K))
    x[2, 1, 0] = np.nan
    (z_u, z_uk) = (rng.standard_normal((U, Q)), rng.standard_normal((U, K, Q)))
    z_b = rng.standard_normal((6, Q))
    adj = env.cov.EdgeAdjustment(rng.standard_normal((C, Q)), np.ones(C), np.zeros((C, 4), dtype=np.int32), z_b.mean(axis=0), z_b,
                                 env.ctx)
    got = adj.apply(x, z_u)
    assert got.shape == (C, U, K)
    assert got.tobytes() == CV.apply_loop(x.reshape(C, U * K), np.repeat(z_u, K, axis=0), adj.z_ref, adj.beta).tobytes()
    got = adj.apply(x, z_uk, as_numpy=False)
    assert tuple(got.shape) == (C, U, K) and got.is_cuda
    assert got.cpu().numpy().tobytes() == CV.apply_loop(x.reshape(C, U * K), z_uk.reshape(U * K, Q), adj.z_ref, adj.beta).tobytes()
    flat = adj.apply(x[:, :, 0], z_u)
    assert flat.tobytes() == CV.apply_loop(x[:, :, 0], z_u, adj.z_ref, adj.beta).tobytes()


# ------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------
def test_entry_point_refusals(env):
    t = env.torch
    p = env.lib.dptr
    buf = t.zeros(4096, dtype=t.float64, device="cuda")
    (o1, o2) = (t.zeros(4096, dtype=t.float64, device="cuda"), t.zeros(4096, dtype=t.float64, device="cuda"))
    info = t.zeros(64, dtype=t.int32, device="cuda")
    s = env.lib.stream_ptr()

    def fit(C, H, Q, flags):
        env.ctx.call("fcd_edge_cov_fit", p(buf), C, H, p(buf), Q, flags, p(o1), p(o2), p(info), s)

    def apply(C, S, Q):
        env.ctx.call("fcd_edge_cov_apply", p(buf), C, S, p(buf), Q, p(buf), p(buf), p(o1), s)
    with pytest.raises(NotImplementedError, match="at most 16"):
        fit(3, 8, 17, 0)
    with pytest.raises(NotImplementedError, match="unknown flags"):
        fit(3, 8, 2, env.lib.FCD_W_PER_EDGE)
    with pytest.raises(ValueError):
        fit(0, 8, 2, 0)
    with pytest.raises(ValueError):
        fit(3, 0, 2, 0)
    with pytest.raises(ValueError):
        fit(3, 8, -1, 0)
    with pytest.raises(NotImplementedError, match="at most 16"):
        apply(3, 8, 17)
    with pytest.raises(ValueError):
        apply(0, 8, 2)
    with pytest.raises(ValueError):
        apply(3, 0, 2)
    fit(3, 8, 2, 0)                                  # the context is still usable
    t.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="at most 16"):
        env.cov.fit_adjustment(np.zeros((3, 20)), np.zeros((20, 17)), ctx=env.ctx)


# ------------------------------------------------------------------------------------------------
# 6. the module, the scenario, reuse for new patients
# ------------------------------------------------------------------------------------------------
def new_fit(env, model, b, bt, **kw):
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (model, b, bt)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


def scenario_model(env):
    m = env.pkg.UnsharedRegionModel()
    m.pi = CV.SCENARIO["pi"]
    return m


def test_module_against_the_reference(env):
    (H, U, Q, C) = (40, 7, 3, 45)
    rng = np.random.default_rng(41)
    (z_b, z_bt) = (CV.make_design(rng, H, Q), CV.make_design(rng, U, Q))
    b = CV.make_rows(rng, C, z_b, 0.05)
    bt = rng.standard_normal((C, U)) * 0.2
    bt[1, 2] = np.nan
    (b_ref, bt_ref, ref) = CV.adjust_ld(b, bt, z_b, z_bt, missing=True)
    CV.assert_conditions(ref)
    (b_adj, bt_adj, adj) = env.cov.adjust(b, bt, z_b, z_bt, missing_data=True, ctx=env.ctx)
    assert adj.n_columns == Q and np.array_equal(adj.info, ref["info"]) and adj.z_ref.tobytes() == z_b.mean(axis=0).tobytes()
    nptest.assert_allclose(adj.beta * ref["norm"], ref["beta"] * ref["norm"], **CV.BETA)
    nptest.assert_allclose(adj.resid_var, ref["resid_var"], **CV.RESID_VAR)
    nptest.assert_allclose(b_adj, b_ref, **CV.BETA)
    nptest.assert_allclose(bt_adj, bt_ref, **CV.BETA)
    # another reference point moves every adjusted value of a connection by the same amount
    other = env.cov.fit_adjustment(b, z_b, missing_data=True, z_ref=np.zeros(Q), ctx=env.ctx)
    assert other.beta.tobytes() == adj.beta.tobytes()
    shift = other.apply(bt, z_bt) - bt_adj
    nptest.assert_allclose(shift[:, [0]] + 0 * shift, shift, rtol=0, atol=1e-13)
    lev = adj.leverage(z_bt)
    assert lev.shape == (U,) and np.all(lev > 0)


def test_scenario_through_the_fit(env):
    """
    test_covariates.py's scenario through UnsharedRegionFit (vb, 8 iterations, symmetric edge ids), on the data as they are
    and on the data the device adjusted: lq_R is the reference loop's on the same arrays (for the adjusted data: on the
    REFERENCE's adjusted arrays), and the same three inequalities hold (reference: 0.147, 0.0043, 0.92).
    """
    s = CV.SCENARIO
    (_b0, _bt0, b, bt, z_b, z_bt, r) = CV.scenario_data(scenario_model(env))
    start = theta_dict(scenario_model(env).theta())
    (b_ref, bt_ref, ref) = CV.adjust_ld(b, bt, z_b, z_bt)
    CV.assert_conditions(ref)
    (b_adj, bt_adj, adj) = env.cov.adjust(b, bt, z_b, z_bt, ctx=env.ctx)
    assert np.all(adj.info == [s["H"], 2, s["H"] - 3, 3])
    nptest.assert_allclose(b_adj, b_ref, **CV.BETA)
    nptest.assert_allclose(bt_adj, bt_ref, **CV.BETA)
    rates = []
    for (name, x, xt, want_on) in (("not adjusted", b, bt, (b, bt)), ("adjusted", b_adj, bt_adj, (b_ref, bt_ref))):
        fit = new_fit(env, scenario_model(env), x, xt, max_iters=s["iters"], rel_tol=-np.inf, edge_index="symmetric")
        fit.run()
        want = NR.vb_fit(want_on[0], want_on[1], start, s["iters"], O.EDGE_SYMMETRIC)
        rates.append(CV.scenario_rates(fit._lq_R, r))
        print("%s: flagged %.4f / %.3f found %.2f; max |d lq_R| %.3g" % ((name,) + rates[-1] + (np.abs(fit._lq_R - want["lq_R"]).max(),)))
        nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
    assert rates[0][0] >= 0.10
    assert rates[1][0] <= 0.02
    assert rates[1][2] >= 0.80


def test_new_patients_are_adjusted_with_the_fit_s_slopes(env):
    """adj.apply(bt_new, z_new), then fit.score(): a new patient at z_ref is unchanged bit for bit and scored as unadjusted."""
    (N, H, U, Q) = (6, 12, 4, 2)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=8)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(N, H, 3, seed=9)
    (b, bt, bt_new) = (np.array(b, dtype=np.float64), np.array(bt, dtype=np.float64), np.array(bt_new, dtype=np.float64))
    rng = np.random.default_rng(9)
    (z_b, z_bt) = (rng.standard_normal((H, Q)), rng.standard_normal((U, Q)))
    b = b + 0.05 * z_b[:, 0][None, :]
    (b_adj, bt_adj, adj) = env.cov.adjust(b, bt, z_b, z_bt, ctx=env.ctx)
    fit = new_fit(env, env.pkg.UnsharedRegionModel(), b_adj, bt_adj, max_iters=3)
    fit.run()
    z_new = rng.standard_normal((3, Q)) + 1.0
    z_new[0] = adj.z_ref
    new_adj = adj.apply(bt_new, z_new)
    assert new_adj[:, 0].tobytes() == bt_new[:, 0].tobytes()
    assert not np.allclose(new_adj[:, 1:], bt_new[:, 1:], rtol=0, atol=1e-4)
    got = fit.score(new_adj, max_iters=6, tol=0.0)
    raw = fit.score(bt_new, max_iters=6, tol=0.0)
    assert got["p_R"].shape == (N, 3) and np.all(np.isfinite(got["p_R"]))
    assert got["p_R"][:, 0].tobytes() == raw["p_R"][:, 0].tobytes()
    assert not np.array_equal(got["p_R"][:, 1:], raw["p_R"][:, 1:])
