"""
NaN as unobserved data on the MI355X (UnsharedRegionFit.missing_data = True): the table kernel against the NumPy oracle
masked test-side, the fits against the same fits with the data removed, the sampler against the C oracle and against
the exact law of the reduced problem, the theta objectives, the connection posterior and the front end end to end.
Never hands the sampler a NaN table: every table here is built with the flag on, or has no NaN.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
import missing_data_ref as MD
from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain, binom_two_sided, histogram

pytestmark = pytest.mark.gpu

TAB = dict(rtol=1e-12, atol=1e-14)      # the tolerances of the existing table tests (test_gpu_parity.py)
FIT = dict(rtol=1e-10, atol=1e-12)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO = torch, fcdiff_amd, _lib, GibbsEngine, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def new_fit(env, model, b, bt, missing=True, **kw):
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.missing_data = model, b, bt, missing
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


def device_tables(env, model, b, bt):
    """(fit, S_B, lM) of the table kernel with the flag on (host copies)."""
    (C, H), U = b.shape, bt.shape[1]
    fit = new_fit(env, model, b, bt)
    fit._init_lps(int(env.pkg.util.C_to_N(C)), H, U)
    fit._update_lps()
    return fit, fit._d["S_B"].cpu().numpy(), fit._lM


def holes(rng, b, bt, frac=0.1):
    """~frac NaN at random, one whole edge row, one whole healthy column, one whole patient column."""
    (b, bt) = (b.copy(), bt.copy())
    b[rng.random(b.shape) < frac] = np.nan
    bt[rng.random(bt.shape) < frac] = np.nan
    c = b.shape[0] // 2
    b[c, :] = np.nan
    bt[c, :] = np.nan
    b[:, b.shape[1] // 3] = np.nan
    bt[:, bt.shape[1] - 1] = np.nan
    return b, bt


def binom_ok(k, n, p):
    return binom_two_sided(k, n, p) >= X.P_CELL


# ------------------------------------------------------------------------------------------------
# 1. tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,U", [(23, 16, 37), (40, 3, 129), (9, 17, 2)])
def test_tables_against_masked_oracle(env, N, H, U):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b0, bt0) = m.sample_fast(N, H, U, seed=N + H + U)
    (b, bt) = holes(np.random.default_rng(N), b0, bt0)
    (fit, S_B, lM) = device_tables(env, m, b, bt)
    (S_exp, lpB_exp, pBt_exp, lM_exp) = MD.masked_lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    nptest.assert_allclose(S_B, S_exp, rtol=1e-12)
    miss = np.isnan(bt)
    nptest.assert_allclose(lM[~miss], lM_exp[~miss], **TAB)
    assert np.all(lM[miss] == 0.0) and not np.signbit(lM[miss]).any()
    assert fit.missing_counts() == (int(np.isnan(b).sum()), int(np.isnan(bt).sum()))
    # the full tables behind the properties: 0.0 / 1.0 at missing entries
    (lpB, pBt) = (fit._lp_B_g_F, fit._p_Bt_g_Ft)
    assert np.all(lpB[np.isnan(b)] == 0.0) and np.all(pBt[miss] == 1.0)
    nptest.assert_allclose(lpB, lpB_exp, **TAB)
    nptest.assert_allclose(pBt, pBt_exp, rtol=1e-12, atol=1e-300)
    # the flag on NaN-free data: bit for bit the flag-off tables
    (fit1, S1, lM1) = device_tables(env, m, b0, bt0)
    fit0 = new_fit(env, m, b0, bt0, missing=False)
    fit0._init_lps(N, H, U)
    fit0._update_lps()
    assert np.array_equal(S1, fit0._d["S_B"].cpu().numpy()) and np.array_equal(lM1, fit0._lM)
    assert np.array_equal(fit1._lp_B_g_F, fit0._lp_B_g_F) and np.array_equal(fit1._p_Bt_g_Ft, fit0._p_Bt_g_Ft)
    assert fit1.missing_counts() == (0, 0)
    with pytest.raises(ValueError):
        fit0.missing_counts()


def test_default_path_keeps_nan_in_the_tables(env):
    """Flag off: NaN is read as a number, exactly as before (asserted on the tables only)."""
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(7, 4, 5, seed=2)
    (b[3, 1], bt[5, 2]) = (np.nan, np.nan)
    fit = new_fit(env, m, b, bt, missing=False)
    fit._init_lps(7, 4, 5)
    fit._update_lps()
    assert np.all(np.isnan(fit._d["S_B"].cpu().numpy()[3])) and np.all(np.isnan(fit._lM[5, 2]))
    assert np.isfinite(fit._lM).sum() == fit._lM.size - 9


# ------------------------------------------------------------------------------------------------
# 2. a missing healthy column equals dropping it (variational fit)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,U,h", [(12, 6, 9, 2), (30, 9, 14, 8)])
def test_vb_missing_column_equals_dropping_it(env, N, H, U, h):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(N, H, U, seed=N * H)
    bn = b.copy()
    bn[:, h] = np.nan
    fits = []
    for (bb, miss) in ((bn, True), (np.delete(b, h, axis=1), False)):
        fit = new_fit(env, env.pkg.UnsharedRegionModel(), bb, bt, missing=miss, max_iters=6, rel_tol=-np.inf)
        fit.run()
        fits.append(fit)
    (a, d) = fits
    assert len(a.energy) == len(d.energy) == 7
    nptest.assert_allclose(a.energy, d.energy, **FIT)
    nptest.assert_allclose(a._lq_F, d._lq_F, **FIT)
    nptest.assert_allclose(a._lq_R, d._lq_R, **FIT)
    nptest.assert_allclose(a.model.pi, d.model.pi, **FIT)
    nptest.assert_allclose(a.model.gamma, d.model.gamma, **FIT)
    assert a.missing_counts() == (C_of(N), 0)


def C_of(N):
    return N * (N - 1) // 2


# ------------------------------------------------------------------------------------------------
# 3. the sampler on masked tables equals the C oracle, chain for chain
# ------------------------------------------------------------------------------------------------
GIBBS_FORMS = [((64, 16, 16, 256), {}), ((40, 5, 128), {"r_path": 3}), ((40, 5, 128), {"r_dsplit": 1}),
               ((40, 5, 128), {"f_form": 2}), ((40, 5, 128), {"f_form": 3}), ((40, 5, 128), {})]


@pytest.mark.parametrize("shape,kn", GIBBS_FORMS, ids=["cfg2-default", "step-per-launch", "one-in-order-workgroup",
                                                       "any-U-f-kernel", "scalar-mask-f-kernel", "default"])
def test_gibbs_on_masked_tables_equals_oracle(env, shape, kn):
    if len(shape) == 4:
        (N, H, U, G) = shape
    else:
        (N, U, G) = shape
        H = 3
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=7 + N)
    (b, bt) = holes(np.random.default_rng(N + U), b, bt)
    (_fit, S_B, lM) = device_tables(env, m, b, bt)
    assert np.all(np.isfinite(S_B)) and np.all(np.isfinite(lM))
    for (k, v) in kn.items():
        env.ctx.set_knob(k, v)
    try:
        seed = 4242 + N
        eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.2)
        (f_o, r_o) = env.CO.gibbs_init(G, N, U, 0.2, seed, 0)
        (lng, lnpi2) = (np.log(m.gamma), np.log(m.pi2()))
        for s in range(2):
            eng.run(s, 1, mstep_every=0)
            env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
            env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES["symmetric"], 0)
        (f_g, r_g) = eng.export_state()
        r_form = env.ctx.stat("r_form_last")
        assert env.ctx.stat("dev_err") == 0
    finally:
        for k in kn:
            env.ctx.set_knob(k, 0)
    assert r_form == (1 if kn.get("r_path") == 3 else 2)
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


# ------------------------------------------------------------------------------------------------
# 4. exact law of the reduced problem, with one patient column all NaN
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x2", "4x2"])
def test_chains_follow_exact_law_of_reduced_problem(env, record_property, name):
    """
    Patient 1's bt is NaN at every edge.  The chains of (f, r of patient 0) must follow the exact law P_k of the problem
    without patient 1, whose tables come from the pinned NumPy oracle (no NaN, no masking code); patient 1's r sites are
    Bernoulli(pi) after every sweep (exact binomial tails).  Same cases, seeds and thresholds as test_gpu_exact_law.py.
    """
    (N, U, data) = X.CASES[name]
    assert U == 2
    m = X.model(data)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)
    bt_n = bt.copy()
    bt_n[:, 1] = np.nan
    (_fit, S_B, lM) = device_tables(env, m, b, bt_n)
    (lpB_r, _pBt_r, lM_r) = O.lik_tables(b, bt[:, :1], m.mu, m.sigma, m.eta, m.epsilon)
    (gamma, pi2) = (np.asarray(m.gamma, dtype=np.float64), m.pi2())
    ec = ExactChain(O.sum_lp_B(lpB_r), lM_r, gamma, pi2)
    G = X.G_CHAINS
    seed = 1234 + 10 * N + U
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    hists = {}
    for s in range(max(X.SWEEPS)):
        eng.run(s, 1, mstep_every=0)
        if s + 1 in X.SWEEPS:
            (f, r) = eng.export_state()
            hists[s + 1] = histogram(ec, f, np.ascontiguousarray(r[:, :, :1]))
            for n in range(N):
                k = int(r[:, n, 1].sum())
                assert binom_ok(k, G, pi2[1]), (s + 1, n, k, G * pi2[1])
    r_form = env.ctx.stat("r_form_last")
    record_property("r_form_last", r_form)
    assert r_form == 2 and env.ctx.stat("dev_err") == 0
    bad = X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# 5. dead region, dead edge
# ------------------------------------------------------------------------------------------------
def dead_data(env, N, H, U, n_dead, u_dead, c_dead, seed):
    m = env.pkg.UnsharedRegionModel()
    m.sigma = np.array([0.1, 0.1, 0.1])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    (en, em) = np.tril_indices(N, -1)
    bt[(en == n_dead) | (em == n_dead), u_dead] = np.nan
    b[c_dead, :] = np.nan
    bt[c_dead, :] = np.nan
    return m, b, bt


def test_vb_dead_region_and_dead_edge(env):
    (N, H, U, n, u, c) = (14, 5, 7, 6, 3, 40)
    (m, b, bt) = dead_data(env, N, H, U, n, u, c, seed=5)
    fit = new_fit(env, m, b, bt, edge_index="symmetric")
    fit._init_lps(N, H, U)
    fit._update_lps()
    rng = np.random.default_rng(1)
    lq_R = np.log(rng.dirichlet(np.ones(2), (N, U)))
    fit._lq_R = lq_R
    fit._update_lq_F()
    qF = np.exp(fit._lq_F)
    g = np.asarray(m.gamma, dtype=np.float64)
    nptest.assert_allclose(qF[c, 0], g / g.sum(), rtol=1e-13, atol=1e-15)
    fit._update_lq_R()
    qR = np.exp(fit._lq_R)
    nptest.assert_allclose(qR[n, u, 1], fit._pi2()[1], rtol=1e-13)
    # every other site saw data
    assert not np.allclose(np.delete(qR[:, u, 1], n), fit._pi2()[1], rtol=1e-6)


def test_gibbs_dead_region_and_dead_edge(env):
    (N, H, U, n, u, c, G) = (14, 5, 7, 6, 3, 40, 1 << 16)
    (m, b, bt) = dead_data(env, N, H, U, n, u, c, seed=5)
    (_fit, S_B, lM) = device_tables(env, m, b, bt)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=99, edge_index="symmetric", ctx=env.ctx)
    (gamma, pi2) = (np.asarray(m.gamma, dtype=np.float64), m.pi2())
    eng.set_hyper(gamma, pi2)
    eng.init(0.5)
    p_f = gamma / gamma.sum()
    for s in range(3):
        eng.run(s, 1, mstep_every=0)
        (f, r) = eng.export_state()
        assert binom_ok(int(r[:, n, u].sum()), G, pi2[1]), s
        cnt = np.bincount(f[:, c], minlength=3)
        for k in range(3):
            assert binom_ok(int(cnt[k]), G, p_f[k]), (s, k, cnt)
    assert env.ctx.stat("dev_err") == 0


# ------------------------------------------------------------------------------------------------
# 6. theta objectives
# ------------------------------------------------------------------------------------------------
def objective_data(env, seed=11):
    (N, H, U) = (11, 5, 8)
    m = env.pkg.UnsharedRegionModel()
    m.eta, m.epsilon = 0.29, 0.07
    m.mu, m.sigma = np.array([-0.2, 0.0, 0.25]), np.array([0.12, 0.1, 0.15])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    rng = np.random.default_rng(seed)
    (b, bt) = holes(rng, b, bt)
    W = rng.uniform(0.0, 2.0, bt.shape + (3, 3))
    W[rng.random(W.shape) < 0.2] = 0.0
    return m, b, bt, W


def test_theta_sub_objective_skips_missing_bt(env):
    from fcdiff_amd.fit import theta_sub_objective, theta_full_objective
    (m, _b, bt, W) = objective_data(env)
    miss = np.isnan(bt)
    (bt_f, W0) = (np.where(miss, 0.3, bt), W.copy())
    W0[miss] = 0.0
    (bt_d, W_d, btf_d, W0_d) = (up(env, bt), up(env, W), up(env, bt_f), up(env, W0))
    for th in (m.theta(), np.r_[m.theta()[:1], 0.6, 0.2, m.theta()[3:]]):
        got = theta_sub_objective(env.ctx, bt_d, W_d, th, missing_data=True)
        want = theta_sub_objective(env.ctx, btf_d, W0_d, th)
        assert np.all(np.isfinite(got))
        nptest.assert_allclose(got, want, rtol=1e-12)
        got9 = theta_full_objective(env.ctx, None, bt_d, W_d, th, missing_data=True)
        nptest.assert_allclose(got9, theta_full_objective(env.ctx, None, btf_d, W0_d, th), rtol=1e-12, atol=1e-12)
        nptest.assert_allclose(got9[:3], got, rtol=1e-12)
    # central differences of the flag-on objective
    (S, dh, de) = theta_sub_objective(env.ctx, bt_d, W_d, m.theta(), missing_data=True)
    for (j, g) in ((1, dh), (2, de)):
        h = 1e-6
        (tp, tm) = (m.theta(), m.theta())
        tp[j] += h
        tm[j] -= h
        fd = (theta_sub_objective(env.ctx, bt_d, W_d, tp, missing_data=True)[0]
              - theta_sub_objective(env.ctx, bt_d, W_d, tm, missing_data=True)[0]) / (2 * h)
        nptest.assert_allclose(g, fd, rtol=1e-6)


def test_theta_full_objective_b_term_and_gradient(env):
    from fcdiff_amd.fit import theta_full_objective
    (m, b, bt, W) = objective_data(env, seed=12)
    (b_d, bt_d, W_d) = (up(env, b), up(env, bt), up(env, W))
    th = m.theta()
    full = theta_full_objective(env.ctx, b_d, bt_d, W_d, th, missing_data=True)
    no_b = theta_full_objective(env.ctx, None, bt_d, W_d, th, missing_data=True)
    assert np.all(np.isfinite(full))
    # the b term: sum_{c,k} wF[c,k] sum_{h observed} ln N(b; mu_k, sigma_k), and its mu / sigma^2 derivatives
    wF = W[:, 0].sum(axis=2)                                   # (C, 3)
    (mu, s2) = (m.mu, m.sigma ** 2)
    d = b[:, :, None] - mu                                     # (C, H, 3), NaN at missing b
    lnN = -(d * d) / (2 * s2) - 0.5 * np.log(2 * np.pi) - np.log(m.sigma)
    S_b = np.nansum(wF[:, None, :] * lnN)
    g_mu = np.nansum(wF[:, None, :] * d / s2, axis=(0, 1))
    g_s2 = np.nansum(wF[:, None, :] * (d * d - s2) / (2 * s2 * s2), axis=(0, 1))
    nptest.assert_allclose(full[0] - no_b[0], S_b, rtol=1e-11, atol=1e-13 * np.nansum(np.abs(wF[:, None, :] * lnN)))
    nptest.assert_allclose(full[1:3], no_b[1:3], rtol=1e-13)
    nptest.assert_allclose(full[3:6] - no_b[3:6], g_mu, rtol=1e-10, atol=1e-8)
    nptest.assert_allclose(full[6:9] - no_b[6:9], g_s2, rtol=1e-10, atol=1e-8)

    # the gradient is the derivative of the objective, in the reference's parametrisation (sigma^2)
    def S_at(x):
        t = th.copy()
        (t[1], t[2], t[6:9], t[9:12]) = (x[0], x[1], x[2:5], np.sqrt(x[5:8]))
        return theta_full_objective(env.ctx, b_d, bt_d, W_d, t, missing_data=True)[0]
    x0 = np.concatenate([[m.eta, m.epsilon], mu, s2])
    for j in range(8):
        h = 1e-6 * max(1.0, abs(x0[j])) if j < 5 else 1e-4 * x0[j]
        (xp, xm) = (x0.copy(), x0.copy())
        xp[j] += h
        xm[j] -= h
        fd = (S_at(xp) - S_at(xm)) / (2 * h)
        nptest.assert_allclose(full[1 + j], fd, rtol=1e-5, atol=1e-6 * abs(full[0]))


# ------------------------------------------------------------------------------------------------
# 7. connection posterior
# ------------------------------------------------------------------------------------------------
def test_conn_posterior_at_missing_and_observed_items(env):
    from fcdiff_amd.fit import conn_posterior
    (Nreg, U) = (13, 9)
    C = C_of(Nreg)
    rng = np.random.default_rng(8)
    theta = np.array([0.1, 0.3, 0.05, 0.3, 0.4, 0.3, -0.15, 0.0, 0.3, 0.03, 0.04, 0.05])
    bt = rng.uniform(-0.5, 0.5, (C, U))
    bt[rng.random(bt.shape) < 0.15] = np.nan
    bt[:, 4] = np.nan
    miss = np.isnan(bt)
    bt_d = up(env, bt)
    cnt = rng.integers(0, 40, (C, U, 3, 3)).astype(np.uint32)
    cnt[:, :, 0, 0] += 1
    lq_F = np.log(rng.dirichlet(np.ones(3), C))[:, None, :]
    lq_R = np.log(rng.dirichlet(np.ones(2), (Nreg, U)))
    import conn_posterior_ref as R
    for (kw, W) in (({"counts": up(env, cnt.view(np.int32))}, cnt), ({"lq_F": up(env, lq_F), "lq_R": up(env, lq_R)},
                                                                         R.vb_weights(lq_F, lq_R))):
        on = conn_posterior(env.ctx, bt_d, Nreg, U, theta, missing_data=True, **kw)
        off = conn_posterior(env.ctx, bt_d, Nreg, U, theta, **kw)
        want = MD.contract_prior(W, theta)
        for key in ("p_T", "p_F_tilde", "p_changed"):
            assert np.all(np.isfinite(on[key])), key
            assert np.array_equal(on[key][~miss], off[key][~miss]), key
            nptest.assert_allclose(on[key][miss], want[key][miss], rtol=1e-13, atol=1e-15, err_msg=key)
        nptest.assert_allclose(on["p_F_tilde"].sum(axis=2), 1.0, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------
# 8. end to end: constant series -> NaN correlations -> both fits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["vb", "gibbs"])
def test_end_to_end_from_time_series(env, method):
    from fcdiff_amd.corr import correlations
    import conn_posterior_ref as R
    (S, N, T, Hn) = (10, 12, 200, 6)
    (n_pat, u_pat, n_hl, h_hl) = (3, 1, 5, 2)
    rs = np.random.RandomState(2)
    ts = rs.standard_normal((S, N, T))
    ts[Hn + u_pat, n_pat, :] = 0.7          # one patient's region and one healthy subject's region are constant
    ts[h_hl, n_hl, :] = -1.5
    out = correlations(ts, ctx=env.ctx)
    (b, bt) = (out[:, :Hn].copy(), out[:, Hn:].copy())
    assert np.isnan(b).sum() == N - 1 and np.isnan(bt).sum() == N - 1
    model = env.pkg.UnsharedRegionModel()
    model.sigma = np.array([0.1, 0.1, 0.1])
    fit = new_fit(env, model, b, bt, method=method, edge_index="symmetric")
    if method == "vb":
        fit.max_iters = 4
    else:
        (fit.n_chains, fit.n_sweeps, fit.burn_in, fit.mstep_every) = (4096, 12, 2, 0)
        fit.connection_marginals = True
    fit.run()
    assert fit.missing_counts() == (N - 1, N - 1)
    assert not np.isnan(fit._lq_F).any() and not np.isnan(fit._lq_R).any()      # (gibbs: log 0 = -inf where no chain went)
    assert all(np.isfinite(fit.energy))
    assert np.isfinite(fit.model.pi) and np.all(np.isfinite(fit.model.gamma))
    post = fit.connection_posterior()
    for key in ("p_T", "p_F_tilde", "p_changed"):
        assert np.all(np.isfinite(post[key])), key
    miss = np.isnan(bt)
    if method == "vb":
        fit._update_lq_R()                     # one q_R update with the pi in force: the dead region sits at pi
        nptest.assert_allclose(np.exp(fit._lq_R[n_pat, u_pat, 1]), fit._pi2()[1], rtol=1e-13)
        W = R.vb_weights(fit._lq_F, fit._lq_R)
        post = fit.connection_posterior()
    else:
        # mstep_every = 0: the dead sites are redrawn from Bernoulli(pi) at every sweep, independently of everything
        eng = fit.sampler
        total = eng.n_accumulated * eng.G
        k = int(round(np.exp(fit._lq_R[n_pat, u_pat, 1]) * total))
        assert binom_ok(k, total, fit._pi2()[1])
        W = fit.connection_counts
    want = MD.contract_prior(W, fit.model.theta())
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(post[key][miss], want[key][miss], rtol=1e-12, atol=1e-14, err_msg=key)
