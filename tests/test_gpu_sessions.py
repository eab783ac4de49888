"""
Repeated sessions per patient on the MI355X: bt (C, U, K) through the table kernels (fcd_lik_tables_sessions,
fcd_lik_shared_tables_sessions), the connection posterior (fcd_conn_posterior_sessions), both fits with both methods,
the evidence and scoring, against the NumPy reference of tests/sessions_ref.py.

Tolerance rule of the tables: rtol 1e-12 (the project's table tolerance), atol = 1e-14 max(1, max |sum_k ln N|) over the
case -- the session sum rounds absolutely in its own magnitude (sessions_ref.tolerance).
"""
import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as CP
import evidence_ref as ER
import exact_law_cases as X
import missing_data_ref as MD
import sessions_ref as SR
from conftest import theta_dict
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu

FIT = dict(rtol=1e-10, atol=1e-12)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.tables, e.CO = torch, fcdiff_amd, _lib, tables, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def C_of(N):
    return N * (N - 1) // 2


def data(env, N, U, K, H=3, seed=None, strong=False):
    m = env.pkg.UnsharedRegionModel()
    if strong:
        m.mu, m.sigma = np.array([-0.5, 0.0, 0.5]), np.array([0.05, 0.05, 0.05])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U + K if seed is None else seed, sessions=K)
    return m, b, bt


def build(env, m, b, bt, flags=0, shared=False, count=False):
    """(S_B, lM, n_missing or None) of tables.build on host arrays."""
    n = env.torch.zeros(2, dtype=env.torch.int64, device="cuda") if count else None
    (S_B, lM) = env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), flags, shared=shared, n_missing=n)
    return S_B.cpu().numpy(), lM.cpu().numpy(), (None if n is None else tuple(n.cpu().tolist()))


def new_fit(env, model, b, bt, shared=False, **kw):
    fit = env.pkg.fit.SharedRegionFit() if shared else env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (model, b, bt)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


# ------------------------------------------------------------------------------------------------
# 1. the unshared table
# ------------------------------------------------------------------------------------------------
SHAPES = [(3, 1, 1), (3, 2, 2), (4, 3, 3),      # smallest
          (23, 1, 2),                           # 253 items: one partial tile, an odd count of doubles, the tail store
          (23, 2, 5),                           # two tiles with the second partial, odd K
          (33, 1, 8),                           # three tiles
          (8, 37, 9),                           # a full 9-session pass
          (8, 37, 10),                          # one more session than a pass
          (46, 1024, 2)]                        # 1 059 840 items > 16 * num_cu * 256: the grid-stride loop (the grid is capped)


@pytest.mark.parametrize("N,U,K", SHAPES)
def test_table_against_reference(env, N, U, K):
    (m, b, bt) = data(env, N, U, K)
    (S_B, lM, _n) = build(env, m, b, bt)
    (S_ref, lM_ref) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    nptest.assert_allclose(lM, lM_ref, **SR.tolerance(bt, m.mu, m.sigma))
    # S_B: the 2-D kernel's, bit for bit
    (S_2d, _lM2) = env.tables.build(env.ctx, up(env, b), up(env, bt[:, :, 0]), m.theta(), 0)
    nptest.assert_array_equal(S_B, S_2d.cpu().numpy())
    nptest.assert_allclose(S_B, S_ref, rtol=1e-12)


def test_lp_B_g_F_equals_the_2d_kernels(env):
    (m, b, bt) = data(env, 9, 4, 3, H=7)
    t = env.torch
    lpB = t.empty((C_of(9), 7, 3), dtype=t.float64, device="cuda")
    lpB2 = t.empty_like(lpB)
    env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), 0, lpB=lpB)
    env.tables.build(env.ctx, up(env, b), up(env, bt[:, :, 1]), m.theta(), 0, lpB=lpB2)
    nptest.assert_array_equal(lpB.cpu().numpy(), lpB2.cpu().numpy())


@pytest.mark.parametrize("N,U", [(23, 2), (8, 37)])
def test_one_session_as_3d_against_the_2d_kernel(env, N, U):
    (m, b, bt) = data(env, N, U, 1)
    (_S, lM, _n) = build(env, m, b, bt)
    (_S2, lM2, _n2) = build(env, m, b, bt[:, :, 0])
    nptest.assert_allclose(lM, lM2, **SR.tolerance(bt, m.mu, m.sigma))


@pytest.mark.parametrize("pattern", ["random", "patient"])
@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_nan_session_is_bit_identical_to_leaving_it_out(env, pattern, where):
    (N, U, K) = (23, 5, 4)
    MISS = env.lib.FCD_DATA_NAN_MISSING
    (m, b, bt) = data(env, N, U, K - 1)
    rng = np.random.default_rng(5)
    if pattern == "random":
        bt[rng.random(bt.shape) < 0.1] = np.nan                # 10 % NaN session entries
    else:
        bt[:, 2, :] = np.nan                                    # one whole patient
    bt[7, 1, :] = np.nan                                        # an item with no observed session
    (S0, lM0, n0) = build(env, m, b, bt, MISS, count=True)
    btn = np.insert(bt, {"front": 0, "middle": 2, "end": K - 1}[where], np.nan, axis=2)
    assert btn.shape == (C_of(N), U, K)
    (S1, lM1, n1) = build(env, m, b, btn, MISS, count=True)
    nptest.assert_array_equal(lM1, lM0)
    nptest.assert_array_equal(S1, S0)
    none = np.isnan(btn).all(axis=2)
    assert none.sum() >= 1 and np.all(lM1[none] == 0.0) and not np.signbit(lM1[none]).any()
    assert np.all(np.isfinite(lM1))
    assert n0 == (0, int(np.isnan(bt).sum())) and n1 == (0, int(np.isnan(btn).sum()))
    (_S, lM_ref) = SR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, missing=True)
    nptest.assert_allclose(lM1, lM_ref, **SR.tolerance(btn, m.mu, m.sigma, missing=True))
    # the fit's own count
    fit = new_fit(env, m, b, btn, missing_data=True)
    fit._init_lps(N, b.shape[1], U)
    fit._update_lps()
    assert fit.missing_counts() == (0, int(np.isnan(btn).sum())) and fit.n_sessions == K
    nptest.assert_array_equal(fit._lM, lM1)


def test_without_the_flag_nan_stays_in_its_item(env):
    (m, b, bt) = data(env, 9, 5, 3)
    (bt[5, 2, 1], bt[20, 0, 0], bt[35, 4, 2]) = (np.nan, np.nan, np.nan)
    (_S, lM, _n) = build(env, m, b, bt)
    bad = np.isnan(bt).any(axis=2)
    assert bad.sum() == 3
    assert np.all(np.isnan(lM[bad])) and np.all(np.isfinite(lM[~bad]))


def test_sixteen_sessions_whose_product_underflows(env):
    """sigma = 0.05, types 0.5 apart, every session at 1.0: every prod_k N_j is 0 in fp64 (sum ln N <= -766); lM is finite."""
    (m, b, _bt) = data(env, 4, 3, 1, strong=True)
    bt = np.ones((C_of(4), 3, 16))
    (a, _n) = SR.session_log_sums(bt, m.mu, m.sigma)
    assert a.max() <= -766.0
    (_S, lM, _n) = build(env, m, b, bt)
    (_S, lM_ref) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    assert np.all(np.isfinite(lM)) and np.all(np.isfinite(lM_ref)) and -775.0 < lM_ref.max() < -765.0
    nptest.assert_allclose(lM, lM_ref, **SR.tolerance(bt, m.mu, m.sigma))
    # the shared table likewise
    (_S, L, _n) = build(env, m, b, bt, shared=True)
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **SR.tolerance(bt, m.mu, m.sigma, scale=3))


def test_entry_point_refusals(env):
    (m, b, bt) = data(env, 4, 2, 2)
    t = env.torch
    (b_d, bt_d) = (up(env, b), up(env, bt))
    (S_B, lM) = (t.empty((6, 3), dtype=t.float64, device="cuda"), t.empty((6, 2, 3, 3), dtype=t.float64, device="cuda"))
    (th, _th) = env.lib.dbl_array(m.theta())
    P = env.lib.dptr

    def tab(C=6, K=2, flags=0):
        env.ctx.call("fcd_lik_tables_sessions", P(b_d), P(bt_d), C, 3, 2, K, th, P(S_B), P(lM), P(None), flags, P(None),
                     env.lib.stream_ptr())

    def shr(C=6, K=2, flags=0):
        env.ctx.call("fcd_lik_shared_tables_sessions", P(b_d), P(bt_d), C, 3, 2, K, th, P(S_B), P(lM), flags, P(None),
                     env.lib.stream_ptr())
    for fn in (tab, shr):
        fn()
        with pytest.raises(ValueError):
            fn(K=0)
        with pytest.raises(NotImplementedError):
            fn(K=1 << 31)
        with pytest.raises(ValueError, match="triangular"):
            fn(C=5)
        with pytest.raises(ValueError, match="flags"):
            fn(flags=4)
    out = [t.empty((6, 2), dtype=t.float64, device="cuda"), t.empty((6, 2, 3), dtype=t.float64, device="cuda"),
           t.empty((6, 2), dtype=t.float64, device="cuda")]
    cnt = t.ones((6, 2, 3, 3), dtype=t.int32, device="cuda")

    def post(K=2, flags=0):
        env.ctx.call("fcd_conn_posterior_sessions", P(bt_d), 4, 2, K, th, P(cnt), P(None), P(None), flags, P(out[0]), P(out[1]),
                     P(out[2]), env.lib.stream_ptr())
    post()
    with pytest.raises(ValueError):
        post(K=0)
    with pytest.raises(NotImplementedError):
        post(K=1 << 31)
    with pytest.raises(ValueError, match="flags"):
        post(flags=2)


# ------------------------------------------------------------------------------------------------
# 2. the shared table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("U", [1, 16, 17, 33, 70])
def test_shared_table_is_the_patient_sum(env, U, K):
    MISS = env.lib.FCD_DATA_NAN_MISSING
    (m, b, bt) = data(env, 6, U, K)
    (S_u, lM, _n) = build(env, m, b, bt)
    (S_s, L, _n) = build(env, m, b, bt, shared=True)
    assert L.shape == (C_of(6), 1, 3, 3)
    nptest.assert_allclose(L[:, 0], lM.sum(axis=1), **SR.tolerance(bt, m.mu, m.sigma, scale=U))
    nptest.assert_array_equal(S_s, S_u)
    (S_2, L2, _n) = build(env, m, b, bt, shared=True)
    nptest.assert_array_equal(L2, L)
    nptest.assert_array_equal(S_2, S_s)
    # NaN sessions: skipped and counted
    btn = bt.copy()
    btn[np.random.default_rng(U + K).random(bt.shape) < 0.2] = np.nan
    btn[3, 0, :] = np.nan
    (_S, lMn, _n) = build(env, m, b, btn, MISS)
    (_S, Ln, n) = build(env, m, b, btn, MISS, shared=True, count=True)
    nptest.assert_allclose(Ln[:, 0], lMn.sum(axis=1), **SR.tolerance(btn, m.mu, m.sigma, missing=True, scale=U))
    assert n == (0, int(np.isnan(btn).sum()))


# ------------------------------------------------------------------------------------------------
# 3. connection posterior
# ------------------------------------------------------------------------------------------------
def enumerated_posterior(W, bt, theta, missing):
    """{p_T, p_F_tilde, p_changed} from missing_data_ref.enumerate_law with like = prod_k N_j (relative to its largest),
    contracted over the weights W (C, U, 3, 3)."""
    theta = np.asarray(theta, dtype=np.float64)
    (a, _n) = SR.session_log_sums(bt, theta[6:9], theta[9:12], missing)
    like = np.exp(a - a.max(axis=2, keepdims=True))
    (C, U) = bt.shape[:2]
    out = {"p_T": np.zeros((C, U)), "p_F_tilde": np.zeros((C, U, 3)), "p_changed": np.zeros((C, U))}
    for c in range(C):
        for u in range(U):
            (_M, pT, pF, pch) = MD.enumerate_law(theta[1], theta[2], like=like[c, u])
            w = W[c, u] / W[c, u].sum()
            out["p_T"][c, u] = (w * pT).sum()
            out["p_F_tilde"][c, u] = np.einsum("kl,klj->j", w, pF)
            out["p_changed"][c, u] = (w * pch).sum()
    return out


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("N,U,K", [(4, 3, 3), (6, 5, 4)])
def test_connection_posterior_against_the_enumeration(env, N, U, K, nan):
    from fcdiff_amd.fit import conn_posterior
    (m, _b, bt) = data(env, N, U, K)
    m.sigma = np.array([0.1, 0.12, 0.15])
    theta = m.theta()
    rng = np.random.default_rng(N + K)
    if nan:
        bt[rng.random(bt.shape) < 0.25] = np.nan
        bt[1, 0, :] = np.nan
    C = C_of(N)
    cnt = rng.integers(0, 40, (C, U, 3, 3)).astype(np.uint32)
    cnt[:, :, 0, 0] += 1
    lq_F = np.log(rng.dirichlet(np.ones(3), C))[:, None, :]
    lq_R = np.log(rng.dirichlet(np.ones(2), (N, U)))
    for (kw, W) in (({"counts": up(env, cnt.view(np.int32))}, cnt.astype(np.float64)),
                    ({"lq_F": up(env, lq_F), "lq_R": up(env, lq_R)}, CP.vb_weights(lq_F, lq_R))):
        got = conn_posterior(env.ctx, up(env, bt), N, U, theta, missing_data=nan, **kw)
        want = enumerated_posterior(W, bt, theta, nan)
        for key in ("p_T", "p_F_tilde", "p_changed"):
            nptest.assert_allclose(got[key], want[key], rtol=1e-12, atol=1e-14, err_msg=key)
        if nan:
            prior = MD.contract_prior(W, theta)
            nptest.assert_allclose(got["p_T"][1, 0], prior["p_T"][1, 0], rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------------------------
# 4. end to end
# ------------------------------------------------------------------------------------------------
def e2e_data(env):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(5, 4, 3, seed=21, sessions=3)
    return b, bt


@pytest.mark.parametrize("shared", [False, True])
def test_vb_fit_against_the_oracle_on_reference_tables(env, shared):
    (b, bt) = e2e_data(env)
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    start = theta_dict(model.theta())
    fit = new_fit(env, model, b, bt, shared=shared, max_iters=4, rel_tol=-np.inf)
    fit.run()
    want = SR.vb_fit(b, bt, start, 4, O.EDGE_SYMMETRIC if shared else O.EDGE_REFERENCE, shared=shared)
    assert len(fit.energy) == 5 and fit.n_sessions == 3
    nptest.assert_allclose(fit.energy, want["energy"], **FIT)
    nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
    nptest.assert_allclose(fit._lq_F, want["lq_F"], **FIT)
    assert fit._lq_R.shape == (5, 1 if shared else 3, 2)
    tol = SR.tolerance(bt, model.mu, model.sigma, scale=3 if shared else 1)
    nptest.assert_allclose(fit._lM, want["lM"], **tol)
    # the queries that read only the fit's state
    cp = fit.anomaly_count_posterior()
    assert all(np.all(np.isfinite(v)) for v in cp.values())
    co = fit.coanomaly_posterior()
    nptest.assert_allclose(np.diag(co["p_region_pair"]), np.exp(fit._lq_R[:, :, 1]).mean(axis=1), rtol=1e-12)
    post = fit.connection_posterior()
    W = CP.vb_weights(fit._lq_F, np.broadcast_to(fit._lq_R, (5, 3, 2)) if shared else fit._lq_R)
    ref = enumerated_posterior(W, bt, fit.model.theta(), False)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(post[key], ref[key], rtol=1e-12, atol=1e-14, err_msg=key)


@pytest.mark.parametrize("shared", [False, True])
def test_gibbs_fit_equals_the_oracle_chain_for_chain(env, shared):
    (b, bt) = e2e_data(env)
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    fit = new_fit(env, model, b, bt, shared=shared, method="gibbs", n_chains=128, n_sweeps=6, burn_in=2, mstep_every=0,
                  seed=77, trace_every=1, connection_marginals=True, anomaly_counts=True, coanomaly=True)
    (gamma, pi2) = (np.array(model.gamma, dtype=np.float64), model.pi2())
    fit.run()
    (S_B, lM) = (fit._d["S_B"].cpu().numpy(), fit._lM)
    (N, U) = (5, 1 if shared else 3)
    (S_ref, lM_ref) = SR.lik_tables(b, bt, model.mu, model.sigma, model.eta, model.epsilon)
    nptest.assert_allclose(lM, lM_ref.sum(axis=1, keepdims=True) if shared else lM_ref,
                           **SR.tolerance(bt, model.mu, model.sigma, scale=3 if shared else 1))
    (f_o, r_o) = env.CO.gibbs_init(128, N, U, float(pi2[1]), 77, 0)
    for s in range(6):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(gamma), 77, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, np.log(pi2), 77, s, env.lib.EDGE_MODES["symmetric"], 0)
    (f_g, r_g) = fit.sampler.export_state()
    assert env.ctx.stat("dev_err") == 0
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    # the queries on a sampler fit of sessions data
    d = fit.diagnostics()
    assert "sum_r" in d
    assert all(np.all(np.isfinite(v)) for v in fit.anomaly_count_posterior().values())
    assert all(np.all(np.isfinite(v)) for v in fit.coanomaly_posterior().values())
    post = fit.connection_posterior()
    W = np.asarray(fit.connection_counts, dtype=np.float64)
    ref = enumerated_posterior(np.broadcast_to(W, (C_of(5), 3, 3, 3)), bt, fit.model.theta(), False)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(post[key], ref[key], rtol=1e-12, atol=1e-14, err_msg=key)
    # membership stays one scan per subject
    with pytest.raises(ValueError, match="x_new must be"):
        fit.membership(bt[:, :2, :])
    out = fit.membership(bt[:, :2, 0], n_anneal=8)
    assert np.all(np.isfinite(out["log_bf"]))


@pytest.mark.parametrize("shared", [False, True])
def test_log_evidence_against_the_enumeration(env, shared):
    """4 regions, 2 patients, 2 sessions: the acceptance rule of test_gpu_evidence.py's enumerated cases."""
    m = X.model("broad")
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(4, 2, 2, seed=42, sessions=2)
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    for k in ("pi", "eta", "epsilon"):
        setattr(model, k, getattr(m, k))
    (model.gamma, model.mu, model.sigma) = (np.array(m.gamma), np.array(m.mu), np.array(m.sigma))
    fit = new_fit(env, model, b, bt, shared=shared, max_iters=2, n_chains=64)
    fit.run()
    for k in ("pi", "eta", "epsilon"):
        setattr(model, k, getattr(m, k))
    model.gamma = np.array(m.gamma)
    (S_B, lM) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    exact = (ER.exact_log_evidence_shared if shared else ER.exact_log_evidence)(S_B, lM, np.asarray(m.gamma, dtype=np.float64),
                                                                                 m.pi2())
    out = fit.log_evidence(n_anneal=50, n_chains=4096, seed=1282)
    print("shared=%s exact %.4f estimate %.4f se %.4f ess %.0f lower %.4f (%.4f)" % (
        shared, exact, out["log_evidence"], out["log_evidence_se"], out["ess"], out["lower"], out["lower_se"]))
    assert out["n_chains"] == 4096 and out["n_anneal"] == 50
    assert abs(out["log_evidence"] - exact) <= 5.0 * out["log_evidence_se"]
    assert out["lower"] - 5.0 * out["lower_se"] <= exact


def snapshot(fit):
    (f, r) = (fit.sampler.export_state() if fit.sampler is not None else (None, None))
    return {"theta": np.asarray(fit.model.theta()).tobytes(), "lq_R": fit._lq_R.tobytes(), "lq_F": fit._lq_F.tobytes(),
            "energy": np.asarray(fit.energy).tobytes(), "lM": fit._lM.tobytes(),
            "S_B": fit._d["S_B"].cpu().numpy().tobytes(), "f": None if f is None else f.tobytes(),
            "r": None if r is None else r.tobytes()}


@pytest.mark.parametrize("method", ["vb", "gibbs"])
def test_score_with_another_number_of_sessions(env, method):
    (N, H, U) = (6, 4, 4)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=8, sessions=3)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(N, H, 3, seed=9, sessions=2)
    kw = dict(method=method, edge_index="symmetric", max_iters=3, n_chains=128, n_sweeps=8, burn_in=2)
    fit = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt, **kw)
    fit.run()
    before = snapshot(fit)
    out = fit.score(bt_new, connections=True, n_anneal=10, n_sweeps=5)
    assert snapshot(fit) == before
    assert out["p_R"].shape == (N, 3) and out["p_T"].shape == (C_of(N), 3)
    assert all(np.all(np.isfinite(out[k])) for k in ("p_R", "p_T", "p_F_tilde", "p_changed"))
    if method == "vb":
        # K' = 1 given as (C, U', 1) on a fit of (C, U, 1) against the same patients, 2-D, on the 2-D fit of the same data
        # (deterministic updates on tables that agree to the table tolerance; the sampler's draws are not compared)
        fit1 = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt[:, :, :1], **kw)
        fit2 = new_fit(env, env.pkg.UnsharedRegionModel(), b, np.ascontiguousarray(bt[:, :, 0]), **kw)
        fit1.run()
        fit2.run()
        s1 = fit1.score(bt_new[:, :, :1])
        s2 = fit2.score(np.ascontiguousarray(bt_new[:, :, 0]))
        nptest.assert_allclose(s1["p_R"], s2["p_R"], **FIT)
        nptest.assert_allclose(s1["elbo"], s2["elbo"], **FIT)
    with pytest.raises(ValueError, match="bt_new must be"):
        fit.score(bt_new[:, :, :, None])


def test_sessions_are_not_extra_patients(env):
    """A patient given as K sessions is one patient: the state keeps U columns and the table is the sessions table, not the
    table of U K patients."""
    (N, H, U, K) = (5, 4, 3, 3)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=21, sessions=K)
    fit = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt, max_iters=2)
    fit.run()
    assert fit._lq_R.shape == (N, U, 2) and fit._lM.shape == (C_of(N), U, 3, 3)
    mm = fit.model
    (_S, lM_ref) = SR.lik_tables(b, bt, mm.mu, mm.sigma, mm.eta, mm.epsilon)
    nptest.assert_allclose(fit._lM, lM_ref, **SR.tolerance(bt, mm.mu, mm.sigma))
    (_lpB, _pBt, lM_stacked) = O.lik_tables(b, bt.reshape(C_of(N), U * K), mm.mu, mm.sigma, mm.eta, mm.epsilon)
    assert not np.allclose(fit._lM, lM_stacked[:, :U], rtol=1e-3, atol=1e-3)
    assert not np.allclose(fit._lM, lM_stacked[:, ::K], rtol=1e-3, atol=1e-3)
    stacked = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt.reshape(C_of(N), U * K), max_iters=2)
    stacked.run()
    assert stacked._lq_R.shape == (N, U * K, 2)
