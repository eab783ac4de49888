"""
The shared-region model on the MI355X: the patient-summed table kernel, the VB and Gibbs fits at U = 1 against the CPU
oracle and the exact enumeration, the per-edge theta_sub objective, the posteriors, the device sampler and the memory
the fit needs.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import shared_region_ref as SR
import conn_posterior_ref as CP
import count_posterior_ref as KP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    from oracle import c_oracle as CO
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO, e.O) = (torch, fcdiff_amd, _lib, GibbsEngine, CO, O)
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=env.ctx.device)


def model(env, pi=0.3, eta=0.4, epsilon=0.1):
    m = env.pkg.SharedRegionModel()
    m.pi, m.eta, m.epsilon = pi, eta, epsilon
    m.sigma = np.array([0.06, 0.06, 0.08])
    return m


def shared_tables(env, b, bt, theta, flags=0, counts=None):
    t = env.torch
    (C, H) = b.shape
    U = bt.shape[1]
    S_B = t.empty((C, 3), dtype=t.float64, device=env.ctx.device)
    L = t.empty((C, 3, 3), dtype=t.float64, device=env.ctx.device)
    (th, _th) = env.lib.dbl_array(theta)
    (b_dev, bt_dev) = (up(env, b), up(env, bt))          # held until the kernel has read them
    env.ctx.call("fcd_lik_shared_tables", env.lib.dptr(b_dev), env.lib.dptr(bt_dev), C, H, U, th, env.lib.dptr(S_B),
                 env.lib.dptr(L), flags, env.lib.dptr(counts), env.lib.stream_ptr())
    out = (S_B.cpu().numpy(), L.cpu().numpy())
    del b_dev, bt_dev
    return out


def unshared_tables(env, b, bt, theta, flags=0, counts=None):
    t = env.torch
    (C, H) = b.shape
    U = bt.shape[1]
    S_B = t.empty((C, 3), dtype=t.float64, device=env.ctx.device)
    lM = t.empty((C, U, 3, 3), dtype=t.float64, device=env.ctx.device)
    (th, _th) = env.lib.dbl_array(theta)
    (b_dev, bt_dev) = (up(env, b), up(env, bt))          # held until the kernel has read them
    env.ctx.call("fcd_lik_tables_ex", env.lib.dptr(b_dev), env.lib.dptr(bt_dev), C, H, U, th, env.lib.dptr(S_B),
                 env.lib.dptr(lM), None, None, flags, env.lib.dptr(counts), env.lib.stream_ptr())
    out = (S_B.cpu().numpy(), lM)
    del b_dev, bt_dev
    return out


# ------------------------------------------------------------------ 1. table kernel
@pytest.mark.parametrize("N,U", [(2, 1), (9, 63), (9, 64), (9, 65), (64, 16), (64, 2000), (400, 250)])
@pytest.mark.parametrize("H", [1, 7])
def test_table_kernel_against_lik_tables_and_oracle(env, N, U, H):
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=N + U + H)
    th = m.theta()
    (S_B, L) = shared_tables(env, b, bt, th)
    (S_B_u, lM_dev) = unshared_tables(env, b, bt, th)
    assert np.array_equal(S_B, S_B_u)                                   # bit for bit
    L_u = lM_dev.sum(dim=1).cpu().numpy()
    scale = lM_dev.abs().sum(dim=1).cpu().numpy()
    del lM_dev
    assert (np.abs(L - L_u) <= 1e-13 * scale).all()
    if N * U <= 64 * 2000:
        (lpB, _pBt, lM) = env.O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
        assert (np.abs(L - lM.sum(axis=1)) <= 1e-13 * np.abs(lM).sum(axis=1)).all()
        nptest.assert_allclose(S_B, lpB.sum(axis=1), rtol=1e-12)
    (S_B2, L2) = shared_tables(env, b, bt, th)
    assert np.array_equal(S_B2, S_B) and np.array_equal(L2, L)


@pytest.mark.parametrize("U", [5, 40, 130])
def test_table_kernel_missing_data_and_edges(env, U):
    t = env.torch
    m = model(env)
    (N, H) = (9, 4)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=U)
    rng = np.random.default_rng(U)
    b[rng.random(b.shape) < 0.1] = np.nan
    bt[rng.random(bt.shape) < 0.1] = np.nan
    th = m.theta()
    cs = t.zeros(2, dtype=t.int64, device=env.ctx.device)
    cu = t.zeros(2, dtype=t.int64, device=env.ctx.device)
    (S_B, L) = shared_tables(env, b, bt, th, env.lib.FCD_DATA_NAN_MISSING, cs)
    (S_B_u, lM_dev) = unshared_tables(env, b, bt, th, env.lib.FCD_DATA_NAN_MISSING, cu)
    assert np.array_equal(S_B, S_B_u)
    lM = lM_dev.cpu().numpy()
    assert (np.abs(L - lM.sum(axis=1)) <= 1e-13 * np.abs(lM).sum(axis=1) + 1e-300).all()
    obs = ~np.isnan(bt)
    (_lpB, _pBt, lM_o) = env.O.lik_tables(b, np.where(obs, bt, 0.0), m.mu, m.sigma, m.eta, m.epsilon)
    L_o = (lM_o * obs[:, :, None, None]).sum(axis=1)
    nptest.assert_allclose(L, L_o, rtol=1e-12, atol=1e-12)
    assert cs.cpu().tolist() == cu.cpu().tolist() == [int(np.isnan(b).sum()), int(np.isnan(bt).sum())]
    # without the flag a NaN propagates
    (_S, L_nan) = shared_tables(env, b, bt, th)
    rows = np.isnan(bt).any(axis=1)
    assert np.isnan(L_nan[rows]).all() and np.isfinite(L_nan[~rows]).all()
    # an item whose density underflows gives -inf, and so does its edge's sum
    bt2 = np.where(obs, bt, 0.0)
    bt2[1, 0] = 40.0
    (_S, L_inf) = shared_tables(env, b, bt2, th)
    assert np.isneginf(L_inf[1]).any()
    (_S, lM2) = unshared_tables(env, b, bt2, th)
    assert np.array_equal(np.isneginf(L_inf[1]), np.isneginf(lM2.cpu().numpy()[1, 0]))


# ------------------------------------------------------------------ 2./3. VB
def oracle_vb(env, S_B, L, m, iters):
    O = env.O
    (C, N) = (S_B.shape[0], env.pkg.util.C_to_N(S_B.shape[0]))
    N = int(N)
    L4 = L[:, None]
    lq_R = np.full((N, 1, 2), -np.log(2))
    lq_F = np.full((C, 1, 3), -np.log(3))
    (pi, gamma) = (float(m.pi), np.asarray(m.gamma, dtype=np.float64))
    energy = [O.eval_energy(lq_F, lq_R, S_B, L4, gamma, [1 - pi, pi])]
    for _ in range(iters):
        lq_F = O.update_lq_F(lq_R, S_B, L4, gamma)
        lq_R = O.update_lq_R(lq_R, lq_F, L4, [1 - pi, pi], O.EDGE_SYMMETRIC)
        (pi, gamma) = (O.update_pi(lq_R), O.update_gamma(lq_F))
        energy.append(O.eval_energy(lq_F, lq_R, S_B, L4, gamma, [1 - pi, pi]))
    return lq_R, lq_F, np.array(energy), pi, gamma


@pytest.mark.parametrize("N,H,U", [(5, 3, 7), (20, 4, 40), (64, 16, 16)])
@pytest.mark.parametrize("missing", [False, True])
def test_vb_fit_against_oracle_composition(env, N, H, U, missing):
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=N * U)
    if missing:
        rng = np.random.default_rng(1)
        b[rng.random(b.shape) < 0.05] = np.nan
        bt[rng.random(bt.shape) < 0.05] = np.nan
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt) = (model(env), b, bt)
    (fit.max_iters, fit.rel_tol, fit.missing_data) = (4, -np.inf, missing)
    fit.run()
    (S_B, L) = shared_tables(env, b, bt, m.theta(), env.lib.FCD_DATA_NAN_MISSING if missing else 0)
    (lq_R, lq_F, energy, pi, gamma) = oracle_vb(env, S_B, L, m, 4)
    assert fit._lq_R.shape == (N, 1, 2) and fit._lq_F.shape == (util_C(env, N), 1, 3)
    nptest.assert_allclose(fit._lq_R, lq_R, rtol=1e-10, atol=1e-10)
    nptest.assert_allclose(fit._lq_F, lq_F, rtol=1e-10, atol=1e-10)
    nptest.assert_allclose(fit.energy, energy, rtol=1e-10)
    nptest.assert_allclose(fit.model.pi, pi, rtol=1e-10)
    nptest.assert_allclose(fit.model.gamma, gamma, rtol=1e-10)
    if missing:
        assert fit.missing_counts() == (int(np.isnan(b).sum()), int(np.isnan(bt).sum()))


def util_C(env, N):
    return env.pkg.util.N_to_C(N)


@pytest.mark.parametrize("N,U", [(3, 4), (4, 3)])
def test_elbo_never_exceeds_log_evidence(env, N, U):
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, 2, U, seed=7 + N)
    ex = SR.enumerate_posterior(b, bt, m.theta())
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt) = (m, b, bt)
    fit._init_lps(N, 2, U)
    fit._update_lps()
    energies = [fit._eval_energy()]
    for _ in range(6):                  # the VB updates at fixed theta: the ELBO of this model rises towards log p(b, bt)
        fit._update_lq_F()
        fit._update_lq_R()
        energies.append(fit._eval_energy())
    assert (-np.array(energies) <= ex["log_evidence"] + 1e-9).all()
    assert -energies[-1] > ex["log_evidence"] - 1.0


# ------------------------------------------------------------------ 4. Gibbs
@pytest.mark.parametrize("N,G", [(17, 64), (5, 1), (30, 200)])
def test_gibbs_chains_on_L_equal_oracle_state_for_state(env, N, G):
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, 3, 11, seed=N)
    (S_B, L) = shared_tables(env, b, bt, m.theta())
    L4 = np.ascontiguousarray(L[:, None])
    seed = 0x0123456789ABCDEF + N
    eng = env.GibbsEngine(up(env, S_B), up(env, L4), N, 1, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.25)
    f_o, r_o = env.CO.gibbs_init(G, N, 1, 0.25, seed, 0)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for s in range(3):
        eng.sweeps(s, 1)
        env.CO.gibbs_f_step(f_o, r_o, S_B, L4, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, L4, lnpi2, seed, s, env.O.EDGE_SYMMETRIC, 0)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


def test_gibbs_fit_against_enumeration(env):
    (N, U, G) = (4, 3, 1 << 14)
    m = model(env, pi=0.3, eta=0.4, epsilon=0.2)
    m.sigma = np.array([0.15, 0.15, 0.2])
    (_r, _t, _f, _ft, b, bt) = m.sample(N, 2, U, seed=11)
    ex = SR.enumerate_posterior(b, bt, m.theta())
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt) = (m, b, bt)
    (fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.mstep_every) = ("gibbs", G, 40, 30, 0)
    (fit.connection_marginals, fit.anomaly_counts, fit.seed) = (True, True, 5)
    fit.run()
    (f, r) = fit.sampler.export_state()
    tol = lambda p: 5 * np.sqrt(np.maximum(p * (1 - p), 1e-4) / G)     # noqa: E731
    p_r = r[:, :, 0].mean(axis=0)
    assert (np.abs(p_r - ex["p_r"]) <= tol(ex["p_r"])).all(), (p_r, ex["p_r"])
    p_f = np.stack([(f == k).mean(axis=0) for k in range(3)], axis=1)
    assert (np.abs(p_f - ex["p_f"]) <= tol(ex["p_f"])).all(), (p_f, ex["p_f"])
    pc = fit.anomaly_count_posterior()
    assert pc["p_count"].shape == (N + 1,)
    assert (np.abs(pc["p_count"] - ex["p_count"]) <= tol(ex["p_count"])).all(), (pc["p_count"], ex["p_count"])
    cp = fit.connection_posterior()
    assert cp["p_T"].shape == (util_C(env, N), U) and cp["p_F_tilde"].shape == (util_C(env, N), U, 3)
    assert (np.abs(cp["p_T"] - ex["p_T"]) <= tol(ex["p_T"])).all()
    assert fit.region_posterior().shape == (N,)


# ------------------------------------------------------------------ 5. theta_sub
def numpy_objective(b, bt, W, theta):
    """S, dS/d eta, dS/d epsilon of sum_c sum_kl W[c,k,l] sum_u ln M_kl(bt_cu) (NaN bt adds nothing) + the b term."""
    th = np.asarray(theta, dtype=np.float64)
    (eta, epsilon, mu, sigma) = (th[1], th[2], th[6:9], th[9:12])
    obs = ~np.isnan(bt)
    x = np.where(obs, bt, 0.0)
    norm = np.stack([np.exp(-((x - mu[k]) / sigma[k]) ** 2 / 2) / np.sqrt(2 * np.pi) / sigma[k] for k in range(3)], axis=2)
    S = dh = de = 0.0
    for k in range(3):
        for l in range(3):
            e = [1 - epsilon, epsilon, eta * epsilon + (1 - eta) * (1 - epsilon)][l]
            js = [j for j in range(3) if j != k]
            M = e * norm[:, :, k] + (1 - e) * 0.5 * (norm[:, :, js[0]] + norm[:, :, js[1]])
            w = W[:, 0, k, l][:, None] * obs
            S += (w * np.log(M)).sum()
            de += (w * O_dlM_de(norm, M, eta, k, l)).sum()
            if l == 2:
                dh += (w * O_dlM_dh(norm, M, epsilon, k)).sum()
    wF = W[:, 0].sum(axis=2)
    ob = ~np.isnan(b)
    xb = np.where(ob, b, 0.0)
    Sb = sum((wF[:, k][:, None] * ob * (-((xb - mu[k]) / sigma[k]) ** 2 / 2 - np.log(np.sqrt(2 * np.pi)) - np.log(sigma[k]))).sum()
             for k in range(3))
    return S, dh, de, Sb


def O_dlM_dh(norm, mix, epsilon, k):
    from oracle import fcdiff_oracle as O
    return O.eval_dlM_dh(norm, mix, epsilon, k)


def O_dlM_de(norm, mix, eta, k, l):
    from oracle import fcdiff_oracle as O
    return O.eval_dlM_de(norm, mix, eta, k, l)


@pytest.mark.parametrize("missing", [False, True])
def test_per_edge_objective_against_numpy(env, missing):
    F = env.pkg.fit
    m = model(env)
    (N, H, U) = (12, 5, 37)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=3)
    if missing:
        rng = np.random.default_rng(3)
        bt[rng.random(bt.shape) < 0.1] = np.nan
        b[rng.random(b.shape) < 0.1] = np.nan
    C = util_C(env, N)
    W = np.random.default_rng(4).random((C, 1, 3, 3))
    W[0, 0, 1, 2] = 0.0
    th = m.theta()
    (S, dh, de, Sb) = numpy_objective(b, bt, W, th)
    o3 = F.theta_sub_objective(env.ctx, up(env, bt), up(env, W), th, missing_data=missing, per_edge=True)
    nptest.assert_allclose(o3, [S, dh, de], rtol=1e-11, atol=1e-8)
    o9 = F.theta_full_objective(env.ctx, up(env, b), up(env, bt), up(env, W), th, missing_data=missing, per_edge=True)
    nptest.assert_allclose(o9[:3], [S + Sb, dh, de], rtol=1e-11, atol=1e-8)
    # the per-edge form equals the per-patient form with W broadcast to every patient
    Wb = np.ascontiguousarray(np.broadcast_to(W, (C, U, 3, 3)))
    o9b = F.theta_full_objective(env.ctx, up(env, b), up(env, bt), up(env, Wb), th, missing_data=missing)
    nptest.assert_allclose(o9, o9b, rtol=1e-11, atol=1e-9)


@pytest.mark.parametrize("method", ["vb", "gibbs"])
def test_theta_sub_step_matches_scipy_on_numpy_objective(env, method):
    import scipy.optimize as spopt
    m = model(env)
    (N, H, U) = (10, 4, 30)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=9)
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt, fit.update_theta_sub, fit.method) = (model(env, eta=0.3, epsilon=0.05), b, bt, True, method)
    if method == "vb":
        fit.max_iters = 1
        start = (fit.model.eta, fit.model.epsilon)
        fit.run()
        W = CP.vb_weights(fit._lq_F, fit._lq_R)           # (C, 1, 3, 3)
    else:
        (fit.n_chains, fit.n_sweeps, fit.burn_in, fit.theta_sub_every) = (256, 3, 0, 2)
        start = (fit.model.eta, fit.model.epsilon)
        # the step at sweep 2 uses the pair counts of the chains after two sweeps: recompute them from a twin engine
        twin = env.pkg.fit.SharedRegionFit()
        (twin.model, twin.b, twin.bt, twin.method) = (model(env, eta=0.3, epsilon=0.05), b, bt, "gibbs")
        (twin.n_chains, twin.n_sweeps, twin.burn_in) = (256, 2, 0)
        twin.run()
        W = twin.sampler.pair_counts().cpu().numpy()
        fit.run()

    def fun(x):
        th = m.theta().copy()
        th[1], th[2] = x
        (S, dh, de, _Sb) = numpy_objective(b, bt, W, th)
        return -S, -np.array([dh, de])
    res = spopt.minimize(fun, np.clip(start, 1e-5, 1 - 1e-5), jac=True, bounds=((1e-5, 1 - 1e-5),) * 2, method="L-BFGS-B")
    nptest.assert_allclose([fit.model.eta, fit.model.epsilon], res.x, atol=1e-6)


# ------------------------------------------------------------------ 6. posteriors
@pytest.mark.parametrize("missing", [False, True])
def test_vb_posteriors_against_references(env, missing):
    m = model(env)
    (N, H, U) = (12, 3, 9)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=21)
    if missing:
        bt[np.random.default_rng(2).random(bt.shape) < 0.1] = np.nan
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt, fit.max_iters, fit.missing_data) = (m, b, bt, 3, missing)
    fit.run()
    cp = fit.connection_posterior()
    lq_R = np.broadcast_to(fit._lq_R, (N, U, 2))
    W = CP.vb_weights(fit._lq_F, lq_R)
    ref = CP.contract(W, np.where(np.isnan(bt), np.nan, bt), fit.model.theta())
    obs = ~np.isnan(bt)
    nptest.assert_allclose(cp["p_T"][obs], ref["p_T"][obs], rtol=1e-12, atol=1e-12)
    nptest.assert_allclose(cp["p_F_tilde"][obs], ref["p_F_tilde"][obs], rtol=1e-12, atol=1e-12)
    nptest.assert_allclose(cp["p_changed"][obs], ref["p_changed"][obs], rtol=1e-12, atol=1e-12)
    pc = fit.anomaly_count_posterior()
    (p_patient, _p_region) = KP.count_posterior(fit._lq_R)
    nptest.assert_allclose(pc["p_count"], p_patient[0], rtol=1e-12, atol=1e-12)
    nptest.assert_allclose(pc["p_any"], 1 - p_patient[0, 0], rtol=1e-12, atol=1e-12)
    nptest.assert_allclose(fit.region_posterior(), np.exp(fit._lq_R[:, 0, 1]), rtol=1e-15)


def test_vb_posteriors_against_enumeration(env):
    """Mean-field error allowed: 0.2 absolute on every probability (measured: 0.14 on one region at this case)."""
    (N, U) = (4, 5)
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, 3, U, seed=13)
    ex = SR.enumerate_posterior(b, bt, m.theta())
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt) = (m, b, bt)
    fit._init_lps(N, 3, U)
    fit._update_lps()
    for _ in range(10):
        fit._update_lq_F()
        fit._update_lq_R()
    nptest.assert_allclose(fit.region_posterior(), ex["p_r"], atol=0.2)
    nptest.assert_allclose(np.exp(fit._lq_F[:, 0]), ex["p_f"], atol=0.2)
    nptest.assert_allclose(fit.connection_posterior()["p_T"], ex["p_T"], atol=0.2)
    nptest.assert_allclose(fit.anomaly_count_posterior()["p_count"], ex["p_count"], atol=0.2)


# ------------------------------------------------------------------ 7. sampler
def test_sample_gpu_statistics(env):
    m = env.pkg.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.gamma, m.mu, m.sigma = np.array([0.2, 0.5, 0.3]), np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (N, H, U) = (300, 6, 50)
    (r, t, f, ft, b, bt) = m.sample_gpu(N, H, U, seed=1, ctx=env.ctx)
    C = util_C(env, N)
    assert r.shape == (N,) and r.dtype == bool and t.shape == (C, U) and f.shape == (C, 3) and ft.shape == (C, U, 3)
    assert b.shape == (C, H) and bt.shape == (C, U) and np.abs(bt).max() <= 1
    nptest.assert_allclose(r.mean(), 0.3, atol=5 * np.sqrt(0.21 / N))
    nptest.assert_allclose(f.mean(axis=0), m.gamma, atol=0.02)
    ends = np.array([env.pkg.c_to_nm(c) for c in range(C)])
    rn, rm = r[ends[:, 0]][:, None], r[ends[:, 1]][:, None]
    assert t[np.broadcast_to(rn & rm, t.shape)].all() and not t[np.broadcast_to(~rn & ~rm, t.shape)].any()
    nptest.assert_allclose(t[np.broadcast_to(rn ^ rm, t.shape)].mean(), 0.4, atol=0.02)
    fk, ftk = np.argmax(f, axis=1), np.argmax(ft, axis=2)
    same = ftk == fk[:, None]
    nptest.assert_allclose(same[~t].mean(), 0.8, atol=0.02)
    nptest.assert_allclose(same[t].mean(), 0.2, atol=0.02)
    for k in range(3):
        nptest.assert_allclose(b[fk == k].mean(), m.mu[k], atol=0.02)
        nptest.assert_allclose(bt[ftk == k].mean(), m.mu[k], atol=0.02)
    again = m.sample_gpu(N, H, U, seed=1, ctx=env.ctx)
    assert all(np.array_equal(x, y) for x, y in zip(again, (r, t, f, ft, b, bt)))
    other = m.sample_gpu(N, H, U, seed=2, ctx=env.ctx)
    assert not np.array_equal(other[5], bt)


# ------------------------------------------------------------------ 8. memory
def test_shared_fit_memory_stays_below_half_of_lM(env):
    t = env.torch
    (N, H, U) = (400, 250, 250)
    m = model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=1)
    C = util_C(env, N)
    fit = env.pkg.fit.SharedRegionFit()
    (fit.model, fit.b, fit.bt, fit.max_iters, fit.rel_tol, fit.update_theta_sub) = (m, b, bt, 3, -np.inf, True)
    t.cuda.synchronize()
    t.cuda.empty_cache()
    base = t.cuda.memory_allocated()
    t.cuda.reset_peak_memory_stats()
    fit.run()
    t.cuda.synchronize()
    used = t.cuda.max_memory_allocated() - base
    ctx = fit._context()
    total = used + ctx.stat("ws_bytes") + ctx.stat("fsq_bytes")
    assert len(fit.energy) == 4 and np.isfinite(fit.energy).all()
    assert total < 0.5 * 72 * C * U, (total, 72 * C * U)
