"""
Anomalous-region counts on the MI355X: the histogram accumulator of fcd_gibbs_run (fcd_gibbs_set_count_accumulator /
fcd_gibbs_count_tally) against the NumPy restatement of tests/count_posterior_ref.py, the C oracle's chains, the marginal
counters and the exact posterior of small models; the Poisson-binomial kernel of the variational fit
(fcd_vb_count_posterior); and UnsharedRegionFit.anomaly_count_posterior() end to end.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest

import count_posterior_ref as R
import exact_law_cases as X
from oracle.exact_chain import ExactChain

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
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO = torch, fcdiff_amd, _lib, GibbsEngine, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def tables(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


@pytest.mark.parametrize("N,H,U,G,n_sweeps,burn", [(64, 16, 16, 256, 9, 2), (200, 50, 50, 1024, 5, 1)],
                         ids=["cfg2", "cfg3"])
def test_accumulator_is_exact(env, N, H, U, G, n_sweeps, burn):
    """
    fcd_gibbs_run with the accumulator, every = 1 / 3: equal, integer for integer, to the NumPy histograms of the C
    oracle's chains over the same sweeps.  The sampler is untouched: chain state and hyper-parameters bit-identical to a
    run without the accumulator.  With every = 1 the histograms' first moments are the marginal counters exactly.
    """
    (m, S_B, lM) = tables(env, N, H, U, seed=N + U)
    (S_B_d, lM_d) = (up(env, S_B), up(env, lM))
    seed = 404

    def engine():
        e = env.GibbsEngine(S_B_d, lM_d, N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.2)
        return e
    # with the in-tally M-step, as the fit runs it; the pair accumulator attached as well in one of the runs
    plain = engine()
    plain.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
    (f0, r0) = plain.export_state()
    h0 = plain.hyper_values()
    for (every, with_pair) in ((1, False), (3, True)):
        acc = engine()
        acc.attach_count_accumulator(every)
        if with_pair:
            acc.attach_pair_accumulator(2)
        acc.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        (hp, hr) = acc.count_hist_host()
        (f1, r1) = acc.export_state()
        nptest.assert_array_equal(f1, f0)
        nptest.assert_array_equal(r1, r0)
        (g1, p1) = acc.hyper_values()
        assert np.array_equal(g1, h0[0]) and p1 == h0[1]
        assert acc.count_sweeps == len(range(burn, n_sweeps, every))
        assert hp.shape == (U, N + 1) and hr.shape == (N, U + 1)
        assert np.all(hp.sum(axis=1) == G * acc.count_sweeps) and np.all(hr.sum(axis=1) == G * acc.count_sweeps)
        if every == 1:
            cnt_r = acc.host(acc.cnt_r).astype(np.int64)
            k_p = np.arange(N + 1, dtype=np.int64)
            k_r = np.arange(U + 1, dtype=np.int64)
            nptest.assert_array_equal(hp.astype(np.int64) @ k_p, cnt_r.sum(axis=0))
            nptest.assert_array_equal(hr.astype(np.int64) @ k_r, cnt_r.sum(axis=1))
        if with_pair:
            assert acc.pair_sweeps == len(range(burn, n_sweeps, 2))
            assert int(acc.pair_counts_host()[0, 0].sum()) == G * acc.pair_sweeps
    # against the C oracle's chains (fixed hyper-parameters)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.2, seed, 0)
    per_sweep = {}
    for s in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES["symmetric"], 0)
        if s >= burn:
            per_sweep[s] = R.histograms(r_o)
    for every in (1, 3):
        eng = engine()
        eng.attach_count_accumulator(every)
        eng.run(0, n_sweeps, mstep_every=0, accumulate_from=burn)
        (hp, hr) = eng.count_hist_host()
        nptest.assert_array_equal(hp.astype(np.int64), sum(per_sweep[s][0] for s in range(burn, n_sweeps, every)))
        nptest.assert_array_equal(hr.astype(np.int64), sum(per_sweep[s][1] for s in range(burn, n_sweeps, every)))
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        nptest.assert_array_equal(r_g, r_o)


def test_run_refuses_another_shape_while_attached(env):
    (N, U, G) = (12, 5, 64)
    (m, S_B, lM) = tables(env, N, 3, U, seed=3)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    hp = env.torch.zeros((U + 1, N + 2), dtype=env.torch.int32, device="cuda")
    hr = env.torch.zeros((N + 1, U + 2), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_set_count_accumulator", env.lib.dptr(hp), env.lib.dptr(hr), N + 1, U + 1, 1)
    try:
        with pytest.raises(Exception):
            eng._run(0, 1, 0, 0, False)
    finally:
        env.ctx.call("fcd_gibbs_set_count_accumulator", None, None, 0, 0, 1)
    assert int(hp.abs().sum()) == 0 and int(hr.abs().sum()) == 0


def import_r_bits(env, r):
    """Pack r (G, Nreg, U) with fcd_gibbs_import_state (f all zero) into an r_bits tensor; no tables needed."""
    t = env.torch
    (G, N, U) = r.shape
    Cn = N * (N - 1) // 2
    GW = (G + 63) // 64
    f_state = t.zeros((GW, Cn, 64), dtype=t.uint8, device="cuda")
    r_bits = t.zeros((GW, N, U), dtype=t.int64, device="cuda")
    f = t.zeros((G, Cn), dtype=t.uint8, device="cuda")
    env.ctx.call("fcd_gibbs_import_state", env.lib.dptr(f), env.lib.dptr(up(env, r.astype(np.uint8))), N, U, G,
                 env.lib.dptr(f_state), env.lib.dptr(r_bits), env.lib.stream_ptr())
    return r_bits


@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (130, 400, 500), (64, 1023, 3), (1, 2, 512)])
def test_count_tally_single_state(env, G, N, U):
    """fcd_gibbs_count_tally on an imported state (partial last chain word, largest shapes): NumPy histograms, and it adds.
    The bits of the chains beyond G in the last word are set on purpose: they must not be counted."""
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    r_bits = import_r_bits(env, r)
    if G % 64:
        w = G // 64
        r_bits[w] |= ~((1 << (G % 64)) - 1)
    hp = env.torch.zeros((U, N + 1), dtype=env.torch.int32, device="cuda")
    hr = env.torch.zeros((N, U + 1), dtype=env.torch.int32, device="cuda")
    for _ in range(2):
        env.ctx.call("fcd_gibbs_count_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hp), env.lib.dptr(hr),
                     env.lib.stream_ptr())
    (want_p, want_r) = R.histograms(r)
    nptest.assert_array_equal(hp.cpu().numpy().astype(np.int64), 2 * want_p)
    nptest.assert_array_equal(hr.cpu().numpy().astype(np.int64), 2 * want_r)


def test_host_side_refusals_with_a_context(env):
    """The checks that come before any device work, on a live context."""
    (lib, ctx, E) = (env.lib.load(), env.ctx.handle, env.lib)
    fake = C.c_void_p(16)          # never dereferenced: every call below is refused on the host
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, None, 4, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, fake, 1, 2, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, fake, 4, 0, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, fake, 4, 2, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, fake, 1024, 2, 1) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_count_accumulator(ctx, fake, fake, 4, 513, 1) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_count_accumulator(ctx, None, None, 0, 0, 1) == 0
    assert lib.fcd_gibbs_count_tally(ctx, None, 4, 2, 64, fake, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_count_tally(ctx, fake, 4, 2, 0, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_count_tally(ctx, fake, 4, 600, 64, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_vb_count_posterior(ctx, fake, 0, 2, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_vb_count_posterior(ctx, fake, 4, 2, None, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_vb_count_posterior(ctx, fake, 4096, 2, fake, fake, None) == E.FCD_ERR_UNSUPPORTED


def exact_count_laws(name):
    """Exact posterior law of both counts of an exact_law_cases problem: (p_patient (U, N+1), p_region (N, U+1), ec, pi)."""
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (_f, r) = ec.all_states()
    (sp, sr) = (r.astype(np.int64).sum(axis=1), r.astype(np.int64).sum(axis=2))     # (S, U), (S, N)
    p_patient = np.zeros((U, N + 1))
    p_region = np.zeros((N, U + 1))
    for u in range(U):
        np.add.at(p_patient[u], sp[:, u], pi)
    for n in range(N):
        np.add.at(p_region[n], sr[:, n], pi)
    return p_patient, p_region, ec, pi


@pytest.mark.parametrize("name", ["3x2", "4x2", "3x2-strong"])
def test_gibbs_counts_against_exact(env, name):
    """2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: within 5 x 0.5/sqrt(G) + 1e-4."""
    (want_p, want_r, ec, pi) = exact_count_laws(name)
    (P, K) = (ec.initial(X.PI0), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    G = X.G_CHAINS
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    eng.attach_count_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.count_sweeps == 1
    (hp, hr) = eng.count_hist_host()
    (got_p, got_r) = (hp / float(G), hr / float(G))
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%s: K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (
        name, K, max(np.abs(got_p - want_p).max(), np.abs(got_r - want_r).max()), tol))
    nptest.assert_allclose(got_p, want_p, rtol=0, atol=tol)
    nptest.assert_allclose(got_r, want_r, rtol=0, atol=tol)


@pytest.mark.parametrize("N,U", [(7, 13), (23, 5), (2, 1), (200, 50), (400, 250)])
def test_vb_count_kernel_against_numpy(env, N, U):
    """fcd_vb_count_posterior: the NumPy recursion at rtol 1e-12, rows summing to 1, q = 0 / 1 exact, lq_R unnormalised."""
    from fcdiff_amd.fit import count_posterior
    rng = np.random.default_rng(N * 1000 + U)
    q1 = rng.uniform(0, 1, (N, U))
    q1[rng.random((N, U)) < 0.1] = 0.0
    q1[rng.random((N, U)) < 0.1] = 1.0
    q1[0, :] = 0.0                                   # region 0 typical outside patient 0: a point mass at 1
    q1[:, 0] = 1.0                                   # patient 0 anomalous everywhere: a point mass at N
    with np.errstate(divide="ignore"):
        lq_R = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))      # not normalised
    (pp, pr) = count_posterior(env.ctx, up(env, lq_R), N, U)
    (want_p, want_r) = R.count_posterior(lq_R)
    nptest.assert_allclose(pp, want_p, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(pr, want_r, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(pp.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(pr.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(pp[0], np.eye(N + 1)[N])
    assert np.array_equal(pr[0], np.eye(U + 1)[1])         # (its site u = 0 is anomalous for sure)


def gibbs_fit(env, **kw):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(10, 6, 7, seed=8)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed = "gibbs", 192, 12, 3, 5
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit


def test_fit_gibbs_anomaly_counts(env):
    """The fit's histograms: from burn_in on, every k-th sweep, the same together with the connection counts and an
    energy callback; the sampler and the marginals are untouched; the default-off path attaches nothing and refuses."""
    off = gibbs_fit(env)
    assert off.patient_count_hist is None and off.sampler.count_hist is None
    with pytest.raises(ValueError):
        off.anomaly_count_posterior()
    on = gibbs_fit(env, anomaly_counts=True)
    (f_off, r_off) = off.sampler.export_state()
    (f_on, r_on) = on.sampler.export_state()
    nptest.assert_array_equal(f_on, f_off)
    nptest.assert_array_equal(r_on, r_off)
    nptest.assert_array_equal(on._lq_F, off._lq_F)
    nptest.assert_array_equal(on._lq_R, off._lq_R)
    (hp, hr) = (on.patient_count_hist, on.region_count_hist)
    assert hp.shape == (7, 11) and hr.shape == (10, 8) and on.anomaly_count_sweeps == 9
    assert np.all(hp.sum(axis=1) == 192 * 9) and np.all(hr.sum(axis=1) == 192 * 9)
    # first moments: the marginals of _lq_R (the same sweeps, every one counted)
    p1 = np.exp(on._lq_R[:, :, 1])
    nptest.assert_allclose(hp @ np.arange(11) / (192 * 9), p1.sum(axis=0), rtol=1e-12)
    nptest.assert_allclose(hr @ np.arange(8) / (192 * 9), p1.sum(axis=1), rtol=1e-12)
    out = on.anomaly_count_posterior()
    nptest.assert_allclose(out["p_patient_count"], hp / (192 * 9), rtol=1e-15)
    nptest.assert_allclose(out["p_region_count"], hr / (192 * 9), rtol=1e-15)
    nptest.assert_allclose(out["p_patient_any"], 1.0 - hp[:, 0] / (192 * 9), rtol=1e-15)
    nptest.assert_allclose(out["p_region_any"], 1.0 - hr[:, 0] / (192 * 9), rtol=1e-15)
    thin = gibbs_fit(env, anomaly_counts=True, anomaly_counts_every=4)
    assert thin.anomaly_count_sweeps == 3 and np.all(thin.patient_count_hist.sum(axis=1) == 192 * 3)   # sweeps 3, 7, 11
    both = gibbs_fit(env, anomaly_counts=True, anomaly_counts_every=4, connection_marginals=True, energy_every=1)
    nptest.assert_array_equal(both.patient_count_hist, thin.patient_count_hist)
    nptest.assert_array_equal(both.region_count_hist, thin.region_count_hist)
    assert both.connection_sweeps == 9 and np.all(both.connection_counts.sum(axis=(2, 3)) == 192 * 9)
    early = gibbs_fit(env, anomaly_counts=True, n_sweeps=3)
    with pytest.raises(ValueError):
        early.anomaly_count_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(env, anomaly_counts=True, anomaly_counts_every=0)


def test_fit_gibbs_anomaly_counts_with_missing_data(env):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(10, 6, 7, seed=8)
    bt = bt.copy()
    bt[::5, 1] = np.nan
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.missing_data = env.pkg.UnsharedRegionModel(), b, bt, True
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed, fit.anomaly_counts = "gibbs", 130, 8, 2, 5, True
    fit.run()
    assert fit.anomaly_count_sweeps == 6 and np.all(fit.patient_count_hist.sum(axis=1) == 130 * 6)
    p1 = np.exp(fit._lq_R[:, :, 1])
    nptest.assert_allclose(fit.region_count_hist @ np.arange(8) / (130 * 6), p1.sum(axis=1), rtol=1e-12)


@pytest.mark.parametrize("edge_index", ["reference", "symmetric"])
def test_vb_anomaly_count_posterior(env, edge_index):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(12, 6, 9, seed=4)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.max_iters, fit.edge_index = env.pkg.UnsharedRegionModel(), b, bt, 3, edge_index
    fit.run()
    out = fit.anomaly_count_posterior()
    (want_p, want_r) = R.count_posterior(fit._lq_R)
    nptest.assert_allclose(out["p_patient_count"], want_p, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_region_count"], want_r, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_patient_any"], 1.0 - want_p[:, 0], rtol=1e-12, atol=1e-15)
    nptest.assert_allclose(out["p_region_any"], 1.0 - want_r[:, 0], rtol=1e-12, atol=1e-15)
