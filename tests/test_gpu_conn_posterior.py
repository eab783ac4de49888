"""
Connection-level posteriors on the MI355X: the contraction kernel (fcd_conn_posterior) and the (f_c, mixture case)
accumulator of fcd_gibbs_run (fcd_gibbs_set_pair_accumulator / fcd_gibbs_pair_tally) against the NumPy restatement of
tests/conn_posterior_ref.py, the C oracle's chains, fcd_gibbs_pair_counts and the exact posterior of small models.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as R
import exact_law_cases as X
from oracle.exact_chain import ExactChain

pytestmark = pytest.mark.gpu

TAB = dict(rtol=1e-12, atol=1e-290)


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


def up_counts(env, cnt):
    return up(env, np.asarray(cnt, dtype=np.uint32).view(np.int32))


def check_outputs(out, want):
    for key in ("p_T", "p_F_tilde", "p_changed"):
        assert np.all(np.isfinite(out[key])), key
        nptest.assert_allclose(out[key], want[key], **TAB, err_msg=key)
    nptest.assert_allclose(out["p_F_tilde"].sum(axis=2), 1.0, rtol=0, atol=1e-14)


def theta_of(eta, epsilon, mu, sigma):
    return np.concatenate([[0.1, eta, epsilon], [0.2, 0.6, 0.2], mu, sigma]).astype(np.float64)


@pytest.mark.parametrize("Nreg,U", [(7, 13), (23, 5), (2, 1), (41, 70)])
def test_contraction_kernel_against_numpy(env, Nreg, U):
    """Both weight sources at ragged C*U, bt with underflowing densities; p_T = 0 exactly where only l = 0 weighs."""
    from fcdiff_amd.fit import conn_posterior
    rng = np.random.default_rng(Nreg * 100 + U)
    Cn = Nreg * (Nreg - 1) // 2
    theta = theta_of(0.3, 0.03, [-0.15, 0.0, 0.3], [0.025, 0.035, 0.05])
    bt = rng.uniform(-1, 1, (Cn, U))
    bt.reshape(-1)[::7] = rng.choice([-40.0, 40.0, -1.0, 1.0, 1e3], size=bt.reshape(-1)[::7].shape)
    bt_d = up(env, bt)
    # counts: random, many zeros, and some items whose whole weight sits in l = 0
    cnt = rng.integers(0, 50, (Cn, U, 3, 3)).astype(np.uint32)
    cnt[rng.random((Cn, U, 3, 3)) < 0.4] = 0
    cnt[:, :, 0, 0] += 1
    typ = rng.random((Cn, U)) < 0.3
    cnt[typ, :, 1:] = 0
    out = conn_posterior(env.ctx, bt_d, Nreg, U, theta, counts=up_counts(env, cnt))
    check_outputs(out, R.contract(cnt, bt, theta))
    assert np.all(out["p_T"][typ] == 0.0)
    # the mean-field weights, read from lq_F / lq_R directly
    lq_F = np.log(rng.dirichlet(np.ones(3), Cn))[:, None, :]
    q1 = rng.uniform(0, 1, (Nreg, U))
    q1[0] = 0.0                       # region 0 typical for sure: some weight only in l = 0 / 2
    with np.errstate(divide="ignore"):
        lq_R = np.log(np.stack([1 - q1, q1], axis=2))
    out = conn_posterior(env.ctx, bt_d, Nreg, U, theta, lq_F=up(env, lq_F), lq_R=up(env, lq_R))
    check_outputs(out, R.contract(R.vb_weights(lq_F, lq_R), bt, theta))


@pytest.mark.parametrize("edge_index", ["reference", "symmetric"])
def test_vb_connection_posterior(env, edge_index):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(12, 6, 9, seed=4)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.max_iters, fit.edge_index = env.pkg.UnsharedRegionModel(), b, bt, 3, edge_index
    fit.run()
    out = fit.connection_posterior()
    assert out["p_T"].shape == bt.shape and out["p_F_tilde"].shape == bt.shape + (3,) and out["p_changed"].shape == bt.shape
    check_outputs(out, R.contract(R.vb_weights(fit._lq_F, fit._lq_R), bt, fit.model.theta()))


def tables(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


@pytest.mark.parametrize("N,H,U,G,n_sweeps,burn", [(64, 16, 16, 256, 9, 2), (200, 50, 50, 1024, 5, 1)],
                         ids=["cfg2", "cfg3"])
def test_accumulator_is_exact(env, N, H, U, G, n_sweeps, burn):
    """
    fcd_gibbs_run with the accumulator, every = 1 / 3: equal, integer for integer, to the sum of
    fcd_gibbs_pair_counts over the same sweeps (one call per sweep), and to the counts of the C oracle's chains.  The
    sampler is untouched: chain state and hyper-parameters bit-identical to a run without the accumulator.
    """
    (m, S_B, lM) = tables(env, N, H, U, seed=N + U)
    (S_B_d, lM_d) = (up(env, S_B), up(env, lM))
    seed = 404

    def engine():
        e = env.GibbsEngine(S_B_d, lM_d, N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.2)
        return e
    # with the in-tally M-step, as the fit runs it
    plain = engine()
    plain.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
    (f0, r0) = plain.export_state()
    h0 = plain.hyper_values()
    for every in (1, 3):
        acc = engine()
        acc.attach_pair_accumulator(every)
        acc.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        got = acc.pair_counts_host()
        (f1, r1) = acc.export_state()
        nptest.assert_array_equal(f1, f0)
        nptest.assert_array_equal(r1, r0)
        (g1, p1) = acc.hyper_values()
        assert np.array_equal(g1, h0[0]) and p1 == h0[1]
        assert acc.pair_sweeps == len(range(burn, n_sweeps, every))
        ref = engine()
        W = env.torch.zeros((ref.C, U, 3, 3), dtype=env.torch.float64, device="cuda")
        for s in range(n_sweeps):
            ref.run(s, 1, mstep_every=1, accumulate_from=burn)
            if s >= burn and (s - burn) % every == 0:
                ref.pair_counts(out=W, accumulate=True)
        nptest.assert_array_equal(got.astype(np.float64), ref.host(W))
        assert int(got[0, 0].sum()) == G * acc.pair_sweeps
    # against the C oracle's chains (fixed hyper-parameters)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.2, seed, 0)
    per_sweep = {}
    for s in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES["symmetric"], 0)
        if s >= burn:
            per_sweep[s] = R.pair_counts(f_o, r_o)
    for every in (1, 3):
        eng = engine()
        eng.attach_pair_accumulator(every)
        eng.run(0, n_sweeps, mstep_every=0, accumulate_from=burn)
        want = sum(per_sweep[s] for s in range(burn, n_sweeps, every))
        nptest.assert_array_equal(eng.pair_counts_host().astype(np.int64), want)
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        nptest.assert_array_equal(r_g, r_o)


def test_accumulator_survives_scratch_growth_inside_the_run(env):
    """
    A C-ABI caller that attaches an accumulator to a context which never saw fcd_ctx_reserve: fcd_gibbs_run grows the
    context's square f copy and workspace inside the call, and every counted sweep must still reach the buffer.
    """
    (N, H, U, G, n_sweeps, burn) = (64, 16, 16, 256, 5, 1)
    (m, S_B, lM) = tables(env, N, H, U, seed=11)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=9, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    fresh = env.lib.Context()                     # no fcd_ctx_reserve: no square f copy, no workspace yet
    n_alloc = fresh.stat("n_alloc")
    acc = env.torch.zeros((eng.C, U, 3, 3), dtype=env.torch.int32, device="cuda")
    fresh.call("fcd_gibbs_set_pair_accumulator", env.lib.dptr(acc), N, U, 1)
    lib = env.lib
    import ctypes as C
    fresh.call("fcd_gibbs_run", lib.dptr(eng.S_B), lib.dptr(eng.lM), lib.dptr(eng.lMf), lib.dptr(eng.lMd), lib.dptr(eng.hyper),
               lib.dptr(eng.f_state), lib.dptr(eng.r_bits), N, U, G, 0, C.c_uint64(9), 0, n_sweeps, lib.EDGE_SYMMETRIC, 0, burn,
               None, None, None, lib.stream_ptr())
    fresh.call("fcd_gibbs_set_pair_accumulator", None, 0, 0, 1)
    assert fresh.stat("n_alloc") > n_alloc        # (the scratch did grow inside the call)
    got = eng.host(acc).view(np.uint32).astype(np.int64)
    assert np.all(got.sum(axis=(2, 3)) == G * (n_sweeps - burn))
    # the same chains, counted sweep by sweep through fcd_gibbs_pair_counts
    ref = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=9, edge_index="symmetric", ctx=env.ctx)
    ref.set_hyper(m.gamma, m.pi2())
    ref.init(0.2)
    W = env.torch.zeros((ref.C, U, 3, 3), dtype=env.torch.float64, device="cuda")
    for s in range(n_sweeps):
        ref.run(s, 1, mstep_every=0)
        if s >= burn:
            ref.pair_counts(out=W, accumulate=True)
    nptest.assert_array_equal(got.astype(np.float64), ref.host(W))
    fresh.close()


def test_pair_tally_single_state(env):
    """fcd_gibbs_pair_tally on an imported state with a partial last chain word: NumPy counts, and it adds."""
    (N, U, G) = (9, 70, 130)
    (m, S_B, lM) = tables(env, N, 3, U, seed=5)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    rng = np.random.default_rng(0)
    f = rng.integers(0, 3, (G, N * (N - 1) // 2)).astype(np.uint8)
    r = (rng.random((G, N, U)) < 0.35).astype(np.uint8)
    eng.import_state(f, r)
    acc = env.torch.zeros((eng.C, U, 3, 3), dtype=env.torch.int32, device="cuda")
    eng.pair_tally(acc)
    eng.pair_tally(acc)
    nptest.assert_array_equal(eng.host(acc).astype(np.int64), 2 * R.pair_counts(f, r))


def exact_posterior(name):
    """(bt, theta, exact {p_T, p_F_tilde, p_changed}, ExactChain) of an exact_law_cases problem."""
    (N, U, data) = X.CASES[name]
    m = X.model(data)
    (_r, _t, _f, _ft, _b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)       # as X.problem() makes its tables
    (_N, _U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    pi = np.exp(ec.L - ec.L.max())
    pi /= pi.sum()
    (f, r) = ec.all_states()
    L = R.mix_cases(r)                                     # (S, C, U)
    p = pi.reshape(-1)
    W = np.zeros((ec.C, U, 3, 3))
    for c in range(ec.C):
        for u in range(U):
            np.add.at(W[c, u], (f[:, c], L[:, c, u]), p)
    return bt, m.theta(), R.contract(W, bt, m.theta()), ec, pi.reshape(-1)


@pytest.mark.parametrize("name", ["3x2", "4x2", "3x2-strong"])
def test_gibbs_posterior_against_exact(env, name):
    """2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: within 5 x 0.5/sqrt(G) + 1e-4."""
    from fcdiff_amd.fit import conn_posterior
    (bt, theta, want, ec, pi) = exact_posterior(name)
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
    eng.attach_pair_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.pair_sweeps == 1
    out = conn_posterior(env.ctx, up(env, bt), N, U, theta, counts=eng.pair_acc)
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%s: K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (
        name, K, max(np.abs(out[k] - want[k]).max() for k in want), tol))
    for key in want:
        nptest.assert_allclose(out[key], want[key], rtol=0, atol=tol, err_msg=key)


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


def test_fit_gibbs_connection_posterior(env):
    """The fit's counts: pooled from burn_in on, every k-th sweep, the same with an on_sweep callback; the posterior is the
    contraction of those counts with the final theta; the default-off path attaches nothing and refuses."""
    off = gibbs_fit(env)
    assert off.connection_counts is None and off.sampler.pair_acc is None
    with pytest.raises(ValueError):
        off.connection_posterior()
    on = gibbs_fit(env, connection_marginals=True)
    (f_off, r_off) = off.sampler.export_state()
    (f_on, r_on) = on.sampler.export_state()
    nptest.assert_array_equal(f_on, f_off)
    nptest.assert_array_equal(r_on, r_off)
    nptest.assert_array_equal(on._lq_F, off._lq_F)
    cnt = on.connection_counts
    assert cnt.shape == (45, 7, 3, 3) and np.all(cnt.sum(axis=(2, 3)) == 192 * 9) and on.connection_sweeps == 9
    out = on.connection_posterior()
    check_outputs(out, R.contract(cnt, on.bt, on.model.theta()))
    thin = gibbs_fit(env, connection_marginals=True, connection_every=4)
    assert np.all(thin.connection_counts.sum(axis=(2, 3)) == 192 * 3) and thin.connection_sweeps == 3   # sweeps 3, 7, 11
    cb = gibbs_fit(env, connection_marginals=True, connection_every=4, energy_every=1)
    nptest.assert_array_equal(cb.connection_counts, thin.connection_counts)
    early = gibbs_fit(env, connection_marginals=True, n_sweeps=3)
    with pytest.raises(ValueError):
        early.connection_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(env, connection_marginals=True, connection_every=0)
