"""
Co-anomaly on the MI355X: the pair-count kernel (fcd_gibbs_coanomaly_tally) and the accumulator of fcd_gibbs_run
(fcd_gibbs_set_coanomaly_accumulator) against the NumPy restatement of tests/coanomaly_ref.py, the C oracle's chains, the
other accumulators of the same run and the exact posterior of small models; the independence form of the variational fit
(fcd_vb_coanomaly); and coanomaly_posterior() of both fits end to end.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest

import coanomaly_ref as R
import exact_law_cases as X
from oracle.exact_chain import ExactChain

pytestmark = pytest.mark.gpu

TILE, CHUNK = 32, 64        # fcd_coanomaly.hip: outputs per tile side, terms per staged chunk


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine, pair_sweeps_in
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO, e.pair_sweeps_in = torch, fcdiff_amd, _lib, GibbsEngine, CO, pair_sweeps_in
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def tables(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


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


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


SINGLE = ([(9, 5, G) for G in (1, 63, 64, 65, 130, 1024)]
          + [(7, 1, 130), (40, 1, 64), (6, 65, 70), (2, 3, 100), (2, 1, 1)]
          + [(N, U, 130) for (N, U) in ((TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1),
                                        (CHUNK - 1, CHUNK + 1), (CHUNK, CHUNK), (CHUNK + 1, CHUNK - 1),
                                        (2 * TILE + 1, 2 * CHUNK + 1))]
          + [(200, 50, 1024), (400, 250, 192)])


@pytest.mark.parametrize("N,U,G", SINGLE)
def test_coanomaly_tally_single_state(env, N, U, G):
    """fcd_gibbs_coanomaly_tally on an imported state: the NumPy matrices integer for integer, and it adds.  The bits of
    the chains beyond G in the last word are set on purpose: they must not be counted."""
    rng = np.random.default_rng(1000 * G + 10 * N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    r_bits = import_r_bits(env, r)
    if G % 64:
        r_bits[G // 64] |= ~((1 << (G % 64)) - 1)
    rp = env.torch.zeros((N, N), dtype=env.torch.int32, device="cuda")
    pp = env.torch.zeros((U, U), dtype=env.torch.int32, device="cuda")
    (want_r, want_p) = R.pair_counts(r)
    for k in (1, 2):
        env.ctx.call("fcd_gibbs_coanomaly_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(rp), env.lib.dptr(pp),
                     env.lib.stream_ptr())
        nptest.assert_array_equal(u32(rp), k * want_r)
        nptest.assert_array_equal(u32(pp), k * want_p)


def test_engine_tally_checks_its_matrices(env):
    (N, U, G) = (6, 4, 70)
    (m, S_B, lM) = tables(env, N, 3, U, seed=2)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.init(0.4)
    t = env.torch
    (rp, pp) = (t.zeros((N, N), dtype=t.int32, device="cuda"), t.zeros((U, U), dtype=t.int32, device="cuda"))
    eng.coanomaly_tally(rp, pp)
    (_f, r) = eng.export_state()
    (want_r, want_p) = R.pair_counts(r)
    nptest.assert_array_equal(u32(rp), want_r)
    nptest.assert_array_equal(u32(pp), want_p)
    with pytest.raises(ValueError):
        eng.coanomaly_tally(pp, rp)
    with pytest.raises(ValueError):
        eng.coanomaly_tally(rp.to(t.int64), pp)


@pytest.mark.parametrize("N,H,U,G,n_sweeps,burn", [(64, 16, 16, 256, 9, 2), (200, 50, 50, 1024, 5, 1)],
                         ids=["cfg2", "cfg3"])
def test_accumulator_is_exact(env, N, H, U, G, n_sweeps, burn):
    """
    fcd_gibbs_run with the accumulator, every = 1 / 3, alone and beside the pair and count accumulators: equal, integer
    for integer, to the NumPy matrices of the C oracle's chains over the same sweeps.  The sampler is untouched: chain
    state and hyper-parameters bit-identical to a run without it.  With every = 1 the diagonals are the marginal
    counters' sums and the totals the second moments of the count histograms of the same run.
    """
    (m, S_B, lM) = tables(env, N, H, U, seed=N + U)
    (S_B_d, lM_d) = (up(env, S_B), up(env, lM))
    seed = 404

    def engine():
        e = env.GibbsEngine(S_B_d, lM_d, N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.2)
        return e
    plain = engine()
    plain.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
    (f0, r0) = plain.export_state()
    h0 = plain.hyper_values()
    for (every, with_others) in ((1, False), (3, True), (1, True)):
        acc = engine()
        acc.attach_coanomaly_accumulator(every)
        if with_others:
            acc.attach_pair_accumulator(2)
            acc.attach_count_accumulator(1)
        acc.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        (rp, pp) = (a.astype(np.int64) for a in acc.coanomaly_host())
        (f1, r1) = acc.export_state()
        nptest.assert_array_equal(f1, f0)
        nptest.assert_array_equal(r1, r0)
        (g1, p1) = acc.hyper_values()
        assert np.array_equal(g1, h0[0]) and p1 == h0[1]
        assert acc.coanomaly_sweeps == len(range(burn, n_sweeps, every))
        assert rp.shape == (N, N) and pp.shape == (U, U)
        assert np.array_equal(rp, rp.T) and np.array_equal(pp, pp.T)
        assert np.trace(rp) == np.trace(pp)
        if every == 1:
            cnt_r = acc.host(acc.cnt_r).astype(np.int64)
            nptest.assert_array_equal(np.diag(rp), cnt_r.sum(axis=1))
            nptest.assert_array_equal(np.diag(pp), cnt_r.sum(axis=0))
        if with_others:
            assert acc.pair_sweeps == len(range(burn, n_sweeps, 2))
            assert int(acc.pair_counts_host()[0, 0].sum()) == G * acc.pair_sweeps
            (hp, hr) = (h.astype(np.int64) for h in acc.count_hist_host())
            assert np.all(hp.sum(axis=1) == G * acc.count_sweeps)
            if every == 1:
                assert rp.sum() == int((hp * np.arange(N + 1) ** 2).sum())
                assert pp.sum() == int((hr * np.arange(U + 1) ** 2).sum())
    # against the C oracle's chains (fixed hyper-parameters)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.2, seed, 0)
    per_sweep = {}
    for s in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES["symmetric"], 0)
        if s >= burn:
            per_sweep[s] = R.pair_counts(r_o)
    for every in (1, 3):
        eng = engine()
        eng.attach_coanomaly_accumulator(every)
        eng.run(0, n_sweeps, mstep_every=0, accumulate_from=burn)
        (rp, pp) = eng.coanomaly_host()
        nptest.assert_array_equal(rp.astype(np.int64), sum(per_sweep[s][0] for s in range(burn, n_sweeps, every)))
        nptest.assert_array_equal(pp.astype(np.int64), sum(per_sweep[s][1] for s in range(burn, n_sweeps, every)))
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        nptest.assert_array_equal(r_g, r_o)


@pytest.mark.parametrize("name", ["3x2", "4x2", "3x2-strong"])
def test_gibbs_coanomaly_against_exact(env, name):
    """2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: p_region_pair and p_patient_pair within
    5 x 0.5/sqrt(G) + 1e-4 of the enumerated values (each entry is an average of Bernoulli frequencies).  In
    "3x2-strong" the exact joint lies further than that from the independence form (tests/test_coanomaly.py)."""
    from fcdiff_amd.fit import coanomaly_from_counts
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    (want_r, want_p, _q1) = R.exact_moments(ec)
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (P, K) = (ec.initial(X.PI0), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    G = X.G_CHAINS
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    eng.attach_coanomaly_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.coanomaly_sweeps == 1
    (rp, pp) = eng.coanomaly_host()
    got = coanomaly_from_counts(rp, pp, G)
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%s: K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (
        name, K, max(np.abs(got["p_region_pair"] - want_r).max(), np.abs(got["p_patient_pair"] - want_p).max()), tol))
    nptest.assert_allclose(got["p_region_pair"], want_r, rtol=0, atol=tol)
    nptest.assert_allclose(got["p_patient_pair"], want_p, rtol=0, atol=tol)


@pytest.mark.parametrize("N,U", [(7, 13), (2, 1), (200, 50), (400, 250)])
def test_vb_coanomaly_kernel_against_numpy(env, N, U):
    """fcd_vb_coanomaly: NumPy at rtol 1e-12 (non-negative terms: U or Nreg roundings bound the error), lq_R
    unnormalised, q = 0 / 1 exact, symmetric, bitwise repeatable."""
    from fcdiff_amd.fit import coanomaly_independent
    rng = np.random.default_rng(N * 1000 + U)
    q1 = rng.uniform(0, 1, (N, U))
    q1[rng.random((N, U)) < 0.1] = 0.0
    q1[rng.random((N, U)) < 0.1] = 1.0
    q1[0, :] = 1.0                                   # region 0 anomalous in every patient
    q1[1, :] = 0.0                                   # region 1 in none
    with np.errstate(divide="ignore"):
        lq_R = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))      # not normalised
    lq_dev = up(env, lq_R)
    (reg, pat) = coanomaly_independent(env.ctx, lq_dev, N, U)
    (want_r, want_p) = R.independent(lq_R)
    nptest.assert_allclose(reg, want_r, rtol=1e-12, atol=0)
    nptest.assert_allclose(pat, want_p, rtol=1e-12, atol=0)
    assert reg[0, 0] == float(U) and np.all(reg[1, :] == 0.0) and np.all(reg[:, 1] == 0.0)
    assert np.array_equal(reg, reg.T) and np.array_equal(pat, pat.T)
    (reg2, pat2) = coanomaly_independent(env.ctx, lq_dev, N, U)
    assert np.array_equal(reg, reg2) and np.array_equal(pat, pat2)


def gibbs_fit(env, bt_nan=False, **kw):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(10, 6, 7, seed=8)
    if bt_nan:
        bt = bt.copy()
        bt[::5, 1] = np.nan
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed = "gibbs", 192, 12, 3, 5
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit


def check_fit_dict(env, fit, N, U, G, n_acc):
    (rp, pp) = (a.astype(np.int64) for a in fit.sampler.coanomaly_host())
    nptest.assert_array_equal(fit.region_pair_counts, rp)
    nptest.assert_array_equal(fit.patient_pair_counts, pp)
    assert fit.region_pair_counts.dtype == np.int64 and fit.patient_pair_counts.dtype == np.int64
    assert fit.region_pair_counts.shape == (N, N) and fit.patient_pair_counts.shape == (U, U)
    assert fit.coanomaly_sweeps == n_acc and fit.coanomaly_states == n_acc * G
    out = fit.coanomaly_posterior()
    assert sorted(out) == ["expected_patients", "expected_regions", "p_patient_pair", "p_patient_pair_independent",
                           "p_region_pair", "p_region_pair_independent"]
    want = R.posterior_from_counts(rp, pp, n_acc * G)
    for k in want:
        assert out[k].dtype == np.float64
        nptest.assert_allclose(out[k], want[k], rtol=1e-15)
    (ind_r, ind_p) = R.independent(fit._lq_R)
    nptest.assert_allclose(out["p_region_pair_independent"], ind_r / U, rtol=1e-12)
    nptest.assert_allclose(out["p_patient_pair_independent"], ind_p / N, rtol=1e-12)
    return out


def test_fit_gibbs_coanomaly(env):
    """The fit's pair counts: from burn_in on, every second sweep; the engine's own; the dict follows from them; the
    sampler and the marginals are untouched; the default-off path attaches nothing and refuses."""
    off = gibbs_fit(env)
    assert off.region_pair_counts is None and off.sampler.coanomaly_acc is None
    with pytest.raises(ValueError):
        off.coanomaly_posterior()
    on = gibbs_fit(env, coanomaly=True, coanomaly_every=2)
    (f_off, r_off) = off.sampler.export_state()
    (f_on, r_on) = on.sampler.export_state()
    nptest.assert_array_equal(f_on, f_off)
    nptest.assert_array_equal(r_on, r_off)
    nptest.assert_array_equal(on._lq_F, off._lq_F)
    nptest.assert_array_equal(on._lq_R, off._lq_R)
    n_acc = env.pair_sweeps_in(0, 12, 3, 2)
    assert n_acc == 5                                          # sweeps 3, 5, 7, 9, 11
    check_fit_dict(env, on, 10, 7, 192, n_acc)
    # every sweep counted: the diagonals are the means of the marginals of _lq_R
    full = gibbs_fit(env, coanomaly=True, anomaly_counts=True, connection_marginals=True, energy_every=1)
    out = check_fit_dict(env, full, 10, 7, 192, 9)
    p1 = np.exp(full._lq_R[:, :, 1])
    nptest.assert_allclose(np.diag(out["p_region_pair"]), p1.mean(axis=1), rtol=1e-12)
    nptest.assert_allclose(np.diag(out["p_patient_pair"]), p1.mean(axis=0), rtol=1e-12)
    early = gibbs_fit(env, coanomaly=True, n_sweeps=3)
    with pytest.raises(ValueError):
        early.coanomaly_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(env, coanomaly=True, coanomaly_every=0)


def test_fit_gibbs_coanomaly_with_missing_data(env):
    fit = gibbs_fit(env, bt_nan=True, missing_data=True, coanomaly=True, coanomaly_every=2, n_chains=130, n_sweeps=8,
                    burn_in=2)
    check_fit_dict(env, fit, 10, 7, 130, 3)                    # sweeps 2, 4, 6


@pytest.mark.parametrize("edge_index", ["reference", "symmetric"])
def test_vb_coanomaly_posterior(env, edge_index):
    """Under the mean field the joint entries are the independent ones."""
    m = env.pkg.UnsharedRegionModel()
    (N, U) = (12, 9)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 6, U, seed=4)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.max_iters, fit.edge_index = env.pkg.UnsharedRegionModel(), b, bt, 3, edge_index
    fit.run()
    out = fit.coanomaly_posterior()
    (ind_r, ind_p) = R.independent(fit._lq_R)
    nptest.assert_allclose(out["p_region_pair"], ind_r / U, rtol=1e-12)
    nptest.assert_allclose(out["expected_patients"], ind_r, rtol=1e-12)
    nptest.assert_allclose(out["p_patient_pair"], ind_p / N, rtol=1e-12)
    nptest.assert_allclose(out["expected_regions"], ind_p, rtol=1e-12)
    assert np.array_equal(out["p_region_pair"], out["p_region_pair_independent"])
    assert np.array_equal(out["p_patient_pair"], out["p_patient_pair_independent"])
    assert out["p_region_pair"].shape == (N, N) and out["p_patient_pair"].shape == (U, U)


@pytest.mark.parametrize("method", ["vb", "gibbs"])
def test_shared_fit_coanomaly(env, method):
    m = env.pkg.SharedRegionModel()
    (N, U) = (8, 5)
    (_r, _t, _f, _ft, b, bt) = m.sample(N, 4, U, seed=3)
    fit = env.pkg.fit.SharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt, fit.method) = (env.pkg.SharedRegionModel(), b, bt, method)
    if method == "gibbs":
        (fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed, fit.coanomaly) = (192, 10, 2, 5, True)
    else:
        fit.max_iters = 3
    fit.run()
    out = fit.coanomaly_posterior()
    assert sorted(out) == ["p_region_pair", "p_region_pair_independent"]
    (joint, ind) = (out["p_region_pair"], out["p_region_pair_independent"])
    assert joint.shape == (N, N) and ind.shape == (N, N) and joint.dtype == np.float64
    p = fit.region_posterior()
    nptest.assert_allclose(np.diag(joint), p, rtol=1e-12)
    nptest.assert_allclose(np.diag(ind), p, rtol=1e-12)
    want = np.outer(p, p)
    np.fill_diagonal(want, p)
    nptest.assert_allclose(ind, want, rtol=1e-12)
    if method == "vb":
        assert np.array_equal(joint, ind)
    else:
        assert fit.patient_pair_counts.shape == (1, 1) and fit.coanomaly_sweeps == 8
        nptest.assert_allclose(joint, fit.region_pair_counts / float(192 * 8), rtol=1e-15)
        assert np.all(joint <= np.minimum.outer(np.diag(joint), np.diag(joint)) + 1e-15)


def test_refusals_with_a_context(env):
    """The checks that come before any device work, on a live context; another shape while attached; overflow."""
    (lib, ctx, E) = (env.lib.load(), env.ctx.handle, env.lib)
    fake = C.c_void_p(16)          # never dereferenced: every call below is refused on the host
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, fake, None, 4, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, None, fake, 4, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, fake, fake, 1, 2, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, fake, fake, 4, 0, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, fake, fake, 4, 2, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_coanomaly_accumulator(ctx, None, None, 0, 0, 1) == 0
    assert lib.fcd_gibbs_coanomaly_tally(ctx, None, 4, 2, 64, fake, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_coanomaly_tally(ctx, fake, 4, 2, 64, fake, None, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_coanomaly_tally(ctx, fake, 4, 2, 0, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_coanomaly_tally(ctx, fake, 1, 2, 64, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_vb_coanomaly(ctx, fake, 0, 2, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_vb_coanomaly(ctx, fake, 4, 2, None, fake, None) == E.FCD_ERR_ARG
    # fcd_gibbs_run refuses another shape while attached, before any launch
    (N, U, G) = (12, 5, 64)
    (m, S_B, lM) = tables(env, N, 3, U, seed=3)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    rp = env.torch.zeros((N + 1, N + 1), dtype=env.torch.int32, device="cuda")
    pp = env.torch.zeros((U + 1, U + 1), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_set_coanomaly_accumulator", env.lib.dptr(rp), env.lib.dptr(pp), N + 1, U + 1, 1)
    try:
        with pytest.raises(ValueError, match="co-anomaly accumulator was made for"):        # (FCD_ERR_SHAPE)
            eng._run(0, 1, 0, 0, False)
    finally:
        env.ctx.call("fcd_gibbs_set_coanomaly_accumulator", None, None, 0, 0, 1)
    assert int(rp.abs().sum()) == 0 and int(pp.abs().sum()) == 0
    (f0, r0) = eng.export_state()
    # overflow is refused before any launch: the state does not move, nothing is added
    with pytest.raises(ValueError):
        eng.attach_coanomaly_accumulator(0)
    eng.attach_coanomaly_accumulator(1)
    eng.coanomaly_sweeps = (1 << 32) // (G * N)
    with pytest.raises(ValueError):
        eng.run(0, 1, accumulate_from=0)
    (f1, r1) = eng.export_state()
    nptest.assert_array_equal(f1, f0)
    nptest.assert_array_equal(r1, r0)
    assert all(int(a.sum()) == 0 for a in eng.coanomaly_host())


def test_each_accumulator_alone_equals_all_together(env):
    """
    The three accumulators of fcd_gibbs_run at periods 1 (pair), 2 (count) and 3 (co-anomaly), so that each counts other
    sweeps: every buffer of a run with all three attached equals, bit for bit, that of a run from the same seed with this
    one attached alone, and the sweep counters are pair_sweeps_in's.  Nreg = 6, U = 3, G = 130: three chain words, two
    live lanes in the last.  fcd_gibbs_sweeps adds nothing, whatever is attached to the context.
    """
    from fcdiff_amd.gibbs import ACCUMULATORS
    (N, U, G, n_sweeps, burn) = (6, 3, 130, 7, 2)
    every = {"pair": 1, "count": 2, "coanomaly": 3}
    ACCUMULATORS = [a for a in ACCUMULATORS if a.key in every]
    (m, S_B, lM) = tables(env, N, 4, U, seed=11)
    (S_B_d, lM_d) = (up(env, S_B), up(env, lM))

    def run(keys):
        e = env.GibbsEngine(S_B_d, lM_d, N, U, G, chain0=0, seed=77, edge_index="symmetric", ctx=env.ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.3)
        for k in keys:
            getattr(e, "attach_%s_accumulator" % k)(every[k])
        e.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        return e

    def buffers(e, k):
        got = {"pair": e.pair_counts_host, "count": e.count_hist_host, "coanomaly": e.coanomaly_host}[k]()
        return got if isinstance(got, tuple) else (got,)
    together = run(["pair", "count", "coanomaly"])
    assert (together.pair_sweeps, together.count_sweeps, together.coanomaly_sweeps) == (5, 3, 2)
    for a in ACCUMULATORS:
        alone = run([a.key])
        assert [getattr(alone, b.attr) is not None for b in ACCUMULATORS] == [b is a for b in ACCUMULATORS]
        want = env.pair_sweeps_in(0, n_sweeps, burn, every[a.key])
        assert getattr(alone, a.key + "_sweeps") == getattr(together, a.key + "_sweeps") == want
        (one, all3) = (buffers(alone, a.key), buffers(together, a.key))
        assert [tuple(x.shape) for x in one] == [tuple(s) for s in a.shapes(alone)]
        for (x, y) in zip(one, all3):
            nptest.assert_array_equal(x, y)
    assert int(together.pair_counts_host()[0, 0].sum()) == G * 5
    assert np.all(together.count_hist_host()[0].astype(np.int64).sum(axis=1) == G * 3)
    (rp, pp) = (x.astype(np.int64) for x in together.coanomaly_host())
    assert np.trace(rp) == np.trace(pp) and np.array_equal(rp, rp.T)
    # fcd_gibbs_sweeps with all three attached to the context: it is not their caller
    t = env.torch
    raw = [[t.zeros(shape, dtype=t.int32, device="cuda") for shape in a.shapes(together)] for a in ACCUMULATORS]
    try:
        for (a, bufs) in zip(ACCUMULATORS, raw):
            env.ctx.call(a.setter, *([env.lib.dptr(b) for b in bufs] + [N, U, 1]))
        together.sweeps(7, 2)
        assert all(int(b.abs().sum()) == 0 for bufs in raw for b in bufs)
    finally:
        for (a, bufs) in zip(ACCUMULATORS, raw):
            env.ctx.call(a.setter, *([None] * len(bufs) + [0, 0, 1]))
    for (x, y) in zip(buffers(together, "coanomaly"), (rp, pp)):
        nptest.assert_array_equal(x.astype(np.int64), y)
