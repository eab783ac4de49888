"""
Scoring new patients on the device (UnsharedRegionFit.score, fcd_score.hip): the per-patient ELBO kernel against the
NumPy reference and the fit's energy, the variational fixed point on the fit's own patients, the annealed importance
sampler against the exact predictive likelihood and the exact posterior of r of tiny models, unobserved patients, and a
fit left exactly as it was.
"""
import math

import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
import score_ref as R
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, score
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.score = torch, fcdiff_amd, _lib, score
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def random_logs(rng, shape):
    a = rng.normal(size=shape) * 1.5
    return a - np.log(np.sum(np.exp(a), axis=-1, keepdims=True))


def device_tables(env, m, b, bt, missing):
    (S_B, lM) = env.score.lik_tables(env.ctx, up(env, b), up(env, bt), m.theta(), missing)
    return lM


@pytest.mark.parametrize("N,U,missing", [(3, 2, False), (3, 2, True), (8, 1, False), (9, 65, True), (200, 3, False),
                                         (200, 2, True), (30, 130, False)])
def test_patient_elbo_kernel(env, N, U, missing):
    """fcd_vb_patient_elbo against score_ref at 1e-10 relative, with and without NaN, bitwise equal over two calls."""
    rng = np.random.default_rng(N * 1000 + U)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 4, U, seed=N + U)
    if missing:
        bt = np.where(rng.random(bt.shape) < 0.2, np.nan, bt)
    lM_d = device_tables(env, m, b, bt, missing)
    C = N * (N - 1) // 2
    lq_F = random_logs(rng, (C, 1, 3))
    lq_R = random_logs(rng, (N, U, 2))
    hyper = env.score.hyper_block(env.ctx, m.gamma, m.pi2(), "cuda")
    got = env.score.patient_elbo(env.ctx, up(env, lq_F), up(env, lq_R), lM_d, hyper, N, U)
    again = env.score.patient_elbo(env.ctx, up(env, lq_F), up(env, lq_R), lM_d, hyper, N, U)
    assert got.tobytes() == again.tobytes()
    want = R.patient_elbo(lq_F, lq_R, lM_d.cpu().numpy(), m.pi2())
    nptest.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * np.max(np.abs(want)))


def vb_fit(env, N, H, U, seed, **kw):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(N, H, U, seed=seed)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit, gen


def test_patient_elbo_sums_to_the_energy(env):
    """On the fit's own patients the per-patient terms add up to the energy's E_lM, E_lp_R and E_lq_R."""
    (fit, _gen) = vb_fit(env, 12, 6, 9, seed=3, max_iters=3)
    (N, C, U) = fit._check_state()
    hyper = env.score.hyper_block(env.ctx, fit.model.gamma, fit._pi2(), "cuda")
    got = env.score.patient_elbo(env.ctx, fit._d["lq_F"], fit._d["lq_R"], fit._d["lM"], hyper, N, U)
    terms = fit._energy_terms()
    nptest.assert_allclose(got[:, 0].sum(), terms[3], rtol=1e-10)
    nptest.assert_allclose(got[:, 1].sum(), terms[2], rtol=1e-10)
    nptest.assert_allclose(got[:, 2].sum(), terms[5], rtol=1e-10)
    nptest.assert_allclose(got[:, 3].sum(), terms[3] + terms[2] - terms[5], rtol=1e-10)


@pytest.mark.parametrize("edge_index", ["reference", "symmetric"])
def test_vb_score_reproduces_the_fit(env, edge_index):
    """A converged VB fit: scoring its own patients gives back exp(_lq_R)[..., 1].  (rel_tol = -inf: the fit's convergence
    test stops a fit of negative energy at its first decrease -- quirk Q6 -- so it runs all max_iters iterations.)"""
    (fit, _gen) = vb_fit(env, 20, 10, 8, seed=11, max_iters=300, rel_tol=-np.inf, edge_index=edge_index)
    assert len(fit.energy) == 301 and abs(fit.energy[-1] - fit.energy[-2]) <= 1e-12 * abs(fit.energy[-1])
    out = fit.score(fit.bt, max_iters=1000, tol=1e-13)
    nptest.assert_allclose(out["p_R"], np.exp(fit._lq_R[:, :, 1]), atol=1e-6)
    assert out["elbo"].shape == (8,) and np.all(np.isfinite(out["elbo"]))
    assert out["iters"].shape == (8,) and np.all((out["iters"] >= 1) & (out["iters"] <= 1000))
    assert out["converged"].dtype == bool and np.all(out["converged"] == (out["iters"] < 1000))
    nptest.assert_allclose(out["p_patient_count"].sum(axis=1), 1.0, rtol=1e-12)
    nptest.assert_allclose(out["p_patient_any"], 1.0 - out["p_patient_count"][:, 0], rtol=1e-15)


def test_vb_score_patients_are_independent(env):
    """Scoring columns [A, B] together gives, bit for bit, what scoring A and B apart gives: each patient stops on its own
    convergence (default tol), and with tol = 0 all run the same max_iters."""
    (fit, gen) = vb_fit(env, 14, 8, 6, seed=21, max_iters=5, missing_data=True)
    (_r, _t, _f, _ft, _b, bt_new) = gen.sample_fast(14, 8, 5, seed=99)
    bt_new[:, 0] = np.nan         # an unobserved patient: q_R = pi after one update, so it stops at the second
    (A, B) = (bt_new[:, :2], bt_new[:, 2:])
    for kw in (dict(connections=True), dict(max_iters=30, tol=0.0, connections=True)):
        both = fit.score(bt_new, **kw)
        (a, b) = (fit.score(A, **kw), fit.score(B, **kw))
        for key in ("elbo", "p_patient_any", "p_patient_count", "iters", "converged"):
            nptest.assert_array_equal(both[key], np.concatenate([a[key], b[key]]))
        for key in ("p_R", "p_T", "p_F_tilde", "p_changed"):
            nptest.assert_array_equal(both[key], np.concatenate([a[key], b[key]], axis=1))
    out = fit.score(bt_new)
    assert out["iters"][0] == 2 and out["converged"][0]


def gibbs_fit(env, N, U, G, data="broad", seed=5, **kw):
    m = X.model(data)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt = X.model(data), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed, fit.mstep_every = "gibbs", G, 4, 1, seed, 0
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit, m


def exact_lM(fit, bt_new):
    th = fit.model
    return O.lik_tables(np.asarray(fit.b), bt_new, th.mu, th.sigma, th.eta, th.epsilon)[2]


@pytest.mark.parametrize("N,U", [(3, 2), (4, 3)])
def test_gibbs_ais_against_exact(env, N, U):
    """
    Every chain holding one known f, then a handful of distinct f rows over the chains: log_pred within 4 standard errors
    (+ 1e-3) of log mean_g p(bt_u | f_g) enumerated over r; with n_sweeps = 1 every chain gives one draw of r, and each
    site's count passes a two-sided binomial test at 1e-6 against the enumerated P(r_nu = 1 | f, bt).
    """
    from scipy.stats import binomtest
    G = 4096
    (fit, m) = gibbs_fit(env, N, 2, G)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(N, 2, U, seed=77 + N)
    lM = exact_lM(fit, bt_new)
    pi = float(fit._pi2()[1])
    C = N * (N - 1) // 2
    rng = np.random.default_rng(N)
    f_one = rng.integers(0, 3, size=C)
    f_rows = rng.integers(0, 3, size=(5, C))
    r0 = np.zeros((G, N, 2), dtype=np.uint8)
    for (label, rows) in (("one", f_one[None, :]), ("rows", f_rows)):
        idx = np.arange(G) % len(rows)
        fit.sampler.import_state(rows[idx], r0)
        env.torch.cuda.synchronize()      # (import_state's host-made inputs are temporaries: let the import finish first)
        out = fit.score(bt_new, n_anneal=200, n_sweeps=1, seed=31)
        cnt = np.bincount(idx, minlength=len(rows)).astype(np.float64)
        for u in range(U):
            per_f = np.array([R.exact_log_pred(lM[:, u], f, pi) for f in rows])
            mx = per_f.max()
            exact = mx + math.log(np.sum(cnt * np.exp(per_f - mx)) / G)      # log mean over the chains' f
            assert abs(out["log_pred"][u] - exact) <= 4 * out["log_pred_se"][u] + 1e-3, (label, u, out["log_pred"][u], exact)
            assert 0 < out["ess"][u] <= G
        if label == "one":
            for u in range(U):
                p = R.exact_p_r(lM[:, u], f_one, pi)
                for n in range(N):
                    k = int(round(out["p_R"][n, u] * G))
                    assert binomtest(k, G, float(p[n])).pvalue > 1e-6, (n, u, k / G, p[n])


def test_unobserved_patient(env):
    """A patient whose bt is all NaN under missing_data: VB p_R = pi and elbo = 0; Gibbs log_pred = 0 exactly."""
    (fit, gen) = vb_fit(env, 10, 6, 5, seed=2, max_iters=4, missing_data=True)
    (_r, _t, _f, _ft, _b, bt_new) = gen.sample_fast(10, 6, 3, seed=8)
    bt_new[:, 1] = np.nan
    out = fit.score(bt_new)
    nptest.assert_allclose(out["p_R"][:, 1], fit._pi2()[1], rtol=1e-12)
    assert abs(out["elbo"][1]) <= 1e-12
    (gfit, m) = gibbs_fit(env, 6, 3, 256, missing_data=True)
    (_r, _t, _f, _ft, _b, bt_g) = m.sample_fast(6, 2, 2, seed=4)
    bt_g[:, 0] = np.nan
    g = gfit.score(bt_g, n_anneal=20, n_sweeps=3)
    assert g["log_pred"][0] == 0.0 and g["ess"][0] == 256.0 and g["log_pred_se"][0] == 0.0
    assert np.isfinite(g["log_pred"][1])


def snapshot(fit):
    f, r = (fit.sampler.export_state() if fit.sampler is not None else (None, None))
    return {"theta": np.asarray(fit.model.theta()).tobytes(), "lq_R": fit._lq_R.tobytes(), "lq_F": fit._lq_F.tobytes(),
            "energy": np.asarray(fit.energy).tobytes(), "lM": fit._lM.tobytes(),
            "S_B": fit._d["S_B"].cpu().numpy().tobytes(), "f": None if f is None else f.tobytes(),
            "r": None if r is None else r.tobytes()}


def test_score_leaves_the_fit_alone(env):
    """model, _lq_R, _lq_F, energy, the tables and the sampler's state byte-identical after score(); ten more sweeps give
    the state of a twin fit that never scored."""
    (fit, m) = gibbs_fit(env, 8, 4, 320, anomaly_counts=True, connection_marginals=True, energy_every=1)
    (twin, _m) = gibbs_fit(env, 8, 4, 320, anomaly_counts=True, connection_marginals=True, energy_every=1)
    before = snapshot(fit)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(8, 2, 3, seed=12)
    fit.score(bt_new, connections=True, n_anneal=10, n_sweeps=4)
    fit.score(bt_new, n_anneal=5, n_sweeps=2, seed=3)
    assert snapshot(fit) == before
    for e in (fit.sampler, twin.sampler):
        e.run(fit.n_sweeps, 10, mstep_every=0)
    (f1, r1) = fit.sampler.export_state()
    (f2, r2) = twin.sampler.export_state()
    nptest.assert_array_equal(f1, f2)
    nptest.assert_array_equal(r1, r2)
    (vfit, gen) = vb_fit(env, 9, 5, 4, seed=6, max_iters=3)
    before = snapshot(vfit)
    vfit.score(gen.sample_fast(9, 5, 2, seed=1)[5], connections=True)
    assert snapshot(vfit) == before


def test_connections_and_count_laws(env):
    """connections=True: the outputs are conn_posterior() of the scoring weights (VB) or counts (Gibbs); count laws are
    normalised."""
    from fcdiff_amd.fit import conn_posterior
    (fit, gen) = vb_fit(env, 10, 6, 5, seed=13, max_iters=4)
    (_r, _t, _f, _ft, _b, bt_new) = gen.sample_fast(10, 6, 3, seed=14)
    out = fit.score(bt_new, connections=True)
    p = out["p_R"]
    lq_R = np.log(np.stack([1.0 - p, p], axis=2))
    want = conn_posterior(env.ctx, up(env, bt_new), 10, 3, fit.model.theta(), lq_F=fit._d["lq_F"], lq_R=up(env, lq_R))
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(out[key], want[key], rtol=1e-9, atol=1e-12)
    nptest.assert_allclose(out["p_patient_count"].sum(axis=1), 1.0, rtol=1e-12)
    (gfit, m) = gibbs_fit(env, 7, 3, 192)
    (_r, _t, _f, _ft, _b, bt_g) = m.sample_fast(7, 2, 4, seed=15)
    g = gfit.score(bt_g, connections=True, n_anneal=8, n_sweeps=5)
    cnt = g["connection_counts"]
    assert cnt.shape == (21, 4, 3, 3) and np.all(cnt.sum(axis=(2, 3)) == 192 * 5)
    counts = env.torch.as_tensor(np.ascontiguousarray(cnt.astype(np.uint32).view(np.int32)), device="cuda")
    want = conn_posterior(env.ctx, up(env, bt_g), 7, 4, gfit.model.theta(), counts=counts)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_array_equal(g[key], want[key])
    nptest.assert_allclose(g["p_patient_count"].sum(axis=1), 1.0, rtol=1e-12)
    assert g["p_R"].shape == (7, 4) and np.all((g["p_R"] >= 0) & (g["p_R"] <= 1))


def test_refusals(env):
    (fit, gen) = vb_fit(env, 6, 4, 3, seed=1, max_iters=2)
    with pytest.raises(ValueError):
        fit.score(np.zeros((14, 1)))                          # C does not match
    with pytest.raises(ValueError):
        fit.score(np.zeros((15, 513)))                        # beyond COUNT_MAX_U
    (gfit, _m) = gibbs_fit(env, 5, 2, 64)
    gfit.edge_index = "reference"
    with pytest.raises(ValueError):
        gfit.score(np.zeros((10, 1)))
    gfit.edge_index = None
    with pytest.raises(ValueError):
        gfit.score(np.zeros((10, 1)), n_sweeps=(1 << 32) // 64 + 1)      # tallies would overflow


def ais_step_ref(lM, f, r):
    """l[g, u] = sum_c lM[c, u, f[g, c], l(r[g, n_c, u], r[g, m_c, u])] (true endpoints of c), edges in chunks."""
    (G, C) = f.shape
    U = lM.shape[1]
    (n, m) = np.tril_indices(r.shape[1], -1)          # c = n(n-1)/2 + m, n > m: the fitter's edge order
    out = np.zeros((G, U))
    for c0 in range(0, C, 512):
        cs = np.arange(c0, min(C, c0 + 512))
        a = r[:, n[cs], :].astype(bool)
        b = r[:, m[cs], :].astype(bool)
        l = np.where(a & b, 1, np.where(a ^ b, 2, 0))
        k = np.broadcast_to(f[:, cs, None], l.shape)
        out += lM[cs[None, :, None], np.arange(U)[None, None, :], k, l].sum(axis=1)
    return out


# (N, U', G): one tile per slice, PT = 2 (N = 200, U' = 20); several tiles per slice and many slices, PT = 1, G not a
# multiple of 64 (N = 200, U' = 1, G = 4000: 33 slices of ~600 edges on 256 CUs); PT = 4 (U' = 40); PT = 8 (U' = 100); two patient
# groups (U' = 130); the smallest shape
@pytest.mark.parametrize("N,U,G", [(200, 20, 200), (200, 1, 4000), (60, 40, 300), (40, 100, 130), (30, 130, 70), (3, 2, 5)])
def test_ais_step_kernel(env, N, U, G):
    """
    One fcd_score_ais_step on random f and r: w += (beta - beta_prev) l_gu against the NumPy sum (1e-12 relative to the
    sum of |terms|), lM_beta = beta * lM bit for bit, w bitwise repeatable from the same start.
    """
    torch = env.torch
    rng = np.random.default_rng(N * 7 + U + G)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 4, U, seed=N + 3 * U)
    lM_d = device_tables(env, m, b, bt, False)
    lM = lM_d.cpu().numpy()
    C = N * (N - 1) // 2
    GW = (G + 63) // 64
    f = rng.integers(0, 3, size=(G, C)).astype(np.uint8)
    r = (rng.random((G, N, U)) < 0.4).astype(np.uint8)
    f_state = torch.zeros((GW, C, 64), dtype=torch.uint8, device="cuda")
    r_bits = torch.zeros((GW, N, U), dtype=torch.int64, device="cuda")
    (f_d, r_d) = (up(env, f), up(env, r))           # (held until the import has run)
    env.ctx.call("fcd_gibbs_import_state", env.lib.dptr(f_d), env.lib.dptr(r_d), N, U, G, env.lib.dptr(f_state),
                 env.lib.dptr(r_bits), env.lib.stream_ptr())
    torch.cuda.synchronize()
    del f_d, r_d
    w0 = rng.normal(size=(G, U))
    (beta_prev, beta) = (0.3, 0.7)
    outs = []
    for _ in range(2):
        w = up(env, w0)
        lMb = torch.full_like(lM_d, np.nan)
        env.ctx.call("fcd_score_ais_step", env.lib.dptr(lM_d), env.lib.dptr(f_state), env.lib.dptr(r_bits), N, U, G,
                     beta_prev, beta, env.lib.dptr(w), env.lib.dptr(lMb), env.lib.stream_ptr())
        outs.append((w.cpu().numpy(), lMb.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes()
    nptest.assert_array_equal(outs[0][1], beta * lM)
    want = w0 + (beta - beta_prev) * ais_step_ref(lM, f.astype(np.int64), r)
    scale = (beta - beta_prev) * ais_step_ref(np.abs(lM), f.astype(np.int64), r) + np.abs(w0)
    assert np.all(np.abs(outs[0][0] - want) <= 1e-12 * scale), np.max(np.abs(outs[0][0] - want) / scale)
    # no table asked for: w alone
    w = up(env, w0)
    env.ctx.call("fcd_score_ais_step", env.lib.dptr(lM_d), env.lib.dptr(f_state), env.lib.dptr(r_bits), N, U, G, beta_prev,
                 beta, env.lib.dptr(w), env.lib.dptr(None), env.lib.stream_ptr())
    assert w.cpu().numpy().tobytes() == outs[0][0].tobytes()


def test_ais_finish_kernel(env):
    """fcd_score_ais_finish against score_ref.ais_parts (a G that is not a multiple of 64, one patient at -inf)."""
    rng = np.random.default_rng(9)
    w = rng.normal(size=(1000, 5)) * np.array([0.1, 1.0, 10.0, 50.0, 1.0]) - 300.0
    w[:, 4] = -np.inf
    o4 = env.torch.empty((5, 4), dtype=env.torch.float64, device="cuda")
    env.ctx.call("fcd_score_ais_finish", env.lib.dptr(up(env, w)), 5, 1000, env.lib.dptr(o4), env.lib.stream_ptr())
    got = o4.cpu().numpy()
    nptest.assert_allclose(got[:4], R.ais_parts(w[:, :4]), rtol=1e-13)
    nptest.assert_array_equal(got[4], [-np.inf, 0.0, 0.0, 1000.0])
