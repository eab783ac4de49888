"""
Per-subject measurement noise on the MI355X: var_b (H,) and var_bt (U, K) through the table kernels
(fcd_lik_tables_noise, fcd_lik_shared_tables_noise), the connection posterior (fcd_conn_posterior_noise), both fits with
both methods, the evidence and scoring, against the NumPy reference of tests/noise_ref.py.

Tolerance rule of the tables: noise_ref.tolerance, which is sessions_ref.tolerance's -- rtol 1e-12, atol = 1e-14
max(1, max |sum_k ln N|) over the case; S_B by the same rule on the control sums (noise_ref.tolerance_b).
"""
import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as CP
import evidence_ref as ER
import exact_law_cases as X
import noise_ref as NR
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
    e.LDS = tables.NOISE_LDS_RECORDS
    return e


def up(env, a):
    return None if a is None else env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def C_of(N):
    return N * (N - 1) // 2


def data(env, N, U, K, H=3, seed=None):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U + K if seed is None else seed, sessions=K)
    return m, b, bt


def variances(H, U, K, seed=0, which="both"):
    """(var_b (H,), var_bt (U, K)) from [0, 0.02] with some exact zeros; which: 'b', 'bt' or 'both' (the other None)."""
    rng = np.random.default_rng(1000 + seed)
    (vb, vbt) = (rng.uniform(0, 0.02, H), rng.uniform(0, 0.02, (U, K)))
    vb[rng.random(H) < 0.25] = 0.0
    vbt[rng.random((U, K)) < 0.25] = 0.0
    vb[0] = 0.0 if H > 1 else vb[0]
    vbt[U - 1, 0] = 0.0
    return (vb if which in ("b", "both") else None, vbt if which in ("bt", "both") else None)


def build(env, m, b, bt, flags=0, shared=False, count=False, noise=None, lpB=False):
    """(S_B, lM, n_missing or None[, lpB]) of tables.build on host arrays; noise = (var_b, var_bt) host arrays or None."""
    t = env.torch
    n = t.zeros(2, dtype=t.int64, device="cuda") if count else None
    lp = t.empty(b.shape + (3,), dtype=t.float64, device="cuda") if lpB else None
    kw = {} if noise is None else {"noise": (up(env, noise[0]), up(env, noise[1]))}
    (S_B, lM) = env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), flags, shared=shared, n_missing=n, lpB=lp, **kw)
    out = (S_B.cpu().numpy(), lM.cpu().numpy(), (None if n is None else tuple(n.cpu().tolist())))
    return out + ((lp.cpu().numpy(),) if lpB else ())


def new_fit(env, model, b, bt, shared=False, **kw):
    fit = env.pkg.fit.SharedRegionFit() if shared else env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (model, b, bt)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


# ------------------------------------------------------------------------------------------------
# 1. the tables
# ------------------------------------------------------------------------------------------------
# (Nreg, U, K, H).  The records are kept in LDS up to tables.NOISE_LDS_RECORDS = 768 of them (max(H, U K)), read from
# global memory above.
SHAPES = [(3, 1, 1, 1), (4, 3, 3, 3),           # smallest
          (23, 1, 2, 17),                       # 253 items: one partial tile, an odd count of doubles, the tail store; H past 16
          (23, 2, 5, 3),                        # two tiles with the second partial, odd K
          (8, 37, 9, 17),                       # a full 9-session pass
          (8, 37, 10, 1),                       # one more session than a pass
          (4, 96, 8, 3),                        # U K = 768: the last shape with the records in LDS
          (4, 769, 1, 3),                       # U K = 769: the first with the records in global memory
          (4, 77, 10, 17),                      # 770 records read from global memory over two passes
          (3, 2, 2, 769),                       # H = 769 control records: global memory on their account
          (46, 1024, 2, 3)]                     # 1 059 840 items > 16 * num_cu * 256: the grid-stride loop (the grid is capped)


def check_placement():
    assert SHAPES[6][1] * SHAPES[6][2] == 768 and SHAPES[7][1] * SHAPES[7][2] == 769


# var_b alone, var_bt alone and both at every shape; the capped-grid shape once, with both
TABLE_CASES = [s + (w,) for s in SHAPES[:-1] for w in ("b", "bt", "both")] + [SHAPES[-1] + ("both",)]


@pytest.mark.parametrize("N,U,K,H,which", TABLE_CASES)
def test_tables_against_reference(env, N, U, K, H, which):
    assert env.LDS == 768
    check_placement()
    (m, b, bt) = data(env, N, U, K, H=H)
    (vb, vbt) = variances(H, U, K, seed=N + K, which=which)
    (S_ref, lM_ref) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, vb, vbt)
    lp_ref = NR.lp_B_g_F(b, m.mu, m.sigma, vb)
    tol = NR.tolerance(bt, m.mu, m.sigma, vbt)
    tol_b = NR.tolerance_b(b, m.mu, m.sigma, vb)
    (S_B, lM, _n, lpB) = build(env, m, b, bt, noise=(vb, vbt), lpB=True)
    nptest.assert_allclose(lM, lM_ref, **tol)
    nptest.assert_allclose(S_B, S_ref, **tol_b)
    nptest.assert_allclose(lpB, lp_ref, **tol_b)
    # the shared build: L = sum_u lM, S_B the unshared build's bit for bit
    (S_s, L, _n) = build(env, m, b, bt, shared=True, noise=(vb, vbt))
    assert L.shape == (C_of(N), 1, 3, 3)
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **NR.tolerance(bt, m.mu, m.sigma, vbt, scale=3))
    nptest.assert_array_equal(S_s, S_B)
    if K == 1:
        # a 2-D bt with a (U,) variance is the same call
        (S_2, lM_2, _n) = build(env, m, b, bt[:, :, 0], noise=(vb, None if vbt is None else vbt[:, 0]))
        nptest.assert_array_equal(lM_2, lM)
        nptest.assert_array_equal(S_2, S_B)
    if vb is None:
        # without control variances S_B is today's, bit for bit
        (S_0, _lM0, _n) = build(env, m, b, bt)
        nptest.assert_array_equal(S_B, S_0)


@pytest.mark.parametrize("N,U,K,H", SHAPES[:9])
def test_zero_variances_against_the_existing_builds(env, N, U, K, H):
    (m, b, bt) = data(env, N, U, K, H=H)
    (S_0, lM_0, _n) = build(env, m, b, bt)                        # the sessions build
    tol = SR.tolerance(bt, m.mu, m.sigma)
    for noise in ((np.zeros(H), np.zeros((U, K))), (None, np.zeros((U, K))), (np.zeros(H), None), (None, None)):
        (S_B, lM, _n) = build(env, m, b, bt, noise=noise)
        nptest.assert_allclose(lM, lM_0, **tol)
        nptest.assert_allclose(S_B, S_0, rtol=1e-12)
        (_S, L, _n) = build(env, m, b, bt, shared=True, noise=noise)
        (_S, L_0, _n) = build(env, m, b, bt, shared=True)
        nptest.assert_allclose(L, L_0, **SR.tolerance(bt, m.mu, m.sigma, scale=3))
    if K == 1:
        (S_2, lM_2, _n) = build(env, m, b, bt[:, :, 0])           # the 2-D build
        (S_B, lM, _n) = build(env, m, b, bt[:, :, 0], noise=(np.zeros(H), np.zeros(U)))
        nptest.assert_allclose(lM, lM_2, **tol)
        nptest.assert_allclose(S_B, S_2, rtol=1e-12)


@pytest.mark.parametrize("K", [None, 3])
@pytest.mark.parametrize("shared", [False, True])
def test_noise_none_is_todays_call_bit_for_bit(env, K, shared):
    (m, b, bt) = data(env, 9, 5, K or 1, H=4)
    bt = bt[:, :, 0] if K is None else bt
    t = env.torch
    P = env.lib.dptr
    (b_d, bt_d) = (up(env, b), up(env, bt))
    (S_B, lM) = env.tables.build(env.ctx, b_d, bt_d, m.theta(), 0, shared=shared, noise=None)
    (S_1, lM_1) = env.tables.build(env.ctx, b_d, bt_d, m.theta(), 0, shared=shared)
    (S_2, lM_2) = (t.empty_like(S_B), t.empty_like(lM))
    (th, _th) = env.lib.dbl_array(m.theta())
    sess = () if K is None else (K,)
    if shared:
        env.ctx.call("fcd_lik_shared_tables_sessions" if K else "fcd_lik_shared_tables", P(b_d), P(bt_d), 36, 4, 5, *sess, th,
                     P(S_2), P(lM_2), 0, P(None), env.lib.stream_ptr())
    elif K:
        env.ctx.call("fcd_lik_tables_sessions", P(b_d), P(bt_d), 36, 4, 5, K, th, P(S_2), P(lM_2), P(None), 0, P(None),
                     env.lib.stream_ptr())
    else:
        env.ctx.call("fcd_lik_tables_ex", P(b_d), P(bt_d), 36, 4, 5, th, P(S_2), P(lM_2), P(None), P(None), 0, P(None),
                     env.lib.stream_ptr())
    for (x, y) in ((S_B, S_2), (lM, lM_2), (S_1, S_2), (lM_1, lM_2)):
        nptest.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    # and a fit without variances makes exactly that table
    fit = new_fit(env, m, b, bt, shared=shared)
    fit._init_lps(9, 4, 5)
    fit._update_lps()
    nptest.assert_array_equal(fit._lM, lM_2.cpu().numpy())
    assert "noise" not in fit._d


@pytest.mark.parametrize("pattern", ["random", "patient"])
@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_nan_session_is_bit_identical_to_leaving_it_out(env, pattern, where):
    """test_gpu_sessions.py's construction with a variance column inserted alongside the NaN session."""
    (N, U, K, H) = (23, 5, 4, 3)
    MISS = env.lib.FCD_DATA_NAN_MISSING
    (m, b, bt) = data(env, N, U, K - 1)
    (vb, vbt) = variances(H, U, K - 1, seed=3)
    rng = np.random.default_rng(5)
    if pattern == "random":
        bt[rng.random(bt.shape) < 0.1] = np.nan                # 10 % NaN session entries
    else:
        bt[:, 2, :] = np.nan                                    # one whole patient
    bt[7, 1, :] = np.nan                                        # an item with no observed session
    b = b.copy()
    b[4, 1] = np.nan
    (S0, lM0, n0) = build(env, m, b, bt, MISS, count=True, noise=(vb, vbt))
    at = {"front": 0, "middle": 2, "end": K - 1}[where]
    btn = np.insert(bt, at, np.nan, axis=2)
    vn = np.insert(vbt, at, rng.uniform(0, 0.02, U), axis=1)    # whatever variance the NaN session carries
    assert btn.shape == (C_of(N), U, K) and vn.shape == (U, K)
    (S1, lM1, n1) = build(env, m, b, btn, MISS, count=True, noise=(vb, vn))
    nptest.assert_array_equal(lM1, lM0)
    nptest.assert_array_equal(S1, S0)
    none = np.isnan(btn).all(axis=2)
    assert none.sum() >= 1 and np.all(lM1[none] == 0.0) and not np.signbit(lM1[none]).any()
    assert np.all(np.isfinite(lM1))
    assert n0 == (1, int(np.isnan(bt).sum())) and n1 == (1, int(np.isnan(btn).sum()))
    (S_ref, lM_ref) = NR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, vb, vn, missing=True)
    nptest.assert_allclose(lM1, lM_ref, **NR.tolerance(btn, m.mu, m.sigma, vn, missing=True))
    nptest.assert_allclose(S1, S_ref, **NR.tolerance_b(b, m.mu, m.sigma, vb, missing=True))
    # the shared build counts the same
    (_S, L, ns) = build(env, m, b, btn, MISS, shared=True, count=True, noise=(vb, vn))
    assert ns == n1
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **NR.tolerance(btn, m.mu, m.sigma, vn, missing=True, scale=3))
    # the fit's own count
    fit = new_fit(env, m, b, btn, missing_data=True, b_noise_var=vb, bt_noise_var=vn)
    fit._init_lps(N, H, U)
    fit._update_lps()
    assert fit.missing_counts() == n1 and fit.n_sessions == K
    nptest.assert_array_equal(fit._lM, lM1)


def test_entry_point_refusals(env):
    (m, b, bt) = data(env, 4, 2, 2)
    t = env.torch
    (b_d, bt_d) = (up(env, b), up(env, bt))
    (vb_d, vbt_d) = (up(env, np.full(3, 0.01)), up(env, np.full((2, 2), 0.01)))
    (S_B, lM) = (t.empty((6, 3), dtype=t.float64, device="cuda"), t.empty((6, 2, 3, 3), dtype=t.float64, device="cuda"))
    (th, _th) = env.lib.dbl_array(m.theta())
    P = env.lib.dptr

    def tab(C=6, K=2, flags=0):
        env.ctx.call("fcd_lik_tables_noise", P(b_d), P(bt_d), C, 3, 2, K, th, P(vb_d), P(vbt_d), P(S_B), P(lM), P(None), flags,
                     P(None), env.lib.stream_ptr())

    def shr(C=6, K=2, flags=0):
        env.ctx.call("fcd_lik_shared_tables_noise", P(b_d), P(bt_d), C, 3, 2, K, th, P(vb_d), P(vbt_d), P(S_B), P(lM), flags,
                     P(None), env.lib.stream_ptr())
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
        env.ctx.call("fcd_conn_posterior_noise", P(bt_d), 4, 2, K, th, P(vbt_d), P(cnt), P(None), P(None), flags, P(out[0]),
                     P(out[1]), P(out[2]), env.lib.stream_ptr())
    post()
    with pytest.raises(ValueError):
        post(K=0)
    with pytest.raises(NotImplementedError):
        post(K=1 << 31)
    with pytest.raises(ValueError, match="flags"):
        post(flags=2)
    env.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 2. connection posterior
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("N,U,K", [(3, 1, 1), (4, 3, 3), (6, 5, 4), (8, 37, 10)])
def test_connection_posterior_against_the_enumeration(env, N, U, K, nan):
    from fcdiff_amd.fit import conn_posterior
    (m, _b, bt) = data(env, N, U, K)
    m.sigma = np.array([0.1, 0.12, 0.15])
    theta = m.theta()
    (_vb, vbt) = variances(1, U, K, seed=N)
    rng = np.random.default_rng(N + K)
    if nan:
        bt[rng.random(bt.shape) < 0.25] = np.nan
        bt[1, 0, :] = np.nan
    C = C_of(N)
    cnt = rng.integers(0, 40, (C, U, 3, 3)).astype(np.uint32)
    cnt[:, :, 0, 0] += 1
    lq_F = np.log(rng.dirichlet(np.ones(3), C))[:, None, :]
    lq_R = np.log(rng.dirichlet(np.ones(2), (N, U)))
    tol = NR.tolerance(bt, m.mu, m.sigma, vbt, missing=nan)
    for (kw, W) in (({"counts": up(env, cnt.view(np.int32))}, cnt.astype(np.float64)),
                    ({"lq_F": up(env, lq_F), "lq_R": up(env, lq_R)}, CP.vb_weights(lq_F, lq_R))):
        got = conn_posterior(env.ctx, up(env, bt), N, U, theta, missing_data=nan, noise_var=up(env, vbt), **kw)
        want = NR.enumerated_posterior(W, bt, theta, vbt, nan)
        for key in ("p_T", "p_F_tilde", "p_changed"):
            nptest.assert_allclose(got[key], want[key], err_msg=key, **tol)
        plain = conn_posterior(env.ctx, up(env, bt), N, U, theta, missing_data=nan, **kw)
        zero = conn_posterior(env.ctx, up(env, bt), N, U, theta, missing_data=nan, noise_var=up(env, np.zeros((U, K))), **kw)
        for key in ("p_T", "p_F_tilde", "p_changed"):
            nptest.assert_allclose(zero[key], plain[key], err_msg=key, **NR.tolerance(bt, m.mu, m.sigma, None, missing=nan))
        if K == 1:
            two_d = conn_posterior(env.ctx, up(env, bt[:, :, 0]), N, U, theta, missing_data=nan, noise_var=up(env, vbt[:, 0]),
                                   **kw)
            nptest.assert_array_equal(two_d["p_T"], got["p_T"])


# ------------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------------
def e2e_data(env, N=5, U=4, K=2, H=4):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=21, sessions=K)
    (vb, vbt) = variances(H, U, K, seed=7)
    return b, bt, vb, vbt


@pytest.mark.parametrize("shared", [False, True])
def test_vb_fit_against_the_reference_loop(env, shared):
    (b, bt, vb, vbt) = e2e_data(env)
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    start = theta_dict(model.theta())
    fit = new_fit(env, model, b, bt, shared=shared, max_iters=4, rel_tol=-np.inf, b_noise_var=vb, bt_noise_var=vbt)
    fit.run()
    want = NR.vb_fit(b, bt, start, 4, O.EDGE_SYMMETRIC if shared else O.EDGE_REFERENCE, shared=shared, var_b=vb, var_bt=vbt)
    plain = SR.vb_fit(b, bt, start, 4, O.EDGE_SYMMETRIC if shared else O.EDGE_REFERENCE, shared=shared)
    assert len(fit.energy) == 5 and fit.n_sessions == 2
    nptest.assert_allclose(fit.energy, want["energy"], **FIT)
    nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
    nptest.assert_allclose(fit._lq_F, want["lq_F"], **FIT)
    assert not np.allclose(fit.energy, plain["energy"], rtol=1e-6)          # (the variances are not ignored)
    nptest.assert_allclose(fit._lM, want["lM"], **NR.tolerance(bt, model.mu, model.sigma, vbt, scale=3 if shared else 1))
    post = fit.connection_posterior()
    W = CP.vb_weights(fit._lq_F, np.broadcast_to(fit._lq_R, (5, 4, 2)) if shared else fit._lq_R)
    ref = NR.enumerated_posterior(W, bt, fit.model.theta(), vbt)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(post[key], ref[key], err_msg=key, **NR.tolerance(bt, model.mu, model.sigma, vbt))
    # the device copies follow the host values
    fit.bt_noise_var = np.zeros_like(vbt)
    fit.b_noise_var = None
    fit._update_lps()
    (_S, lM_0) = SR.lik_tables(b, bt, fit.model.mu, fit.model.sigma, fit.model.eta, fit.model.epsilon)
    nptest.assert_allclose(fit._lM, lM_0.sum(axis=1, keepdims=True) if shared else lM_0,
                           **SR.tolerance(bt, model.mu, model.sigma, scale=3 if shared else 1))
    fit.bt_noise_var = vbt
    fit._update_lps()
    vbt[0, 0] = 0.015                                                       # edited in place
    fit._update_lps()
    (_S, lM_1) = NR.lik_tables(b, bt, fit.model.mu, fit.model.sigma, fit.model.eta, fit.model.epsilon, None, vbt)
    nptest.assert_allclose(fit._lM, lM_1.sum(axis=1, keepdims=True) if shared else lM_1,
                           **NR.tolerance(bt, model.mu, model.sigma, vbt, scale=3 if shared else 1))


@pytest.mark.parametrize("shared", [False, True])
def test_gibbs_fit_equals_the_oracle_chain_for_chain(env, shared):
    """(4, 3, 1): the sampler on the noise tables is the oracle's sampler on the reference's noise tables, chain for chain."""
    (N, U, H) = (4, 3, 4)
    (b, bt, vb, vbt) = e2e_data(env, N=N, U=U, K=1, H=H)
    bt = np.ascontiguousarray(bt[:, :, 0])
    vbt = vbt[:, 0].copy()
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    fit = new_fit(env, model, b, bt, shared=shared, method="gibbs", n_chains=128, n_sweeps=6, burn_in=2, mstep_every=0,
                  seed=77, connection_marginals=True, b_noise_var=vb, bt_noise_var=vbt)
    (gamma, pi2) = (np.array(model.gamma, dtype=np.float64), model.pi2())
    fit.run()
    (S_B, lM) = (fit._d["S_B"].cpu().numpy(), fit._lM)
    Us = 1 if shared else U
    (S_ref, lM_ref) = NR.lik_tables(b, bt, model.mu, model.sigma, model.eta, model.epsilon, vb, vbt)
    nptest.assert_allclose(lM, lM_ref.sum(axis=1, keepdims=True) if shared else lM_ref,
                           **NR.tolerance(bt, model.mu, model.sigma, vbt, scale=3 if shared else 1))
    nptest.assert_allclose(S_B, S_ref, **NR.tolerance_b(b, model.mu, model.sigma, vb))
    (f_o, r_o) = env.CO.gibbs_init(128, N, Us, float(pi2[1]), 77, 0)
    for s in range(6):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(gamma), 77, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, np.log(pi2), 77, s, env.lib.EDGE_MODES["symmetric"], 0)
    (f_g, r_g) = fit.sampler.export_state()
    assert env.ctx.stat("dev_err") == 0
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    post = fit.connection_posterior()
    W = np.asarray(fit.connection_counts, dtype=np.float64)
    ref = NR.enumerated_posterior(np.broadcast_to(W, (C_of(N), U, 3, 3)), bt, fit.model.theta(), vbt)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(post[key], ref[key], err_msg=key, **NR.tolerance(bt, model.mu, model.sigma, vbt))
    with pytest.raises(NotImplementedError, match="noise"):
        fit.membership(bt[:, :2])


@pytest.mark.parametrize("shared", [False, True])
def test_log_evidence_against_the_enumeration(env, shared):
    """4 regions, 3 patients, one scan, with variances: the acceptance rule of test_gpu_sessions.py's sibling."""
    m = X.model("broad")
    (N, H, U) = (4, 2, 3)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=42)
    (vb, vbt) = variances(H, U, 1, seed=11)
    vbt = vbt[:, 0].copy()
    model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    for k in ("pi", "eta", "epsilon"):
        setattr(model, k, getattr(m, k))
    (model.gamma, model.mu, model.sigma) = (np.array(m.gamma), np.array(m.mu), np.array(m.sigma))
    fit = new_fit(env, model, b, bt, shared=shared, max_iters=2, n_chains=64, b_noise_var=vb, bt_noise_var=vbt)
    fit.run()
    for k in ("pi", "eta", "epsilon"):
        setattr(model, k, getattr(m, k))
    model.gamma = np.array(m.gamma)
    (S_B, lM) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, vb, vbt)
    exact_fn = ER.exact_log_evidence_shared if shared else ER.exact_log_evidence
    exact = exact_fn(S_B, lM, np.asarray(m.gamma, dtype=np.float64), m.pi2())
    (lpB, _pBt, lM_p) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    plain = exact_fn(O.sum_lp_B(lpB), lM_p, np.asarray(m.gamma, dtype=np.float64), m.pi2())
    out = fit.log_evidence(n_anneal=50, n_chains=4096, seed=1282)
    print("shared=%s exact %.4f (without variances %.4f) estimate %.4f se %.4f ess %.0f lower %.4f (%.4f)" % (
        shared, exact, plain, out["log_evidence"], out["log_evidence_se"], out["ess"], out["lower"], out["lower_se"]))
    assert out["n_chains"] == 4096 and out["n_anneal"] == 50
    assert abs(out["log_evidence"] - exact) <= 5.0 * out["log_evidence_se"]
    assert out["lower"] - 5.0 * out["lower_se"] <= exact
    assert abs(plain - exact) > 10.0 * out["log_evidence_se"]               # (an estimate of the other model would fail)


@pytest.mark.parametrize("K_new", [None, 2])
def test_score_against_a_reference_vb_of_the_new_patients(env, K_new):
    (N, H, U) = (6, 4, 4)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=8)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(N, H, 3, seed=9, sessions=K_new)
    (vb, vbt) = variances(H, U, 1, seed=5)
    (_v, v_new) = variances(H, 3, K_new or 1, seed=6)
    v_new = v_new[:, 0].copy() if K_new is None else v_new
    fit = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt, max_iters=3, b_noise_var=vb, bt_noise_var=vbt[:, 0])
    fit.run()
    with pytest.raises(ValueError, match="noise_var"):
        fit.score(bt_new)
    out = fit.score(bt_new, noise_var=v_new, connections=True, max_iters=6, tol=0.0)        # tol 0: six iterations each
    assert np.all(out["iters"] == 6)
    th = theta_dict(fit.model.theta())
    want = NR.vb_fit(b, bt_new, th, 6, O.EDGE_REFERENCE, var_b=vb, var_bt=v_new, lq_F=fit._lq_F, update_theta=False)
    nptest.assert_allclose(out["p_R"], np.exp(want["lq_R"][:, :, 1]), **FIT)
    W = CP.vb_weights(fit._lq_F, want["lq_R"])
    ref = NR.enumerated_posterior(W, bt_new, fit.model.theta(), v_new)
    # (the weights come from the reference's lq_R, which the device's equals to FIT: ten times FIT for what is made of them)
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_allclose(out[key], ref[key], rtol=1e-9, atol=1e-11, err_msg=key)
    # zeros are allowed, and are the scores of the plain tables
    zero = fit.score(bt_new, noise_var=np.zeros(3), max_iters=6, tol=0.0)
    want0 = NR.vb_fit(b, bt_new, th, 6, O.EDGE_REFERENCE, var_b=vb, lq_F=fit._lq_F, update_theta=False)
    nptest.assert_allclose(zero["p_R"], np.exp(want0["lq_R"][:, :, 1]), **FIT)
    assert not np.allclose(zero["p_R"], out["p_R"], rtol=1e-6, atol=1e-9)


def test_score_of_a_sampler_fit_takes_the_variances(env):
    (N, H, U) = (6, 4, 4)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=8)
    (_r, _t, _f, _ft, _b, bt_new) = m.sample_fast(N, H, 3, seed=9)
    (vb, vbt) = variances(H, U, 1, seed=5)
    (_v, v_new) = variances(H, 3, 1, seed=6)
    fit = new_fit(env, env.pkg.UnsharedRegionModel(), b, bt, method="gibbs", edge_index="symmetric", n_chains=128, n_sweeps=8,
                  burn_in=2, b_noise_var=vb, bt_noise_var=vbt[:, 0])
    fit.run()
    out = fit.score(bt_new, noise_var=v_new[:, 0], connections=True, n_anneal=10, n_sweeps=5, seed=3)
    big = fit.score(bt_new, noise_var=np.full(3, 0.5), n_anneal=10, n_sweeps=5, seed=3)
    assert out["p_R"].shape == (N, 3) and out["p_T"].shape == (C_of(N), 3)
    assert all(np.all(np.isfinite(out[k])) for k in ("p_R", "p_T", "p_F_tilde", "p_changed", "log_pred"))
    # sd 0.7 of measurement noise leaves nothing to tell the states apart: the maps fall back to the prior's
    assert np.abs(big["p_R"] - fit._pi2()[1]).max() < 0.25 and not np.allclose(big["log_pred"], out["log_pred"])


# ------------------------------------------------------------------------------------------------
# 4. the scenario: half the patients measured with more noise
# ------------------------------------------------------------------------------------------------
def test_scenario_through_the_fit(env):
    """
    test_noise.py's scenario through UnsharedRegionFit (vb, 8 iterations, symmetric edge ids -- see there), with and without
    bt_noise_var: lq_R is the reference's, and the same three inequalities hold (reference: 0.270, 0.018, 0.82).
    """
    s = NR.SCENARIO

    def model():
        m = env.pkg.UnsharedRegionModel()
        m.pi = s["pi"]
        return m
    (b, bt, r, var_bt) = NR.scenario_data(model())
    start = theta_dict(model().theta())
    rates = []
    for v in (None, var_bt):
        fit = new_fit(env, model(), b, bt, max_iters=s["iters"], rel_tol=-np.inf, edge_index="symmetric", bt_noise_var=v)
        fit.run()
        want = NR.vb_fit(b, bt, start, s["iters"], O.EDGE_SYMMETRIC, var_bt=v)
        nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
        rates.append(NR.scenario_rates(fit._lq_R, r))
        print("bt_noise_var %s: fp %.3f hits %.3f pi %.3f" % ("given" if v is not None else "None", rates[-1][0],
                                                            rates[-1][1], float(fit.model.pi)))
    assert rates[0][0] >= 0.15
    assert rates[1][0] <= 0.05
    assert rates[1][1] >= 0.6
