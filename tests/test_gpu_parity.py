"""
GPU parity tests (run with -m gpu on an MI355X).  Every call goes through the C ABI
(include/fcdiff_hip.h) via the Python mirror of the reference API; expected values come from
  * fixtures captured from the reference itself (tests/golden), and
  * the CPU oracle (oracle/), which test_oracle_golden.py / test_oracle_c.py pin to those fixtures.

Tolerances (fp64): tables rtol 1e-12 (device exp/log are within a few ulp of libm's); quantities
that sum over patients/edges rtol 1e-10; integer state (Gibbs chains, counts) bit-exact.
"""
import os

import numpy as np
import numpy.testing as nptest
import pytest

from conftest import ROOT, load_golden, theta_dict

pytestmark = pytest.mark.gpu

TAB = dict(rtol=1e-12, atol=1e-14)
SUM = dict(rtol=1e-10, atol=1e-11)


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
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO, e.O = torch, fcdiff_amd, _lib, GibbsEngine, CO, O
    e.ctx = _lib.Context()
    return e


def make_model(env, theta):
    th = theta_dict(theta)
    m = env.pkg.UnsharedRegionModel()
    m.pi, m.eta, m.epsilon = th["pi"], th["eta"], th["epsilon"]
    m.gamma, m.mu, m.sigma = th["gamma"], th["mu"], th["sigma"]
    return m


def new_fit(env):
    f = env.pkg.fit.UnsharedRegionFit()
    f._ctx = env.ctx
    return f


def up(env, a, dtype=None):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@pytest.fixture
def knobs(env):
    """Set tuning / test knobs of the shared context (fcd_ctx_set_knob) for one test; all back to default afterwards."""
    touched = []

    def set_(**kw):
        for (k, v) in kw.items():
            env.ctx.set_knob(k, v)
            touched.append(k)
    yield set_
    for k in touched:
        env.ctx.set_knob(k, 0)


# ------------------------------------------------------------------------------------------------
# K_lik: UnsharedRegionFit._update_lps  (test_fcdiff/test_fit.py:131-166)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G2_update_lps", "G2b_update_lps_default"])
def test_update_lps_against_reference_fixture(env, name):
    g = load_golden(name)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = g["b"], g["bt"], make_model(env, g["theta"])
    (C, H) = g["b"].shape
    U = g["bt"].shape[1]
    N = int(round(env.pkg.util.C_to_N(C)))
    fit._init_lps(N, H, U)
    assert fit._lq_R.shape == (N, U, 2) and fit._lq_F.shape == (C, 1, 3) and fit._lM.shape == (C, U, 3, 3)
    nptest.assert_allclose(np.sum(np.exp(fit._lq_R), axis=2), 1)
    nptest.assert_allclose(np.sum(np.exp(fit._lq_F), axis=2), 1)
    fit._update_lps()
    nptest.assert_allclose(fit._lM, g["lM"], **TAB)
    nptest.assert_allclose(fit._lp_B_g_F, g["lp_B_g_F"], **TAB)
    nptest.assert_allclose(fit._p_Bt_g_Ft, g["p_Bt_g_Ft"], rtol=1e-12, atol=0)
    nptest.assert_allclose(fit._d["S_B"].cpu().numpy(), g["lp_B_g_F"].sum(axis=1), rtol=1e-12)
    assert fit._lp_B_g_F.shape == (C, H, 3) and fit._p_Bt_g_Ft.shape == (C, U, 3)


@pytest.mark.parametrize("N,H,U", [(2, 1, 1), (3, 1, 70), (9, 17, 1), (23, 16, 37), (40, 3, 129)])
def test_lik_tables_ragged_shapes(env, N, H, U):
    """Sizes that are not multiples of the 256-item tile / 16-lane groups, against the C oracle."""
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    nptest.assert_allclose(fit._lM, lM, **TAB)
    nptest.assert_allclose(fit._d["S_B"].cpu().numpy(), S_B, rtol=1e-12)


def test_lik_tables_underflow_gives_minus_inf_like_reference(env):
    """The reference forms M from linear-space densities (fit.py:115,121-122): |z| > 38.6 underflows."""
    m = env.pkg.UnsharedRegionModel()
    m.sigma = np.array([1e-3, 1e-3, 1e-3])
    b = np.zeros((3, 2))
    bt = np.array([[1.0, -1.0], [0.0, 0.3], [-0.15, 1.0]])
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(3, 2, 2)
    fit._update_lps()
    with np.errstate(divide="ignore"):
        _, _, lM = env.O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    got = fit._lM
    assert np.array_equal(np.isneginf(got), np.isneginf(lM)) and np.isneginf(lM).any()
    fin = np.isfinite(lM)
    nptest.assert_allclose(got[fin], lM[fin], **TAB)


def test_lik_tables_wide_dynamic_range(env):
    """
    K_lik uses its own table-driven log (fcd_lik.hip): sweep the mixture density over its whole range --
    from ~40 down through the subnormals to exact underflow -- and compare with NumPy's log in the oracle.
    """
    m = env.pkg.UnsharedRegionModel()
    m.sigma = np.array([0.0211, 0.0207, 0.0219])
    (N, H, U) = (10, 2, 89)
    C = 45
    bt = np.linspace(-1.0, 1.0, C * U).reshape(C, U)
    bt[3, 5] = m.mu[1]                      # exactly at a mode
    b = np.zeros((C, H))
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    with np.errstate(divide="ignore"):
        _, pBt, lM = env.O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    got = fit._lM
    assert np.isneginf(lM).any() and (lM > 2).any() and ((lM < -700) & np.isfinite(lM)).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(lM))
    fin = np.isfinite(lM)
    nptest.assert_allclose(got[fin], lM[fin], rtol=5e-13, atol=2e-15)
    # near M = 1 (log ~ 0) the table log has no cancellation: the absolute error is that of M itself (a few ulp,
    # from the reciprocal multiplies that stand in for the reference's divisions)
    near1 = fin & (np.abs(lM) < 0.05)
    if near1.any():
        assert np.max(np.abs(got[near1] - lM[near1])) < 3e-15


def test_lik_tables_cfg3_size(env):
    """BASELINE cfg 3 shape (Nreg=200, H=U=50) against the C oracle."""
    (N, H, U) = (200, 50, 50)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    nptest.assert_allclose(fit._lM, lM, **TAB)
    nptest.assert_allclose(fit._d["S_B"].cpu().numpy(), S_B, rtol=1e-12)


# ------------------------------------------------------------------------------------------------
# VB updates (test_fit.py:428-557) and energy (170-230, 389-425)
# ------------------------------------------------------------------------------------------------
def test_update_lq_F(env):
    g = load_golden("G4_update_lq_F")
    fit = new_fit(env)
    fit._lq_R = np.log(g["q_R"])
    fit._lp_B_g_F = g["lp_B_g_F"]
    fit._lM = g["lM"]
    fit.model = env.pkg.UnsharedRegionModel()
    fit.model.gamma = g["gamma"]
    fit._update_lq_F()
    assert fit._lq_F.shape == g["lq_F"].shape
    nptest.assert_allclose(fit._lq_F, g["lq_F"], **SUM)


def test_update_lq_R_reference_and_symmetric(env):
    g = load_golden("G5_update_lq_R")
    for mode in ("reference", "symmetric"):
        fit = new_fit(env)
        fit.edge_index = mode
        fit._lq_R = np.log(g["q_R"])
        fit._lq_F = np.log(g["q_F"])
        fit._lM = g["lM"]
        fit.model = env.pkg.UnsharedRegionModel()
        fit.model.pi = g["pi"]                      # 2-vector, as the reference's test passes it
        fit._update_lq_R()
        if mode == "reference":
            nptest.assert_allclose(fit._lq_R, g["lq_R"], **SUM)
        else:
            exp = env.O.update_lq_R(np.log(g["q_R"]), np.log(g["q_F"]), g["lM"], g["pi"], env.O.EDGE_SYMMETRIC)
            nptest.assert_allclose(fit._lq_R, exp, **SUM)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("N,U", [(5, 3), (64, 16), (70, 65), (130, 7), (200, 50), (300, 9), (520, 3)])
def test_update_lq_R_forms_against_oracle(env, knobs, form, N, U):
    """
    fcd_vb_update_qR has two forms (knob qr_form): 1 = operands gathered from the edge-major table inside the region loop,
    2 = region-major weights made first, then one wave per patient (round 4; the default up to 192 MB of weights).  Both
    against the C oracle's update_lq_R (fcdiff/fit.py:176-198) on the same inputs, every wave count / regions-per-lane
    variant of the kernels (Nreg <= 64, 128, 256, 512, above), both edge-id modes.
    """
    rng = np.random.default_rng(N * 1000 + U)
    C = N * (N - 1) // 2
    lM = rng.normal(size=(C, U, 3, 3)) * 2.0
    q_R = rng.dirichlet([1.0, 1.0], size=(N, U))
    q_F = rng.dirichlet([1.0, 1.0, 1.0], size=(C, 1))
    pi2 = np.array([0.7, 0.3])
    knobs(qr_form=form)
    for mode in ("reference", "symmetric"):
        fit = new_fit(env)
        fit.edge_index = mode
        fit._lq_R, fit._lq_F, fit._lM = np.log(q_R), np.log(q_F), lM
        fit.model = env.pkg.UnsharedRegionModel()
        fit.model.pi = pi2
        fit._update_lq_R()
        exp = env.CO.update_lq_R(np.log(q_R), np.log(q_F), lM, pi2, 0 if mode == "reference" else 1)
        nptest.assert_allclose(fit._lq_R, exp, rtol=1e-9, atol=1e-10)
        nptest.assert_allclose(np.exp(fit._lq_R).sum(axis=2), 1.0, rtol=1e-12)


def test_update_lq_R_reference_ids_need_three_regions(env):
    fit = new_fit(env)
    fit._lq_R = np.log(np.full((2, 3, 2), 0.5))
    fit._lq_F = np.log(np.full((1, 1, 3), 1 / 3))
    fit._lM = np.zeros((1, 3, 3, 3))
    fit.model = env.pkg.UnsharedRegionModel()
    with pytest.raises(IndexError):                 # the reference indexes _lM[1] of a size-1 axis
        fit._update_lq_R()
    fit.edge_index = "symmetric"
    fit._update_lq_R()


def test_energy_terms(env):
    g = load_golden("G6_energy_terms")
    fit = new_fit(env)
    fit.model = env.pkg.UnsharedRegionModel()
    fit.model.gamma, fit.model.pi = g["gamma"], g["pi2"]
    fit._lq_F, fit._lq_R, fit._lp_B_g_F, fit._lM = np.log(g["q_F"]), np.log(g["q_R"]), g["lp_B_g_F"], g["lM"]
    nptest.assert_allclose(fit._energy_terms(), g["terms"], **SUM)
    nptest.assert_allclose(fit._eval_energy(), g["energy"], **SUM)
    e1, e2 = fit._eval_energy(), fit._eval_energy()
    assert e1 == e2                                 # fixed reduction order: bitwise repeatable


def test_update_pi_gamma(env):
    g = load_golden("G7_pi_gamma")
    fit = new_fit(env)
    fit.model = env.pkg.UnsharedRegionModel()
    fit._lq_R = np.log(g["q_R"])
    fit._update_pi()
    nptest.assert_allclose(fit.model.pi, g["pi"], rtol=1e-13)
    assert np.ndim(fit.model.pi) == 0
    fit2 = new_fit(env)
    fit2.model = env.pkg.UnsharedRegionModel()
    fit2._lq_F = np.log(g["q_F"])
    fit2._update_gamma()
    nptest.assert_allclose(fit2.model.gamma, g["gamma"], rtol=1e-13)


@pytest.mark.parametrize("name,iters", [("G10_vb_trajectory_cfg1", 4), ("G10b_vb_trajectory_cfg1_ideal", 4),
                                        ("G12_vb_trajectory_mid", 3)])
def test_run_reproduces_reference_vb_trajectory(env, name, iters):
    """run() = the documented loop; energies, q's, pi, gamma after each iteration vs the reference's."""
    g = load_golden(name)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = g["b"], g["bt"], make_model(env, g["theta0"])
    fit.max_iters = iters
    fit.rel_tol = -np.inf                            # never 'converged': record the whole trajectory
    fit.run()
    assert len(fit.energy) == iters + 1
    nptest.assert_allclose(fit.energy, g["energy"], rtol=1e-10)
    nptest.assert_allclose(fit._lq_F, g["lq_F"][iters - 1], rtol=1e-8, atol=1e-10)
    nptest.assert_allclose(fit._lq_R, g["lq_R"][iters - 1], rtol=1e-8, atol=1e-10)
    nptest.assert_allclose(fit.model.pi, g["pi"][iters], rtol=1e-10)
    nptest.assert_allclose(fit.model.gamma, g["gamma"][iters], rtol=1e-10)


def test_run_convergence_and_errors(env):
    g = load_golden("G10_vb_trajectory_cfg1")
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = g["b"], g["bt"], make_model(env, g["theta0"])
    fit.run()                                        # defaults: max_iters 10, rel_tol 1e-5
    # quirk Q6: e0 > 0 so the first decrease does not stop; e1 < 0 so the next one does (fit.py:138-140)
    assert len(fit.energy) == 3
    nptest.assert_allclose(fit.energy, g["energy"][:3], rtol=1e-10)
    bad = new_fit(env)
    bad.b, bad.bt, bad.model = np.zeros((7, 2)), np.zeros((7, 3)), make_model(env, g["theta0"])
    with pytest.raises(ValueError, match=r"Number of connections \(7\) must be a triangular number."):
        bad.run()
    nomodel = new_fit(env)
    nomodel.b, nomodel.bt = g["b"], g["bt"]
    with pytest.raises(ValueError, match="Model has not been initialized."):
        nomodel.run()


def test_is_converged_cases(env):
    """test_fit.py:86-129."""
    for (e, expect) in (([1, 1.25], True), ([1, 1], True), ([1, 0.501], True), ([1, 0.5], False), ([1, 0.499], False)):
        fit = env.pkg.fit.UnsharedRegionFit()
        fit.rel_tol = 0.5
        fit.energy = e
        assert bool(fit._is_converged(1)) is expect


def test_vb_iteration_cfg2_size_against_c_oracle(env):
    """BASELINE cfg 2 shape (Nreg=64, H=U=16): one full iteration against the C oracle."""
    (N, H, U) = (64, 16, 16)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=2)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    lq_R0 = fit._lq_R
    fit._update_lq_F()
    lq_F = env.CO.update_lq_F(lq_R0, S_B, lM, m.gamma)
    nptest.assert_allclose(fit._lq_F, lq_F, rtol=1e-9, atol=1e-10)
    fit._update_lq_R()
    lq_R = env.CO.update_lq_R(lq_R0, lq_F, lM, m.pi2(), 0)
    nptest.assert_allclose(fit._lq_R, lq_R, rtol=1e-9, atol=1e-10)
    t = env.CO.energy_terms(lq_F, lq_R, S_B, lM, m.gamma, m.pi2())
    nptest.assert_allclose(fit._energy_terms(), t, rtol=1e-10)


def test_update_lps_cost_and_data_contract_cfg3_shape(env):
    """
    VERDICT r3 item 1: _update_lps() is called once per variational iteration (fcdiff/fit.py:75-82) and must cost a
    kernel, not a host digest of b / bt (round 3: CRC-32 of 16 MB per call, 8.6 ms per iteration at cfg3).  Ten calls
    at cfg3's shape, each under 1 ms; and the data contract of `data_check` through the fit itself.
    """
    import time
    (N, H, U) = (200, 50, 50)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    env.torch.cuda.synchronize()
    times = []
    for _ in range(10):
        t0 = time.perf_counter()
        fit._update_lps()
        env.torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert max(times) < 1e-3, times
    lM0 = fit._lM
    # whole-column edit in place: seen by the default sample
    bt[:, 7] = np.clip(bt[:, 7] * 0.5, -1, 1)
    fit._update_lps()
    lM1 = fit._lM
    assert not np.array_equal(lM1[:, 7], lM0[:, 7])
    nptest.assert_array_equal(lM1[:, 8], lM0[:, 8])
    # single-element edit: documented to need invalidate_data() under the default, seen by data_check='full'
    bt[4321, 9] = 0.123456
    fit.invalidate_data()
    fit._update_lps()
    lM2 = fit._lM
    assert not np.array_equal(lM2[4321, 9], lM1[4321, 9])
    fit.data_check = "full"
    fit._update_lps()
    bt[4322, 9] = -0.123456
    fit._update_lps()
    assert not np.array_equal(fit._lM[4322, 9], lM2[4322, 9])
    # rebinding to another array is always seen
    fit.data_check = "none"
    fit.bt = bt.copy()
    fit.bt[0, 0] = 0.5
    fit._update_lps()
    S_B, lM = env.CO.lik_tables(b, fit.bt, m.theta())
    nptest.assert_allclose(fit._lM, lM, **TAB)


# ------------------------------------------------------------------------------------------------
# Gibbs sampler
# ------------------------------------------------------------------------------------------------
def tables_for(env, N, H, U, seed, ideal=False):
    m = env.pkg.UnsharedRegionModel()
    if ideal:
        m.pi, m.epsilon, m.eta = 0.1, 0.01, 0.3
        m.gamma, m.mu, m.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def test_philox_device_equals_oracle(env):
    rs = np.random.RandomState(0)
    ctr = rs.randint(0, 2 ** 32, size=(257, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0] = 0
    ctr[1] = 0xFFFFFFFF
    seed = 0xA4093822299F31D0
    out = env.torch.empty(257 * 2, dtype=env.torch.float64, device="cuda")
    import ctypes
    env.ctx.call("fcd_philox_uniforms", env.lib.dptr(up(env, ctr)), 257, ctypes.c_uint64(seed), env.lib.dptr(out),
                 env.lib.stream_ptr())
    got = out.cpu().numpy().reshape(257, 2)
    for i in range(257):
        for half in range(2):
            assert got[i, half] == env.O.site_uniform(seed, ctr[i, 0], ctr[i, 1], ctr[i, 2], ctr[i, 3], half)
    assert (got >= 0).all() and (got < 1).all()


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("N,U,G,chain0,mode", [(10, 4, 64, 0, "symmetric"), (10, 4, 100, 7, "reference"),
                                                (13, 7, 130, 64, "symmetric"), (5, 1, 1, 0, "symmetric"),
                                                (3, 9, 65, 1, "reference"), (24, 70, 192, 5, "symmetric"),
                                                (2, 3, 64, 0, "symmetric"), (33, 5, 70, 2, "reference"),
                                                (35, 6, 128, 9, "symmetric"), (16, 2, 64, 0, "reference")])
def test_gibbs_chains_equal_oracle_state_for_state(env, N, U, G, chain0, mode, blocked):
    """init + 3 sweeps: every f_c and r_nu of every chain equals the C oracle's (same Philox counters).
    blocked = difference tables (f: 2 log-odds per edge; r: panel + diagonal kernels); else the generic kernels."""
    (m, S_B, lM) = tables_for(env, N, 5, U, seed=N * 100 + U)
    seed = 0x0123456789ABCDEF + N
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=chain0, seed=seed, edge_index=mode, ctx=env.ctx,
                          region_major=blocked)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.25)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.25, seed, chain0)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    emode = env.lib.EDGE_MODES[mode]
    for s in range(3):
        eng.f_step(s)
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, chain0)
        f_g, _ = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        eng.r_step(s)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, emode, chain0)
        _, r_g = eng.export_state()
        nptest.assert_array_equal(r_g, r_o)
    nptest.assert_array_equal(eng.stats().cpu().numpy()[:5], env.CO.gibbs_stats(f_o, r_o)[:5])
    nptest.assert_allclose(eng.logjoint().cpu().numpy(), env.CO.gibbs_logjoint(f_o, r_o, S_B, lM, lng, lnpi2), rtol=1e-12)


@pytest.mark.parametrize("tag", ["cfg1", "mid"])
def test_gibbs_conditionals_against_reference_pins(env, tag):
    """Device conditionals at the fixture's state vs the reference's own one-hot evaluations (G11)."""
    g = load_golden("G11_gibbs_conditionals_" + tag)
    m = make_model(env, g["theta"])
    S_B = g["lp_B_g_F"].sum(axis=1)
    (N, U) = g["r_state"].shape
    G = 3
    f = np.tile(g["f_state"][None], (G, 1))
    r = np.tile(g["r_state"][None], (G, 1, 1))
    for mode in ("reference", "symmetric"):
        eng = env.GibbsEngine(up(env, S_B), up(env, g["lM"]), N, U, G, edge_index=mode, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.import_state(f, r)
        f2, r2 = eng.export_state()
        nptest.assert_array_equal(f2, f)
        nptest.assert_array_equal(r2, r)
        cf, cr = eng.conditionals()
        cf, cr = cf.cpu().numpy(), cr.cpu().numpy()
        for gi in range(G):
            a = cf[gi] - env.O.logsumexp(cf[gi], axis=1)
            nptest.assert_allclose(a, g["cond_f"][:, 0, :], rtol=1e-10, atol=1e-10)       # fit.py:157-174
            if mode == "reference":
                row0 = cr[gi, 0] - env.O.logsumexp(cr[gi, 0], axis=1)
                nptest.assert_allclose(row0, g["lq_R_after_update"][0], rtol=1e-10, atol=1e-10)  # fit.py:176-198
            else:
                nptest.assert_allclose(cr[gi, :, :, 1] - cr[gi, :, :, 0],
                                       g["logjoint_r"][:, :, 1] - g["logjoint_r"][:, :, 0], rtol=1e-8, atol=1e-8)
        nptest.assert_allclose(eng.logjoint().cpu().numpy(), np.full(G, g["logjoint_base"]), rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("kn", [{"r_path": 3}, {"r_path": 3, "r_tol": 1e30}, {"r_path": 3, "r_ub": 1}, {"f_tol": 1e30}, {"f_form": 2},
                                {"f_form": 2, "f_tol": 1e30}, {"f_form": 3}, {"r_path": 3, "r_nopad": 1},
                                {}, {"r_tol": 1e30}, {"r_ub": 1}, {"r_nopad": 1}, {"r_dsplit": 1}, {"r_dsplit": 1, "r_tol": 1e30},
                                {"r_refill": 1}],
                         ids=["step-per-launch", "exact-thresholds", "one-patient", "exact-f-draws", "any-U-f-kernel",
                              "any-U-f-kernel-exact", "scalar-mask-f-kernel", "no-pad",
                              "pipelined", "pipelined-exact", "pipelined-one-patient", "pipelined-no-pad",
                              "pipelined-one-in-order-workgroup", "pipelined-one-in-order-workgroup-exact",
                              "pipelined-sentinels-every-sweep"])
@pytest.mark.parametrize("N,U,G,mode", [(40, 5, 128, "symmetric"), (37, 6, 1024, "reference")])
def test_gibbs_r_pass_forms(env, knobs, kn, N, U, G, mode):
    """
    Both forms of the blocked r pass (pipelined one-launch form with device-side hand-over / one launch per block step),
    the re-decision paths of the fast draws (r_tol / f_tol huge: every r / f draw is repeated with the exact
    logit / exponentials), a one-patient panel and the other forms of the f pass give the oracle's chains: several blocks
    of 16 regions, a partial last block, odd U.  Knobs go through fcd_ctx_set_knob (nothing reads the environment).
    """
    knobs(**kn)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    seed = 5 + N
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=64, seed=seed, edge_index=mode, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, 64)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for s in range(2):
        eng.sweeps(s, 1)
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 64)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES[mode], 64)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


@pytest.mark.gpu
@pytest.mark.parametrize("N,U,G,mode,ub", [(40, 9, 128, "symmetric", 0), (33, 21, 1024, "reference", 0), (70, 12, 200, "symmetric", 1),
                                           (16, 3, 64, "symmetric", 0), (12, 2, 2048, "symmetric", 0), (97, 5, 1024, "symmetric", 0),
                                           (200, 50, 1024, "symmetric", 0)])
def test_gibbs_r_pass_pipelined(env, knobs, N, U, G, mode, ub):
    """
    The default: the blocked r pass in ONE launch whose workgroups hand the redrawn bits / panel sums over through
    marks and sentinels in device memory.  Same chains as the oracle sweep after sweep: odd U, one and two patients per
    panel workgroup, a single block, two groups of chain words, a short last block, and BASELINE cfg 3's full size
    (where the first 64 chains are compared).  The context's error word stays clear (no wait was given up).
    """
    knobs(r_ub=ub)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    seed = 23 + N
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=64, seed=seed, edge_index=mode, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    Go = G if N < 200 else 64
    f_o, r_o = env.CO.gibbs_init(Go, N, U, 0.3, seed, 64)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    n_sw = 3
    eng.run(0, n_sw, mstep_every=0)
    for s in range(n_sw):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 64)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES[mode], 64)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g[:Go], f_o)
    nptest.assert_array_equal(r_g[:Go], r_o)
    assert env.ctx.stat("r_form_last") == 2          # the pipelined kernel itself ran (not its fallback) ...
    assert env.ctx.stat("dev_err") == 0              # ... and no wait was given up (export_state checked it too)


@pytest.mark.gpu
def test_gibbs_r_pass_falls_back_where_the_grid_does_not_fit(env):
    """A grid larger than the device holds at once (cfg5-like: 400 + 16 x 400 workgroups) runs one launch per block step."""
    (N, U, G) = (33, 400, 64)
    (m, S_B, lM) = tables_for(env, N, 2, U, seed=N + U)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=3, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, 3, 0)
    eng.run(0, 1, mstep_every=0)
    env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(m.gamma), 3, 0, 0)
    env.CO.gibbs_r_step(f_o, r_o, lM, np.log(m.pi2()), 3, 0, env.lib.EDGE_MODES["symmetric"], 0)
    f_g, r_g = eng.export_state()
    assert env.ctx.stat("r_form_last") == 1
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


@pytest.mark.gpu
def test_gibbs_pipelined_give_up_is_reported(env):
    """
    A device-side wait that is abandoned must not go unnoticed: with the test hooks r_withhold (the
    in-order role never announces a block) and r_poll_limit (64 polls instead of ~1 s) a panel wave gives its wait up; the
    error word of the context is raised, GibbsEngine refuses to hand out the state, the fit raises instead of returning
    marginals, and every later sampler call on the context returns FCD_ERR_DEVICE until the error is cleared.
    """
    ctx = env.lib.Context()
    ctx.set_knob("r_withhold", 1)
    ctx.set_knob("r_poll_limit", 64)
    (N, U, G) = (40, 6, 128)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=5, ctx=ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    eng.run(0, 2, mstep_every=0)                     # (queued: nothing has looked at the error word yet)
    assert ctx.stat("r_form_last") == 2
    with pytest.raises(env.lib.FcdiffHipError):
        eng.export_state()
    assert ctx.stat("dev_err") != 0
    with pytest.raises(env.lib.FcdiffHipError):
        eng.sweeps(2, 1)
    # the fit: no marginals from such a state
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = ctx
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 3, U, seed=N + U)
    fit.model, fit.b, fit.bt = m, b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in = "gibbs", 128, 3, 1
    ctx.clear_error()
    with pytest.raises(env.lib.FcdiffHipError):
        fit.run()
    # cleared and without the hooks the context works again
    ctx.clear_error()
    ctx.set_knob("r_withhold", 0)
    ctx.set_knob("r_poll_limit", 0)
    eng.init(0.3)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, 5, 0)
    eng.run(0, 1, mstep_every=0)
    env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(m.gamma), 5, 0, 0)
    env.CO.gibbs_r_step(f_o, r_o, lM, np.log(m.pi2()), 5, 0, env.lib.EDGE_MODES["symmetric"], 0)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(r_g, r_o)
    # ... and its pooled accumulators are clean (fcd_ctx_clear_error puts them back to zero; an abandoned
    # call must not leak counts into the next M-step): one more sweep with the M-step inside the tally launch
    c = eng.run(1, 1, mstep_every=1, want_counts=True).cpu().numpy()
    f_g, r_g = eng.export_state()
    assert c[0] == r_g.sum() and c[4] == G and [c[1 + k] for k in range(3)] == [(f_g == k).sum() for k in range(3)]
    (gamma, pi) = eng.hyper_values()
    (pi_h, gamma_h) = env.O.gibbs_mstep(c, N, U)
    nptest.assert_allclose(pi, pi_h, rtol=1e-14)
    nptest.assert_allclose(gamma, gamma_h, rtol=1e-14)
    ctx.close()


@pytest.mark.gpu
def test_gibbs_pipelined_pass_beside_a_foreign_kernel(env):
    """
    The pipelined r pass needs all its workgroups resident at once; the host checks that against an EMPTY device.  Here
    another stream keeps the device busy with large matrix products (tens of milliseconds, every CU) while cfg3-sized
    sweeps are queued: workgroups of the pass that find no slot start late, the others wait for them (bounded polls,
    ~1 s) -- the chains must still be the oracle's and no wait may be given up.
    """
    t = env.torch
    (N, U, G) = (200, 50, 1024)
    (m, S_B, lM) = tables_for(env, N, 2, U, seed=11)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=9, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    Go = 64
    f_o, r_o = env.CO.gibbs_init(Go, N, U, 0.3, 9, 0)
    side = t.cuda.Stream()
    a = t.randn((6144, 6144), device="cuda")
    b = t.randn((6144, 6144), device="cuda")
    t.cuda.synchronize()
    n_sw = 3
    with t.cuda.stream(side):
        for _ in range(12):
            a = (a @ b) * 1e-3
    eng.run(0, n_sw, mstep_every=0)                  # queued while the products run
    with t.cuda.stream(side):
        for _ in range(4):
            a = (a @ b) * 1e-3
    t.cuda.synchronize()
    assert env.ctx.stat("r_form_last") == 2 and env.ctx.stat("dev_err") == 0
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for s in range(n_sw):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, 9, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, 9, s, env.lib.EDGE_MODES["symmetric"], 0)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g[:Go], f_o)
    nptest.assert_array_equal(r_g[:Go], r_o)


@pytest.mark.gpu
@pytest.mark.parametrize("N,U,G,mode", [(17, 1, 64, "symmetric"), (16, 2, 70, "symmetric"), (32, 3, 2048, "symmetric"),
                                        (250, 4, 64, "symmetric"), (33, 7, 1100, "reference"), (3, 2, 64, "symmetric"),
                                        (48, 66, 64, "symmetric"), (100, 17, 1024, "symmetric"),
                                        (20, 250, 128, "symmetric"), (11, 129, 70, "reference"), (9, 321, 64, "symmetric"),
                                        (6, 700, 64, "symmetric")])
def test_gibbs_sweeps_odd_shapes(env, N, U, G, mode):
    """
    Corners of the sweep kernels against the C oracle, two sweeps each: one patient, exactly one block of regions,
    more than 16 chain words (two word groups), 16 blocks of regions, a partial chain word with the reference edge
    ids, three regions, more than 64 patients (the any-U pair kernel of the f pass: tiles of 8, 2, 4, 2 and 1 edges,
    a last slot word of 5, 1 and 15 pairs of patients, odd U), an odd number of patients at 1024 chains.
    """
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=3, seed=5, edge_index=mode, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, 5, 3)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for s in range(2):
        eng.sweeps(s, 1)
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, 5, s, 3)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, 5, s, env.lib.EDGE_MODES[mode], 3)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


def _random_shapes(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        N = int(rng.choice([2, 3, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 90, 120]))
        U = int(rng.choice([1, 2, 3, 4, 5, 8, 11, 16, 23, 37]))
        G = int(rng.choice([64, 70, 128, 200, 512, 1024, 1100, 2048]))
        mode = "reference" if (rng.rand() < 0.3 and N > 2) else "symmetric"
        out.append((N, U, G, mode))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,U,G,mode", _random_shapes(14, 20261004))
def test_gibbs_default_path_random_shapes(env, N, U, G, mode):
    """
    The default path (pair-record f kernel, pipelined one-launch r pass wherever it fits, fused tally) on shapes drawn at
    random from the awkward ones -- two regions, exactly one / just over one / several blocks of 16 regions, one patient,
    odd patient counts, partial chain words, two groups of chain words, both edge-id modes -- against the C oracle,
    three sweeps through fcd_gibbs_run.
    """
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=7 * N + U)
    seed = 1000 + N + U
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=128, seed=seed, edge_index=mode, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, 128)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    eng.run(0, 3, mstep_every=0)
    for s in range(3):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 128)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES[mode], 128)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


@pytest.mark.gpu
def test_gibbs_sweeps_driver_equals_separate_passes(env):
    """
    fcd_gibbs_sweeps (the f pass leaves a square copy of the f state, the r pass packs from it) and the two passes
    called one by one (the r pass gathers from the edge-major state) walk the same chains: 3 sweeps, several blocks
    of regions, a partial chain word.
    """
    (N, U, G) = (45, 7, 200)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=21)
    states = []
    for fused in (True, False):
        eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=8, seed=77, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.25)
        for s in range(3):
            if fused:
                eng.sweeps(s, 1)
            else:
                eng.f_step(s)
                eng.r_step(s)
        states.append(eng.export_state())
    nptest.assert_array_equal(states[0][0], states[1][0])
    nptest.assert_array_equal(states[0][1], states[1][1])


@pytest.mark.parametrize("N,U,G,mode", [(45, 7, 200, "symmetric"), (18, 70, 64, "symmetric"), (33, 5, 130, "reference"),
                                        (32, 3, 2048, "symmetric")])
def test_gibbs_run_equals_call_by_call_loop(env, N, U, G, mode):
    """
    fcd_gibbs_run (one call: per sweep f pass, r pass and ONE tally launch that also carries the M-step and the packed
    r words of the next f pass) against the same loop made of the separate entry points (f step, r step, tally,
    M-step kernel): chains, hyper-parameters, marginal counters and pooled counts must be identical.  Shapes: several
    blocks of regions with a partial chain word, the any-U f kernel, the reference edge ids (no square copy), more than
    16 chain words (two word groups per kernel).
    """
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + 2 * U)
    (n_sweeps, burn) = (5, 2)
    out = []
    for fused in (True, False):
        eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=8, seed=77, edge_index=mode, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.25)
        if fused:
            counts = eng.run(0, n_sweeps, mstep_every=2, accumulate_from=burn, want_counts=True).cpu().numpy().copy()
        else:
            for s in range(n_sweeps):
                eng.f_step(s)
                eng.r_step(s)
                do_m = (s + 1) % 2 == 0
                c = eng.tally(want_counts=True, accumulate=s >= burn)
                if do_m:
                    eng.mstep(c)
            counts = eng.counts.cpu().numpy().copy()
        (f, r) = eng.export_state()
        out.append((f, r, eng.hyper.cpu().numpy().copy(), eng.cnt_f.cpu().numpy().copy(), eng.cnt_r.cpu().numpy().copy(),
                    counts, eng.n_accumulated))
    for (a, b_) in zip(out[0], out[1]):
        nptest.assert_array_equal(a, b_)
    assert out[0][6] == n_sweeps - burn
    assert out[0][5][4] == G and out[0][5][5:].sum() == 0
    # the context's accumulators are back at zero: a second tally gives the same counts again
    again = eng.tally(want_counts=True, accumulate=False).cpu().numpy()
    nptest.assert_array_equal(again, out[1][5])


def test_gibbs_f_pass_fp32_sums_repeat_path(env):
    """
    Round 4: the f pass accumulates its log-odds in fp32 and repeats an edge in fp64 when any lane's draw lies inside the
    error-aware margin.  On WEAK data (two healthy subjects, broad components: the three types stay comparable)
    the margin bites: the repeat path must run (counter f_repeats) and the chains must still be the oracle's, for the
    U <= 64 kernel, the any-U kernel and with every draw forced down the exact path.
    """
    for (N, H, U, G, knob) in [(30, 2, 8, 256, {}), (30, 2, 8, 256, {"f_form": 2}), (12, 2, 70, 128, {}), (30, 2, 8, 256, {"f_tol": 1e30})]:
        m = env.pkg.UnsharedRegionModel()
        m.sigma = np.array([0.2, 0.25, 0.3])
        m.mu = np.array([-0.05, 0.0, 0.05])
        (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U)
        S_B, lM = env.CO.lik_tables(b, bt, m.theta())
        ctx = env.ctx
        for (k, v) in knob.items():
            ctx.set_knob(k, v)
        try:
            eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=17, ctx=ctx)
            eng.set_hyper(m.gamma, m.pi2())
            eng.init(0.3)
            rep0 = ctx.stat("f_repeats")
            eng.sweeps(0, 3)
            reps = ctx.stat("f_repeats") - rep0
        finally:
            for k in knob:
                ctx.set_knob(k, 0)
        f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, 17, 0)
        for s_ in range(3):
            env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(m.gamma), 17, s_, 0)
            env.CO.gibbs_r_step(f_o, r_o, lM, np.log(m.pi2()), 17, s_, env.lib.EDGE_MODES["symmetric"], 0)
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        nptest.assert_array_equal(r_g, r_o)
        wave_edges = 3 * ((G + 63) // 64) * (N * (N - 1) // 2)
        assert reps > 0, (N, U, knob)
        if "f_tol" in knob:
            assert reps == wave_edges                      # every (edge, chain word) went down the exact path


def test_gibbs_chain_sharding_invariance(env):
    """A chain's path depends only on (seed, global chain id): 2 shards of 96 == one run of 192."""
    (N, U, G) = (12, 6, 192)
    (m, S_B, lM) = tables_for(env, N, 4, U, seed=5)
    outs = []
    for (c0, g) in ((0, 192), (0, 96), (96, 96)):
        eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, g, chain0=c0, seed=11, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.1)
        eng.sweeps(0, 4)
        outs.append(eng.export_state())
    nptest.assert_array_equal(outs[0][0], np.concatenate([outs[1][0], outs[2][0]]))
    nptest.assert_array_equal(outs[0][1], np.concatenate([outs[1][1], outs[2][1]]))


def test_gibbs_mstep_and_accumulate(env):
    (N, U, G) = (9, 5, 70)
    (m, S_B, lM) = tables_for(env, N, 4, U, seed=8, ideal=True)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=3, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    cf = np.zeros((eng.C, 3), dtype=np.int64)
    cr = np.zeros((N, U), dtype=np.int64)
    for s in range(3):
        eng.sweeps(s, 1)
        eng.accumulate()
        f, r = eng.export_state()
        for k in range(3):
            cf[:, k] += (f == k).sum(axis=0)
        cr += r.sum(axis=0, dtype=np.int64)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy(), cf)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy(), cr)
    # the fused pass (what the sampler loop calls) = stats() + accumulate()
    ref_counts = eng.stats().cpu().numpy().copy()
    t_counts = eng.tally(want_counts=True, accumulate=True).cpu().numpy()
    nptest.assert_array_equal(t_counts[:5], ref_counts[:5])
    for k in range(3):
        cf[:, k] += (f == k).sum(axis=0)
    cr += r.sum(axis=0, dtype=np.int64)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy(), cf)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy(), cr)
    assert eng.n_accumulated == 4
    counts = eng.stats()
    c = counts.cpu().numpy()
    assert c[4] == G and c[1] + c[2] + c[3] == G * eng.C and c[0] == r.sum()
    eng.mstep(counts)
    (gamma, pi) = eng.hyper_values()
    (pi_h, gamma_h) = env.O.gibbs_mstep(c, N, U)
    nptest.assert_allclose(pi, pi_h, rtol=1e-14)                 # fit.py:213 over chains
    nptest.assert_allclose(gamma, gamma_h, rtol=1e-14)           # fit.py:220 over chains
    nptest.assert_allclose(pi, r.mean(), rtol=1e-14)


def test_fit_gibbs_recovers_planted_structure(env):
    """End to end through UnsharedRegionFit(method='gibbs') on well separated synthetic data."""
    (N, H, U) = (16, 8, 8)
    gen = env.pkg.UnsharedRegionModel()
    gen.pi, gen.epsilon, gen.eta = 0.1, 0.01, 0.3
    gen.gamma, gen.mu, gen.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (r, t, f, ft, b, bt) = gen.sample_fast(N, H, U, seed=4)
    fit = new_fit(env)
    fit.method = "gibbs"
    fit.model = make_model(env, gen.theta())
    fit.b, fit.bt = b, bt
    fit.n_chains, fit.n_sweeps, fit.burn_in, fit.energy_every, fit.trace_every = 128, 40, 10, 10, 2
    fit.run()
    d = fit.diagnostics()                     # per-chain log-joint trace: 128 chains x 15 recorded sweeps
    assert fit.trace.shape == (128, 15) and d["chains"] == 128 and np.isfinite(d["rhat"]) and d["ess"] > 10
    # ... and the number of anomalous sites per chain (the other scalar of SURVEY 8f item 4), equal to a recount
    assert fit.trace_r.shape == (128, 15) and d["sum_r"]["chains"] == 128 and np.isfinite(d["sum_r"]["rhat"])
    (_f_last, r_last) = fit.sampler.export_state()
    nptest.assert_array_equal(fit.sampler.r_sums().cpu().numpy(), r_last.reshape(128, -1).sum(axis=1))
    nptest.assert_array_equal(fit.trace_r[:, -1], r_last.reshape(128, -1).sum(axis=1))
    assert fit._lq_F.shape == (N * (N - 1) // 2, 1, 3) and fit._lq_R.shape == (N, U, 2)
    assert (np.argmax(fit._lq_F[:, 0, :], axis=1) == np.argmax(f, axis=1)).mean() > 0.98
    assert ((np.exp(fit._lq_R[:, :, 1]) > 0.5) == r).mean() > 0.9
    assert len(fit.energy) == 4 and np.all(np.isfinite(fit.energy))
    assert 0 < fit.model.pi < 0.5 and abs(np.sum(fit.model.gamma) - 1) < 1e-12
    # and the variational fit of the same data agrees on the template
    vb = new_fit(env)
    vb.model, vb.b, vb.bt, vb.edge_index = make_model(env, gen.theta()), b, bt, "symmetric"
    vb.rel_tol = -np.inf
    vb.run()
    assert (np.argmax(vb._lq_F[:, 0, :], axis=1) == np.argmax(fit._lq_F[:, 0, :], axis=1)).mean() > 0.98


def test_gibbs_cfg3_size_properties(env):
    """
    BASELINE cfg 3 shape (Nreg=200, H=U=50), 1024 chains, 2 sweeps: EVERY chain equals the C oracle state for state
    (2048 chain-sweeps of the oracle, OpenMP over chains); plus the size-independent properties -- a re-run is bitwise
    identical, a shard equals the matching slice of the full run, pooled counts equal a recount of the exported
    state -- and no entry point allocates once fcd_ctx_reserve has seen the shape.
    """
    (N, H, U, G) = (200, 50, 50, 1024)
    (m, S_B, lM) = tables_for(env, N, H, U, seed=33)
    S_B_d, lM_d = up(env, S_B), up(env, lM)
    seed = 2024

    def run(c0, g):
        eng = env.GibbsEngine(S_B_d, lM_d, N, U, g, chain0=c0, seed=seed, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.05)
        eng.sweeps(0, 2)
        return eng
    rep0 = env.ctx.stat("f_repeats")
    full = run(0, G)
    f_repeats = env.ctx.stat("f_repeats") - rep0          # waves of the f pass that redid an edge's sums in fp64 (2 sweeps)
    n_alloc = env.ctx.stat("n_alloc")
    f_g, r_g = full.export_state()
    again = run(0, G).export_state()
    assert env.ctx.stat("n_alloc") == n_alloc          # second engine at the same shape: no hipMalloc, no sync
    assert np.array_equal(f_g, again[0]) and np.array_equal(r_g, again[1])
    shard = run(640, 128).export_state()
    assert np.array_equal(f_g[640:768], shard[0]) and np.array_equal(r_g[640:768], shard[1])
    c = full.stats().cpu().numpy()
    assert c[0] == r_g.sum() and [c[1], c[2], c[3]] == [(f_g == k).sum() for k in range(3)] and c[4] == G
    # oracle: all 1024 chains
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.05, seed, 0)
    (mf, mr) = (1.0, np.inf)
    for s in range(2):
        mf = min(mf, env.CO.gibbs_f_step_margin(f_o, r_o, S_B, lM, lng, seed, s, 0))
        mr = min(mr, env.CO.gibbs_r_step_margin(f_o, r_o, lM, lnpi2, seed, s, 1, 0))
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    # Tie margins of these 2 x (1024 x 19900 f draws + 1024 x 10000 r draws), from the oracle: the draw that came closest
    # to a tie.  The HIP kernels add the same terms in another order (pairs of patients / of regions, blocks), which moves
    # a sum by a few ulp -- about 200 terms of size <= 50: < 1e-11 absolute for the r draws, < 1e-13 relative to the sum
    # of weights for the f draws.  A draw nearer to its threshold than that could come out differently; the closest one
    # here is orders of magnitude away (and the fast thresholds are re-decided exactly inside 16 x 2e-5 / the f margin).
    margins = {"f_min_rel_distance_to_threshold": mf, "r_min_abs_v": mr, "r_fast_tolerance": 16 * 2e-5,
               "r_min_abs_v_over_fast_tolerance": mr / (16 * 2e-5), "r_sum_rounding_bound": 1e-11,
               "r_min_abs_v_over_rounding_bound": mr / 1e-11, "f_sum_rounding_bound": 1e-13,
               "f_min_over_rounding_bound": mf / 1e-13, "draws_f": 2 * G * (N * (N - 1) // 2), "draws_r": 2 * G * N * U,
               # round 4: the f sums are fp32; a wave repeats an edge in fp64 when a lane's draw lies inside the error-aware margin
               "f_wave_edges": 2 * (G // 64) * (N * (N - 1) // 2), "f_wave_edges_repeated_in_fp64": int(f_repeats),
               "f_repeat_rate": float(f_repeats) / (2 * (G // 64) * (N * (N - 1) // 2))}
    print("tie margins (cfg3, 2 sweeps, 1024 chains):", margins)
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        import json
        with open(os.path.join(out_dir, "tie_margin_cfg3.json"), "w") as fh:
            json.dump(margins, fh, indent=1)
    assert mr > 1e-9 and mf > 1e-11
    assert margins["f_repeat_rate"] < 0.01               # (the floor of the margin alone is ~3e-4 per wave and edge)
    lj = full.logjoint().cpu().numpy()
    nptest.assert_allclose(lj[:8], env.CO.gibbs_logjoint(f_g[:8].copy(), r_g[:8].copy(), S_B, lM, lng, lnpi2), rtol=1e-12)


@pytest.mark.parametrize("N,H,U,G", [(200, 50, 50, 1024),     # cfg3: the U <= 64 pair kernel of the f pass
                                     (100, 20, 80, 512)])     # U > 64: the any-U pair kernel
def test_gibbs_reserve_covers_run_and_sweeps(env, N, H, U, G):
    """
    fcd_ctx_reserve (GibbsEngine.__init__) sizes every scratch buffer of the sweep: on a fresh context, run() with M-step,
    accumulation and counts, then sweeps() with counts, allocate nothing more (no hipMalloc, no synchronisation).
    """
    (m, S_B, lM) = tables_for(env, N, H, U, seed=5)
    fresh = env.lib.Context()
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=77, ctx=fresh)
    assert fresh.stat("ws_bytes") > 1 << 20            # (above the workspace's 1 MiB floor, which would hide a shortfall)
    n_alloc = fresh.stat("n_alloc")
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.05)
    counts = eng.run(0, 3, mstep_every=1, accumulate_from=1, want_counts=True).cpu().numpy()
    assert counts[4] == G
    counts = eng.sweeps(3, 2, with_counts=True).cpu().numpy()
    assert counts[4] == G
    env.torch.cuda.synchronize()
    assert fresh.stat("n_alloc") == n_alloc
    fresh.check_device()


def test_fit_gibbs_cfg3_shape_end_to_end(env):
    """
    VERDICT r3 item 6b: the path bench.py times -- UnsharedRegionFit(method='gibbs').run() -> run_chains -> fcd_gibbs_run with
    accumulation after burn-in and the (pi, gamma) M-step in every sweep's tally launch -- at BASELINE cfg 3's shape with all
    1024 chains, against the C oracle walking the same chains with the oracle's M-step (gibbs_mstep) between sweeps:
    final chain state, marginal counters (a recount from the oracle's chains), pi, gamma and the fit's log-marginals.
    4 sweeps (1 burn-in): 4096 chain-sweeps of the oracle, what the suite's time budget allows.
    """
    (N, H, U, G, n_sweeps, burn) = (200, 50, 50, 1024, 4, 1)
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(N, H, U, seed=21)
    fit = new_fit(env)
    fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.mstep_every, fit.seed = "gibbs", G, n_sweeps, burn, 1, 77
    m0 = env.pkg.UnsharedRegionModel()
    fit.run()
    assert env.ctx.stat("r_form_last") == 2 and env.ctx.stat("dev_err") == 0
    # the oracle's side
    S_B, lM = env.CO.lik_tables(b, bt, m0.theta())
    (gamma, pi) = (np.asarray(m0.gamma, dtype=np.float64), float(m0.pi))
    f_o, r_o = env.CO.gibbs_init(G, N, U, pi, 77, 0)
    C = N * (N - 1) // 2
    cf = np.zeros((C, 3), dtype=np.int64)
    cr = np.zeros((N, U), dtype=np.int64)
    for s_ in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(gamma), 77, s_, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, np.log(np.array([1.0 - pi, pi])), 77, s_, env.lib.EDGE_MODES["symmetric"], 0)
        if s_ >= burn:
            for k in range(3):
                cf[:, k] += (f_o == k).sum(axis=0)
            cr += r_o.sum(axis=0, dtype=np.int64)
        counts = [int(r_o.sum())] + [int((f_o == k).sum()) for k in range(3)] + [G]
        (pi, gamma) = env.O.gibbs_mstep(counts, N, U)
    eng = fit.sampler
    (f_g, r_g) = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy(), cf)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy(), cr)
    assert eng.n_accumulated == n_sweeps - burn
    nptest.assert_allclose(fit.model.pi, pi, rtol=1e-14)
    nptest.assert_allclose(fit.model.gamma, gamma, rtol=1e-14)
    total = float((n_sweeps - burn) * G)
    with np.errstate(divide="ignore"):
        nptest.assert_array_equal(fit._lq_F, np.log(cf.reshape(C, 1, 3) / total))
        p1 = cr / total
        nptest.assert_array_equal(fit._lq_R, np.log(np.stack([1.0 - p1, p1], axis=2)))


@pytest.mark.parametrize("N,U,G", [(40, 6, 1024), (97, 5, 320), (33, 9, 64)])
def test_gibbs_run_keeps_the_sentinels_between_sweeps(env, knobs, N, U, G):
    """
    Inside ONE fcd_gibbs_run call the pipelined r pass's packing launch writes the panel-value sentinels in the first sweep
    only (a completed pass leaves every slot holding its sentinel again; the f pass's slot words live behind the r pass's
    workspace there): five sweeps in one call walk the oracle's chains, as do the same five sweeps with the sentinels
    written every time (knob r_refill) and as five calls of one sweep; no device-side wait is given up.
    """
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + G)
    seed = 31 + N
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, 0)
    for s_ in range(5):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s_, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s_, 1, 0)

    def fresh():
        e = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=seed, ctx=env.ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.3)
        return e
    for mode in ("one call", "refill", "five calls"):
        knobs(r_refill=1 if mode == "refill" else 0)
        e = fresh()
        if mode == "five calls":
            for s_ in range(5):
                e.run(s_, 1, mstep_every=0)
        else:
            e.run(0, 5, mstep_every=0)
        (f_g, r_g) = e.export_state()
        assert env.ctx.stat("dev_err") == 0 and env.ctx.stat("r_form_last") == 2, mode
        nptest.assert_array_equal(f_g, f_o, err_msg=mode)
        nptest.assert_array_equal(r_g, r_o, err_msg=mode)


def test_gibbs_cfg2_full_size_against_oracle(env):
    """BASELINE cfg 2 (Nreg=64, H=U=16, 256 chains): every chain, 2 sweeps, state for state against the C oracle."""
    (N, H, U, G) = (64, 16, 16, 256)
    (m, S_B, lM) = tables_for(env, N, H, U, seed=22)
    seed = 64016
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=seed, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.05)
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.05, seed, 0)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for s in range(2):
        eng.sweeps(s, 1)
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, 1, 0)
    f_g, r_g = eng.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


def test_gibbs_cfg5_full_size(env):
    """
    BASELINE cfg 5, one GPU's share at FULL size: Nreg=400 (C=79 800), H=U=250, 1024 chains.  U > 64 runs the any-U
    pair kernel of the f pass (tiles of 2 edges, 16 slot words per region) with the square copy, the r pass walks 25
    blocks of 16 regions.  Chains 0..31 and 992..1023 equal the C oracle state for state; a shard equals its slice;
    pooled counts equal a recount; the tables equal the oracle's.
    """
    (N, H, U, G) = (400, 250, 250, 1024)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=55)
    fit = new_fit(env)
    fit.b, fit.bt, fit.model = b, bt, m
    fit._init_lps(N, H, U)
    fit._update_lps()
    S_B_d, lM_d = fit._d["S_B"], fit._d["lM"]
    seed = 555

    def run(c0, g):
        eng = env.GibbsEngine(S_B_d, lM_d, N, U, g, chain0=c0, seed=seed, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.05)
        eng.sweeps(0, 1)
        return eng
    full = run(0, G)
    f_g, r_g = full.export_state()
    c = full.stats().cpu().numpy()
    del full
    shard = run(960, 64).export_state()
    assert np.array_equal(f_g[960:], shard[0]) and np.array_equal(r_g[960:], shard[1])
    assert c[0] == r_g.sum(dtype=np.int64) and [c[1], c[2], c[3]] == [(f_g == k).sum() for k in range(3)] and c[4] == G
    S_B, lM = S_B_d.cpu().numpy(), lM_d.cpu().numpy()
    S_Bo, lMo = env.CO.lik_tables(b, bt, m.theta())
    nptest.assert_allclose(lM, lMo, **TAB)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    for c0 in (0, 992):
        f_o, r_o = env.CO.gibbs_init(32, N, U, 0.05, seed, c0)
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, 0, c0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, 0, 1, c0)
        assert np.array_equal(f_g[c0:c0 + 32], f_o) and np.array_equal(r_g[c0:c0 + 32], r_o)


@pytest.mark.parametrize("S,N,T", [(3, 10, 200), (2, 37, 53), (5, 64, 400), (1, 2, 2), (2, 17, 1201), (9, 130, 97), (3, 200, 64),
                                   (2, 257, 40)])
def test_corr_front_end_against_numpy(env, S, N, T):
    """
    K_corr (fp64 MFMA Gram: one block, diagonal / full / partial 64 x 64 blocks, more than eight subjects, odd T) vs
    numpy.corrcoef; oracle is third-party (not in the reference): parity unpinned.
    """
    from fcdiff_amd.corr import correlations
    rs = np.random.RandomState(S * 1000 + N)
    base = rs.standard_normal((S, 1, T))
    ts = rs.standard_normal((S, N, T)) + 0.7 * base          # correlated regions
    ts[:, 0, :] *= 1e3                                        # scale invariance
    if N > 3:
        ts[:, 3, :] = -2.0 * ts[:, 1, :] + 5.0               # exactly anti-correlated pair -> clipped to -1
    got = correlations(ts, ctx=env.ctx)
    exp = env.O.corr_edges(ts)
    assert got.shape == (N * (N - 1) // 2, S)
    nptest.assert_allclose(got, exp, rtol=1e-11, atol=1e-13)
    assert got.min() >= -1.0 and got.max() <= 1.0
    if N > 3 and T > 2:
        z = correlations(ts[:, [0, 2]], fisher_z=True, ctx=env.ctx)
        nptest.assert_allclose(z, env.O.corr_edges(ts[:, [0, 2]], fisher_z=True), rtol=1e-10, atol=1e-13)


def test_corr_cfg3_size(env):
    """The bench's K_corr leg at full size (S = 100 subjects, Nreg = 200, T = 1200) against numpy.corrcoef."""
    from fcdiff_amd.corr import correlations
    (S, N, T) = (100, 200, 1200)
    rs = np.random.RandomState(7)
    ts = rs.standard_normal((S, N, T)) + 0.5 * rs.standard_normal((S, 1, T))
    got = correlations(ts, ctx=env.ctx)
    exp = env.O.corr_edges(ts)
    assert got.shape == (N * (N - 1) // 2, S)
    nptest.assert_allclose(got, exp, rtol=1e-11, atol=1e-13)


def test_corr_cfg5_size(env):
    """
    The block kernel (64 x 64 blocks + moments pass: Nreg = 400 > 208) at BASELINE cfg 5's full size -- S = 500 subjects,
    Nreg = 400, T = 1200, 1.92 GB of series, 79 800 x 500 correlations -- against numpy.corrcoef, subject by subject
    (the bench timed this shape unchecked).  Oracle third-party: parity unpinned by the reference.
    """
    from fcdiff_amd.corr import correlations
    (S, N, T) = (500, 400, 1200)
    rs = np.random.RandomState(5)
    ts = rs.standard_normal((S, N, T))
    ts += 0.5 * rs.standard_normal((S, 1, T))
    ts[:, 7, :] += 300.0                                      # a region far from zero mean
    got = correlations(ts, ctx=env.ctx)
    assert got.shape == (N * (N - 1) // 2, S)
    for s_ in range(S):
        exp = env.O.corr_edges(ts[s_:s_ + 1])
        nptest.assert_allclose(got[:, s_:s_ + 1], exp, rtol=1e-11, atol=1e-13, err_msg="subject %d" % s_)


def test_corr_both_kernels(env, knobs):
    """The one-workgroup-per-subject kernel (centring by the first sample, slices of the time axis meeting in memory) and
    the 64 x 64 block kernel with its moments pass: both against numpy.corrcoef, odd and even T, slices of uneven length,
    a series far from zero mean (what the shift is for), S larger than the number of CUs / 2 (one slice)."""
    from fcdiff_amd.corr import correlations
    rng = np.random.RandomState(12)
    for (S, N, T) in [(7, 50, 333), (3, 200, 1200), (150, 33, 97), (2, 17, 16)]:
        ts = rng.randn(S, N, T) + 1e3 * rng.randn(S, N, 1)
        exp = env.O.corr_edges(ts)
        for form in (0, 1):
            knobs(corr_form=form)
            got = correlations(ts, ctx=env.ctx)
            nptest.assert_allclose(got, exp, rtol=1e-9, atol=1e-12, err_msg="form %d shape %s" % (form, (S, N, T)))


def test_corr_constant_series_gives_nan_like_numpy(env):
    """A region whose series is constant has zero variance: numpy.corrcoef gives NaN for its edges, and so must K_corr
    (round 2 clipped the NaN to -1 through fmin / fmax: ADVICE); every other edge is unaffected."""
    from fcdiff_amd.corr import correlations
    (S, N, T) = (3, 20, 50)
    rs = np.random.RandomState(4)
    ts = rs.standard_normal((S, N, T))
    ts[1, 5, :] = 2.5
    with np.errstate(invalid="ignore", divide="ignore"):
        exp = env.O.corr_edges(ts)
    got = correlations(ts, ctx=env.ctx)
    assert np.isnan(exp).sum() == N - 1 and np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    nptest.assert_allclose(got[ok], exp[ok], rtol=1e-11, atol=1e-13)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = correlations(ts, fisher_z=True, ctx=env.ctx)
    assert np.array_equal(np.isnan(z), np.isnan(exp))


def test_corr_feeds_the_fitter(env):
    """time series -> correlations -> variational fit: the edge order of K_corr is the fitter's."""
    from fcdiff_amd.corr import correlations
    (S, N, T) = (8, 12, 300)
    rs = np.random.RandomState(1)
    ts = rs.standard_normal((S, N, T))
    out = correlations(ts, ctx=env.ctx)
    fit = new_fit(env)
    fit.model = env.pkg.UnsharedRegionModel()
    fit.model.sigma = np.array([0.1, 0.1, 0.1])
    fit.b, fit.bt = out[:, :4].copy(), out[:, 4:].copy()
    fit.max_iters = 2
    fit.run()
    assert len(fit.energy) >= 2 and np.all(np.isfinite(fit.energy))


# ------------------------------------------------------------------------------------------------
# (eta, epsilon) step
# ------------------------------------------------------------------------------------------------
def test_theta_sub_objective_matches_reference_derivative_helpers(env):
    """
    Kernel objective / gradient with W = q_F w_l against the reference's own formulas: E_lM (fit.py:489-511),
    _eval_dE_dh (600-615), _eval_dE_de (644-664) -- the oracle's restatements of those are pinned by fixture G8.
    """
    from fcdiff_amd.fit import theta_sub_objective
    (N, H, U) = (9, 3, 7)
    m = env.pkg.UnsharedRegionModel()
    m.eta, m.epsilon = 0.29, 0.07
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    C = N * (N - 1) // 2
    rs = np.random.RandomState(5)
    q_F = rs.uniform(1e-7, 1, (C, 1, 3))
    q_F /= q_F.sum(axis=2, keepdims=True)
    q_R = rs.uniform(1e-7, 1, (N, U, 2))
    q_R /= q_R.sum(axis=2, keepdims=True)
    fit = new_fit(env)
    fit.model, fit.b, fit.bt = m, b, bt
    fit._init_lps(N, H, U)
    fit._update_lps()
    fit._lq_F, fit._lq_R = np.log(q_F), np.log(q_R)
    W = fit._theta_sub_weights()
    nptest.assert_allclose(W.cpu().numpy(), env.O.vb_weights(q_F, q_R), rtol=1e-13)
    (S, dh, de) = theta_sub_objective(env.ctx, fit._d["bt"], W, m.theta())
    norm = np.stack([env.O.norm_pdf(bt, m.mu[k], m.sigma[k]) for k in range(3)], axis=2)
    mix = np.stack([np.stack([env.O.eval_M(norm, m.eta, m.epsilon, k, l) for l in range(3)], axis=2) for k in range(3)], axis=2)
    nptest.assert_allclose(S, env.O.eval_E_lM(q_F, q_R, np.log(mix)), rtol=1e-11)
    nptest.assert_allclose(-dh, env.O.eval_dE_dh(q_R, q_F, norm, mix, m.epsilon), rtol=1e-10)
    nptest.assert_allclose(-de, env.O.eval_dE_de(q_R, q_F, norm, mix, m.eta), rtol=1e-10)
    # and the gradient is the derivative of the objective (central differences)
    for (j, g) in ((1, dh), (2, de)):
        h = 1e-6
        (tp, tm) = (m.theta(), m.theta())
        tp[j] += h
        tm[j] -= h
        fd = (theta_sub_objective(env.ctx, fit._d["bt"], W, tp)[0] - theta_sub_objective(env.ctx, fit._d["bt"], W, tm)[0]) / (2 * h)
        nptest.assert_allclose(g, fd, rtol=1e-6)


def test_pair_counts_and_mcem_theta_sub(env):
    """Pooled (f, mixture case) counts equal a recount; the MCEM step moves (eta, epsilon) towards the planted values."""
    (N, H, U, G) = (14, 6, 20, 96)
    gen = env.pkg.UnsharedRegionModel()
    gen.pi, gen.eta, gen.epsilon = 0.15, 0.6, 0.08
    gen.gamma, gen.mu, gen.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (r, t, f, ft, b, bt) = gen.sample_fast(N, H, U, seed=9)
    fit = new_fit(env)
    fit.method, fit.b, fit.bt = "gibbs", b, bt
    fit.model = make_model(env, gen.theta())
    fit.model.eta, fit.model.epsilon = 0.3, 0.02                     # start away from the truth
    fit.n_chains, fit.n_sweeps, fit.burn_in = G, 30, 10
    fit.update_theta_sub, fit.theta_sub_every = True, 10
    fit.run()
    eng = fit.sampler
    (f_g, r_g) = eng.export_state()
    nptest.assert_array_equal(eng.pair_counts().cpu().numpy(), env.O.pair_counts(f_g, r_g))
    assert abs(fit.model.eta - 0.6) < abs(0.3 - 0.6) and 1e-5 <= fit.model.eta <= 1 - 1e-5
    assert abs(fit.model.epsilon - 0.08) < abs(0.02 - 0.08) + 0.02


def test_vb_run_with_theta_sub(env):
    """run() with the (eta, epsilon) step enabled: the free energy after the step is not above the one before it."""
    (N, H, U) = (12, 6, 10)
    gen = env.pkg.UnsharedRegionModel()
    gen.pi, gen.eta, gen.epsilon = 0.15, 0.6, 0.08
    gen.gamma, gen.mu, gen.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (r, t, f, ft, b, bt) = gen.sample_fast(N, H, U, seed=2)
    fit = new_fit(env)
    fit.b, fit.bt, fit.edge_index = b, bt, "symmetric"
    fit.model = make_model(env, gen.theta())
    fit.model.eta, fit.model.epsilon = 0.3, 0.02
    fit._init_lps(N, H, U)
    fit._update_lps()
    fit._update_lq_F()
    fit._update_lq_R()
    e0 = fit._eval_energy()
    fit._update_theta_sub()
    assert fit._theta_sub_info.success or fit._theta_sub_info.status in (0, 1, 2)
    fit._update_lps()
    e1 = fit._eval_energy()
    assert e1 <= e0 + 1e-9 * abs(e0)
    assert 1e-5 <= fit.model.eta <= 1 - 1e-5 and 1e-5 <= fit.model.epsilon <= 1 - 1e-5
    full = new_fit(env)
    full.b, full.bt, full.edge_index, full.update_theta_sub = b, bt, "symmetric", True
    full.model = make_model(env, gen.theta())
    full.model.eta, full.model.epsilon = 0.3, 0.02
    full.rel_tol, full.max_iters = -np.inf, 3
    full.run()
    assert len(full.energy) == 4 and np.all(np.isfinite(full.energy))


def test_theta_full_objective_against_oracle_and_differences(env):
    """
    The full theta_sub objective (mu and sigma^2 beside eta, epsilon; SURVEY section 8f item 1, second half): the kernel's
    nine numbers against the oracle's composition of the reference's derivative helpers (pinned by fixture G8:
    _eval_dlN_dm / _eval_dN_dm fit.py:709-719, _eval_dlN_ds / _eval_dN_ds fit.py:721-733, coefficient of fit.py:700-707),
    for VB weights and for chain counts, with and without the healthy-subject term -- and against central differences
    of the objective itself in all eight parameters.
    """
    from fcdiff_amd.fit import theta_full_objective
    (N, H, U) = (9, 4, 7)
    m = env.pkg.UnsharedRegionModel()
    m.eta, m.epsilon = 0.29, 0.07
    m.mu, m.sigma = np.array([-0.2, 0.01, 0.33]), np.array([0.06, 0.08, 0.11])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    C = N * (N - 1) // 2
    rs = np.random.RandomState(5)
    q_F = rs.uniform(1e-7, 1, (C, 1, 3))
    q_F /= q_F.sum(axis=2, keepdims=True)
    q_R = rs.uniform(1e-7, 1, (N, U, 2))
    q_R /= q_R.sum(axis=2, keepdims=True)
    W_vb = env.O.vb_weights(q_F, q_R)
    f = rs.randint(0, 3, (70, C)).astype(np.uint8)
    r = (rs.rand(70, N, U) < 0.3).astype(np.uint8)
    W_ct = env.O.pair_counts(f, r)                               # zeros inside: the w != 0 guards are exercised
    (b_d, bt_d) = (up(env, b), up(env, bt))
    for W in (W_vb, W_ct):
        W_d = up(env, W)
        for with_b in (True, False):
            got = theta_full_objective(env.ctx, b_d if with_b else None, bt_d, W_d, m.theta())
            (S, dh, de, dm, ds) = env.O.theta_full_objective(b if with_b else None, bt, W, m.mu, m.sigma, m.eta, m.epsilon)
            nptest.assert_allclose(got, np.concatenate([[S, dh, de], dm, ds]), rtol=1e-10)
    # the first three numbers without b are fcd_theta_sub_objective's
    from fcdiff_amd.fit import theta_sub_objective
    W_d = up(env, W_vb)
    nptest.assert_allclose(theta_full_objective(env.ctx, None, bt_d, W_d, m.theta())[:3],
                           theta_sub_objective(env.ctx, bt_d, W_d, m.theta()), rtol=1e-12)
    # gradient = derivative of the objective: theta index -> (out9 index, step through sigma^2 for the last three)
    base = np.array(m.theta())
    g = theta_full_objective(env.ctx, b_d, bt_d, W_d, base)

    def S_at(x8):
        th = base.copy()
        th[1], th[2], th[6:9], th[9:12] = x8[0], x8[1], x8[2:5], np.sqrt(x8[5:8])
        return theta_full_objective(env.ctx, b_d, bt_d, W_d, th)[0]
    x = np.concatenate([[m.eta, m.epsilon], m.mu, m.sigma ** 2])
    for i in range(8):
        h = 1e-6 * max(abs(x[i]), 1e-2)
        (xp, xm) = (x.copy(), x.copy())
        xp[i] += h
        xm[i] -= h
        nptest.assert_allclose(g[1 + i], (S_at(xp) - S_at(xm)) / (2 * h), rtol=2e-6)


def test_vb_theta_sub_step_with_mu_sigma(env):
    """
    _update_theta_sub with theta_sub_params='all' (the reference's commented-out intent, fit.py:232-237, 250-251,
    266-267, 282): the free energy after the step is not above the one before it, the parameters respect the
    reference's bounds, and mu / sigma move towards the planted values from a perturbed start.
    """
    (N, H, U) = (12, 8, 10)
    gen = env.pkg.UnsharedRegionModel()
    gen.pi, gen.eta, gen.epsilon = 0.15, 0.6, 0.08
    gen.gamma, gen.mu, gen.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (r, t, f, ft, b, bt) = gen.sample_fast(N, H, U, seed=2)
    fit = new_fit(env)
    fit.b, fit.bt, fit.edge_index = b, bt, "symmetric"
    fit.model = make_model(env, gen.theta())
    fit.model.eta, fit.model.epsilon = 0.3, 0.02
    fit.model.mu, fit.model.sigma = np.array([-0.42, 0.004, 0.43]), np.array([0.08, 0.07, 0.09])
    fit.theta_sub_params = "all"
    fit._init_lps(N, H, U)
    fit._update_lps()
    fit._update_lq_F()
    fit._update_lq_R()
    e0 = fit._eval_energy()
    fit._update_theta_sub()
    assert fit._theta_sub_info.success or fit._theta_sub_info.status in (0, 1, 2)
    fit._update_lps()
    e1 = fit._eval_energy()
    assert e1 <= e0 + 1e-9 * abs(e0)
    (mu, sg) = (np.asarray(fit.model.mu), np.asarray(fit.model.sigma))
    e = 1e-5
    assert -1 + e <= mu[0] <= -e and -e <= mu[1] <= e and e <= mu[2] <= 1 - e and np.all(sg ** 2 >= e)   # fit.py:232-237
    assert abs(mu[0] + 0.5) < 0.08 - 0.02 and abs(mu[2] - 0.5) < 0.07 - 0.02
    assert np.all(np.abs(sg - 0.05) < np.abs(np.array([0.08, 0.07, 0.09]) - 0.05))
    # the whole loop with the full step
    full = new_fit(env)
    full.b, full.bt, full.edge_index, full.update_theta_sub, full.theta_sub_params = b, bt, "symmetric", True, "all"
    full.model = make_model(env, gen.theta())
    full.model.mu, full.model.sigma = np.array([-0.42, 0.004, 0.43]), np.array([0.08, 0.07, 0.09])
    full.rel_tol, full.max_iters = -np.inf, 3
    full.run()
    assert len(full.energy) == 4 and np.all(np.isfinite(full.energy)) and full.energy[-1] <= full.energy[1]


def test_model_sample_gpu_statistics(env):
    """Device forward sampler: the statistical checks of test_fcdiff/test_model.py."""
    m = env.pkg.UnsharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.gamma, m.mu, m.sigma = np.array([0.2, 0.5, 0.3]), np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (N, H, U) = (40, 6, 50)
    (r, t, f, ft, b, bt) = m.sample_gpu(N, H, U, seed=1, ctx=env.ctx)
    C = N * (N - 1) // 2
    assert r.shape == (N, U) and r.dtype == bool and t.shape == (C, U) and f.shape == (C, 3) and ft.shape == (C, U, 3)
    assert b.shape == (C, H) and bt.shape == (C, U) and b.dtype == np.float64
    assert (f.sum(axis=1) == 1).all() and (ft.sum(axis=2) == 1).all() and np.abs(b).max() <= 1 and np.abs(bt).max() <= 1
    nptest.assert_allclose(r.mean(), 0.3, atol=0.03)
    nptest.assert_allclose(f.mean(axis=0), m.gamma, atol=0.05)
    ends = np.array([env.pkg.c_to_nm(c) for c in range(C)])
    rn, rm = r[ends[:, 0]], r[ends[:, 1]]
    assert t[rn & rm].all() and not t[~rn & ~rm].any()
    nptest.assert_allclose(t[rn ^ rm].mean(), 0.4, atol=0.03)
    fk, ftk = np.argmax(f, axis=1), np.argmax(ft, axis=2)
    same = ftk == fk[:, None]
    nptest.assert_allclose(same[~t].mean(), 0.8, atol=0.02)
    nptest.assert_allclose(same[t].mean(), 0.2, atol=0.03)
    for k in range(3):
        other = ftk[(fk == k)[:, None] & ~same]
        counts = np.bincount(other, minlength=3)
        assert counts[k] == 0 and abs(counts[(k + 1) % 3] / counts.sum() - 0.5) < 0.05       # the two others equally
        nptest.assert_allclose(b[fk == k].mean(), m.mu[k], atol=0.02)
        nptest.assert_allclose(b[fk == k].std(), m.sigma[k], atol=0.02)
        nptest.assert_allclose(bt[ftk == k].mean(), m.mu[k], atol=0.02)
        nptest.assert_allclose(bt[ftk == k].std(), m.sigma[k], atol=0.02)
    again = m.sample_gpu(N, H, U, seed=1, ctx=env.ctx)
    other_seed = m.sample_gpu(N, H, U, seed=2, ctx=env.ctx)
    assert all(np.array_equal(a, c) for a, c in zip((r, t, f, ft, b, bt), again))
    assert not np.array_equal(bt, other_seed[5])
