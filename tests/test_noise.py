"""
Per-subject measurement noise without a GPU: the NumPy reference of the noise tables (noise_ref.py) against the sessions
reference at zero variance and against a brute-force product of densities, the host refusals (all before any device
work), corr.sampling_variance, the C ABI, and the scenario that motivates the feature on the reference alone.
"""
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import missing_data_ref as MD
import noise_ref as NR
import sessions_ref as SR
import fcdiff_amd
from conftest import theta_dict
from fcdiff_amd import _lib, corr, tables
from oracle import fcdiff_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcdiff_hip.h")
NAMES = ("fcd_lik_tables_noise", "fcd_lik_shared_tables_noise", "fcd_conn_posterior_noise")


def problem(K, N=4, H=5, U=5, seed=3):
    """A 6 x 5 problem of K sessions (broad sigmas: no density of a session underflows), with variances of both sides."""
    m = fcdiff_amd.UnsharedRegionModel()
    m.mu, m.sigma = np.array([-0.3, 0.0, 0.3]), np.array([0.2, 0.25, 0.3])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed, sessions=K)
    rng = np.random.default_rng(seed + 100)
    (var_b, var_bt) = (rng.uniform(0, 0.02, H), rng.uniform(0, 0.02, (U, K)))
    var_b[1] = 0.0
    var_bt[2, :] = 0.0
    return m, b, bt, var_b, var_bt


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 5])
def test_reference_at_zero_variance_is_the_sessions_reference(K):
    (m, b, bt, var_b, var_bt) = problem(K)
    (S0, lM0) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    for (vb, vbt) in ((None, None), (np.zeros_like(var_b), np.zeros_like(var_bt)), (None, np.zeros(bt.shape[1]))):
        (S_B, lM) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, vb, vbt)
        nptest.assert_allclose(S_B, S0, rtol=1e-12)
        nptest.assert_allclose(lM, lM0, rtol=1e-12)
    if K == 1:
        # a 2-D bt is one session
        (S2, lM2) = NR.lik_tables(b, bt[:, :, 0], m.mu, m.sigma, m.eta, m.epsilon, var_b, var_bt[:, 0])
        (S3, lM3) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, var_b, var_bt)
        nptest.assert_array_equal(S2, S3)
        nptest.assert_array_equal(lM2, lM3)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_reference_is_the_log_of_the_brute_force_product(K):
    """ln M of missing_data_ref.enumerate_law with like = prod_k N(x_k; mu_j, sigma_j^2 + v_uk) written out, item by item; S_B
    likewise from the densities of b."""
    (m, b, bt, var_b, var_bt) = problem(K, seed=20 + K)
    (S_B, lM) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, var_b, var_bt)
    want = np.zeros_like(lM)
    for c in range(bt.shape[0]):
        for u in range(bt.shape[1]):
            like = NR.product_like(bt[c, u], m.mu, m.sigma, var_bt[u])
            assert like.min() > 1e-250
            want[c, u] = np.log(MD.enumerate_law(m.eta, m.epsilon, like=like)[0])
    nptest.assert_allclose(lM, want, **NR.tolerance(bt, m.mu, m.sigma, var_bt))
    S_want = np.zeros_like(S_B)
    for c in range(b.shape[0]):
        for h in range(b.shape[1]):
            S_want[c] += np.log(NR.product_like(b[c, h:h + 1], m.mu, m.sigma, var_b[h:h + 1]))
    nptest.assert_allclose(S_B, S_want, rtol=1e-12, atol=1e-12)
    # the variances matter: the table without them is another table
    (_S, lM_plain) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    assert np.abs(lM - lM_plain).max() > 1e-3


def test_a_one_dimensional_variance_applies_to_every_session():
    (m, b, bt, _vb, var_bt) = problem(3)
    v = var_bt[:, 0].copy()
    (_S, lM1) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, None, v)
    (_S, lM2) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, None, np.repeat(v[:, None], 3, axis=1))
    nptest.assert_array_equal(lM1, lM2)


@pytest.mark.parametrize("where", [0, 2, 4])
def test_nan_session_leaves_the_reference_bit_identical(where):
    (m, b, bt, var_b, var_bt) = problem(4)
    (_S, want) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, var_b, var_bt, missing=True)
    btn = np.insert(bt, where, np.nan, axis=2)
    vn = np.insert(var_bt, where, 0.0173, axis=1)
    (_S, got) = NR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, var_b, vn, missing=True)
    nptest.assert_array_equal(got, want)
    btn[2, 1, :] = np.nan
    (_S, got) = NR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, var_b, vn, missing=True)
    assert np.all(got[2, 1] == 0.0)


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_noise_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert "int64_t K" in args and "int flags" in args and "const double *var_bt" in args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    assert _lib.ABI_VERSION == 4


def test_library_exports_the_noise_entry_points():
    import ctypes as C
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name


def test_the_record_placement_constant_is_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "fcd_lik_sessions.hip")).read()
    m = re.search(r"#define\s+FCD_NOISE_LDS_RECORDS\s+(\d+)", src)
    assert m and int(m.group(1)) == tables.NOISE_LDS_RECORDS


# ------------------------------------------------------------------------------------------------
# host refusals: all of them before any device work (no context exists here)
# ------------------------------------------------------------------------------------------------
def noise_fit(cls=None, K=None, **kw):
    (m, b, bt, var_b, var_bt) = problem(1 if K is None else K)
    fit = (cls or fcdiff_amd.fit.UnsharedRegionFit)()
    (fit.model, fit.b, fit.bt) = (m, b, bt[:, :, 0] if K is None else bt)
    (fit.b_noise_var, fit.bt_noise_var) = (var_b, var_bt[:, 0] if K is None else var_bt)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


def untouched(fit):
    return fit._ctx is None and fit._query_ctx is None and fit._d == {}


CLASSES = [fcdiff_amd.fit.UnsharedRegionFit, fcdiff_amd.fit.SharedRegionFit]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("K", [None, 3])
@pytest.mark.parametrize("bad", ["shape_b", "shape_bt", "shape_bt_2d", "negative", "nan", "inf", "inf_b"])
def test_bad_noise_variances_are_refused_before_any_context(cls, K, bad):
    fit = noise_fit(cls, K)
    (H, U, Kn) = (5, 5, 1 if K is None else K)
    if bad == "shape_b":
        fit.b_noise_var = np.zeros(H + 1)
    elif bad == "shape_bt":
        fit.bt_noise_var = np.zeros(U + 1)
    elif bad == "shape_bt_2d":
        fit.bt_noise_var = np.zeros((U, Kn + 1))
    elif bad == "inf_b":
        fit.b_noise_var = np.array([0.0, 0.01, np.inf, 0.0, 0.0])
    else:
        v = np.full((U, Kn), 0.01)
        v[3, Kn - 1] = {"negative": -1e-6, "nan": np.nan, "inf": np.inf}[bad]
        fit.bt_noise_var = v
    for method in ("vb", "gibbs"):
        fit.method = method
        with pytest.raises(ValueError, match="noise"):
            fit.run()
    with pytest.raises(ValueError, match="noise"):
        fit._update_lps()
    assert untouched(fit)


def test_good_noise_variances_pass_the_host_check():
    for K in (None, 3):
        fit = noise_fit(K=K)
        (vb, vbt) = fit._noise_host()
        assert vb.shape == (5,) and vbt.shape == (5, 1 if K is None else K)
        fit.bt_noise_var = np.arange(5) * 0.01               # (U,): every session
        (_vb, vbt) = fit._noise_host()
        nptest.assert_array_equal(vbt, np.repeat((np.arange(5) * 0.01)[:, None], 1 if K is None else K, axis=1))
        (fit.b_noise_var, fit.bt_noise_var) = (None, None)
        assert fit._noise_host() is None and not fit._has_noise()
        assert untouched(fit)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("which", ["b", "bt", "both"])
@pytest.mark.parametrize("knobs", [{"update_theta_sub": True}, {"theta_sub_every": 2},
                                   {"update_theta_sub": True, "theta_sub_params": "all"}])
def test_theta_sub_with_noise_is_refused_before_any_launch(cls, which, knobs):
    fit = noise_fit(cls, **knobs)
    if which == "b":
        fit.bt_noise_var = None
    elif which == "bt":
        fit.b_noise_var = None
    for method in ("vb", "gibbs"):
        fit.method = method
        with pytest.raises(NotImplementedError, match="noise"):
            fit.run()
    with pytest.raises(NotImplementedError, match="noise"):
        fit._update_theta_sub()
    assert untouched(fit)


class FakeSampler:
    (C, G, chain0) = (6, 64, 0)


@pytest.mark.parametrize("cls", CLASSES)
def test_membership_with_noise_is_refused(cls):
    fit = noise_fit(cls, method="gibbs", edge_index="symmetric")
    fit.sampler = FakeSampler()
    with pytest.raises(NotImplementedError, match="noise"):
        fit.membership(np.zeros((6, 2)))
    assert untouched(fit)


def test_p_Bt_g_Ft_with_noise_is_refused():
    import torch
    fit = noise_fit()
    with pytest.raises(ValueError, match="_p_Bt_g_Ft"):
        fit._p_Bt_g_Ft
    assert untouched(fit)
    z = torch.zeros((3, 2), dtype=torch.float64)
    theta = fcdiff_amd.UnsharedRegionModel().theta()
    with pytest.raises(ValueError, match="p_Bt_g_Ft"):
        tables.build(None, z, z, theta, 0, pBt=torch.zeros((3, 2, 3)), noise=(None, torch.zeros(2, dtype=torch.float64)))
    with pytest.raises(ValueError, match="noise"):
        tables.build(None, z, z, theta, 0, noise=(torch.zeros(3, dtype=torch.float64), None))
    with pytest.raises(ValueError, match="noise"):
        tables.build(None, z, z[:, :, None], theta, 0, noise=(None, torch.zeros(2, dtype=torch.float64)))


def test_score_of_a_noise_fit_needs_the_new_patients_variances():
    fit = noise_fit(method="gibbs", edge_index="symmetric")
    fit.sampler = FakeSampler()
    with pytest.raises(ValueError, match="noise_var"):
        fit.score(np.zeros((6, 2)))
    for bad in (np.zeros(3), np.array([0.01, -0.01]), np.array([0.01, np.inf]), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="noise"):
            fit.score(np.zeros((6, 2)), noise_var=bad)
    with pytest.raises(ValueError, match="noise"):
        fit.score(np.zeros((6, 2, 3)), noise_var=np.zeros((2, 2)))
    assert untouched(fit)


# ------------------------------------------------------------------------------------------------
# corr.sampling_variance
# ------------------------------------------------------------------------------------------------
def test_sampling_variance_on_a_hand_made_info():
    info = np.array([[400, 6, 393], [60, 6, 53], [10, 6, 3], [9, 6, 2], [7, 6, 0], [5, 6, -2]])
    raw = corr.sampling_variance(info)
    z = corr.sampling_variance(info, fisher_z=True)
    assert raw.dtype == np.float64 and raw.shape == (6,)
    nptest.assert_array_equal(raw, [1 / 393, 1 / 53, 1 / 3, 1 / 2, np.inf, np.inf])
    nptest.assert_array_equal(z, [1 / 391, 1 / 51, 1.0, np.inf, np.inf, np.inf])
    # 1 / dof is the rho = 0 value of (1 - rho^2)^2 / dof: an upper bound over rho
    rho = np.linspace(-0.99, 0.99, 199)
    assert np.all((1 - rho ** 2) ** 2 / 53 <= raw[1] + 1e-18)
    doc = corr.sampling_variance.__doc__
    assert "upper bound" in doc.lower() and "autocorrelation" in doc and "effective" in doc
    with pytest.raises(ValueError):
        corr.sampling_variance(np.zeros((3, 2)))
    # a finite variance goes into a fit, an infinite one is refused there
    fit = noise_fit()
    fit.bt_noise_var = raw[:5]
    with pytest.raises(ValueError, match="noise"):
        fit.run()
    assert untouched(fit)


# ------------------------------------------------------------------------------------------------
# the scenario: half the patients measured with more noise
# ------------------------------------------------------------------------------------------------
def test_scenario_noise_ignored_looks_anomalous_noise_given_does_not():
    """
    noise_ref.SCENARIO on the reference alone, 8 VB iterations: the share of the noisy patients' healthy regions that are
    flagged is >= 0.15 with the noise ignored and <= 0.05 with the variances given, and >= 0.6 of their truly anomalous
    regions (17) are still found.  With the symmetric edge ids the figures are 30/111 = 0.270, 2/111 = 0.018 and 14/17 = 0.82
    (15/17 = 0.88 found with the noise ignored).  With the reference implementation's own edge ids (`reference`, its quirk
    Q1) the same data give 0.279 / 0.090 and 0.71 / 0.71: the <= 0.05 bound is a statement about the model, met under the
    ids of the documented maths, and this test runs those.
    """
    m = fcdiff_amd.UnsharedRegionModel()
    m.pi = NR.SCENARIO["pi"]
    (b, bt, r, var_bt) = NR.scenario_data(m)
    assert int(r[:, NR.SCENARIO["first_noisy"]:].sum()) == 17
    start = theta_dict(m.theta())
    ignored = NR.vb_fit(b, bt, start, NR.SCENARIO["iters"], O.EDGE_SYMMETRIC)
    given = NR.vb_fit(b, bt, start, NR.SCENARIO["iters"], O.EDGE_SYMMETRIC, var_bt=var_bt)
    (fp0, hit0) = NR.scenario_rates(ignored["lq_R"], r)
    (fp1, hit1) = NR.scenario_rates(given["lq_R"], r)
    print("noise ignored: fp %.3f hits %.3f pi %.3f;  noise given: fp %.3f hits %.3f pi %.3f"
          % (fp0, hit0, ignored["theta"]["pi"], fp1, hit1, given["theta"]["pi"]))
    assert fp0 >= 0.15
    assert fp1 <= 0.05
    assert hit1 >= 0.6
    # the figures quoted in README.md
    assert (round(fp0, 3), round(fp1, 3), round(hit0, 2), round(hit1, 2)) == (0.270, 0.018, 0.88, 0.82)
