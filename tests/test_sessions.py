"""
Repeated sessions per patient, bt (C, U, K), without a GPU: the NumPy reference of the sessions tables (sessions_ref.py)
against the oracle's 2-D table and against the brute-force law over (T, F~), the C ABI, the host refusals and the
sessions argument of UnsharedRegionModel.sample_fast.
"""
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import missing_data_ref as MD
import sessions_ref as SR
import fcdiff_amd
from fcdiff_amd import _lib, tables
from oracle import fcdiff_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcdiff_hip.h")
NAMES = ("fcd_lik_tables_sessions", "fcd_lik_shared_tables_sessions", "fcd_conn_posterior_sessions")


def problem(K, N=4, H=5, U=5, seed=3):
    """A 6 x 5 problem of K sessions (broad sigmas: no density of a session underflows)."""
    m = fcdiff_amd.UnsharedRegionModel()
    m.mu, m.sigma = np.array([-0.3, 0.0, 0.3]), np.array([0.2, 0.25, 0.3])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed, sessions=K)
    return m, b, bt


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_reference_at_one_session_is_the_oracle_table():
    (m, b, bt) = problem(1)
    (S_B, lM) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    (lpB, _pBt, lM2) = O.lik_tables(b, bt[:, :, 0], m.mu, m.sigma, m.eta, m.epsilon)
    nptest.assert_array_equal(S_B, O.sum_lp_B(lpB))
    nptest.assert_allclose(lM, lM2, **SR.tolerance(bt, m.mu, m.sigma))


@pytest.mark.parametrize("K", range(1, 9))
def test_reference_is_the_log_of_the_enumerated_law(K):
    """ln M of missing_data_ref.enumerate_law with like = prod_k N_j, item by item."""
    (m, b, bt) = problem(K, seed=10 + K)
    (_S_B, lM) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    want = np.zeros_like(lM)
    for c in range(bt.shape[0]):
        for u in range(bt.shape[1]):
            like = SR.product_like(bt[c, u], m.mu, m.sigma)
            assert like.min() > 1e-250                      # (the product itself is representable in this problem)
            want[c, u] = np.log(MD.enumerate_law(m.eta, m.epsilon, like=like)[0])
    nptest.assert_allclose(lM, want, **SR.tolerance(bt, m.mu, m.sigma))


@pytest.mark.parametrize("where", [0, 2, 4])
def test_nan_session_leaves_the_reference_bit_identical(where):
    (m, b, bt) = problem(4)
    (_S, want) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, missing=True)
    btn = np.insert(bt, where, np.nan, axis=2)
    assert btn.shape[2] == 5
    (_S, got) = SR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, missing=True)
    nptest.assert_array_equal(got, want)
    # no observed session: exactly 0; without the rule the item is NaN
    btn[2, 1, :] = np.nan
    (_S, got) = SR.lik_tables(b, btn, m.mu, m.sigma, m.eta, m.epsilon, missing=True)
    assert np.all(got[2, 1] == 0.0)
    (_S, off) = SR.lik_tables(b, btn[:, :, 1:] if where == 0 else btn[:, :, :4], m.mu, m.sigma, m.eta, m.epsilon)
    assert np.all(np.isnan(off[2, 1]))


def test_reference_is_finite_where_the_product_underflows():
    m = fcdiff_amd.UnsharedRegionModel()
    m.mu, m.sigma = np.array([-0.5, 0.0, 0.5]), np.array([0.05, 0.05, 0.05])
    bt = np.ones((3, 2, 16))
    (a, _n) = SR.session_log_sums(bt, m.mu, m.sigma)
    assert a.max() <= -766 and np.all(SR.product_like(bt[0, 0], m.mu, m.sigma) == 0.0)
    (_S, lM) = SR.lik_tables(np.zeros((3, 2)), bt, m.mu, m.sigma, m.eta, m.epsilon)
    assert np.all(np.isfinite(lM)) and -775 < lM.max() < -765


# ------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_sessions_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert "int64_t K" in args and "int flags" in args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(args), name
    assert _lib.ABI_VERSION == 4


def test_library_exports_the_sessions_entry_points():
    import ctypes as C
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name


# ------------------------------------------------------------------------------------------------
# host refusals: all of them before any device work (no context exists here)
# ------------------------------------------------------------------------------------------------
def sessions_fit(cls=None, K=3):
    (m, b, bt) = problem(K)
    fit = (cls or fcdiff_amd.fit.UnsharedRegionFit)()
    (fit.model, fit.b, fit.bt) = (m, b, bt)
    return fit


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("knobs", [{"update_theta_sub": True}, {"theta_sub_every": 2},
                                   {"update_theta_sub": True, "theta_sub_params": "all"}])
def test_theta_sub_with_sessions_is_refused_before_any_launch(shared, knobs):
    fit = sessions_fit(fcdiff_amd.fit.SharedRegionFit if shared else None)
    for (k, v) in knobs.items():
        setattr(fit, k, v)
    for method in ("vb", "gibbs"):
        fit.method = method
        with pytest.raises(NotImplementedError, match="theta_sub"):
            fit.run()
    with pytest.raises(NotImplementedError, match="theta_sub"):
        fit._update_theta_sub()
    assert fit._ctx is None and fit._d == {}


def test_n_sessions():
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    assert fit.n_sessions == 1
    fit.bt = np.zeros((3, 4))
    assert fit.n_sessions == 1
    fit.bt = np.zeros((3, 4, 5))
    assert fit.n_sessions == 5
    with pytest.raises(AttributeError):
        fit.n_sessions = 2


def test_membership_refuses_three_dimensions():
    class Sampler:
        C = 6
    for cls in (fcdiff_amd.fit.UnsharedRegionFit, fcdiff_amd.fit.SharedRegionFit):
        fit = sessions_fit(cls)
        (fit.method, fit.sampler) = ("gibbs", Sampler())
        with pytest.raises(ValueError, match="x_new must be"):
            fit.membership(np.zeros((6, 2, 3)))
        assert fit._ctx is None and fit._query_ctx is None


def test_tables_build_refuses_pBt_and_zero_sessions():
    import torch
    b = torch.zeros((3, 2), dtype=torch.float64)
    theta = fcdiff_amd.UnsharedRegionModel().theta()
    with pytest.raises(ValueError, match="p_Bt_g_Ft"):
        tables.build(None, b, torch.zeros((3, 2, 2), dtype=torch.float64), theta, 0, pBt=torch.zeros((3, 2, 3)))
    for shared in (False, True):
        with pytest.raises(ValueError, match="K >= 1"):
            tables.build(None, b, torch.zeros((3, 2, 0), dtype=torch.float64), theta, 0, shared=shared)
    with pytest.raises(ValueError, match=r"\(C, U\) or \(C, U, K\)"):
        tables.build(None, b, torch.zeros((3, 2, 2, 2), dtype=torch.float64), theta, 0)
    # the fit's own property, and run() with K = 0
    fit = sessions_fit()
    with pytest.raises(ValueError, match="_p_Bt_g_Ft"):
        fit._p_Bt_g_Ft
    fit.bt = np.zeros((6, 5, 0))
    with pytest.raises(ValueError, match="K >= 1"):
        fit.run()
    assert fit._ctx is None


def test_data_digest_visits_every_session_of_every_patient():
    """The strided sample of a (C, U, K) array sees an edit of any one (patient, session) column."""
    digest = fcdiff_amd.fit.UnsharedRegionFit._data_digest
    rng = np.random.default_rng(0)
    a = rng.standard_normal((300, 8, 6))                       # 14 400 elements: the sampled mode
    base = digest(a, "sample")
    for u in range(8):
        for k in range(6):
            e = a.copy()
            e[:, u, k] += 1.0
            assert digest(e, "sample") != base, (u, k)
    # a 2-D array is digested as before: the stride is coprime to U
    a2 = rng.standard_normal((3000, 6))
    step = max(1, a2.size // 4096)
    while np.gcd(step, 6) != 1:
        step += 1
    import zlib
    flat = a2.reshape(-1)
    assert digest(a2, "sample") == (zlib.crc32(np.ascontiguousarray(flat[::step]).view(np.uint8))
                                    ^ zlib.crc32(flat[-64:].view(np.uint8)))


# ------------------------------------------------------------------------------------------------
# sample_fast(sessions=...)
# ------------------------------------------------------------------------------------------------
def test_sample_fast_without_sessions_draws_what_it_always_drew():
    """sessions=None against the draw stream written out here (PCG64 of the seed, the order of the draws fixed)."""
    m = fcdiff_amd.UnsharedRegionModel()
    (N, H, U, seed) = (9, 4, 7, 11)
    out = m.sample_fast(N, H, U, seed=seed)
    again = m.sample_fast(N, H, U, seed=seed, sessions=None)
    g = np.random.default_rng(seed)
    C = N * (N - 1) // 2
    il = np.tril_indices(N, -1)
    r = g.random((N, U)) < m.pi
    (rn, rm) = (r[il[0], :], r[il[1], :])
    t = np.where(rn ^ rm, g.random((C, U)) < m.eta, rn & rm)
    fk = g.choice(3, size=C, p=m.gamma / m.gamma.sum())
    keep = np.where(t, g.random((C, U)) < m.epsilon, g.random((C, U)) < (1 - m.epsilon))
    other = (fk[:, None] + 1 + (g.random((C, U)) < 0.5)) % 3
    ftk = np.where(keep, fk[:, None], other)
    b = (m.mu[fk][:, None] + m.sigma[fk][:, None] * g.standard_normal((C, H))).clip(-1, 1)
    bt = (m.mu[ftk] + m.sigma[ftk] * g.standard_normal((C, U))).clip(-1, 1)
    for (got, got2, want) in zip(out, again, (r, t, np.eye(3, dtype=bool)[fk], np.eye(3, dtype=bool)[ftk], b, bt)):
        nptest.assert_array_equal(got, want)
        nptest.assert_array_equal(got2, want)
    assert out[5].shape == (C, U)


def test_sample_fast_sessions_share_the_patients_state():
    m = fcdiff_amd.UnsharedRegionModel()
    m.pi, m.epsilon, m.eta = 0.3, 0.2, 0.4
    m.gamma, m.mu, m.sigma = np.ones(3) / 3, np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (N, H, U, K) = (40, 6, 50, 4)
    (r, t, f, ft, b, bt) = m.sample_fast(N, H, U, seed=1, sessions=K)
    C = N * (N - 1) // 2
    assert bt.shape == (C, U, K) and bt.dtype == np.float64 and np.abs(bt).max() <= 1
    assert ft.shape == (C, U, 3) and b.shape == (C, H)
    # everything before bt is the draw of sessions=None
    for (x, y) in zip((r, t, f, ft, b), m.sample_fast(N, H, U, seed=1)):
        nptest.assert_array_equal(x, y)
    ftk = np.argmax(ft, axis=2)
    for k in range(3):
        x = bt[ftk == k]                                        # (items, K): every session at the item's own type
        nptest.assert_allclose(x.mean(axis=0), m.mu[k], atol=0.02)
        nptest.assert_allclose(x.std(axis=0), m.sigma[k], atol=0.02)
        # all sessions of an item sit at the same type (types are 10 sigma apart) ...
        assert np.all(np.abs(x - m.mu[k]) < 6 * m.sigma[k])
        # ... and are independent given it
        cc = np.corrcoef((x - m.mu[k]).T)
        assert np.abs(cc - np.eye(K)).max() < 0.03
    with pytest.raises(ValueError):
        m.sample_fast(N, H, U, sessions=0)
