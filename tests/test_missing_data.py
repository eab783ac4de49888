"""
NaN as unobserved data (UnsharedRegionFit.missing_data), without a GPU: the C ABI declares what the binding binds, and
the law behind the rule -- an unobserved bt has M_kl = 1 and leaves T and F~ at their prior law given (k, l).
"""
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as R
import missing_data_ref as MD
from fcdiff_amd import _lib
from fcdiff_amd.fit import _eval_M

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcdiff_hip.h")
EX = ("fcd_lik_tables_ex", "fcd_theta_sub_objective_ex", "fcd_theta_full_objective_ex", "fcd_conn_posterior_ex")

# (eta, epsilon) over the optimiser's box (fit.py:228-231) and the model's defaults
GRID = [(eta, eps) for eta in (1e-5, 0.01, 0.3, 0.5, 0.7, 0.99, 1 - 1e-5) for eps in (1e-5, 0.001, 0.02, 0.1, 0.5, 0.93, 1 - 1e-5)]


def test_header_and_binding_agree_on_the_flag_and_the_ex_entry_points():
    text = open(HEADER).read()
    flags = dict(re.findall(r"#define (FCD_DATA_[A-Z_]+) (\d+)", text))
    assert flags == {"FCD_DATA_NAN_MISSING": "1"}
    assert _lib.FCD_DATA_NAN_MISSING == 1
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in EX:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, decl)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert "int flags" in args, name
        assert len(_lib.SIGNATURES[name][1]) == len(args), name
        # the _ex form is the plain form plus `int flags` (and, for the tables, the counter pointer)
        plain = _lib.SIGNATURES[name[:-3]][1]
        assert len(args) == len(plain) + (2 if name == "fcd_lik_tables_ex" else 1), name
    assert _lib.ABI_VERSION == 4 and "#define FCD_ABI_VERSION 4" in text


def test_library_exports_the_ex_entry_points():
    import ctypes as C
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = C.CDLL(_lib.LIB_PATH)
    for name in EX:
        assert hasattr(raw, name), name


@pytest.mark.parametrize("eta,epsilon", GRID)
def test_unit_likelihood_gives_M_equal_one(eta, epsilon):
    """M_kl with N_j = 1 for every j is 1 for every (k, l): the fitter's own _eval_M to 2 ulp, and the enumeration."""
    N = np.ones((1, 1, 3))
    for k in range(3):
        for l in range(3):
            M = float(_eval_M(N, eta, epsilon, k, l)[0, 0])
            assert abs(M - 1.0) <= 2 * np.spacing(1.0), (k, l, M)
    (M, _pT, _pF, _pch) = MD.enumerate_law(eta, epsilon)
    nptest.assert_allclose(M, 1.0, rtol=0, atol=2 * np.spacing(1.0))


@pytest.mark.parametrize("eta,epsilon", GRID)
def test_prior_law_of_T_and_F_tilde(eta, epsilon):
    """
    With an unobserved bt the law of (T, F~) given (k, l) is the generative model's: P(T = 1) = (0, 1, eta)[l], P(F~ = k)
    = e_l, the two others (1 - e_l)/2 each.  The enumeration agrees with those forms and with the closed forms of
    conn_posterior_ref at a unit likelihood (equal mu and sigma make every relative density exactly 1).
    """
    (pT, pF, pch) = MD.prior_law([0.1, eta, epsilon, 0.3, 0.4, 0.3, 0.0, 0.0, 0.0, 0.2, 0.2, 0.2])
    e = R.eps_l(eta, epsilon)
    for k in range(3):
        for l in range(3):
            assert pT[k, l] == pytest.approx((0.0, 1.0, eta)[l], rel=1e-15, abs=1e-16)
            for j in range(3):
                assert pF[k, l, j] == pytest.approx(e[l] if j == k else (1 - e[l]) / 2, rel=1e-14, abs=1e-16)
            assert pch[k, l] == pytest.approx(1 - e[l], rel=1e-12, abs=1e-16)      # (1 - e_l cancels)
    theta = np.array([0.1, eta, epsilon, 0.3, 0.4, 0.3, 0.1, 0.1, 0.1, 0.25, 0.25, 0.25])
    assert np.all(R.rel_densities(np.array([0.37]), theta[6:9], theta[9:12]) == 1.0)
    (rT, rF, rch) = R.tables(np.array([0.37]), theta)
    nptest.assert_allclose(rT[0], pT, rtol=1e-14, atol=1e-16)
    nptest.assert_allclose(rF[0], pF, rtol=1e-14, atol=1e-16)
    nptest.assert_allclose(rch[0], pch, rtol=1e-13, atol=1e-16)


def test_enumeration_reproduces_the_closed_forms_at_observed_bt():
    """The same enumeration with the Normal likelihood of an observed bt gives conn_posterior_ref's tables (so the
    unit-likelihood case above is the same model, with only the likelihood changed)."""
    theta = np.array([0.1, 0.3, 0.07, 0.3, 0.4, 0.3, -0.2, 0.0, 0.25, 0.05, 0.07, 0.09])
    for x in (-0.3, -0.05, 0.0, 0.11, 0.4):
        like = R.rel_densities(np.array([x]), theta[6:9], theta[9:12])[0]
        (_M, pT, pF, pch) = MD.enumerate_law(theta[1], theta[2], like)
        (rT, rF, rch) = R.tables(np.array([x]), theta)
        nptest.assert_allclose(pT, rT[0], rtol=1e-12, atol=1e-300)
        nptest.assert_allclose(pF, rF[0], rtol=1e-12, atol=1e-300)
        nptest.assert_allclose(pch, rch[0], rtol=1e-11, atol=1e-300)


def test_masked_oracle_tables_follow_the_rule():
    """The test-side masking of the NumPy oracle: a NaN b drops out of S_B exactly as a removed column does."""
    rng = np.random.default_rng(3)
    (C, H, U) = (10, 6, 4)
    (b, bt) = (rng.uniform(-0.6, 0.6, (C, H)), rng.uniform(-0.6, 0.6, (C, U)))
    (mu, sigma) = (np.array([-0.2, 0.0, 0.25]), np.array([0.1, 0.12, 0.15]))
    bn = b.copy()
    bn[:, 2] = np.nan
    btn = bt.copy()
    btn[3, 1] = np.nan
    (S_B, lpB, pBt, lM) = MD.masked_lik_tables(bn, btn, mu, sigma, 0.3, 0.02)
    (lpB_d, _pBt, lM_d) = O_tables(np.delete(b, 2, axis=1), bt, mu, sigma)
    nptest.assert_allclose(S_B, lpB_d.sum(axis=1), rtol=1e-14)
    assert np.all(lpB[:, 2] == 0.0) and np.all(pBt[3, 1] == 1.0) and np.all(lM[3, 1] == 0.0)
    keep = np.ones((C, U), dtype=bool)
    keep[3, 1] = False
    assert np.array_equal(lM[keep], lM_d[keep])


def O_tables(b, bt, mu, sigma):
    from oracle import fcdiff_oracle as O
    return O.lik_tables(b, bt, mu, sigma, 0.3, 0.02)
