"""
membership() on the host: the NumPy reference of its two per-chain sums against the explicit enumeration of the
shared-region model, the declaration and binding of its kernel, what it refuses, the pooling over ranks and the formulas of
the Bayes factor.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import numpy.testing as nptest
import pytest

import fcdiff_amd
from fcdiff_amd import _lib, membership, score
from conftest import ROOT

import membership_ref as MR
import score_ref as R
import shared_region_ref as SR


def small_case(N, H, U, seed):
    m = fcdiff_amd.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.sigma = np.array([0.15, 0.15, 0.2])
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=seed)
    return m, b, bt


@pytest.mark.parametrize("missing", [False, True])
def test_reference_against_enumeration(missing):
    """
    N = 4 (C = 6).  A new patient of the shared model is one more column of bt, a new control one more column of b, so
        log p(x | data, patient) = log_evidence(b, [bt, x]) - log_evidence(b, bt)
        log p(x | data, control) = log_evidence([b, x], bt) - log_evidence(b, bt)
    with log_evidence from shared_region_ref.enumerate_posterior, which sums T and F~ explicitly: the reference's lp and lc,
    averaged over the enumerated posterior of (f, r), must give the same numbers.
    """
    (m, b, bt) = small_case(4, 2, 3, seed=5)
    th = m.theta()
    (_r, _t, _f, _ft, _b, x_new) = m.sample(4, 1, 2, seed=8)
    if missing:
        (bt, x_new) = (bt.copy(), x_new.copy())
        bt[1, 0] = np.nan
        x_new[2, 1] = np.nan
    base = SR.enumerate_posterior(b, bt, th, missing=missing)["log_evidence"]
    got = MR.exact_shared(b, bt, th, x_new, missing=missing)
    for u in range(x_new.shape[1]):
        col = x_new[:, u:u + 1]
        as_patient = SR.enumerate_posterior(b, np.concatenate([bt, col], axis=1), th, missing=missing)["log_evidence"] - base
        as_control = SR.enumerate_posterior(np.concatenate([b, col], axis=1), bt, th, missing=missing)["log_evidence"] - base
        nptest.assert_allclose(got["log_patient"][u], as_patient, rtol=1e-10)
        nptest.assert_allclose(got["log_control"][u], as_control, rtol=1e-10)
    assert np.all(got["rel_patient"] > 0) and np.all(got["rel_control"] > 0)


def test_reference_r_per_subject_and_oracle_tables():
    """r (G, N, U) with equal columns gives what r (G, N) gives; the mixture logs are the oracle's lM; a NaN adds 0."""
    from oracle import fcdiff_oracle as O
    rng = np.random.default_rng(3)
    (m, b, bt) = small_case(5, 2, 4, seed=2)
    th = m.theta()
    nptest.assert_allclose(MR.mixture_logs(bt, th), O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)[2], rtol=1e-12)
    f = rng.integers(0, 3, size=(7, 10))
    r = rng.integers(0, 2, size=(7, 5))
    one = MR.patient_loglik(bt, th, f, r)
    nptest.assert_array_equal(one, MR.patient_loglik(bt, th, f, np.repeat(r[:, :, None], 4, axis=2)))
    for g in range(7):
        for u in range(4):
            lM_u = MR.mixture_logs(bt, th)[:, u]
            want = R.log_joint_r(lM_u, f[g], r[g], 0.5) - 5 * np.log(0.5)
            nptest.assert_allclose(one[g, u], want, rtol=1e-12)
    x = bt.copy()
    x[:, 1] = np.nan
    assert np.all(MR.patient_loglik(x, th, f, r, missing=True)[:, 1] == 0.0)
    assert np.all(MR.control_loglik(x, th, f, missing=True)[:, 1] == 0.0)
    assert np.all(np.isnan(MR.control_loglik(x, th, f)[:, 1]))


def test_header_and_binding_declare_the_kernel():
    text = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int\s+fcd_member_loglik\s*\(([^;]*)\)\s*;", text)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 13 and args[0].startswith("fcd_ctx") and "r_cols" in args[8] and "flags" in args[9]
    (res, argtypes) = _lib.SIGNATURES["fcd_member_loglik"]
    assert res is C.c_int and len(argtypes) == 13
    assert argtypes[2] == C.POINTER(C.c_double) and argtypes[8] is C.c_int and argtypes[9] is C.c_int
    assert hasattr(C.CDLL(_lib.LIB_PATH), "fcd_member_loglik")
    assert _lib.ABI_VERSION == 4


def fake_fitted(cls, C_edges=6):
    """A fit that looks fitted to the host-side checks (they run before anything touches a device)."""
    fit = cls()
    fit.model = fcdiff_amd.SharedRegionModel() if cls is fcdiff_amd.fit.SharedRegionFit else fcdiff_amd.UnsharedRegionModel()
    fit.method = "gibbs"
    fit.sampler = types.SimpleNamespace(C=C_edges, G=64)
    return fit


@pytest.mark.parametrize("cls", [fcdiff_amd.fit.UnsharedRegionFit, fcdiff_amd.fit.SharedRegionFit])
def test_refusals(cls):
    x = np.zeros((6, 2))
    fit = cls()
    fit.model = fcdiff_amd.UnsharedRegionModel()
    fit.method = "gibbs"
    with pytest.raises(ValueError, match="run"):                       # before run()
        fit.membership(x)
    fit = fake_fitted(cls)
    fit.method = "vb"
    with pytest.raises(ValueError, match="bound"):                     # mean-field q: a difference of bounds is not a bound
        fit.membership(x)
    fit = fake_fitted(cls)
    with pytest.raises(ValueError, match="connections"):               # wrong C
        fit.membership(np.zeros((10, 2)))
    with pytest.raises(ValueError, match=r"\(C, U'\)"):                 # not 2-D
        fit.membership(np.zeros(6))
    with pytest.raises(ValueError, match=r"\(C, U'\)"):
        fit.membership(np.zeros((6, 2, 1)))
    fit.edge_index = "reference"
    with pytest.raises(ValueError, match="symmetric"):
        fit.membership(x)


def test_shared_score_still_not_provided():
    with pytest.raises(NotImplementedError):
        fcdiff_amd.fit.SharedRegionFit().score(np.zeros((6, 1)))


def test_pooling_ranks_equals_pooling_all_chains():
    """Three ranks' parts (of unequal size, one with a chain at -inf) pool to what the concatenated chains give."""
    rng = np.random.default_rng(11)
    U = 4
    lp = rng.normal(size=(300, U)) * np.array([0.1, 2.0, 20.0, 1.0]) - 50.0
    lc = rng.normal(size=(300, U)) * 3.0 - 80.0
    lp[7, 3] = -np.inf
    cuts = [(0, 64), (64, 200), (200, 300)]
    both = membership.pool(np.stack([R.ais_parts(lp)]), np.stack([R.ais_parts(lc)]))
    split = membership.pool(np.stack([R.ais_parts(lp[a:b]) for (a, b) in cuts]),
                            np.stack([R.ais_parts(lc[a:b]) for (a, b) in cuts]))
    assert both["n_chains"] == split["n_chains"] == 300
    for key in ("log_patient", "log_patient_se", "ess_patient", "log_control", "log_control_se", "ess_control", "log_bf",
                "log_bf_se"):
        assert both[key].shape == (U,) and both[key].dtype == np.float64
        nptest.assert_allclose(split[key], both[key], rtol=1e-12)
    # ... and those are the plain formulas on all chains
    w = np.exp(lp - lp.max(axis=0))
    nptest.assert_allclose(both["log_patient"], lp.max(axis=0) + np.log(w.mean(axis=0)), rtol=1e-13)
    nptest.assert_allclose(both["ess_patient"], w.sum(axis=0) ** 2 / (w * w).sum(axis=0), rtol=1e-12)
    nptest.assert_allclose(both["log_patient_se"], w.std(axis=0, ddof=1) / np.sqrt(300) / w.mean(axis=0), rtol=1e-10)


def test_bayes_factor_formulas():
    rng = np.random.default_rng(2)
    lp = rng.normal(size=(128, 3)) - 10.0
    lc = rng.normal(size=(128, 3)) - 12.0
    out = membership.pool(R.ais_parts(lp)[None], R.ais_parts(lc)[None])
    (p, sp, _e) = score.pool_ais(R.ais_parts(lp)[None])
    (c, sc, _e) = score.pool_ais(R.ais_parts(lc)[None])
    nptest.assert_array_equal(out["log_bf"], p - c)
    nptest.assert_array_equal(out["log_bf_se"], np.sqrt(sp * sp + sc * sc))
    nptest.assert_array_equal(out["log_patient"], p)
    nptest.assert_array_equal(out["log_control"], c)
    assert "covariance" in fcdiff_amd.fit.UnsharedRegionFit.membership.__doc__


def test_chunks_cover_the_cohort():
    assert membership.chunks(1) == [(0, 1)]
    assert membership.chunks(membership.CHUNK) == [(0, membership.CHUNK)]
    assert membership.chunks(membership.CHUNK + 1) == [(0, membership.CHUNK), (membership.CHUNK, membership.CHUNK + 1)]
    assert membership.chunks(7, 3) == [(0, 3), (3, 6), (6, 7)]
