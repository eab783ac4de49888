"""
The shared-region model on the host: the reduction of its collapsed joint to the unshared model at one patient, the
law of SharedRegionModel.sample, and what SharedRegionFit refuses.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import fcdiff_amd
from fcdiff_amd import util
from oracle import fcdiff_oracle as O

import shared_region_ref as SR


def small_case(N, H, U, seed, missing=False):
    m = fcdiff_amd.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.1
    m.sigma = np.array([0.06, 0.06, 0.08])
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=seed)
    if missing:
        bt = bt.copy()
        bt[0, 0] = np.nan
    return m, b, bt


@pytest.mark.parametrize("N,H,U,missing", [(3, 2, 3, False), (4, 1, 2, False), (3, 2, 2, True)])
def test_enumeration_equals_collapsed_joint_of_summed_tables(N, H, U, missing):
    """Summing T and F~ explicitly gives the collapsed joint built from Sum_u of the oracle's lM (the U = 1 reduction)."""
    (m, b, bt) = small_case(N, H, U, seed=N + 10 * U, missing=missing)
    th = m.theta()
    ex = SR.enumerate_posterior(b, bt, th, missing=missing)
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    if missing:
        lM[np.isnan(bt)] = 0.0
    S_B = lpB.sum(axis=1)
    L = lM.sum(axis=1)
    lj = SR.collapsed_logjoint(S_B, L, th, N)
    nptest.assert_allclose(ex["logjoint"], lj, rtol=0, atol=1e-12 * np.abs(lj).max())
    assert abs(ex["p_r"].sum() - (ex["p_count"] * np.arange(N + 1)).sum()) < 1e-12
    nptest.assert_allclose(ex["p_f"].sum(axis=1), 1.0, atol=1e-12)


def test_sample_has_the_models_law():
    m = fcdiff_amd.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.gamma, m.mu, m.sigma = np.array([0.2, 0.5, 0.3]), np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    (N, H, U) = (200, 4, 60)
    (r, t, f, ft, b, bt) = m.sample(N, H, U, seed=3)
    C = util.N_to_C(N)
    assert r.shape == (N,) and r.dtype == bool and t.shape == (C, U) and f.shape == (C, 3) and ft.shape == (C, U, 3)
    assert b.shape == (C, H) and bt.shape == (C, U)
    nptest.assert_allclose(r.mean(), 0.3, atol=5 * np.sqrt(0.21 / N))
    ends = np.array([util.c_to_nm(c) for c in range(C)])
    rn, rm = r[ends[:, 0]], r[ends[:, 1]]
    assert t[rn & rm].all() and not t[~rn & ~rm].any()          # concordant pairs, in every patient
    nptest.assert_allclose(t[rn ^ rm].mean(), 0.4, atol=0.01)
    fk, ftk = np.argmax(f, axis=1), np.argmax(ft, axis=2)
    same = ftk == fk[:, None]
    nptest.assert_allclose(same[~t].mean(), 0.8, atol=0.01)
    nptest.assert_allclose(same[t].mean(), 0.2, atol=0.01)
    nptest.assert_allclose(f.mean(axis=0), m.gamma, atol=0.02)
    for k in range(3):
        nptest.assert_allclose(b[fk == k].mean(), m.mu[k], atol=0.01)
        nptest.assert_allclose(bt[ftk == k].mean(), m.mu[k], atol=0.01)
    again = m.sample(N, H, U, seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(again, (r, t, f, ft, b, bt)))


def test_fit_refuses_reference_edges_and_score():
    fit = fcdiff_amd.fit.SharedRegionFit()
    fit.edge_index = "reference"
    with pytest.raises(ValueError):
        fit._edge_mode()
    fit.model = fcdiff_amd.SharedRegionModel()
    (fit.b, fit.bt) = (np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        fit.run()
    fit.edge_index = None
    assert fit._edge_mode() == "symmetric"
    with pytest.raises(NotImplementedError):
        fit.score(np.zeros((3, 2)))


def test_fit_without_gpu_raises_like_the_unshared_fit():
    """No GPU or no library: SharedRegionFit.run() raises what UnsharedRegionFit.run() raises (with one, both run)."""
    def outcome(fit, model):
        fit.model = model
        (_r, _t, _f, _ft, fit.b, fit.bt) = fcdiff_amd.SharedRegionModel().sample(4, 2, 3)
        fit.edge_index = "symmetric"
        fit.max_iters = 1
        try:
            fit.run()
        except Exception as e:          # noqa: BLE001 -- the type is what is compared
            return type(e)
        return None
    unshared = outcome(fcdiff_amd.fit.UnsharedRegionFit(), fcdiff_amd.UnsharedRegionModel())
    shared = outcome(fcdiff_amd.fit.SharedRegionFit(), fcdiff_amd.SharedRegionModel())
    assert shared is unshared
