"""
Anomalous-region counts without a GPU: the NumPy restatement of tests/count_posterior_ref.py against brute force, the new
C-ABI symbols and their host-side refusals, and the defaults and refusals of UnsharedRegionFit.anomaly_count_posterior().
"""
import itertools

import numpy as np
import numpy.testing as nptest
import pytest

import count_posterior_ref as R
from fcdiff_amd import _lib


@pytest.mark.parametrize("N", [1, 2, 5, 9, 12])
def test_poisson_binomial_equals_enumeration(N):
    rng = np.random.default_rng(N)
    q1 = rng.uniform(0, 1, N)
    q1[::4] = 0.0
    q1[1::5] = 1.0
    q0 = 1.0 - q1
    want = np.zeros(N + 1)
    for bits in itertools.product((0, 1), repeat=N):
        b = np.array(bits)
        want[b.sum()] += np.prod(np.where(b == 1, q1, q0))
    got = R.poisson_binomial(q0, q1)
    nptest.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
    nptest.assert_allclose(got.sum(), 1.0, rtol=0, atol=1e-14)


def test_poisson_binomial_point_masses():
    q1 = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    got = R.poisson_binomial(1.0 - q1, q1)
    assert np.array_equal(got, np.eye(6)[3])
    # from log-weights that are not normalised, with log 0 = -inf
    with np.errstate(divide="ignore"):
        lq = np.log(np.stack([1.0 - q1, q1], axis=1)) + 3.0
    (q0, q1b) = R.q_of(lq)
    assert np.array_equal(q1b, q1) and np.array_equal(q0, 1.0 - q1)


def test_count_posterior_rows_and_layout():
    rng = np.random.default_rng(4)
    (N, U) = (6, 4)
    lq = rng.normal(0, 2, (N, U, 2))
    (pp, pr) = R.count_posterior(lq)
    assert pp.shape == (U, N + 1) and pr.shape == (N, U + 1)
    nptest.assert_allclose(pp.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(pr.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    (q0, q1) = R.q_of(lq)
    # the means are the sums of the marginals
    nptest.assert_allclose(pp @ np.arange(N + 1), q1.sum(axis=0), rtol=1e-13)
    nptest.assert_allclose(pr @ np.arange(U + 1), q1.sum(axis=1), rtol=1e-13)


@pytest.mark.parametrize("G,N,U", [(1, 2, 1), (37, 6, 4), (130, 9, 70), (64, 13, 3)])
def test_histograms_equal_explicit_loops(G, N, U):
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.1, 0.9)).astype(np.uint8)
    (hp, hr) = R.histograms(r)
    want_p = np.zeros((U, N + 1), dtype=np.int64)
    want_r = np.zeros((N, U + 1), dtype=np.int64)
    for g in range(G):
        for u in range(U):
            want_p[u, int(sum(r[g, n, u] for n in range(N)))] += 1
        for n in range(N):
            want_r[n, int(sum(r[g, n, u] for u in range(U)))] += 1
    assert np.array_equal(hp, want_p) and np.array_equal(hr, want_r)


def test_new_symbols_load_and_abi_stays_4():
    lib = _lib.load()
    for name in ("fcd_gibbs_count_tally", "fcd_gibbs_set_count_accumulator", "fcd_vb_count_posterior"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fcd_abi_version() == _lib.ABI_VERSION == 4
    # host-side argument checks: no context, no device work
    assert lib.fcd_gibbs_set_count_accumulator(None, None, None, 4, 2, 1) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_count_tally(None, None, 4, 2, 64, None, None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_vb_count_posterior(None, None, 4, 2, None, None, None) == _lib.FCD_ERR_ARG


def test_fit_defaults_and_refusals_without_a_run():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    assert fit.anomaly_counts is False and fit.anomaly_counts_every == 1
    assert fit.patient_count_hist is None and fit.region_count_hist is None and fit.anomaly_count_sweeps == 0
    with pytest.raises(ValueError):
        fit.anomaly_count_posterior()                        # no model, no data
    fit.model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fit.model.sample_fast(5, 3, 2, seed=1)
    (fit.b, fit.bt) = (b, bt)
    with pytest.raises(ValueError):
        fit.anomaly_count_posterior()                        # vb without a run: no _lq_R
    fit.method = "gibbs"
    with pytest.raises(ValueError):
        fit.anomaly_count_posterior()                        # gibbs without anomaly_counts
    fit.patient_count_hist = np.zeros((2, 6), dtype=np.int64)
    fit.region_count_hist = np.zeros((5, 3), dtype=np.int64)
    with pytest.raises(ValueError):
        fit.anomaly_count_posterior()                        # no sweep accumulated
    fit.patient_count_hist[:, 1] = 8
    fit.region_count_hist[:, 2] = 8
    out = fit.anomaly_count_posterior()
    assert np.array_equal(out["p_patient_count"], np.eye(6)[[1, 1]]) and np.array_equal(out["p_patient_any"], [1.0, 1.0])
    assert np.array_equal(out["p_region_count"], np.eye(3)[[2] * 5]) and np.array_equal(out["p_region_any"], np.ones(5))


@pytest.mark.parametrize("every", [0, -1, 1.5])
def test_fit_refuses_bad_every_before_the_run(every):
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit.anomaly_counts, fit.anomaly_counts_every) = (True, every)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 2)                                  # refused before any engine or device state is made


def test_fit_refuses_overflow_before_the_run():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit.anomaly_counts, fit.n_chains, fit.n_sweeps, fit.burn_in) = (True, 1 << 22, 2000, 0)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 2)


def test_engine_run_refuses_overflow():
    """GibbsEngine.run's bound, checked on a stand-in that has only what the check reads."""
    from fcdiff_amd.gibbs import GibbsEngine
    eng = GibbsEngine.__new__(GibbsEngine)
    (eng.G, eng.pair_acc, eng.count_hist, eng.count_every, eng.count_sweeps) = (1 << 22, None, (None, None), 1, 0)
    with pytest.raises(ValueError):
        eng.run(0, 2000, accumulate_from=0)
