"""
Co-anomaly without a GPU: the NumPy restatement of tests/coanomaly_ref.py against brute force, its identities with the
anomalous-region counts, the gap between the exact joint and the product of the exact marginals that the GPU test leans
on, the host normalisation of coanomaly_posterior(), the new C-ABI symbols and the refusals that need no device.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import coanomaly_ref as R
import count_posterior_ref as CR
import exact_law_cases as X
from fcdiff_amd import _lib
from oracle.exact_chain import ExactChain


def random_state(G, N, U, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)


@pytest.mark.parametrize("G,N,U", [(1, 2, 1), (37, 6, 4), (70, 5, 9), (64, 7, 3)])
def test_pair_counts_equal_explicit_loops(G, N, U):
    r = random_state(G, N, U, G + N + U)
    (rp, pp) = R.pair_counts(r)
    want_r = np.zeros((N, N), dtype=np.int64)
    want_p = np.zeros((U, U), dtype=np.int64)
    for g in range(G):
        for n in range(N):
            for m in range(N):
                want_r[n, m] += sum(int(r[g, n, u]) & int(r[g, m, u]) for u in range(U))
        for u in range(U):
            for v in range(U):
                want_p[u, v] += sum(int(r[g, n, u]) & int(r[g, n, v]) for n in range(N))
    assert np.array_equal(rp, want_r) and np.array_equal(pp, want_p)
    assert np.array_equal(rp, rp.T) and np.array_equal(pp, pp.T)


@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (64, 13, 3), (200, 40, 1)])
def test_identities_with_the_counts(G, N, U):
    """Diagonals are the marginal counters' sums; the totals are the second moments of the count histograms."""
    r = random_state(G, N, U, 7 * G + N + U)
    (rp, pp) = R.pair_counts(r)
    cnt_r = r.astype(np.int64).sum(axis=0)                       # (N, U): the marginal counter of one state
    nptest.assert_array_equal(np.diag(rp), cnt_r.sum(axis=1))
    nptest.assert_array_equal(np.diag(pp), cnt_r.sum(axis=0))
    (hp, hr) = CR.histograms(r)
    assert rp.sum() == int((hp * np.arange(N + 1) ** 2).sum())   # sum_{g,u} (sum_n r)^2
    assert pp.sum() == int((hr * np.arange(U + 1) ** 2).sum())   # sum_{g,n} (sum_u r)^2


def test_independent_form_against_loops():
    rng = np.random.default_rng(3)
    (N, U) = (5, 4)
    q1 = rng.uniform(0, 1, (N, U))
    q1[0, 1] = 0.0
    q1[2, 3] = 1.0
    with np.errstate(divide="ignore"):
        lq = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))
    (reg, pat) = R.independent(lq)
    for n in range(N):
        for m in range(N):
            want = sum(q1[n, u] if n == m else q1[n, u] * q1[m, u] for u in range(U))
            nptest.assert_allclose(reg[n, m], want, rtol=1e-13)
    for u in range(U):
        for v in range(U):
            want = sum(q1[n, u] if u == v else q1[n, u] * q1[n, v] for n in range(N))
            nptest.assert_allclose(pat[u, v], want, rtol=1e-13)


def test_exact_joint_is_not_the_product_of_its_marginals():
    """In "3x2-strong" some entry of the exact joint lies further from the independence form than the tolerance the GPU
    test holds the sampler to: passing there tells the joint from the product."""
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem("3x2-strong")
    (region, patient, q1) = R.exact_moments(ExactChain(S_B, lM, gamma, pi2))
    (ind_r, ind_p) = R.independent_from_marginals(q1)
    tol = 5 * 0.5 / np.sqrt(X.G_CHAINS) + 1e-4
    gap = max(np.abs(region - ind_r).max(), np.abs(patient - ind_p).max())
    print("3x2-strong: largest |joint - independent| = %.3e, tolerance %.3e" % (gap, tol))
    assert gap > tol
    # the diagonals are the marginals' means in both forms
    nptest.assert_allclose(np.diag(region), q1.mean(axis=1), rtol=1e-13)
    nptest.assert_allclose(np.diag(patient), q1.mean(axis=0), rtol=1e-13)
    nptest.assert_allclose(np.diag(ind_r), q1.mean(axis=1), rtol=1e-13)


def test_host_normalisation():
    from fcdiff_amd.fit import coanomaly_from_counts
    r = random_state(96, 6, 5, 11)
    (rp, pp) = R.pair_counts(r)
    sweeps = 3
    out = coanomaly_from_counts(3 * rp, 3 * pp, 96 * sweeps)
    want = R.posterior_from_counts(3 * rp, 3 * pp, 96 * sweeps)
    assert sorted(out) == sorted(want)
    for k in want:
        assert out[k].dtype == np.float64
        nptest.assert_allclose(out[k], want[k], rtol=1e-15)
    rf = r.astype(np.float64)
    nptest.assert_allclose(out["p_region_pair"], np.einsum("gnu,gmu->nm", rf, rf) / (96 * 5), rtol=1e-14)
    nptest.assert_allclose(out["expected_regions"], np.einsum("gnu,gnv->uv", rf, rf) / 96, rtol=1e-14)
    assert out["p_region_pair"].max() <= 1.0 and out["p_patient_pair"].max() <= 1.0
    with pytest.raises(ValueError):
        coanomaly_from_counts(rp, pp, 0)
    with pytest.raises(ValueError):
        coanomaly_from_counts(rp[:, :3], pp, 96)


def test_new_symbols_load_and_abi_stays_4():
    lib = _lib.load()
    for name in ("fcd_gibbs_coanomaly_tally", "fcd_gibbs_set_coanomaly_accumulator", "fcd_vb_coanomaly"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fcd_abi_version() == _lib.ABI_VERSION == 4
    # host-side argument checks: no context, no device work
    assert lib.fcd_gibbs_set_coanomaly_accumulator(None, None, None, 4, 2, 1) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_coanomaly_tally(None, None, 4, 2, 64, None, None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_vb_coanomaly(None, None, 4, 2, None, None, None) == _lib.FCD_ERR_ARG


def test_fit_defaults_and_refusals_without_a_run():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    assert fit.coanomaly is False and fit.coanomaly_every == 1
    assert fit.region_pair_counts is None and fit.patient_pair_counts is None and fit.coanomaly_sweeps == 0
    with pytest.raises(ValueError):
        fit.coanomaly_posterior()                            # no model, no data
    fit.model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fit.model.sample_fast(5, 3, 2, seed=1)
    (fit.b, fit.bt) = (b, bt)
    with pytest.raises(ValueError):
        fit.coanomaly_posterior()                            # vb without a run: no _lq_R
    fit.method = "gibbs"
    with pytest.raises(ValueError):
        fit.coanomaly_posterior()                            # gibbs without coanomaly = True
    fit.region_pair_counts = np.zeros((5, 5), dtype=np.int64)
    fit.patient_pair_counts = np.zeros((2, 2), dtype=np.int64)
    with pytest.raises(ValueError):
        fit.coanomaly_posterior()                            # no sweep accumulated
    shared = fcdiff_amd.fit.SharedRegionFit()
    assert shared.coanomaly is False
    with pytest.raises(ValueError):
        shared.coanomaly_posterior()


@pytest.mark.parametrize("every", [0, -1, 1.5])
def test_fit_refuses_bad_every_before_the_run(every):
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit.coanomaly, fit.coanomaly_every) = (True, every)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 2)                                  # refused before any engine or device state is made


def test_fit_refuses_overflow_before_the_run():
    """The bound carries the max(Nreg, U) factor: 2^20 chains x 100 sweeps fit a histogram counter, not a diagonal entry
    of 200 regions."""
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit.coanomaly, fit.n_chains, fit.n_sweeps, fit.burn_in) = (True, 1 << 20, 100, 0)
    fit._check_accumulator("coanomaly_every", "co-anomaly counts", sites=1)
    with pytest.raises(ValueError):
        fit._run_gibbs(200, 50)


def engine_stand_in(G, N, U):
    """GibbsEngine.run's bounds, checked on a stand-in that has only what the checks read."""
    from fcdiff_amd.gibbs import GibbsEngine
    eng = GibbsEngine.__new__(GibbsEngine)
    (eng.G, eng.Nreg, eng.U, eng.pair_acc, eng.count_hist) = (G, N, U, None, None)
    (eng.coanomaly_acc, eng.coanomaly_every, eng.coanomaly_sweeps) = ((None, None), 1, 0)
    return eng


def test_engine_run_refuses_overflow():
    eng = engine_stand_in(1 << 20, 200, 50)
    with pytest.raises(ValueError, match="co-anomaly"):
        eng.run(0, 100, accumulate_from=0)                    # 2^20 x 200 x 100 > 2^32
    eng = engine_stand_in(1 << 10, 50, 200)
    eng.coanomaly_sweeps = 20000
    with pytest.raises(ValueError, match="co-anomaly"):
        eng.run(20000, 1000, accumulate_from=0)               # earlier sweeps count too; U is the larger side here


def test_engine_attach_refuses_bad_every():
    eng = engine_stand_in(64, 4, 2)
    for every in (0, -3):
        with pytest.raises(ValueError):
            eng.attach_coanomaly_accumulator(every)
    eng.coanomaly_acc = None
    with pytest.raises(ValueError):
        eng.coanomaly_host()
