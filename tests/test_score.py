"""
Scoring new patients, host side (no GPU): the NumPy reference of tests/score_ref.py against explicit loops and the oracle's
energy, the variational bound against its enumerated target, and the host helpers of fcdiff_amd/score.py.
"""
import itertools

import numpy as np
import numpy.testing as nptest
import pytest

import score_ref as R
from oracle import fcdiff_oracle as O


def random_logs(rng, shape):
    a = rng.normal(size=shape) * 1.5
    return a - np.log(np.sum(np.exp(a), axis=-1, keepdims=True))


def tables(N, U, seed, nan_frac=0.0):
    from fcdiff_amd.model import UnsharedRegionModel
    m = UnsharedRegionModel()
    m.mu, m.sigma = np.array([-0.3, 0.0, 0.3]), np.array([0.2, 0.25, 0.3])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 3, U, seed=seed)
    if nan_frac:
        rng = np.random.default_rng(seed)
        bt = np.where(rng.random(bt.shape) < nan_frac, np.nan, bt)
    with np.errstate(invalid="ignore", divide="ignore"):
        (_lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    lM = np.where(np.isnan(bt)[:, :, None, None], 0.0, lM)
    return m, lM


@pytest.mark.parametrize("N,U,nan_frac", [(3, 2, 0.0), (5, 3, 0.0), (6, 4, 0.3)])
def test_patient_elbo_matches_loops_and_the_energy(N, U, nan_frac):
    """Per-patient terms: explicit loops over (c, k, l) and (n, j); their sums over u are the oracle's energy terms."""
    rng = np.random.default_rng(N * 10 + U)
    (m, lM) = tables(N, U, seed=N + U, nan_frac=nan_frac)
    C = lM.shape[0]
    lq_F = random_logs(rng, (C, 1, 3))
    lq_R = random_logs(rng, (N, U, 2))
    pi2 = m.pi2()
    got = R.patient_elbo(lq_F, lq_R, lM, pi2)
    (q_F, q_R) = (np.exp(lq_F), np.exp(lq_R))
    for u in range(U):
        eM = 0.0
        for c in range(C):
            (n, mm) = O.c_to_nm(c)
            w = [q_R[n, u, 0] * q_R[mm, u, 0], q_R[n, u, 1] * q_R[mm, u, 1],
                 q_R[n, u, 0] * q_R[mm, u, 1] + q_R[n, u, 1] * q_R[mm, u, 0]]
            for k in range(3):
                for l in range(3):
                    eM += q_F[c, 0, k] * w[l] * lM[c, u, k, l]
        eR = sum(q_R[n, u, j] * np.log(pi2[j]) for n in range(N) for j in range(2))
        eq = sum(q_R[n, u, j] * lq_R[n, u, j] for n in range(N) for j in range(2))
        nptest.assert_allclose(got[u], [eM, eR, eq, eM + eR - eq], rtol=1e-12, atol=1e-12)
    S_B = np.zeros((C, 3))
    terms = O.energy_terms(lq_F, lq_R, S_B, lM, np.array([0.3, 0.4, 0.3]), pi2)
    nptest.assert_allclose(got[:, 0].sum(), terms[3], rtol=1e-12)
    nptest.assert_allclose(got[:, 1].sum(), terms[2], rtol=1e-12)
    nptest.assert_allclose(got[:, 2].sum(), terms[5], rtol=1e-12)


@pytest.mark.parametrize("N", [3, 4])
def test_exact_predictive_by_enumeration(N):
    """log p(bt_u | f) by enumeration against the same sum written out as products of probabilities; an unobserved
    patient has p = 1 and the prior as its posterior of r."""
    (m, lM) = tables(N, 2, seed=3 * N)
    C = lM.shape[0]
    rng = np.random.default_rng(N)
    f = rng.integers(0, 3, size=C)
    pi = float(m.pi2()[1])
    for u in range(2):
        lp = R.exact_log_pred(lM[:, u], f, pi)
        # brute force: the same sum written out over the 2^N configurations
        tot = 0.0
        for r in itertools.product((0, 1), repeat=N):
            pr = np.prod([pi if x else 1.0 - pi for x in r])
            lik = np.prod([np.exp(lM[c, u, f[c], R.mix_case(r[O.c_to_nm(c)[0]], r[O.c_to_nm(c)[1]])]) for c in range(C)])
            tot += pr * lik
        nptest.assert_allclose(lp, np.log(tot), rtol=1e-12)
        p = R.exact_p_r(lM[:, u], f, pi)
        assert p.shape == (N,) and np.all((p >= 0) & (p <= 1))
    # an unobserved patient (lM = 0): p(bt | f) = 1 and the posterior of r is the prior
    zero = np.zeros((C, 3, 3))
    assert R.exact_log_pred(zero, f, pi) == pytest.approx(0.0, abs=1e-14)
    nptest.assert_allclose(R.exact_p_r(zero, f, pi), pi, rtol=1e-12)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_elbo_is_a_lower_bound(seed):
    """elbo_u <= sum_F q_F(F) log p(bt_u | F) for any q_R, on C = 3 (every F and r enumerated); also at a one-hot q_F with
    q_R set to the exact marginals of r given that F."""
    rng = np.random.default_rng(seed)
    (m, lM) = tables(3, 2, seed=20 + seed)
    pi = float(m.pi2()[1])
    lq_F = random_logs(rng, (3, 1, 3))
    lq_R = random_logs(rng, (3, 2, 2))
    elbo = R.patient_elbo(lq_F, lq_R, lM, m.pi2())[:, 3]
    for u in range(2):
        assert elbo[u] <= R.expected_log_pred_qF(lq_F, lM[:, u], pi) + 1e-12
    # (the exact posterior of r is not a product over regions, so the mean-field bound stays a bound here too)
    F = rng.integers(0, 3, size=3)
    with np.errstate(divide="ignore"):
        lq_F1 = np.log(np.eye(3)[F])[:, None, :]
    for u in range(2):
        p = R.exact_p_r(lM[:, u], F, pi)
        lq = np.log(np.stack([1.0 - p, p], axis=1))[:, None, :]
        e = R.patient_elbo(lq_F1, lq, lM[:, u:u + 1], m.pi2())[0, 3]
        assert e <= R.exact_log_pred(lM[:, u], F, pi) + 1e-12


def test_pool_ais_equals_one_logsumexp():
    """Pooling (max, sum exp, sum exp^2, G) over ranks is the logsumexp, ESS and delta-method error of all chains at once."""
    from fcdiff_amd.score import pool_ais
    rng = np.random.default_rng(5)
    w = rng.normal(size=(1000, 4)) * np.array([0.1, 1.0, 5.0, 40.0]) - np.array([0.0, 3.0, 100.0, 700.0])
    (lp1, se1, ess1) = pool_ais(R.ais_parts(w))
    m = np.max(w, axis=0)
    s = np.exp(w - m)
    want = m + np.log(s.mean(axis=0))
    nptest.assert_allclose(lp1, want, rtol=1e-13)
    nptest.assert_allclose(ess1, s.sum(axis=0) ** 2 / (s * s).sum(axis=0), rtol=1e-12)
    nptest.assert_allclose(se1, s.std(axis=0, ddof=1) / np.sqrt(1000) / s.mean(axis=0), rtol=1e-10)
    # three ranks of unequal size, one of them far below the others
    cuts = [0, 150, 700, 1000]
    parts = np.stack([R.ais_parts(w[a:b]) for (a, b) in zip(cuts[:-1], cuts[1:])])
    (lp, se, ess) = pool_ais(parts)
    nptest.assert_allclose(lp, lp1, rtol=1e-13)
    nptest.assert_allclose(se, se1, rtol=1e-10)
    nptest.assert_allclose(ess, ess1, rtol=1e-12)
    # all weights equal (an unobserved patient): log_pred exactly 0, se 0, ess = G
    (lp0, se0, ess0) = pool_ais(R.ais_parts(np.zeros((64, 2))))
    assert np.all(lp0 == 0.0) and np.all(se0 == 0.0) and np.all(ess0 == 64.0)
    # every weight zero on every rank
    dead = np.array([[[-np.inf, 0.0, 0.0, 10.0]], [[-np.inf, 0.0, 0.0, 6.0]]])
    (lpd, _sed, essd) = pool_ais(dead)
    assert lpd[0] == -np.inf and essd[0] == 0.0


def test_schedule_and_key():
    from fcdiff_amd.score import ais_schedule, score_key, SCORE_SWEEP0
    for T in (1, 2, 5, 200):
        b = ais_schedule(T)
        assert b.shape == (T + 1,) and b[0] == 0.0 and b[-1] == 1.0 and np.all(np.diff(b) > 0)
    with pytest.raises(ValueError):
        ais_schedule(0)
    keys = {score_key(s) for s in range(1000)}
    assert len(keys) == 1000 and not any(score_key(s) == s for s in range(1000))
    assert score_key(7) == score_key(7) and 0 <= score_key(2 ** 64 - 1) < 2 ** 64
    assert SCORE_SWEEP0 == 2 ** 31


def test_score_refuses_before_run():
    """score() is for a fitted model: before run() it raises (no device needed for the refusal)."""
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    with pytest.raises(ValueError):
        fit.score(np.zeros((3, 1)))
    fit.model = fcdiff_amd.UnsharedRegionModel()
    fit.method = "gibbs"
    with pytest.raises(ValueError):
        fit.score(np.zeros((3, 1)))
