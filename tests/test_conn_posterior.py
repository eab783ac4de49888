"""
Connection-level posteriors without a GPU: the closed forms of tests/conn_posterior_ref.py against an explicit enumeration
of T and F~ from the generative model (doc/methods.rst:70-177), their mixture against the oracle's M_kl, the new C-ABI
symbols, and the host-side refusals of UnsharedRegionFit.connection_posterior().
"""
import ctypes as C
import itertools

import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as R
from fcdiff_amd import _lib
from oracle import fcdiff_oracle as O


def enumerate_joint(k, l, bt, theta):
    """
    ln p(T = t, F~ = j, bt | F = k, case l) for t in {0, 1}, j in {0, 1, 2}, written from the generative model alone:
    T | l: both typical -> 0, both anomalous -> 1, discordant -> Bernoulli(eta) (model.sample_T); F~ | F = k, T: keeps k
    with 1 - epsilon (T = 0) or epsilon (T = 1), else one of the other two types uniformly (model.sample_F_tilde);
    bt | F~ = j: Normal(mu_j, sigma_j).  Entries of probability zero are -inf.
    """
    (eta, epsilon, mu, sigma) = (theta[1], theta[2], theta[6:9], theta[9:12])
    p_t1 = {0: 0.0, 1: 1.0, 2: eta}[l]
    out = np.full((2, 3), -np.inf)
    for (t, j) in itertools.product(range(2), range(3)):
        pt = p_t1 if t == 1 else 1.0 - p_t1
        keep = epsilon if t == 1 else 1.0 - epsilon
        pj = keep if j == k else (1.0 - keep) / 2.0
        if pt > 0 and pj > 0:
            out[t, j] = np.log(pt) + np.log(pj) + O.norm_logpdf(bt, mu[j], sigma[j])
    return out


def random_theta(rng, small_sigma=False):
    from fcdiff_amd.model import UnsharedRegionModel
    m = UnsharedRegionModel()
    if not small_sigma:
        m.eta, m.epsilon = rng.uniform(0.01, 0.99, 2)
        m.mu = np.sort(rng.uniform(-0.6, 0.6, 3))
        m.sigma = rng.uniform(0.03, 0.4, 3)
    return m.theta()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_closed_forms_equal_explicit_enumeration(seed):
    rng = np.random.default_rng(seed)
    theta = random_theta(rng, small_sigma=(seed == 0))      # seed 0: the model's default (small) sigma
    bts = np.concatenate([rng.uniform(-1, 1, 12), [-1.0, 1.0, 0.0]])
    (pT, pF, pch) = R.tables(bts, theta)
    (eta, epsilon, mu, sigma) = (theta[1], theta[2], theta[6:9], theta[9:12])
    for (i, bt) in enumerate(bts):
        Nd = np.array([O.norm_pdf(bt, mu[j], sigma[j]) for j in range(3)])
        for (k, l) in itertools.product(range(3), range(3)):
            lj = enumerate_joint(k, l, bt, theta)
            mx = lj.max()
            p = np.exp(lj - mx)
            p /= p.sum()
            nptest.assert_allclose(pT[i, k, l], p[1].sum(), rtol=0, atol=1e-14)
            nptest.assert_allclose(pF[i, k, l], p.sum(axis=0), rtol=0, atol=1e-14)
            nptest.assert_allclose(pch[i, k, l], 1.0 - p[:, k].sum(), rtol=0, atol=1e-14)
            # the mixture itself: sum over (t, j) of the joint = M_kl of the oracle (pinned to the reference by G2)
            nptest.assert_allclose(np.exp(lj).sum(), O.eval_M(Nd, eta, epsilon, k, l), rtol=1e-13)
    # p_T is exactly 0 where both endpoints are typical; every F~ row is a distribution
    assert np.all(pT[:, :, 0] == 0.0)
    nptest.assert_allclose(pF.sum(axis=-1), 1.0, rtol=0, atol=1e-14)


def test_closed_forms_finite_where_every_density_underflows():
    rng = np.random.default_rng(5)
    theta = random_theta(rng, small_sigma=True)
    bts = np.array([-40.0, 40.0, 1e3, -1e3])
    from oracle.fcdiff_oracle import norm_pdf
    assert all(norm_pdf(b, theta[6 + j], theta[9 + j]) == 0.0 for b in bts for j in range(3))     # lM = -inf there
    (pT, pF, pch) = R.tables(bts, theta)
    assert np.all(np.isfinite(pT)) and np.all(np.isfinite(pF)) and np.all(np.isfinite(pch))
    nptest.assert_allclose(pF.sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    # that far out, F~ is the type whose log-density is largest, with certainty
    for (i, b) in enumerate(bts):
        top = int(np.argmax([O.norm_logpdf(b, theta[6 + j], theta[9 + j]) for j in range(3)]))
        assert np.all(pF[i, :, :, top] == 1.0)


def test_contraction_of_one_hot_and_rank_one_weights():
    rng = np.random.default_rng(7)
    theta = random_theta(rng)
    (Nreg, U) = (5, 3)
    Cn = Nreg * (Nreg - 1) // 2
    bt = rng.uniform(-1, 1, (Cn, U))
    (pT, pF, pch) = R.tables(bt, theta)
    for (k, l) in itertools.product(range(3), range(3)):
        W = np.zeros((Cn, U, 3, 3))
        W[:, :, k, l] = 3.0
        out = R.contract(W, bt, theta)
        nptest.assert_allclose(out["p_T"], pT[:, :, k, l], rtol=1e-15)
        nptest.assert_allclose(out["p_F_tilde"], pF[:, :, k, l], rtol=1e-15)
        nptest.assert_allclose(out["p_changed"], pch[:, :, k, l], rtol=1e-15)
    lq_F = np.log(rng.dirichlet(np.ones(3), Cn))[:, None, :]
    q1 = rng.uniform(0, 1, (Nreg, U))
    lq_R = np.log(np.stack([1 - q1, q1], axis=2))
    W = R.vb_weights(lq_F, lq_R)
    nptest.assert_allclose(W.sum(axis=(2, 3)), 1.0, rtol=1e-14)
    # the weights of the fitter's own helper (fit.py:382-406) at edge c = (n, m)
    from fcdiff_amd.fit import _eval_q_R_w
    (n, m) = R.endpoints(Nreg)
    for c in range(Cn):
        w = _eval_q_R_w(np.exp(lq_R), n[c], m[c])
        nptest.assert_allclose(W[c], np.exp(lq_F[c, 0])[None, :, None] * w[:, None, :], rtol=1e-15)


def test_pair_counts_of_chain_states():
    rng = np.random.default_rng(3)
    (G, Nreg, U) = (37, 6, 4)
    f = rng.integers(0, 3, (G, Nreg * (Nreg - 1) // 2)).astype(np.uint8)
    r = (rng.random((G, Nreg, U)) < 0.4).astype(np.uint8)
    cnt = R.pair_counts(f, r, chunk=4)
    ends = O.edge_endpoints(Nreg)
    for (c, (n, m)) in enumerate(ends):
        for u in range(U):
            for g in range(G):
                l = int(O.mix_index(r[g, n, u], r[g, m, u]))
                cnt[c, u, f[g, c], l] -= 1
    assert np.all(cnt == 0)


def test_new_symbols_load_and_abi_stays_4():
    lib = _lib.load()
    for name in ("fcd_gibbs_pair_tally", "fcd_gibbs_set_pair_accumulator", "fcd_conn_posterior"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fcd_abi_version() == _lib.ABI_VERSION == 4
    # host-side argument checks: no context, no device work
    assert lib.fcd_gibbs_set_pair_accumulator(None, None, 4, 2, 1) == _lib.FCD_ERR_ARG
    th = (C.c_double * 12)()
    assert lib.fcd_conn_posterior(None, None, 4, 2, th, None, None, None, None, None, None, None) == _lib.FCD_ERR_ARG


def test_pair_sweep_count():
    from fcdiff_amd.gibbs import pair_sweeps_in
    for (s0, n, a, e) in itertools.product(range(5), range(7), range(6), range(1, 4)):
        want = sum(1 for s in range(s0, s0 + n) if s >= a and (s - a) % e == 0)
        assert pair_sweeps_in(s0, n, a, e) == want


def test_connection_posterior_refusals_without_a_run():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    with pytest.raises(ValueError):
        fit.connection_posterior()                           # no model, no data
    fit.model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fit.model.sample_fast(5, 3, 2, seed=1)
    (fit.b, fit.bt, fit.method) = (b, bt, "gibbs")
    assert fit.connection_marginals is False and fit.connection_every == 1 and fit.connection_counts is None
    with pytest.raises(ValueError):
        fit.connection_posterior()                           # gibbs without connection_marginals
    fit.connection_counts = np.zeros((10, 2, 3, 3), dtype=np.int64)
    with pytest.raises(ValueError):
        fit.connection_posterior()                           # no sweep accumulated
