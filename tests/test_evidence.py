"""
Model evidence by annealed importance sampling, host side (no GPU): the annealing loop of fcdiff_amd/evidence.py driven by
a stand-in engine over the C oracle against the enumerated evidence, the prior draw of its first sweep, the pooling over
ranks, the argument errors of log_evidence() and the new entry points' ABI.
"""
import ctypes as C
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import evidence_ref as R
import exact_law_cases as X
from conftest import ROOT

CASES = ("3x1", "3x2", "4x2", "3x2-strong")


@pytest.mark.parametrize("name", CASES)
def test_anneal_over_the_oracle_matches_the_enumerated_evidence(name):
    """|log_evidence - exact| <= 5 se and lower - 5 lower_se <= exact (G = 4096, 50 rungs): a condition, not a measurement --
    two-sided tail 6e-7 per case under normality."""
    from fcdiff_amd import evidence as E
    from fcdiff_amd.score import ais_schedule
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    exact = R.exact_log_evidence(S_B, lM, gamma, pi2)
    eng = R.OracleEngine(S_B, lM, gamma, pi2, 4096, seed)
    w = E.anneal(eng, ais_schedule(50))
    out = E.pool(E.weight_parts(w)[None], 50)
    print("%s exact %.4f estimate %.4f se %.4f ess %.0f lower %.4f (%.4f)" % (name, exact, out["log_evidence"],
          out["log_evidence_se"], out["ess"], out["lower"], out["lower_se"]))
    assert out["n_chains"] == 4096 and out["n_anneal"] == 50
    assert abs(out["log_evidence"] - exact) <= 5.0 * out["log_evidence_se"]
    assert out["lower"] - 5.0 * out["lower_se"] <= exact
    assert 1.0 <= out["ess"] <= 4096.0


def test_the_first_sweep_draws_the_prior():
    """Zero tables, one sweep: f ~ gamma = (0.3, 0.4, 0.3) and r ~ Bernoulli(pi), by a z-test per cell at Z_MAX.  (A loop that
    started from gibbs_init's uniform f would put 1/3 on every type: z > 30 at 2^16 chains.)"""
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem("4x2")
    G = 1 << 16
    eng = R.OracleEngine(S_B, lM, gamma, pi2, G, seed)
    eng.temper(0.0)
    eng.sweep(0)
    for c in range(eng.f.shape[1]):
        for k in range(3):
            p = gamma[k]
            z = (np.count_nonzero(eng.f[:, c] == k) - G * p) / np.sqrt(G * p * (1 - p))
            assert abs(z) < X.Z_MAX, ("f", c, k, z)
    p = pi2[1]
    z = (eng.r.reshape(G, -1).sum(axis=0) - G * p) / np.sqrt(G * p * (1 - p))
    assert np.all(np.abs(z) < X.Z_MAX), z
    # ... and the power of the test: the uniform start is rejected
    from oracle import c_oracle as CO
    (f0, _r0) = CO.gibbs_init(G, N, U, float(p), seed)
    z0 = (np.count_nonzero(f0[:, 0] == 1) - G * gamma[1]) / np.sqrt(G * gamma[1] * (1 - gamma[1]))
    assert abs(z0) > X.Z_MAX


def test_anneal_refuses_a_ladder_that_does_not_run_from_0_to_1():
    from fcdiff_amd import evidence as E
    for bad in ([0.0, 0.5], [0.1, 1.0], [0.0, 0.6, 0.4, 1.0], [1.0]):
        with pytest.raises(ValueError):
            E.anneal(None, bad)


def test_pool_of_two_ranks_is_the_single_rank_result():
    from fcdiff_amd import evidence as E
    rng = np.random.default_rng(11)
    for (scale, shift) in ((0.3, -3.0), (4.0, -700.0), (25.0, 1.0e5)):
        w = rng.normal(size=1000) * scale + shift
        one = E.pool(E.weight_parts(w)[None], 7)
        two = E.pool(np.stack([E.weight_parts(w[:350]), E.weight_parts(w[350:])]), 7)
        m = w.max()
        e = np.exp(w - m)
        nptest.assert_allclose(one["log_evidence"], m + np.log(e.mean()), rtol=1e-13)
        nptest.assert_allclose(one["ess"], e.sum() ** 2 / (e * e).sum(), rtol=1e-12)
        nptest.assert_allclose(one["log_evidence_se"], e.std(ddof=1) / np.sqrt(w.size) / e.mean(), rtol=1e-10)
        nptest.assert_allclose(one["lower"], w.mean(), rtol=1e-14)
        nptest.assert_allclose(one["lower_se"], w.std(ddof=1) / np.sqrt(w.size), rtol=1e-11)
        assert one["lower"] <= one["log_evidence"]
        for key in ("log_evidence", "log_evidence_se", "ess", "lower", "lower_se"):
            nptest.assert_allclose(two[key], one[key], rtol=1e-12, atol=1e-12, err_msg=key)
        assert two["n_chains"] == one["n_chains"] == 1000 and two["n_anneal"] == 7


def test_evidence_key_is_apart_from_the_fit_and_from_score():
    from fcdiff_amd.evidence import evidence_key
    from fcdiff_amd.score import score_key
    keys = {evidence_key(s) for s in range(1000)}
    assert len(keys) == 1000
    assert not any(evidence_key(s) in (s, score_key(s)) for s in range(1000))
    assert not keys & {score_key(s) for s in range(1000)}
    assert 0 <= evidence_key(2 ** 64 - 1) < 2 ** 64


def test_log_evidence_argument_errors_need_no_device():
    import fcdiff_amd
    for cls in (fcdiff_amd.fit.UnsharedRegionFit, fcdiff_amd.fit.SharedRegionFit):
        fit = cls()
        with pytest.raises(ValueError, match="run"):
            fit.log_evidence()
        fit.model = fcdiff_amd.UnsharedRegionModel()
        (fit.b, fit.bt) = (np.zeros((3, 2)), np.zeros((3, 2)))
        with pytest.raises(ValueError, match="run"):
            fit.log_evidence()
        fit.method = "gibbs"
        with pytest.raises(ValueError, match="run"):
            fit.log_evidence()
        with pytest.raises(ValueError, match="n_anneal"):
            fit.log_evidence(n_anneal=0)
        with pytest.raises(ValueError, match="n_anneal"):
            fit.log_evidence(n_anneal=2.5)
        with pytest.raises(ValueError, match="n_chains"):
            fit.log_evidence(n_chains=0)
        fit.n_chains = 0
        with pytest.raises(ValueError, match="n_chains"):
            fit.log_evidence()
        assert fit._ctx is None and fit._query_ctx is None


def test_abi_of_the_new_entry_points():
    from fcdiff_amd import _lib
    text = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("fcd_evidence_energy", "fcd_evidence_temper"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
        assert hasattr(raw, name)
    assert len(_lib.SIGNATURES["fcd_evidence_energy"][1]) == 12 and len(_lib.SIGNATURES["fcd_evidence_temper"][1]) == 7
    assert re.search(r"#define FCD_ABI_VERSION 4\b", text) and _lib.ABI_VERSION == 4
    assert _lib.load().fcd_abi_version() == 4
