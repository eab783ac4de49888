"""
The C oracle's Gibbs sampler against the EXACT law of its sweeps (oracle/exact_chain.py) on models small enough to
enumerate: (Nreg, U) = (3,1), (3,2), (4,1), (4,2) with broad data and (3,2) with strong data (the exponential-free f
draw's regime).  The oracle and the kernels are bit-exact with each other, so these tests are what ties both to the
distribution the model defines; tests/test_gpu_exact_law.py runs the same cases on the kernels.

  * exact, every state: the oracle's log-joint and conditionals equal the enumerator's (differences of log-joints of
    neighbouring states);
  * statistical: 2^18 independent chains (fixed seeds: each test always passes or always fails) after k = 1, 2, 3, 6
    sweeps against P_k -- a G-test of the joint histogram (<= 11 664 states; cells expecting < 5 chains merged; fail at
    p < 1e-6) and every cell of the f_c, r_nu, (r_nu, r_mu) and (f_c, r_nu at an endpoint of c) marginals (fail where
    the two-sided tail is below that of |z| > 5.5, 3.8e-8; exact binomial tails for cells expecting few chains);
  * power: the same chains must REJECT the laws of wrong samplers -- pi x 1.05, one lM entry + 0.05, the r scan in
    reverse region order, f drawn after r (the two passes swapped).
"""
import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain, mix_case

CASE_NAMES = list(X.CASES)


@pytest.fixture(scope="module")
def chains():
    """{case: (ExactChain, {k: histogram}, final (f, r))} of the C oracle's 2^18 chains (about 0.5 s a case)."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = X.oracle_histograms(name)
        return cache[name]
    return get


def test_mix_case_is_the_oracles_mix_index():
    rr = np.array([0, 1])
    nptest.assert_array_equal(mix_case(rr[:, None], rr[None, :]), np.array([[0, 2], [2, 1]]))
    nptest.assert_array_equal(mix_case(rr[:, None], rr[None, :]), O.mix_index(rr[:, None], rr[None, :]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_logjoint_and_conditionals_at_every_state(name):
    """Every state of the model imported as a chain: C oracle log-joint = enumerator (rtol 1e-12); f and r conditionals
    of the C oracle, as logit differences, = the enumerator's neighbouring-state differences (atol 1e-10)."""
    from oracle import c_oracle as CO
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    (f, r) = ec.all_states()
    (lng, lnpi2) = (np.log(gamma), np.log(pi2))
    nptest.assert_allclose(CO.gibbs_logjoint(f, r, S_B, lM, lng, lnpi2), ec.L.reshape(-1), rtol=1e-12)
    cf = CO.gibbs_f_step(f.copy(), r.copy(), S_B, lM, lng, 0, 0, want_cond=True, draw=False)
    cr = CO.gibbs_r_step(f.copy(), r.copy(), lM, lnpi2, 0, 0, O.EDGE_SYMMETRIC, want_cond=True, draw=False)
    nptest.assert_allclose(cf - cf[:, :, :1], ec.f_logit_diffs(f, r), rtol=0, atol=1e-10)
    nptest.assert_allclose(cr[..., 1] - cr[..., 0], ec.r_logit_diffs(f, r), rtol=0, atol=1e-10)


def test_cases_cover_the_regimes():
    """broad data: every edge's leading type is within e^4 of the next (posterior spread); strong: every edge's leading
    type is ahead by more than e^15 (the f pass's exponential-free draw)."""
    for name in CASE_NAMES:
        (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
        a = np.sort(S_B + np.log(gamma), axis=1)
        lead = a[:, 2] - a[:, 1]
        if X.CASES[name][2] == "strong":
            assert lead.min() > 15.0, (name, lead)
        else:
            assert lead.max() < 4.0, (name, lead)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_chains_follow_the_exact_law(chains, name):
    """
    2^18 chains of the C oracle after k = 1, 2, 3, 6 sweeps against P_k: joint G-test (p < 1e-6 fails, <= 11 664
    states) and every low-order marginal cell (two-sided tail < 3.8e-8 fails, i.e. |z| > 5.5).
    Measured power (smallest perturbation of the law these same chains reject, see test_wrong_laws_are_rejected):
    pi x 1.02 (3x1, 3x2-strong) / x 1.01 (3x2, 4x1, 4x2); the lM entry + 0.03 (+ 0.02 at 3x2); reverse scan and swapped
    passes at every case.
    """
    (ec, hists, _state) = chains(name)
    bad = X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    print("%s: %d chains, %d states, sweeps %s" % (name, X.G_CHAINS, ec.n_states, X.SWEEPS))
    assert not bad, bad


def _wrong(name, what, size=None):
    """The law of a wrong sampler of case `name`."""
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    if what == "pi":
        pi = pi2[1] * size
        return ExactChain(S_B, lM, gamma, np.array([1.0 - pi, pi]))
    if what == "lM":
        # the lM entry that matters most: (edge whose two leading types are closest, patient 0, its leading type, both typical)
        a = S_B + np.log(gamma)
        s = np.sort(a, axis=1)
        c = int(np.argmin(s[:, 2] - s[:, 1]))
        lM = lM.copy()
        lM[c, 0, int(np.argmax(a[c])), 0] += size
        return ExactChain(S_B, lM, gamma, pi2)
    if what == "reverse":
        return ExactChain(S_B, lM, gamma, pi2, r_order=[(n, u) for n in reversed(range(N)) for u in range(U)])
    assert what == "swap"
    return ExactChain(S_B, lM, gamma, pi2, f_first=False)


# smallest (pi factor, lM shift) the chains of each case reject -- measured with these seeds, recorded in the docstrings
POWER = {"3x1": (1.02, 0.03), "3x2": (1.01, 0.02), "4x1": (1.01, 0.03), "4x2": (1.01, 0.03), "3x2-strong": (1.02, 0.03)}


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("what,size", [("pi", 1.05), ("lM", 0.05), ("reverse", None), ("swap", None)])
def test_wrong_laws_are_rejected(chains, name, what, size):
    """
    Proof the statistical test has teeth: the oracle's chains of test_oracle_chains_follow_the_exact_law must reject the
    law of each wrong sampler -- pi x 1.05, lM + 0.05 at one entry, the r scan in reverse region order, f drawn after r.
    """
    (_ec, hists, _state) = chains(name)
    ec = _wrong(name, what, size)
    assert X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_measured_power(chains, name):
    """The power recorded in the docstrings: the smallest pi factor / lM shift rejected, and the next smaller accepted."""
    (_ec, hists, _state) = chains(name)
    (pi_min, lm_min) = POWER[name]
    steps = [1.0025, 1.005, 1.01, 1.02, 1.03, 1.05]
    below = steps[steps.index(pi_min) - 1]
    ec = _wrong(name, "pi", pi_min)
    assert X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    ec = _wrong(name, "pi", below)
    assert not X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    shifts = [0.0025, 0.005, 0.01, 0.02, 0.03, 0.05]
    ec = _wrong(name, "lM", lm_min)
    assert X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    ec = _wrong(name, "lM", shifts[shifts.index(lm_min) - 1])
    assert not X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
