"""
The Gibbs kernels against the EXACT law of their sweeps (oracle/exact_chain.py), and the three M-step implementations
at their clamps against the oracle's gibbs_mstep.  Cases, seeds and thresholds: tests/exact_law_cases.py; the same
statistics on the C oracle, with the measured power of every test, are in tests/test_exact_law.py.  The C oracle is
bit-exact with the kernels, so each statistical outcome here was known before the run.

Chain count: 2^18 chains (4 096 chain words), 128 times the largest count of the parity tests, are accepted by every
entry point used here (fcd_gibbs_run, fcd_gibbs_sweeps, import / export, log-joint, conditionals).  Each test prints the
count and the r form it ran (ctx.stat("r_form_last"): 1 = one launch per block step, 2 = the pipelined one-launch pass):
at these shapes the pipelined form fits the device at 2^18 chains and runs everywhere but under r_path 3.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain, histogram

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine = torch, fcdiff_amd, _lib, GibbsEngine
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def engine(env, name, G):
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    return eng


@pytest.fixture(scope="module")
def oracle_final():
    """{case: the C oracle's state of the 2^18 chains after the last sweep}"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = X.oracle_histograms(name)[2]
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(X.CASES))
def test_kernel_logjoint_and_conditionals_at_every_state(env, name):
    """Every state of the model imported as a chain (186 624 chains at 4x2): device log-joint = enumerator (rtol 1e-12);
    device conditionals, as logit differences, = the enumerator's neighbouring-state differences (atol 1e-10)."""
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    (f, r) = ec.all_states()
    eng = engine(env, name, ec.n_states)
    eng.import_state(f, r)
    (f2, r2) = eng.export_state()
    nptest.assert_array_equal(f2, f)
    nptest.assert_array_equal(r2, r)
    nptest.assert_allclose(eng.host(eng.logjoint()), ec.L.reshape(-1), rtol=1e-12)
    (cf, cr) = eng.conditionals()
    (cf, cr) = (eng.host(cf), eng.host(cr))
    nptest.assert_allclose(cf - cf[:, :, :1], ec.f_logit_diffs(f, r), rtol=0, atol=1e-10)
    nptest.assert_allclose(cr[..., 1] - cr[..., 0], ec.r_logit_diffs(f, r), rtol=0, atol=1e-10)


KNOB_FORMS = [("4x2", {"r_path": 3}), ("3x2", {"r_tol": 1e30}), ("4x1", {"f_form": 2}), ("3x2-strong", {"f_tol": 1e30}),
              ("3x1", {"r_dsplit": 1})]
PATHS = [(n, "run", {}) for n in X.CASES] + [(n, "sweeps", {}) for n in X.CASES] + [(n, "run", k) for (n, k) in KNOB_FORMS]


@pytest.mark.parametrize("name,path,kn", PATHS,
                         ids=["%s-%s%s" % (n, p, "".join("-%s" % k for k in kn)) for (n, p, kn) in PATHS])
def test_kernel_chains_follow_the_exact_law(env, oracle_final, record_property, name, path, kn):
    """
    2^18 chains of the kernels (fcd_gibbs_run with mstep_every = 0, or fcd_gibbs_sweeps; the knob forms: the step-per-launch
    r pass, exact r thresholds, the any-U f kernel, exact f draws, one in-order workgroup) after k = 1, 2, 3, 6 sweeps
    against P_k: joint G-test (fail at p < 1e-6, <= 11 664 states) and every low-order marginal cell (fail where the
    two-sided tail is below that of |z| > 5.5).  Power, measured with these chains (test_exact_law.py): pi x 1.01-1.02,
    one lM entry + 0.02-0.03, the reverse r scan and swapped passes rejected at every case.
    Then the chains' final state equals the C oracle's, chain for chain.
    """
    G = X.G_CHAINS
    for (k, v) in kn.items():
        env.ctx.set_knob(k, v)
    try:
        eng = engine(env, name, G)
        eng.init(X.PI0)
        ec = X.exact(name)
        hists = {}
        for s in range(max(X.SWEEPS)):
            if path == "run":
                eng.run(s, 1, mstep_every=0)
            else:
                eng.sweeps(s, 1)
            if s + 1 in X.SWEEPS:
                (f, r) = eng.export_state()
                hists[s + 1] = histogram(ec, f, r)
        r_form = env.ctx.stat("r_form_last")
        assert env.ctx.stat("dev_err") == 0
    finally:
        for k in kn:
            env.ctx.set_knob(k, 0)
    record_property("chains", G)
    record_property("r_form_last", r_form)
    print("%s %s %s: %d chains, r form %d" % (name, path, kn, G, r_form))
    assert r_form == (1 if kn.get("r_path") == 3 else 2)
    bad = X.failures(ec, hists, ec.laws(X.PI0, X.SWEEPS))
    assert not bad, bad
    (f_o, r_o) = oracle_final(name)
    nptest.assert_array_equal(f, f_o)
    nptest.assert_array_equal(r, r_o)


# ------------------------------------------------------------------------------------------------
# M-step at its clamps: fcd_gibbs_mstep, the fused M-step of fcd_gibbs_run, against oracle.gibbs_mstep
# ------------------------------------------------------------------------------------------------
def assert_hyper_is(hyper, pi, gamma):
    """hyper = {ln gamma_0..2, ln(1-pi), ln pi}, rtol 1e-14."""
    want = np.concatenate([np.log(gamma), [np.log(1.0 - pi), np.log(pi)]])
    nptest.assert_allclose(hyper[0:5], want, rtol=1e-14, atol=0)


def mstep_cases():
    """(Nreg, U, counts {sum r, #0, #1, #2, G}) at every clamp, also with G*Nreg*U and G*C above 2^31."""
    out = []
    for (N, U, G) in [(5, 3, 256), (200, 50, 1 << 20)]:
        (nr, nf) = (G * N * U, G * N * (N - 1) // 2)
        out += [(N, U, [0, nf // 3, nf // 3, nf - 2 * (nf // 3), G]),          # sum r = 0
                (N, U, [nr, nf // 2, nf - nf // 2 - 1, 1, G]),                 # sum r = n_r
                (N, U, [nr // 3, 0, nf // 2, nf - nf // 2, G]),                # one class count 0
                (N, U, [1, 0, nf, 0, G]),                                       # two class counts 0
                (N, U, [nr - 1, nf - 2, 1, 1, G])]                             # no clamp
    return out


@pytest.mark.parametrize("N,U,counts", mstep_cases())
def test_mstep_kernel_at_the_clamps(env, N, U, counts):
    """fcd_gibbs_mstep (the kernel after the all-reduce) on synthetic pooled counts = ln of oracle.gibbs_mstep."""
    t = env.torch
    c = t.tensor(counts + [0, 0, 0], dtype=t.int64, device="cuda")
    hyper = t.zeros(8, dtype=t.float64, device="cuda")
    env.ctx.call("fcd_gibbs_mstep", env.lib.dptr(c), N, U, env.lib.dptr(hyper), env.lib.stream_ptr())
    (pi, gamma) = O.gibbs_mstep(counts, N, U)
    assert_hyper_is(hyper.cpu().numpy(), pi, gamma)


def _force_bound(S_B, lM, lngamma, lnpi2):
    """
    Upper bounds, from the tables alone, of the probability of the outcome a forcing hyper-parameter set excludes:
    (ln P(r_nu flips away from the favoured value), ln P(f_c takes a type of weight 1e-300)), maximised over every state.
    """
    (C, U) = lM.shape[0:2]
    Nreg = int(round(O.C_to_N(C)))
    # r: logit(r = 1) = ln pi - ln(1 - pi) + d,  |d| <= sum over the other regions of the largest |lM difference|
    dmax = (Nreg - 1) * float(np.max(np.abs(lM[..., :, None] - lM[..., None, :])))
    lr = min(lnpi2[1] - lnpi2[0], lnpi2[0] - lnpi2[1]) + dmax
    # f: ln P(f_c = k) <= ln gamma_k - ln gamma_j + (data of k at its best) - (data of j at its worst), j the favoured type
    lf = -np.inf
    for c in range(C):
        hi = S_B[c] + np.sum(np.max(lM[c], axis=2), axis=0)
        lo = S_B[c] + np.sum(np.min(lM[c], axis=2), axis=0)
        j = int(np.argmax(lngamma))
        for k in range(3):
            if lngamma[k] < -600:
                lf = max(lf, lngamma[k] - lngamma[j] + hi[k] - lo[j])
    return lr, lf


@pytest.mark.parametrize("force", ["pi-0,gamma-two-zero", "pi-1,gamma-one-zero"])
def test_fused_mstep_at_the_clamps(env, force):
    """
    The M-step inside fcd_gibbs_run's tally launch (lane per logarithm) at its clamps, reached by hyper-parameters that
    force the sweep's outcome: pi = 1e-300 (sum r = 0) or 1 - pi = 1e-300 (sum r = n_r), gamma = (1, 1e-300, 1e-300) (two
    class counts 0) or (0.5, 0.5, 1e-300) (one).  The tables bound the probability of any other outcome below 1e-30 per
    draw (besides the 2^-53 atom at a uniform of exactly 0); the stored logarithms = ln of oracle.gibbs_mstep of the counts.
    """
    (N, U, G) = (5, 3, 256)
    m = X.model("broad")
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 4, U, seed=3)
    (lpB, _p, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    S_B = O.sum_lp_B(lpB)
    if force == "pi-0,gamma-two-zero":
        (pi2, gamma, want_r, zero) = (np.array([1.0, 1e-300]), np.array([1.0, 1e-300, 1e-300]), 0, [1, 2])
    else:
        (pi2, gamma, want_r, zero) = (np.array([1e-300, 1.0]), np.array([0.5, 0.5, 1e-300]), N * U, [2])
    (lr, lf) = _force_bound(S_B, lM, np.log(gamma), np.log(pi2))
    assert lr < np.log(1e-30) and lf < np.log(1e-30), (lr, lf)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=41, ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(0.5)
    counts = eng.host(eng.run(0, 1, mstep_every=1, want_counts=True)).copy()
    hyper = eng.host(eng.hyper)
    (f, r) = eng.export_state()
    assert (r.sum(axis=(1, 2)) == want_r).all()
    for k in zero:
        assert (f != k).all()
    assert list(counts[:5]) == [int(r.sum())] + [int((f == k).sum()) for k in range(3)] + [G]
    (pi, gam) = O.gibbs_mstep(counts[:5], N, U)
    assert pi == (0.5 / (G * N * U) if want_r == 0 else 1.0 - 0.5 / (G * N * U))        # the clamp itself was reached
    assert all(gam[k] == 0.5 / (G * eng.C) for k in zero)
    assert_hyper_is(hyper, pi, gam)
