"""
Model evidence on the device (UnsharedRegionFit.log_evidence / SharedRegionFit.log_evidence, fcd_evidence.hip): the energy
kernel against the NumPy reference at every layout boundary, the one-launch tempering of the working tables, the estimate
against the enumerated evidence of small models for both region models, a Bayes factor against its exact value, a fit left
exactly as it was, and one run at 200 regions x 100 patients.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import numpy.testing as nptest
import pytest

import evidence_ref as R
import exact_law_cases as X
from conftest import ROOT
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu

CASES = ("3x1", "3x2", "4x2", "3x2-strong")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, evidence
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.evidence = torch, fcdiff_amd, _lib, evidence
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# G in {1, 63, 64, 65, 1024}: partial and several chain words (2113: more words than one workgroup serves, both of its
# passes); U in {1, 2, 64, 65, 100}; Nreg in {2, 3, 17, 200}: one edge only, slices of a few items, tiles that end mid-row
# (U = 100: 896 items are 8.96 rows), several tiles per slice
SHAPES = [(1, 1, 2), (63, 2, 3), (64, 64, 17), (65, 65, 17), (1024, 1, 200), (65, 100, 200), (1024, 16, 17), (2113, 2, 17),
          (64, 100, 3), (1, 65, 200), (64, 1, 3), (65, 64, 2)]


@pytest.mark.parametrize("G,U,N", SHAPES)
def test_energy_kernel(env, G, U, N):
    """fcd_evidence_energy against chain_energy: error <= 1e-12 of sum |terms| (fp64 sums in another order: n 2^-53 with
    n <= 2e6 terms is 2.2e-10 at worst, the typical error far below; 1e-12 is the issue's bound), two calls bitwise equal,
    and w accumulates."""
    from fcdiff_amd.gibbs import GibbsEngine
    rng = np.random.default_rng(G * 7 + U * 3 + N)
    Cn = N * (N - 1) // 2
    S_B = rng.normal(size=(Cn, 3)) * 30.0 - 20.0
    lM = rng.normal(size=(Cn, U, 3, 3)) * 3.0 - 1.0
    f = rng.integers(0, 3, size=(G, Cn)).astype(np.uint8)
    r = (rng.random((G, N, U)) < 0.4).astype(np.uint8)
    (S_Bd, lMd) = (up(env, S_B), up(env, lM))
    eng = GibbsEngine(S_Bd, lMd, N, U, G, seed=1, edge_index="symmetric", ctx=env.ctx, region_major=False)
    eng.import_state(f, r)

    def step(w, b0, b1):
        env.ctx.call("fcd_evidence_energy", env.lib.dptr(S_Bd), env.lib.dptr(lMd), env.lib.dptr(eng.f_state),
                     env.lib.dptr(eng.r_bits), N, U, G, float(b0), float(b1), env.lib.dptr(w), env.lib.stream_ptr())
    w1 = env.torch.zeros(G, dtype=env.torch.float64, device="cuda")
    w2 = env.torch.zeros(G, dtype=env.torch.float64, device="cuda")
    step(w1, 0.0, 1.0)
    step(w2, 0.0, 1.0)
    (got, again) = (w1.cpu().numpy(), w2.cpu().numpy())
    env.ctx.check_device()
    assert got.tobytes() == again.tobytes()
    want = np.empty(G)
    scale = np.empty(G)
    for g0 in range(0, G, 16):              # (in pieces: the reference makes a (G, C, U) array)
        sl = slice(g0, min(g0 + 16, G))
        want[sl] = R.chain_energy(S_B, lM, f[sl], r[sl])
        scale[sl] = R.chain_energy_abs(S_B, lM, f[sl], r[sl])
    err = np.abs(got - want) / scale
    print("G=%d U=%d Nreg=%d max error / sum|terms| = %.3g" % (G, U, N, err.max()))
    assert np.all(err <= 1e-12)
    # a chain's number does not depend on the chains that share the launch: the first word alone
    if G > 64:
        eng1 = GibbsEngine(S_Bd, lMd, N, U, 64, seed=1, edge_index="symmetric", ctx=env.ctx, region_major=False)
        eng1.import_state(f[:64], r[:64])
        w64 = env.torch.zeros(64, dtype=env.torch.float64, device="cuda")
        env.ctx.call("fcd_evidence_energy", env.lib.dptr(S_Bd), env.lib.dptr(lMd), env.lib.dptr(eng1.f_state),
                     env.lib.dptr(eng1.r_bits), N, U, 64, 0.0, 1.0, env.lib.dptr(w64), env.lib.stream_ptr())
        assert w64.cpu().numpy().tobytes() == got[:64].tobytes()
    # w accumulates: a second call with another step adds (beta - beta_prev) E to what is there
    step(w1, 0.25, 0.625)
    nptest.assert_allclose(w1.cpu().numpy(), got + 0.375 * got, rtol=1e-15, atol=0)
    env.ctx.check_device()


def temper(env, beta, src, dst):
    n = len(src)
    env.ctx.call("fcd_evidence_temper", float(beta), n, (env.lib._p * n)(*[t.data_ptr() for t in src]),
                 (env.lib._p * n)(*[t.data_ptr() for t in dst]), (C.c_int64 * n)(*[t.numel() for t in src]),
                 env.lib.stream_ptr())


def test_temper_launch(env):
    """beta = 1: the sources bit for bit; beta = 0.37: torch's beta * src bit for bit; sizes that are not multiples of the
    block or of two, a pointer that is only 8-byte aligned, -inf entries, and memory beyond each table left alone."""
    t = env.torch
    rng = np.random.default_rng(3)
    sizes = [1, 255, 257, 1000003, 4096, 600]
    src = []
    for (i, n) in enumerate(sizes):
        a = rng.normal(size=n + 1) * 10.0 ** rng.integers(-5, 6)
        a[rng.integers(0, n + 1)] = -np.inf
        full = up(env, a)
        src.append(full[1:] if i in (2, 5) else full[:n])          # (tables 2 and 5 start at an odd element)
    for beta in (1.0, 0.37):
        store = [t.full((n + 3,), 7.0, dtype=t.float64, device="cuda") for n in sizes]
        dst = [s[1:n + 1] if i in (1, 5) else s[:n] for (i, (s, n)) in enumerate(zip(store, sizes))]
        temper(env, beta, src, dst)
        for (s, d, st, n) in zip(src, dst, store, sizes):
            want = s.clone() if beta == 1.0 else beta * s
            assert d.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
            assert float((st == 7.0).sum()) == 3.0                   # nothing written outside the table
    # in place, one table
    a = src[3].clone()
    temper(env, 0.37, [a], [a])
    assert a.cpu().numpy().tobytes() == (0.37 * src[3]).cpu().numpy().tobytes()
    for bad in (0, 9):
        with pytest.raises(ValueError):
            env.ctx.call("fcd_evidence_temper", 0.5, bad, (env.lib._p * 9)(), (env.lib._p * 9)(), (C.c_int64 * 9)(),
                         env.lib.stream_ptr())
    env.ctx.check_device()


def case_data(name):
    (N, U, data) = X.CASES[name]
    m = X.model(data)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)
    return N, U, m, b, bt


def set_params(dst, src):
    (dst.pi, dst.eta, dst.epsilon) = (src.pi, src.eta, src.epsilon)
    (dst.gamma, dst.mu, dst.sigma) = (np.array(src.gamma), np.array(src.mu), np.array(src.sigma))


def fitted(env, shared, b, bt, method, start):
    """A fit of (b, bt) after a short run(), started from the parameters of `start`."""
    fit = env.pkg.fit.SharedRegionFit() if shared else env.pkg.fit.UnsharedRegionFit()
    fit.model = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    set_params(fit.model, start)
    (fit.b, fit.bt, fit.method) = (b, bt, method)
    (fit.max_iters, fit.n_chains, fit.n_sweeps, fit.burn_in) = (2, 64, 12, 4)
    fit.run()
    return fit


def exact_at(fit, b, bt, shared):
    """The enumerated evidence at the fit's current parameters (tables by the NumPy oracle)."""
    m = fit.model
    (lpB, _pBt, lM) = O.lik_tables(b, bt, np.asarray(m.mu), np.asarray(m.sigma), m.eta, m.epsilon)
    fn = R.exact_log_evidence_shared if shared else R.exact_log_evidence
    return fn(O.sum_lp_B(lpB), lM, np.asarray(m.gamma, dtype=np.float64), fit._pi2())


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_log_evidence_against_the_enumeration(env, name, shared):
    """log_evidence() of both models on the four small cases at the cases' own parameters (put back after a short run():
    theta is the model's CURRENT one), 4096 chains, 50 rungs: |estimate - exact| <= 5 se, lower - 5 lower_se <= exact."""
    (N, U, m, b, bt) = case_data(name)
    fit = fitted(env, shared, b, bt, "gibbs" if shared else "vb", m)
    set_params(fit.model, m)
    (_N, _U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    exact = (R.exact_log_evidence_shared if shared else R.exact_log_evidence)(S_B, lM, gamma, pi2)
    out = fit.log_evidence(n_anneal=50, n_chains=4096, seed=seed)
    print("%s shared=%s exact %.4f estimate %.4f se %.4f ess %.0f lower %.4f (%.4f)" % (
        name, shared, exact, out["log_evidence"], out["log_evidence_se"], out["ess"], out["lower"], out["lower_se"]))
    assert out["n_chains"] == 4096 and out["n_anneal"] == 50
    assert abs(out["log_evidence"] - exact) <= 5.0 * out["log_evidence_se"]
    assert out["lower"] - 5.0 * out["lower_se"] <= exact
    # the same call again gives the same numbers (own key, fixed reduction order)
    again = fit.log_evidence(n_anneal=50, n_chains=4096, seed=seed)
    assert again == out


@pytest.mark.parametrize("source", ["unshared", "shared"])
def test_bayes_factor_against_the_exact_difference(env, source):
    """Data sampled from each model (Nreg 4, U 2): the difference of the two fits' log evidences, each at its own fitted
    theta, agrees with the exact difference within 5 x the combined standard error.  (No claim about its sign.)"""
    start = X.model("broad")
    if source == "unshared":
        (_r, _t, _f, _ft, b, bt) = start.sample_fast(4, 2, 2, seed=77)
    else:
        gen = env.pkg.SharedRegionModel()
        set_params(gen, start)
        (_r, _t, _f, _ft, b, bt) = gen.sample(4, 2, 2, seed=78)
    fu = fitted(env, False, b, bt, "vb", start)
    fs = fitted(env, True, b, bt, "vb", start)
    (eu, es) = (fu.log_evidence(n_anneal=50, n_chains=4096, seed=5), fs.log_evidence(n_anneal=50, n_chains=4096, seed=5))
    got = es["log_evidence"] - eu["log_evidence"]
    want = exact_at(fs, b, bt, True) - exact_at(fu, b, bt, False)
    se = float(np.hypot(es["log_evidence_se"], eu["log_evidence_se"]))
    print("%s data: log BF (shared - unshared) AIS %.4f exact %.4f combined se %.4f" % (source, got, want, se))
    assert abs(got - want) <= 5.0 * se


@pytest.mark.parametrize("shared", [False, True])
def test_the_fit_is_untouched(env, shared):
    (N, U, m, b, bt) = case_data("4x2")
    fit = fitted(env, shared, b, bt, "gibbs", m)
    before = (fit.model.theta().copy(), fit._lq_R.copy(), fit._lq_F.copy(), list(fit.energy), fit.sampler.f_state.clone(),
              fit.sampler.r_bits.clone(), fit._lM.copy(), fit._d["S_B"].clone(), fit.sampler)
    out = fit.log_evidence(n_anneal=8, n_chains=128)
    assert np.isfinite(out["log_evidence"])
    assert np.array_equal(fit.model.theta(), before[0])
    assert np.array_equal(fit._lq_R, before[1]) and np.array_equal(fit._lq_F, before[2])
    assert fit.energy == before[3] and fit.sampler is before[8]
    assert env.torch.equal(fit.sampler.f_state, before[4]) and env.torch.equal(fit.sampler.r_bits, before[5])
    assert np.array_equal(fit._lM, before[6]) and env.torch.equal(fit._d["S_B"], before[7])
    # n_chains=None takes the fit's
    assert fit.log_evidence(n_anneal=3)["n_chains"] == 64


CFG3_SCRIPT = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
import fcdiff_amd
gen = fcdiff_amd.UnsharedRegionModel()
(_r, _t, _f, _ft, b, bt) = gen.sample_fast(200, 50, 100, seed=0)
fit = fcdiff_amd.fit.UnsharedRegionFit()
fit.model, fit.b, fit.bt = fcdiff_amd.UnsharedRegionModel(), b, bt
fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in = "gibbs", 1024, 4, 2
fit.run()
out = fit.log_evidence(n_anneal=20)
fit._query_ctx.check_device()
fit._context().check_device()
print("RESULT " + json.dumps(out))
"""


def test_one_run_at_200_regions_100_patients(env):
    """Nreg 200, U 100, 1024 chains, 20 rungs, in a process of its own under a time limit: finite numbers, ess >= 1,
    lower <= log_evidence + 5 se, and no device-side error on either context."""
    p = subprocess.run([sys.executable, "-c", CFG3_SCRIPT % ROOT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240,
                       cwd=ROOT, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(out)
    for key in ("log_evidence", "log_evidence_se", "ess", "lower", "lower_se"):
        assert np.isfinite(out[key]), key
    assert out["ess"] >= 1.0 and out["n_chains"] == 1024 and out["n_anneal"] == 20
    assert out["lower"] <= out["log_evidence"] + 5.0 * out["log_evidence_se"]
