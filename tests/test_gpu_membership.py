"""
membership() on the device (fcd_member.hip, fcdiff_amd/membership.py): the kernel against the NumPy reference and against
the table path it replaces, its determinism, both models end to end against the enumerated predictive laws of N = 4, the
Bayes factor on drawn patients and controls, a fit left as it was, and the host's chunking.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import membership_ref as MR

pytestmark = pytest.mark.gpu

# The project's table-parity tolerance for sums over edges (tests/test_gpu_parity.py: SUM).  The numbers compared are sums of
# up to 780 log-densities of either sign and magnitude 1 to 10, so a sum can cancel to 1e-5 while both sides carry the rounding
# of its terms: with sum |terms| <= 1e4 and 1.1e-16 per operation that is up to ~1e-12 absolute, whatever the sum's own size.
# 1e-11 absolute is 1e-15 of sum |terms|; everything larger than 0.1 is held to 1e-10 relative.
SUM = dict(rtol=1e-10, atol=1e-11)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, membership, score
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.score, e.membership = torch, fcdiff_amd, _lib, score, membership
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def pack(env, f, r):
    """Packed chain state (f_state (GW, C, 64), r_bits (GW, N, U)) of plain f (G, C) and r (G, N, U)."""
    torch = env.torch
    (G, C) = f.shape
    (N, U) = r.shape[1:]
    GW = (G + 63) // 64
    f_state = torch.zeros((GW, C, 64), dtype=torch.uint8, device="cuda")
    r_bits = torch.zeros((GW, N, U), dtype=torch.int64, device="cuda")
    (f_d, r_d) = (up(env, f.astype(np.uint8)), up(env, r.astype(np.uint8)))           # (held until the import has run)
    env.ctx.call("fcd_gibbs_import_state", env.lib.dptr(f_d), env.lib.dptr(r_d), N, U, G, env.lib.dptr(f_state),
                 env.lib.dptr(r_bits), env.lib.stream_ptr())
    torch.cuda.synchronize()
    return f_state, r_bits


def model(env, shared=True):
    m = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.sigma = np.array([0.15, 0.15, 0.2])
    return m


def kernel(env, x, theta, f_state, r_bits, N, G, r_cols, missing, patient=True):
    (lc, lp) = env.membership.member_loglik(env.ctx, up(env, x), theta, f_state, r_bits, N, G, r_cols, missing, patient=patient)
    return lc.cpu().numpy(), (None if lp is None else lp.cpu().numpy())


def case(env, N, U, G, nan):
    rng = np.random.default_rng(1000 * N + 10 * U + G)
    m = model(env)
    (_r, _t, _f, _ft, _b, x) = m.sample(N, 1, U, seed=N + U)
    if nan:
        x = np.where(rng.random(x.shape) < 0.2, np.nan, x)
        x[0, 0] = np.nan
    C = N * (N - 1) // 2
    f = rng.integers(0, 3, size=(G, C))
    r = (rng.random((G, N, U)) < 0.4).astype(np.int64)
    return m.theta(), x, f, r


def rel_err(got, want):
    """Largest |got - want| / |want| over the entries where that is a number (printed beside the assertion)."""
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130, 1100])
@pytest.mark.parametrize("U", [1, 3, 70])
@pytest.mark.parametrize("N", [4, 17, 40])
def test_kernel_against_reference(env, N, U, G):
    """
    fcd_member_loglik on random states against membership_ref at 1e-10 relative: r one column per subject and one column for
    all, clean data, NaN with the flag (adds 0) and without it (NaN comes out), and the control side alone (out_patient
    NULL), which equals the control side of the full call exactly.
    """
    for nan in (False, True):
        (theta, x, f, r) = case(env, N, U, G, nan)
        for missing in ((False, True) if nan else (False,)):
            want_c = MR.control_loglik(x, theta, f, missing)
            (f_state, r_bits) = pack(env, f, r)
            (lc, lp) = kernel(env, x, theta, f_state, r_bits, N, G, U, missing)
            want_p = MR.patient_loglik(x, theta, f, r, missing)
            print("N=%d U=%d G=%d nan=%s missing=%s r_cols=U: max rel err control %.2e patient %.2e"
                  % (N, U, G, nan, missing, rel_err(lc, want_c), rel_err(lp, want_p)))
            nptest.assert_allclose(lc, want_c, **SUM)
            nptest.assert_allclose(lp, want_p, **SUM)
            if nan and not missing:
                assert np.isnan(lc[:, 0]).all() and np.isnan(lp[:, 0]).all()
            (f_state1, r_bits1) = pack(env, f, r[:, :, :1])
            (lc1, lp1) = kernel(env, x, theta, f_state1, r_bits1, N, G, 1, missing)
            nptest.assert_array_equal(lc1, lc)           # (equal numbers; a NaN's sign and payload are not compared)
            nptest.assert_allclose(lp1, MR.patient_loglik(x, theta, f, r[:, :, 0], missing), **SUM)
            (lc0, none) = kernel(env, x, theta, f_state, None, N, G, 1, missing, patient=False)
            assert none is None
            nptest.assert_array_equal(lc0, lc)


@pytest.mark.parametrize("N,U,G,missing", [(4, 3, 65, False), (17, 70, 130, True), (40, 3, 1100, False), (200, 5, 64, False)])
def test_patient_side_against_the_table_path(env, N, U, G, missing):
    """out_patient = fcd_lik_tables + one fcd_score_ais_step from beta 0 to 1 on the same state with r broadcast."""
    torch = env.torch
    (theta, x, f, r) = case(env, N, U, G, missing)
    r = np.repeat(r[:, :, :1], U, axis=2)
    (f_state, r_bits) = pack(env, f, r)
    b = np.zeros((x.shape[0], 1))
    (_S_B, lM) = env.score.lik_tables(env.ctx, up(env, b), up(env, x), theta, missing)
    w = torch.zeros((G, U), dtype=torch.float64, device="cuda")
    env.ctx.call("fcd_score_ais_step", env.lib.dptr(lM), env.lib.dptr(f_state), env.lib.dptr(r_bits), N, U, G, 0.0, 1.0,
                 env.lib.dptr(w), env.lib.dptr(None), env.lib.stream_ptr())
    (f_state1, r_bits1) = pack(env, f, r[:, :, :1])
    (_lc, lp) = kernel(env, x, theta, f_state1, r_bits1, N, G, 1, missing)
    nptest.assert_allclose(lp, w.cpu().numpy(), **SUM)
    (_lc, lpU) = kernel(env, x, theta, f_state, r_bits, N, G, U, missing)
    nptest.assert_allclose(lpU, w.cpu().numpy(), **SUM)


@pytest.mark.parametrize("N,U", [(17, 3), (40, 70)])
def test_kernel_is_deterministic_and_chains_are_independent(env, N, U):
    """Two runs agree bit for bit, and chain g's row at G = 130 is its row when only the first 64 or 65 chains are run."""
    (theta, x, f, r) = case(env, N, U, 130, False)
    for r_cols in (U, 1):
        rr = r if r_cols == U else r[:, :, :1]
        (f_state, r_bits) = pack(env, f, rr)
        (lc, lp) = kernel(env, x, theta, f_state, r_bits, N, 130, r_cols, False)
        (lc2, lp2) = kernel(env, x, theta, f_state, r_bits, N, 130, r_cols, False)
        assert lc.tobytes() == lc2.tobytes() and lp.tobytes() == lp2.tobytes()
        for G in (64, 65):
            (fs, rb) = pack(env, f[:G], rr[:G])
            (lcg, lpg) = kernel(env, x, theta, fs, rb, N, G, r_cols, False)
            assert lcg.tobytes() == lc[:G].tobytes() and lpg.tobytes() == lp[:G].tobytes()


def test_kernel_refusals(env):
    (theta, x, f, r) = case(env, 4, 3, 64, False)
    (f_state, r_bits) = pack(env, f, r)
    with pytest.raises(ValueError):
        kernel(env, x, theta, f_state, r_bits, 4, 64, 2, False)                      # r_cols neither 1 nor U
    (th, _th) = env.lib.dbl_array(theta)
    out = env.torch.empty((64, 3), dtype=env.torch.float64, device="cuda")
    with pytest.raises(ValueError):                                                    # the patient side without r
        env.ctx.call("fcd_member_loglik", env.lib.dptr(up(env, x)), th, env.lib.dptr(f_state), env.lib.dptr(None), 4, 3, 64, 1,
                     0, env.lib.dptr(out), env.lib.dptr(env.torch.empty_like(out)), env.lib.stream_ptr())
    with pytest.raises(ValueError):                                                    # unknown flag
        env.ctx.call("fcd_member_loglik", env.lib.dptr(up(env, x)), th, env.lib.dptr(f_state), env.lib.dptr(None), 4, 3, 64, 1,
                     8, env.lib.dptr(out), env.lib.dptr(None), env.lib.stream_ptr())


G_FIT = 4096


def fitted(env, shared, b, bt, m, G=G_FIT, **kw):
    fit = env.pkg.fit.SharedRegionFit() if shared else env.pkg.fit.UnsharedRegionFit()
    (fit.model, fit.b, fit.bt) = (m, b, bt)
    (fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.mstep_every, fit.seed) = ("gibbs", G, 40, 30, 0, 5)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit


def snapshot(fit):
    (f, r) = fit.sampler.export_state()
    return (np.asarray(fit.model.theta()).tobytes(), fit.sampler.f_state.cpu().numpy().tobytes(),
            fit.sampler.r_bits.cpu().numpy().tobytes(), np.asarray(fit.energy).tobytes(), f.tobytes(), r.tobytes())


@pytest.mark.parametrize("shared", [True, False])
def test_end_to_end_against_enumeration(env, shared):
    """
    N = 4, data from the model's sampler (3 new patients and 3 new controls held out of one draw), G = 4096 chains after 30
    sweeps of burn-in.  log_control (both models) and the shared log_patient lie within 5 EXACT standard errors of the
    enumerated value, se = sqrt(Var_post[e^l] / G) / E_post[e^l] from the enumeration (a correct sampler fails with
    probability < 1e-6 per number).  The unshared log_patient carries AIS noise on top: within 5 reported standard errors,
    and ess >= G / 8 -- the enumerated law alone (no AIS noise) has ess / G = 1 / (1 + rel^2) >= 1 / 4 here, which the test
    checks first, so n_anneal = 200 leaves a factor of two for the ladder.  The call leaves the fit as it was.
    """
    m = model(env, shared)
    draw = m.sample(4, 2 + 3, 3 + 3, seed=11) if shared else m.sample_fast(4, 2 + 3, 3 + 3, seed=11)
    (b, bt) = (draw[4], draw[5])
    x_new = np.concatenate([bt[:, 3:], b[:, 2:]], axis=1)
    fit = fitted(env, shared, b[:, :2], bt[:, :3], m)
    before = snapshot(fit)
    out = fit.membership(x_new, n_anneal=200, seed=3)
    assert snapshot(fit) == before
    ex = (MR.exact_shared if shared else MR.exact_unshared)(b[:, :2], bt[:, :3], fit.model.theta(), x_new)
    assert out["n_chains"] == G_FIT
    for key in ("log_patient", "log_patient_se", "ess_patient", "log_control", "log_control_se", "ess_control", "log_bf",
                "log_bf_se"):
        assert out[key].shape == (6,) and out[key].dtype == np.float64
    se_c = ex["rel_control"] / np.sqrt(G_FIT)
    print("control  got %s exact %s exact se %s reported se %s" % (out["log_control"], ex["log_control"], se_c,
                                                                   out["log_control_se"]))
    print("patient  got %s exact %s exact se %s reported se %s ess %s" % (out["log_patient"], ex["log_patient"],
          ex["rel_patient"] / np.sqrt(G_FIT), out["log_patient_se"], out["ess_patient"]))
    assert np.all(np.abs(out["log_control"] - ex["log_control"]) <= 5 * se_c)
    if shared:
        assert np.all(np.abs(out["log_patient"] - ex["log_patient"]) <= 5 * ex["rel_patient"] / np.sqrt(G_FIT))
    else:
        assert np.all(1.0 / (1.0 + ex["rel_patient"] ** 2) >= 0.25)                 # the condition on the enumerated law
        assert np.all(np.abs(out["log_patient"] - ex["log_patient"]) <= 5 * out["log_patient_se"])
        assert np.all(out["ess_patient"] >= G_FIT / 8)
    nptest.assert_array_equal(out["log_bf"], out["log_patient"] - out["log_control"])
    nptest.assert_array_equal(out["log_bf_se"], np.sqrt(out["log_patient_se"] ** 2 + out["log_control_se"] ** 2))
    again = fit.membership(x_new, n_anneal=200, seed=3)
    for key in out:
        nptest.assert_array_equal(again[key], out[key])


@pytest.mark.parametrize("shared", [True, False])
def test_bayes_factor_separates_patients_from_controls(env, shared):
    """Held-out subjects of one draw of a well-separated model: the patients with anomalous regions have the larger mean
    log_bf (enumerated at these seeds: about +20 to +45 nats against -2 to -10 for the controls)."""
    m = model(env, shared)
    m.pi, m.eta, m.epsilon = 0.4, 0.9, 0.05
    m.sigma = np.array([0.06, 0.06, 0.08])
    if shared:
        (r, _t, _f, _ft, b, bt) = m.sample(4, 3 + 6, 4 + 6, seed=2)
        assert r.sum() >= 2
        anomalous = np.ones(6, dtype=bool)
    else:
        (r, _t, _f, _ft, b, bt) = m.sample_fast(4, 3 + 6, 4 + 12, seed=1)
        anomalous = r[:, 4:].sum(axis=0) >= 2
        assert anomalous.sum() >= 3
    fit = fitted(env, shared, b[:, :3], bt[:, :4], m, G=1024)
    pat = fit.membership(bt[:, 4:], n_anneal=100)["log_bf"][anomalous]
    ctl = fit.membership(b[:, 3:], n_anneal=100)["log_bf"]
    print("log_bf patients %s controls %s" % (pat, ctl))
    assert np.all(np.isfinite(pat)) and np.all(np.isfinite(ctl))
    assert pat.mean() > ctl.mean()


@pytest.mark.parametrize("shared", [True, False])
def test_chunked_cohort_equals_separate_calls(env, shared):
    """CHUNK + 1 subjects give, bit for bit, what the first CHUNK and the last one give when scored apart."""
    m = model(env, shared)
    draw = m.sample(4, 2, 3, seed=4) if shared else m.sample_fast(4, 2, 3, seed=4)
    fit = fitted(env, shared, draw[4], draw[5], m, G=192)
    n = env.membership.CHUNK
    x = (m.sample(4, 1, n + 1, seed=9) if shared else m.sample_fast(4, 1, n + 1, seed=9))[5]
    whole = fit.membership(x, n_anneal=5)
    (a, b) = (fit.membership(x[:, :n], n_anneal=5), fit.membership(x[:, n:], n_anneal=5))
    assert whole["n_chains"] == a["n_chains"] == b["n_chains"] == 192
    for key in whole:
        if key != "n_chains":
            assert whole[key].shape == (n + 1,)
            nptest.assert_array_equal(whole[key], np.concatenate([a[key], b[key]]))
    assert np.isfinite(whole["log_bf"]).all()


def test_unobserved_subject(env):
    """missing_data: an all-NaN subject has likelihood 1 on both sides of both models, exactly."""
    for shared in (True, False):
        m = model(env, shared)
        draw = m.sample(4, 2, 3, seed=6) if shared else m.sample_fast(4, 2, 3, seed=6)
        fit = fitted(env, shared, draw[4], draw[5], m, G=128, missing_data=True)
        x = draw[5][:, :2].copy()
        x[:, 0] = np.nan
        out = fit.membership(x, n_anneal=10)
        assert out["log_patient"][0] == 0.0 and out["log_control"][0] == 0.0 and out["log_bf"][0] == 0.0
        assert out["ess_patient"][0] == 128.0 and out["ess_control"][0] == 128.0
        assert np.isfinite(out["log_bf"][1])
