"""
The subtype-region model on the MI355X: the weighted table sum (fcd_lik_weighted_tables) and the per-(patient, subtype)
expected log-likelihood (fcd_vb_subtype_loglik) against NumPy contractions of the device's own per-patient table, against the
existing kernels they generalise (fcd_lik_grouped_tables at one-hot weights, fcd_vb_patient_elbo column by column), at the
shapes where their lane loops, patient blocks, edge slices and the capped grid of the exponentials wrap; then SubtypeRegionFit against the NumPy loop of
tests/subtype_region_ref.py iteration by iteration, and its queries.

Tolerance rules.  The weighted sum: per entry U 2^-52 sum_u |s lM|, the bound of a reordered fp64 sum of U terms.  The
log-likelihood: (9 C + 16) 2^-52 sum |q_F w lM| per (u, g): 9 C terms in another order, and 16 for the roundings inside a term
(three exponentials, three products).  The fit: test_gpu_grouped_region.py's rule for fits on reference tables.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import sessions_ref as SR
import subtype_region_ref as R
from conftest import theta_dict
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu

FIT = dict(rtol=1e-10, atol=1e-12)                  # test_gpu_grouped_region.py's rule for the fits on reference tables
EPS = 2.0 ** -52
U_SIZES = (1, 7, 63, 64, 65, 130)                   # 7 patients per wave pass and 64 per block: below, at and past both
G_SIZES = (1, 2, 3, 8)
PLANTED_LABELS = [0] * 12 + [1] * 12


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.tables = torch, fcdiff_amd, _lib, tables
    e.ctx = _lib.Context()
    e.cache = {}
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def device_table(env, N, U, sessions=None):
    """(model, b, bt, lM device (C, U, 3, 3)): the device's own per-patient table of a sampled case, made once per shape."""
    key = (N, U, sessions)
    if key not in env.cache:
        m = env.pkg.UnsharedRegionModel()
        m.pi = 0.2
        (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 3, U, seed=N + U, sessions=sessions)
        (_S_B, lM) = env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), 0)
        env.cache[key] = (m, b, bt, lM)
    return env.cache[key]


def random_resp(U, G, seed, zeros=True):
    rng = np.random.default_rng(seed)
    s = rng.dirichlet(np.ones(G), size=U)
    if zeros and G > 1:                              # some weights exactly 0, some rows one-hot
        s[rng.random((U, G)) < 0.2] = 0.0
        s[s.sum(axis=1) == 0, 0] = 1.0
        s /= s.sum(axis=1, keepdims=True)
    return np.ascontiguousarray(s)


def random_q(N, G, seed):
    """(lq_F (C, 1, 3), lq_R (N, G, 2)): normalised random log-probabilities."""
    rng = np.random.default_rng(seed)
    C = N * (N - 1) // 2
    lq_F = np.log(rng.dirichlet(np.ones(3), size=C))[:, None, :]
    lq_R = np.log(rng.dirichlet(np.ones(2), size=(N, G)))
    return np.ascontiguousarray(lq_F), np.ascontiguousarray(lq_R)


def weighted(env, lM, resp):
    (C, U) = (int(lM.shape[0]), int(lM.shape[1]))
    G = resp.shape[1]
    L = env.torch.full((C, G, 3, 3), np.nan, dtype=env.torch.float64, device="cuda")
    resp_d = up(env, resp)
    env.ctx.call("fcd_lik_weighted_tables", env.lib.dptr(lM), env.lib.dptr(resp_d), C, U, G, env.lib.dptr(L), env.lib.stream_ptr())
    return L.cpu().numpy()


def loglik(env, lq_F, lq_R, lM):
    (N, G) = lq_R.shape[:2]
    U = int(lM.shape[1])
    E = env.torch.full((U, G), np.nan, dtype=env.torch.float64, device="cuda")
    (lq_F_d, lq_R_d) = (up(env, lq_F), up(env, lq_R))               # (held until the result is read)
    env.ctx.call("fcd_vb_subtype_loglik", env.lib.dptr(lq_F_d), env.lib.dptr(lq_R_d), env.lib.dptr(lM), N, U, G, env.lib.dptr(E),
                 env.lib.stream_ptr())
    return E.cpu().numpy()


def loglik_reference(lq_F, lq_R, lM):
    """(E, sum of |terms|), both (U, G), by NumPy."""
    ep = O.edge_endpoints(lq_R.shape[0])
    (n, m) = (ep[:, 0], ep[:, 1])
    (q_R, q_F) = (np.exp(lq_R), np.exp(lq_F)[:, 0, :])
    w = np.stack([q_R[n, :, 0] * q_R[m, :, 0], q_R[n, :, 1] * q_R[m, :, 1],
                  q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]], axis=2)
    return np.einsum("ck,cgl,cukl->ug", q_F, w, lM), np.einsum("ck,cgl,cukl->ug", q_F, w, np.abs(lM))


def check_weighted(env, lM, G, seed):
    lM_h = lM.cpu().numpy()
    U = lM_h.shape[1]
    s = random_resp(U, G, seed)
    got = weighted(env, lM, s)
    want = np.einsum("ug,cukl->cgkl", s, lM_h)
    bound = U * EPS * np.einsum("ug,cukl->cgkl", s, np.abs(lM_h))
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= bound), (U, G, np.abs(got - want).max())
    nptest.assert_array_equal(weighted(env, lM, s), got)                 # a fixed summation order: bit for bit


def check_loglik(env, N, lM, G, seed):
    lM_h = lM.cpu().numpy()
    (C, U) = lM_h.shape[:2]
    (lq_F, lq_R) = random_q(N, G, seed)
    got = loglik(env, lq_F, lq_R, lM)
    (want, mag) = loglik_reference(lq_F, lq_R, lM_h)
    bound = (9 * C + 16) * EPS * mag
    assert np.all(np.abs(got - want) <= bound), (N, U, G, np.abs(got - want).max())
    nptest.assert_array_equal(loglik(env, lq_F, lq_R, lM), got)
    return lq_F, lq_R, got, bound


# ------------------------------------------------------------------------------------------------
# 1. the two kernels against NumPy, at every shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 12, 24])
def test_weighted_tables_against_einsum(env, N):
    for U in U_SIZES:
        (_m, _b, _bt, lM) = device_table(env, N, U)
        for G in G_SIZES:
            check_weighted(env, lM, G, seed=100 * U + G)


@pytest.mark.parametrize("N", [3, 12, 24])
def test_subtype_loglik_against_numpy(env, N):
    for U in U_SIZES:
        (_m, _b, _bt, lM) = device_table(env, N, U)
        for G in G_SIZES:
            check_loglik(env, N, lM, G, seed=100 * U + G)


def test_both_kernels_past_the_slice_cap(env):
    """N = 363: C = 65 703 edges, more than the 1024 slices of 64 edges the log-likelihood's grid is capped at."""
    (_m, _b, _bt, lM) = device_table(env, 363, 3)
    assert int(lM.shape[0]) == 65703 > 1024 * 64
    check_weighted(env, lM, 2, seed=1)
    check_loglik(env, 363, lM, 2, seed=2)


def test_both_kernels_past_the_grid_cap_of_the_exponentials(env):
    """
    subtype_exp_kernel makes q_F (3 C numbers) and q_R (2 N G) in one grid-stride loop whose grid is capped at 8 workgroups
    of 256 threads per CU: the smallest N with 3 C above that many threads makes the loop wrap, with the end of q_F and
    all of q_R in a thread's second pass (N = 592, C = 174 936 on 256 CUs).  It is past the slice cap too.
    """
    threads = 8 * 256 * env.torch.cuda.get_device_properties(0).multi_processor_count
    N = 3
    while 3 * (N * (N - 1) // 2) <= threads:
        N += 1
    (U, G) = (2, 2)
    (_m, _b, _bt, lM) = device_table(env, N, U)
    C = int(lM.shape[0])
    assert 3 * C > threads and 3 * C + 2 * N * G < 2 * threads and C > 1024 * 64
    check_weighted(env, lM, G, seed=3)
    check_loglik(env, N, lM, G, seed=4)


@pytest.mark.parametrize("U, G", [(65, 3), (64, 1), (23, 2), (7, 2)])
def test_one_hot_weights_give_the_grouped_table(env, U, G):
    """
    The sessions-form table (bt (C, U, 1)) is the one whose entries fcd_lik_grouped_tables sums: only the order differs.
    One subtype is the shared table.  U: a multiple of the 7 patients of a wave pass and not, of the 64 of a lane group and not.
    """
    N = 12
    (m, b, bt, lM) = device_table(env, N, U, sessions=1)
    labels = (np.random.default_rng(3).permutation(U) % G).tolist()
    s = np.zeros((U, G))
    s[np.arange(U), labels] = 1.0
    got = weighted(env, lM, s)
    (_names, offsets, order) = env.pkg.fit.group_labels_csr(labels, U)
    (b_d, bt_d) = (up(env, b), up(env, bt))
    (_S_B, L) = env.tables.build(env.ctx, b_d, bt_d, m.theta(), 0, groups=(up(env, order), up(env, offsets), G))
    bound = U * EPS * np.einsum("ug,cukl->cgkl", s, np.abs(lM.cpu().numpy()))
    assert np.all(np.abs(got - L.cpu().numpy()) <= bound)
    if G == 1:
        (_S_B, L1) = env.tables.build(env.ctx, b_d, bt_d, m.theta(), 0, shared=True)
        assert tuple(L1.shape) == (66, 1, 3, 3)
        assert np.all(np.abs(got - L1.cpu().numpy()) <= bound)


def test_zero_weight_on_minus_infinity_adds_nothing(env):
    (_m, _b, _bt, lM) = device_table(env, 12, 7)
    lM = lM.clone()
    lM[5, 2, 1, :] = -np.inf
    lM[9, 2] = -np.inf
    s = random_resp(7, 3, seed=4, zeros=False)
    s[2] = [0.0, 0.25, 0.75]
    got = weighted(env, lM, s)
    assert np.all(np.isfinite(got[:, 0])) and not np.any(np.isnan(got))
    assert np.all(np.isneginf(got[5, 1:, 1, :])) and np.all(np.isneginf(got[9, 1:]))
    finite = lM.cpu().numpy().copy()
    finite[~np.isfinite(finite)] = 0.0
    want = np.einsum("ug,cukl->cgkl", s, finite)
    ok = np.isfinite(got)
    assert np.all(np.abs(got - want)[ok] <= 7 * EPS * np.einsum("ug,cukl->cgkl", s, np.abs(finite))[ok])


def test_loglik_column_is_the_patient_elbo_term(env):
    """Column g against fcd_vb_patient_elbo's E_lM[u] with subtype g's q_R broadcast to every patient."""
    (N, U, G) = (12, 65, 3)
    (_m, _b, _bt, lM) = device_table(env, N, U)
    (lq_F, lq_R, got, bound) = check_loglik(env, N, lM, G, seed=11)
    hyper = env.tables.write_hyper(env.ctx, env.torch.zeros(8, dtype=env.torch.float64, device="cuda"), [0.1, 0.8, 0.1], [0.9, 0.1])
    lq_F_d = up(env, lq_F)
    for g in range(G):
        col = up(env, np.repeat(lq_R[:, g:g + 1, :], U, axis=1))
        out4 = env.torch.empty((U, 4), dtype=env.torch.float64, device="cuda")
        env.ctx.call("fcd_vb_patient_elbo", env.lib.dptr(lq_F_d), env.lib.dptr(col), env.lib.dptr(lM), env.lib.dptr(hyper), N, U,
                     env.lib.dptr(out4), env.lib.stream_ptr())
        assert np.all(np.abs(got[:, g] - out4.cpu().numpy()[:, 0]) <= bound[:, g])


def test_a_patients_row_does_not_depend_on_the_other_patients(env):
    (N, U, G) = (24, 130, 8)
    (_m, _b, _bt, lM) = device_table(env, N, U)
    (lq_F, lq_R) = random_q(N, G, seed=12)
    full = loglik(env, lq_F, lq_R, lM)
    for u in (0, 63, 64, 129):
        alone = loglik(env, lq_F, lq_R, lM[:, u:u + 1].contiguous())
        nptest.assert_array_equal(alone[0], full[u])
    nptest.assert_array_equal(loglik(env, lq_F, lq_R, lM[:, 60:70].contiguous()), full[60:70])


def test_entry_point_refusals(env):
    (_m, _b, _bt, lM) = device_table(env, 12, 7)
    (d, sp) = (env.lib.dptr, env.lib.stream_ptr)
    resp = up(env, random_resp(7, 2, 0))
    L = env.torch.empty((66, 2, 3, 3), dtype=env.torch.float64, device="cuda")
    (lq_F, lq_R) = [up(env, a) for a in random_q(12, 2, 0)]
    E = env.torch.empty((7, 2), dtype=env.torch.float64, device="cuda")

    def wt(lM_=lM, resp_=resp, C=66, U=7, G=2, L_=L):
        env.ctx.call("fcd_lik_weighted_tables", d(lM_), d(resp_), C, U, G, d(L_), sp())

    def ll(lq_F_=lq_F, lq_R_=lq_R, lM_=lM, N=12, U=7, G=2, E_=E):
        env.ctx.call("fcd_vb_subtype_loglik", d(lq_F_), d(lq_R_), d(lM_), N, U, G, d(E_), sp())
    for kw in (dict(lM_=None), dict(resp_=None), dict(L_=None), dict(G=0), dict(G=9), dict(U=0), dict(L_=lM)):
        with pytest.raises(ValueError):
            wt(**kw)
    for C in (65, 67, 0):
        with pytest.raises(ValueError, match="triangular"):
            wt(C=C)
    with pytest.raises(NotImplementedError):
        wt(U=(1 << 24) + 1)
    for kw in (dict(lq_F_=None), dict(lq_R_=None), dict(lM_=None), dict(E_=None), dict(G=0), dict(G=9), dict(U=0), dict(N=1)):
        with pytest.raises(ValueError):
            ll(**kw)
    for kw in (dict(N=46341), dict(U=(1 << 24) + 1)):
        with pytest.raises(NotImplementedError):
            ll(**kw)
    wt()                                             # the context still works after the refusals
    ll()
    assert np.all(np.isfinite(E.cpu().numpy())) and np.all(np.isfinite(L.cpu().numpy()))


# ------------------------------------------------------------------------------------------------
# 2. the fit against the NumPy loop
# ------------------------------------------------------------------------------------------------
def planted_case(env, variant):
    """(b, bt, missing): the planted case of the issue, or its variant of two sessions with NaN entries."""
    m = env.pkg.GroupedRegionModel()
    if variant == "plain":
        (_r, _t, _f, _ft, b, bt) = m.sample(12, 24, PLANTED_LABELS, seed=0)
        return b, bt, False
    (_r, _t, _f, _ft, b, bt) = m.sample(12, 24, PLANTED_LABELS, seed=0, sessions=2)
    rng = np.random.default_rng(8)
    (b, bt) = (b.copy(), bt.copy())
    bt[rng.random(bt.shape) < 0.1] = np.nan
    bt[7, 3, :] = np.nan                             # an item with no observed session
    b[rng.random(b.shape) < 0.05] = np.nan
    return b, bt, True


def new_fit(env, b, bt, missing=False, **kw):
    fit = env.pkg.fit.SubtypeRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (env.pkg.SubtypeRegionModel(), b, bt)
    (fit.n_subtypes, fit.missing_data) = (2, missing)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


@pytest.fixture(scope="module")
def references(env):
    """Per variant: the data and the reference's four restarts of 30 iterations, computed once."""
    out = {}
    for variant in ("plain", "sessions_nan"):
        (b, bt, missing) = planted_case(env, variant)
        th = theta_dict(env.pkg.SubtypeRegionModel().theta())
        (S_B, lM) = R.tables(b, bt, th, missing=missing)
        fits = [R.vb_fit(S_B, lM, R.default_init(24, 2, 0, i), th["pi"], th["gamma"], alpha=1.0, iters=30) for i in range(4)]
        out[variant] = dict(b=b, bt=bt, missing=missing, fits=fits)
    return out


@pytest.mark.parametrize("variant", ["plain", "sessions_nan"])
def test_fit_tracks_the_reference_iteration_by_iteration(env, references, variant):
    ref = references[variant]
    want = ref["fits"][1]
    s0 = R.default_init(24, 2, 0, 1)
    for iters in (1, 2, 3, 6):
        fit = new_fit(env, ref["b"], ref["bt"], ref["missing"], init_responsibilities=s0, max_iters=iters, rel_tol=-np.inf)
        fit.run()
        assert len(fit.energy) == iters + 1 and fit.restart_energies == [fit.energy[-1]]
        nptest.assert_allclose(fit.energy, want["energy"][:iters + 1], **FIT)
        (lq_F, lq_R, pi, gamma, resp) = want["hist"][iters - 1]
        order = np.argsort(-resp.sum(axis=0), kind="stable")
        nptest.assert_allclose(fit._lq_F, lq_F, **FIT)
        nptest.assert_allclose(fit._lq_R, lq_R[:, order], **FIT)
        nptest.assert_allclose(fit.model.pi, pi, **FIT)
        nptest.assert_allclose(fit.model.gamma, gamma, **FIT)
        nptest.assert_allclose(fit.responsibilities, resp[:, order], rtol=0, atol=1e-8)
        assert list(fit.responsibilities.argmax(axis=1)) == list(resp[:, order].argmax(axis=1))
        assert fit._lM.shape == (66, 2, 3, 3) and fit._lM_patients.shape == (66, 24, 3, 3) and fit._lq_R.shape == (12, 2, 2)
        bound = 24 * EPS * np.einsum("ug,cukl->cgkl", fit.responsibilities, np.abs(fit._lM_patients))
        assert np.all(np.abs(fit._lM - np.einsum("ug,cukl->cgkl", fit.responsibilities, fit._lM_patients)) <= bound)
    if ref["missing"]:
        assert fit.n_sessions == 2
        assert fit.missing_counts() == (int(np.isnan(ref["b"]).sum()), int(np.isnan(ref["bt"]).sum()))


@pytest.mark.parametrize("variant", ["plain", "sessions_nan"])
def test_default_run_keeps_the_best_restart_and_finds_the_planted_labels(env, references, variant):
    ref = references[variant]
    fit = new_fit(env, ref["b"], ref["bt"], ref["missing"], max_iters=30, rel_tol=-np.inf)
    fit.run()
    finals = [out["energy"][-1] for out in ref["fits"]]
    nptest.assert_allclose(fit.restart_energies, finals, rtol=1e-9)
    best = R.renumbered(ref["fits"][int(np.argmin(fit.restart_energies))])
    nptest.assert_allclose(fit.energy[-1], min(finals), rtol=1e-9)
    nptest.assert_allclose(fit.responsibilities, best["resp"], rtol=0, atol=1e-8)
    labels = fit.subtype_posterior()["labels"]
    assert list(labels) == list(best["resp"].argmax(axis=1))
    truth = np.array(PLANTED_LABELS)
    assert max((labels == truth).sum(), (labels == 1 - truth).sum()) == 24
    assert np.all(np.diff(fit.energy) <= 1e-9 * np.abs(fit.energy[:-1]))
    n = fit.responsibilities.sum(axis=0)
    assert n[0] >= n[1]


# ------------------------------------------------------------------------------------------------
# 3. the queries
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(env, references):
    ref = references["sessions_nan"]
    fit = new_fit(env, ref["b"], ref["bt"], True, max_iters=30, rel_tol=-np.inf, n_restarts=2)
    fit.run()
    return fit


def snapshot(fit):
    return dict(lq_R=fit._lq_R.copy(), lq_F=fit._lq_F.copy(), lM=fit._lM.copy(), lM_u=fit._lM_patients.copy(),
                S_B=fit._d["S_B"].cpu().numpy(), resp=fit.responsibilities.copy(), energy=list(fit.energy),
                restarts=list(fit.restart_energies), pi=float(fit.model.pi), gamma=np.array(fit.model.gamma))


def test_subtype_and_region_posteriors(fitted):
    out = fitted.subtype_posterior()
    s = fitted.responsibilities
    nptest.assert_array_equal(out["responsibilities"], s)
    nptest.assert_array_equal(out["labels"], s.argmax(axis=1))
    nptest.assert_allclose(out["n_effective"], s.sum(axis=0), rtol=1e-15)
    nptest.assert_allclose(out["rho_mean"], (1.0 + s.sum(axis=0)) / (2.0 + 24), rtol=1e-15)
    nptest.assert_allclose(out["coassignment"], s @ s.T, rtol=1e-15)
    assert out["coassignment"].shape == (24, 24) and abs(out["rho_mean"].sum() - 1) < 1e-14
    reg = fitted.region_posterior()
    assert reg["subtype_names"] == [0, 1]
    nptest.assert_allclose(reg["p_region"], np.exp(fitted._lq_R[:, :, 1]), rtol=1e-15)
    # inherited, with the subtypes as their "patients"
    pc = fitted.anomaly_count_posterior()
    assert pc["p_patient_count"].shape == (2, 13) and pc["p_region_count"].shape == (12, 3)
    co = fitted.coanomaly_posterior()
    assert co["p_patient_pair"].shape == (2, 2) and co["p_region_pair"].shape == (12, 12)


def test_assign_on_the_fits_own_patients_returns_its_responsibilities(fitted):
    """After 30 iterations the fit is at its fixed point: n, and with it q(rho), no longer moves between two steps."""
    out = fitted.assign(fitted.bt)
    assert out["responsibilities"].shape == (24, 2) and out["expected_loglik"].shape == (24, 2)
    nptest.assert_allclose(out["responsibilities"], fitted.responsibilities, rtol=0, atol=1e-8)
    # one patient, one session of it: any K', and a row does not depend on the other patients of the call
    one = fitted.assign(fitted.bt[:, 5:6, :])
    nptest.assert_array_equal(one["expected_loglik"][0], out["expected_loglik"][5])
    first = fitted.assign(fitted.bt[:, :, 0])
    assert first["responsibilities"].shape == (24, 2) and np.all(np.isfinite(first["expected_loglik"]))
    nptest.assert_allclose(first["responsibilities"].sum(axis=1), 1.0, rtol=1e-14)
    with pytest.raises(ValueError, match="connections"):
        fitted.assign(fitted.bt[:10])


def test_connection_posterior_with_one_hot_responsibilities_is_the_grouped_fits(env, references):
    ref = references["sessions_nan"]
    grouped = env.pkg.fit.GroupedRegionFit()
    grouped._ctx = env.ctx
    (grouped.model, grouped.b, grouped.bt) = (env.pkg.GroupedRegionModel(), ref["b"], ref["bt"])
    (grouped.group_labels, grouped.missing_data, grouped.max_iters) = (PLANTED_LABELS, True, 3)
    grouped.run()
    want = grouped.connection_posterior()
    fit = new_fit(env, ref["b"], ref["bt"], True, max_iters=1, n_restarts=1)
    fit.run()
    onehot = np.zeros((24, 2))
    onehot[np.arange(24), PLANTED_LABELS] = 1.0
    (fit._lq_R, fit._lq_F, fit.responsibilities) = (grouped._lq_R, grouped._lq_F, onehot)
    (fit.model.pi, fit.model.gamma) = (grouped.model.pi, grouped.model.gamma)
    got = fit.connection_posterior()
    for key in ("p_T", "p_F_tilde", "p_changed"):
        assert got[key].shape == want[key].shape
        nptest.assert_array_equal(got[key], want[key], err_msg=key)     # weights of exactly 1 and 0: the same numbers
    # soft responsibilities: the mixture of the two one-hot answers
    (fit.responsibilities, a) = (onehot[:, ::-1].copy(), got)
    b = fit.connection_posterior()
    s = np.full((24, 2), 0.5)
    s[:, 0] = np.linspace(0.1, 0.9, 24)
    s[:, 1] = 1 - s[:, 0]
    fit.responsibilities = s
    mix = fit.connection_posterior()
    # patient u of group z has a's answer at weight s[u, z] and b's at the other
    wa = s[np.arange(24), PLANTED_LABELS]
    nptest.assert_allclose(mix["p_T"], wa[None, :] * a["p_T"] + (1 - wa)[None, :] * b["p_T"], rtol=1e-13, atol=1e-15)
    nptest.assert_allclose(mix["p_F_tilde"].sum(axis=2), 1.0, rtol=1e-12)


def test_every_query_leaves_the_fit_unchanged(fitted):
    before = snapshot(fitted)
    fitted.subtype_posterior()
    fitted.region_posterior()
    fitted.connection_posterior()
    fitted.assign(fitted.bt[:, :3, :])
    fitted.anomaly_count_posterior()
    fitted.coanomaly_posterior()
    fitted.region_sets = {"a": [0, 1, 2], "b": [3, 11]}
    out = fitted.region_set_posterior()
    fitted.region_sets = None
    assert out["p_count"].shape[:2] == (2, 2)
    after = snapshot(fitted)
    for key in before:
        nptest.assert_array_equal(after[key], before[key], err_msg=key)
