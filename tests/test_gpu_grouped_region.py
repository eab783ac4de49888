"""
The grouped-region model on the MI355X: the grouped table kernel (fcd_lik_grouped_tables) against the NumPy references of
tests/sessions_ref.py and tests/noise_ref.py summed over each group's members, its two degenerate forms bit for bit, the
shapes at which its lane width, lane stride and pair loop change, and GroupedRegionFit with both methods against the
oracle's loops on the summed tables, against SharedRegionFit / UnsharedRegionFit at one label / distinct labels, and
against the exact enumeration of tests/grouped_region_ref.py.

Tolerance rule of the tables: sessions_ref.tolerance(..., scale = members of the largest group), the rule the shared table
is held to at scale = U (rtol 1e-12, atol = 1e-14 max(1, max |sum_k ln N|) per summed item).
"""
import numpy as np
import numpy.testing as nptest
import pytest

import evidence_ref as ER
import exact_law_cases as X
import grouped_region_ref as GR
import noise_ref as NR
import sessions_ref as SR
from conftest import theta_dict
from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain

pytestmark = pytest.mark.gpu

FIT = dict(rtol=1e-10, atol=1e-12)                  # test_gpu_sessions.py's rule for the fits on reference tables
LABELS7 = [2, 0, 1, 0, 2, 2, 0]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.tables, e.CO = torch, fcdiff_amd, _lib, tables, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def C_of(N):
    return N * (N - 1) // 2


def data(env, N, U, K, H=3, seed=None):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U + K if seed is None else seed, sessions=K)
    return m, b, bt


def csr(env, labels):
    (names, offsets, order) = env.pkg.fit.group_labels_csr(list(labels), len(labels))
    return up(env, order), up(env, offsets), len(names)


def group_of(labels):
    names = sorted(set(labels))
    return np.array([names.index(v) for v in labels])


def build(env, m, b, bt, flags=0, count=False, labels=None, noise=None, **kw):
    """(S_B, lM, n_missing or None) of tables.build on host arrays; labels: the grouped call."""
    n = env.torch.zeros(2, dtype=env.torch.int64, device="cuda") if count else None
    if labels is not None:
        kw["groups"] = csr(env, labels)
    if noise is not None:
        kw["noise"] = tuple(None if v is None else up(env, np.asarray(v, dtype=np.float64)) for v in noise)
    (S_B, lM) = env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), flags, n_missing=n, **kw)
    return S_B.cpu().numpy(), lM.cpu().numpy(), (None if n is None else tuple(n.cpu().tolist()))


def summed(lM, labels):
    """(C, G, 3, 3): the reference table summed over each group's members."""
    g = group_of(labels)
    return np.stack([lM[:, g == j].sum(axis=1) for j in range(g.max() + 1)], axis=1)


def largest(labels):
    return int(np.bincount(group_of(labels)).max())


def new_fit(env, model, b, bt, labels=None, cls=None, **kw):
    fit = (cls or env.pkg.fit.GroupedRegionFit)()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (model, b, bt)
    if labels is not None:
        fit.group_labels = list(labels)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


# ------------------------------------------------------------------------------------------------
# 1. the table against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_table_against_reference(env, K):
    (m, b, bt) = data(env, 5, 7, K)
    (S_B, L, _n) = build(env, m, b, bt, labels=LABELS7)
    assert L.shape == (10, 3, 3, 3)
    (S_ref, lM_ref) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    nptest.assert_allclose(L, summed(lM_ref, LABELS7), **SR.tolerance(bt, m.mu, m.sigma, scale=3))
    (S_s, _lM, _n) = build(env, m, b, bt)
    nptest.assert_array_equal(S_B, S_s)                          # the sessions form's S_B, bit for bit
    nptest.assert_allclose(S_B, S_ref, rtol=1e-12)
    if K == 1:                                                    # a 2-D bt is K = 1
        (S_2, L_2, _n) = build(env, m, b, bt[:, :, 0], labels=LABELS7)
        nptest.assert_array_equal(L_2, L)
        nptest.assert_array_equal(S_2, S_B)


@pytest.mark.parametrize("K", [1, 3])
def test_table_with_missing_data(env, K):
    MISS = env.lib.FCD_DATA_NAN_MISSING
    (m, b, bt) = data(env, 5, 7, K)
    rng = np.random.default_rng(K)
    bt[rng.random(bt.shape) < 0.15] = np.nan
    b[rng.random(b.shape) < 0.1] = np.nan
    bt[:, 4, :] = np.nan                                          # a patient with all sessions NaN
    bt[3, 2, :] = np.nan                                          # group 1 = {2}: its every item NaN at edge 3
    bt[5, [1, 3, 6], :] = np.nan                                  # group 0 = {1, 3, 6}: likewise at edge 5
    (S_B, L, n) = build(env, m, b, bt, MISS, count=True, labels=LABELS7)
    (S_ref, lM_ref) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, missing=True)
    nptest.assert_allclose(L, summed(lM_ref, LABELS7), **SR.tolerance(bt, m.mu, m.sigma, missing=True, scale=3))
    for (c, g) in ((3, 1), (5, 0)):
        assert np.all(L[c, g] == 0.0) and not np.signbit(L[c, g]).any()
    assert np.all(np.isfinite(L))
    assert n == (int(np.isnan(b).sum()), int(np.isnan(bt).sum()))
    (S_s, _lM, _n) = build(env, m, b, bt, MISS)
    nptest.assert_array_equal(S_B, S_s)
    fit = new_fit(env, m, b, bt, LABELS7, missing_data=True)
    fit._init_lps(5, 3, 7)
    fit._update_lps()
    assert fit.missing_counts() == n
    nptest.assert_array_equal(fit._lM, L)
    # without the flag a NaN stays in its group's record
    (_S, L_nan, _n) = build(env, m, b, bt, labels=LABELS7)
    bad = summed(np.isnan(bt).any(axis=2)[:, :, None, None] * np.ones((1, 1, 3, 3)), LABELS7) > 0
    assert np.all(np.isnan(L_nan[bad])) and np.all(np.isfinite(L_nan[~bad]))


@pytest.mark.parametrize("K,missing", [(1, False), (3, True), (110, False)])
def test_table_with_noise_variances(env, K, missing):
    """7 K records: 7 and 21 are below tables.NOISE_LDS_RECORDS (records in LDS), 770 is above it (records from global memory)."""
    assert (7 * K > env.tables.NOISE_LDS_RECORDS) == (K == 110)
    (m, b, bt) = data(env, 5, 7, K)
    rng = np.random.default_rng(K)
    (var_b, var_bt) = (rng.random(3) * 0.01, rng.random((7, K)) * 0.02)
    flags = 0
    if missing:
        bt[rng.random(bt.shape) < 0.2] = np.nan
        bt[3, 2, :] = np.nan
        flags = env.lib.FCD_DATA_NAN_MISSING
    (S_B, L, n) = build(env, m, b, bt, flags, count=missing, labels=LABELS7, noise=(var_b, var_bt))
    (S_ref, lM_ref) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, var_b, var_bt, missing)
    nptest.assert_allclose(L, summed(lM_ref, LABELS7), **NR.tolerance(bt, m.mu, m.sigma, var_bt, missing, scale=3))
    nptest.assert_allclose(S_B, S_ref, **NR.tolerance_b(b, m.mu, m.sigma, var_b, missing))
    (S_n, _lM, _n) = build(env, m, b, bt, flags, noise=(var_b, var_bt))
    nptest.assert_array_equal(S_B, S_n)                          # the noise form's S_B, bit for bit
    if missing:
        assert n == (0, int(np.isnan(bt).sum())) and np.all(L[3, 1] == 0.0)
    # one side given: the other is all zeros
    (_S, L_bt, _n) = build(env, m, b, bt, flags, labels=LABELS7, noise=(None, var_bt))
    nptest.assert_array_equal(L_bt, L)


# ------------------------------------------------------------------------------------------------
# 2. the degenerate forms, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("U,K", [(7, 1), (17, 3), (40, 2), (70, 3)])
def test_one_group_and_singletons_are_the_other_two_tables_bit_for_bit(env, U, K, noise):
    MISS = env.lib.FCD_DATA_NAN_MISSING
    (m, b, bt) = data(env, 6, U, K)
    bt[np.random.default_rng(U).random(bt.shape) < 0.1] = np.nan
    rng = np.random.default_rng(U + K)
    kw = {"noise": (rng.random(3) * 0.01, rng.random((U, K)) * 0.02)} if noise else {}
    (S_s, L_s, n_s) = build(env, m, b, bt, MISS, count=True, shared=True, **kw)
    (S_u, lM_u, _n) = build(env, m, b, bt, MISS, **kw)
    (S_1, L_1, n_1) = build(env, m, b, bt, MISS, count=True, labels=["all"] * U, **kw)
    assert L_1.shape == L_s.shape == (15, 1, 3, 3)
    nptest.assert_array_equal(L_1, L_s)
    (S_d, L_d, n_d) = build(env, m, b, bt, MISS, count=True, labels=list(range(U)), **kw)
    assert L_d.shape == lM_u.shape
    assert np.all(L_d == lM_u)                                    # a one-term sum and a butterfly of zeros change nothing
    for S in (S_1, S_d, S_u):
        nptest.assert_array_equal(S, S_s)
    assert n_1 == n_d == n_s == (0, int(np.isnan(bt).sum()))
    (S_2, L_2, _n) = build(env, m, b, bt, MISS, labels=["all"] * U, **kw)
    nptest.assert_array_equal(L_2, L_1)
    nptest.assert_array_equal(S_2, S_1)


# ------------------------------------------------------------------------------------------------
# 3. where the kernel can go wrong
# ------------------------------------------------------------------------------------------------
def check_against_reference(env, N, labels, K, seed=None):
    U = len(labels)
    (m, b, bt) = data(env, N, U, K, seed=seed)
    (S_B, L, _n) = build(env, m, b, bt, labels=labels)
    (_S, lM_ref) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    nptest.assert_allclose(L, summed(lM_ref, labels), **SR.tolerance(bt, m.mu, m.sigma, scale=largest(labels)))
    (S_2, L_2, _n) = build(env, m, b, bt, labels=labels)
    nptest.assert_array_equal(L_2, L)                             # two calls agree bit for bit
    nptest.assert_array_equal(S_2, S_B)
    return m, b, bt, L


@pytest.mark.parametrize("big", [16, 17, 32, 33, 64, 65, 130])
def test_lane_width_switches_and_a_stride_that_wraps(env, big):
    """The largest group on both sides of 16 and 32 members, of 64 and 65 (the 64 lanes wrap once) and of 130 (twice); a
    second group of 3 rides on the same width; 12 pairs: not a multiple of the 16 or 8 lane groups of a block."""
    labels = ["big"] * big + ["small"] * 3
    labels = [labels[i] for i in np.random.default_rng(big).permutation(len(labels))]
    check_against_reference(env, 4, labels, 2)


def test_group_sizes_mixed_in_one_call(env):
    """1, 17 and 65 members under one width (64 lanes: 4 lane groups per block, 30 pairs are not a multiple of them)."""
    labels = ["a"] + ["b"] * 17 + ["c"] * 65
    labels = [labels[i] for i in np.random.default_rng(1).permutation(len(labels))]
    check_against_reference(env, 5, labels, 3)


def test_permuted_labels_against_sorted_ones(env):
    labels = sorted(["a"] * 5 + ["b"] * 20 + ["c"] * 9)
    (m, b, bt, L) = check_against_reference(env, 5, labels, 2, seed=77)
    perm = np.random.default_rng(2).permutation(len(labels))
    (_S, L_p, _n) = build(env, m, b, np.ascontiguousarray(bt[:, perm]), labels=[labels[i] for i in perm])
    # the same members in another order: the two sums differ by their rounding, each within the table's tolerance
    tol = SR.tolerance(bt, m.mu, m.sigma, scale=20)
    nptest.assert_allclose(L_p, L, rtol=2 * tol["rtol"], atol=2 * tol["atol"])


def test_pair_loop_past_the_grid_cap(env):
    """N = 200: 19 900 edges x 4 groups = 79 600 pairs, above 16 lane groups x 16 blocks per CU x 256 CUs = 65 536."""
    check_against_reference(env, 200, [0, 1, 2, 3, 3, 2, 1, 0], 1)


def test_one_patient_one_group(env):
    (m, b, bt, L) = check_against_reference(env, 3, ["only"], 2)
    assert L.shape == (3, 1, 3, 3)


def test_entry_point_refusals(env):
    (m, b, bt) = data(env, 4, 2, 2)
    t = env.torch
    (b_d, bt_d) = (up(env, b), up(env, bt))
    (order, offsets, _G) = csr(env, [0, 1])
    (S_B, L) = (t.empty((6, 3), dtype=t.float64, device="cuda"), t.empty((6, 2, 3, 3), dtype=t.float64, device="cuda"))
    (th, _th) = env.lib.dbl_array(m.theta())
    P = env.lib.dptr
    var = up(env, np.zeros((2, 2)))

    def call(C=6, K=2, G=2, flags=0, order=order, offsets=offsets, var_bt=None, U=2):
        env.ctx.call("fcd_lik_grouped_tables", P(b_d), P(bt_d), C, 3, U, K, th, P(None), P(var_bt), P(order), P(offsets), G,
                     P(S_B), P(L), flags, P(None), env.lib.stream_ptr())
    call()
    call(var_bt=var)
    for kw in (dict(K=0), dict(G=0), dict(G=3), dict(flags=4), dict(order=None), dict(offsets=None)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match="triangular"):
        call(C=5)
    with pytest.raises(NotImplementedError):
        call(K=1 << 31)
    with pytest.raises(NotImplementedError):
        call(U=1 << 16, K=1 << 16, var_bt=var)                    # the record form's 32-bit index limit (refused on the host)


# ------------------------------------------------------------------------------------------------
# 4. the fits on reference tables
# ------------------------------------------------------------------------------------------------
def e2e_data(env):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(5, 4, 7, seed=21, sessions=3)
    return b, bt


def vb_reference(b, bt, labels, theta, iters):
    """sessions_ref.vb_fit's loop at G columns on the tables summed over each group's members (symmetric edge ids)."""
    (C, _H) = b.shape
    N = int(O.C_to_N(C))
    G = len(set(labels))
    th = dict(theta)
    lq_R = np.full((N, G, 2), -np.log(2))
    lq_F = np.full((C, 1, 3), -np.log(3))

    def tables():
        (S_B, lM) = SR.lik_tables(b, bt, th["mu"], th["sigma"], th["eta"], th["epsilon"])
        return S_B, summed(lM, labels)

    def pi2():
        return [1 - th["pi"], th["pi"]]
    (S_B, lM) = tables()
    energy = [O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2())]
    for _ in range(iters):
        lq_F = O.update_lq_F(lq_R, S_B, lM, th["gamma"])
        lq_R = O.update_lq_R(lq_R, lq_F, lM, pi2(), O.EDGE_SYMMETRIC)
        th["pi"] = O.update_pi(lq_R)
        th["gamma"] = O.update_gamma(lq_F)
        (S_B, lM) = tables()
        energy.append(O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2()))
    return dict(energy=np.array(energy), lq_F=lq_F, lq_R=lq_R, theta=th, S_B=S_B, lM=lM)


def test_vb_fit_against_the_oracle_on_reference_tables(env):
    (b, bt) = e2e_data(env)
    model = env.pkg.GroupedRegionModel()
    start = theta_dict(model.theta())
    fit = new_fit(env, model, b, bt, LABELS7, max_iters=4, rel_tol=-np.inf)
    fit.run()
    want = vb_reference(b, bt, LABELS7, start, 4)
    assert len(fit.energy) == 5 and fit.n_sessions == 3 and fit.group_names == [0, 1, 2]
    nptest.assert_allclose(fit.energy, want["energy"], **FIT)
    nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
    nptest.assert_allclose(fit._lq_F, want["lq_F"], **FIT)
    assert fit._lq_R.shape == (5, 3, 2) and fit._lM.shape == (10, 3, 3, 3)
    nptest.assert_allclose(fit._lM, want["lM"], **SR.tolerance(bt, model.mu, model.sigma, scale=3))
    out = fit.region_posterior()
    assert out["group_names"] == [0, 1, 2]
    nptest.assert_allclose(out["p_region"], np.exp(want["lq_R"][:, :, 1]), **FIT)


def test_gibbs_fit_equals_the_oracle_chain_for_chain(env):
    (b, bt) = e2e_data(env)
    model = env.pkg.GroupedRegionModel()
    fit = new_fit(env, model, b, bt, LABELS7, method="gibbs", n_chains=128, n_sweeps=6, burn_in=2, mstep_every=0, seed=77,
                  trace_every=1, connection_marginals=True, anomaly_counts=True, coanomaly=True, group_contrasts=[(0, 2), (2, 1)])
    (gamma, pi2) = (np.array(model.gamma, dtype=np.float64), model.pi2())
    fit.run()
    (S_B, lM) = (fit._d["S_B"].cpu().numpy(), fit._lM)
    (N, G) = (5, 3)
    (_S, lM_ref) = SR.lik_tables(b, bt, model.mu, model.sigma, model.eta, model.epsilon)
    nptest.assert_allclose(lM, summed(lM_ref, LABELS7), **SR.tolerance(bt, model.mu, model.sigma, scale=3))
    (f_o, r_o) = env.CO.gibbs_init(128, N, G, float(pi2[1]), 77, 0)
    for s in range(6):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, np.log(gamma), 77, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, np.log(pi2), 77, s, env.lib.EDGE_MODES["symmetric"], 0)
    (f_g, r_g) = fit.sampler.export_state()
    assert env.ctx.stat("dev_err") == 0
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    # the queries of a sampler fit: the groups are the "patients" of the inherited ones, the connections are per patient
    pc = fit.anomaly_count_posterior()
    assert pc["p_patient_count"].shape == (G, N + 1) and pc["p_region_count"].shape == (N, G + 1)
    co = fit.coanomaly_posterior()
    assert co["p_patient_pair"].shape == (G, G) and co["p_region_pair"].shape == (N, N)
    post = fit.connection_posterior()
    assert post["p_T"].shape == (10, 7) and post["p_F_tilde"].shape == (10, 7, 3)
    assert all(np.all(np.isfinite(v)) for v in post.values())
    assert fit.connection_counts.shape == (10, G, 3, 3)
    gc = fit.group_contrast_posterior()
    assert gc["contrasts"] == [(0, 2), (2, 1)] and gc["p_both"].shape == (2, N) and gc["row_names"] == [str(n) for n in range(N)]
    nptest.assert_allclose(gc["p_both"] + gc["p_only_a"] + gc["p_only_b"] + gc["p_neither"], 1.0, atol=1e-14)
    # the joint's marginals are the chains' frequencies of the two columns over the same sweeps
    p1 = np.exp(fit._lq_R[:, :, 1])
    nptest.assert_allclose(gc["p_a"], p1[:, [0, 2]].T, atol=1e-12)
    nptest.assert_allclose(gc["p_b"], p1[:, [2, 1]].T, atol=1e-12)
    assert fit.patient_groups is None and fit.patient_group_contrasts is None


# ------------------------------------------------------------------------------------------------
# 5. equivalences through the public classes
# ------------------------------------------------------------------------------------------------
def twin_models(env):
    return env.pkg.GroupedRegionModel(), env.pkg.SharedRegionModel(), env.pkg.UnsharedRegionModel()


@pytest.mark.parametrize("distinct", [False, True])
def test_vb_with_sessions_equals_the_other_fits(env, distinct):
    """bt (C, U, K): one label builds the shared sessions table and distinct labels the unshared one bit for bit, so the
    trajectories are those of SharedRegionFit / UnsharedRegionFit('symmetric') exactly."""
    (b, bt) = e2e_data(env)
    (mg, ms, mu) = twin_models(env)
    labels = list(range(7)) if distinct else ["all"] * 7
    kw = dict(max_iters=3, rel_tol=-np.inf)
    fit = new_fit(env, mg, b, bt, labels, **kw)
    other = new_fit(env, mu if distinct else ms, b, bt, edge_index="symmetric",
                    cls=env.pkg.fit.UnsharedRegionFit if distinct else env.pkg.fit.SharedRegionFit, **kw)
    fit.run()
    other.run()
    nptest.assert_array_equal(fit._lM, other._lM)
    nptest.assert_array_equal(fit.energy, other.energy)
    nptest.assert_array_equal(fit._lq_R, other._lq_R)
    nptest.assert_array_equal(fit._lq_F, other._lq_F)
    (a, o) = (fit.connection_posterior(), other.connection_posterior())
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_array_equal(a[key], o[key])


@pytest.mark.parametrize("distinct", [False, True])
def test_vb_with_a_theta_sub_step_equals_the_other_fits(env, distinct):
    """bt (C, U): the 2-D fits build their tables with the tuned 2-D kernels, the grouped fit with the sessions arithmetic at
    K = 1, so the comparison carries the table tolerance (the FIT rule of the fits on reference tables); one theta_sub step
    (L-BFGS-B on objectives that agree to rounding) to 1e-6 on (eta, epsilon)."""
    (N, H, U) = (8, 4, 9)
    (_r, _t, _f, _ft, b, bt) = env.pkg.UnsharedRegionModel().sample_fast(N, H, U, seed=9)
    (mg, ms, mu) = twin_models(env)
    labels = list(range(U)) if distinct else ["all"] * U
    kw = dict(max_iters=1, rel_tol=-np.inf, update_theta_sub=True)
    fit = new_fit(env, mg, b, bt, labels, **kw)
    other = new_fit(env, mu if distinct else ms, b, bt, edge_index="symmetric",
                    cls=env.pkg.fit.UnsharedRegionFit if distinct else env.pkg.fit.SharedRegionFit, **kw)
    fit.run()
    other.run()
    nptest.assert_allclose([fit.model.eta, fit.model.epsilon], [other.model.eta, other.model.epsilon], atol=1e-6)
    nptest.assert_allclose(fit._lq_R, other._lq_R, **FIT)
    nptest.assert_allclose(fit._lq_F, other._lq_F, **FIT)
    nptest.assert_allclose(fit.energy[0], other.energy[0], **FIT)
    nptest.assert_allclose(fit.energy[1], other.energy[1], rtol=1e-6)      # (after the optimiser's step)


@pytest.mark.parametrize("distinct", [False, True])
def test_gibbs_with_a_fixed_seed_equals_the_other_fits(env, distinct):
    (b, bt) = e2e_data(env)
    (mg, ms, mu) = twin_models(env)
    labels = list(range(7)) if distinct else ["all"] * 7
    kw = dict(method="gibbs", n_chains=128, n_sweeps=8, burn_in=2, seed=5, connection_marginals=True, anomaly_counts=True)
    fit = new_fit(env, mg, b, bt, labels, **kw)
    other = new_fit(env, mu if distinct else ms, b, bt,
                    cls=env.pkg.fit.UnsharedRegionFit if distinct else env.pkg.fit.SharedRegionFit, **kw)
    fit.run()
    other.run()
    for (x, y) in zip(fit.sampler.export_state(), other.sampler.export_state()):
        nptest.assert_array_equal(x, y)
    nptest.assert_array_equal(fit._lq_R, other._lq_R)
    nptest.assert_array_equal(fit._lq_F, other._lq_F)
    nptest.assert_array_equal(fit.connection_counts, other.connection_counts)
    assert (fit.model.pi, list(fit.model.gamma)) == (other.model.pi, list(other.model.gamma))
    (a, o) = (fit.connection_posterior(), other.connection_posterior())
    for key in ("p_T", "p_F_tilde", "p_changed"):
        nptest.assert_array_equal(a[key], o[key])


@pytest.mark.parametrize("distinct", [False, True])
def test_gibbs_theta_sub_step_equals_the_other_fits(env, distinct):
    """The Monte-Carlo EM step for (eta, epsilon) at sweep 2 of 3: the chains' (C, G, 3, 3) pair counts gathered to the
    patients against SharedRegionFit's per-edge objective / UnsharedRegionFit's own, on 2-D data (L-BFGS-B to 1e-6)."""
    (N, H, U) = (8, 4, 9)
    (_r, _t, _f, _ft, b, bt) = env.pkg.UnsharedRegionModel().sample_fast(N, H, U, seed=9)
    (mg, ms, mu) = twin_models(env)
    labels = list(range(U)) if distinct else ["all"] * U
    kw = dict(method="gibbs", n_chains=256, n_sweeps=3, burn_in=0, seed=5, update_theta_sub=True, theta_sub_every=2)
    fit = new_fit(env, mg, b, bt, labels, **kw)
    other = new_fit(env, mu if distinct else ms, b, bt,
                    cls=env.pkg.fit.UnsharedRegionFit if distinct else env.pkg.fit.SharedRegionFit, **kw)
    start = (fit.model.eta, fit.model.epsilon)
    fit.run()
    other.run()
    assert (fit.model.eta, fit.model.epsilon) != start
    nptest.assert_allclose([fit.model.eta, fit.model.epsilon], [other.model.eta, other.model.epsilon], atol=1e-6)
    assert fit._lM.shape == other._lM.shape and np.all(np.isfinite(fit._lM))      # rebuilt at the stepped (eta, epsilon)


# ------------------------------------------------------------------------------------------------
# 6. the exact law end to end
# ------------------------------------------------------------------------------------------------
LABELS5 = ["x", "y", "x", "x", "y"]


def broad_model(env):
    src = X.model("broad")
    m = env.pkg.GroupedRegionModel()
    for k in ("pi", "eta", "epsilon"):
        setattr(m, k, getattr(src, k))
    (m.gamma, m.mu, m.sigma) = (np.array(src.gamma), np.array(src.mu), np.array(src.sigma))
    return m


@pytest.fixture(scope="module")
def exact_case(env):
    """N = 3, G = 2, U = 5, H = 3: the data, the enumeration (once for the tests below) and the reference tables."""
    m = broad_model(env)
    (_r, _t, _f, _ft, b, bt) = m.sample(3, 3, LABELS5, seed=4)
    ex = GR.enumerate_posterior(b, bt, LABELS5, m.theta())
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    return dict(b=b, bt=bt, ex=ex, S_B=O.sum_lp_B(lpB), L=summed(lM, LABELS5))


def test_gibbs_posteriors_against_the_enumeration(env, exact_case):
    """The rule of the exact-law tests of the posteriors (test_gpu_patient_groups.py): 2^18 chains, K sweeps with
    ||P_K - pi||_1 < 1e-4 on the exact chain of the summed tables, only the last one counted: within 5 x 0.5/sqrt(G) + 1e-4."""
    (b, bt, ex) = (exact_case["b"], exact_case["bt"], exact_case["ex"])
    m = broad_model(env)
    ec = ExactChain(exact_case["S_B"], exact_case["L"], np.asarray(m.gamma, dtype=np.float64), m.pi2())
    assert abs(ER.logsumexp(ec.L) - ex["log_evidence"]) < 1e-10 * abs(ex["log_evidence"])
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (P, K) = (ec.initial(float(m.pi2()[1])), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    G = X.G_CHAINS
    fit = new_fit(env, m, b, bt, LABELS5, method="gibbs", n_chains=G, n_sweeps=K, burn_in=K - 1, mstep_every=0, seed=11,
                  connection_marginals=True, anomaly_counts=True, group_contrasts=[("x", "y")])
    fit.run()
    assert fit.connection_sweeps == fit.anomaly_count_sweeps == fit.patient_group_sweeps == 1
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    got = {"p_r": fit.region_posterior()["p_region"]}
    pc = fit.anomaly_count_posterior()
    (got["p_group_count"], got["p_region_count"]) = (pc["p_patient_count"], pc["p_region_count"])
    cp = fit.connection_posterior()
    (got["p_T"], got["p_Ft"], got["p_changed"]) = (cp["p_T"], cp["p_F_tilde"], cp["p_changed"])
    worst = 0.0
    for (key, val) in got.items():
        assert val.shape == ex[key].shape, key
        worst = max(worst, float(np.abs(val - ex[key]).max()))
        nptest.assert_allclose(val, ex[key], rtol=0, atol=tol, err_msg=key)
    gc = fit.group_contrast_posterior()
    assert gc["contrasts"] == [("x", "y")]
    joint = ex["p_pair"][0, 1]                                   # (N, 2, 2): [r_nx, r_ny]
    for (key, want) in (("p_both", joint[:, 1, 1]), ("p_only_a", joint[:, 1, 0]), ("p_only_b", joint[:, 0, 1]),
                        ("p_neither", joint[:, 0, 0])):
        worst = max(worst, float(np.abs(gc[key][0] - want).max()))
        nptest.assert_allclose(gc[key][0], want, rtol=0, atol=tol, err_msg=key)
    print("K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (K, worst, tol))
    # independent=True on a sampler fit: the product of its marginals
    ind = fit.group_contrast_posterior(independent=True)
    nptest.assert_allclose(ind["p_both"], ind["p_a"] * ind["p_b"], rtol=1e-12)
    nptest.assert_allclose(ind["p_a"], gc["p_a"], atol=1e-12)


def test_vb_contrasts_are_products_and_log_evidence_against_the_enumeration(env, exact_case):
    (b, bt, ex) = (exact_case["b"], exact_case["bt"], exact_case["ex"])
    m = broad_model(env)
    fit = new_fit(env, m, b, bt, LABELS5, max_iters=2, n_chains=64, group_contrasts=[("x", "y"), ("y", "x")],
                  region_sets={"pair": [0, 2]})
    fit.run()
    gc = fit.group_contrast_posterior()
    q1 = np.exp(fit._lq_R[:, :, 1])
    rows = np.concatenate([q1, 1.0 - np.prod(1.0 - q1[[0, 2]], axis=0, keepdims=True)], axis=0)      # (R, G)
    assert gc["row_names"] == ["0", "1", "2", "set:pair"] and gc["contrasts"] == [("x", "y"), ("y", "x")]
    nptest.assert_allclose(gc["p_a"], rows[:, [0, 1]].T, rtol=1e-12)
    nptest.assert_allclose(gc["p_b"], rows[:, [1, 0]].T, rtol=1e-12)
    nptest.assert_allclose(gc["p_both"], gc["p_a"] * gc["p_b"], rtol=1e-12)
    nptest.assert_allclose(gc["p_only_a"], gc["p_a"] * (1 - gc["p_b"]), rtol=1e-12)
    nptest.assert_allclose(gc["p_only_b"], (1 - gc["p_a"]) * gc["p_b"], rtol=1e-12)
    nptest.assert_allclose(gc["p_neither"], (1 - gc["p_a"]) * (1 - gc["p_b"]), rtol=1e-12)
    # the evidence at the generating parameters, under test_log_evidence_against_the_enumeration's rule
    src = broad_model(env)
    for k in ("pi", "eta", "epsilon"):
        setattr(m, k, getattr(src, k))
    m.gamma = np.array(src.gamma)
    out = fit.log_evidence(n_anneal=50, n_chains=4096, seed=1282)
    print("exact %.4f estimate %.4f se %.4f ess %.0f lower %.4f (%.4f)" % (
        ex["log_evidence"], out["log_evidence"], out["log_evidence_se"], out["ess"], out["lower"], out["lower_se"]))
    assert out["n_chains"] == 4096 and out["n_anneal"] == 50
    assert abs(out["log_evidence"] - ex["log_evidence"]) <= 5.0 * out["log_evidence_se"]
    assert out["lower"] - 5.0 * out["lower_se"] <= ex["log_evidence"]


# ------------------------------------------------------------------------------------------------
# 7. invariants
# ------------------------------------------------------------------------------------------------
def snapshot(fit):
    (f, r) = (fit.sampler.export_state() if fit.sampler is not None else (None, None))
    return {"theta": np.asarray(fit.model.theta()).tobytes(), "lq_R": fit._lq_R.tobytes(), "lq_F": fit._lq_F.tobytes(),
            "energy": np.asarray(fit.energy).tobytes(), "lM": fit._lM.tobytes(),
            "S_B": fit._d["S_B"].cpu().numpy().tobytes(), "f": None if f is None else f.tobytes(),
            "r": None if r is None else r.tobytes(), "groups": (fit.patient_groups, fit.patient_group_contrasts)}


@pytest.mark.parametrize("method", ["vb", "gibbs"])
def test_a_fit_is_left_unchanged_by_the_queries(env, method):
    (b, bt) = e2e_data(env)
    fit = new_fit(env, env.pkg.GroupedRegionModel(), b, bt, LABELS7, method=method, max_iters=2, n_chains=128, n_sweeps=6,
                  burn_in=2, seed=3, connection_marginals=True, anomaly_counts=True, coanomaly=True, region_sets=[[0, 1], [2, 3, 4]],
                  group_contrasts=[(0, 1)], missing_data=True)
    fit.run()
    before = snapshot(fit)
    fit.region_posterior()
    fit.connection_posterior()
    fit.anomaly_count_posterior()
    fit.coanomaly_posterior()
    rs = fit.region_set_posterior()
    assert rs["p_any"].shape == (2, 3)                               # per set and GROUP
    gc = fit.group_contrast_posterior()
    assert gc["p_both"].shape == (1, 7) and gc["row_names"][5:] == ["set:0", "set:1"]
    fit.group_contrast_posterior(independent=True)
    fit.log_evidence(n_anneal=5, n_chains=64)
    assert fit.missing_counts() == (0, 0)
    assert snapshot(fit) == before


def test_refusals(env):
    (b, bt) = e2e_data(env)

    def fit_with(**kw):
        return new_fit(env, env.pkg.GroupedRegionModel(), b, bt, LABELS7, max_iters=1, **kw)
    for kw in (dict(group_contrasts=[(0, 3)]), dict(group_contrasts=[(0, 1), (0, 1)]), dict(group_contrasts=[(1, 1)]),
               dict(group_contrasts=[(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)] * 11),
               dict(patient_groups=[[0], [1]]), dict(patient_traits=[np.arange(3.0)]), dict(edge_index="reference")):
        with pytest.raises(ValueError):
            fit_with(**kw).run()
    fit = fit_with()
    fit.run()
    with pytest.raises(NotImplementedError, match="separate question"):
        fit.score(bt)
    with pytest.raises(NotImplementedError, match="separate question"):
        fit.membership(bt[:, :, 0])
    with pytest.raises(ValueError, match="group_contrasts"):
        fit.group_contrast_posterior()
    fit.method = "gibbs"
    fit.group_contrasts = [(0, 1)]
    with pytest.raises(ValueError):
        fit.group_contrast_posterior()                               # no sampler run counted them
