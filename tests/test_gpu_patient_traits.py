"""
Patient traits on the MI355X: fcd_gibbs_patient_trait_tally / fcd_gibbs_set_patient_trait_accumulator against the NumPy
restatement of tests/patient_traits_ref.py, the patient-group joint histogram of a binary trait's two groups, the sampler's
own chains recounted sweep by sweep, the exact posterior of small models, and patient_trait_posterior() of a fit end to end.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
import patient_traits_ref as PT
from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd import gibbs
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.gibbs, e.GibbsEngine, e.CO = torch, fcdiff_amd, _lib, gibbs, gibbs.GibbsEngine, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def tables(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def import_r_bits(env, r):
    """Pack r (G, Nreg, U) with fcd_gibbs_import_state (f all zero) into an r_bits tensor; no tables needed."""
    t = env.torch
    (G, N, U) = r.shape
    Cn = N * (N - 1) // 2
    GW = (G + 63) // 64
    f_state = t.zeros((GW, Cn, 64), dtype=t.uint8, device="cuda")
    r_bits = t.zeros((GW, N, U), dtype=t.int64, device="cuda")
    f = t.zeros((G, Cn), dtype=t.uint8, device="cuda")
    env.ctx.call("fcd_gibbs_import_state", env.lib.dptr(f), env.lib.dptr(up(env, r.astype(np.uint8))), N, U, G,
                 env.lib.dptr(f_state), env.lib.dptr(r_bits), env.lib.stream_ptr())
    if G % 64:                                       # the bits of the chains beyond G: set on purpose, never to be counted
        r_bits[G // 64] |= ~((1 << (G % 64)) - 1)
    return r_bits


def i32p(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.c_void_p)


def u8p(a):
    return np.ascontiguousarray(a, dtype=np.uint8).ctypes.data_as(C.c_void_p)


def send_sets(env, sets, N):
    env.ctx.region_sets_owner = None                 # (no engine's)
    if sets is None:
        env.ctx.call("fcd_region_sets_set", None, None, 0)
        return 0
    (_names, offsets, members) = env.gibbs.region_sets_csr(sets, N)
    env.ctx.call("fcd_region_sets_set", i32p(offsets), i32p(members), len(offsets) - 1)
    return len(offsets) - 1


def send_traits(env, traits, U, with_sets):
    """The traits to the context, straight through the C entry; (Q, Umax, n_known)."""
    (names, scores, known, n_known) = env.gibbs.patient_traits_scores(traits, U)
    env.ctx.patient_traits_owner = None
    env.ctx.call("fcd_patient_traits_set", i32p(scores), u8p(known), len(names), U, 1 if with_sets else 0)
    return len(names), int(n_known.max()), n_known


def tally(env, r_bits, N, U, G, Q, rows, umax, times=1):
    hist = env.torch.zeros((Q, rows, umax + 1 + PT.NB + 3), dtype=env.torch.int32, device="cuda")
    total = env.torch.zeros((Q, rows, umax + 1), dtype=env.torch.int64, device="cuda")
    for _ in range(times):
        env.ctx.call("fcd_gibbs_patient_trait_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hist), env.lib.dptr(total),
                     env.lib.stream_ptr())
    return hist.cpu().numpy().view(np.uint32).astype(np.int64), total.cpu().numpy()


def single_state_case(G, N, U):
    """
    The traits: one continuous, one with ties (three values), one binary, one that is not known for patients on both sides of
    patients 63 / 64 (where U allows; else for the middle patient), one known for exactly two patients (the first and the last).
    """
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    tied = rng.integers(0, 3, U).astype(np.float64)
    tied[:2] = (0.0, 2.0)
    binary = (np.arange(U) % 3 == 0).astype(np.float64)
    gaps = rng.normal(size=U)
    gaps[[61, 63, 64, 66] if U > 66 else [U // 2]] = NAN
    two = np.full(U, NAN)
    two[[0, U - 1]] = (4.0, -1.0)
    traits = [rng.normal(size=U), tied, binary, gaps, two]
    sets = [[N - 1], list(range(N)), [0, N - 1]]
    return r, traits, sets


@pytest.mark.parametrize("with_sets", [False, True], ids=["regions", "regions+sets"])
@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (64, 3, 3), (1, 2, 512), (130, 40, 5)])
def test_patient_trait_tally_single_state(env, G, N, U, with_sets):
    """fcd_gibbs_patient_trait_tally on an imported state: both NumPy buffers, integer for integer; a second run adds."""
    (r, traits, sets) = single_state_case(G, N, U)
    sets = sets if with_sets else None
    rows = N + send_sets(env, sets, N)
    (Q, umax, n_known) = send_traits(env, traits, U, with_sets)
    assert Q == 5 and umax == U and n_known[4] == 2
    r_bits = import_r_bits(env, r)
    (want_h, want_s) = PT.tally(r, traits, sets)
    assert want_h.shape == (Q, rows, umax + 1 + PT.NB + 3) and want_s.shape == (Q, rows, umax + 1)
    for times in (1, 2):
        (hist, total) = tally(env, r_bits, N, U, G, Q, rows, umax, times=times)
        nptest.assert_array_equal(hist, times * want_h)
        nptest.assert_array_equal(total, times * want_s)
    assert np.all(hist[:, :, :umax + 1].sum(axis=2) == 2 * G)
    nptest.assert_array_equal(hist[:, :, umax + 1:umax + 1 + PT.NB].sum(axis=2), hist[:, :, umax + 1 + PT.NB:].sum(axis=2))
    env.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)
    send_sets(env, None, N)


def test_patient_trait_tally_where_both_grids_wrap(env):
    """Both kernels walk grid-stride loops under a cap of 8 workgroups per CU (2048 on 256 CUs): 130 rows x 52 chain words
    = 6760 pairs in phase 1, 16 traits x 130 rows = 2080 rows in phase 2, so every workgroup takes a second pair or row."""
    (G, N, U, Q) = (3300, 130, 5, 16)
    rng = np.random.default_rng(G + N)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    traits = [rng.normal(size=U) for _ in range(Q)]
    for q in range(8, Q):
        traits[q][q % U] = NAN
    assert N * ((G + 63) // 64) > 2048 and Q * N > 2048
    send_sets(env, None, N)
    (Q_sent, umax, _n) = send_traits(env, traits, U, False)
    (hist, total) = tally(env, import_r_bits(env, r), N, U, G, Q_sent, N, umax)
    (want_h, want_s) = PT.tally(r, traits)
    nptest.assert_array_equal(hist, want_h)
    nptest.assert_array_equal(total, want_s)
    env.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)


def test_binary_trait_signs_are_the_patient_group_contrast(env):
    """
    In one state: the three sign counters of a binary trait equal the sums of the patient-group joint histogram of the
    contrast (ones, zeros) over k_a/|a| <, =, > k_b/|b|, the states with k = 0 or k = n left out on both sides.  Two patients
    the trait is not known for belong to neither group.
    """
    (G, N, U) = (200, 9, 70)
    rng = np.random.default_rng(17)
    r = (rng.random((G, N, U)) < rng.uniform(0.02, 0.98, (1, N, 1))).astype(np.uint8)
    y = (rng.random(U) < 0.35).astype(np.float64)
    y[[3, 64]] = NAN
    ones = np.flatnonzero(y == 1.0).tolist()
    zeros = np.flatnonzero(y == 0.0).tolist()
    (n1, n0) = (len(ones), len(zeros))
    sets = [[0, 1], [N - 1]]
    rows = N + send_sets(env, sets, N)
    r_bits = import_r_bits(env, r)
    (Q, umax, _n) = send_traits(env, [y], U, True)
    (hist, _total) = tally(env, r_bits, N, U, G, Q, rows, umax)
    signs = hist[0, :, umax + 1 + PT.NB:]
    (_names, offsets, members) = env.gibbs.patient_groups_csr([ones, zeros], U)
    env.ctx.patient_groups_owner = None
    env.ctx.call("fcd_patient_groups_set", i32p(offsets), i32p(members), 2, i32p([0, 1]), 1, 1)
    hg = env.torch.zeros((2, rows, max(n1, n0) + 1), dtype=env.torch.int32, device="cuda")
    hj = env.torch.zeros(rows * (n1 + 1) * (n0 + 1), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_patient_group_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hg), env.lib.dptr(hj),
                 env.lib.stream_ptr())
    joint = hj.cpu().numpy().astype(np.int64).reshape(rows, n1 + 1, n0 + 1)
    (ka, kb) = np.meshgrid(np.arange(n1 + 1), np.arange(n0 + 1), indexing="ij")
    inside = (ka + kb > 0) & (ka + kb < n1 + n0)
    rate = ka * n0 - kb * n1                         # the sign of k_a/|a| - k_b/|b|, and A itself
    for (column, pick) in enumerate((rate < 0, rate == 0, rate > 0)):
        nptest.assert_array_equal(signs[:, column], joint[:, pick & inside].sum(axis=1))
    assert signs.sum() > G * rows // 2 and np.all(signs.sum(axis=0) > 0)
    env.ctx.call("fcd_patient_groups_set", None, None, 0, None, 0, 0)
    env.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)
    send_sets(env, None, N)


def small_traits():
    rng = np.random.default_rng(12)
    dose = rng.integers(0, 4, 70).astype(np.float64)
    onset = rng.normal(size=70)
    onset[[2, 62, 63, 64, 69]] = NAN
    return {"severity": rng.normal(size=70), "dose": dose, "medicated": (np.arange(70) % 2).astype(np.float64), "onset": onset}


TRAITS = small_traits()
SETS = {"front": [0, 1, 2], "hub": [7], "whole": list(range(12))}
GROUPS = {"low": list(range(0, 30)), "high": list(range(30, 70))}


@pytest.fixture(scope="module")
def small(env):
    (m, S_B, lM) = tables(env, 12, 4, 70, seed=21)
    return m, up(env, S_B), up(env, lM)


def small_engine(env, small, seed=77, G=130):
    (m, S_B_d, lM_d) = small
    e = env.GibbsEngine(S_B_d, lM_d, 12, 70, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    e.set_hyper(m.gamma, m.pi2())
    e.init(0.2)
    return e


@pytest.fixture(scope="module")
def stepped(env, small):
    """One engine stepped sweep by sweep: the state r after every sweep (computed once, shared, never changed)."""
    e = small_engine(env, small)
    states = []
    for s in range(9):
        e.run(s, 1, mstep_every=0, accumulate_from=None)
        states.append(e.export_state()[1])
    return states


@pytest.fixture(scope="module")
def recounts(stepped):
    """The reference's buffers of every stepped state, without and with the sets as rows (computed once, shared)."""
    trait_list = list(TRAITS.values())
    return {with_sets: [PT.tally(s, trait_list, list(SETS.values()) if with_sets else None) for s in stepped]
            for with_sets in (False, True)}


@pytest.mark.parametrize("with_sets", [False, True], ids=["regions", "regions+sets"])
def test_accumulator_inside_run_is_exact(env, small, stepped, recounts, with_sets):
    """Nine sweeps in two calls with the accumulator from sweep 2, every 1 and 3: bit for bit the NumPy recount of a second
    engine's states; the sweep counter; the one-shot tally of the end state is the last sweep's share."""
    (K, s0) = (9, 2)
    for every in (1, 3):
        e = small_engine(env, small)
        if with_sets:
            e.set_region_sets(SETS)
        e.set_patient_traits(TRAITS)
        e.attach_patient_trait_accumulator(every)
        e.run(0, 4, mstep_every=0, accumulate_from=s0)               # in two calls: the counters carry over
        e.run(4, K - 4, mstep_every=0, accumulate_from=s0)
        nptest.assert_array_equal(e.export_state()[1], stepped[K - 1])
        counted = list(range(s0, K, every))
        assert e.patient_trait_sweeps == len(counted)
        (hist, total) = e.patient_trait_host()
        rows = 12 + (3 if with_sets else 0)
        assert hist.shape == (4, rows, 71 + PT.NB + 3) and hist.dtype == np.uint32
        assert total.shape == (4, rows, 71) and total.dtype == np.int64
        nptest.assert_array_equal(hist.astype(np.int64), sum(recounts[with_sets][s][0] for s in counted))
        nptest.assert_array_equal(total, sum(recounts[with_sets][s][1] for s in counted))
        assert e.patient_trait_row_names()[-1] == ("set:whole" if with_sets else "11")
        (one_h, one_s) = e.patient_trait_tally(env.torch.zeros_like(e.patient_trait_acc[0]), env.torch.zeros_like(e.patient_trait_acc[1]))
        last = recounts[with_sets][K - 1]
        nptest.assert_array_equal(one_h.cpu().numpy().view(np.uint32).astype(np.int64), last[0])
        nptest.assert_array_equal(one_s.cpu().numpy(), last[1])
        assert np.abs(total).max() > 0 and hist[:, :, 71:71 + PT.NB].sum() > 0           # (defined states occur)


def test_with_the_other_five_accumulators(env, small):
    """The new buffers alone or with the other five: equal; the other five and the chains with or without the new one: equal."""
    (K, s0) = (9, 2)
    periods = {"pair": 2, "count": 1, "coanomaly": 4, "region_set": 3, "patient_group": 2}

    def run(with_traits, with_five):
        e = small_engine(env, small)
        e.set_region_sets(SETS)
        if with_five:
            e.attach_pair_accumulator(periods["pair"])
            e.attach_count_accumulator(periods["count"])
            e.attach_coanomaly_accumulator(periods["coanomaly"])
            e.attach_region_set_accumulator(periods["region_set"])
            e.set_patient_groups(GROUPS, [("low", "high")])
            e.attach_patient_group_accumulator(periods["patient_group"])
        if with_traits:
            e.set_patient_traits(TRAITS)
            e.attach_patient_trait_accumulator(2)
        e.run(0, K, mstep_every=1, accumulate_from=s0)
        return e
    (alone, both, five) = (run(True, False), run(True, True), run(False, True))
    for (a, b) in zip(alone.patient_trait_host(), both.patient_trait_host()):
        nptest.assert_array_equal(a, b)
    assert alone.patient_trait_sweeps == both.patient_trait_sweeps == env.gibbs.pair_sweeps_in(0, K, s0, 2) == 4
    assert alone.patient_trait_host()[0][:, :, :71].sum() == 4 * 15 * 4 * 130
    nptest.assert_array_equal(both.pair_counts_host(), five.pair_counts_host())
    for (a, b) in zip(both.count_hist_host() + both.coanomaly_host() + both.region_set_host() + both.patient_group_host(),
                      five.count_hist_host() + five.coanomaly_host() + five.region_set_host() + five.patient_group_host()):
        nptest.assert_array_equal(a, b)
    for key in periods:
        assert getattr(both, key + "_sweeps") == getattr(five, key + "_sweeps") == env.gibbs.pair_sweeps_in(0, K, s0, periods[key])
    nptest.assert_array_equal(both.export_state()[1], five.export_state()[1])
    nptest.assert_array_equal(both.export_state()[0], five.export_state()[0])
    nptest.assert_array_equal(alone.export_state()[1], five.export_state()[1])


@pytest.mark.parametrize("N,U,y", [(3, 3, (1.0, 2.0, 3.0)), (3, 4, (1.0, 5.0, 5.0, 9.0))], ids=["3x3", "3x4-tied"])
def test_gibbs_trait_statistics_against_exact(env, N, U, y):
    """
    2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: the k histogram, the sign counters, the AUC
    bins and the unnormalised sum over the defined states of AUC / G, each within 5 x 0.5/sqrt(G) + 1e-4 of the enumerated
    posterior (every one is the mean over chains of a quantity in [0, 1]).
    """
    m = X.model("broad")
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    (S_B, gamma, pi2, seed) = (O.sum_lp_B(lpB), np.asarray(m.gamma, dtype=np.float64), m.pi2(), 1234 + 10 * N + U)
    ec = ExactChain(S_B, lM, gamma, pi2)
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (_f, r) = ec.all_states()                        # (S, N, U)
    (a, kn) = PT.scores(y)
    (k, A) = PT.k_and_A(r, a, kn)                    # (S, N)
    want_k = np.zeros((N, U + 1))
    want_bins = np.zeros((N, PT.NB))
    want_signs = np.zeros((N, 3))
    want_auc = np.zeros(N)
    for n in range(N):
        np.add.at(want_k[n], k[:, n], pi)
        ok = (k[:, n] > 0) & (k[:, n] < U)
        d = k[ok, n] * (U - k[ok, n])
        np.add.at(want_bins[n], np.minimum(PT.NB - 1, (PT.NB * (A[ok, n] + d)) // (2 * d)), pi[ok])
        np.add.at(want_signs[n], np.sign(A[ok, n]) + 1, pi[ok])
        want_auc[n] = (pi[ok] * (0.5 + A[ok, n] / (2.0 * d))).sum()
    assert want_signs.min() > 0.1 and 0.5 < want_signs.sum(axis=1).min() and want_signs.sum(axis=1).max() < 0.75
    (P, K) = (ec.initial(X.PI0), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    G = X.G_CHAINS
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    eng.set_patient_traits([list(y)])
    eng.attach_patient_trait_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.patient_trait_sweeps == 1
    (hist, total) = eng.patient_trait_host()
    hist = hist.astype(np.int64)
    got_k = hist[0, :, :U + 1] / float(G)
    got_bins = hist[0, :, U + 1:U + 1 + PT.NB] / float(G)
    got_signs = hist[0, :, U + 1 + PT.NB:] / float(G)
    kk = np.arange(1, U)
    got_auc = 0.5 * got_signs.sum(axis=1) + (total[0, :, 1:U] / (2.0 * kk * (U - kk))).sum(axis=1) / float(G)
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%dx%d: K = %d sweeps, worst deviations k %.2e signs %.2e bins %.2e auc %.2e (tolerance %.2e)" % (
        N, U, K, np.abs(got_k - want_k).max(), np.abs(got_signs - want_signs).max(), np.abs(got_bins - want_bins).max(),
        np.abs(got_auc - want_auc).max(), tol))
    nptest.assert_allclose(got_k, want_k, rtol=0, atol=tol)
    nptest.assert_allclose(got_signs, want_signs, rtol=0, atol=tol)
    nptest.assert_allclose(got_bins, want_bins, rtol=0, atol=tol)
    nptest.assert_allclose(got_auc, want_auc, rtol=0, atol=tol)


def test_fit_gibbs_patient_traits(env):
    """
    The fit end to end: 12 regions x 70 patients, 128 chains, region sets given; patient_trait_posterior() equals the
    reference summaries of the engine's pooled buffers.  One qualitative fact: the trait "tied" is 2 x (the patient's TRUE
    anomaly of region 11, which 6 of the 70 patients have) + standard normal noise, so the patients the sampler finds
    anomalous at region 11 have the higher trait; region 0 (one truly anomalous patient) is not tied to it.  With the (pi,
    gamma) step off the fit's chains are oracle/c_oracle's (gibbs_init at the model's pi, 12 sweeps, seed 5, the states of
    sweeps 3 .. 11 counted): run on the CPU, they give p_greater = 1.000 at region 11 (auc_mean 0.846) and 0.236 at region 0
    (auc_mean 0.434), and for the binary trait "carrier" (the true anomaly itself) auc_mean = 0.948 at region 11.  The
    thresholds 0.9 and 0.5 on p_greater leave margins of 0.1 and 0.26, the threshold 0.85 on that auc_mean one of 0.1.
    """
    (N, H, U) = (12, 6, 70)
    gen = env.pkg.UnsharedRegionModel()
    (r_true, _t, _f, _ft, b, bt) = gen.sample_fast(N, H, U, seed=8)
    assert r_true[11].sum() == 6 and r_true[0].sum() == 1
    tied = r_true[11].astype(np.float64) * 2.0 + np.random.default_rng(3).normal(size=U)
    tied[[5, 64]] = NAN
    traits = {"tied": tied, "carrier": r_true[11].astype(np.float64)}
    sets = {"front": [0, 1, 2], "tail": [9, 10, 11]}

    def gibbs_fit(**kw):
        fit = env.pkg.fit.UnsharedRegionFit()
        fit._ctx = env.ctx
        fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
        fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed, fit.mstep_every = "gibbs", 128, 12, 3, 5, 0
        for (k, v) in kw.items():
            setattr(fit, k, v)
        fit.run()
        return fit
    off = gibbs_fit()
    assert off.patient_trait_hist is None and off.sampler.patient_trait_acc is None
    with pytest.raises(ValueError, match="set patient_traits before run"):
        off.patient_trait_posterior()
    on = gibbs_fit(patient_traits=traits, region_sets=sets)
    nptest.assert_array_equal(on.sampler.export_state()[1], off.sampler.export_state()[1])
    nptest.assert_array_equal(on._lq_R, off._lq_R)
    n_acc = 9                                        # sweeps 3 .. 11
    assert on.patient_trait_sweeps == n_acc and on.patient_trait_names == ["tied", "carrier"]
    assert on.patient_trait_n_known.tolist() == [68, 70]
    (hist, total) = (on.patient_trait_hist, on.patient_trait_sum)
    (eh, es) = on.sampler.patient_trait_host()       # one rank: the pooled buffers are the engine's
    nptest.assert_array_equal(hist, eh.astype(np.int64))
    nptest.assert_array_equal(total, es)
    assert hist.shape == (2, 14, 71 + PT.NB + 3) and hist.dtype == np.int64 and total.shape == (2, 14, 71) and total.dtype == np.int64
    assert np.all(hist[:, :, :71].sum(axis=2) == 128 * n_acc) and not hist[0, :, 69:71].any()
    out = on.patient_trait_posterior()
    assert out["names"] == ["tied", "carrier"] and out["n_known"].tolist() == [68, 70] and out["sweeps"] == n_acc
    assert out["rows"] == [str(n) for n in range(N)] + ["set:front", "set:tail"]
    want = PT.summaries(hist, total, [68, 70], 0.95)
    for key in ("p_count", "p_defined", "p_greater", "p_less", "p_equal", "auc_mean", "auc_hist"):
        nptest.assert_allclose(out[key], want[key], rtol=1e-13, atol=1e-15, err_msg=key)
    nptest.assert_array_equal(out["auc_interval"], want["auc_interval"])
    print("p_greater of 'tied': region 11 %.4f (auc_mean %.4f), region 0 %.4f (auc_mean %.4f)" % (
        out["p_greater"][0, 11], out["auc_mean"][0, 11], out["p_greater"][0, 0], out["auc_mean"][0, 0]))
    assert out["p_greater"][0, 11] > 0.9 and out["p_greater"][0, 0] < 0.5
    assert out["auc_mean"][1, 11] > 0.85             # the carriers themselves
    narrow = on.patient_trait_posterior(level=0.5)["auc_interval"]
    ok = ~np.isnan(narrow[:, :, 0])
    assert np.all(out["auc_interval"][:, :, 0][ok] <= narrow[:, :, 0][ok]) and np.all(narrow[:, :, 1][ok] <= out["auc_interval"][:, :, 1][ok])
    early = gibbs_fit(patient_traits=traits, n_sweeps=3)
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        early.patient_trait_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(patient_traits={"flat": np.ones(U)})


def test_refusals_through_the_c_abi(env):
    """The checks that come before any device work, on a live context; the device pointers are never dereferenced."""
    (lib, ctx, E) = (env.lib.load(), env.ctx.handle, env.lib)
    fake = C.c_void_p(16)
    (env.ctx.region_sets_owner, env.ctx.patient_traits_owner) = (None, None)
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_patient_traits_set(ctx, None, None, 0, 0, 0) == 0                                        # clears
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 4, 4, 64, fake, fake, None) == E.FCD_ERR_ARG        # no traits
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 4, 4, 1) == E.FCD_ERR_ARG
    good = (i32p([[-3, -1, 1, 3]]), u8p([[1, 1, 1, 1]]))
    assert lib.fcd_patient_traits_set(ctx, None, good[1], 1, 4, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_traits_set(ctx, good[0], None, 1, 4, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_traits_set(ctx, good[0], good[1], 0, 4, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_traits_set(ctx, good[0], good[1], 1, 0, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_traits_set(ctx, i32p(np.zeros((17, 4))), u8p(np.ones((17, 4))), 17, 4, 0) == E.FCD_ERR_UNSUPPORTED
    assert b"at most 16 traits" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p(np.zeros((1, 513))), u8p(np.ones((1, 513))), 1, 513, 0) == E.FCD_ERR_UNSUPPORTED
    assert b"at most 512 patients" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p([[0, 0, 0, 0]]), u8p([[0, 1, 0, 0]]), 1, 4, 0) == E.FCD_ERR_ARG          # n_q = 1
    assert b"at least 2" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p([[0, 0, 0, 0]]), u8p([[1, 1, 1, 0]]), 1, 4, 0) == E.FCD_ERR_ARG          # all equal
    assert b"one score" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p([[-3, 0, 0, 3]]), u8p([[1, 1, 1, 0]]), 1, 4, 0) == E.FCD_ERR_ARG         # |score| > n_q - 1
    assert b"beyond n_q - 1 = 2" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p([[-3, -1, 1, 2]]), u8p([[1, 1, 1, 1]]), 1, 4, 0) == E.FCD_ERR_ARG        # sum != 0
    assert b"sum to -1" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, i32p([[-2, 0, 1, 1]]), u8p([[1, 1, 1, 0]]), 1, 4, 0) == E.FCD_ERR_ARG         # a score where not known
    assert b"not known" in lib.fcd_last_message(ctx)
    # one good trait of 4 patients: the shape checks of the tally and of the accumulator
    assert lib.fcd_patient_traits_set(ctx, good[0], good[1], 1, 4, 0) == 0
    assert lib.fcd_gibbs_patient_trait_tally(ctx, None, 6, 4, 64, fake, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 4, 64, fake, None, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 4, 64, None, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 4, 0, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 3, 64, fake, fake, None) == E.FCD_ERR_SHAPE      # traits of 4 patients
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 5, 64, fake, fake, None) == E.FCD_ERR_SHAPE
    assert b"set for 4 patients" in lib.fcd_last_message(ctx)
    # scratch: 1 trait x 40000 rows x 2^20 chains x 6 bytes > 1 GiB
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 40000, 4, 1 << 20, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    assert b"1 GiB" in lib.fcd_last_message(ctx)
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, None, 6, 4, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, None, fake, 6, 4, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 1, 4, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 0, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 3, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 4, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 4, 1) == 0
    assert lib.fcd_patient_traits_set(ctx, good[0], good[1], 1, 4, 0) == E.FCD_ERR_ARG                      # attached
    assert b"is attached" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_traits_set(ctx, None, None, 0, 0, 0) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32p([0, 1]), i32p([0]), 1) == 0                                    # no set rows: free to change
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, None, None, 0, 0, 1) == 0
    # the same trait with the region sets {0, 5}, {2} as rows
    assert lib.fcd_patient_traits_set(ctx, good[0], good[1], 1, 4, 1) == 0
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 6, 4, 64, fake, fake, None) == E.FCD_ERR_ARG        # ... and there are none
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 4, 1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32p([0, 2, 3]), i32p([0, 5, 2]), 2) == 0
    assert lib.fcd_gibbs_patient_trait_tally(ctx, fake, 5, 4, 64, fake, fake, None) == E.FCD_ERR_SHAPE      # member 5 of 5 regions
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 5, 4, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, fake, fake, 6, 4, 1) == 0
    assert lib.fcd_region_sets_set(ctx, i32p([0, 1]), i32p([0]), 1) == E.FCD_ERR_ARG                        # the sets are rows
    assert b"patient-trait accumulator" in lib.fcd_last_message(ctx)
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_trait_accumulator(ctx, None, None, 0, 0, 1) == 0
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_patient_traits_set(ctx, None, None, 0, 0, 0) == 0
    # the context is still usable: a real tally of a small state
    r = (np.random.default_rng(2).random((70, 3, 4)) < 0.5).astype(np.uint8)
    (Q, umax, _n) = send_traits(env, [[1.0, 2.0, 2.0, 3.0]], 4, False)
    (hist, total) = tally(env, import_r_bits(env, r), 3, 4, 70, Q, 3, umax)
    (want_h, want_s) = PT.tally(r, [[1.0, 2.0, 2.0, 3.0]])
    nptest.assert_array_equal(hist, want_h)
    nptest.assert_array_equal(total, want_s)
    env.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)


def test_run_refuses_another_shape_while_attached(env):
    (N, U, G) = (12, 5, 64)
    (m, S_B, lM) = tables(env, N, 3, U, seed=3)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    send_sets(env, None, N)
    (Q, umax, _n) = send_traits(env, [np.arange(U + 1.0)], U + 1, False)
    hist = env.torch.zeros((Q, N + 1, umax + 1 + PT.NB + 3), dtype=env.torch.int32, device="cuda")
    total = env.torch.zeros((Q, N + 1, umax + 1), dtype=env.torch.int64, device="cuda")
    env.ctx.call("fcd_gibbs_set_patient_trait_accumulator", env.lib.dptr(hist), env.lib.dptr(total), N + 1, U + 1, 1)
    try:
        with pytest.raises(ValueError, match="patient-trait accumulator was made for"):
            eng._run(0, 1, 0, 0, False)
        with pytest.raises(ValueError, match="is attached"):            # and the traits cannot change under it
            send_traits(env, [np.arange(float(U))], U, False)
    finally:
        env.ctx.call("fcd_gibbs_set_patient_trait_accumulator", None, None, 0, 0, 1)
    assert int(hist.abs().sum()) == 0 and int(total.abs().sum()) == 0
    eng.run(0, 2, mstep_every=0, accumulate_from=None)                  # the context and the engine still run
    send_traits(env, [np.arange(float(U))], U, False)
    env.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)
