"""
Patient groups and contrasts on the MI355X: fcd_gibbs_patient_group_tally / fcd_gibbs_set_patient_group_accumulator against
the NumPy restatement of tests/patient_groups_ref.py, the shipped count and region-set kernels (the group of all patients),
the sampler's own chains recounted sweep by sweep, and the exact posterior of small models; the mean-field path through
fcd_vb_count_posterior; and patient_group_posterior() of a fit end to end.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
import patient_groups_ref as PG
from oracle.exact_chain import ExactChain

pytestmark = pytest.mark.gpu


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


def send_sets(env, sets, N):
    env.ctx.region_sets_owner = None                 # (no engine's)
    if sets is None:
        env.ctx.call("fcd_region_sets_set", None, None, 0)
        return 0
    (_names, offsets, members) = env.gibbs.region_sets_csr(sets, N)
    env.ctx.call("fcd_region_sets_set", i32p(offsets), i32p(members), len(offsets) - 1)
    return len(offsets) - 1


def send_groups(env, groups, contrasts, U, with_sets):
    """The groups to the context, straight through the C entry; (J, Umax, joint bins of all contrasts)."""
    (names, offsets, members) = env.gibbs.patient_groups_csr(groups, U)
    (pairs, bins) = env.gibbs.patient_group_contrasts(contrasts, names, offsets, members)
    env.ctx.patient_groups_owner = None
    env.ctx.call("fcd_patient_groups_set", i32p(offsets), i32p(members), len(names), i32p(pairs) if len(pairs) else None,
                 len(pairs), 1 if with_sets else 0)
    return len(names), int(np.diff(offsets).max()), int(bins[-1])


def tally(env, r_bits, N, U, G, J, rows, umax, bins, times=1):
    hg = env.torch.zeros((J, rows, umax + 1), dtype=env.torch.int32, device="cuda")
    hj = env.torch.zeros(max(1, rows * bins), dtype=env.torch.int32, device="cuda")
    for _ in range(times):
        env.ctx.call("fcd_gibbs_patient_group_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hg), env.lib.dptr(hj),
                     env.lib.stream_ptr())
    return hg.cpu().numpy().astype(np.int64), hj.cpu().numpy().astype(np.int64)


def single_state_case(G, N, U):
    """
    The groups: {0}, {U-1}, all patients, the two halves, two overlapping groups and, where U > 64, one that straddles patients
    63 / 64.  The contrasts: the two halves, and {0} against the second half (unequal sizes).  At U = 512 the halves have
    257 x 257 joint bins, above the cap of 16384 (refused: test_refusals_through_the_c_abi); the halves contrast is there
    between the first 127 patients of each half, 128 x 128 bins: exactly the cap.
    """
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    h = (U + 1) // 2
    groups = [[0], [U - 1], list(range(U)), list(range(h)), list(range(h, U)),
              list(range(0, max(2, 2 * U // 3))), list(range(U // 3, U))]
    contrasts = [(3, 4), (0, 4)]
    if U > 64:
        groups.append([62, 63, 64, 65])
    if (h + 1) * (U - h + 1) > 16384:
        groups += [list(range(127)), list(range(h, h + 127))]
        contrasts[0] = (len(groups) - 2, len(groups) - 1)
    sets = [[N - 1], list(range(N)), [0, N - 1]]
    return r, groups, contrasts, sets


@pytest.mark.parametrize("with_sets", [False, True], ids=["regions", "regions+sets"])
@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (64, 3, 3), (1, 2, 512), (130, 40, 5)])
def test_patient_group_tally_single_state(env, G, N, U, with_sets):
    """fcd_gibbs_patient_group_tally on an imported state: the NumPy histograms, integer for integer; a second run adds."""
    (r, groups, contrasts, sets) = single_state_case(G, N, U)
    sets = sets if with_sets else None
    rows = N + send_sets(env, sets, N)
    (J, umax, bins) = send_groups(env, groups, contrasts, U, with_sets)
    r_bits = import_r_bits(env, r)
    (want_g, want_j) = PG.histograms(r, groups, contrasts, sets)
    want_j = PG.flat_joint(want_j)
    assert want_g.shape == (J, rows, umax + 1) and want_j.shape == (rows * bins,)
    for times in (1, 2):
        (hg, hj) = tally(env, r_bits, N, U, G, J, rows, umax, bins, times=times)
        nptest.assert_array_equal(hg, times * want_g)
        nptest.assert_array_equal(hj, times * want_j)
    assert np.all(hg.sum(axis=2) == 2 * G) and hj.sum() == 2 * G * rows * len(contrasts)


def test_identities_with_the_count_and_region_set_kernels(env):
    """On one state, bit for bit: all patients at a region row is hist_region, at a set row hist_prev; {u} at the set of all
    regions is whether patient u has any anomalous region."""
    (G, N, U) = (200, 37, 70)
    rng = np.random.default_rng(G * N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.005, 0.1, (1, N, 1)) * rng.uniform(0.0, 1.0, (1, 1, U))).astype(np.uint8)
    r_bits = import_r_bits(env, r)
    hp = env.torch.zeros((U, N + 1), dtype=env.torch.int32, device="cuda")
    hr = env.torch.zeros((N, U + 1), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_count_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hp), env.lib.dptr(hr), env.lib.stream_ptr())
    (hp, hr) = (hp.cpu().numpy().astype(np.int64), hr.cpu().numpy().astype(np.int64))
    sets = [list(range(N)), [3], [0, 5, 36], list(range(10, 30))]
    JS = send_sets(env, sets, N)
    hs = env.torch.zeros((JS, U, N + 1), dtype=env.torch.int32, device="cuda")
    hv = env.torch.zeros((JS, U + 1), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_region_set_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hs), env.lib.dptr(hv), env.lib.stream_ptr())
    hv = hv.cpu().numpy().astype(np.int64)
    groups = [list(range(U))] + [[u] for u in (0, 1, 63, 64, 69)]
    (J, umax, bins) = send_groups(env, groups, None, U, True)
    (hg, _hj) = tally(env, r_bits, N, U, G, J, N + JS, umax, bins)
    nptest.assert_array_equal(hg[0, :N], hr)
    nptest.assert_array_equal(hg[0, N:], hv)
    for (j, u) in enumerate((0, 1, 63, 64, 69), start=1):
        assert hg[j, N, 1] == G - hp[u, 0] and hg[j, N, 0] == hp[u, 0] and not hg[j, N, 2:].any()
    assert hp[:, 0].max() > 0 and hp[:, 0].min() < G                  # (both outcomes occur)


GROUPS = {"low": list(range(0, 30)), "high": list(range(30, 70)), "straddle": [60, 63, 64, 69], "all": list(range(70)), "one": [64]}
CONTRASTS = [("low", "high"), ("one", "low")]
SETS = {"front": [0, 1, 2], "hub": [7], "whole": list(range(12))}


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


@pytest.mark.parametrize("with_sets", [False, True], ids=["regions", "regions+sets"])
def test_accumulator_inside_run_is_exact(env, small, stepped, with_sets):
    """K sweeps with the accumulator from sweep s0, every e: bit for bit the NumPy recount of a second engine's states."""
    (K, s0) = (9, 2)
    group_lists = list(GROUPS.values())
    pairs = [(0, 1), (4, 0)]
    sets = list(SETS.values()) if with_sets else None
    for every in (1, 3):
        e = small_engine(env, small)
        if with_sets:
            e.set_region_sets(SETS)
        e.set_patient_groups(GROUPS, CONTRASTS)
        e.attach_patient_group_accumulator(every)
        e.run(0, 4, mstep_every=0, accumulate_from=s0)               # in two calls: the counters carry over
        e.run(4, K - 4, mstep_every=0, accumulate_from=s0)
        nptest.assert_array_equal(e.export_state()[1], stepped[K - 1])
        counted = list(range(s0, K, every))
        assert e.patient_group_sweeps == len(counted)
        (hg, hj) = e.patient_group_host()
        rows = 12 + (3 if with_sets else 0)
        assert hg.shape == (5, rows, 71) and hj.shape == (rows * (31 * 41 + 2 * 31),)
        want = [PG.histograms(stepped[s], group_lists, pairs, sets) for s in counted]
        nptest.assert_array_equal(hg.astype(np.int64), sum(w[0] for w in want))
        nptest.assert_array_equal(hj.astype(np.int64), sum(PG.flat_joint(w[1]) for w in want))
        assert e.patient_group_row_names()[-1] == ("set:whole" if with_sets else "11")
        # the one-shot tally of the end state adds to fresh buffers what the last sweep added
        (one_g, one_j) = e.patient_group_tally(env.torch.zeros_like(e.patient_group_acc[0]), env.torch.zeros_like(e.patient_group_acc[1]))
        last = PG.histograms(stepped[K - 1], group_lists, pairs, sets)
        nptest.assert_array_equal(one_g.cpu().numpy().astype(np.int64), last[0])
        nptest.assert_array_equal(one_j.cpu().numpy().astype(np.int64), PG.flat_joint(last[1]))


def test_with_the_other_four_accumulators(env, small):
    """The new buffers alone or with the other four: equal; the other four with or without the new one: equal."""
    (K, s0) = (9, 2)
    periods = {"pair": 2, "count": 1, "coanomaly": 4, "region_set": 3}

    def run(with_groups, with_four):
        e = small_engine(env, small)
        e.set_region_sets(SETS)
        if with_four:
            e.attach_pair_accumulator(periods["pair"])
            e.attach_count_accumulator(periods["count"])
            e.attach_coanomaly_accumulator(periods["coanomaly"])
            e.attach_region_set_accumulator(periods["region_set"])
        if with_groups:
            e.set_patient_groups(GROUPS, CONTRASTS)
            e.attach_patient_group_accumulator(2)
        e.run(0, K, mstep_every=1, accumulate_from=s0)
        return e
    (alone, both, four) = (run(True, False), run(True, True), run(False, True))
    for (a, b) in zip(alone.patient_group_host(), both.patient_group_host()):
        nptest.assert_array_equal(a, b)
    assert alone.patient_group_sweeps == both.patient_group_sweeps == env.gibbs.pair_sweeps_in(0, K, s0, 2) == 4
    nptest.assert_array_equal(both.pair_counts_host(), four.pair_counts_host())
    for (a, b) in zip(both.count_hist_host() + both.coanomaly_host() + both.region_set_host(),
                      four.count_hist_host() + four.coanomaly_host() + four.region_set_host()):
        nptest.assert_array_equal(a, b)
    for key in periods:
        assert getattr(both, key + "_sweeps") == getattr(four, key + "_sweeps") == env.gibbs.pair_sweeps_in(0, K, s0, periods[key])
    nptest.assert_array_equal(both.export_state()[1], four.export_state()[1])
    # all patients inside the same run, at the count accumulator's period: its hist_region
    e = small_engine(env, small)
    e.attach_count_accumulator(3)
    e.set_patient_groups([list(range(70))])
    e.attach_patient_group_accumulator(3)
    e.run(0, K, mstep_every=1, accumulate_from=s0)
    nptest.assert_array_equal(e.patient_group_host()[0][0], e.count_hist_host()[1])


@pytest.mark.parametrize("name", ["4x2", "3x2"])
def test_gibbs_group_counts_against_exact(env, name):
    """2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: within 5 x 0.5/sqrt(G) + 1e-4."""
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    (groups, contrasts) = ([[0], [1], [0, 1]], [(0, 1)])
    ec = ExactChain(S_B, lM, gamma, pi2)
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (_f, r) = ec.all_states()                        # (S, N, U)
    r = r.astype(np.int64)
    want_g = np.zeros((3, N, 3))
    want_j = np.zeros((N, 2, 2))
    for n in range(N):
        for (j, g) in enumerate(groups):
            np.add.at(want_g[j, n], r[:, n, g].sum(axis=1), pi)
        np.add.at(want_j[n], (r[:, n, 0], r[:, n, 1]), pi)
    (P, K) = (ec.initial(X.PI0), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    G = X.G_CHAINS
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    eng.set_patient_groups(groups, contrasts)
    eng.attach_patient_group_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.patient_group_sweeps == 1
    (hg, hj) = eng.patient_group_host()
    (got_g, got_j) = (hg / float(G), hj.reshape(N, 2, 2) / float(G))
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%s: K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (
        name, K, max(np.abs(got_g - want_g).max(), np.abs(got_j - want_j).max()), tol))
    nptest.assert_allclose(got_g, want_g, rtol=0, atol=tol)
    nptest.assert_allclose(got_j, want_j, rtol=0, atol=tol)


def check_independent(out, lq_R, groups, contrasts, sets, names):
    (want_c, want_j) = PG.independent_laws(lq_R, groups, contrasts, sets)
    sizes = [len(g) for g in groups]
    assert out["names"] == names and out["sizes"].tolist() == sizes
    nptest.assert_allclose(out["p_count"], want_c, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_count"].sum(axis=2), 1.0, rtol=0, atol=1e-14)
    for (j, size) in enumerate(sizes):
        assert not out["p_count"][j, :, size + 1:].any()
    assert len(out["p_joint"]) == len(contrasts)
    for (got, want) in zip(out["p_joint"], want_j):
        nptest.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
    # the derived quantities: a joint cell is a product of two marginals (2e-12), its sums and the float arithmetic add a
    # little; the mean of the difference is a signed sum of terms of magnitude <= 1, so its bound is absolute
    want = PG.summaries(want_c, want_j, sizes, contrasts, 0.95)
    for key in ("prevalence", "p_greater", "p_less", "p_equal", "diff_mean"):
        nptest.assert_allclose(out[key], want[key], rtol=4e-12, atol=4e-12 if key == "diff_mean" else 1e-300, err_msg=key)


def test_vb_patient_group_posterior(env):
    """The mean-field path against the NumPy laws on _lq_R at rtol 1e-12, with q = 0 and q = 1 rows, with and without sets."""
    (N, U) = (12, 9)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 6, U, seed=4)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.max_iters = env.pkg.UnsharedRegionModel(), b, bt, 3
    fit.run()
    groups = [[0, 1, 2, 3], [4], [5, 6, 7, 8], list(range(U)), [3, 8], [1, 2]]
    contrasts = [(0, 2), (1, 2), (4, 5)]
    (fit.patient_groups, fit.patient_group_contrasts) = (groups, contrasts)
    out = fit.patient_group_posterior()
    check_independent(out, fit._lq_R, groups, contrasts, None, [str(j) for j in range(len(groups))])
    assert out["row_names"] == [str(n) for n in range(N)] and out["contrasts"] == [("0", "2"), ("1", "2"), ("4", "5")]
    rng = np.random.default_rng(9)
    q1 = rng.uniform(0.02, 0.98, (N, U))
    q1[4, :] = 0.0                                   # region 4 never (but in patient 5, below): a point mass
    q1[3, :] = 1.0                                   # region 3 always: a point mass at the group's size
    q1[1:3, 2] = 0.0
    q1[:, 5] = 1.0
    with np.errstate(divide="ignore"):
        fit._lq_R = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))     # not normalised
    names = ["g%d" % j for j in range(len(groups))]
    sets = {"front": [0, 1, 2], "never": [4], "all": list(range(N))}
    (fit.patient_groups, fit.region_sets) = (dict(zip(names, groups)), sets)
    fit.patient_group_contrasts = [("g0", "g2"), ("g1", "g2"), (4, 5)]
    out = fit.patient_group_posterior()
    check_independent(out, fit._lq_R, groups, contrasts, list(sets.values()), names)
    assert out["row_names"][N:] == ["set:front", "set:never", "set:all"]
    for (j, size) in enumerate(out["sizes"]):
        k4 = int(5 in groups[j])                                                 # (patient 5 has every region, region 4 too)
        assert np.array_equal(out["p_count"][j, 4], np.eye(U + 1)[k4])           # region 4, and the set {4}
        assert np.array_equal(out["p_count"][j, N + 1], np.eye(U + 1)[k4])
        assert np.array_equal(out["p_count"][j, 3], np.eye(U + 1)[size])         # region 3, and the set of all regions
        assert np.array_equal(out["p_count"][j, N + 2], np.eye(U + 1)[size])
    assert np.array_equal(out["p_equal"][:, 3], [1.0, 1.0, 1.0]) and np.array_equal(out["diff_interval"][:, 3], np.zeros((3, 2)))
    again = fit.patient_group_posterior(independent=True)
    for key in ("p_count", "prevalence", "diff_mean"):
        nptest.assert_array_equal(again[key], out[key])


def test_fit_gibbs_patient_groups(env):
    """The fit end to end: 16 regions x 16 patients, 256 chains, two groups and a contrast; the default-off path attaches nothing."""
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(16, 6, 16, seed=8)

    def gibbs_fit(**kw):
        fit = env.pkg.fit.UnsharedRegionFit()
        fit._ctx = env.ctx
        fit.model, fit.b, fit.bt = env.pkg.UnsharedRegionModel(), b, bt
        fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed = "gibbs", 256, 12, 3, 5
        for (k, v) in kw.items():
            setattr(fit, k, v)
        fit.run()
        return fit
    off = gibbs_fit()
    assert off.patient_group_hist is None and off.sampler.patient_group_acc is None
    with pytest.raises(ValueError, match="set patient_groups before run"):
        off.patient_group_posterior()
    groups = {"treated": list(range(0, 6)), "untreated": list(range(6, 16))}
    on = gibbs_fit(patient_groups=groups, patient_group_contrasts=[("treated", "untreated")], patient_groups_every=2,
                   region_sets={"front": [0, 1, 2], "all": list(range(16))}, region_sets_every=2)
    nptest.assert_array_equal(on.sampler.export_state()[1], off.sampler.export_state()[1])
    nptest.assert_array_equal(on._lq_R, off._lq_R)
    n_acc = 5                                        # sweeps 3, 5, 7, 9, 11
    assert on.patient_group_sweeps == n_acc
    (hg, hj) = (on.patient_group_hist, on.patient_group_joint_hist)
    assert hg.shape == (2, 18, 11) and hg.dtype == np.int64 and [j.shape for j in hj] == [(18, 7, 11)]
    assert np.all(hg.sum(axis=2) == 256 * n_acc) and np.all(hj[0].sum(axis=(1, 2)) == 256 * n_acc)
    assert not hg[0, :, 7:].any()
    out = on.patient_group_posterior()
    assert out["names"] == ["treated", "untreated"] and out["sizes"].tolist() == [6, 10]
    assert out["row_names"] == [str(n) for n in range(16)] + ["set:front", "set:all"]
    assert out["contrasts"] == [("treated", "untreated")]
    nptest.assert_allclose(out["p_count"], hg / (256.0 * n_acc), rtol=1e-15)
    nptest.assert_allclose(out["p_joint"][0].sum(axis=2), out["p_count"][0, :, :7], rtol=1e-13, atol=1e-16)
    nptest.assert_allclose(out["p_joint"][0].sum(axis=1), out["p_count"][1], rtol=1e-13, atol=1e-16)
    want = PG.summaries(out["p_count"], out["p_joint"], [6, 10], [(0, 1)], 0.95)
    for key in ("prevalence", "p_greater", "p_less", "p_equal", "diff_mean", "diff_interval"):
        nptest.assert_allclose(out[key], want[key], rtol=1e-13, atol=1e-15, err_msg=key)
    nptest.assert_allclose(out["diff_mean"][0], out["prevalence"][0] - out["prevalence"][1], rtol=1e-12, atol=1e-14)
    # the set rows against the region-set histograms of the same sweeps: the two groups split the patients, so their counts add
    # up to the number of patients the set is hit in
    nptest.assert_allclose((hg[0, 16:] @ np.arange(11)) + (hg[1, 16:] @ np.arange(11)),
                           on.region_set_prevalence_hist @ np.arange(17), rtol=0, atol=0)
    ind = on.patient_group_posterior(independent=True)
    (want_c, want_j) = PG.independent_laws(on._lq_R, list(groups.values()), [(0, 1)], [[0, 1, 2], list(range(16))])
    nptest.assert_allclose(ind["p_count"], want_c, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(ind["p_joint"][0], want_j[0], rtol=1e-12, atol=1e-300)
    assert np.abs(ind["p_joint"][0] - out["p_joint"][0]).max() > 1e-3            # the joint form is not the mean field
    early = gibbs_fit(patient_groups=groups, n_sweeps=3)
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        early.patient_group_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(patient_groups={"bad": [3, 16]})


def test_refusals_through_the_c_abi(env):
    """The checks that come before any device work, on a live context; the device pointers are never dereferenced."""
    (lib, ctx, E) = (env.lib.load(), env.ctx.handle, env.lib)
    fake = C.c_void_p(16)
    (env.ctx.region_sets_owner, env.ctx.patient_groups_owner) = (None, None)
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_patient_groups_set(ctx, None, None, 0, None, 0, 0) == 0                                  # clears
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 4, 2, 64, fake, fake, None) == E.FCD_ERR_ARG       # no groups
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 4, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_patient_groups_set(ctx, None, None, 0, i32p([0, 1]), 1, 0) == E.FCD_ERR_ARG             # contrasts alone
    assert lib.fcd_patient_groups_set(ctx, None, i32p([0]), 1, None, 0, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 1]), i32p([0]), 0, None, 0, 0) == E.FCD_ERR_ARG
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 1, 1]), i32p([0]), 2, None, 0, 0) == E.FCD_ERR_ARG     # an empty group
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 2]), i32p([-1, 3]), 1, None, 0, 0) == E.FCD_ERR_ARG    # negative
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 2]), i32p([3, 3]), 1, None, 0, 0) == E.FCD_ERR_ARG     # a duplicate
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 3]), i32p([1, 3, 2]), 1, None, 0, 0) == E.FCD_ERR_ARG  # not ascending
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 1]), i32p([512]), 1, None, 0, 0) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_patient_groups_set(ctx, i32p(np.arange(66)), i32p(np.zeros(65)), 65, None, 0, 0) == E.FCD_ERR_UNSUPPORTED
    two = (i32p([0, 2, 4]), i32p([0, 1, 2, 3]), 2)
    assert lib.fcd_patient_groups_set(ctx, *two, None, 1, 0) == E.FCD_ERR_ARG                              # P without pairs
    assert lib.fcd_patient_groups_set(ctx, *two, i32p([0, 1] * 65), 65, 0) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_patient_groups_set(ctx, *two, i32p([0, 2]), 1, 0) == E.FCD_ERR_ARG                      # no such group
    assert lib.fcd_patient_groups_set(ctx, *two, i32p([1, 1]), 1, 0) == E.FCD_ERR_ARG                      # one group twice
    assert b"twice" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 2, 4]), i32p([0, 1, 1, 3]), 2, i32p([0, 1]), 1, 0) == E.FCD_ERR_ARG
    assert b"overlap" in lib.fcd_last_message(ctx)
    # the two halves of 512 patients: fine as groups, but 257 x 257 joint bins are above the cap; the message names the contrast
    halves = (i32p([0, 256, 512]), i32p(np.arange(512)), 2)
    assert lib.fcd_patient_groups_set(ctx, *halves, None, 0, 0) == 0
    assert lib.fcd_patient_groups_set(ctx, *halves, i32p([1, 0]), 1, 0) == E.FCD_ERR_UNSUPPORTED
    assert b"contrast 0 has 66049 joint bins" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_groups_set(ctx, i32p([0, 127, 254]), i32p(np.arange(254)), 2, i32p([0, 1]), 1, 0) == 0      # the cap itself
    # {0, 1} against {2, 3}: the shape checks of the tally and of the accumulator
    assert lib.fcd_patient_groups_set(ctx, *two, i32p([0, 1]), 1, 0) == 0
    assert lib.fcd_gibbs_patient_group_tally(ctx, None, 6, 4, 64, fake, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 6, 4, 64, fake, None, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 6, 4, 0, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 6, 3, 64, fake, fake, None) == E.FCD_ERR_SHAPE     # member 3 of 3 patients
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 6, 513, 64, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    # scratch: 2 groups x 40000 rows x 2^20 chains x 2 bytes > 1 GiB
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 40000, 4, 1 << 20, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, None, 6, 4, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 1, 4, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 0, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 3, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 513, 1) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 4, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 4, 1) == 0
    assert lib.fcd_patient_groups_set(ctx, *two, None, 0, 0) == E.FCD_ERR_ARG                              # attached
    assert b"is attached" in lib.fcd_last_message(ctx)
    assert lib.fcd_patient_groups_set(ctx, None, None, 0, None, 0, 0) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32p([0, 1]), i32p([0]), 1) == 0                                    # no set rows: free to change
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, None, None, 0, 0, 1) == 0
    # the same groups with the region sets {0, 5}, {2} as rows
    assert lib.fcd_patient_groups_set(ctx, *two, i32p([0, 1]), 1, 1) == 0
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 6, 4, 64, fake, fake, None) == E.FCD_ERR_ARG       # ... and there are none
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 4, 1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32p([0, 2, 3]), i32p([0, 5, 2]), 2) == 0
    assert lib.fcd_gibbs_patient_group_tally(ctx, fake, 5, 4, 64, fake, fake, None) == E.FCD_ERR_SHAPE     # member 5 of 5 regions
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 5, 4, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, fake, fake, 6, 4, 1) == 0
    assert lib.fcd_region_sets_set(ctx, i32p([0, 1]), i32p([0]), 1) == E.FCD_ERR_ARG                       # the sets are rows
    assert b"patient-group accumulator" in lib.fcd_last_message(ctx)
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_group_accumulator(ctx, None, None, 0, 0, 1) == 0
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0
    assert lib.fcd_patient_groups_set(ctx, None, None, 0, None, 0, 0) == 0


def test_run_refuses_another_shape_while_attached(env):
    (N, U, G) = (12, 5, 64)
    (m, S_B, lM) = tables(env, N, 3, U, seed=3)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    send_sets(env, None, N)
    (J, umax, bins) = send_groups(env, [[0, 1], [5]], [(0, 1)], U + 1, False)
    hg = env.torch.zeros((J, N + 1, umax + 1), dtype=env.torch.int32, device="cuda")
    hj = env.torch.zeros((N + 1) * bins, dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_set_patient_group_accumulator", env.lib.dptr(hg), env.lib.dptr(hj), N + 1, U + 1, 1)
    try:
        with pytest.raises(ValueError, match="patient-group accumulator was made for"):
            eng._run(0, 1, 0, 0, False)
        with pytest.raises(ValueError, match="is attached"):            # and the groups cannot change under it
            send_groups(env, [[0]], None, U, False)
    finally:
        env.ctx.call("fcd_gibbs_set_patient_group_accumulator", None, None, 0, 0, 1)
    assert int(hg.abs().sum()) == 0 and int(hj.abs().sum()) == 0
    send_groups(env, [[0]], None, U, False)
    env.ctx.call("fcd_patient_groups_set", None, None, 0, None, 0, 0)
