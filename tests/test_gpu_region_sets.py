"""
Region-set counts on the MI355X: fcd_gibbs_region_set_tally / fcd_gibbs_set_region_set_accumulator against the NumPy
restatement of tests/region_sets_ref.py, the shipped count kernels (the set of all regions, the singletons), the C oracle's
chains and the exact posterior of small models; the mean-field path through fcd_vb_count_posterior; and
region_set_posterior() of both fits end to end.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest

import exact_law_cases as X
import region_sets_ref as RS
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


def send_sets(env, sets, N):
    """The sets to the context, straight through the C entry; (J, S_max)."""
    (_names, offsets, members) = env.gibbs.region_sets_csr(sets, N)
    env.ctx.region_sets_owner = None                 # (no engine's)
    env.ctx.call("fcd_region_sets_set", offsets.ctypes.data_as(C.c_void_p), members.ctypes.data_as(C.c_void_p), len(offsets) - 1)
    return len(offsets) - 1, int(np.diff(offsets).max())


def tally(env, r_bits, N, U, G, J, s_max, times=1):
    hs = env.torch.zeros((J, U, s_max + 1), dtype=env.torch.int32, device="cuda")
    hv = env.torch.zeros((J, U + 1), dtype=env.torch.int32, device="cuda")
    for _ in range(times):
        env.ctx.call("fcd_gibbs_region_set_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hs), env.lib.dptr(hv),
                     env.lib.stream_ptr())
    return hs.cpu().numpy().astype(np.int64), hv.cpu().numpy().astype(np.int64)


def many_sets(N, rng):
    """700 sets from repeats, overlaps, singletons and {first, last}: with three chain words, more pairs than the block cap."""
    sets = [[0, N - 1], list(range(N))]
    sets += [[n] for n in range(N)]
    sets += [list(range(a, min(N, a + 7))) for a in range(0, N, 3)]                       # overlapping runs
    while len(sets) < 700:
        k = int(rng.integers(1, N + 1))
        sets.append(sorted(rng.choice(N, size=k, replace=False).tolist()))
        if len(sets) % 5 == 0:
            sets.append(list(sets[-1]))                                                   # a repeat
    return sets[:700]


def single_state_case(G, N, U):
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.05, 0.95, (1, N, 1))).astype(np.uint8)
    if (G, N, U) == (130, 9, 70):
        sets = [list(range(N)), [0], [N - 1], [0, N - 1], [1, 3, 5], [1, 3, 5], [2, 3, 4, 5, 6]]
    elif N == 1023:
        sets = [list(range(N))]
        r[0] = 1                                     # a chain with all 1023: every bit plane carries
        r[1] = 0
    elif (G, N, U) == (1, 2, 512):
        sets = [[0], [1], [0, 1]]
    else:
        sets = many_sets(N, rng)
    return r, sets


@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (64, 1023, 3), (1, 2, 512), (130, 40, 5)])
def test_region_set_tally_single_state(env, G, N, U):
    """fcd_gibbs_region_set_tally on an imported state: the NumPy histograms, integer for integer, and it adds."""
    (r, sets) = single_state_case(G, N, U)
    (J, s_max) = send_sets(env, sets, N)
    if N == 40:
        assert J == 700 and J * ((G + 63) // 64) > 8 * env.torch.cuda.get_device_properties(0).multi_processor_count
    (hs, hv) = tally(env, import_r_bits(env, r), N, U, G, J, s_max, times=2)
    (want_s, want_v) = RS.histograms(r, sets)
    nptest.assert_array_equal(hs, 2 * want_s)
    nptest.assert_array_equal(hv, 2 * want_v)
    assert np.all(hs.sum(axis=2) == 2 * G) and np.all(hv.sum(axis=1) == 2 * G)
    if N == 1023:
        assert hs[0, :, 1023].min() >= 2 and hs[0, :, 0].min() >= 2


@pytest.mark.parametrize("G,N,U", [(130, 9, 70), (200, 37, 5)])
def test_identities_with_the_count_kernels(env, G, N, U):
    """On one state, bit for bit: the set of all regions is hist_patient, the singletons are hist_region and the marginal counts."""
    rng = np.random.default_rng(G * N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.02, 0.6, (1, N, 1))).astype(np.uint8)
    r_bits = import_r_bits(env, r)
    hp = env.torch.zeros((U, N + 1), dtype=env.torch.int32, device="cuda")
    hr = env.torch.zeros((N, U + 1), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_count_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(hp), env.lib.dptr(hr), env.lib.stream_ptr())
    (hp, hr) = (hp.cpu().numpy().astype(np.int64), hr.cpu().numpy().astype(np.int64))
    (J, s_max) = send_sets(env, [list(range(N))], N)
    (hs, _hv) = tally(env, r_bits, N, U, G, J, s_max)
    nptest.assert_array_equal(hs[0], hp)
    (J, s_max) = send_sets(env, [[n] for n in range(N)], N)
    (hs, hv) = tally(env, r_bits, N, U, G, J, s_max)
    nptest.assert_array_equal(hv, hr)
    nptest.assert_array_equal(hs[:, :, 1], r.astype(np.int64).sum(axis=0))


CFG2_SETS = {"a": range(0, 10), "b": range(10, 19), "c": range(19, 30), "d": range(30, 37), "e": range(37, 50),
             "f": range(50, 58), "g": range(58, 64), "ends": [0, 63], "one": [17], "overlap": range(5, 40), "a again": range(0, 10)}
CFG2_SETS = {k: list(v) for (k, v) in CFG2_SETS.items()}


def cfg2_engine(env, tabs, seed=404, G=256):
    (m, S_B_d, lM_d) = tabs
    e = env.GibbsEngine(S_B_d, lM_d, 64, 16, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    e.set_hyper(m.gamma, m.pi2())
    e.init(0.2)
    return e


@pytest.fixture(scope="module")
def cfg2(env):
    (m, S_B, lM) = tables(env, 64, 16, 16, seed=80)
    return m, S_B, lM, (m, up(env, S_B), up(env, lM))


def test_accumulator_is_exact(env, cfg2):
    """
    fcd_gibbs_run with the accumulator, every = 1 / 3: equal, integer for integer, to the NumPy histograms of the C
    oracle's chains over the same sweeps.  The sampler is untouched: chain state and hyper block bit-identical to a run
    with nothing attached.
    """
    (N, U, G, n_sweeps, burn, seed) = (64, 16, 256, 9, 2, 404)
    (m, S_B, lM, tabs) = cfg2
    sets = list(CFG2_SETS.values())
    plain = cfg2_engine(env, tabs)
    plain.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
    (f0, r0) = plain.export_state()
    h0 = plain.host(plain.hyper)
    for every in (1, 3):
        acc = cfg2_engine(env, tabs)
        acc.set_region_sets(CFG2_SETS)
        acc.attach_region_set_accumulator(every)
        acc.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        (f1, r1) = acc.export_state()
        nptest.assert_array_equal(f1, f0)
        nptest.assert_array_equal(r1, r0)
        assert np.array_equal(acc.host(acc.hyper), h0)
        assert acc.region_set_sweeps == len(range(burn, n_sweeps, every))
        (hs, hv) = acc.region_set_host()
        assert hs.shape == (len(sets), U, 36) and hv.shape == (len(sets), U + 1)
        assert np.all(hs.sum(axis=2) == G * acc.region_set_sweeps) and np.all(hv.sum(axis=1) == G * acc.region_set_sweeps)
    # against the C oracle's chains (fixed hyper-parameters)
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.2, seed, 0)
    per_sweep = {}
    for s in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, 0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, env.lib.EDGE_MODES["symmetric"], 0)
        if s >= burn:
            per_sweep[s] = RS.histograms(r_o, sets)
    for every in (1, 3):
        eng = cfg2_engine(env, tabs)
        eng.set_region_sets(CFG2_SETS)
        eng.attach_region_set_accumulator(every)
        eng.run(0, n_sweeps, mstep_every=0, accumulate_from=burn)
        (hs, hv) = eng.region_set_host()
        nptest.assert_array_equal(hs.astype(np.int64), sum(per_sweep[s][0] for s in range(burn, n_sweeps, every)))
        nptest.assert_array_equal(hv.astype(np.int64), sum(per_sweep[s][1] for s in range(burn, n_sweeps, every)))
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o)
        nptest.assert_array_equal(r_g, r_o)
        # the one-shot tally of the end state adds to a fresh pair of buffers what the last sweep added
        (one_s, one_v) = eng.region_set_tally(env.torch.zeros_like(eng.region_set_acc[0]), env.torch.zeros_like(eng.region_set_acc[1]))
        nptest.assert_array_equal(one_s.cpu().numpy().astype(np.int64), per_sweep[n_sweeps - 1][0])
        nptest.assert_array_equal(one_v.cpu().numpy().astype(np.int64), per_sweep[n_sweeps - 1][1])


def test_with_the_other_three_accumulators(env, cfg2):
    """The new buffers alone or with the other three: equal; the other three with or without the new one: equal."""
    (n_sweeps, burn) = (9, 2)
    tabs = cfg2[3]
    periods = {"pair": 2, "count": 1, "coanomaly": 4}

    def run(with_sets, with_three):
        e = cfg2_engine(env, tabs)
        if with_three:
            e.attach_pair_accumulator(periods["pair"])
            e.attach_count_accumulator(periods["count"])
            e.attach_coanomaly_accumulator(periods["coanomaly"])
        if with_sets:
            e.set_region_sets(CFG2_SETS)
            e.attach_region_set_accumulator(3)
        e.run(0, 4, mstep_every=1, accumulate_from=burn)              # in two calls: the counters carry over
        e.run(4, n_sweeps - 4, mstep_every=1, accumulate_from=burn)
        return e
    alone = run(True, False)
    both = run(True, True)
    three = run(False, True)
    for (a, b) in zip(alone.region_set_host(), both.region_set_host()):
        nptest.assert_array_equal(a, b)
    assert alone.region_set_sweeps == both.region_set_sweeps == env.gibbs.pair_sweeps_in(0, n_sweeps, burn, 3) == 3
    nptest.assert_array_equal(both.pair_counts_host(), three.pair_counts_host())
    for (a, b) in zip(both.count_hist_host() + both.coanomaly_host(), three.count_hist_host() + three.coanomaly_host()):
        nptest.assert_array_equal(a, b)
    for key in periods:
        assert getattr(both, key + "_sweeps") == getattr(three, key + "_sweeps") == env.gibbs.pair_sweeps_in(0, n_sweeps, burn, periods[key])
    # the set of all regions inside the same run: the count accumulator's hist_patient at the same period
    e = cfg2_engine(env, tabs)
    e.attach_count_accumulator(3)
    e.set_region_sets([list(range(64))])
    e.attach_region_set_accumulator(3)
    e.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
    nptest.assert_array_equal(e.region_set_host()[0][0], e.count_hist_host()[0])


def test_run_refuses_another_shape_while_attached(env):
    (N, U, G) = (12, 5, 64)
    (m, S_B, lM) = tables(env, N, 3, U, seed=3)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.2)
    (J, s_max) = send_sets(env, [[0, 1], [11]], N)
    hs = env.torch.zeros((J, U + 1, s_max + 1), dtype=env.torch.int32, device="cuda")
    hv = env.torch.zeros((J, U + 2), dtype=env.torch.int32, device="cuda")
    env.ctx.call("fcd_gibbs_set_region_set_accumulator", env.lib.dptr(hs), env.lib.dptr(hv), N + 1, U + 1, 1)
    try:
        with pytest.raises(ValueError, match="region-set accumulator was made for"):
            eng._run(0, 1, 0, 0, False)
        with pytest.raises(ValueError, match="is attached"):            # and the sets cannot change under it
            send_sets(env, [[0]], N)
    finally:
        env.ctx.call("fcd_gibbs_set_region_set_accumulator", None, None, 0, 0, 1)
    assert int(hs.abs().sum()) == 0 and int(hv.abs().sum()) == 0
    send_sets(env, [[0]], N)


def test_host_side_refusals_with_a_context(env):
    """The checks that come before any device work, on a live context; the device pointers are never dereferenced."""
    (lib, ctx, E) = (env.lib.load(), env.ctx.handle, env.lib)
    fake = C.c_void_p(16)
    i32 = lambda *v: np.asarray(v, dtype=np.int32).ctypes.data_as(C.c_void_p)      # noqa: E731
    env.ctx.region_sets_owner = None
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0                        # clears
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 4, 2, 64, fake, fake, None) == E.FCD_ERR_ARG          # no sets
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 4, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, None, i32(0), 1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32(0, 1), None, 1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32(0, 1), i32(0), 0) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32(0, 1), i32(0), -1) == E.FCD_ERR_ARG
    assert lib.fcd_region_sets_set(ctx, i32(0, 1, 1), i32(0), 2) == E.FCD_ERR_ARG                          # an empty set
    assert lib.fcd_region_sets_set(ctx, i32(0, 2, 1), i32(0, 1), 2) == E.FCD_ERR_ARG                       # offsets go back
    assert lib.fcd_region_sets_set(ctx, i32(0, 2), i32(-1, 3), 1) == E.FCD_ERR_ARG                         # negative
    assert lib.fcd_region_sets_set(ctx, i32(0, 2), i32(3, 3), 1) == E.FCD_ERR_ARG                          # a duplicate
    assert lib.fcd_region_sets_set(ctx, i32(0, 3), i32(1, 3, 2), 1) == E.FCD_ERR_ARG                       # not increasing
    big = np.arange(1024, dtype=np.int32)
    assert lib.fcd_region_sets_set(ctx, i32(0, 1024), big.ctypes.data_as(C.c_void_p), 1) == E.FCD_ERR_UNSUPPORTED
    offs = np.arange(1026, dtype=np.int32)
    assert lib.fcd_region_sets_set(ctx, offs.ctypes.data_as(C.c_void_p), np.zeros(1025, dtype=np.int32).ctypes.data_as(C.c_void_p),
                                   1025) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 4, 2, 64, fake, fake, None) == E.FCD_ERR_ARG          # still no sets
    assert lib.fcd_region_sets_set(ctx, i32(0, 2, 3), i32(0, 5, 2), 2) == 0                                # {0, 5}, {2}
    assert lib.fcd_gibbs_region_set_tally(ctx, None, 6, 2, 64, fake, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 6, 2, 64, None, fake, None) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 6, 2, 0, fake, fake, None) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 5, 2, 64, fake, fake, None) == E.FCD_ERR_SHAPE        # member 5 of 5 regions
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 6, 513, 64, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    # scratch: (2 * 512 + 2) rows x 2^20 chains x 2 bytes > 1 GiB
    assert lib.fcd_gibbs_region_set_tally(ctx, fake, 6, 512, 1 << 20, fake, fake, None) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, None, 6, 2, 1) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 1, 2, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 6, 0, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 5, 2, 1) == E.FCD_ERR_SHAPE
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 6, 513, 1) == E.FCD_ERR_UNSUPPORTED
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 6, 2, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, fake, fake, 6, 2, 1) == 0
    assert lib.fcd_region_sets_set(ctx, i32(0, 1), i32(0), 1) == E.FCD_ERR_ARG                             # attached
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == E.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_region_set_accumulator(ctx, None, None, 0, 0, 1) == 0
    assert lib.fcd_region_sets_set(ctx, None, None, 0) == 0


def exact_set_laws(name, sets):
    """Exact posterior law of both set counts of an exact_law_cases problem: (p_count (J, U, S_max+1), p_prev (J, U+1), ec, pi)."""
    (N, U, S_B, lM, gamma, pi2, _seed) = X.problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (_f, r) = ec.all_states()                        # (S, N, U)
    s_max = max(len(s) for s in sets)
    p_count = np.zeros((len(sets), U, s_max + 1))
    p_prev = np.zeros((len(sets), U + 1))
    for (j, s) in enumerate(sets):
        k = r.astype(np.int64)[:, s, :].sum(axis=1)  # (S, U)
        for u in range(U):
            np.add.at(p_count[j, u], k[:, u], pi)
        np.add.at(p_prev[j], (k > 0).sum(axis=1), pi)
    return p_count, p_prev, ec, pi


@pytest.mark.parametrize("name", ["4x2", "3x2"])
def test_gibbs_set_counts_against_exact(env, name):
    """2^18 chains, K sweeps with ||P_K - pi||_1 < 1e-4, only the last one counted: within 5 x 0.5/sqrt(G) + 1e-4."""
    (N, U, S_B, lM, gamma, pi2, seed) = X.problem(name)
    sets = [[0, 1], list(range(1, N)), [0]]
    (want_c, want_v, ec, pi) = exact_set_laws(name, sets)
    (P, K) = (ec.initial(X.PI0), 0)
    while np.abs(P.reshape(-1) - pi).sum() >= 1e-4:
        P = ec.sweep(P)
        K += 1
        assert K <= 400
    G = X.G_CHAINS
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=0, seed=seed, edge_index="symmetric", ctx=env.ctx)
    eng.set_hyper(gamma, pi2)
    eng.init(X.PI0)
    eng.set_region_sets(sets)
    eng.attach_region_set_accumulator(1)
    eng.run(0, K, mstep_every=0, accumulate_from=K - 1)
    assert eng.region_set_sweeps == 1
    (hs, hv) = eng.region_set_host()
    (got_c, got_v) = (hs / float(G), hv / float(G))
    tol = 5 * 0.5 / np.sqrt(G) + 1e-4
    print("%s: K = %d sweeps, worst deviation %.2e (tolerance %.2e)" % (
        name, K, max(np.abs(got_c - want_c).max(), np.abs(got_v - want_v).max()), tol))
    nptest.assert_allclose(got_c, want_c, rtol=0, atol=tol)
    nptest.assert_allclose(got_v, want_v, rtol=0, atol=tol)


def check_independent(out, lq_R, sets, names):
    (want_c, want_v) = RS.independent_laws(lq_R, sets)
    assert out["names"] == names and out["sizes"].tolist() == [len(s) for s in sets]
    nptest.assert_allclose(out["p_count"], want_c, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_prevalence"], want_v, rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_any"], 1.0 - want_c[:, :, 0], rtol=1e-12, atol=1e-15)
    nptest.assert_allclose(out["expected"], want_c @ np.arange(want_c.shape[2]), rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_none"], want_v[:, 0], rtol=1e-12, atol=1e-300)
    nptest.assert_allclose(out["p_count"].sum(axis=2), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(out["p_prevalence"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    for (j, s) in enumerate(sets):
        assert not out["p_count"][j, :, len(s) + 1:].any()


def test_vb_region_set_posterior(env):
    """The mean-field path against the NumPy laws on _lq_R at rtol 1e-12, with q = 0 and q = 1 rows, in all three input forms."""
    (N, U) = (12, 9)
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 6, U, seed=4)
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.max_iters = env.pkg.UnsharedRegionModel(), b, bt, 3
    fit.run()
    sets = [[0, 1, 2, 3], [4], [5, 6, 7, 8, 9, 10, 11], list(range(N)), [3, 11], [1, 2]]
    fit.region_sets = sets
    check_independent(fit.region_set_posterior(), fit._lq_R, sets, [str(j) for j in range(len(sets))])
    rng = np.random.default_rng(9)
    q1 = rng.uniform(0.02, 0.98, (N, U))
    q1[4, :] = 0.0                                   # region 4 never: its singleton is a point mass at 0, in no patient
    q1[3, :] = 1.0                                   # region 3 always: every set with it is hit in all patients
    q1[1:3, 2] = 0.0
    q1[:, 5] = 1.0
    with np.errstate(divide="ignore"):
        fit._lq_R = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))     # not normalised
    names = ["n%d" % j for j in range(len(sets))]
    fit.region_sets = dict(zip(names, sets))
    out = fit.region_set_posterior()
    check_independent(out, fit._lq_R, sets, names)
    want = np.tile(np.eye(N + 1)[0], (U, 1))         # the singleton {4}: a point mass at 0, at 1 in patient 5
    want[5] = np.eye(N + 1)[1]
    assert np.array_equal(out["p_count"][1], want)
    assert np.array_equal(out["p_prevalence"][0], np.eye(U + 1)[U]) and out["p_none"][0] == 0.0
    mask = np.zeros((len(sets), N), dtype=bool)
    for (j, s) in enumerate(sets):
        mask[j, s] = True
    fit.region_sets = mask
    again = fit.region_set_posterior(independent=True)
    for key in ("p_count", "p_prevalence", "expected"):
        nptest.assert_array_equal(again[key], out[key])


def gibbs_fit(env, cls=None, **kw):
    gen = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(10, 6, 7, seed=8)
    fit = (cls or env.pkg.fit.UnsharedRegionFit)()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt = (env.pkg.SharedRegionModel() if cls else env.pkg.UnsharedRegionModel()), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in, fit.seed = "gibbs", 192, 12, 3, 5
    for (k, v) in kw.items():
        setattr(fit, k, v)
    fit.run()
    return fit


NETWORKS = {"all": list(range(10)), "front": [0, 1, 2], "back": [9, 7, 8], "hub": [4], "mixed": [2, 4, 6, 8]}


def test_fit_gibbs_region_sets(env):
    """The fit end to end: a dict of sets every second sweep beside the anomaly counts; the default-off path attaches nothing."""
    off = gibbs_fit(env, anomaly_counts=True, anomaly_counts_every=2, energy_every=4)
    assert off.region_set_hist is None and off.region_set_prevalence_hist is None and off.sampler.region_set_acc is None
    with pytest.raises(ValueError, match="set region_sets before run"):
        off.region_set_posterior()
    on = gibbs_fit(env, anomaly_counts=True, anomaly_counts_every=2, energy_every=4, region_sets=NETWORKS, region_sets_every=2)
    (f_off, r_off) = off.sampler.export_state()
    (f_on, r_on) = on.sampler.export_state()
    nptest.assert_array_equal(f_on, f_off)
    nptest.assert_array_equal(r_on, r_off)
    nptest.assert_array_equal(on._lq_F, off._lq_F)
    nptest.assert_array_equal(on._lq_R, off._lq_R)
    assert len(on.energy) == 3 and on.energy == off.energy
    nptest.assert_array_equal(on.patient_count_hist, off.patient_count_hist)
    n_acc = 5                                        # sweeps 3, 5, 7, 9, 11
    assert on.region_set_sweeps == on.anomaly_count_sweeps == n_acc
    (hs, hv) = (on.region_set_hist, on.region_set_prevalence_hist)
    assert hs.shape == (5, 7, 11) and hv.shape == (5, 8) and hs.dtype == np.int64
    assert np.all(hs.sum(axis=2) == 192 * n_acc) and np.all(hv.sum(axis=1) == 192 * n_acc)
    out = on.region_set_posterior()
    assert out["names"] == list(NETWORKS) and out["sizes"].tolist() == [10, 3, 3, 1, 4]
    nptest.assert_array_equal(hs[0], on.patient_count_hist)
    nptest.assert_allclose(out["p_count"][0], on.anomaly_count_posterior()["p_patient_count"], rtol=1e-15)
    nptest.assert_allclose(out["p_count"], hs / (192.0 * n_acc), rtol=1e-15)
    nptest.assert_allclose(out["p_prevalence"], hv / (192.0 * n_acc), rtol=1e-15)
    nptest.assert_allclose(out["p_any"], 1.0 - hs[:, :, 0] / (192.0 * n_acc), rtol=1e-15)
    nptest.assert_allclose(out["p_none"], hv[:, 0] / (192.0 * n_acc), rtol=1e-15)
    nptest.assert_allclose(out["expected"], hs @ np.arange(11) / (192.0 * n_acc), rtol=1e-13)
    for (j, size) in enumerate(out["sizes"]):
        assert not hs[j, :, size + 1:].any()
    # the independent law of the same fit: the mean-field laws of its marginals (joint minus independent is the excess)
    check_independent(on.region_set_posterior(independent=True), on._lq_R, [sorted(s) for s in NETWORKS.values()], list(NETWORKS))
    # every sweep counted: the first moments are the marginals of _lq_R
    every1 = gibbs_fit(env, region_sets=NETWORKS, energy_every=1)
    p1 = np.exp(every1._lq_R[:, :, 1])
    want = np.stack([p1[sorted(s)].sum(axis=0) for s in NETWORKS.values()])
    nptest.assert_allclose(every1.region_set_posterior()["expected"], want, rtol=1e-12)
    assert every1.region_set_sweeps == 9
    early = gibbs_fit(env, region_sets=NETWORKS, n_sweeps=3)
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        early.region_set_posterior()
    with pytest.raises(ValueError):
        gibbs_fit(env, region_sets={"bad": [3, 10]})


def test_shared_fit_region_sets(env):
    """SharedRegionFit: patient extent 1; the set of all regions is its anomaly_count_posterior(), the vb path the mean field."""
    cls = env.pkg.fit.SharedRegionFit
    fit = gibbs_fit(env, cls=cls, region_sets=NETWORKS, anomaly_counts=True)
    out = fit.region_set_posterior()
    assert out["p_count"].shape == (5, 1, 11) and out["p_prevalence"].shape == (5, 2)
    nptest.assert_allclose(out["p_count"][0, 0], fit.anomaly_count_posterior()["p_count"], rtol=1e-15)
    nptest.assert_allclose(out["p_prevalence"][:, 1], out["p_any"][:, 0], rtol=1e-15)
    nptest.assert_allclose(out["p_any"][3, 0], fit.region_posterior()[4], rtol=1e-12)          # the singleton {4}
    fit.method = "vb"
    fit.max_iters = 3
    fit.run()
    check_independent(fit.region_set_posterior(), fit._lq_R, [sorted(s) for s in NETWORKS.values()], list(NETWORKS))
