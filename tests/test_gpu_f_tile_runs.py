"""
Several sweeps in ONE fcd_gibbs_run call, at shapes where the f pass's pair tiles and the tally's rounds are cut short: a
number of regions that is no multiple of 16 or of 8, a last block of 2, 4 and 6 regions, U = 1, 2, 49, 50, 64 patients,
and G = 64, 65, 1000, 1024 chains plus one G above 1024 (more than 16 chain words: the tally then loops over groups of
words).  From the second sweep of the call on the pair-tile f pass is the one that runs; the default path counts the f
states in the tally after the sweep, f_pack = 1 counts them in the packing launch (four-wave workgroups).

Both paths must walk the C oracle's chains bit for bit, and the marginal counters cnt_f / cnt_r and the pooled counts are
required to equal what NumPy counts in the oracle's chains -- not only each other.  (The packed f words f_S have no
read-back in the ABI: the r pass reads f through them and nothing else, so r equal to the oracle's over several sweeps is
what checks them.)
"""
import numpy as np
import numpy.testing as nptest
import pytest


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO = torch, fcdiff_amd, _lib, GibbsEngine, CO
    e.ctx = _lib.Context()
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def tables_for(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def f_hist(f):
    """(G, C) states -> (C, 3) counts over the chains"""
    return np.stack([(f == k).sum(axis=0) for k in range(3)], axis=1).astype(np.int64)


N_SWEEPS, BURN = 4, 1
# 13: no multiple of 8, one block; 18, 20, 22: a last block of 2, 4, 6 regions; 45: three blocks, odd
NS = (13, 18, 20, 22, 45)
US = (1, 2, 49, 50, 64)
GS = (64, 65, 1000, 1024, 1100)
# every (N, U), (N, G) and (U, G) pair once
SHAPES = [(NS[i], US[j], GS[(i + j) % 5]) for i in range(5) for j in range(5)]


def oracle_run(env, m, S_B, lM, N, U, G, seed, chain0):
    """the oracle's chains after N_SWEEPS sweeps, and the counters of the sweeps from BURN on"""
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    cnt_f = np.zeros((f_o.shape[1], 3), dtype=np.int64)
    cnt_r = np.zeros((N, U), dtype=np.int64)
    for s in range(N_SWEEPS):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, chain0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, 1, chain0)
        if s >= BURN:
            cnt_f += f_hist(f_o)
            cnt_r += r_o.astype(np.int64).sum(axis=0)
    return f_o, r_o, cnt_f, cnt_r


def gpu_run(env, m, S_B, lM, N, U, G, seed, chain0, f_pack):
    env.ctx.set_knob("f_pack", f_pack)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    n0 = env.ctx.stat("pack_launches")
    counts = eng.run(0, N_SWEEPS, mstep_every=0, accumulate_from=BURN, want_counts=True).cpu().numpy().copy()
    (f_g, r_g) = eng.export_state()
    assert env.ctx.stat("dev_err") == 0
    return f_g, r_g, eng.cnt_f.cpu().numpy().astype(np.int64), eng.cnt_r.cpu().numpy().astype(np.int64), counts, \
        env.ctx.stat("pack_launches") - n0


def check_against_oracle(env, m, S_B, lM, N, U, G, seed, chain0):
    (f_o, r_o, cf_o, cr_o) = oracle_run(env, m, S_B, lM, N, U, G, seed, chain0)
    pooled = np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5]
    assert (cf_o.sum(axis=1) == (N_SWEEPS - BURN) * G).all()
    try:
        for f_pack in (0, 1):
            (f_g, r_g, cf_g, cr_g, counts, n_pack) = gpu_run(env, m, S_B, lM, N, U, G, seed, chain0, f_pack)
            what = "N=%d U=%d G=%d f_pack=%d" % (N, U, G, f_pack)
            nptest.assert_array_equal(f_g, f_o, err_msg=what)
            nptest.assert_array_equal(r_g, r_o, err_msg=what)
            nptest.assert_array_equal(cf_g, cf_o, err_msg=what)
            nptest.assert_array_equal(cr_g, cr_o, err_msg=what)
            nptest.assert_array_equal(counts[:5], pooled, err_msg=what)
            assert counts[5:].sum() == 0, what
            # the packing launch: in every sweep with f_pack = 1, else in the first sweep of the call only
            assert n_pack == (N_SWEEPS if f_pack == 1 else 1), what
    finally:
        env.ctx.set_knob("f_pack", 0)


@pytest.mark.parametrize("N,U,G", SHAPES)
def test_cut_short_shapes_equal_oracle(env, N, U, G):
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=5 * N + U)
    check_against_oracle(env, m, S_B, lM, N, U, G, seed=977 + 31 * N + U, chain0=3)


def test_every_draw_on_the_exact_path(env):
    """f_tol = 1e30: every f draw is re-decided on the exact path, whatever Philox block it took its number from."""
    (N, U, G) = (22, 49, 65)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=11)
    r0 = env.ctx.stat("f_repeats")
    try:
        env.ctx.set_knob("f_tol", 1e30)
        check_against_oracle(env, m, S_B, lM, N, U, G, seed=1234, chain0=7)
    finally:
        env.ctx.set_knob("f_tol", 0.0)
    # every (edge, chain word) of every sweep, on both paths
    assert env.ctx.stat("f_repeats") - r0 == 2 * N_SWEEPS * ((G + 63) // 64) * (N * (N - 1) // 2)


@pytest.mark.parametrize("N,U,G", [(200, 50, 1024), (45, 7, 2100)])
def test_counters_equal_the_state_they_count(env, N, U, G):
    """
    The bench's shape (every wave of the tally has one round of four edges, 16 chain words) and one with 33 chain words
    (three groups of words, the last of one word): with the counters fed by the LAST sweep alone they must be the histogram
    of the exported state, on both paths; chains, counters, pooled counts and the M-step's result must agree between the
    paths.
    """
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    out = []
    try:
        for f_pack in (0, 1):
            env.ctx.set_knob("f_pack", f_pack)
            eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=64, seed=99, ctx=env.ctx)
            eng.set_hyper(m.gamma, m.pi2())
            eng.init(0.25)
            counts = eng.run(0, 4, mstep_every=2, accumulate_from=3, want_counts=True).cpu().numpy().copy()
            (f, r) = eng.export_state()
            cnt_f = eng.cnt_f.cpu().numpy().astype(np.int64)
            cnt_r = eng.cnt_r.cpu().numpy().astype(np.int64)
            what = "f_pack=%d" % f_pack
            nptest.assert_array_equal(cnt_f, f_hist(f), err_msg=what)
            nptest.assert_array_equal(cnt_r, r.astype(np.int64).sum(axis=0), err_msg=what)
            nptest.assert_array_equal(counts[:5], np.asarray(env.CO.gibbs_stats(f, r))[:5], err_msg=what)
            out.append((f, r, eng.hyper.cpu().numpy().copy(), cnt_f, cnt_r, counts))
    finally:
        env.ctx.set_knob("f_pack", 0)
    for (a, b_) in zip(out[0], out[1]):
        nptest.assert_array_equal(a, b_)
