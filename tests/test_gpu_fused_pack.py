"""
The sweep without the r pass's packing launch: from the second sweep of a fcd_gibbs_run call on, the U <= 64 f pass works
in pair-aligned tiles and writes the r pass's packed f words itself, and the tally of the sweep before has written the r
words and cleared the marks.  Knob f_pack = 1 keeps the packing launch in every sweep.  Both must walk the C oracle's
chains bit for bit, and the default must not launch the packing kernel after the first sweep of a call.
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


N_SWEEPS = 5
CALLS = {"one call": [(0, N_SWEEPS)], "several calls": [(0, 2), (2, 1), (3, 2)]}

SHAPES = [(N, U, G) for N in (2, 3, 16, 17, 33) for U in (1, 7, 50, 64) for G in (70,)] + \
         [(200, 50, 130), (200, 64, 70), (200, 7, 100), (200, 1, 70)]


@pytest.mark.parametrize("N,U,G", SHAPES)
def test_packed_sweeps_equal_oracle(env, N, U, G):
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=3 * N + U)
    seed = 4242 + N * 100 + U
    chain0 = 5
    lng, lnpi2 = np.log(m.gamma), np.log(m.pi2())
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    for s in range(N_SWEEPS):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, lng, seed, s, chain0)
        env.CO.gibbs_r_step(f_o, r_o, lM, lnpi2, seed, s, 1, chain0)
    try:
        for f_pack in (0, 1):
            env.ctx.set_knob("f_pack", f_pack)
            for (name, calls) in CALLS.items():
                eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
                eng.set_hyper(m.gamma, m.pi2())
                eng.init(0.3)
                n0 = env.ctx.stat("pack_launches")
                for (s0, n) in calls:
                    eng.run(s0, n, mstep_every=0)
                (f_g, r_g) = eng.export_state()
                what = "f_pack=%d, %s" % (f_pack, name)
                assert env.ctx.stat("dev_err") == 0, what
                nptest.assert_array_equal(f_g, f_o, err_msg=what)
                nptest.assert_array_equal(r_g, r_o, err_msg=what)
                # the packing launch: in every sweep with f_pack = 1, else in the first sweep of each call only
                want = N_SWEEPS if f_pack == 1 else len(calls)
                assert env.ctx.stat("pack_launches") - n0 == want, what
    finally:
        env.ctx.set_knob("f_pack", 0)


@pytest.mark.parametrize("N,U,G", [(45, 7, 200), (33, 7, 1100), (200, 50, 1024)])
def test_packed_sweeps_keep_counts_and_mstep(env, N, U, G):
    """M-step, marginal counters and pooled counts: the default path (the f counts in the tally after the pass) and
    f_pack = 1 (the f counts in the packing launch) agree exactly, as do the chains."""
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    out = []
    try:
        for f_pack in (0, 1):
            env.ctx.set_knob("f_pack", f_pack)
            eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=64, seed=99, ctx=env.ctx)
            eng.set_hyper(m.gamma, m.pi2())
            eng.init(0.25)
            counts = eng.run(0, 6, mstep_every=2, accumulate_from=2, want_counts=True).cpu().numpy().copy()
            (f, r) = eng.export_state()
            out.append((f, r, eng.hyper.cpu().numpy().copy(), eng.cnt_f.cpu().numpy().copy(), eng.cnt_r.cpu().numpy().copy(),
                        counts))
    finally:
        env.ctx.set_knob("f_pack", 0)
    for (a, b_) in zip(out[0], out[1]):
        nptest.assert_array_equal(a, b_)
    assert out[0][5][4] == G
