"""
The f half of the sweep's tally inside the pipelined r pass (knob tally_in_r, stat tally_f_in_r), the r-word buffers that
swap roles from sweep to sweep (knob r_keep_words) and the tally that is left: slot words, cleared marks, r counts.

From the second sweep of a fcd_gibbs_run call on there is no packing launch to carry the f half, so the in-order workgroups
of the pipelined pass count f before their first block -- once per launch, whatever the number of chain-word groups --
where they have 16 waves (G >= 961) and a wave's rounds R = ceil(C / (64 nD)) * ceil(GW / 16) are at most
tally_in_r_max_rounds.  Shapes are the smallest at which each piece can go wrong: one block of regions, a last block of 6,
three blocks; nD = 2, 4, 14 in-order workgroups (at Nreg 13 most waves meet no edge, at Nreg 45 / U 1 a wave walks 8 rounds
or more: over the limit, only knob 2 rides); a partial last chain word, exactly 16 words, 18 words (two groups); and G = 64
and 577, whose in-order workgroups are short: nothing rides there and the tally after the pass counts f.

Every case goes against the C oracle's chains and NumPy counts of those chains.  With an M-step in every sweep the oracle
takes each sweep's hyper block from one-sweep calls of the parent's path (tally_in_r = 1, r_keep_words = 1) whose chains
are the oracle's and whose block is checked against the oracle's M-step of those chains; the hyper block after the
four-sweep call must then be the same bytes under every knob setting.
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
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO, e.O = torch, fcdiff_amd, _lib, GibbsEngine, CO, O
    e.ctx = _lib.Context()
    e.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    e.r_max = e.ctx.stat("tally_in_r_max_rounds")
    return e


KNOBS = ("tally_in_r", "r_keep_words", "r_coop")


@pytest.fixture
def knobs(env):
    def set_(**kw):
        for (k, v) in kw.items():
            env.ctx.set_knob(k, v)
    yield set_
    for k in KNOBS:
        env.ctx.set_knob(k, 0)


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


def cdiv(a, b):
    return -(-a // b)


def rounds(env, N, U, G):
    """-> (16-wave in-order workgroups?, rounds per wave of the f half) as fcd_gibbs_r_pass works them out"""
    GW = cdiv(G, 64)
    wpb = min(GW, 16)
    nD = 2 * U if (wpb > 8 and 2 * U <= env.n_cu) else U
    return wpb == 16, cdiv(N * (N - 1) // 2, 64 * nD) * cdiv(GW, 16)


def rides(env, N, U, G, knob):
    (full, R) = rounds(env, N, U, G)
    return full and knob != 1 and (knob == 2 or R <= env.r_max)


N_SWEEPS, BURN = 4, 1
NS = (13, 22, 45)
US = (1, 2, 7)
GS = (1000, 1024, 1100)
# every (N, U), (N, G) and (U, G) pair once, then the two shapes with short in-order workgroups
SHAPES = [(NS[i], US[j], GS[(i + j) % 3]) for i in range(3) for j in range(3)] + [(22, 2, 64), (22, 7, 577)]


def new_engine(env, m, S_B, lM, N, U, G, seed, chain0):
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    return eng


def oracle_run(env, knobs, m, S_B, lM, N, U, G, seed, chain0, mstep):
    """
    The oracle's chains after N_SWEEPS sweeps, the counters of the sweeps from BURN on and the hyper block at the end.
    mstep: an M-step after every sweep -- the device's own, from one-sweep calls of the parent's path, checked here.
    """
    knobs(tally_in_r=1, r_keep_words=1)
    ref = new_engine(env, m, S_B, lM, N, U, G, seed, chain0)
    h = ref.hyper.cpu().numpy().copy()
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    cnt_f = np.zeros((f_o.shape[1], 3), dtype=np.int64)
    cnt_r = np.zeros((N, U), dtype=np.int64)
    for s in range(N_SWEEPS):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, h[0:3], seed, s, chain0)
        env.CO.gibbs_r_step(f_o, r_o, lM, h[3:5], seed, s, 1, chain0)
        if mstep:
            ref.run(s, 1, mstep_every=1)
            (f_g, r_g) = ref.export_state()
            assert np.array_equal(f_g, f_o) and np.array_equal(r_g, r_o), "one-sweep calls left the oracle's chains"
            h = ref.hyper.cpu().numpy().copy()
            (pi_h, gamma_h) = env.O.gibbs_mstep(np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5], N, U)
            nptest.assert_allclose(h[0:3], np.log(gamma_h), rtol=1e-14, atol=0)
            nptest.assert_allclose(h[3:5], [np.log(1.0 - pi_h), np.log(pi_h)], rtol=1e-14, atol=0)
        if s >= BURN:
            cnt_f += f_hist(f_o)
            cnt_r += r_o.astype(np.int64).sum(axis=0)
    knobs(tally_in_r=0, r_keep_words=0)
    return f_o, r_o, cnt_f, cnt_r, h


def gpu_run(env, m, S_B, lM, N, U, G, seed, chain0, mstep):
    """one four-sweep call -> state, counters, counts, hyper bytes, stats that rose, form of the last r pass"""
    eng = new_engine(env, m, S_B, lM, N, U, G, seed, chain0)
    (n_pack, n_in_r) = (env.ctx.stat("pack_launches"), env.ctx.stat("tally_f_in_r"))
    counts = eng.run(0, N_SWEEPS, mstep_every=1 if mstep else 0, accumulate_from=BURN, want_counts=True).cpu().numpy().copy()
    (f_g, r_g) = eng.export_state()
    assert env.ctx.stat("dev_err") == 0
    return dict(f=f_g, r=r_g, cnt_f=eng.cnt_f.cpu().numpy().astype(np.int64), cnt_r=eng.cnt_r.cpu().numpy().astype(np.int64),
                counts=counts, hyper=eng.hyper.cpu().numpy().tobytes(), n_pack=env.ctx.stat("pack_launches") - n_pack,
                n_in_r=env.ctx.stat("tally_f_in_r") - n_in_r, form=env.ctx.stat("r_form_last"))


def assert_oracle(env, got, f_o, r_o, cf_o, cr_o, what):
    nptest.assert_array_equal(got["f"], f_o, err_msg=what)
    nptest.assert_array_equal(got["r"], r_o, err_msg=what)
    nptest.assert_array_equal(got["cnt_f"], cf_o, err_msg=what)
    nptest.assert_array_equal(got["cnt_r"], cr_o, err_msg=what)
    nptest.assert_array_equal(got["counts"][:5], np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5], err_msg=what)
    assert got["counts"][5:].sum() == 0, what


@pytest.mark.parametrize("mstep", (0, 1))
@pytest.mark.parametrize("N,U,G", SHAPES)
def test_every_knob_setting_equals_oracle(env, knobs, N, U, G, mstep):
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=5 * N + U)
    (seed, chain0) = (977 + 31 * N + U, 3)
    (f_o, r_o, cf_o, cr_o, h_o) = oracle_run(env, knobs, m, S_B, lM, N, U, G, seed, chain0, mstep)
    assert (cf_o.sum(axis=1) == (N_SWEEPS - BURN) * G).all()
    hypers = set()
    for in_r in (0, 1, 2):
        for keep in (0, 1):
            knobs(tally_in_r=in_r, r_keep_words=keep)
            got = gpu_run(env, m, S_B, lM, N, U, G, seed, chain0, mstep)
            what = "N=%d U=%d G=%d mstep=%d tally_in_r=%d r_keep_words=%d" % (N, U, G, mstep, in_r, keep)
            assert_oracle(env, got, f_o, r_o, cf_o, cr_o, what)
            assert got["form"] == 2, what
            # sweeps 1 .. 3 want counts and have no packing launch; sweep 0's f half (M-step) rides in the packing launch
            assert got["n_in_r"] == ((N_SWEEPS - 1) if rides(env, N, U, G, in_r) else 0), what
            assert got["n_pack"] == 1, what
            hypers.add(got["hyper"])
    assert hypers == {h_o.tobytes()}


def test_rule_of_the_default(env):
    """What the shapes above are chosen for, with the library's own constant."""
    assert env.r_max >= 1
    assert rounds(env, 45, 1, 1100) == (True, 16) and not rides(env, 45, 1, 1100, 0) and rides(env, 45, 1, 1100, 2)
    assert rounds(env, 45, 1, 1024)[1] == 8 and rounds(env, 200, 50, 1024) == (True, 4)
    assert rounds(env, 200, 8, 1024) == (True, 20)
    assert not rounds(env, 22, 2, 64)[0] and not rounds(env, 22, 7, 577)[0]
    assert not any(rides(env, 22, 7, 577, k) for k in (0, 1, 2))


def test_refused_launch_counts_once(env, knobs):
    """
    r_coop = 2 with tally_in_r = 2: every pipelined launch is refused, the step form runs and the f half must be counted
    exactly once per sweep, by the launches that do run.  (After a step-form pass the next sweep needs its sentinels again,
    so under the hook every sweep has a packing launch, which carries the f half: the pass never gets to ask for it.)
    """
    (N, U, G) = (22, 2, 1024)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=5 * N + U)
    (seed, chain0) = (4242, 3)
    (f_o, r_o, cf_o, cr_o, _h) = oracle_run(env, knobs, m, S_B, lM, N, U, G, seed, chain0, 0)
    knobs(tally_in_r=2, r_coop=2)
    got = gpu_run(env, m, S_B, lM, N, U, G, seed, chain0, 0)
    assert_oracle(env, got, f_o, r_o, cf_o, cr_o, "refused launch")
    assert got["form"] == 1
    assert got["n_in_r"] == 0


@pytest.mark.parametrize("N,U,G", [(45, 7, 1024), (22, 2, 1000)])
def test_buffers_swap_inside_a_call_only(env, knobs, N, U, G):
    """Calls of 3, 2 and 1 sweeps on one engine (odd, even, no swap at all): every call starts from the same assignment."""
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    (seed, chain0) = (31 + N, 64)
    knobs(tally_in_r=2)
    eng = new_engine(env, m, S_B, lM, N, U, G, seed, chain0)
    h = eng.hyper.cpu().numpy().copy()
    f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    s0 = 0
    for n in (3, 2, 1):
        for s in range(s0, s0 + n):
            env.CO.gibbs_f_step(f_o, r_o, S_B, lM, h[0:3], seed, s, chain0)
            env.CO.gibbs_r_step(f_o, r_o, lM, h[3:5], seed, s, 1, chain0)
        eng.run(s0, n, mstep_every=0)
        s0 += n
        (f_g, r_g) = eng.export_state()
        nptest.assert_array_equal(f_g, f_o, err_msg="f after %d sweeps" % s0)
        nptest.assert_array_equal(r_g, r_o, err_msg="r after %d sweeps" % s0)
        assert env.ctx.stat("r_form_last") == 2 and env.ctx.stat("dev_err") == 0


def test_flagship_shape_counters_equal_the_state(env, knobs):
    """
    cfg3's own shape (R = 4: the default rides), counters fed by the last sweep alone: they are the histogram of the
    exported state, and chains, counters, counts and the M-step's result agree with the parent's path.
    """
    (N, U, G) = (200, 50, 1024)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=N + U)
    out = []
    for (in_r, keep) in ((0, 0), (1, 1)):
        knobs(tally_in_r=in_r, r_keep_words=keep)
        eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=64, seed=99, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.25)
        n0 = env.ctx.stat("tally_f_in_r")
        counts = eng.run(0, 4, mstep_every=2, accumulate_from=3, want_counts=True).cpu().numpy().copy()
        (f, r) = eng.export_state()
        cnt_f = eng.cnt_f.cpu().numpy().astype(np.int64)
        cnt_r = eng.cnt_r.cpu().numpy().astype(np.int64)
        what = "tally_in_r=%d r_keep_words=%d" % (in_r, keep)
        assert env.ctx.stat("dev_err") == 0 and env.ctx.stat("r_form_last") == 2, what
        # sweeps 1 and 3 have an M-step (3 also the counters and the counts); sweep 0 wants no f counts
        assert env.ctx.stat("tally_f_in_r") - n0 == (2 if in_r == 0 else 0), what
        nptest.assert_array_equal(cnt_f, f_hist(f), err_msg=what)
        nptest.assert_array_equal(cnt_r, r.astype(np.int64).sum(axis=0), err_msg=what)
        nptest.assert_array_equal(counts[:5], np.asarray(env.CO.gibbs_stats(f, r))[:5], err_msg=what)
        out.append((f, r, eng.hyper.cpu().numpy().copy(), cnt_f, cnt_r, counts))
    for (a, b_) in zip(out[0], out[1]):
        nptest.assert_array_equal(a, b_)
