"""
The decided-tile path of the pair-tile f pass (gibbs_f_pair_kernel<.., SURE>): a tile whose edges the tables decide
(fcd_f_edge_mode) draws no sums.  Every case runs the same calls with knob f_sure = 1 (the path off) and 0, compares chains,
marginal counters and pooled counts of both with the C oracle bit for bit, f_repeats of the two with each other, and the
counters f_sure_passes / f_sure_tiles / f_sure_fallbacks with what the NumPy restatement of the rule (tests/f_sure_ref.py)
and the oracle's Philox words predict on the CPU.  A "tile" of the counters is a workgroup: a pair-aligned tile x 16 chain
words.

Shapes: Nreg = 2 (one edge), 3 (a row pair without its second row), 5 (diagonal-only and empty tiles), 13, 18, 45 (short last
blocks, three blocks); U = 1, 3, 50, 64; G = 1, 65, 1100 (one wave, a partial chain word, two workgroups per tile).
"""
import os
import sys

import numpy as np
import numpy.testing as nptest
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_sure_ref as R  # noqa: E402

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


def tables_for(env, N, H, U, seed, weak=False):
    m = env.pkg.UnsharedRegionModel()
    if weak:        # broad components, two healthy subjects: no edge is decided
        m.sigma = np.array([0.2, 0.25, 0.3])
        m.mu = np.array([-0.05, 0.0, 0.05])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def f_hist(f):
    return np.stack([(f == k).sum(axis=0) for k in range(3)], axis=1).astype(np.int64)


STATS = ("f_repeats", "f_rec_passes", "f_sure_passes", "f_sure_tiles", "f_sure_fallbacks")


def stats(env):
    return np.array([env.ctx.stat(k) for k in STATS], dtype=np.int64)


class Call(object):
    """one fcd_gibbs_run call: its tables, gamma set before it (None: as it stands), sweeps, an M-step after every sweep?"""

    def __init__(self, S_B, lM, n, gamma=None, mstep=False):
        self.S_B, self.lM, self.n, self.gamma, self.mstep = S_B, lM, n, gamma, mstep


def prepare(env, eng, m, call, first):
    if not first:
        eng.S_B.copy_(up(env, call.S_B))
        eng.lM.copy_(up(env, call.lM))
        eng.refresh_tables()
    if call.gamma is not None:
        eng.set_hyper(call.gamma, m.pi2())
    return eng.hyper.cpu().numpy().copy()


def new_engine(env, m, call, N, U, G, seed, chain0):
    eng = env.GibbsEngine(up(env, call.S_B), up(env, call.lM), N, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    return eng


def run_case(env, m, N, U, G, seed, chain0, calls, after_call=None):
    """-> the rise of STATS under f_sure = 1 and under f_sure = 0, and the prediction (passes, tiles, fallbacks);
    after_call(knob f_sure, index of the call): called behind every call of both runs, to read the context's counters"""
    what = "N=%d U=%d G=%d" % (N, U, G)
    try:
        env.ctx.set_knob("f_records", 2)
        env.ctx.set_knob("f_sure", 1)
        # the oracle's chains and the hyper block of every sweep; with M-steps the device's own, from one-sweep calls
        ref = new_engine(env, m, calls[0], N, U, G, seed, chain0) if any(c.mstep for c in calls) else None
        hyp = new_engine(env, m, calls[0], N, U, G, seed, chain0) if ref is None else ref
        f_o, r_o = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
        cnt_f = np.zeros((f_o.shape[1], 3), dtype=np.int64)
        cnt_r = np.zeros((N, U), dtype=np.int64)
        (hs, sweep) = ([], 0)
        for (i, c) in enumerate(calls):
            h = prepare(env, hyp, m, c, i == 0)
            hc = []
            for s in range(sweep, sweep + c.n):
                hc.append(h)
                env.CO.gibbs_f_step(f_o, r_o, c.S_B, c.lM, h[0:3], seed, s, chain0)
                env.CO.gibbs_r_step(f_o, r_o, c.lM, h[3:5], seed, s, 1, chain0)
                cnt_f += f_hist(f_o)
                cnt_r += r_o.astype(np.int64).sum(axis=0)
                if c.mstep:
                    ref.run(s, 1, mstep_every=1)
                    h = ref.hyper.cpu().numpy().copy()
            hs.append(hc)
            sweep += c.n
        pred = np.zeros(3, dtype=np.int64)
        rise = {}
        for knob in (1, 0):
            env.ctx.set_knob("f_sure", knob)
            eng = new_engine(env, m, calls[0], N, U, G, seed, chain0)
            s0 = stats(env)
            sweep = 0
            for (i, c) in enumerate(calls):
                prepare(env, eng, m, c, i == 0)
                counts = eng.run(sweep, c.n, mstep_every=1 if c.mstep else 0, accumulate_from=0, want_counts=True).cpu().numpy().copy()
                if after_call is not None:
                    after_call(knob, i)
                if knob == 0:
                    later = [(sweep + j, hs[i][j][0:3]) for j in range(1, c.n)]      # (the first sweep of a call runs edge tiles)
                    pred += np.array(R.predict(N, U, G, chain0, seed, c.S_B, R.edge_table(c.lM), hs[i][0][0:3], later))
                sweep += c.n
            (f_g, r_g) = eng.export_state()
            assert env.ctx.stat("dev_err") == 0, what
            nptest.assert_array_equal(f_g, f_o, err_msg=what)
            nptest.assert_array_equal(r_g, r_o, err_msg=what)
            nptest.assert_array_equal(eng.cnt_f.cpu().numpy().astype(np.int64), cnt_f, err_msg=what)
            nptest.assert_array_equal(eng.cnt_r.cpu().numpy().astype(np.int64), cnt_r, err_msg=what)
            nptest.assert_array_equal(counts[:5], np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5], err_msg=what)
            rise[knob] = dict(zip(STATS, stats(env) - s0))
    finally:
        env.ctx.set_knob("f_records", 0)
        env.ctx.set_knob("f_sure", 0)
    n_pair = sum(c.n - 1 for c in calls)
    for knob in (1, 0):
        assert rise[knob]["f_rec_passes"] == n_pair, (what, rise)
    assert rise[0]["f_repeats"] == rise[1]["f_repeats"], (what, rise)
    assert (rise[1]["f_sure_passes"], rise[1]["f_sure_tiles"], rise[1]["f_sure_fallbacks"]) == (0, 0, 0), (what, rise)
    assert (rise[0]["f_sure_passes"], rise[0]["f_sure_tiles"], rise[0]["f_sure_fallbacks"]) == tuple(pred), (what, rise, pred)
    return rise[0], pred


NS = (2, 3, 5, 13, 18, 45)
US = (1, 3, 50, 64)
GS = (1, 65, 1100)
SHAPES = [(NS[i], US[j], GS[(i + j) % 3]) for i in range(6) for j in range(4)]


@pytest.mark.parametrize("N,U,G", SHAPES)
def test_decided_tables(env, N, U, G):
    """H = 16 controls: all or nearly all tiles decided"""
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=5 * N + U)
    (rise, pred) = run_case(env, m, N, U, G, 900 + 13 * N + U, 3, [Call(S_B, lM, 4)])
    assert pred[1] > 0


@pytest.mark.parametrize("U", (3, 7))
def test_mixed_tables(env, U):
    """H = 3: tiles of both kinds in one pass"""
    N = 13
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=7 * N + U)
    (rise, pred) = run_case(env, m, N, U, 130, 311 + U, 5, [Call(S_B, lM, 4)])
    n_tiles = sum(len(t) > 0 for t in R.tiles(N))
    assert 0 < pred[1] < 3 * n_tiles           # (three pair-tile passes, one workgroup per tile)


def test_weak_tables_run_the_kernel_without_the_path(env):
    (N, U, G) = (30, 8, 256)
    (m, S_B, lM) = tables_for(env, N, 2, U, seed=N + U, weak=True)
    (rise, pred) = run_case(env, m, N, U, G, 17, 0, [Call(S_B, lM, 4)])
    assert tuple(pred) == (0, 0, 0)
    assert (rise["f_sure_passes"], rise["f_rec_passes"], rise["f_sure_tiles"]) == (0, 3, 0)


@pytest.mark.parametrize("side", (+1, -1))
def test_an_edge_at_the_threshold(env, side):
    """one edge of an otherwise decided tile with its margin at T +- 1e-3: the tile is on the path / off it"""
    (N, U, G) = (13, 3, 65)
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=21)
    lng = np.log(m.gamma)
    (a, b) = R.edge_bounds(R.edge_table(lM))
    mode = R.edge_modes(S_B, lng, U, a, b)
    full = [t for t in R.decided_tiles(N, mode) if len(t) == 8]
    c = int(full[0][5])
    S_B2 = R.place_margin(S_B, c, int(mode[c]), lng, b, R.T + side * 1e-3)
    mode2 = R.edge_modes(S_B2, lng, U, a, b)
    assert (mode2[c] >= 0) == (side > 0) and (np.delete(mode2, c) == np.delete(mode, c)).all()
    tile_in = any(np.array_equal(t, full[0]) for t in R.decided_tiles(N, mode2))
    assert tile_in == (side > 0)
    run_case(env, m, N, U, G, 77, 1, [Call(S_B2, lM, 3)])


def test_rule_follows_the_m_steps(env):
    """mstep_every = 1 over six sweeps: every pass evaluates the rule at its own gamma"""
    (N, U, G) = (13, 7, 130)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=98)
    run_case(env, m, N, U, G, 5, 2, [Call(S_B, lM, 6, mstep=True)])


def test_set_hyper_between_calls_changes_the_modes(env):
    """gamma = (1e-40, 1, 1e-40), then (1, 1e-40, 1e-40): other edges decided, other modes (H = 3: 92 nats move them)"""
    (N, U, G) = (13, 3, 65)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=21)
    calls = [Call(S_B, lM, 3), Call(S_B, lM, 3, gamma=np.array([1e-40, 1.0, 1e-40])), Call(S_B, lM, 3, gamma=np.array([1.0, 1e-40, 1e-40]))]
    (a, b) = R.edge_bounds(R.edge_table(lM))
    modes = [R.edge_modes(S_B, np.log(g), U, a, b) for g in (m.gamma, calls[1].gamma, calls[2].gamma)]
    assert not np.array_equal(modes[0], modes[1]) and not np.array_equal(modes[1], modes[2])
    run_case(env, m, N, U, G, 31, 0, calls)


FALLBACK_SEED = 2


def test_vote_sends_tiles_back(env):
    """8 M draws: some lanes' uniforms lie outside fcd_draw_f_sure's range, and their workgroups run the sums"""
    (N, U, G) = (45, 16, 2048)
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=1)
    (rise, pred) = run_case(env, m, N, U, G, FALLBACK_SEED, 0, [Call(S_B, lM, 4)])
    assert pred[2] >= 3, pred


def test_f_tol_keeps_every_draw_on_the_exact_path(env):
    (N, U, G) = (18, 49, 65)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=11)
    try:
        env.ctx.set_knob("f_tol", 1e30)
        env.ctx.set_knob("f_records", 2)
        eng = new_engine(env, m, Call(S_B, lM, 4), N, U, G, 1234, 7)
        s0 = stats(env)
        eng.run(0, 4, mstep_every=0)
        rise = dict(zip(STATS, stats(env) - s0))
    finally:
        env.ctx.set_knob("f_tol", 0.0)
        env.ctx.set_knob("f_records", 0)
    wave_edges = ((G + 63) // 64) * (N * (N - 1) // 2)
    assert rise["f_repeats"] == 4 * wave_edges
    assert (rise["f_rec_passes"], rise["f_sure_passes"], rise["f_sure_tiles"], rise["f_sure_fallbacks"]) == (3, 0, 0, 0)


def test_tables_changed_in_place_between_calls(env):
    """the second call's bounds are those of the tables it finds behind the same pointers"""
    (N, U, G) = (13, 7, 130)
    (m, S_B1, lM1) = tables_for(env, N, 3, U, seed=3)
    (_m, S_B2, lM2) = tables_for(env, N, 16, U, seed=4)
    (p1, p2) = [R.predict(N, U, G, 2, 99, S, R.edge_table(L), np.log(m.gamma), [(1, np.log(m.gamma))])[1] for (S, L) in ((S_B1, lM1), (S_B2, lM2))]
    assert p1 != p2
    run_case(env, m, N, U, G, 99, 2, [Call(S_B1, lM1, 3), Call(S_B2, lM2, 3)])
