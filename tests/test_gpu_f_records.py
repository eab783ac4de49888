"""
The pair-tile f pass on pair records made once per fcd_gibbs_run call (knob f_records, gibbs_f_records_kernel) against the
same pass building its records in every tile, and both against the C oracle, bit for bit.

Shapes of the path comparison: the smallest at which the copy of a tile's records, the tile geometry or the last pair can go
wrong -- Nreg = 2 (one edge), 3 (a row pair without its second row), 5 (diagonal-only tiles), 13, 18 and 45 (last blocks of
13 and 2 regions, three blocks); U = 1, 2, 3, 49, 50, 63, 64 (an odd U has a last pair without a second patient, 64 fills four
slot words); G = 1, 64, 65, 1000, 1100 (fewer waves than edges, a partial chain word, more than 16 chain words).

A record must not outlive its call: test_tables_changed_in_place_between_calls overwrites the tables behind the same
pointers between two calls.
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


def tables_for(env, N, H, U, seed, weak=False):
    m = env.pkg.UnsharedRegionModel()
    if weak:        # broad components, two healthy subjects: the three types stay comparable and the fp32 margin bites
        m.sigma = np.array([0.2, 0.25, 0.3])
        m.mu = np.array([-0.05, 0.0, 0.05])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def f_hist(f):
    """(G, C) states -> (C, 3) counts over the chains"""
    return np.stack([(f == k).sum(axis=0) for k in range(3)], axis=1).astype(np.int64)


N_SWEEPS, BURN = 4, 1
NS = (2, 3, 5, 13, 18, 45)
US = (1, 2, 3, 49, 50, 63, 64)
GS = (1, 64, 65, 1000, 1100)
# every (N, U) pair once; a row of it meets 7 and a column 6 consecutive G indices mod 5: every (N, G) and (U, G) pair too
SHAPES = [(NS[i], US[j], GS[(i + j) % 5]) for i in range(6) for j in range(7)]


class Oracle(object):
    """the oracle's chains, sweep by sweep, with the counters of the sweeps from `burn` on"""

    def __init__(self, env, m, N, U, G, seed, chain0, burn):
        self.env, self.N, self.seed, self.chain0, self.burn = env, N, seed, chain0, burn
        self.lng, self.lnpi2 = np.log(m.gamma), np.log(m.pi2())
        self.f, self.r = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
        self.cnt_f = np.zeros((self.f.shape[1], 3), dtype=np.int64)
        self.cnt_r = np.zeros((N, U), dtype=np.int64)
        self.sweep = 0

    def run(self, n, S_B, lM):
        CO = self.env.CO
        for s in range(self.sweep, self.sweep + n):
            CO.gibbs_f_step(self.f, self.r, S_B, lM, self.lng, self.seed, s, self.chain0)
            CO.gibbs_r_step(self.f, self.r, lM, self.lnpi2, self.seed, s, 1, self.chain0)
            if s >= self.burn:
                self.cnt_f += f_hist(self.f)
                self.cnt_r += self.r.astype(np.int64).sum(axis=0)
        self.sweep += n


def assert_equals_oracle(env, eng, counts, o, what):
    (f_g, r_g) = eng.export_state()
    assert env.ctx.stat("dev_err") == 0, what
    nptest.assert_array_equal(f_g, o.f, err_msg=what)
    nptest.assert_array_equal(r_g, o.r, err_msg=what)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy().astype(np.int64), o.cnt_f, err_msg=what)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy().astype(np.int64), o.cnt_r, err_msg=what)
    nptest.assert_array_equal(counts[:5], np.asarray(env.CO.gibbs_stats(o.f, o.r))[:5], err_msg=what)


def both_paths(env, m, S_B, lM, N, U, G, seed, chain0):
    """N_SWEEPS sweeps in one run() call with f_records = 2 and with f_records = 1: both the oracle's; -> f_repeats of each"""
    o = Oracle(env, m, N, U, G, seed, chain0, BURN)
    o.run(N_SWEEPS, S_B, lM)
    reps = {}
    try:
        for knob in (2, 1):
            env.ctx.set_knob("f_records", knob)
            eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
            eng.set_hyper(m.gamma, m.pi2())
            eng.init(0.3)
            (p0, b0, r0) = (env.ctx.stat("f_rec_passes"), env.ctx.stat("f_rec_builds"), env.ctx.stat("f_repeats"))
            counts = eng.run(0, N_SWEEPS, mstep_every=0, accumulate_from=BURN, want_counts=True).cpu().numpy().copy()
            what = "N=%d U=%d G=%d f_records=%d" % (N, U, G, knob)
            assert_equals_oracle(env, eng, counts, o, what)
            reps[knob] = env.ctx.stat("f_repeats") - r0
            # every sweep of the call but the first is a pair-tile sweep
            assert env.ctx.stat("f_rec_passes") - p0 == (N_SWEEPS - 1 if knob == 2 else 0), what
            assert env.ctx.stat("f_rec_builds") - b0 == (1 if knob == 2 else 0), what
    finally:
        env.ctx.set_knob("f_records", 0)
    assert reps[2] == reps[1], (N, U, G, reps)
    return reps[1]


@pytest.mark.parametrize("N,U,G", SHAPES)
def test_paths_agree(env, N, U, G):
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=7 * N + U)
    both_paths(env, m, S_B, lM, N, U, G, seed=311 + 17 * N + U, chain0=5)


def test_exact_path_on_weak_tables(env):
    """
    Weak tables: the fp32 sums cannot decide some draws and the edge is repeated in fp64 from lMf in memory -- the same waves
    on both paths (both_paths compares the two counts), and some of them: the kernel that builds its records per tile
    repeats 26 (edge, chain word) items in these four sweeps.
    """
    (N, U, G) = (30, 8, 256)
    (m, S_B, lM) = tables_for(env, N, 2, U, seed=N + U, weak=True)
    reps = both_paths(env, m, S_B, lM, N, U, G, seed=17, chain0=0)
    print("f_repeats on weak tables, %d sweeps: %d" % (N_SWEEPS, reps))
    assert reps == 26


def test_every_draw_on_the_exact_path(env):
    """f_tol = 1e30: every (edge, chain word) of every sweep repeats, on both paths."""
    (N, U, G) = (18, 49, 65)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=11)
    try:
        env.ctx.set_knob("f_tol", 1e30)
        reps = both_paths(env, m, S_B, lM, N, U, G, seed=1234, chain0=7)
    finally:
        env.ctx.set_knob("f_tol", 0.0)
    wave_edges = ((G + 63) // 64) * (N * (N - 1) // 2)
    # the first sweep of the call (edge tiles) and the N_SWEEPS - 1 pair-tile sweeps
    assert reps - wave_edges == wave_edges * (N_SWEEPS - 1)


def test_tables_changed_in_place_between_calls(env):
    """
    Call A, three sweeps; then S_B and lM are overwritten with another data set's tables -- same buffers, same pointers -- and
    refresh_tables() re-derives lMf and lMd in place; call B, three sweeps.  The records of call A describe tables that no
    longer exist: call B must make its own.
    """
    (N, U, G) = (13, 7, 130)
    (m, S_B1, lM1) = tables_for(env, N, 3, U, seed=3)
    (_m, S_B2, lM2) = tables_for(env, N, 3, U, seed=4)
    assert not np.array_equal(lM1, lM2)
    o = Oracle(env, m, N, U, G, 99, 2, burn=0)
    o.run(3, S_B1, lM1)
    o.run(3, S_B2, lM2)
    try:
        env.ctx.set_knob("f_records", 2)
        eng = env.GibbsEngine(up(env, S_B1), up(env, lM1), N, U, G, chain0=2, seed=99, ctx=env.ctx)
        eng.set_hyper(m.gamma, m.pi2())
        eng.init(0.3)
        p0 = env.ctx.stat("f_rec_passes")
        eng.run(0, 3, mstep_every=0, accumulate_from=0)
        ptrs = (eng.S_B.data_ptr(), eng.lM.data_ptr(), eng.lMf.data_ptr(), eng.lMd.data_ptr())
        eng.S_B.copy_(up(env, S_B2))
        eng.lM.copy_(up(env, lM2))
        eng.refresh_tables()
        assert ptrs == (eng.S_B.data_ptr(), eng.lM.data_ptr(), eng.lMf.data_ptr(), eng.lMd.data_ptr())
        counts = eng.run(3, 3, mstep_every=0, accumulate_from=0, want_counts=True).cpu().numpy().copy()
        assert env.ctx.stat("f_rec_passes") - p0 == 4
    finally:
        env.ctx.set_knob("f_records", 0)
    assert_equals_oracle(env, eng, counts, o, "tables switched between calls")


def test_rule_builds_only_for_calls_with_enough_pair_tile_sweeps(env):
    """f_records = 0: a build for a call of at least F_REC_MIN_SWEEPS pair-tile sweeps (its sweeps but the first), else none."""
    (N, U, G) = (13, 3, 64)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=1)
    k = env.ctx.stat("f_rec_min_sweeps")
    assert k >= 2
    env.ctx.set_knob("f_records", 0)
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=5, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    (b0, p0) = (env.ctx.stat("f_rec_builds"), env.ctx.stat("f_rec_passes"))
    eng.run(0, k, mstep_every=0)                     # k - 1 pair-tile sweeps
    assert (env.ctx.stat("f_rec_builds") - b0, env.ctx.stat("f_rec_passes") - p0) == (0, 0)
    eng.run(k, k + 1, mstep_every=0)                 # k pair-tile sweeps
    assert (env.ctx.stat("f_rec_builds") - b0, env.ctx.stat("f_rec_passes") - p0) == (1, k)
    for s in range(2 * k + 1, 2 * k + 4):
        eng.sweeps(s, 1)
        eng.f_step(s)
    assert (env.ctx.stat("f_rec_builds") - b0, env.ctx.stat("f_rec_passes") - p0) == (1, k)
    assert env.ctx.stat("dev_err") == 0


def test_reserve_covers_the_record_table(env):
    """fcd_ctx_reserve (GibbsEngine.__init__) sizes the record table: a forced run on a fresh context allocates nothing."""
    (N, U, G) = (18, 5, 70)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=2)
    fresh = env.lib.Context()
    eng = env.GibbsEngine(up(env, S_B), up(env, lM), N, U, G, seed=7, ctx=fresh)
    n_alloc = fresh.stat("n_alloc")
    assert fresh.stat("f_rec_bytes") > 0
    fresh.set_knob("f_records", 2)
    eng.set_hyper(m.gamma, m.pi2())
    eng.init(0.3)
    p0 = fresh.stat("f_rec_passes")
    eng.run(0, 3, mstep_every=1, accumulate_from=1, want_counts=True)
    env.torch.cuda.synchronize()
    assert fresh.stat("f_rec_passes") - p0 == 2
    assert fresh.stat("n_alloc") == n_alloc
    fresh.check_device()
