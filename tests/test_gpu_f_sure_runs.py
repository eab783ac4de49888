"""
The run form of the f pass's decided path (gibbs_f_run_kernel, knob f_runs): one wave per (block-wide run of up to four
pair-aligned tiles, chain word) writes the modes of the decided edges and draws by itself the edges that the rule leaves open
or for which one of its lanes' uniforms is out of fcd_draw_f_sure's range.  Every case goes through run_case of
tests/test_gpu_f_sure_tiles.py: chains, marginal counters and pooled counts against the C oracle bit for bit, f_repeats against
the f_sure = 1 run, the three counters against the CPU's prediction (tests/f_sure_ref.py) -- and asserts through f_run_passes
which form ran.

Decided tables: H = 16 controls as in the per-tile tests; at U = 50 and 64 with Nreg >= 17 sixteen controls leave 4 - 117 of
the edges open at the hint (counted on the CPU for six seeds each), so those cases take H = 32, where none is.  Each case
asserts on the CPU that every tile of its table is decided at the hint -- the auto choice would otherwise run the per-tile kernel
and the case pass vacuously.

Shapes: Nreg = 2, 3, 5 (runs of one tile, a diagonal-only tile, a missing second row), 17, 18 (a second block of one or two
columns: a run that is one partial tile), 33, 34, 45 (three blocks; odd Nreg: a last row pair without its second row);
U = 1, 3, 50, 64; G = 1, 65, 1100 (one wave, a partial chain word, two groups per run).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_sure_ref as R  # noqa: E402
from test_gpu_f_sure_tiles import Call, env, new_engine, run_case, stats, tables_for, STATS  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def all_decided_at_hint(m, S_B, lM, U):
    (a, b) = R.edge_bounds(R.edge_table(lM))
    return bool((R.edge_modes(S_B, np.log(m.gamma), U, a, b, R.T - R.DRIFT) >= 0).all())


def decided_tables(env, N, U, seed):
    H = 32 if (U >= 50 and N >= 17) else 16
    (m, S_B, lM) = tables_for(env, N, H, U, seed=seed)
    assert all_decided_at_hint(m, S_B, lM, U), (N, U, H, seed)
    return m, S_B, lM


def with_runs(env, knob, *args):
    """run_case under knob f_runs -> (rise, pred, rise of f_run_passes over both of its runs: f_sure = 1 adds none)"""
    p0 = env.ctx.stat("f_run_passes")
    try:
        env.ctx.set_knob("f_runs", knob)
        (rise, pred) = run_case(env, *args)
    finally:
        env.ctx.set_knob("f_runs", 0)
    return rise, pred, env.ctx.stat("f_run_passes") - p0


def groups(G):
    return ((G + 63) // 64 + 15) // 16


NS = (2, 3, 5, 17, 18, 33, 34, 45)
US = (1, 3, 50, 64)
GS = (1, 65, 1100)
SHAPES = [(NS[i], US[j], GS[(i + j) % 3]) for i in range(8) for j in range(4)]


@pytest.mark.parametrize("N,U,G", SHAPES)
def test_decided_tables_run_form(env, N, U, G):
    (m, S_B, lM) = decided_tables(env, N, U, 5 * N + U + (1 if (N, U) == (5, 64) else 0))
    (rise, pred, runs) = with_runs(env, 0, m, N, U, G, 900 + 13 * N + U, 3, [Call(S_B, lM, 4)])
    assert runs == 3 and rise["f_sure_passes"] == 3
    n_tiles = sum(len(t) > 0 for t in R.tiles(N))
    assert pred[1] + pred[2] == 3 * n_tiles * groups(G) and pred[1] > 0


@pytest.mark.parametrize("N,U,G,seed", ((13, 3, 130, 94), (13, 7, 130, 98), (45, 16, 130, 1)))
def test_open_edges_inside_the_run_kernel(env, N, U, G, seed):
    """H = 3 and f_runs = 2: the run kernel meets edges the rule leaves open and draws them itself"""
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=seed)
    assert not all_decided_at_hint(m, S_B, lM, U)
    (rise, pred, runs) = with_runs(env, 2, m, N, U, G, 311 + U, 5, [Call(S_B, lM, 4)])
    assert runs == 3
    n_tiles = sum(len(t) > 0 for t in R.tiles(N))
    assert 0 < pred[1] < 3 * n_tiles * groups(G)


def test_mixed_table_keeps_the_per_tile_kernel(env):
    """the auto choice: a table with an open tile at the hint does not run the run form"""
    (N, U) = (13, 7)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=98)
    assert not all_decided_at_hint(m, S_B, lM, U)
    (rise, pred, runs) = with_runs(env, 0, m, N, U, 130, 318, 5, [Call(S_B, lM, 4)])
    assert runs == 0 and rise["f_sure_passes"] == 3


def run_table(env, N):
    """the runs of Nreg = N from the library: rows of (n0, mb, cnt0, cnt1, tile0, ntile, cr0, cr1, philox blocks)"""
    out = (C.c_int64 * 9)()
    rows = []
    for t in range(env.lib.load().fcd_f_run_count(N)):
        assert env.lib.load().fcd_f_run_locate(N, t, out) == 0
        rows.append(list(out))
    return np.array(rows, dtype=np.int64)


def out_of_range_places(N, G, chain0, seed, sweeps, runs):
    """the out-of-range uniforms of the pair-tile passes as (shared, edge) flags: shared = the draw's Philox block holds edges of
    two tiles of its run's row, edge = it is the first or the last block of that row of the run"""
    Cn = N * (N - 1) // 2
    c = np.arange(Cn, dtype=np.int64)
    chains = chain0 + np.arange(64 * ((G + 63) // 64), dtype=np.int64)
    seg = {}
    for (n0, mb, cnt0, cnt1, _t0, _nt, cr0, cr1, _pb) in runs:
        for (cr, cnt) in ((cr0, cnt0), (cr1, cnt1)):
            for k in range(cnt):
                seg[int(cr + k)] = (int(cr), int(cnt))
    flags = []
    for s in sweeps:
        w = R.philox_words((c >> 2)[:, None], chains[None, :], s, 2, seed)
        bad = ~R.in_range(w[np.arange(Cn), :, c & 3])                  # (C, chains)
        for e in np.nonzero(bad.any(axis=1))[0]:
            (cr, cnt) = seg[int(e)]
            ids = [i for i in range(4 * (int(e) >> 2), 4 * (int(e) >> 2) + 4) if cr <= i < cr + cnt]
            shared = len({(i - cr) // 4 for i in ids}) > 1
            edge = (int(e) >> 2) in (cr >> 2, (cr + cnt - 1) >> 2)
            flags.append((shared, edge))
    return flags


RUN_FALLBACK_SEED = 2


def test_out_of_range_lanes_are_drawn_by_their_wave(env):
    """8 M draws: some uniforms lie outside fcd_draw_f_sure's range; those (wave, edge) draws run the sums, nothing else does"""
    (N, U, G) = (45, 16, 2048)
    (m, S_B, lM) = decided_tables(env, N, U, 1)
    flags = out_of_range_places(N, G, 0, RUN_FALLBACK_SEED, (1, 2, 3), run_table(env, N))
    assert any(s for (s, _e) in flags) and any(e for (_s, e) in flags), flags
    (rise, pred, runs) = with_runs(env, 0, m, N, U, G, RUN_FALLBACK_SEED, 0, [Call(S_B, lM, 4)])
    assert runs == 3
    assert pred[2] >= 3, pred


def test_f_runs_1_walks_the_same_chains_with_the_same_counters(env):
    (N, U, G) = (34, 3, 1100)
    (m, S_B, lM) = decided_tables(env, N, U, 5 * N + U)
    args = (m, N, U, G, 900 + 13 * N + U, 3, [Call(S_B, lM, 4)])
    (rise0, pred0, runs0) = with_runs(env, 0, *args)
    (rise1, pred1, runs1) = with_runs(env, 1, *args)
    assert (runs0, runs1) == (3, 0)
    assert rise0 == rise1 and tuple(pred0) == tuple(pred1)


@pytest.mark.parametrize("H,knob", ((16, 0), (3, 2)))
def test_m_steps_after_every_sweep(env, H, knob):
    """six sweeps, the rule evaluated at each pass's own gamma: the decided table in the run form, the H = 3 table under f_runs = 2"""
    (N, U, G) = (13, 7, 130)
    (m, S_B, lM) = tables_for(env, N, H, U, seed=98)
    assert all_decided_at_hint(m, S_B, lM, U) == (H == 16)
    (rise, pred, runs) = with_runs(env, knob, m, N, U, G, 5, 2, [Call(S_B, lM, 6, mstep=True)])
    assert runs == 5


def test_f_tol_keeps_both_forms_off(env):
    (N, U, G) = (18, 3, 65)
    (m, S_B, lM) = decided_tables(env, N, U, 5 * N + U)
    try:
        env.ctx.set_knob("f_tol", 1e30)
        env.ctx.set_knob("f_records", 2)
        env.ctx.set_knob("f_runs", 2)
        eng = new_engine(env, m, Call(S_B, lM, 4), N, U, G, 1234, 7)
        (s0, p0) = (stats(env), env.ctx.stat("f_run_passes"))
        eng.run(0, 4, mstep_every=0)
        rise = dict(zip(STATS, stats(env) - s0))
        runs = env.ctx.stat("f_run_passes") - p0
    finally:
        env.ctx.set_knob("f_tol", 0.0)
        env.ctx.set_knob("f_records", 0)
        env.ctx.set_knob("f_runs", 0)
    wave_edges = ((G + 63) // 64) * (N * (N - 1) // 2)
    assert rise["f_repeats"] == 4 * wave_edges
    assert (rise["f_rec_passes"], rise["f_sure_passes"], rise["f_sure_tiles"], rise["f_sure_fallbacks"], runs) == (3, 0, 0, 0, 0)
