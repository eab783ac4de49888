"""
The f half of the sweep's tally counted by the f pass's run kernel (gibbs_f_run_kernel, knob tally_in_f, counter tally_f_in_f):
the kernel leaves the pooled counts of f and the marginal counters of the edges as it stores the draws, and neither the r pass
nor the tally behind it reads the f state back.

Every case runs its calls as ONE fcd_gibbs_run call each (14 sweeps) and compares, the way run_case of
tests/test_gpu_r_decided.py does, f, r, cnt_f, cnt_r, the five counts of the last sweep and the hyper block after every call with
the C oracle's walk bit for bit (the hyper block of every sweep is the device's own, from one-sweep calls of a second engine:
those never build a record table, so they never launch the run kernel), dev_err with 0, and the rises of tally_f_in_f,
tally_f_in_r and tally_f_in_pack with what the rule predicts sweep by sweep (carriers() below).  Which sweeps run the run form
and the sparse r pass is predicted on the CPU (tests/f_sure_ref.py, tests/r_sure_ref.py) and checked against f_run_passes and
r_sure_passes, so that no case passes without the form it is about.

A call of n sweeps: sweep 0 on edge tiles with a packing launch (which carries the f half), sweeps 1 .. n - 1 in the run form
where the record build's hint (or knob f_runs = 2) says so, sweeps 2 .. n - 1 with a sparse r pass where knob r_sure says so.
"""
import os
import sys

import numpy as np
import numpy.testing as nptest
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_sure_ref as R  # noqa: E402
import r_sure_ref as RS  # noqa: E402
from test_gpu_f_sure_tiles import Call, env, f_hist, new_engine, prepare, tables_for  # noqa: E402,F401
from test_gpu_r_decided import off_of, scaled  # noqa: E402

pytestmark = pytest.mark.gpu

N_SWEEPS = 14
STATS = ("tally_f_in_f", "tally_f_in_r", "tally_f_in_pack", "f_run_passes", "r_sure_passes", "pack_launches", "f_repeats",
         "f_sure_fallbacks")
R_TALLY_MAX_ROUNDS = 5


def stats(env):
    return dict((k, env.ctx.stat(k)) for k in STATS)


class Sched(object):
    """mstep_every, accumulate_from (None: no counters) and want_counts of every call of a case"""

    def __init__(self, mstep=1, acc_from=0, want=True):
        self.mstep, self.acc_from, self.want = mstep, acc_from, want

    def do_m(self, i):
        return self.mstep > 0 and (i + 1) % self.mstep == 0

    def do_a(self, s):
        return self.acc_from is not None and s >= self.acc_from

    def counts_f(self, i, n, s):
        """does sweep i of n (number s) of a call count f at all"""
        return self.do_m(i) or self.do_a(s) or (self.want and i + 1 == n)


_REF = {}


def reference(env, key, m, N, U, G, seed, chain0, calls, sched, hyper0=None):
    """the oracle's walk of the calls, once per key -> final f, r, counters, and per call (starting hyper, hyper after it,
    the oracle's five counts after it)"""
    if key in _REF:
        return _REF[key]
    ref = new_engine(env, m, calls[0], N, U, G, seed, chain0)
    if hyper0 is not None:
        ref.set_hyper(*hyper0)
    (f_o, r_o) = env.CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    cnt_f = np.zeros((f_o.shape[1], 3), dtype=np.int64)
    cnt_r = np.zeros((N, U), dtype=np.int64)
    (per_call, sweep) = ([], 0)
    for (i, c) in enumerate(calls):
        h = prepare(env, ref, m, c, i == 0)
        h0 = h
        for j in range(c.n):
            s = sweep + j
            env.CO.gibbs_f_step(f_o, r_o, c.S_B, c.lM, h[0:3], seed, s, chain0)
            env.CO.gibbs_r_step(f_o, r_o, c.lM, h[3:5], seed, s, 1, chain0)
            if sched.do_a(s):
                cnt_f += f_hist(f_o)
                cnt_r += r_o.astype(np.int64).sum(axis=0)
            ref.run(s, 1, mstep_every=1 if sched.do_m(j) else 0)
            h = ref.hyper.cpu().numpy().copy()
        per_call.append((h0, h, np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5].copy()))
        sweep += c.n
    (f_r, r_r) = ref.export_state()         # (the second engine walked the oracle's chains: its hyper blocks are the oracle's)
    nptest.assert_array_equal(f_r, f_o, err_msg=key)
    nptest.assert_array_equal(r_r, r_o, err_msg=key)
    _REF[key] = (f_o, r_o, cnt_f, cnt_r, per_call)
    return _REF[key]


def forms_of_call(N, U, c, h0, f_runs, r_sure):
    """-> (the run form runs in sweeps 1 .. n - 1, the sparse r pass in sweeps 2 .. n - 1) of a call that starts at hyper h0"""
    with np.errstate(invalid="ignore"):
        (a, b) = R.edge_bounds(R.edge_table(c.lM))
        mode = R.edge_modes(c.S_B, h0[0:3], U, a, b, R.T - R.DRIFT)
    some = len(R.decided_tiles(N, mode)) > 0
    every = some and bool((mode >= 0).all())
    run = some and f_runs != 1 and (every or f_runs == 2)
    sparse = False
    if r_sure != 1 and (some or r_sure == 2):
        with np.errstate(invalid="ignore"):
            (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, c.S_B, c.lM, h0[0:3])
            sparse = r_sure == 2 or RS.share(hi, lo, off_of(h0), rowflag) >= RS.MIN_SHARE
    return run, sparse


def carriers(env, N, U, G, calls, sched, per_call, f_runs, r_sure, in_f, in_r, pipe):
    """-> the rises (tally_f_in_f, tally_f_in_r, tally_f_in_pack, f_run_passes, r_sure_passes) the rule predicts, and the number
    of sweeps that count f.  pipe: the r passes that are not sparse run the pipelined form (read from r_form_last by the caller)"""
    GW = (G + 63) // 64
    C = N * (N - 1) // 2
    out = np.zeros(5, dtype=np.int64)
    (counted, sweep) = (0, 0)
    for (c, (h0, _h1, _cts)) in zip(calls, per_call):
        (run, sparse) = forms_of_call(N, U, c, h0, f_runs, r_sure)
        for i in range(c.n):
            (run_i, sparse_i) = (run and i >= 1, sparse and i >= 2)
            out[3] += run_i
            out[4] += sparse_i
            if not sched.counts_f(i, c.n, sweep + i):
                continue
            counted += 1
            if run_i and in_f != 1 and (sparse_i or in_f == 2):
                out[0] += 1
            elif i == 0:
                out[2] += 1         # the call's packing launch (C GW is far below its limit here)
            elif not sparse_i and pipe and in_r != 1 and min(GW, 16) == 16:
                nD = 2 * U          # (more than 8 chain words: two in-order workgroups per patient)
                rounds = -(-C // (64 * nD)) * ((GW + 15) // 16)
                out[1] += in_r == 2 or rounds <= R_TALLY_MAX_ROUNDS
        sweep += c.n
    return out, counted


def run_case(env, key, m, N, U, G, seed, chain0, calls, sched=None, in_f=2, f_runs=2, r_sure=2, hyper0=None, pipe=False):
    sched = sched or Sched()
    what = "%s N=%d U=%d G=%d tally_in_f=%d f_runs=%d r_sure=%d mstep=%d acc_from=%s" % (key, N, U, G, in_f, f_runs, r_sure,
                                                                                       sched.mstep, sched.acc_from)
    (f_o, r_o, cnt_f, cnt_r, per_call) = reference(env, key, m, N, U, G, seed, chain0, calls, sched, hyper0)
    (pred, counted) = carriers(env, N, U, G, calls, sched, per_call, f_runs, r_sure, in_f, 0, pipe)
    try:
        env.ctx.set_knob("tally_in_f", in_f)
        env.ctx.set_knob("f_runs", f_runs)
        env.ctx.set_knob("r_sure", r_sure)
        eng = new_engine(env, m, calls[0], N, U, G, seed, chain0)
        if hyper0 is not None:
            eng.set_hyper(*hyper0)
        s0 = stats(env)
        sweep = 0
        for (i, c) in enumerate(calls):
            prepare(env, eng, m, c, i == 0)
            counts = eng.run(sweep, c.n, mstep_every=sched.mstep, accumulate_from=sched.acc_from, want_counts=sched.want)
            sweep += c.n
            (_h0, h1, cts) = per_call[i]
            nptest.assert_array_equal(eng.hyper.cpu().numpy(), h1, err_msg=what + " hyper after call %d" % i)
            if sched.want:
                nptest.assert_array_equal(counts.cpu().numpy()[:5], cts, err_msg=what + " counts of call %d" % i)
        (f_g, r_g) = eng.export_state()
        s1 = stats(env)
    finally:
        env.ctx.set_knob("tally_in_f", 0)
        env.ctx.set_knob("f_runs", 0)
        env.ctx.set_knob("r_sure", 0)
    rise = dict((k, s1[k] - s0[k]) for k in STATS)
    print(what, "rise", rise, "predicted", pred, "sweeps that count f", counted)
    assert env.ctx.stat("dev_err") == 0, what
    nptest.assert_array_equal(f_g, f_o, err_msg=what)
    nptest.assert_array_equal(r_g, r_o, err_msg=what)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy().astype(np.int64), cnt_f, err_msg=what)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy().astype(np.int64), cnt_r, err_msg=what)
    got = tuple(rise[k] for k in STATS[:5])
    assert got == tuple(pred), (what, got, pred)
    # no sweep is counted twice: at most one carrier per sweep that counts (the tally takes the rest)
    assert rise["tally_f_in_f"] + rise["tally_f_in_r"] + rise["tally_f_in_pack"] <= counted, (what, rise, counted)
    assert rise["pack_launches"] == len(calls), (what, rise)
    return rise


def strong(env, N, U):
    """the tables of test_gpu_r_decided.py, scaled so that the run form and the sparse r pass have decided edges and sites"""
    factor = {(33, 7): 2.0}.get((N, U), 8.0)
    return scaled(env, N, U, factor)


# ---- chain-word edges: one valid lane, a partial second word, one workgroup of three waves, a full workgroup and one whose
# last word is partial, a second group of 16 chain words holding one word; chain0 != 0 in two of them
@pytest.mark.parametrize("G,chain0", ((1, 0), (65, 3), (130, 0), (581, 64), (1029, 0)))
def test_chain_words(env, G, chain0):
    (N, U) = (13, 7)
    (m, S_B, lM) = strong(env, N, U)
    rise = run_case(env, "words-%d-%d" % (G, chain0), m, N, U, G, 500 + G, chain0, [Call(S_B, lM, N_SWEEPS)])
    assert rise["tally_f_in_f"] == N_SWEEPS - 1 and rise["r_sure_passes"] == N_SWEEPS - 2


# ---- row edges: odd Nreg (a last row pair of one row, partial runs), full runs at Nreg 64; U = 1, 7, 16
@pytest.mark.parametrize("N,U", ((13, 1), (13, 7), (33, 7), (64, 16)))
def test_rows_and_patients(env, N, U):
    (m, S_B, lM) = strong(env, N, U)
    rise = run_case(env, "rows-%d-%d" % (N, U), m, N, U, 130, 900 + N + U, 3, [Call(S_B, lM, N_SWEEPS)])
    assert rise["tally_f_in_f"] == N_SWEEPS - 1


# ---- exceptional edges
def test_open_edges_are_counted_lane_by_lane(env):
    """H = 3 under f_runs = 2: the run kernel meets edges the rule leaves open; their pairs come from the lanes' own draws"""
    (N, U, G) = (13, 7, 130)
    (m, S_B, lM) = tables_for(env, N, 3, U, seed=98)
    with np.errstate(invalid="ignore"):
        (a, b) = R.edge_bounds(R.edge_table(lM))
        mode = R.edge_modes(S_B, np.log(m.gamma), U, a, b, R.T - R.DRIFT)
    assert (mode < 0).any() and len(R.decided_tiles(N, mode)) > 0
    rise = run_case(env, "mixed", m, N, U, G, 318, 5, [Call(S_B, lM, N_SWEEPS)])
    assert rise["tally_f_in_f"] == N_SWEEPS - 1


def test_tables_with_minus_infinity(env):
    """the `firm` set of tests/nonfinite_tables.py: edges with -inf entries have no mode and are drawn by the wave"""
    import nonfinite_tables as NF
    T = NF.build_set("firm-33-7", 130)
    m = env.pkg.UnsharedRegionModel()
    (m.gamma, m.pi) = (T.gamma.copy(), float(T.pi2[1]))
    rise = run_case(env, "firm-33-7", m, T.Nreg, T.U, 130, T.seed, 0, [Call(T.S_B, T.lM, N_SWEEPS)], hyper0=(T.gamma, T.pi2))
    assert rise["tally_f_in_f"] == N_SWEEPS - 1


def test_the_fp64_repeat_inside_the_wave(env):
    """a table scaled until an edge's fp32 sums cannot decide its draws: f_repeats rises inside the counting run kernel"""
    import f_pass_table_cases as FC
    (S_B, lM, N, U, _p) = FC.build("scaled-13")
    rise = run_case(env, "scaled-13", FC.model(), N, U, 65, 41, 2, [Call(S_B, lM, N_SWEEPS)])
    assert rise["tally_f_in_f"] == N_SWEEPS - 1 and rise["f_repeats"] > 0


FALLBACK_SEED = 2


def test_out_of_range_lanes(env):
    """3.4 M draws of decided edges: the CPU reference itself predicts lanes whose uniform is outside fcd_draw_f_sure's range
    (about 7 per call); the wave draws those edges itself and counts them lane by lane.  No M-step: gamma stays."""
    (N, U, G) = (64, 16, 130)
    (m, S_B, lM) = strong(env, N, U)
    lng = np.log(m.gamma)
    later = [(s, lng) for s in range(1, N_SWEEPS)]
    pred = R.predict(N, U, G, 0, FALLBACK_SEED, S_B, R.edge_table(lM), lng, later)
    assert pred[2] >= 1, pred
    rise = run_case(env, "fallback", m, N, U, G, FALLBACK_SEED, 0, [Call(S_B, lM, N_SWEEPS)], sched=Sched(mstep=0))
    assert rise["f_sure_fallbacks"] == pred[2], (rise, pred)
    assert rise["tally_f_in_f"] == N_SWEEPS - 1


# ---- schedule: acc null in some sweeps (mstep_every 0, 3), cnt_f null throughout or in the first half, counts on the last
# sweep alone
SCHEDULES = ((0, 100, True), (0, 7, True), (1, 100, True), (3, 7, True), (3, 0, False), (1, None, False), (0, None, True))


@pytest.mark.parametrize("mstep,acc_from,want", SCHEDULES)
def test_schedules(env, mstep, acc_from, want):
    (N, U, G) = (13, 7, 130)
    (m, S_B, lM) = strong(env, N, U)
    sched = Sched(mstep, acc_from, want)
    n_count = sum(sched.counts_f(i, N_SWEEPS, i) for i in range(N_SWEEPS))
    rise = run_case(env, "sched-%d-%s-%d" % (mstep, acc_from, want), m, N, U, G, 71, 1, [Call(S_B, lM, N_SWEEPS)], sched=sched)
    assert rise["tally_f_in_f"] + rise["tally_f_in_pack"] == n_count        # (tally_in_f = 2: every sweep has a carrier)


# ---- the rule: 1024 chains are 16 chain words, where the pipelined r pass's waiting workgroups can carry the count
@pytest.mark.parametrize("in_f", (0, 1, 2))
@pytest.mark.parametrize("r_sure", (1, 2))
def test_rule(env, in_f, r_sure):
    (N, U, G) = (13, 7, 1024)
    (m, S_B, lM) = strong(env, N, U)
    lng = np.log(m.gamma)
    with np.errstate(invalid="ignore"):
        (a, b) = R.edge_bounds(R.edge_table(lM))
    assert (R.edge_modes(S_B, lng, U, a, b, R.T - R.DRIFT) >= 0).all()       # (f_runs = 0 takes the run form)
    # the form of the passes that are not sparse, from a call of the same shape with every knob at the parent's behaviour
    try:
        env.ctx.set_knob("tally_in_f", 1)
        env.ctx.set_knob("r_sure", 1)
        probe = new_engine(env, m, Call(S_B, lM, 2), N, U, G, 5, 0)
        probe.run(0, 2, mstep_every=1)
        pipe = env.ctx.stat("r_form_last") == 2
    finally:
        env.ctx.set_knob("tally_in_f", 0)
        env.ctx.set_knob("r_sure", 0)
    assert pipe, "this shape runs the pipelined r pass on a whole device"
    rise = run_case(env, "rule-1024", m, N, U, G, 61, 0, [Call(S_B, lM, N_SWEEPS)], in_f=in_f, f_runs=0, r_sure=r_sure, pipe=pipe)
    n = N_SWEEPS
    want = {(0, 1): (0, n - 1, 1), (1, 1): (0, n - 1, 1), (2, 1): (n - 1, 0, 1),
            (0, 2): (n - 2, 1, 1), (1, 2): (0, 1, 1), (2, 2): (n - 1, 0, 1)}[(in_f, r_sure)]
    assert (rise["tally_f_in_f"], rise["tally_f_in_r"], rise["tally_f_in_pack"]) == want, rise


@pytest.mark.parametrize("in_f", (0, 2))
def test_ladder_of_calls_on_one_engine(env, in_f):
    """every -> no -> some -> every tile decided, as successive calls under the auto choice of the f form: the run kernel counts
    in the first and the last call only, the context's sums are zero when the form changes, and nothing is counted twice"""
    import f_pass_table_cases as FC
    cases = FC.build_ladder()
    (N, U) = (cases[0][2], cases[0][3])
    calls = [Call(c[0], c[1], N_SWEEPS) for c in cases]
    rise = run_case(env, "ladder", FC.model(), N, U, 65, 19, 1, calls, in_f=in_f, f_runs=0)
    assert rise["f_run_passes"] == 2 * (N_SWEEPS - 1)
    assert rise["tally_f_in_f"] == 2 * (N_SWEEPS - (1 if in_f == 2 else 2))
