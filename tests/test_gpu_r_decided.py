"""
The sparse form of the r pass (gibbs_r_range_kernel + gibbs_r_sparse_kernel, knob r_sure): sites whose draw the tables decide
get their r word without a sum, the others are walked in order.  Every case runs its calls as ONE fcd_gibbs_run call each
(14 sweeps, an M-step after every sweep so that pi moves), compares chains, marginal counters and pooled counts with the C
oracle bit for bit, and the counters r_sure_passes / r_sure_builds / r_sure_sites / r_sure_exceptions with what the NumPy
restatement of the rule (tests/r_sure_ref.py), the oracle's f states and the oracle's Philox words predict on the CPU.
The hyper block of every sweep is the device's own, from one-sweep calls of a second engine (those never build a record table,
so they run the blocked forms).

A call of n sweeps runs its first sweep on edge tiles, learns the f hint with its second -- which queues the bound build --
and reads the r hint with its third: sweeps 2 .. n - 1 are sparse where the knob's rule says so.

Shapes: Nreg 64, H 16, U 16, G 130 (the smallest with a natural mix: 63 % decided, three chain words, the last partial);
Nreg 33 and 13 (not a multiple of 16, a last block of one region; lM and S_B scaled on the CPU so that the share lies strictly
between 0.2 and 0.8, asserted before anything runs); U = 7 (a half-used Philox block), U = 1, G = 1.
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

pytestmark = pytest.mark.gpu

N_SWEEPS = 14
STATS = ("r_sure_passes", "r_sure_builds", "r_sure_sites", "r_sure_exceptions")


def stats(env):
    return np.array([env.ctx.stat(k) for k in STATS], dtype=np.int64)


def off_of(h):
    return float(h[4] - h[3])


_REF = {}


def reference(env, key, m, N, U, G, seed, chain0, calls, hyper0=None):
    """the oracle's walk of the calls, once per key: final state, counters, and per call its starting hyper and, for every
    sweep, (sweep number, hyper of the sweep, the f state its f pass left)"""
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
        rows = []
        for s in range(sweep, sweep + c.n):
            env.CO.gibbs_f_step(f_o, r_o, c.S_B, c.lM, h[0:3], seed, s, chain0)
            rows.append((s, h, f_o.copy()))
            env.CO.gibbs_r_step(f_o, r_o, c.lM, h[3:5], seed, s, 1, chain0)
            cnt_f += f_hist(f_o)
            cnt_r += r_o.astype(np.int64).sum(axis=0)
            ref.run(s, 1, mstep_every=1)
            h = ref.hyper.cpu().numpy().copy()
        per_call.append(rows)
        sweep += c.n
    _REF[key] = (f_o, r_o, cnt_f, cnt_r, per_call)
    return _REF[key]


def predict(N, U, G, chain0, seed, calls, per_call, knob, x_lo, off_knobs=False):
    """-> (passes, builds, sites, exceptions) of the calls under knob r_sure"""
    out = np.zeros(4, dtype=np.int64)
    if knob == 1 or off_knobs:
        return out
    for (c, rows) in zip(calls, per_call):
        h0 = rows[0][1]
        with np.errstate(invalid="ignore"):
            (a, b) = R.edge_bounds(R.edge_table(c.lM))
        if not (knob == 2 or R.hint(N, c.S_B, h0[0:3], U, a, b)):
            continue
        out[1] += 1
        (km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, c.S_B, c.lM, h0[0:3])
        if not (knob == 2 or RS.share(hi, lo, off_of(h0), rowflag) >= RS.MIN_SHARE):
            continue
        for (s, h, f) in rows[2:]:
            (sure, exc) = RS.predict_pass(N, U, G, chain0, seed, s, off_of(h), f, km, hi, lo, rowflag, x_lo)
            out += np.array([1, 0, sure, exc])
    return out


def run_case(env, key, m, N, U, G, seed, chain0, calls, knob=0, x=0.0, r_tol=0.0, hyper0=None):
    what = "%s N=%d U=%d G=%d knob=%d x=%g" % (key, N, U, G, knob, x)
    (f_o, r_o, cnt_f, cnt_r, per_call) = reference(env, key, m, N, U, G, seed, chain0, calls, hyper0)
    pred = predict(N, U, G, chain0, seed, calls, per_call, knob, max(x, RS.X_LO), off_knobs=r_tol > 0)
    try:
        env.ctx.set_knob("r_sure", knob)
        env.ctx.set_knob("r_sure_x", x)
        env.ctx.set_knob("r_tol", r_tol)
        eng = new_engine(env, m, calls[0], N, U, G, seed, chain0)
        if hyper0 is not None:
            eng.set_hyper(*hyper0)
        s0 = stats(env)
        (sweep, forms) = (0, [])
        for (i, c) in enumerate(calls):
            prepare(env, eng, m, c, i == 0)
            counts = eng.run(sweep, c.n, mstep_every=1, accumulate_from=0, want_counts=True).cpu().numpy().copy()
            forms.append(env.ctx.stat("r_form_last"))
            sweep += c.n
        (f_g, r_g) = eng.export_state()
        rise = stats(env) - s0
    finally:
        env.ctx.set_knob("r_sure", 0)
        env.ctx.set_knob("r_sure_x", 0.0)
        env.ctx.set_knob("r_tol", 0.0)
    print(what, "counters", dict(zip(STATS, rise)), "predicted", pred, "forms", forms)
    assert env.ctx.stat("dev_err") == 0, what
    nptest.assert_array_equal(r_g, r_o, err_msg=what)
    nptest.assert_array_equal(f_g, f_o, err_msg=what)
    nptest.assert_array_equal(eng.cnt_f.cpu().numpy().astype(np.int64), cnt_f, err_msg=what)
    nptest.assert_array_equal(eng.cnt_r.cpu().numpy().astype(np.int64), cnt_r, err_msg=what)
    nptest.assert_array_equal(counts[:5], np.asarray(env.CO.gibbs_stats(f_o, r_o))[:5], err_msg=what)
    assert tuple(rise) == tuple(pred), (what, rise, pred)
    return dict(zip(STATS, rise)), forms


def start_share(m, N, U, S_B, lM):
    (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
    return RS.share(hi, lo, float(np.log(m.pi) - np.log(1.0 - m.pi)), rowflag)


_TAB = {}


def natural(env):
    if "natural" not in _TAB:
        _TAB["natural"] = tables_for(env, 64, 16, 16, seed=3)
    return _TAB["natural"]


def scaled(env, N, U, factor, seed=3):
    key = (N, U, factor, seed)
    if key not in _TAB:
        (m, S_B, lM) = tables_for(env, N, 16, U, seed=seed)
        _TAB[key] = (m, factor * S_B, factor * lM)
    return _TAB[key]


@pytest.mark.parametrize("knob,x,r_tol", ((0, 0.0, 0.0), (1, 0.0, 0.0), (2, 0.0, 0.0), (2, 0.25, 0.0), (2, 0.0, 1e30)))
def test_natural_mix(env, knob, x, r_tol):
    """Nreg 64, H 16, U 16, G 130: 63 % of the sites decided -- below the share the auto rule asks for, so r_sure = 0 and 1 keep
    the old form and 2 runs the sparse one; r_sure_x = 0.25 makes half of all draws exceptions; r_tol = 1e30 keeps the old forms"""
    (N, U, G) = (64, 16, 130)
    (m, S_B, lM) = natural(env)
    assert 0.55 < start_share(m, N, U, S_B, lM) < 0.75
    (rise, forms) = run_case(env, "natural", m, N, U, G, 77, 5, [Call(S_B, lM, N_SWEEPS)], knob=knob, x=x, r_tol=r_tol)
    if knob != 2 or r_tol > 0:
        assert rise["r_sure_passes"] == 0 and forms == [2]
        assert rise["r_sure_builds"] == (1 if knob == 0 else 0)
    else:
        assert rise["r_sure_passes"] == N_SWEEPS - 2 and forms == [4] and rise["r_sure_sites"] > 0
    if x > 0:
        assert rise["r_sure_exceptions"] > rise["r_sure_sites"]


def test_auto_rule_takes_a_strong_table(env):
    """the same data with S_B and lM times 8: 95 % decided, r_sure = 0 runs the sparse form"""
    (N, U, G) = (64, 16, 130)
    (m, S_B, lM) = scaled(env, N, U, 8.0)
    assert start_share(m, N, U, S_B, lM) > RS.MIN_SHARE
    (rise, forms) = run_case(env, "strong", m, N, U, G, 78, 4, [Call(S_B, lM, N_SWEEPS)], knob=0)
    assert rise["r_sure_passes"] == N_SWEEPS - 2 and forms == [4] and rise["r_sure_sites"] > 0


# (Nreg, U, G, factor on S_B and lM): shares measured on the CPU 0.62, 0.59, 0.69, 0.54
SCALED = ((33, 7, 130, 2.0), (13, 7, 130, 8.0), (13, 1, 130, 8.0), (13, 7, 1, 4.0))


@pytest.mark.parametrize("N,U,G,factor", SCALED)
def test_short_blocks_odd_u_one_patient_one_chain(env, N, U, G, factor):
    (m, S_B, lM) = scaled(env, N, U, factor)
    assert 0.2 < start_share(m, N, U, S_B, lM) < 0.8
    key = "scaled-%d-%d-%d" % (N, U, G)
    (rise, forms) = run_case(env, key, m, N, U, G, 900 + N + U, 3, [Call(S_B, lM, N_SWEEPS)], knob=2)
    assert rise["r_sure_passes"] == N_SWEEPS - 2 and forms == [4] and rise["r_sure_sites"] > 0
    (rise, forms) = run_case(env, key, m, N, U, G, 900 + N + U, 3, [Call(S_B, lM, N_SWEEPS)], knob=0)
    assert (rise["r_sure_passes"], rise["r_sure_builds"]) == (0, 1) and forms[0] != 4


def test_exceptions_change_no_chain_at_a_short_last_block(env):
    (N, U, G, factor) = SCALED[0]
    (m, S_B, lM) = scaled(env, N, U, factor)
    (rise, _forms) = run_case(env, "scaled-%d-%d-%d" % (N, U, G), m, N, U, G, 900 + N + U, 3, [Call(S_B, lM, N_SWEEPS)], knob=2, x=0.25)
    assert rise["r_sure_exceptions"] > 0 and rise["r_sure_sites"] > 0


def test_an_open_edge_inside_known_rows(env):
    """masked tables (f_pass_table_cases.missing, LONE_CONTROL): edge (4, 3) has no mode, its two rows are walked in full.  The
    tables are scaled by 8 so that other rows have decided sites -- but for S_B of that edge, which would decide it"""
    import f_pass_table_cases as FC
    (S_B, lM, N, U, p) = FC.build("missing-13")
    m = FC.model()
    S8 = 8.0 * S_B
    S8[p["zero_lM"]] = S_B[p["zero_lM"]]
    (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S8, 8.0 * lM, np.log(m.gamma))
    assert rowflag[4] and rowflag[3] and not rowflag.all()
    assert 0.0 < RS.share(hi, lo, float(np.log(m.pi) - np.log(1.0 - m.pi)), rowflag) < 0.8
    (rise, forms) = run_case(env, "missing-13", m, N, U, 65, 41, 2, [Call(S8, 8.0 * lM, N_SWEEPS)], knob=2)
    assert rise["r_sure_passes"] == N_SWEEPS - 2 and rise["r_sure_sites"] > 0


def test_tables_with_minus_infinity(env):
    """the `firm` set of tests/nonfinite_tables.py: bounds that touch a -inf entry are NaN, those sites are open"""
    import nonfinite_tables as NF
    T = NF.build_set("firm-33-7", 130)
    m = env.pkg.UnsharedRegionModel()
    (m.gamma, m.pi) = (T.gamma.copy(), float(T.pi2[1]))
    with np.errstate(invalid="ignore"):
        (_km, _lMd, hi, _lo, _base, rowflag) = RS.tables_for_call(T.Nreg, T.U, T.S_B, T.lM, T.lng)
    assert np.isnan(hi).any() and rowflag.any() and not rowflag.all()
    (rise, forms) = run_case(env, "firm-33-7", m, T.Nreg, T.U, 130, T.seed, 0, [Call(T.S_B, T.lM, N_SWEEPS)], knob=2,
                             hyper0=(T.gamma, T.pi2))
    assert rise["r_sure_passes"] == N_SWEEPS - 2 and forms == [4]


@pytest.mark.parametrize("knob", (0, 2))
def test_ladder_of_calls_on_one_engine(env, knob):
    """every -> none -> some -> every tile decided, as successive calls: bounds, rows of differences and mode words left over
    from an earlier call would show"""
    import f_pass_table_cases as FC
    cases = FC.build_ladder()
    (N, U) = (cases[0][2], cases[0][3])
    calls = [Call(c[0], c[1], N_SWEEPS) for c in cases]
    (rise, forms) = run_case(env, "ladder", FC.model(), N, U, 65, 19, 1, calls, knob=knob)
    if knob == 2:
        assert rise["r_sure_builds"] == 4 and forms == [4, 4, 4, 4]
    else:       # (no build on the call without a decided tile; which decided calls reach the auto rule's share depends on where
        # the M-steps have taken pi by then -- the prediction in run_case follows it)
        assert rise["r_sure_builds"] == 3 and forms[1] != 4


def test_a_weak_table_builds_nothing(env):
    (N, U, G) = (30, 8, 256)
    (m, S_B, lM) = tables_for(env, N, 2, U, seed=N + U, weak=True)
    (rise, forms) = run_case(env, "weak", m, N, U, G, 17, 0, [Call(S_B, lM, N_SWEEPS)], knob=0)
    assert (rise["r_sure_passes"], rise["r_sure_builds"]) == (0, 0) and forms[0] != 4
