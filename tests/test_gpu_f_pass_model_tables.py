"""
The f pass's record, decided-tile and run forms (gibbs_f_pair_kernel<.., SURE>, gibbs_f_run_kernel) on the tables of every
model the fits hand the sampler: patient sums of the shared and grouped models (U' = 1, 3, 64), sessions and noise tables,
masked tables with rows that are exactly 0.0, a weighted table with -inf, a table scaled until the fp32 error bound passes
its cap inside live tiles, and a ladder of tables changed in place between calls (tests/f_pass_table_cases.py builds them,
tests/test_f_pass_table_cases.py pins on the CPU which form each must take).

Every case goes through run_case of tests/test_gpu_f_sure_tiles.py: chains, marginal counters and pooled counts against the
C oracle bit for bit, f_repeats of f_sure = 1 against f_sure = 0, the three counters against the CPU's prediction
(tests/f_sure_ref.py).  Each case runs under the auto choice (f_runs = 0) and under its other form (f_runs = 1 where auto took
the run form, 2 where it took the per-tile kernel) and asserts from f_run_passes which one ran.  The last tests leave every
knob alone: the production configuration, in the engine and through the three fits.  No comparison has a tolerance.
"""
import os
import sys

import numpy as np
import numpy.testing as nptest
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_pass_table_cases as FC  # noqa: E402
from test_gpu_f_sure_tiles import Call, env, new_engine, run_case  # noqa: E402,F401
from test_gpu_f_sure_runs import groups, with_runs  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("f_rec_passes", "f_sure_passes", "f_run_passes")


def forms(env):
    return np.array([env.ctx.stat(k) for k in FORMS], dtype=np.int64)


def both_forms(env, name, case, G, seed, chain0, n=4, mstep=False):
    """the case under f_runs = 0 and under its other form -> (rise, prediction) of the auto run"""
    (S_B, lM, N, U, p) = case
    m = FC.model()
    n_pair = n - 1
    out = []
    with np.errstate(invalid="ignore"):                      # (the log-odds of a -inf table on the CPU: NaN, as on the device)
        for knob in (0, 1 if p["all"] else 2):
            (rise, pred, runs) = with_runs(env, knob, m, N, U, G, seed, chain0, [Call(S_B, lM, n, mstep=mstep)])
            run_form = p["any"] and (p["all"] if knob == 0 else knob == 2)
            assert runs == (n_pair if run_form else 0), (name, knob, runs)
            assert rise["f_sure_passes"] == (n_pair if p["any"] else 0) and rise["f_rec_passes"] == n_pair, (name, knob, rise)
            out.append((rise, tuple(pred)))
    assert out[0] == out[1], (name, out)                     # the same counters from both forms (the chains are the oracle's in both)
    return out[0]


@pytest.mark.parametrize("name", list(FC.CASES))
def test_model_tables_in_both_forms(env, name):
    case = FC.build(name)
    p = case[4]
    G = FC.CASES[name][3]
    i = list(FC.CASES).index(name)
    (_rise, pred) = both_forms(env, name, case, G, 4100 + 17 * i, i % 4)
    n_wg = 3 * p["tiles"] * groups(G)                        # (three pair-tile passes; a counted "tile" is a workgroup)
    if p["all"]:
        assert pred[1] + pred[2] == n_wg and pred[1] > 0, (name, pred)
    else:
        assert p["decided_T"] > 0 and 0 < pred[1] + pred[2] == 3 * p["decided_T"] * groups(G) < n_wg, (name, pred)


def test_ladder_of_tables_changed_in_place(env):
    """all -> none -> some -> all on one engine: every call's form is that of the tables it finds, not of the call before"""
    steps = FC.build_ladder()
    assert tuple(FC.hint_state(s[4]) for s in steps) == ("all", "none", "some", "all")
    (N, U, G) = (steps[0][2], steps[0][3], FC.LADDER[2])
    calls = [Call(s[0], s[1], 3) for s in steps]
    seen = {}
    last = [forms(env)]

    def after_call(knob, i):
        now = forms(env)
        seen[(knob, i)] = tuple(now - last[0])
        last[0] = now
    run_case(env, FC.model(), N, U, G, 73, 1, calls, after_call=after_call)
    # f_sure = 1: records, no decided path; f_sure = 0: (records, decided path, run form) of two pair-tile passes per call
    assert [seen[(1, i)] for i in range(4)] == [(2, 0, 0)] * 4, seen
    assert [seen[(0, i)] for i in range(4)] == [(2, 2, 2), (2, 0, 0), (2, 2, 0), (2, 2, 2)], seen
    # ... and with the run form forced (f_runs = 2), the "some" call takes it too, the "none" call still has no decided path
    seen.clear()
    last[0] = forms(env)
    try:
        env.ctx.set_knob("f_runs", 2)
        run_case(env, FC.model(), N, U, G, 73, 1, calls, after_call=after_call)
    finally:
        env.ctx.set_knob("f_runs", 0)
    assert [seen[(0, i)] for i in range(4)] == [(2, 2, 2), (2, 0, 0), (2, 2, 2), (2, 2, 2)], seen


@pytest.mark.parametrize("name", ("shared-13", "missing-13"))
def test_m_steps_after_every_sweep(env, name):
    """six sweeps, the rule evaluated at each pass's own gamma; the form is the one the hint chose at the call's start"""
    both_forms(env, name, FC.build(name), 130, 5, 2, n=6, mstep=True)


def oracle_sweeps(env, f, r, S_B, lM, gamma, pi2, seed, n, chain0=0):
    for s in range(n):
        env.CO.gibbs_f_step(f, r, S_B, lM, np.log(gamma), seed, s, chain0)
        env.CO.gibbs_r_step(f, r, lM, np.log(pi2), seed, s, env.lib.EDGE_MODES["symmetric"], chain0)


@pytest.mark.parametrize("name", ("shared-13", "missing-13"))
def test_default_knobs_take_the_forms_the_premise_names(env, name):
    """one 12-sweep call, no knob set: eleven passes on the records, in the run form where every tile is decided at the hint"""
    (S_B, lM, N, U, p) = FC.build(name)
    (m, G, seed) = (FC.model(), 130, 2024)
    assert env.ctx.stat("f_rec_min_sweeps") <= 11
    eng = new_engine(env, m, Call(S_B, lM, 12), N, U, G, seed, 0)
    f0 = forms(env)
    eng.run(0, 12, mstep_every=0)
    (f_g, r_g) = eng.export_state()
    assert env.ctx.stat("dev_err") == 0
    assert tuple(forms(env) - f0) == (11, 11, 11 if p["all"] else 0), name
    (f_o, r_o) = env.CO.gibbs_init(G, N, U, 0.3, seed, 0)
    oracle_sweeps(env, f_o, r_o, S_B, lM, m.gamma, m.pi2(), seed, 12)
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)


LABELS = [0, 1, 1] + [2] * 6                                  # group sizes (1, 2, U - 3)


@pytest.mark.parametrize("which", ("shared", "grouped", "unshared"))
def test_fits_reach_the_record_forms_and_equal_the_oracle(env, which):
    """sessions + NaN data through the fit, default knobs, 14 sweeps in one call: the chains are the C oracle's on the fit's
    own device-built tables, and thirteen passes ran on the records"""
    F = env.pkg.fit
    (N, H, U, K, G, seed) = (13, 16, 9, 3, 128, 41)
    (_m, b, bt) = FC.data(N, H, U, 5, sessions=K)
    rng = np.random.default_rng(6)
    bt[rng.random(bt.shape) < 0.15] = np.nan
    b[rng.random(b.shape) < 0.05] = np.nan
    bt[FC.edge_id(4, 3), :, :] = np.nan                       # an edge no patient has: its rows are exactly 0.0
    (fit, model) = {"shared": (F.SharedRegionFit(), env.pkg.SharedRegionModel()),
                    "grouped": (F.GroupedRegionFit(), env.pkg.GroupedRegionModel()),
                    "unshared": (F.UnsharedRegionFit(), env.pkg.UnsharedRegionModel())}[which]
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt, fit.missing_data) = (model, b, bt, True)
    if which == "grouped":
        fit.group_labels = list(LABELS)
    (fit.method, fit.n_sweeps, fit.burn_in, fit.mstep_every, fit.n_chains, fit.seed) = ("gibbs", 14, 4, 0, G, seed)
    (fit.connection_marginals, fit.anomaly_counts) = (True, True)
    (gamma, pi2) = (np.array(model.gamma, dtype=np.float64), np.array(model.pi2(), dtype=np.float64))
    f0 = forms(env)
    fit.run()
    rise = forms(env) - f0
    (S_B, lM) = (fit._d["S_B"].cpu().numpy(), np.ascontiguousarray(fit._lM))
    Up = {"shared": 1, "grouped": 3, "unshared": U}[which]
    assert lM.shape == (N * (N - 1) // 2, Up, 3, 3) and (lM[FC.edge_id(4, 3)] == 0.0).all()
    p = FC.premise(N, S_B, lM, Up, np.log(gamma))
    assert p["any"], which                                    # (... or the passes below would be the plain record kernel's)
    assert env.ctx.stat("dev_err") == 0
    assert tuple(rise) == (13, 13, 13 if p["all"] else 0), (which, rise, p["decided_hint"], p["tiles"])
    (f_o, r_o) = env.CO.gibbs_init(G, N, Up, float(pi2[1]), seed, 0)
    oracle_sweeps(env, f_o, r_o, S_B, lM, gamma, pi2, seed, 14)
    (f_g, r_g) = fit.sampler.export_state()
    nptest.assert_array_equal(f_g, f_o)
    nptest.assert_array_equal(r_g, r_o)
    assert fit.connection_sweeps == 10 and fit.anomaly_count_sweeps == 10
