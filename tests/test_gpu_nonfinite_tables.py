"""
The sampler on tables with -inf entries and on zero gamma / pi (run with -m gpu on an MI355X).

Every draw of the device kernels is the draw of the oracle's fp64 formulas from the ABSOLUTE log-weights (header of
test_gpu_draw_boundaries.py); the other sampler suites check that on finite inputs only.  Here the table sets of
tests/nonfinite_tables.py (test_nonfinite_tables.py pins them on the CPU) run through every form of both passes: two sweeps
from the imported state, and f and r of EVERY chain must equal the C oracle's -- there is no tolerance.  The fast f forms
work on log-odds against type 0, which are +inf or NaN where type 0 is impossible (gamma_0 = 0, lM[c, u, 0, l] = -inf): their
exact repeat then takes the draw from the absolute log-weights (fcd_f_open / fcd_f_abs_draw of fcd_gibbs.hip).  The r pass
works on differences too; a site with s0 = s1 = -inf gives a genuine NaN, which the pipelined form meets in its "panel value
not there yet" test -- it sums the row again and draws 0, like the oracle's logit(x) < NaN.  Nothing here provokes a fault:
all inputs are states and tables the library accepts.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import boundary_probes as BP
import f_sure_ref as FR
import nonfinite_tables as NT
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    from fcdiff_amd.gibbs import GibbsEngine
    from oracle import c_oracle as CO
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.tables, e.GibbsEngine, e.CO = torch, fcdiff_amd, _lib, tables, GibbsEngine, CO
    e.ctx = _lib.Context()
    return e


@pytest.fixture
def knobs(env):
    """Set tuning / test knobs of the shared context (fcd_ctx_set_knob) for one test; all back to default afterwards."""
    touched = []

    def set_(**kw):
        for (k, v) in kw.items():
            env.ctx.set_knob(k, v)
            touched.append(k)
    yield set_
    for k in touched:
        env.ctx.set_knob(k, 0)


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# The forms of test_gpu_draw_boundaries.PATHS, and: every r draw / every f draw through its exact path (r_tol, f_tol), the
# pair-tile f pass on records made once per call with and without the decided-tile rule (f_records = 2; f_sure = 1 is "off"),
# and the decided path in its run form whatever the hint says of the other tiles (f_runs = 2: gibbs_f_run_kernel).
PATHS = {
    "steps": dict(driver="steps", knobs={}),
    "packed": dict(driver="sweeps", knobs={}, pipelined=True),
    "run": dict(driver="run", knobs={}, pipelined=True),
    "anyU+rstep": dict(driver="sweeps", knobs={"f_form": 2, "r_path": 3}),
    "mask+ub1": dict(driver="sweeps", knobs={"f_form": 3, "r_ub": 1}),
    "dsplit": dict(driver="sweeps", knobs={"r_dsplit": 1}, pipelined=True),
    "generic": dict(driver="steps", knobs={}, region_major=False),
    "r_tol": dict(driver="sweeps", knobs={"r_tol": 1e30}, pipelined=True),
    "f_tol": dict(driver="sweeps", knobs={"f_tol": 1e30}, pipelined=True),
    "run+rec": dict(driver="run", knobs={"f_records": 2}, pipelined=True),
    "run+rec-nosure": dict(driver="run", knobs={"f_records": 2, "f_sure": 1}, pipelined=True),
    "run+rec+runs": dict(driver="run", knobs={"f_records": 2, "f_runs": 2}, pipelined=True),
}
REC_PATHS = ("run+rec", "run+rec+runs")                               # the decided-tile rule is on: check_sweeps asserts which form ran
STEP_FORMS = ("steps", "anyU+rstep", "generic")                       # no pipelined r pass in them
COUNTS_REPEATS = ("steps", "packed", "run", "anyU+rstep", "dsplit", "r_tol", "f_tol", "run+rec", "run+rec-nosure", "run+rec+runs")
# not the full product: every source meets every f form (pair, pair tiles, any-U, scalar masks, generic) and every r form
# (pipelined, one in-order workgroup, step per launch, one patient per panel workgroup, generic); gamma0 and item meet all paths
_A = ["steps", "packed", "dsplit", "generic"]
_B = ["run", "anyU+rstep", "mask+ub1"]
_X = ["r_tol", "f_tol", "run+rec", "run+rec-nosure", "run"]
_R = ["run+rec", "run+rec+runs"]
PLAN = {
    "item-33-7": _A + _X + ["run+rec+runs"], "item-16-2": ["mask+ub1", "anyU+rstep", "generic"], "item-17-64": _B + _R, "item-33-70": ["run", "steps"],
    "gamma0-33-7": _A + _X, "gamma0-16-2": ["mask+ub1", "anyU+rstep", "generic"], "gamma0-17-64": _B, "gamma0-33-70": ["run", "steps"],
    "gamma0-16-1": ["steps", "run", "mask+ub1"],
    "plant-all-l-33-7": _A, "plant-all-l-17-64": _B,
    "plant-one-l-33-7": _A + _R, "plant-one-l-16-2": _B, "plant-one-l-33-70": ["steps", "run"],
    "gamma1-33-7": _A, "gamma1-16-1": _B, "gamma2-33-7": _A, "gamma2-33-70": _B,
    "pi0-33-7": _A + ["r_tol"], "pi0-16-2": _B, "pi1-33-7": _A + ["r_tol"], "pi1-17-64": _B,
    "pi0+item-33-7": _A + ["r_tol"] + _R, "pi0+item-33-70": _B,
    "from-data-33-7": _A + _R, "from-data-16-2": _B,
    "firm-33-7": ["packed", "f_tol", "run+rec-nosure"] + _R, "firm-17-64": ["run"] + _R,
}
assert set(PLAN) == set(NT.SETS)
CASES = [(s, p) for (s, ps) in PLAN.items() for p in ps]
STEP_CASES = [(s, p) for (s, p) in CASES if p in STEP_FORMS]
PIPE_CASES = [(s, p) for (s, p) in CASES if p not in STEP_FORMS]


def engine(env, T, spec, S_B=None, lM=None):
    eng = env.GibbsEngine(up(env, T.S_B) if S_B is None else S_B, up(env, T.lM) if lM is None else lM, T.Nreg, T.U, T.G,
                          chain0=T.chain0, seed=T.seed, edge_index="symmetric", ctx=env.ctx, region_major=spec.get("region_major", True))
    eng.set_hyper(T.gamma, T.pi2)
    eng.import_state(T.f0, T.r0)
    return eng


def run_case(env, knobs, T, path, n_sweeps, S_B=None, lM=None):
    """Import the initial state, run n_sweeps through `path`, export; returns (f, r, f_repeats, engine, the rise of F_FORMS)."""
    spec = PATHS[path]
    knobs(**spec["knobs"])
    eng = engine(env, T, spec, S_B, lM)
    rep0 = env.ctx.stat("f_repeats")
    forms0 = [env.ctx.stat(k) for k in F_FORMS]
    if spec["driver"] == "steps":
        for s in range(n_sweeps):
            eng.f_step(T.sweep + s)
            eng.r_step(T.sweep + s)
    elif spec["driver"] == "sweeps":
        eng.sweeps(T.sweep, n_sweeps)
    else:
        eng.run(T.sweep, n_sweeps, mstep_every=0)
    (f_g, r_g) = eng.export_state()
    # no wait was given up, and the pipelined r pass itself ran where it fits the device (at U = 64, 70 its workgroups do
    # not, and the step-per-launch form is the default)
    assert env.ctx.stat("dev_err") == 0
    if spec.get("pipelined") and T.U <= 8:
        assert env.ctx.stat("r_form_last") == 2
    return f_g, r_g, env.ctx.stat("f_repeats") - rep0, eng, tuple(env.ctx.stat(k) - v for (k, v) in zip(F_FORMS, forms0))


F_FORMS = ("f_rec_passes", "f_sure_passes", "f_run_passes")


def expected_forms(T, path, n_sweeps):
    """The rise of F_FORMS over a call of n_sweeps on a REC_PATHS path: every sweep after the first reads the call's records;
    it runs the decided-tile path where the CPU's restatement of the record build's hint finds a decided tile, and that in
    the run form under f_runs = 2 only -- none of these tables has every tile decided, the auto choice's condition."""
    (hint, mode, _nan) = NT.decided_rule(T)
    n_tiles_open = any(len(t) and (mode[t] < 0).any() for t in FR.tiles(T.Nreg))
    assert n_tiles_open, "a set with every tile decided at the hint: the auto choice takes the run form too"
    n = n_sweeps - 1
    return (n, n if hint else 0, n if (hint and path == "run+rec+runs") else 0)


def report(T, s, f_g, r_g):
    """Per pattern of -inf among the oracle's log-weights of compared sweep s: the draws that differ, the first 20 named."""
    lines = []
    p = NT.f_pattern(T.cond_f[s])
    bad = f_g != T.f_after[s]
    for (i, name) in [(-1, "finite")] + list(enumerate(NT.PATTERNS)):
        m = bad & (p == i)
        if m.any():
            lines.append("f, -inf at %s: %d of %d draws differ" % (name, m.sum(), (p == i).sum()))
            for (g, c) in np.argwhere(m)[:20]:
                lines.append("   edge %d chain word %d lane %d: device %d, oracle %d, a = %s" % (c, g // 64, g % 64, f_g[g, c], T.f_after[s][g, c], T.cond_f[s][g, c]))
    rp = NT.r_pattern(T.cond_r[s])
    badr = r_g != T.r_after[s]
    for (i, name) in enumerate(("finite", "s0 = -inf", "s1 = -inf", "both -inf")):
        m = badr & (rp == i)
        if m.any():
            lines.append("r, %s: %d of %d draws differ" % (name, m.sum(), (rp == i).sum()))
            for (g, n, u) in np.argwhere(m)[:20]:
                lines.append("   region %d patient %d chain word %d lane %d: device %d, oracle %d, s = %s" % (n, u, g // 64, g % 64, r_g[g, n, u], T.r_after[s][g, n, u], T.cond_r[s][g, n, u]))
    return "\n".join(lines)


def check_sweeps(env, knobs, T, name, path, S_B=None, lM=None):
    """One sweep (a difference is named per pattern while the conditionals of the oracle still describe the device's
    draws), then two from the same start: the issue's check."""
    reps = 0
    for n_sweeps in (1, 2):
        (f_g, r_g, rep, _eng, forms) = run_case(env, knobs, T, path, n_sweeps, S_B, lM)
        reps = rep
        if path in REC_PATHS:
            assert forms == expected_forms(T, path, n_sweeps), (name, path, n_sweeps, forms)
        if not (np.array_equal(f_g, T.f_after[n_sweeps - 1]) and np.array_equal(r_g, T.r_after[n_sweeps - 1])):
            pytest.fail("%s / %s: %d f and %d r states differ from the oracle after %d sweep(s)\n%s"
                        % (name, path, int((f_g != T.f_after[n_sweeps - 1]).sum()), int((r_g != T.r_after[n_sweeps - 1]).sum()), n_sweeps,
                           report(T, 0, f_g, r_g) if n_sweeps == 1 else "(the first sweep alone agreed)"))
    # an edge whose log-odds are not finite in some lane takes the exact path: every such (chain word, edge) of both sweeps
    open_we = sum(int((NT.f_pattern(T.cond_f[s]) >= 0).reshape(T.G // 64, 64, T.C).any(axis=1).sum()) for s in range(2))
    print("%s / %s: f_repeats %d over two sweeps of %d wave-edges each, %d of them with a -inf log-weight" % (name, path, reps, (T.G // 64) * T.C, open_we))
    if path in COUNTS_REPEATS:
        assert reps >= open_we


@pytest.mark.parametrize("name,path", STEP_CASES)
def test_step_forms_equal_oracle(env, knobs, name, path):
    check_sweeps(env, knobs, NT.build_set(name), name, path)


@pytest.mark.parametrize("name,path", PIPE_CASES)
def test_pipelined_forms_equal_oracle(env, knobs, name, path):
    check_sweeps(env, knobs, NT.build_set(name), name, path)


@pytest.mark.parametrize("name", ["gamma0-16-2", "pi0-16-2"])
def test_mstep_leaves_the_zero_and_the_chains_stay_the_oracles(env, knobs, name):
    """run(mstep_every=1) sweep by sweep: the counts are the oracle's, the hyper block after each M-step is ln of
    O.gibbs_mstep (the clamps lift the zero) at rtol 1e-14, and the second sweep, on that hyper, is still the oracle's."""
    T = NT.build_set(name)
    eng = engine(env, T, PATHS["run"])
    (f, r) = (T.f0.copy(), T.r0.copy())
    (lng, lnpi2) = (T.lng, T.lnpi2)
    for s in range(2):
        counts = eng.run(T.sweep + s, 1, mstep_every=1, want_counts=True)
        counts = eng.host(counts)
        env.CO.gibbs_f_step(f, r, T.S_B, T.lM, lng, T.seed, T.sweep + s, T.chain0)
        env.CO.gibbs_r_step(f, r, T.lM, lnpi2, T.seed, T.sweep + s, BP.EDGE_SYMMETRIC, T.chain0)
        want = env.CO.gibbs_stats(f, r)
        assert np.array_equal(counts[:5], want[:5]), (name, s, counts[:5], want[:5])
        (pi, gamma) = O.gibbs_mstep(want, T.Nreg, T.U)
        (lng, lnpi2) = (np.log(gamma), np.log([1.0 - pi, pi]))
        hyper = eng.host(eng.hyper)
        assert np.isfinite(hyper[0:5]).all()
        nptest.assert_allclose(hyper[0:5], np.concatenate([lng, lnpi2]), rtol=1e-14, atol=0)
        (f_g, r_g) = eng.export_state()
        assert np.array_equal(f_g, f) and np.array_equal(r_g, r), "%s: chains differ after sweep %d" % (name, s + 1)
    assert env.ctx.stat("dev_err") == 0


def same_classes(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == -np.inf, b == -np.inf) and np.array_equal(a == np.inf, b == np.inf))


@pytest.mark.parametrize("name", ["item-16-2", "gamma0-16-2", "pi0-16-2", "plant-one-l-16-2", "from-data-16-2"])
def test_read_outs_at_the_final_state(env, knobs, name):
    """logjoint() and conditionals() at the oracle's state after two sweeps: NaN / -inf / +inf at the same places, finite
    log-joints at rtol 1e-12, finite pairwise logit differences at atol 1e-10 (the tolerances of test_gpu_exact_law.py)."""
    T = NT.build_set(name)
    eng = engine(env, T, PATHS["run"])
    eng.import_state(T.f2, T.r2)
    lj = eng.host(eng.logjoint())
    with np.errstate(invalid="ignore"):
        lj_o = env.CO.gibbs_logjoint(T.f2, T.r2, T.S_B, T.lM, T.lng, T.lnpi2)
    assert same_classes(lj, lj_o), name
    fin = np.isfinite(lj_o)
    nptest.assert_allclose(lj[fin], lj_o[fin], rtol=1e-12, atol=0)
    (cf, cr) = eng.conditionals()
    (cf, cr) = (eng.host(cf), eng.host(cr))
    cf_o = env.CO.gibbs_f_step(T.f2.copy(), T.r2, T.S_B, T.lM, T.lng, T.seed, 0, T.chain0, want_cond=True, draw=False)
    cr_o = env.CO.gibbs_r_step(T.f2, T.r2.copy(), T.lM, T.lnpi2, T.seed, 0, BP.EDGE_SYMMETRIC, T.chain0, want_cond=True, draw=False)
    assert same_classes(cf, cf_o) and same_classes(cr, cr_o), name
    print("%s: log-joints %d finite of %d; f conditionals %d -inf, r conditionals %d -inf" % (name, fin.sum(), len(lj), (cf_o == -np.inf).sum(), (cr_o == -np.inf).sum()))
    with np.errstate(invalid="ignore"):
        for (i, j) in ((0, 1), (0, 2), (1, 2)):
            (d, d_o) = (cf[..., i] - cf[..., j], cf_o[..., i] - cf_o[..., j])
            ok = np.isfinite(d_o)
            nptest.assert_allclose(d[ok], d_o[ok], rtol=0, atol=1e-10)
        (d, d_o) = (cr[..., 1] - cr[..., 0], cr_o[..., 1] - cr_o[..., 0])
        ok = np.isfinite(d_o)
        nptest.assert_allclose(d[ok], d_o[ok], rtol=0, atol=1e-10)


@pytest.mark.parametrize("name,path", [("from-data-33-7", "packed"), ("from-data-16-2", "anyU+rstep")])
def test_tables_from_data_built_on_the_device(env, knobs, name, path):
    """The library's table kernel on the same b, bt, theta: -inf exactly where the oracle's table has it (the underflow of
    N_0 at the outliers), and the sweeps FROM THE DEVICE-BUILT tables equal the oracle's on the oracle's tables -- a draw
    depends on the finite entries only through sums the other suites pin."""
    T = NT.build_set(name)
    (b, bt, theta, outl) = T.data
    (S_B, lM) = env.tables.build(env.ctx, up(env, b), up(env, bt), theta, 0)
    lM_h = lM.cpu().numpy()
    assert np.array_equal(lM_h == -np.inf, T.lM == -np.inf) and not np.isnan(lM_h).any() and not (lM_h == np.inf).any()
    assert np.array_equal((lM_h == -np.inf)[:, :, 0, 0], outl)
    check_sweeps(env, knobs, T, name, path, S_B=S_B, lM=lM)
