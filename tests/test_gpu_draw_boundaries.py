"""
The sampler's fast draws at their decision boundaries (run with -m gpu on an MI355X).

Every draw of the device kernels must be the draw of the exact fp64 formulas (fcd_draw_f / fcd_draw_r, the oracle's).  The hot
paths decide in fp32 and repeat a draw exactly only inside hand-derived margins: fcd_draw_f_fast32 with eta from
fcd_f32_sum_err / fcd_f32_offset_err, the no-exponential short-cut fcd_draw_f_sure, fcd_draw_f_fast of the generic kernel, and
the r pass's fp32 threshold fcd_logit_fast inside 16 FCD_LOGIT_FAST_ERR.  tests/boundary_probes.py builds tables that put one
draw per edge and per site at a KNOWN distance just inside or just outside those margins (test_boundary_probes.py pins the
builder on the CPU); here one or two sweeps run from the imported state and f and r of EVERY chain must equal the C oracle's,
in four table regimes (weak, model, heavy cancellation, shared-region-like) crossed with the forms of both passes.  A failure
names the probes that flipped.  Nothing here provokes a fault: all of it is arithmetic on valid states.

Counters.  fcd_ctx_stat("f_repeats") shows that the exact f path ran on the probe sets and stayed rare on the companion sets
whose probes all lie outside 1e-3 / 1e-2.  "r_exact_rows" is declared by the library but no r kernel feeds it (it reads 0); for
the r pass both sides of the margin follow from the kernel's own rule instead: |v| < tol with v within FCD_LOGIT_FAST_ERR of the
exact value, so a probe with |d| < tol - 2e-5 is re-decided exactly and one with |d| > tol + 2e-5 is not (margin_report()).
"""
import numpy as np
import pytest

import boundary_probes as BP

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


# f forms: default pair kernel (steps), its packed-tile form (sweeps, run), the any-U kernel (f_form 2; automatic at U = 70),
# the scalar-mask form (f_form 3), the generic kernel.  r forms: pipelined (default of sweeps / run), one launch per block
# step (r_path 3), one patient per panel workgroup (r_ub 1), one in-order workgroup (r_dsplit 1; it differs from the default
# above 8 chain words: the G = 2048 scan), generic.
PATHS = {
    "steps": dict(driver="steps", knobs={}),
    "packed": dict(driver="sweeps", knobs={}, pipelined=True),
    "run": dict(driver="run", knobs={}, pipelined="where it fits"),
    "anyU+rstep": dict(driver="sweeps", knobs={"f_form": 2, "r_path": 3}),
    "mask+ub1": dict(driver="sweeps", knobs={"f_form": 3, "r_ub": 1}),
    "dsplit": dict(driver="sweeps", knobs={"r_dsplit": 1}, pipelined=True),
    "generic": dict(driver="steps", knobs={}, region_major=False),
}
# not the full product: every regime meets every f form and every r form at least once
_A = ["steps", "packed", "dsplit", "generic"]
_B = ["mask+ub1", "anyU+rstep", "generic"]
_C = ["run", "anyU+rstep", "mask+ub1"]
COUNTS_REPEATS = ("steps", "packed", "run", "anyU+rstep", "dsplit")     # the pair kernels feed f_repeats, the other forms do not
PLAN = {"weak-33-7": _A, "weak-16-2": _B, "weak-33-70": _C,
        "model-33-7": _A, "model-16-64": _B, "model-33-2": _C,
        "heavy-33-7": _A, "heavy-16-70": _B, "heavy-33-64": _C,
        "shared-33-1": _A, "shared-16-1": _B + ["run"]}
CASES = [(s, p) for (s, ps) in PLAN.items() for p in ps]
SCAN_CASES = [(s, p) for s in BP.SCAN_SETS for p in ("steps", "packed", "anyU+rstep", "dsplit", "generic")]


def kernel_f_margin(P):
    """The pair kernel's ambiguity margin for every f probe, relative to sum(w), as fcd_common.h states it:
    2 eta (1 - p_mode) + FCD_DRAW_F_MARGIN with eta = fcd_draw_f_eta(fcd_f32_sum_err + fcd_f32_offset_err)."""
    e = P.f["edge"]
    d1 = np.abs(P.lM[e][:, :, 1:, :] - P.lM[e][:, :, :1, :]).max(axis=(2, 3)).sum(axis=1)       # sum_u max |record entry|
    c = (P.lng[1:] - P.lng[0])[None, :] + (P.S_B[e, 1:] - P.S_B[e, :1])
    cm = np.abs(c).max(axis=1)
    npair = (P.U + 1) // 2
    delta = (npair + 1) * 5.97e-8 * 1.01 * d1 + 2.0 * 5.97e-8 * 1.01 * (cm + d1)
    eta = np.expm1(2.0 * delta) * 1.001 + 2e-5
    a = BP.f_logits_ld(P.S_B, P.lM, P.lng, P.r0[P.f["chain"]], e)
    w = np.exp(a - a.max(axis=1, keepdims=True))
    p_mode = (1.0 / w.sum(axis=1)).astype(np.float64)
    return 2.0 * eta * (1.0 - p_mode) + 1e-6


def margin_report(P):
    mf = kernel_f_margin(P)
    df = np.abs(P.f["d"])
    plain = P.f["kind"] != 1
    (ins, outs) = (plain & (df < mf), plain & (df >= mf))
    dr = np.abs(P.r["d"])
    tol = 16 * 2e-5
    return dict(f_probes=int(plain.sum()), f_inside=int(ins.sum()), f_outside=int(outs.sum()),
                f_closest_fast=float(df[outs].min()) if outs.any() else None, f_margin_median=float(np.median(mf)),
                r_probes=len(dr), r_inside=int((dr < tol - 2e-5).sum()), r_outside=int((dr > tol + 2e-5).sum()),
                r_closest_fast=float(dr[dr > tol + 2e-5].min()) if (dr > tol + 2e-5).any() else None)


def run_case(env, knobs, P, path, n_sweeps=1):
    """Import the initial state, run n_sweeps through `path`, export; returns (f, r, f_repeats) of the device."""
    spec = PATHS[path]
    knobs(**spec["knobs"])
    eng = env.GibbsEngine(up(env, P.S_B), up(env, P.lM), P.Nreg, P.U, P.G, chain0=P.chain0, seed=P.seed, edge_index="symmetric",
                          ctx=env.ctx, region_major=spec.get("region_major", True))
    eng.set_hyper(P.gamma, P.pi2)
    eng.import_state(P.f0, P.r0)
    rep0 = env.ctx.stat("f_repeats")
    if spec["driver"] == "steps":
        for s in range(n_sweeps):
            eng.f_step(P.sweep + s)
            eng.r_step(P.sweep + s)
    elif spec["driver"] == "sweeps":
        eng.sweeps(P.sweep, n_sweeps)
    else:
        eng.run(P.sweep, n_sweeps, mstep_every=0)
    (f_g, r_g) = eng.export_state()
    # the pipelined r pass itself ran (not its fall-back; at U = 64, 70 its U + 16 ceil(U / 2) workgroups do not fit the
    # device at once and the step-per-launch form is the default) and no wait was given up
    assert env.ctx.stat("dev_err") == 0
    if spec.get("pipelined") is True or (spec.get("pipelined") and P.U <= 8):
        assert env.ctx.stat("r_form_last") == 2
    return f_g, r_g, env.ctx.stat("f_repeats") - rep0


def oracle_state(env, P, n_sweeps):
    """The C oracle's state after n_sweeps (the first is the builder's own: computed once per table set and left unchanged)."""
    (f, r) = (P.f1.copy(), P.r1.copy())
    for s in range(1, n_sweeps):
        env.CO.gibbs_f_step(f, r, P.S_B, P.lM, P.lng, P.seed, P.sweep + s, P.chain0)
        env.CO.gibbs_r_step(f, r, P.lM, P.lnpi2, P.seed, P.sweep + s, BP.EDGE_SYMMETRIC, P.chain0)
    return f, r


_ORACLE2 = {}


def check_against_oracle(env, P, name, path, f_g, r_g, n_sweeps):
    if n_sweeps == 1:
        (f_o, r_o) = (P.f1, P.r1)
    else:
        if name not in _ORACLE2:
            _ORACLE2[name] = oracle_state(env, P, n_sweeps)
        (f_o, r_o) = _ORACLE2[name]
    if np.array_equal(f_g, f_o) and np.array_equal(r_g, r_o):
        return
    # name the probes that flipped (state after the FIRST sweep decides; after two sweeps a flip has spread)
    lines = []
    if n_sweeps == 1:
        pf = P.f
        bad = np.flatnonzero(f_g[pf["chain"], pf["edge"]] != pf["outcome"])
        for i in bad[:20]:
            lines.append("f probe kind=%s edge=%d d=%+.3e thr=%d x=%.9g lead=%.2f lane=%d word=%d: device %d, oracle %d"
                         % (("f", "sure", "floor")[pf["kind"][i]], pf["edge"][i], pf["d"][i], pf["thr"][i], pf["x"][i], pf["lead"][i],
                            pf["chain"][i] % 64, pf["chain"][i] // 64, f_g[pf["chain"][i], pf["edge"][i]], pf["outcome"][i]))
        pr = P.r
        badr = np.flatnonzero(r_g[pr["chain"], pr["n"], pr["u"]] != pr["outcome"])
        for i in badr[:20]:
            lines.append("r probe site=(%d, %d) d=%+.3e x=%.9g extreme=%s lane=%d word=%d: device %d, oracle %d"
                         % (pr["n"][i], pr["u"][i], pr["d"][i], pr["x"][i], bool(pr["extreme"][i]), pr["chain"][i] % 64,
                            pr["chain"][i] // 64, r_g[pr["chain"][i], pr["n"][i], pr["u"][i]], pr["outcome"][i]))
        lines.insert(0, "%d f probes and %d r probes flipped" % (len(bad), len(badr)))
    pytest.fail("%s / %s (regime %s): %d f and %d r states differ from the oracle after %d sweep(s)\n%s"
                % (name, path, P.regime, int((f_g != f_o).sum()), int((r_g != r_o).sum()), n_sweeps, "\n".join(lines)))


@pytest.mark.parametrize("name,path", CASES)
def test_probed_sweep_equals_oracle(env, knobs, name, path):
    """One sweep on the probed tables, and on the shapes with one block of regions a second, ordinary one after it: every
    chain equals the oracle's."""
    P = BP.build_set(name)
    (f_g, r_g, reps) = run_case(env, knobs, P, path, 1)
    rep = margin_report(P)
    print("%s / %s: f_repeats %d of %d wave-edges, r_exact_rows stat %d, %s" % (name, path, reps, ((P.G + 63) // 64) * P.C,
                                                                               env.ctx.stat("r_exact_rows"), rep))
    check_against_oracle(env, P, name, path, f_g, r_g, 1)
    if P.Nreg == 16:
        (f_g, r_g, _reps) = run_case(env, knobs, P, path, 2)
        check_against_oracle(env, P, name, path, f_g, r_g, 2)
    # both sides of each margin were met: probes inside (the exact path ran) and outside
    assert rep["f_inside"] >= 20 and rep["f_outside"] >= 10 and rep["r_outside"] >= 3
    assert rep["r_inside"] >= 10 or P.U == 1
    assert reps > 0 or path not in COUNTS_REPEATS


@pytest.mark.parametrize("name,path", SCAN_CASES)
def test_extreme_uniform_scan_equals_oracle(env, knobs, name, path):
    """G = 2048: the draws with x next to 0 and 1 of a whole f pass, leads of 12 .. 18 nats about fcd_draw_f_sure's 15.01, and
    the all-but-one-hot floor probes that only FCD_DRAW_F_MARGIN protects."""
    P = BP.build_set(name)
    (f_g, r_g, reps) = run_case(env, knobs, P, path, 1)
    k = P.f["kind"]
    print("%s / %s: %d sure probes (%d not the argmax), %d floor probes, f_repeats %d" %
          (name, path, (k == 1).sum(), ((k == 1) & (P.f["outcome"] != P.f["argmax"])).sum(), (k == 2).sum(), reps))
    check_against_oracle(env, P, name, path, f_g, r_g, 1)
    assert reps > 0 or path not in COUNTS_REPEATS


@pytest.mark.parametrize("name", list(BP.FAR_SETS))
@pytest.mark.parametrize("path", ["packed", "anyU+rstep"])
def test_far_probes_are_decided_by_the_fast_path(env, knobs, name, path):
    """Companion sets: every probe at least 1e-3 (f) / 1e-2 (r) from its threshold.  Same chains as the oracle, and fewer
    than 5 % of the (edge, chain word) items repeat in fp64."""
    P = BP.build_set(name)
    (f_g, r_g, reps) = run_case(env, knobs, P, path, 1)
    wave_edges = ((P.G + 63) // 64) * P.C
    rep = margin_report(P)
    print("%s / %s: f_repeats %d of %d wave-edges; %s" % (name, path, reps, wave_edges, rep))
    check_against_oracle(env, P, name, path, f_g, r_g, 1)
    assert rep["r_inside"] == 0 and np.abs(P.f["d"]).min() >= 1e-3 and np.abs(P.r["d"]).min() >= 1e-2
    assert reps < 0.05 * wave_edges


def test_probe_census(env):
    """Per regime: the probes, how many fall inside / outside the kernels' margins, the closest one the fast path decides
    (the figures of DESIGN.md, printed with -s)."""
    for regime in BP.REGIMES:
        reps = [margin_report(BP.build_set(n)) for (n, s) in BP.SETS.items() if s[0] == regime]
        tot = {k: sum(r[k] for r in reps) for k in ("f_probes", "f_inside", "f_outside", "r_probes", "r_inside", "r_outside")}
        tot["f_closest_fast"] = min(r["f_closest_fast"] for r in reps if r["f_closest_fast"] is not None)
        tot["r_closest_fast"] = min([r["r_closest_fast"] for r in reps if r["r_closest_fast"] is not None], default=None)
        print(regime, tot)
        assert tot["f_inside"] >= 100 and tot["f_outside"] >= 100
