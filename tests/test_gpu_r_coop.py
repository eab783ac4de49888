"""
The pipelined r pass launched cooperatively (knob r_coop = 1), and its fall-back to one launch per block step after the
runtime refuses that launch (test hook r_coop = 2: the launch acts as refused and launches nothing).

The pipelined form is correct only if every workgroup of its grid is resident at once.  The library checks that with the
occupancy query (stats pipe_grid / pipe_capacity: the grid of the last pipelined attempt, empty workgroups included, and
the workgroups resident at once for it); a cooperative launch has the runtime check it too.  The two must agree, and the
fall-back -- which starts after the sweep has already laid the pipelined form's marks and sentinels out -- must walk the
C oracle's chains bit for bit, in one call and across calls that change the form.
"""
import math

import numpy as np
import numpy.testing as nptest
import pytest


pytestmark = pytest.mark.gpu

SLOT_MARGIN = 8         # free workgroup slots the pipelined form insists on (R_PIPE_SLOT_MARGIN)
R_NB = 16               # regions per block of the r pass


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
    e.num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return e


@pytest.fixture
def knobs(env):
    """Set knobs of the shared context for one test; all back to default afterwards."""
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


def tables_for(env, N, H, U, seed):
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


class Case:
    """Tables, one engine on the shared context, and the oracle's chains of the same shape, seed and first chain."""

    def __init__(self, env, N, U, G, mode="symmetric", chain0=64, seed=None, n_oracle=None):
        self.env, self.N, self.U, self.G, self.mode, self.chain0 = env, N, U, G, mode, chain0
        self.seed = 31 + N + 7 * U if seed is None else seed
        (self.m, self.S_B, self.lM) = tables_for(env, N, 3, U, seed=N + U)
        self.Go = G if n_oracle is None else n_oracle
        self.lng, self.lnpi2 = np.log(self.m.gamma), np.log(self.m.pi2())
        self.eng = env.GibbsEngine(up(env, self.S_B), up(env, self.lM), N, U, G, chain0=chain0, seed=self.seed,
                                   edge_index=mode, ctx=env.ctx)
        self.oracle = [env.CO.gibbs_init(self.Go, N, U, 0.3, self.seed, chain0)]     # oracle[s]: state after s sweeps

    def restart(self):
        self.eng.set_hyper(self.m.gamma, self.m.pi2())
        self.eng.init(0.3)

    def oracle_after(self, s):
        while len(self.oracle) <= s:
            (f, r) = (a.copy() for a in self.oracle[-1])
            sw = len(self.oracle) - 1
            self.env.CO.gibbs_f_step(f, r, self.S_B, self.lM, self.lng, self.seed, sw, self.chain0)
            self.env.CO.gibbs_r_step(f, r, self.lM, self.lnpi2, self.seed, sw, self.env.lib.EDGE_MODES[self.mode], self.chain0)
            self.oracle.append((f, r))
        return self.oracle[s]

    def assert_oracle(self, s, what=""):
        (f_g, r_g) = self.eng.export_state()
        (f_o, r_o) = self.oracle_after(s)
        nptest.assert_array_equal(f_g[:self.Go], f_o, err_msg="f after sweep %d %s" % (s, what))
        nptest.assert_array_equal(r_g[:self.Go], r_o, err_msg="r after sweep %d %s" % (s, what))

    def run_with_everything(self, n_sweeps):
        """fcd_gibbs_run with an M-step every sweep, marginal counters, pair and count-histogram accumulators attached."""
        self.restart()
        self.eng.attach_pair_accumulator(every=1)
        self.eng.attach_count_accumulator(every=1)
        self.eng.cnt_f.zero_()
        self.eng.cnt_r.zero_()
        counts = self.eng.run(0, n_sweeps, mstep_every=1, accumulate_from=1, want_counts=True)
        host = self.eng.host
        out = dict(counts=host(counts).copy(), hyper=host(self.eng.hyper).copy(), cnt_f=host(self.eng.cnt_f).copy(),
                   cnt_r=host(self.eng.cnt_r).copy(), pair=self.eng.pair_counts_host().copy())
        (out["hist_patient"], out["hist_region"]) = (h.copy() for h in self.eng.count_hist_host())
        (out["f"], out["r"]) = self.eng.export_state()
        self.eng.detach_pair_accumulator()
        self.eng.detach_count_accumulator()
        return out


def assert_same_run(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        nptest.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def plan_grid(env, U, G, ub, dsplit_knob=0):
    """The pipelined form's grid as fcd_gibbs_r_pass first asks for it: nD in-order + nP panel + npad empty workgroups."""
    GW = (G + 63) // 64
    wpb = min(GW, 16)
    (nD, nP) = (U, R_NB * ((U + ub - 1) // ub))
    npad = nD if (nD <= env.num_cu and nD + nP > env.num_cu) else 0
    if dsplit_knob != 1 and wpb > 8 and 2 * nD <= env.num_cu:
        (nD, npad) = (2 * U, 0)
    return nD, nP, npad


def assert_checked(env, what):
    """What the library checked for its last pipelined attempt: the whole grid with the margin inside the capacity."""
    (grid, cap) = (env.ctx.stat("pipe_grid"), env.ctx.stat("pipe_capacity"))
    assert grid > 0 and cap > 0, what
    assert grid + SLOT_MARGIN <= cap, "%s: grid %d + %d > capacity %d" % (what, grid, SLOT_MARGIN, cap)
    return grid, cap


# The seven shapes of test_gpu_parity.py::test_gibbs_r_pass_pipelined: two edge modes, one and two patients per panel
# workgroup, a single block, two groups of chain words, a short last block, cfg 3 (its first 64 chains compared).
PIPE_SHAPES = [(40, 9, 128, "symmetric", 0), (33, 21, 1024, "reference", 0), (70, 12, 200, "symmetric", 1),
               (16, 3, 64, "symmetric", 0), (12, 2, 2048, "symmetric", 0), (97, 5, 1024, "symmetric", 0),
               (200, 50, 1024, "symmetric", 0)]


@pytest.mark.parametrize("N,U,G,mode,ub", PIPE_SHAPES)
def test_cooperative_launch_equals_oracle_and_plain_launch(env, knobs, N, U, G, mode, ub):
    """
    r_coop = 1: the same chains as the oracle over 3 sweeps, in the pipelined form (the runtime accepted the grid the plan
    accepted), no wait given up; and a run with an M-step every sweep, counters and both accumulators gives the plain
    launch's hyper-parameters, counts and accumulators bit for bit.
    """
    knobs(r_ub=ub)
    c = Case(env, N, U, G, mode, n_oracle=(64 if N >= 200 else None))
    runs = {}
    for coop in (1, 0):
        env.ctx.set_knob("r_coop", coop)
        try:
            c.restart()
            c.eng.run(0, 3, mstep_every=0)
            c.assert_oracle(3, "r_coop=%d" % coop)
            assert env.ctx.stat("r_form_last") == 2, "r_coop=%d" % coop
            assert env.ctx.stat("dev_err") == 0
            assert_checked(env, "r_coop=%d" % coop)
            runs[coop] = c.run_with_everything(3)
            assert env.ctx.stat("r_form_last") == 2 and env.ctx.stat("dev_err") == 0
        finally:
            env.ctx.set_knob("r_coop", 0)
    assert_same_run(runs[1], runs[0], "cooperative against plain launch")
    assert runs[1]["counts"][4] == G


def _boundary_shapes(env):
    """
    [(N, U, G, knobs, nD + nP, npad, capacity)]: the first where the empty workgroups cross the capacity (npad > 8 and
    nD + nP + 8 <= capacity < nD + nP + npad: one in-order workgroup per patient, r_dsplit = 1 at 16 chain words), then
    the largest two-in-order-workgroup (dsplit) grid that still fits.  The capacity is asked of the library at U = 2 (the
    same LDS and threads per workgroup as every U >= 2 at this N and G).
    """
    out = []
    N = 40
    for (G, kn) in ((1024, dict(r_dsplit=1)), (1024, {})):
        for (k, v) in kn.items():
            env.ctx.set_knob(k, v)
        try:
            c = Case(env, N, 2, G)
            c.restart()
            c.eng.r_step(0)
            cap = env.ctx.stat("pipe_capacity")
        finally:
            for k in kn:
                env.ctx.set_knob(k, 0)
        fits = []
        for U in range(2, env.num_cu + 1):
            (nD, nP, npad) = plan_grid(env, U, G, 2, kn.get("r_dsplit", 0))
            if kn:
                if npad > SLOT_MARGIN and nD + nP + SLOT_MARGIN <= cap < nD + nP + npad:
                    out.append((N, U, G, kn, nD + nP, npad, cap))
                    break
            elif npad == 0 and nD + nP + SLOT_MARGIN <= cap:
                fits.append((N, U, G, kn, nD + nP, npad, cap))
        if fits:
            out.append(fits[-1])
    return out


def test_runtime_agrees_with_the_plan_at_the_residency_boundary(env, knobs):
    """
    Where the plan picks the pipelined form, the runtime must accept the same grid cooperatively (r_form_last == 2 with
    r_coop = 1), and what the plan checked must be the grid that is launched: with its empty workgroups where they fit,
    without them where only they do not.  Shapes: the empty workgroups across the capacity, and a dsplit grid just inside
    it; one past that dsplit grid the plan itself refuses.
    """
    shapes = _boundary_shapes(env)
    assert [s[5] > SLOT_MARGIN for s in shapes] == [True, False], "boundary shapes not found: %r" % (shapes,)
    for (N, U, G, kn, grid, npad, cap) in shapes:
        what = "N=%d U=%d G=%d %r (grid %d + %d empty, capacity %d)" % (N, U, G, kn, grid, npad, cap)
        knobs(**kn)
        c = Case(env, N, U, G)
        for coop in (0, 1):
            env.ctx.set_knob("r_coop", coop)
            try:
                c.restart()
                c.eng.run(0, 2, mstep_every=0)
                c.assert_oracle(2, what)
                assert env.ctx.stat("r_form_last") == 2, "r_coop=%d: %s" % (coop, what)
                assert env.ctx.stat("dev_err") == 0
                assert assert_checked(env, what) == (grid, cap), what      # (the empty workgroups dropped)
            finally:
                env.ctx.set_knob("r_coop", 0)
        for k in kn:
            env.ctx.set_knob(k, 0)
    # one patient more than the dsplit grid that fits: the plan refuses, both launches run the step form
    (N, U, G, kn, grid, npad, cap) = shapes[1]
    c = Case(env, N, U + 1, G)
    for coop in (0, 1):
        env.ctx.set_knob("r_coop", coop)
        try:
            c.restart()
            c.eng.run(0, 1, mstep_every=0)
            c.assert_oracle(1)
            assert env.ctx.stat("r_form_last") == 1
            assert env.ctx.stat("pipe_grid") + SLOT_MARGIN > env.ctx.stat("pipe_capacity")
        finally:
            env.ctx.set_knob("r_coop", 0)


# Fall-back after a refusal: U <= 64 pair form (the packed path from the second sweep of a call on), the any-U pair kernel
# of the f pass (f_form = 2: the packing launch in every sweep), reference edge ids, one group of chain words, more than 16
# chain words (two in-order workgroups per patient: dsplit), a short last block of regions.
FALLBACK_SHAPES = [(40, 9, 128, "symmetric", {}), (17, 5, 64, "symmetric", dict(f_form=2)),
                   (33, 21, 1024, "reference", {}), (16, 3, 64, "symmetric", {}), (33, 7, 1100, "symmetric", {}),
                   (70, 12, 200, "symmetric", {})]


@pytest.mark.parametrize("N,U,G,mode,kn", FALLBACK_SHAPES)
def test_fallback_after_refusal_equals_oracle_and_step_form(env, knobs, N, U, G, mode, kn):
    """
    r_coop = 2 (every pipelined launch acts as refused): the plan accepts the pipelined form, lays its marks and sentinels
    out, and the pass then runs one launch per block step.  Chains equal the oracle's after each of 1..4 sweeps of one
    fcd_gibbs_run call, r_form_last == 1, no wait given up; with M-step, counters and accumulators the run equals
    r_path = 3 (the step form from the start) bit for bit.
    """
    knobs(**kn)
    c = Case(env, N, U, G, mode)
    # the plan does accept the pipelined form here: the refusal is what sends the pass to the step form
    c.restart()
    c.eng.run(0, 1, mstep_every=0)
    assert env.ctx.stat("r_form_last") == 2
    assert_checked(env, "default")
    knobs(r_coop=2)
    for n in range(1, 5):
        c.restart()
        n_pack = env.ctx.stat("pack_launches")
        c.eng.run(0, n, mstep_every=0)
        c.assert_oracle(n, "r_coop=2, %d sweeps in one call" % n)
        assert env.ctx.stat("r_form_last") == 1
        assert env.ctx.stat("dev_err") == 0
        assert_checked(env, "r_coop=2")
        # (after a refused pass the step form has overwritten the sentinels: every sweep packs and writes them again)
        assert env.ctx.stat("pack_launches") - n_pack == n
    refused = c.run_with_everything(4)
    assert env.ctx.stat("r_form_last") == 1 and env.ctx.stat("dev_err") == 0
    knobs(r_coop=0, r_path=3)
    step = c.run_with_everything(4)
    assert env.ctx.stat("r_form_last") == 1
    assert_same_run(refused, step, "refused pipelined launch against r_path=3")
    assert refused["counts"][4] == G


@pytest.mark.parametrize("N,U,G", [(40, 9, 128), (33, 7, 1100)])
@pytest.mark.parametrize("first", ["refused", "default"])
def test_form_changes_between_calls(env, knobs, N, U, G, first):
    """
    One engine and context: k sweeps with r_coop = 2, k with the default, k with r_coop = 2 again (and the same starting
    from the default).  Stale sentinels or marks left by the form of the call before would show as chains that leave the
    oracle's.
    """
    k = 2
    c = Case(env, N, U, G)
    c.restart()
    order = ["refused", "default", "refused"] if first == "refused" else ["default", "refused", "default"]
    try:
        for (i, form) in enumerate(order):
            env.ctx.set_knob("r_coop", 2 if form == "refused" else 0)
            c.eng.run(i * k, k, mstep_every=0)
            c.assert_oracle((i + 1) * k, "after call %d (%s)" % (i, form))
            assert env.ctx.stat("r_form_last") == (1 if form == "refused" else 2), form
            assert env.ctx.stat("dev_err") == 0
    finally:
        env.ctx.set_knob("r_coop", 0)


@pytest.mark.parametrize("form,kn", [("pipelined", {}), ("cooperative", dict(r_coop=1)), ("refused", dict(r_coop=2)),
                                     ("step", dict(r_path=3))])
@pytest.mark.parametrize("N,U,G", [(40, 9, 128), (70, 12, 200)])
def test_profiler_pairs_match_the_launches(env, knobs, form, kn, N, U, G):
    """
    prof_collect() (what bench.py's per-kernel numbers come from): one f pair per sweep, one pack pair per packing launch,
    one r pair per sweep for the pipelined and cooperative launch, one per non-empty block step (ceil(Nreg/16) + 1 per
    sweep) for the step form and after a refusal -- the refused launch itself adds none.  Every duration is positive.
    """
    knobs(**kn)
    n_sw = 3
    c = Case(env, N, U, G)
    c.restart()
    env.torch.cuda.synchronize()
    env.ctx.prof_enable(True)
    try:
        n_pack = env.ctx.stat("pack_launches")
        c.eng.run(0, n_sw, mstep_every=0)
        got = env.ctx.prof_collect()
    finally:
        env.ctx.prof_enable(False)
    c.assert_oracle(n_sw, form)
    assert env.ctx.stat("r_form_last") == (2 if form in ("pipelined", "cooperative") else 1)
    r_per_sweep = 1 if form in ("pipelined", "cooperative") else math.ceil(N / R_NB) + 1
    want = {"lik_kernel": 0, "gibbs_f_pair_kernel": n_sw, "gibbs_r_step_kernel": n_sw * r_per_sweep,
            "pack_f_kernel": env.ctx.stat("pack_launches") - n_pack}
    assert {k: v[1] for (k, v) in got.items()} == want, form
    assert want["pack_f_kernel"] >= 1
    for (k, (ms, n)) in got.items():
        if n:
            assert math.isfinite(ms) and ms > 0, (k, ms)
