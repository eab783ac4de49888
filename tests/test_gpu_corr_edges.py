"""
K_corr (fcd_corr.hip behind fcdiff_amd.corr.correlations) against the extended-precision reference of tests/corr_ref.py,
aimed at the kernels' seams: the 208 / 209 switch between the one-workgroup-per-subject kernel and the 64 x 64 block
kernel, T around the 16- and 32-sample steps, the split of the time axis in slices (uneven and empty ones), the reuse
of the tickets across calls, rows whose first sample says nothing about their level, non-finite samples, Fisher z and
the Python wrapper.

Every comparison uses the bound the project documents for this kernel, rtol 1e-11 / atol 1e-13 (corr_ref.BOUND), and
Fisher z the rtol 1e-10 of test_corr_front_end_against_numpy.  corr_form 0 is the automatic choice (subject kernel up
to 208 regions), corr_form 1 the block kernel everywhere.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import corr_ref as R

pytestmark = pytest.mark.gpu

FORMS = (0, 1)
FISHER = dict(rtol=1e-10, atol=1e-13)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.corr import correlations
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib, e.O, e.correlations) = (torch, fcdiff_amd, _lib, O, correlations)
    e.ctx = _lib.Context()
    # what fcd_ctx_create reads into ctx->num_cu
    e.num_cu = int(torch.cuda.get_device_properties(e.ctx.device).multi_processor_count)
    return e


@pytest.fixture
def knobs(env):
    """Set knobs of the shared context (fcd_ctx_set_knob) for one test; all back to default afterwards."""
    touched = []

    def set_(**kw):
        for (k, v) in kw.items():
            env.ctx.set_knob(k, v)
            touched.append(k)
    yield set_
    for k in touched:
        env.ctx.set_knob(k, 0)


def series(seed, S, N, T, level=0.0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((S, N, T)) + 0.7 * rs.standard_normal((S, 1, T)) + level * rs.standard_normal((S, N, 1))


def check(got, exp, what):
    assert got.shape == exp.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what
    ok = ~np.isnan(exp)
    nptest.assert_allclose(got[ok], exp[ok], err_msg=what, **R.BOUND)
    assert got[ok].min() >= -1.0 and got[ok].max() <= 1.0, what


# ---------------------------------------------------------------------------------------------------------------------
# the switch between the kernels, tile padding
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [207, 208, 209, 210, 16, 17, 32, 33, 129])
def test_kernel_switch_and_tile_padding(env, knobs, N):
    """208 regions are the last shape of the subject kernel (13 tile rows, 91 of its 96 tile slots), 209 the first of
    the block kernel; 16 / 17 and 32 / 33 step over a tile edge, 129 reaches the second group of staging rows."""
    (S, T) = (2, 40)
    ts = series(N, S, N, T, level=3.0)
    exp = R.corr_edges_ld(ts)
    for form in FORMS:
        knobs(corr_form=form)
        check(env.correlations(ts, ctx=env.ctx), exp, "Nreg %d form %d" % (N, form))


# ---------------------------------------------------------------------------------------------------------------------
# T around the steps of 16 and 32 samples
# ---------------------------------------------------------------------------------------------------------------------
T_SEAMS = (2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 97)


@pytest.mark.parametrize("N", [5, 70])
def test_t_seams(env, knobs, N):
    """Odd T (8-byte loads) and even T (16-byte loads), the clamped last load, a last half-step of 16 that is empty."""
    S = 3
    for T in T_SEAMS:
        ts = series(100 * N + T, S, N, T, level=2.0)
        exp = R.corr_edges_ld(ts)
        for form in FORMS:
            knobs(corr_form=form)
            check(env.correlations(ts, ctx=env.ctx), exp, "Nreg %d T %d form %d" % (N, T, form))


# ---------------------------------------------------------------------------------------------------------------------
# the split of the time axis (subject kernel)
# ---------------------------------------------------------------------------------------------------------------------
def slice_plan(num_cu, S, T):
    """(KS, steps per slice, slices that hold a step) as fcd_corr_edges and corr_gram_subject_kernel work them out."""
    steps = (T + 31) // 32
    KS = num_cu // S
    KS = min(KS, steps // 2)
    KS = max(KS, 1)
    KS = min(KS, 16)
    per = (steps + KS - 1) // KS
    used = (steps + per - 1) // per
    return (KS, per, used)


def slice_cases(num_cu):
    """(S, T) pairs for: one slice; two slices; sixteen uneven slices; slice counts whose last slices are empty."""
    cases = {}
    cases["one slice"] = (num_cu // 2 + 1, 200)
    cases["two slices"] = (max(num_cu // 2, 1), 200)
    cases["sixteen uneven slices"] = (max(num_cu // 16, 1), 47 * 32 - 5)            # 47 steps: 15 slices of 3, one of 2
    empties = []
    for k in range(2, 17):
        S = num_cu // k
        if S < 1:
            continue
        for steps in range(2 * k, 2 * k + 24):
            T = 32 * steps - 31
            (KS, _per, used) = slice_plan(num_cu, S, T)
            if used < KS and not any(e[2] == KS for e in empties):
                empties.append((S, T, KS))
                break
    # two of them are enough: the smallest and the largest slice count with an empty tail
    for e in ([empties[0], empties[-1]] if len(empties) > 1 else empties):
        cases["%d slices, empty tail" % e[2]] = (e[0], e[1])
    return cases


def test_slice_cases_for_256_cus():
    """The derivation gives what the kernel's author worked out by hand for 256 CUs."""
    assert slice_plan(256, 64, 288) == (4, 3, 3)
    assert slice_plan(256, 16, 1025) == (16, 3, 11)
    c = slice_cases(256)
    assert slice_plan(256, *c["one slice"])[0] == 1 and slice_plan(256, *c["two slices"])[0] == 2
    assert slice_plan(256, *c["sixteen uneven slices"]) == (16, 3, 16)
    assert any("empty" in k for k in c)


def test_slice_split(env, knobs):
    cases = slice_cases(env.num_cu)
    plans = {k: slice_plan(env.num_cu, *v) for (k, v) in cases.items()}
    print("num_cu %d: %s" % (env.num_cu, {k: (cases[k], plans[k]) for k in cases}))
    assert plans["one slice"][0] == 1
    assert plans["two slices"][0] == 2 and plans["two slices"][2] == 2
    (KS, per, used) = plans["sixteen uneven slices"]
    assert KS == 16 and used == 16 and (cases["sixteen uneven slices"][1] + 31) // 32 != 16 * per
    assert any(p[2] < p[0] for p in plans.values()), "no (S, T) with an empty slice on a device with %d CUs" % env.num_cu
    N = 20
    knobs(corr_form=0)
    for (name, (S, T)) in cases.items():
        ts = series(S + T, S, N, T, level=5.0)
        check(env.correlations(ts, ctx=env.ctx), R.corr_edges_ld(ts), "%s: S %d T %d plan %s" % (name, S, T, plans[name]))


# ---------------------------------------------------------------------------------------------------------------------
# tickets across calls, determinism, a refused call
# ---------------------------------------------------------------------------------------------------------------------
def test_ticket_reuse_and_determinism(env):
    """One context of its own: the tickets are allocated for 5 subjects, grow for 40, and are reused for 5 and 3; each
    launch must find them at zero.  Every call has several slices per subject (else no ticket is drawn)."""
    ctx = env.lib.Context()
    try:
        (N, T) = (12, 300)
        for form in FORMS:
            ctx.set_knob("corr_form", form)
            for S in (5, 40, 5, 3):
                assert slice_plan(env.num_cu, S, T)[0] > 1
                ts = series(10 * S + form, S, N, T, level=4.0)
                check(env.correlations(ts, ctx=ctx), R.corr_edges_ld(ts), "S %d form %d" % (S, form))
            # same bits whoever comes last: sixteen slices of many subjects, twice
            S = max(env.num_cu // 16, 1)
            ts = series(77, S, N, 1499, level=4.0)
            first = env.correlations(ts, ctx=ctx)
            assert np.array_equal(first, env.correlations(ts, ctx=ctx)), "form %d" % form
            check(first, R.corr_edges_ld(ts), "repeat, form %d" % form)
            # a call refused for its shape leaves the next one right
            with pytest.raises(ValueError):
                env.correlations(np.zeros((3, N, 1)), ctx=ctx)
            ts = series(78, 3, N, T)
            check(env.correlations(ts, ctx=ctx), R.corr_edges_ld(ts), "after the refusal, form %d" % form)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# rows whose first sample is far from their level
# ---------------------------------------------------------------------------------------------------------------------
_atypical = {}


def atypical(variant, T):
    if (variant, T) not in _atypical:
        ts = R.atypical_input(variant, T)
        _atypical[(variant, T)] = (ts, R.corr_edges_ld(ts))
    return _atypical[(variant, T)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T", R.ATYPICAL_T)
@pytest.mark.parametrize("variant", R.ATYPICAL_VARIANTS)
def test_atypical_first_sample(env, knobs, variant, T, form):
    """
    S = 2, Nreg = 16, unit noise plus a shared component on mean 100; (a) frame 0 moved by +-1000 sd, (b) frames 0-3
    decaying from +50 sd.  numpy.corrcoef is at 5e-15 on these inputs (tests/test_corr_ref.py).  A subject kernel that
    shifts every row by its FIRST sample is emulated at 1.4e-11 (a, T = 20001) and 7.9e-11 (a, T = 60001), outside the
    bound; shifted by the median of eight samples spread over the row it is at numpy's error.  Measured on one MI355X,
    worst |error| of form 0 with the first-sample shift / with the median shift: a 1200 5.9e-13 / 1.8e-15, a 20001
    1.76e-11 (failed) / 6.2e-15, a 60001 8.76e-11 (failed) / 9.0e-15, b 1200 4.0e-13 / 1.4e-15, b 20001 2.1e-12 / 8.3e-16,
    b 60001 3.2e-12 / 8.3e-16; form 1 (means in a pass of their own) 4.8e-15 ... 2.8e-14 on the six inputs.
    """
    (ts, exp) = atypical(variant, T)
    knobs(corr_form=form)
    got = env.correlations(ts, ctx=env.ctx)
    (err, frac) = R.worst_excess(got, exp, **R.BOUND)
    print("atypical first sample: variant %s T %d form %d: worst |error| %.3e = %.4f of the bound" % (variant, T, form, err, frac))
    check(got, exp, "variant %s T %d form %d" % (variant, T, form))


# ---------------------------------------------------------------------------------------------------------------------
# non-finite samples
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fisher_z", [False, True])
def test_non_finite_samples(env, knobs, fisher_z):
    """One NaN and one +Inf sample in two rows of subject 1: exactly the edges of those rows, of that subject, are NaN."""
    (S, N, T) = (3, 20, 100)
    ts = series(9, S, N, T)
    ts[1, 5, 37] = np.nan
    ts[1, 12, 70] = np.inf
    exp = R.corr_edges_ld(ts, fisher_z=fisher_z)
    ends = env.O.edge_endpoints(N)
    touched = np.isin(ends[:, 0], (5, 12)) | np.isin(ends[:, 1], (5, 12))
    assert not np.isnan(exp[:, [0, 2]]).any() and np.array_equal(np.isnan(exp[:, 1]), touched)
    for form in FORMS:
        knobs(corr_form=form)
        got = env.correlations(ts, fisher_z=fisher_z, ctx=env.ctx)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), "form %d" % form
        ok = ~np.isnan(exp)
        nptest.assert_allclose(got[ok], exp[ok], err_msg="form %d" % form, **(FISHER if fisher_z else R.BOUND))


# ---------------------------------------------------------------------------------------------------------------------
# Fisher z
# ---------------------------------------------------------------------------------------------------------------------
def test_fisher_z(env, knobs):
    """atanh against the long-double one; an exactly collinear pair (corr_ref.exact_collinear_input: every intermediate
    is exact in fp64) gives -inf / +inf on both sides."""
    ts = series(21, 3, 11, 150, level=2.0)
    exp = R.corr_edges_ld(ts, fisher_z=True)
    tc = R.exact_collinear_input()
    expc = R.corr_edges_ld(tc, fisher_z=True)
    assert expc[0, 0] == -np.inf and expc[1, 0] == np.inf and expc[2, 0] == -np.inf
    for form in FORMS:
        knobs(corr_form=form)
        nptest.assert_allclose(env.correlations(ts, fisher_z=True, ctx=env.ctx), exp, err_msg="form %d" % form, **FISHER)
        with np.errstate(invalid="ignore"):
            got = env.correlations(tc, fisher_z=True, ctx=env.ctx)
        assert np.array_equal(np.isinf(got), np.isinf(expc)) and np.array_equal(got[:3], expc[:3]), "form %d" % form
        nptest.assert_allclose(got[3:], expc[3:], err_msg="form %d" % form, **FISHER)


# ---------------------------------------------------------------------------------------------------------------------
# the wrapper
# ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_inputs(env, knobs):
    t = env.torch
    (S, N, T) = (3, 9, 50)
    ts32 = series(31, S, N, T).astype(np.float32)
    ts = np.ascontiguousarray(ts32, dtype=np.float64)
    for form in FORMS:
        knobs(corr_form=form)
        base = env.correlations(ts, ctx=env.ctx)
        check(base, R.corr_edges_ld(ts), "form %d" % form)
        # float32: a NumPy array and a tensor
        assert np.array_equal(env.correlations(ts32, ctx=env.ctx), base)
        assert np.array_equal(env.correlations(t.from_numpy(ts32), ctx=env.ctx), base)
        # views that are not contiguous: every other region of a larger array, a transposed tensor on the device
        big = np.zeros((S, 2 * N, T))
        big[:, ::2, :] = ts
        big[:, 1::2, :] = -7.0
        view = big[:, ::2, :]
        assert not view.flags["C_CONTIGUOUS"]
        assert np.array_equal(env.correlations(view, ctx=env.ctx), base)
        dev = t.as_tensor(np.ascontiguousarray(ts.transpose(0, 2, 1)), device=env.ctx.device).transpose(1, 2)
        assert not dev.is_contiguous() and tuple(dev.shape) == (S, N, T)
        out = env.correlations(dev, ctx=env.ctx, as_numpy=False)
        assert isinstance(out, t.Tensor) and out.is_cuda and out.dtype == t.float64 and tuple(out.shape) == (N * (N - 1) // 2, S)
        assert np.array_equal(out.cpu().numpy(), base)
    with pytest.raises(ValueError):
        env.correlations(ts[0], ctx=env.ctx)
