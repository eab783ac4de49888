"""
The baselines on the device on exact, tied and degenerate data, against tests/baseline_exact_ref.py (rational arithmetic) and,
for the normative scores, tests/baseline_ref.py.  tests/test_gpu_baseline.py and tests/test_gpu_network.py cover the launch
geometry on data where nothing is close; here every comparison that the statistics are defined by (>= against the observed
value, a strict > against the threshold) meets exact ties, and connections without variance or without within-group variance
meet the rules that fcdiff_amd.baseline documents for them.

Tolerances.  On integer rows Q and A are exact in doubles.  g = A^2 kf takes two roundings, Q - g one more, amplified by
g / (Q - g) = t^2 / dof; with the product by dof and the division, t^2 is within 8 (1 + t^2 / dof) 2^-52 relative of the
rational value, t within half of that; region sums and maxima within the largest bound among their terms plus (N - 1) 2^-52.
Derived, not measured; each test prints the worst ratio of error to bound.  Real-valued rows (D2's non-dyadic connection under
the permuted labellings, the normative cases) keep rtol 1e-10.  Counts, bits, components and p-values are compared exactly,
which baseline_exact_ref.Exact.check_conditions makes legitimate (asserted without a device in tests/test_baseline_exact.py
and again here before the device is asked).
"""
import math

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_exact_ref as XR
import baseline_ref as BR

pytestmark = pytest.mark.gpu

FLOATS = ("t", "region", "null_max_t", "null_max_region")
GROUP_EXACT = ("count_t", "count_region", "p_t", "p_region", "p_fwe_t", "p_fwe_region")
NET_EXACT = ("edge_mask", "component", "component_label", "component_edges", "component_regions", "null_max_extent",
             "null_max_regions", "null_n_edges", "p_fwe", "p_fwe_region")
NET_CASES = [(name, thr, tail) for name in sorted(XR.CASES) for thr in XR.THRESHOLDS for tail in XR.TAILS] + \
            [("E4", 2.0, tail) for tail in XR.TAILS]                # the boundary itself: t^2 == threshold^2 on two connections
TAIL_CODE = {"both": 0, "greater": 1, "less": 2}
RTOL = 1e-10
GAP = 1e-9


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.bl = torch, fcdiff_amd, _lib, baseline
    e.ctx = _lib.Context()
    return e


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def held(case, key, got, want, bound, skip=None):
    """NaN and infinite values at the same places and equal; elsewhere |got - want| <= bound |want|.  Prints the worst ratio
    of error to bound.  skip: entries left to the caller."""
    (got, want, bound) = (np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound))
    assert got.shape == want.shape == bound.shape, key
    use = np.ones(want.shape, dtype=bool) if skip is None else ~skip
    (got, want, bound) = (got[use], want[use], bound[use])
    special = ~np.isfinite(want)
    assert same(got[special], want[special]) and np.isfinite(got[~special]).all(), "%s %s: NaN or inf elsewhere" % (case, key)
    err = np.abs(got[~special] - want[~special])
    lim = bound[~special] * np.abs(want[~special])
    with np.errstate(all="ignore"):
        ratio = np.where(err > 0, err / lim, 0.0)
    print("%s %s: worst error / bound %.3g over %d values" % (case, key, float(ratio.max()) if ratio.size else 0.0, ratio.size))
    assert (err <= lim).all(), "%s %s" % (case, key)


def regions_of(env, c):
    return list(env.pkg.util.c_to_nm(c))


def abi_bits(env, k, threshold, tail, labels):
    """(P, C) bool from fcd_baseline_network_bits; labels None: the observed labelling, P = 1."""
    t = env.torch
    C = k.b.shape[0]
    W = (C + 31) // 32
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device="cuda")
    (bd, btd) = (dev(k.b), dev(k.bt))
    labd = None if labels is None else dev(labels)
    P = 1 if labels is None else labels.shape[0]
    bits = t.full((P, W), -1, dtype=t.int32, device="cuda")
    env.ctx.call("fcd_baseline_network_bits", env.lib.dptr(bd), env.lib.dptr(btd), C, k.H, k.U, env.lib.dptr(labd), P,
                 float(threshold), TAIL_CODE[tail], env.lib.dptr(bits), env.lib.dptr(None), env.lib.stream_ptr())
    got = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert not got[:, C:].any()
    return got[:, :C].astype(bool)


# ---- group_test ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(XR.CASES))
def test_group_test_against_the_exact_reference(env, name):
    (k, ex) = XR.case(name)
    ex.check_conditions(thresholds=k.thresholds, boundary=k.boundary)
    ref = XR.group(name)
    bounds = ex.bounds()
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    assert set(out) == set(ref) | {"labels"} and np.array_equal(out["labels"], k.labels)
    skip_c = np.zeros(ex.C, dtype=bool)
    skip_n = np.zeros(ex.N, dtype=bool)
    for c in k.rounding_c:
        skip_c[c] = True
        skip_n[regions_of(env, c)] = True
        # no exact outcome is fixed: not NaN, the sign of the difference, huge or infinite
        assert out["t"][c] * k.rounding_sign[c] > 1e6 and (out["region"][regions_of(env, c)] > 1e12).all()
    skips = {"t": skip_c, "region": skip_n, "null_max_t": None, "null_max_region": None}
    for key in FLOATS:
        held(name, key, out[key], ref[key], bounds[key], skips[key])
    for key in ("count_t", "count_region"):
        assert out[key].dtype == np.int64, key
    for key in GROUP_EXACT:
        nptest.assert_array_equal(out[key], ref[key], err_msg="%s %s" % (name, key))
    # repeated calls agree bit for bit, degenerate values included
    again = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    assert all(same(out[key], again[key]) for key in out)


@pytest.mark.parametrize("name", ["E1", "E2", "D1", "D2"])
def test_observed_rows_reproduce_the_observed_statistics(env, name):
    """A row equal to the observed labelling gives the observed maxima bit for bit, constant and separated connections or not."""
    (k, _ex) = XR.case(name)
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    for r in k.obs_rows:
        assert out["null_max_t"][r] == np.nanmax(np.abs(out["t"])) and out["null_max_region"][r] == out["region"].max()
    for thr in k.thresholds:
        obs = abi_bits(env, k, thr, "both", None)[0]
        rows = abi_bits(env, k, thr, "both", k.labels)
        assert all(np.array_equal(rows[r], obs) for r in k.obs_rows)


def test_e2_complement_rows(env):
    """H == U: the complement of the observed labelling has A = -A on every connection, an exact tie of every statistic."""
    (k, _ex) = XR.case("E2")
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    base = env.bl.group_test(k.b, k.bt, labels=k.base_labels, ctx=env.ctx)
    extra = len(k.comp_rows) + len(k.obs_rows)
    assert np.array_equal(out["count_t"], base["count_t"] + extra)
    assert np.array_equal(out["count_region"], base["count_region"] + extra)
    assert same(out["t"], base["t"]) and same(out["region"], base["region"])
    for r in k.comp_rows:
        assert out["null_max_t"][r] == np.abs(out["t"]).max() and out["null_max_region"][r] == out["region"].max()
    for thr in k.thresholds:
        obs = dict((tail, abi_bits(env, k, thr, tail, None)[0]) for tail in XR.TAILS)
        rows = dict((tail, abi_bits(env, k, thr, tail, k.labels)) for tail in XR.TAILS)
        assert obs["both"].any() and obs["greater"].any() and obs["less"].any()
        assert np.array_equal(obs["both"], obs["greater"] | obs["less"]) and not (obs["greater"] & obs["less"]).any()
        for r in k.comp_rows:
            assert np.array_equal(rows["both"][r], obs["both"])
            assert np.array_equal(rows["greater"][r], obs["less"]) and np.array_equal(rows["less"][r], obs["greater"])


def test_e3_rows_that_differ_between_duplicate_subjects(env):
    """Two labellings that differ only between subjects with equal data give bit-identical results."""
    (k, _ex) = XR.case("E3")
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    for (ra, rb) in k.pair_rows:
        assert out["null_max_t"][ra] == out["null_max_t"][rb] and out["null_max_region"][ra] == out["null_max_region"][rb]
    for thr in k.thresholds:
        for tail in XR.TAILS:
            rows = abi_bits(env, k, thr, tail, k.labels)
            net = env.bl.network_test(k.b, k.bt, thr, labels=k.labels, tail=tail, ctx=env.ctx)
            for (ra, rb) in k.pair_rows:
                assert np.array_equal(rows[ra], rows[rb])
                assert net["null_max_extent"][ra] == net["null_max_extent"][rb]
                assert net["null_n_edges"][ra] == net["null_n_edges"][rb]


def test_e4_threshold_boundary_through_the_c_abi(env):
    """t^2 = 4.0 exactly on connections 0 (A = 4) and 1 (A = -4): clear at threshold 2.0, because > is strict, set just below."""
    (k, ex) = XR.case("E4")
    ex.check_conditions(thresholds=(2.0,), boundary=(2.0,))
    below = math.nextafter(2.0, 0.0)
    tie = k.tie_row
    for tail in XR.TAILS:
        want = ex.bits(2.0, tail)
        assert np.array_equal(abi_bits(env, k, 2.0, tail, None)[0], want[0]), tail
        assert np.array_equal(abi_bits(env, k, 2.0, tail, k.labels), want[1:]), tail
        want = ex.bits(below, tail)
        assert np.array_equal(abi_bits(env, k, below, tail, None)[0, :2], want[0, :2]), tail
        assert np.array_equal(abi_bits(env, k, below, tail, k.labels)[tie, :2], want[1 + tie, :2]), tail
    assert not ex.bits(2.0, "both")[0, :2].any() and ex.bits(below, "both")[0, :2].all()
    assert ex.bits(below, "greater")[0, :2].tolist() == [True, False] and ex.bits(below, "less")[0, :2].tolist() == [False, True]
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    assert (out["t"][0], out["t"][1]) == (2.0, -2.0) and out["count_t"][0] == XR.group("E4")["count_t"][0] >= 1


def test_d1_constant_connections(env):
    """The documented values, spelled out: NaN t, nothing to any sum, maximum, count or bit; a dead region has p_region = 1.
    Without the rule a constant connection makes t^2 = 0 * dof / (0 - 0) = NaN, the region sums of both its endpoints NaN and
    their p_region = 1 / (1 + P); a constant that is not dyadic (0.3) leaves Q about 1e-33 and a t of rounding noise."""
    (k, ex) = XR.case("D1")
    P = k.labels.shape[0]
    dead = np.array(ex.const)
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    assert np.array_equal(np.isnan(out["t"]), dead) and (out["count_t"][dead] == 0).all()
    assert np.isnan(out["p_t"][dead]).all() and np.isnan(out["p_fwe_t"][dead]).all()
    assert np.isfinite(out["t"][~dead]).all() and np.isfinite(out["t"][k.half_constant_c])
    n = k.dead_region
    assert (out["region"][n], out["count_region"][n], out["p_region"][n]) == (0.0, P, 1.0)
    for key in ("region", "null_max_t", "null_max_region", "p_region", "p_fwe_region"):
        assert np.isfinite(out[key]).all(), key
    assert (out["p_region"] > 1.0 / (1.0 + P)).all()          # what a NaN region sum would give: the smallest p there is
    for tail in XR.TAILS:
        net = env.bl.network_test(k.b, k.bt, 1.5, labels=k.labels, tail=tail, ctx=env.ctx)
        assert np.array_equal(np.isnan(net["t"]), dead) and not net["edge_mask"][dead].any()
        assert not abi_bits(env, k, 1.5, tail, k.labels)[:, dead].any()
        assert net["component"][n] == -1 and math.isnan(net["p_fwe_region"][n])


def test_d2_separation(env):
    (k, _ex) = XR.case("D2")
    P = k.labels.shape[0]
    out = env.bl.group_test(k.b, k.bt, labels=k.labels, ctx=env.ctx)
    c = k.separated_c
    assert out["t"][c] == math.inf and (out["region"][[0, 1]] == math.inf).all() and out["count_t"][c] == 1
    assert (out["count_region"][[0, 1]] == 1).all() and (out["p_region"][[0, 1]] == 2.0 / (1.0 + P)).all()
    assert out["null_max_t"][k.obs_rows[0]] == math.inf and out["null_max_region"][k.obs_rows[0]] == math.inf
    for key in out:
        assert not np.isnan(out[key]).any(), key
    assert (out["region"] >= 0).all() and (out["null_max_region"] >= 0).all()
    for tail in XR.TAILS:
        net = env.bl.network_test(k.b, k.bt, 2.5, labels=k.labels, tail=tail, ctx=env.ctx)
        assert not np.isnan(net["t"]).any()
        for (cc, sign) in [(c, 1.0)] + sorted(k.rounding_sign.items()):
            assert net["edge_mask"][cc] == (tail == "both" or (tail == "greater") == (sign > 0)), (tail, cc)


# ---- network_test ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,thr,tail", NET_CASES)
def test_network_test_against_the_exact_reference(env, name, thr, tail):
    (k, ex) = XR.case(name)
    ex.check_conditions(thresholds=(thr,), boundary=k.boundary)
    ref = XR.network(name, thr, tail)
    out = env.bl.network_test(k.b, k.bt, thr, labels=k.labels, tail=tail, ctx=env.ctx)
    assert set(out) == set(ref) | {"labels"}
    skip_c = np.zeros(ex.C, dtype=bool)
    for c in k.rounding_c:
        skip_c[c] = True
        assert out["t"][c] * k.rounding_sign[c] > 1e6
    held("%s %g %s" % (name, thr, tail), "t", out["t"], ref["t"], ex.bounds()["t"], skip_c)
    for key in NET_EXACT:
        assert out[key].dtype == ref[key].dtype and out[key].shape == ref[key].shape, key
        nptest.assert_array_equal(out[key], ref[key], err_msg=key)
    assert out["threshold"] == thr and out["tail"] == tail and np.array_equal(out["labels"], k.labels)


# ---- normative: a deviation of exactly 0 -----------------------------------------------------------------------------------

def normative_data(N, H, U, seed, missing):
    """
    normal(0.3, 0.1) with three rows replaced (dyadic values, so their sums are exact on the device and in the reference):
    row 1  every control 0.25: the deviation is 0, nobody is scored there
    row 2  every control 0.5 but control 1 at 0.75: the others' deviation is 0 for control 1 alone
    With `missing`, NaN at a few places, and row 0 constant over its observed controls only.
    """
    rng = np.random.default_rng(seed)
    C = N * (N - 1) // 2
    b = rng.normal(0.3, 0.1, (C, H))
    bt = rng.normal(0.3, 0.1, (C, U))
    b[1] = 0.25
    b[2] = 0.5
    b[2, 1] = 0.75
    if missing:
        b[0] = -1.5
        b[0, [0, H - 2]] = np.nan
        b[1, H - 1] = np.nan
        b[2, 0] = np.nan
        bt[2, U - 1] = np.nan
    return b, bt


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("shape", [(7, 5, 4, 21), (3, 1024, 3, 22), (3, 1000, 3, 23)])
def test_normative_with_a_deviation_of_zero(env, shape, missing):
    """(7, 5, 4): controls and patients side by side in one block of 64 subjects.  (3, 1024, 3) is the limit: 1024 controls
    fill the LDS row and sixteen blocks, the three patients are the first lanes of a seventeenth.  (3, 1000, 3): the last
    block holds controls 960 .. 999 and the three patients side by side."""
    (N, H, U, seed) = shape
    (b, bt) = normative_data(N, H, U, seed, missing)
    ref = BR.normative(b, bt)
    out = env.bl.normative(b, bt, missing_data=missing, return_z=True, ctx=env.ctx)
    assert set(out) == set(ref)
    for key in ("z", "z0", "msq", "msq0", "max0"):
        assert np.array_equal(np.isnan(out[key]), np.isnan(ref[key])), key
        nptest.assert_allclose(out[key], ref[key], rtol=RTOL, atol=0, err_msg=key)
    for key in ("n_edges", "n_over", "n_edges0", "n_over0", "n_controls"):
        assert np.array_equal(out[key], ref[key]), key
    # the documented outcome, spelled out on the device's arrays
    assert np.isnan(out["z"][1]).all() and np.isnan(out["z0"][1]).all()
    h_seen = np.flatnonzero(~np.isnan(b[2]))
    assert np.isnan(out["z0"][2, 1]) and not np.isnan(out["z0"][2, h_seen[h_seen != 1]]).any()
    assert not np.isnan(out["z"][2, :U - 1]).any() and np.isnan(out["z"][2, U - 1]) == missing
    assert np.isnan(out["z"][0]).all() == missing
    dead = [1] + ([0] if missing else [])
    touched = np.zeros(N, dtype=np.int64)
    for c in dead:
        touched[regions_of(env, c)] += 1
    full = N - 1 - touched
    assert np.array_equal(out["n_edges"][:, 0], full) and (out["n_edges"] <= full[:, None]).all()
    assert BR.smallest_gap(ref["max0"], ref["msq"]) > GAP
    assert min(BR.smallest_gap(ref["msq0"][n], ref["msq"][n]) for n in range(N)) > GAP
    nptest.assert_array_equal(out["p_region"], ref["p_region"])
    nptest.assert_array_equal(out["p_fwe"], ref["p_fwe"])
