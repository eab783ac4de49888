"""
The exact reference of the baselines (baseline_exact_ref.py) without a GPU: against the loop-level references baseline_ref.py
and network_ref.py on data without ties, its own arithmetic on the cases worked by hand, and, for every named case of
tests/test_gpu_baseline_exact.py, the conditions under which exact comparison with the device is legitimate.  Also the host
half of group_test() on the reference's arrays, and the refusal of non-finite data, which runs before any context exists.
"""
import math
from fractions import Fraction

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_exact_ref as XR
import baseline_ref as BR
import network_ref as NR
from fcdiff_amd import baseline

GROUP_KEYS = ("t", "region", "null_max_t", "null_max_region", "count_t", "count_region", "p_t", "p_region", "p_fwe_t",
              "p_fwe_region")


@pytest.mark.parametrize("shape", [BR.SHAPES[0], BR.SHAPES[1], BR.SHAPES[3]])
def test_exact_reference_against_the_loop_level_references(shape):
    (b, bt, labels, ex) = XR.plain_case(shape)
    ref = BR.group_test(b, bt, labels)
    got = ex.group_test()
    assert set(got) == set(GROUP_KEYS) == set(ref) - {"null_t", "null_region"}
    for k in GROUP_KEYS:
        if k.startswith("count"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), k
        else:
            nptest.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    assert ex.ties() == (0, 0) and not any(ex.const) and not any(ex.integer)
    ex.check_conditions(thresholds=(1.5, 2.5))
    t_pair = NR.group_t(b, bt, labels)
    for (thr, tail) in ((1.5, "both"), (2.5, "both"), (1.5, "greater"), (1.5, "less")):
        nref = NR.network_test(b, bt, labels, thr, tail, t_pair=t_pair)
        ngot = ex.network_test(thr, tail)
        assert set(ngot) == set(nref) - {"null_t", "null_components"}
        nptest.assert_allclose(ngot["t"], nref["t"], rtol=1e-12, atol=0)
        for k in set(ngot) - {"t", "threshold", "tail"}:
            assert ngot[k].dtype == nref[k].dtype, k
            nptest.assert_array_equal(ngot[k], nref[k], err_msg=k)
        assert (ngot["threshold"], ngot["tail"]) == (nref["threshold"], nref["tail"])


def test_e4_arithmetic_is_exact():
    """t^2 of connection 0 is 4.0 exactly, in Fractions and in the doubles the device works in, step by step."""
    (k, ex) = XR.case("E4")
    assert (ex.A[0][0], ex.A[0][1], ex.Q[0], ex.Q[1], ex.kf, ex.dof) == (4, -4, 20, 20, Fraction(1, 2), 6)
    assert ex.t2[0][0] == ex.t2[0][1] == Fraction(4)
    (A, Q, kf, dof) = (4.0, 20.0, 8.0 / (4.0 * 4.0), 6.0)
    gq = A * A * kf
    assert (kf, gq, Q - gq, gq * dof / (Q - gq)) == (0.5, 8.0, 12.0, 4.0)
    tie = 1 + k.tie_row
    assert abs(ex.A[tie][0]) == 4 and abs(ex.A[tie][1]) == 4 and not ex.same_row(tie)
    g = XR.group("E4")
    assert (g["t"][0], g["t"][1]) == (2.0, -2.0)
    for (thr, want) in ((2.0, False), (math.nextafter(2.0, 0.0), True)):
        assert ex.bits(thr, "both")[0, :2].tolist() == [want, want]
        assert ex.bits(thr, "greater")[0, :2].tolist() == [want, False]
        assert ex.bits(thr, "less")[0, :2].tolist() == [False, want]
        assert ex.bits(thr, "both")[tie, :2].tolist() == [want, want]
    assert ex.integer_count_t()[0] >= 1


@pytest.mark.parametrize("name", sorted(XR.CASES))
def test_conditions_hold_for_every_case(name):
    (k, ex) = XR.case(name)
    ex.check_conditions(thresholds=k.thresholds, boundary=k.boundary)
    g = XR.group(name)
    ints = ex.integer_count_t()
    at = ints >= 0
    assert np.array_equal(g["count_t"][at], ints[at])
    (tt, tr) = ex.ties()
    print("%s: %d ties in count_t, %d in count_region" % (name, tt, tr))
    if name in XR.TIED:
        assert all(ex.integer) and tt >= k.min_ties[0] and tr >= k.min_ties[1]
    # no NaN from defined input, and the documented values of the constant connections
    dead = np.array(ex.const)
    assert np.array_equal(np.isnan(g["t"]), dead) and np.array_equal(np.isnan(g["p_t"]), dead)
    assert np.array_equal(np.isnan(g["p_fwe_t"]), dead) and (g["count_t"][dead] == 0).all()
    for key in ("region", "null_max_t", "null_max_region", "p_region", "p_fwe_region"):
        assert not np.isnan(g[key]).any(), key
    assert (g["region"] >= 0).all()


def test_e2_complement_rows_tie_everything():
    (k, ex) = XR.case("E2")
    g = XR.group("E2")
    base = XR.Exact(k.b, k.bt, k.base_labels).group_test()
    extra = len(k.comp_rows) + len(k.obs_rows)
    assert np.array_equal(g["count_t"], base["count_t"] + extra)
    assert np.array_equal(g["count_region"], base["count_region"] + extra)
    for r in k.comp_rows:
        assert np.array_equal(k.labels[r], 1 - XR.observed_row(k.H, k.U))
        assert all(a == -o for (a, o) in zip(ex.A[1 + r], ex.A[0]))
        assert g["null_max_t"][r] == np.abs(g["t"]).max() and g["null_max_region"][r] == g["region"].max()
        assert np.array_equal(ex.bits(1.5, "both")[1 + r], ex.bits(1.5, "both")[0])
        assert np.array_equal(ex.bits(1.5, "greater")[1 + r], ex.bits(1.5, "less")[0])


def test_e3_duplicate_subjects_and_label_pairs():
    (k, ex) = XR.case("E3")
    X = np.concatenate([k.b, k.bt], axis=1)
    assert np.array_equal(X[:, 127], X[:, 128]) and np.array_equal(X[:, k.H - 1], X[:, k.H])
    assert sorted(r for pair in k.pair_rows for r in pair) == list(range(20))
    for (ra, rb) in k.pair_rows:
        differ = np.flatnonzero(k.labels[ra] != k.labels[rb]).tolist()
        assert differ in ([127, 128], [k.H - 1, k.H], [])
        assert ex.A[1 + ra] == ex.A[1 + rb]


def test_d1_and_d2_reference_values():
    (k, ex) = XR.case("D1")
    g = XR.group("D1")
    P = k.labels.shape[0]
    assert np.flatnonzero(ex.const).tolist() == k.constant_c and not ex.const[k.half_constant_c]
    n = k.dead_region
    assert (g["region"][n], g["count_region"][n], g["p_region"][n]) == (0.0, P, 1.0)
    assert np.isfinite(g["t"][k.half_constant_c])
    (k, ex) = XR.case("D2")
    g = XR.group("D2")
    assert ex.t2[0][k.separated_c] == math.inf and g["t"][k.separated_c] == math.inf
    assert (g["region"][[0, 1]] == math.inf).all() and g["count_t"][k.separated_c] == 1
    assert (g["count_region"][[0, 1]] == 1).all() and g["null_max_t"][k.obs_rows[0]] == math.inf
    assert (g["p_region"][[0, 1]] == 2.0 / (1.0 + k.labels.shape[0])).all()


def test_loop_level_references_follow_the_rules_for_degenerate_connections():
    """baseline_ref.group_test and network_ref.network_test on D1 (constant connections) and on D2's integer connection."""
    (k, ex) = XR.case("D1")
    (ref, g) = (BR.group_test(k.b, k.bt, k.labels), XR.group("D1"))
    for key in GROUP_KEYS:
        if key.startswith("count") or key.startswith("p_"):
            nptest.assert_array_equal(ref[key], g[key], err_msg=key)
        else:
            assert np.array_equal(np.isnan(ref[key]), np.isnan(g[key])), key
            nptest.assert_allclose(ref[key], g[key], rtol=1e-12, atol=0, err_msg=key)
    (nref, ngot) = (NR.network_test(k.b, k.bt, k.labels, 1.5), XR.network("D1", 1.5, "both"))
    for key in set(ngot) - {"t", "threshold", "tail"}:
        nptest.assert_array_equal(nref[key], ngot[key], err_msg=key)
    (k, ex) = XR.case("D2")
    ref = BR.group_test(k.b, k.bt, k.labels)
    c = k.separated_c
    assert ref["t"][c] == math.inf and (ref["region"][[0, 1]] == math.inf).all() and ref["count_t"][c] == 1
    assert not any(np.isnan(ref[key]).any() for key in GROUP_KEYS) and (ref["count_region"][[0, 1]] == 1).all()


def test_host_pvalues_on_degenerate_values():
    """baseline.group_pvalues on the exact reference's arrays: NaN t, infinite statistics, inf >= inf."""
    for name in ("D1", "D2", "E2"):
        g = XR.group(name)
        pv = baseline.group_pvalues(g["t"], g["region"], g["null_max_t"], g["null_max_region"], g["count_t"], g["count_region"])
        for key in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
            nptest.assert_array_equal(pv[key], g[key], err_msg="%s %s" % (name, key))


def test_non_finite_data_is_refused():
    rng = np.random.default_rng(0)
    (b, bt) = (rng.normal(size=(6, 5)), rng.normal(size=(6, 4)))
    for bad in (np.inf, -np.inf, np.nan):
        for (x, y) in ((0, 1), (1, 0)):
            args = [b.copy(), bt.copy()]
            args[x][2, 1] = bad
            with pytest.raises(ValueError, match="infinite"):
                baseline.group_test(*args)
            with pytest.raises(ValueError, match="infinite"):
                baseline.network_test(*args, 2.0)
            with pytest.raises(ValueError, match="infinite"):
                baseline.normative(*args)
            if not math.isnan(bad):
                with pytest.raises(ValueError, match="infinite"):
                    baseline.normative(*args, missing_data=True)
