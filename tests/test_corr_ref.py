"""
CPU tests of tests/corr_ref.py: the extended-precision reference the K_corr GPU tests compare against, and the fp64
restatement of the subject kernel's shifted formula.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import corr_ref as R
from oracle import fcdiff_oracle as O


def test_longdouble_is_wider_than_double():
    """The reference is only a reference where long double carries more than fp64's 53 bits (x86-64: 64)."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


@pytest.mark.parametrize("S,N,T", [(3, 10, 200), (2, 37, 53), (1, 2, 2), (2, 17, 1201)])
@pytest.mark.parametrize("fisher_z", [False, True])
def test_reference_agrees_with_numpy_on_benign_input(S, N, T, fisher_z):
    rs = np.random.RandomState(S * 1000 + N)
    ts = rs.standard_normal((S, N, T)) + 0.7 * rs.standard_normal((S, 1, T))
    if T == 2:
        ts[:, :, 1] = ts[:, :, 0] + np.where(rs.rand(S, N) < 0.5, -1.0, 1.0)        # correlations of exactly +-1
        fisher_z = False
    exp = O.corr_edges(ts, fisher_z=fisher_z)
    got = R.corr_edges_ld(ts, fisher_z=fisher_z)
    assert got.shape == (N * (N - 1) // 2, S) and got.dtype == np.float64
    nptest.assert_allclose(got, exp, rtol=1e-13, atol=1e-13)
    assert np.abs(R.corr_edges_ld(ts)).max() <= 1.0


def test_reference_edge_order():
    """Edge c of subject s is the correlation of regions (n, m) = edge_endpoints[c]."""
    rs = np.random.RandomState(3)
    ts = rs.standard_normal((2, 6, 40))
    got = R.corr_edges_ld(ts)
    ends = O.edge_endpoints(6)
    for (c, (n, m)) in enumerate(ends):
        for s in range(2):
            nptest.assert_allclose(got[c, s], np.corrcoef(ts[s, n], ts[s, m])[0, 1], rtol=1e-13, atol=1e-15)


def test_reference_nan_pattern_of_a_constant_row():
    (S, N, T) = (3, 20, 50)
    rs = np.random.RandomState(4)
    ts = rs.standard_normal((S, N, T))
    ts[1, 5, :] = 2.5
    with np.errstate(invalid="ignore", divide="ignore"):
        exp = O.corr_edges(ts)
    for fz in (False, True):
        got = R.corr_edges_ld(ts, fisher_z=fz)
        assert np.isnan(exp).sum() == N - 1 and np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    nptest.assert_allclose(R.corr_edges_ld(ts)[ok], exp[ok], rtol=1e-13, atol=1e-13)


def test_reference_nan_pattern_of_non_finite_samples():
    """A NaN sample and an infinite sample make exactly the edges of their rows NaN, in that subject only."""
    (S, N, T) = (2, 7, 30)
    ts = np.random.RandomState(5).standard_normal((S, N, T))
    ts[1, 2, 11] = np.nan
    ts[1, 4, 0] = np.inf
    got = R.corr_edges_ld(ts)
    ends = O.edge_endpoints(N)
    touched = np.isin(ends[:, 0], (2, 4)) | np.isin(ends[:, 1], (2, 4))
    assert not np.isnan(got[:, 0]).any() and np.array_equal(np.isnan(got[:, 1]), touched)


def test_fisher_z_of_an_exactly_collinear_pair_is_infinite():
    ts = R.exact_collinear_input()
    z = R.corr_edges_ld(ts, fisher_z=True)
    c = R.corr_edges_ld(ts)
    assert c[0, 0] == -1.0 and c[1, 0] == 1.0 and c[2, 0] == -1.0
    assert z[0, 0] == -np.inf and z[1, 0] == np.inf and z[2, 0] == -np.inf
    assert np.isfinite(z[3:]).all()


@pytest.mark.parametrize("variant", R.ATYPICAL_VARIANTS)
@pytest.mark.parametrize("T", R.ATYPICAL_T)
def test_numpy_meets_the_bound_on_the_atypical_first_sample_inputs(variant, T):
    """What makes the bound of the GPU test fair: numpy.corrcoef, the kernel's oracle everywhere else, stays inside it
    (by three orders) on the very inputs where the first sample is no estimate of the row's level."""
    ts = R.atypical_input(variant, T)
    exp = R.corr_edges_ld(ts)
    got = O.corr_edges(ts)
    nptest.assert_allclose(got, exp, **R.BOUND)
    assert R.worst_excess(got, exp, **R.BOUND)[1] < 1e-2


def test_what_the_shift_does():
    """
    The record of why the subject kernel does not shift by the first sample: in fp64 the shifted one-pass formula loses
    about T * 2^-53 * (shift - mean)^2 / variance.  With frame 0 moved 1000 sd the first-sample shift is outside the bound
    at T = 20001 and T = 60001; the median of eight samples spread over the row is at numpy's error at every T.
    """
    for variant in R.ATYPICAL_VARIANTS:
        for T in R.ATYPICAL_T:
            ts = R.atypical_input(variant, T)
            exp = R.corr_edges_ld(ts)
            first = R.worst_excess(R.shift_form(ts, R.first_sample_shift(ts)), exp, **R.BOUND)
            med = R.worst_excess(R.shift_form(ts, R.median8_shift(ts)), exp, **R.BOUND)
            print("variant %s T %6d: first-sample shift %.2e (%.3f of the bound), median-of-8 shift %.2e (%.5f)"
                  % (variant, T, first[0], first[1], med[0], med[1]))
            assert med[1] < 1e-2
            assert first[0] > 30 * med[0]
            if variant == "a" and T >= 20001:
                assert first[1] > 1.0


def test_median8_shift_is_a_sample_of_the_row():
    ts = R.atypical_input("a", 1200)
    m = R.median8_shift(ts)
    pos = R.spread_positions(1200)
    assert pos[0] > 0 and pos[-1] < 1200 and len(set(pos.tolist())) == 8
    assert np.all(np.abs(m - 100.0) < 5.0)
    for T in (2, 3, 7, 8, 9, 15, 16, 17, 2 ** 31 - 1):
        p = R.spread_positions(T)
        assert p.min() >= 0 and p.max() <= T - 1 and np.all(np.diff(p) >= 0)
