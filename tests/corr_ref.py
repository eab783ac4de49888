"""
Plain references for K_corr (fcdiff_amd.corr.correlations), independent of numpy.corrcoef and of the kernels.

corr_edges_ld  the sample correlation of every pair of regions in extended precision (np.longdouble: the 80-bit format
               with a 64-bit significand on x86-64, eps 1.1e-19), rounded to fp64 last.  Its own error is a few 2^-64
               times the condition of the input, three decimal orders below what any fp64 formula can reach, so it can
               judge numpy.corrcoef and the kernels alike.
shift_form     the one-workgroup-per-subject kernel's formula restated in fp64 NumPy: rows shifted by a given value
               instead of centred by their mean, Gram matrix and row sums in one pass.  It is not a reference: it is
               there so that the CPU suite records what the choice of shift does to the error.
inputs         the atypical-first-sample series of the GPU tests, shared with the CPU tests that show the bound is fair.
"""
import numpy as np

from oracle import fcdiff_oracle as O

# the project's documented bound for K_corr against its oracle (tests/test_gpu_parity.py, the kernel's own comment)
BOUND = dict(rtol=1e-11, atol=1e-13)

LD = np.longdouble


def corr_edges_ld(ts, fisher_z=False):
    """(S, Nreg, T) -> (C, S) fp64, edge c = n(n-1)/2 + m (n > m): O.edge_endpoints order.  NaN where a deviation is 0 or
    not finite (a constant row, a row with a NaN or an infinite sample), as numpy.corrcoef gives them."""
    ts = np.asarray(ts)
    (S, Nreg, T) = ts.shape
    ends = O.edge_endpoints(Nreg)
    out = np.zeros((ends.shape[0], S), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            X = ts[s].astype(LD)
            X = X - (X.sum(axis=1) / LD(T))[:, None]
            G = X.dot(X.T)
            d = np.sqrt(np.diagonal(G))
            c = G / d[:, None]
            c = c / d[None, :]
            c = np.clip(c, LD(-1), LD(1))
            bad = ~np.isfinite(d) | (d == 0)
            c[bad, :] = np.nan
            c[:, bad] = np.nan
            e = c[ends[:, 0], ends[:, 1]]
            if fisher_z:
                e = np.arctanh(e)
            out[:, s] = e.astype(np.float64)
    return out


def shift_form(ts, shift, fisher_z=False):
    """
    The subject kernel's arithmetic in fp64: X = ts - shift (shift: (S, Nreg), one value per row), G = X X^T, s = row sums,
    cov = (G - s s^T / T) / (T - 1), then two multiplications by 1 / sqrt(diag cov), clip.  (S, Nreg, T) -> (C, S).
    NumPy's summation order is not the MFMA's, so this predicts the size of the kernel's error, not its bits.
    """
    ts = np.asarray(ts, dtype=np.float64)
    (S, Nreg, T) = ts.shape
    ends = O.edge_endpoints(Nreg)
    out = np.zeros((ends.shape[0], S), dtype=np.float64)
    (inv, invT) = (1.0 / (T - 1), 1.0 / T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            X = ts[s] - np.asarray(shift[s], dtype=np.float64)[:, None]
            G = X.dot(X.T)
            sm = X.sum(axis=1)
            cov = (G - sm[:, None] * sm[None, :] * invT) * inv
            sd = 1.0 / np.sqrt(np.diagonal(cov))
            c = cov * sd[:, None]
            c = c * sd[None, :]
            c = np.clip(c, -1.0, 1.0)
            e = c[ends[:, 0], ends[:, 1]]
            out[:, s] = np.arctanh(e) if fisher_z else e
    return out


def first_sample_shift(ts):
    return np.asarray(ts, dtype=np.float64)[:, :, 0]


def spread_positions(T):
    """The eight samples the subject kernel's shift looks at: the middles of the eighths of the row."""
    return np.array([((2 * p + 1) * int(T)) >> 4 for p in range(8)], dtype=np.int64)


def median8_shift(ts):
    """The lower median (rank 3 of 0..7) of eight samples spread over the row: the subject kernel's shift."""
    ts = np.asarray(ts, dtype=np.float64)
    v = np.sort(ts[:, :, spread_positions(ts.shape[2])], axis=2)
    return v[:, :, 3]


def worst_excess(got, exp, rtol, atol):
    """(largest |got - exp|, largest |got - exp| / (atol + rtol |exp|)) over the entries where exp is finite."""
    ok = np.isfinite(exp)
    d = np.abs(got[ok] - exp[ok])
    if d.size == 0:
        return (0.0, 0.0)
    return (float(d.max()), float((d / (atol + rtol * np.abs(exp[ok]))).max()))


# ---------------------------------------------------------------------------------------------------------------------
# the atypical-first-sample inputs: S = 2, Nreg = 16, unit noise plus a shared component, on mean 100
# ---------------------------------------------------------------------------------------------------------------------
ATYPICAL_T = (1200, 20001, 60001)
ATYPICAL_VARIANTS = ("a", "b")


def atypical_input(variant, T, S=2, Nreg=16):
    """
    variant "a": frame 0 moved by +-1000 sd, the sign alternating over regions (a scanner's first volume);
    variant "b": frames 0-3 decaying from +50 sd to the baseline (the approach to steady state).
    The sd is that of the row without the outliers: sqrt(1 + 0.7^2).
    """
    rs = np.random.RandomState(1000 * int(T) % 2 ** 31 + (1 if variant == "a" else 2))
    ts = rs.standard_normal((S, Nreg, T)) + 0.7 * rs.standard_normal((S, 1, T)) + 100.0
    sd = np.sqrt(1.0 + 0.7 ** 2)
    if variant == "a":
        sign = np.where(np.arange(Nreg) % 2 == 0, 1.0, -1.0)
        ts[:, :, 0] += 1000.0 * sd * sign[None, :]
    elif variant == "b":
        ts[:, :, 0:4] += sd * np.array([50.0, 50.0 / 3, 50.0 / 9, 50.0 / 27])[None, None, :]
    else:
        raise ValueError(variant)
    return ts


def exact_collinear_input(S=2, Nreg=6):
    """
    Rows 0, 1, 2 of every subject are x, -x and 2 x with T = 65 and x at its baseline 0 except for eight excursions to +1
    and eight to -1 (odd positions of the first half).  Every sum any of the formulas forms is then a small integer and
    T - 1 = 64 a power of two: mean 0, first sample 0, median 0, Gram diagonal 16, covariance 1/4, deviation 1/2, so
    the correlations of edges 0, 1, 2 are exactly -1, +1, -1 in fp64 and in long double, before any clip.  Only for such
    an input is "atanh gives +-inf" a fair demand: with rounded deviations c = v / sqrt(v) / sqrt(v) may be 1 - 2^-53
    for numpy.corrcoef as well.  The other rows are noise.
    """
    T = 65
    rs = np.random.RandomState(65)
    ts = rs.standard_normal((S, Nreg, T))
    x = np.zeros(T)
    x[1:32:4] = 1.0
    x[3:32:4] = -1.0
    assert (x == 1).sum() == 8 and (x == -1).sum() == 8
    ts[:, 0, :] = x
    ts[:, 1, :] = -x
    ts[:, 2, :] = 2.0 * x
    return ts
