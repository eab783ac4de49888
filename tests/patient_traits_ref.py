"""
NumPy restatement of the patient-trait rank-sum statistics (fcd_patient_traits.hip), written from the definitions:

  trait q: values y (U,), NaN = not known; n = number of known patients; score of a known patient
      a_u = 2 midrank_u - (n + 1),   midrank_u = #{v known: y_v < y_u} + (#{v known: y_v = y_u} + 1) / 2     (ranks from 1)
  and 0 for the others.  For a chain state and a row rho (the regions, then the region sets with the indicator "patient u has
  an anomalous region in S"):
      k = #{u known: indicator 1},   A = sum_{u known, indicator 1} a_u;   defined where 0 < k < n, and then
      AUC = 1/2 + A / (2 k (n - k)),   bin = min(NB - 1, floor(NB (A + k (n - k)) / (2 k (n - k)))),  NB = 128, in integers.
  trait_hist (Q, R, Umax+1 + NB + 3): [k] the histogram of k, [Umax+1 + bin] of the AUC bins of the defined states, the last
  three words the defined states with A < 0, = 0, > 0.  trait_sum (Q, R, Umax+1): [k] the sum of A over the states with that k.

Used by tests/test_patient_traits.py and tests/test_gpu_patient_traits.py.
"""
import numpy as np

from patient_groups_ref import row_indicators

NB = 128


def scores(y):
    """y (U,) -> (a (U,) int64, known (U,) bool) by counting pairs: 2 midrank = 2 #less + #equal + 1."""
    y = np.asarray(y, dtype=np.float64)
    known = ~np.isnan(y)
    n = int(known.sum())
    a = np.zeros(y.shape, dtype=np.int64)
    for u in np.flatnonzero(known):
        less = int((y[known] < y[u]).sum())
        equal = int((y[known] == y[u]).sum())
        a[u] = 2 * less + equal + 1 - (n + 1)
    return a, known


def k_and_A(x, a, known):
    """x (..., U) of 0 / 1 -> (k, A) int64 of shape x.shape[:-1]."""
    x = np.asarray(x, dtype=np.int64)
    return (x * known.astype(np.int64)).sum(axis=-1), (x * (a * known)).sum(axis=-1)


def auc_bin(A, k, n):
    """The integer bin rule for one defined state."""
    d = k * (n - k)
    assert 0 < k < n and 0 <= A + d <= 2 * d
    return min(NB - 1, (NB * (A + d)) // (2 * d))


def brute_auc(y, x):
    """P(an anomalous known patient has the higher trait) + P(tie) / 2 by counting the pairs, as (2 x wins with a tie half a
    win, number of pairs): AUC = first / (2 x second); None where there is no pair."""
    y = np.asarray(y, dtype=np.float64)
    ones = [y[u] for u in range(len(y)) if x[u] and not np.isnan(y[u])]
    zeros = [y[u] for u in range(len(y)) if not x[u] and not np.isnan(y[u])]
    if not ones or not zeros:
        return None
    wins = sum(2 * (p > q) + (p == q) for p in ones for q in zeros)          # doubled
    return int(wins), len(ones) * len(zeros)


def tally(r, traits, sets=None):
    """
    r (G, Nreg, U), traits: a list of (U,) value vectors -> (trait_hist (Q, R, Umax+1+NB+3) int64, trait_sum (Q, R, Umax+1)
    int64) of this state's G chains.
    """
    x = row_indicators(r, sets)
    (G, rows, _U) = x.shape
    sc = [scores(y) for y in traits]
    ns = [int(kn.sum()) for (_a, kn) in sc]
    umax = max(ns)
    hist = np.zeros((len(traits), rows, umax + 1 + NB + 3), dtype=np.int64)
    total = np.zeros((len(traits), rows, umax + 1), dtype=np.int64)
    for (q, ((a, kn), n)) in enumerate(zip(sc, ns)):
        (k, A) = k_and_A(x, a, kn)                                            # (G, R)
        for rho in range(rows):
            np.add.at(hist[q, rho], k[:, rho], 1)
            np.add.at(total[q, rho], k[:, rho], A[:, rho])
            ok = (k[:, rho] > 0) & (k[:, rho] < n)
            (kk, AA) = (k[ok, rho], A[ok, rho])
            d = kk * (n - kk)
            assert np.all(AA + d >= 0) and np.all(AA <= d)
            np.add.at(hist[q, rho], umax + 1 + np.minimum(NB - 1, (NB * (AA + d)) // (2 * d)), 1)
            np.add.at(hist[q, rho], umax + 1 + NB + np.sign(AA) + 1, 1)
    return hist, total


def state_aucs(r, y, sets=None):
    """Per (chain, row) the AUC of the state as a float, NaN where not defined: for the mean of per-state AUCs."""
    x = row_indicators(r, sets)
    (a, kn) = scores(y)
    n = int(kn.sum())
    (k, A) = k_and_A(x, a, kn)
    out = np.full(k.shape, np.nan)
    ok = (k > 0) & (k < n)
    out[ok] = 0.5 + A[ok] / (2.0 * k[ok] * (n - k[ok]))
    return out


def summaries(hist, total, n_known, level=0.95):
    """The derived quantities of patient_trait_posterior(), cell by cell in plain loops."""
    hist = np.asarray(hist).astype(np.int64)
    total = np.asarray(total).astype(np.int64)
    (Q, R, K) = total.shape
    out = {"p_count": np.zeros((Q, R, K)), "auc_hist": np.full((Q, R, NB), np.nan), "auc_interval": np.full((Q, R, 2), np.nan)}
    for key in ("p_defined", "p_greater", "p_less", "p_equal", "auc_mean"):
        out[key] = np.full((Q, R), np.nan)
    alpha = (1.0 - level) / 2.0
    for q in range(Q):
        n = int(n_known[q])
        for rho in range(R):
            states = int(hist[q, rho, :K].sum())
            (less, equal, greater) = (int(v) for v in hist[q, rho, K + NB:])
            defined = less + equal + greater
            out["p_count"][q, rho] = hist[q, rho, :K] / float(states)
            out["p_defined"][q, rho] = defined / float(states)
            if not defined:
                continue
            assert defined == int(hist[q, rho, 1:n].sum()) == int(hist[q, rho, K:K + NB].sum())
            out["p_less"][q, rho] = less / float(defined)
            out["p_equal"][q, rho] = equal / float(defined)
            out["p_greater"][q, rho] = greater / float(defined)
            out["auc_mean"][q, rho] = 0.5 + sum(int(total[q, rho, k]) / (2.0 * k * (n - k)) for k in range(1, n)) / defined
            p = hist[q, rho, K:K + NB] / float(defined)
            out["auc_hist"][q, rho] = p
            (lo, acc) = (0, p[0])
            while acc < alpha - 1e-12 and lo < NB - 1:
                lo += 1
                acc += p[lo]
            (hi, acc) = (NB - 1, p[NB - 1])
            while acc < alpha - 1e-12 and hi > 0:
                hi -= 1
                acc += p[hi]
            out["auc_interval"][q, rho] = (lo / float(NB), (hi + 1) / float(NB))
    return out
