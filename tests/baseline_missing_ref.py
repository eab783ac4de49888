"""
Reference of baseline.group_test and baseline.network_test with their options missing_data=True and variance="welch".

Loop level (group_test, network_test): the direct two-sample formulas on the observed values of the two groups -- group
means, sums of squares about them -- not the centred closed forms the kernel evaluates.  A NaN is an unobserved value.
Exact (class Exact): the same statistics in rational arithmetic (fractions.Fraction), ties included, in the style of
baseline_exact_ref.Exact; on integer-valued rows whose OBSERVED sum is a multiple of n the centred values, Q, A, B and n1 are
integers, exact in doubles in any summation order, so the device's t^2 is a deterministic function of them.

The rules restated (fcdiff_amd.baseline.group_test):
    per connection   O = observed subjects, n = |O|; constant where all observed values are equal (none included)
    pooled           defined iff not constant, n >= 3, n1 >= 1, n0 >= 1; SS_w = 0: t = +/-inf with the sign of the difference
    welch            defined iff not constant, n1 >= 2, n0 >= 2; v = s1^2/n1 + s0^2/n0 = 0: +/-inf (the means differ), else 0
    undefined under a labelling            0 to the sums, no maximum, no bit, but an exceedance in count_t
    undefined under the observed labelling the connection is dead: t NaN, count_t 0, p_t and p_fwe_t NaN, no part anywhere
"""
import math
from fractions import Fraction

import numpy as np

import baseline_exact_ref as XR
import baseline_ref as BR
import network_ref as NR
from fcdiff_amd import util

VARIANCES = ("pooled", "welch")


# ---- loop level --------------------------------------------------------------------------------------------------------------

def two_sample_t(row, lab, variance):
    """t of one row (NaN = unobserved) under the 0/1 labelling lab by the direct formulas; None where it is undefined."""
    g1 = [float(v) for (v, l) in zip(row, lab) if l and not math.isnan(v)]
    g0 = [float(v) for (v, l) in zip(row, lab) if not l and not math.isnan(v)]
    both = g1 + g0
    (n1, n0, n) = (len(g1), len(g0), len(both))
    if n == 0 or min(both) == max(both):
        return None
    if variance == "pooled":
        if n < 3 or n1 < 1 or n0 < 1:
            return None
    elif n1 < 2 or n0 < 2:
        return None
    (m1, m0) = (sum(g1) / n1, sum(g0) / n0)
    ss1 = sum((v - m1) ** 2 for v in g1)
    ss0 = sum((v - m0) ** 2 for v in g0)
    diff = m1 - m0
    if variance == "pooled":
        ss_w = ss1 + ss0
        if not ss_w > 0.0:
            return math.copysign(math.inf, diff)
        return diff / math.sqrt(ss_w / (n - 2) * (1.0 / n1 + 1.0 / n0))
    v = ss1 / (n1 * (n1 - 1)) + ss0 / (n0 * (n0 - 1))
    if not v > 0.0:
        return math.copysign(math.inf, diff) if diff != 0.0 else 0.0
    return diff / math.sqrt(v)


def all_t(b, bt, labels, variance):
    """(t (C,), null_t (P, C)), NaN where undefined; null_t[:, c] is left as computed on a dead connection."""
    X = np.concatenate([b, bt], axis=1)
    (C, H) = b.shape
    observed = [0] * H + [1] * bt.shape[1]

    def row_t(lab):
        return np.array([(lambda v: math.nan if v is None else v)(two_sample_t(X[c], lab, variance)) for c in range(C)])

    return row_t(observed), np.array([row_t(lab) for lab in labels]).reshape(len(labels), C)


def group_test(b, bt, labels, variance="pooled", t_pair=None):
    """Every key of baseline.group_test(b, bt, labels=labels, missing_data=True, variance=variance) but `labels`; also the
    (P, C) null_t (NaN: undefined, or a dead connection) and the (P, N) null_region behind them."""
    (C, H) = b.shape
    U = bt.shape[1]
    N = int(round(util.C_to_N(C)))
    P = labels.shape[0]
    E = BR.edges_of(N)
    (t, tp) = t_pair if t_pair is not None else all_t(b, bt, labels, variance)
    live = ~np.isnan(t)
    tp = np.where(live[None, :], tp, np.nan)

    def sums(row):
        return np.array([sum(row[c] ** 2 for c in E[n] if live[c] and not math.isnan(row[c])) for n in range(N)])

    region = sums(t)
    Rp = np.array([sums(tp[p]) for p in range(P)]).reshape(P, N)
    null_max_t = np.array([max([0.0] + [abs(v) for v in tp[p] if not math.isnan(v)]) for p in range(P)])
    null_max_region = Rp.max(axis=1)
    count_t = np.array([sum(1 for p in range(P) if live[c] and (math.isnan(tp[p, c]) or abs(tp[p, c]) >= abs(t[c])))
                        for c in range(C)], dtype=np.int64)
    count_region = np.array([sum(1 for p in range(P) if Rp[p, n] >= region[n]) for n in range(N)], dtype=np.int64)
    dead = ~live
    return {"t": t, "region": region, "null_max_t": null_max_t, "null_max_region": null_max_region, "count_t": count_t,
            "count_region": count_region, "p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)),
            "p_region": (1.0 + count_region) / (1.0 + P),
            "p_fwe_t": np.array([math.nan if dead[c] else (1.0 + sum(1 for v in null_max_t if v >= abs(t[c]))) / (1.0 + P)
                                 for c in range(C)]),
            "p_fwe_region": np.array([(1.0 + sum(1 for v in null_max_region if v >= region[n])) / (1.0 + P) for n in range(N)]),
            "n_controls": (~np.isnan(b)).sum(axis=1).astype(np.int64), "n_patients": (~np.isnan(bt)).sum(axis=1).astype(np.int64),
            "null_t": tp, "null_region": Rp}


def network_test(b, bt, labels, threshold, tail="both", variance="pooled", t_pair=None):
    """Every key of baseline.network_test(..., missing_data=True, variance=variance) but `labels`, on network_ref's
    union-find; also null_t (P, C).  NaN (undefined, dead) is never suprathreshold."""
    (t, tp) = t_pair if t_pair is not None else all_t(b, bt, labels, variance)
    tp = np.where(np.isnan(t)[None, :], np.nan, tp)
    with np.errstate(invalid="ignore"):
        out = NR.network_test(b, bt, labels, threshold, tail, t_pair=(t, tp))
    out["n_controls"] = (~np.isnan(b)).sum(axis=1).astype(np.int64)
    out["n_patients"] = (~np.isnan(bt)).sum(axis=1).astype(np.int64)
    return out


def make_missing(shape, f):
    """baseline_ref's data of a shape with a fraction f of NaN (its own recipe), as (b, bt, labels)."""
    return BR.make_data(*shape, f=f)


# ---- exact -------------------------------------------------------------------------------------------------------------------

class Exact:
    """
    Row 0 = the observed labelling, rows 1 .. P = labels.  Per connection n[c], const[c], Q[c], integer[c] (the centred
    observed values are integers); per row and connection n1, A, B (Fractions) and t2: None (undefined under that row, or the
    connection is constant), math.inf or a Fraction.  dead[c]: undefined under the observed labelling.  R[p][n], mt2[p], mR[p]
    leave the dead connections and the undefined values out.
    """

    def __init__(self, b, bt, labels, variance="pooled"):
        assert variance in VARIANCES
        (C, H) = b.shape
        U = bt.shape[1]
        (self.C, self.H, self.U, self.S, self.P, self.variance) = (C, H, U, H + U, labels.shape[0], variance)
        self.N = N = int(round(util.C_to_N(C)))
        self.E = BR.edges_of(N)
        X = [[None if math.isnan(v) else Fraction(float(v)) for v in row] for row in np.concatenate([b, bt], axis=1)]
        self.obs = [[v is not None for v in row] for row in X]
        self.n = [sum(o) for o in self.obs]
        self.const = []
        xc = []
        for row in X:
            vals = [v for v in row if v is not None]
            self.const.append(len(vals) == 0 or min(vals) == max(vals))
            mean = sum(vals) / len(vals) if vals else Fraction(0)
            xc.append([Fraction(0) if v is None else v - mean for v in row])
        self.integer = [all(v.denominator == 1 for v in row) for row in xc]
        self.Q = [sum(v * v for v in row) for row in xc]
        self.rows = [XR.observed_row(H, U)] + [np.asarray(r, dtype=np.uint8) for r in labels]
        on = [np.flatnonzero(r).tolist() for r in self.rows]
        R = range(self.P + 1)
        self.n1 = [[sum(1 for s in on[p] if self.obs[c][s]) for c in range(C)] for p in R]
        self.A = [[sum((xc[c][s] for s in on[p]), Fraction(0)) for c in range(C)] for p in R]
        self.B = [[sum((xc[c][s] ** 2 for s in on[p]), Fraction(0)) for c in range(C)] for p in R]
        self.t2 = [[self._t2(p, c) for c in range(C)] for p in R]
        self.dead = [self.t2[0][c] is None for c in range(C)]
        self.live = [c for c in range(C) if not self.dead[c]]
        self.R = [[XR._sum(self.t2[p][c] for c in self.E[n] if not self.dead[c]) for n in range(N)] for p in R]
        self.mt2 = [XR._max([Fraction(0)] + [self.t2[p][c] for c in self.live if self.t2[p][c] is not None]) for p in R]
        self.mR = [XR._max(row) for row in self.R]

    def _t2(self, p, c):
        (n, n1, A, B, Q) = (self.n[c], self.n1[p][c], self.A[p][c], self.B[p][c], self.Q[c])
        n0 = n - n1
        if self.const[c]:
            return None
        if self.variance == "pooled":
            if n < 3 or n1 < 1 or n0 < 1:
                return None
            g = A * A * Fraction(n, n1 * n0)
            ss_w = Q - g
            assert ss_w >= 0
            return math.inf if ss_w == 0 else g * (n - 2) / ss_w
        if n1 < 2 or n0 < 2:
            return None
        (ss1, ss0) = (B - A * A / n1, (Q - B) - A * A / n0)
        assert ss1 >= 0 and ss0 >= 0
        v = ss1 / (n1 * (n1 - 1)) + ss0 / (n0 * (n0 - 1))
        d = A * Fraction(n, n1 * n0)
        if v == 0:
            return math.inf if A != 0 else Fraction(0)
        return d * d / v

    def key(self, p, c):
        """Equal keys on integer rows: the device evaluates t^2 on the same doubles (a labelling and its complement included:
        n1 n0 and the sum of the two variance terms commute), so the results agree bit for bit."""
        (n, n1, A, B, Q) = (self.n[c], self.n1[p][c], self.A[p][c], self.B[p][c], self.Q[c])
        if A == 0:
            return (0,)                    # t^2 = 0 exactly, whatever the rest: 0 k = 0 and 0 / x = 0
        if self.variance == "pooled":
            return (abs(A), Q, n, n1 * (n - n1))
        return (abs(A), Q, n, frozenset([(n1, B), (n - n1, Q - B)]))

    def same_row(self, p):
        return np.array_equal(self.rows[p], self.rows[0])

    def same_on(self, p, c):
        """Row p labels the observed subjects of connection c as the observed labelling does: the labels differ only where the
        centred value and the mask are 0, so the device adds exact zeros to the same sums."""
        return all(self.rows[p][s] == self.rows[0][s] for s in range(self.S) if self.obs[c][s])

    def t(self, p=0):
        out = np.full(self.C, np.nan)
        for c in self.live:
            v = self.t2[p][c]
            if v is not None:
                out[c] = math.copysign(XR._root(v), 1.0 if self.A[p][c] >= 0 else -1.0)
        return out

    def counts(self):
        n_controls = np.array([sum(o[:self.H]) for o in self.obs], dtype=np.int64)
        n_patients = np.array([sum(o[self.H:]) for o in self.obs], dtype=np.int64)
        return n_controls, n_patients

    def group_test(self):
        """Every key of baseline.group_test(..., missing_data=True, variance=...) but `labels`."""
        (C, N, P) = (self.C, self.N, self.P)
        rows = range(1, P + 1)
        count_t = np.zeros(C, dtype=np.int64)
        fwe_t = np.zeros(C, dtype=np.int64)
        for c in self.live:
            count_t[c] = sum(1 for p in rows if self.t2[p][c] is None or XR._ge(self.t2[p][c], self.t2[0][c]))
            fwe_t[c] = sum(1 for p in rows if XR._ge(self.mt2[p], self.t2[0][c]))
        count_region = np.array([sum(1 for p in rows if XR._ge(self.R[p][n], self.R[0][n])) for n in range(N)], dtype=np.int64)
        fwe_region = np.array([sum(1 for p in rows if XR._ge(self.mR[p], self.R[0][n])) for n in range(N)], dtype=np.int64)
        dead = np.array(self.dead)
        (n_controls, n_patients) = self.counts()
        return {"t": self.t(), "region": np.array([XR._f(v) for v in self.R[0]]),
                "null_max_t": np.array([XR._root(self.mt2[p]) for p in rows]),
                "null_max_region": np.array([XR._f(self.mR[p]) for p in rows]),
                "count_t": count_t, "count_region": count_region,
                "p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)), "p_region": (1.0 + count_region) / (1.0 + P),
                "p_fwe_t": np.where(dead, np.nan, (1.0 + fwe_t) / (1.0 + P)), "p_fwe_region": (1.0 + fwe_region) / (1.0 + P),
                "n_controls": n_controls, "n_patients": n_patients}

    def bits(self, threshold, tail):
        """(P + 1, C) bool: t^2 > threshold^2 on the side of the tail; row 0 is the observed labelling."""
        thr2 = Fraction(float(threshold)) ** 2
        out = np.zeros((self.P + 1, self.C), dtype=bool)
        for p in range(self.P + 1):
            for c in self.live:
                (v, A) = (self.t2[p][c], self.A[p][c])
                side = tail == "both" or (A > 0 if tail == "greater" else A < 0)
                out[p, c] = v is not None and side and (v == math.inf or v > thr2)
        return out

    def network_test(self, threshold, tail="both"):
        """Every key of baseline.network_test(..., missing_data=True, variance=...) but `labels`."""
        bits = self.bits(threshold, tail)
        (N, P) = (self.N, self.P)
        obs = NR.components(bits[0], N)
        null = [NR.components(bits[p], N) for p in range(1, P + 1)]
        null_max_extent = np.array([r["max_extent"] for r in null], dtype=np.int64)
        p_fwe = np.array([(1.0 + sum(1 for v in null_max_extent if v >= e)) / (1.0 + P) for e in obs["component_edges"]])
        p_of = dict(zip(obs["component_label"].tolist(), p_fwe.tolist()))
        (n_controls, n_patients) = self.counts()
        return {"t": self.t(), "edge_mask": bits[0], "component": obs["component"], "component_label": obs["component_label"],
                "component_edges": obs["component_edges"], "component_regions": obs["component_regions"],
                "null_max_extent": null_max_extent,
                "null_max_regions": np.array([r["max_regions"] for r in null], dtype=np.int64),
                "null_n_edges": np.array([r["n_edges"] for r in null], dtype=np.int64), "p_fwe": p_fwe,
                "p_fwe_region": np.array([p_of.get(int(lab), math.nan) for lab in obs["component"]]),
                "threshold": float(threshold), "tail": tail, "n_controls": n_controls, "n_patients": n_patients}

    # -- ties and conditions (baseline_exact_ref.Exact.check_conditions, with the undefined values left out) --

    def ties(self):
        rows = range(1, self.P + 1)
        tt = sum(1 for p in rows for c in self.live if self.t2[p][c] is not None and self.t2[p][c] == self.t2[0][c])
        tr = sum(1 for p in rows for n in range(self.N) if self.R[p][n] == self.R[0][n])
        return tt, tr

    def _terms(self, p, n):
        return [None if self.dead[c] or self.t2[p][c] is None else self.key(p, c) for c in self.E[n]]

    def _region_tie_is_safe(self, p, n_null, n_obs):
        same = n_null == n_obs and all(self.same_on(p, c) for c in self.E[n_obs] if not self.dead[c])
        exact = same or all(self.integer[c] for c in self.E[n_null] + self.E[n_obs])
        return exact and self._terms(p, n_null) == self._terms(0, n_obs)

    def _t_tie_is_safe(self, p, c_null, c_obs):
        exact = (c_null == c_obs and self.same_on(p, c_obs)) or (self.integer[c_null] and self.integer[c_obs])
        return exact and self.key(p, c_null) == self.key(0, c_obs)

    def check_conditions(self, thresholds=(), boundary=()):
        """AssertionError unless exact comparison with a device working in doubles is legitimate: every exact tie is one the
        device reproduces bit for bit, every other pair of compared values differs by more than relative GAP, and every t^2
        is farther than GAP from threshold^2 or, for a threshold in `boundary`, exactly equal to it."""
        GAP = XR.GAP
        rows = range(1, self.P + 1)
        for p in rows:
            defined = [c for c in self.live if self.t2[p][c] is not None]
            for c in self.live:
                (a, o) = (self.t2[p][c], self.t2[0][c])
                if a is not None:
                    assert (self._t_tie_is_safe(p, c, c) if a == o else XR._rel_gap(a, o) > GAP), ("t", p, c)
                (a, o) = (self.mt2[p], self.t2[0][c])
                if a == o:
                    assert any(self.t2[p][k] == a and self._t_tie_is_safe(p, k, c) for k in defined), ("max t", p, c)
                else:
                    assert XR._rel_gap(a, o) > GAP, ("max t", p, c)
            for n in range(self.N):
                (a, o) = (self.R[p][n], self.R[0][n])
                assert (self._region_tie_is_safe(p, n, n) if a == o else XR._rel_gap(a, o) > GAP), ("region", p, n)
                (a, o) = (self.mR[p], self.R[0][n])
                if a == o:
                    assert any(self.R[p][k] == a and self._region_tie_is_safe(p, k, n) for k in range(self.N)), ("max region", p, n)
                else:
                    assert XR._rel_gap(a, o) > GAP, ("max region", p, n)
        for thr in thresholds:
            thr2 = Fraction(float(thr)) ** 2
            for p in range(self.P + 1):
                for c in self.live:
                    v = self.t2[p][c]
                    if v is None:
                        continue
                    if v == thr2:
                        assert thr in boundary and self.integer[c], ("threshold", thr, p, c)
                    else:
                        assert v == math.inf or float(abs(v - thr2) / thr2) > GAP, ("threshold", thr, p, c)


def integer_rows_missing(C, S, rng, f, span=8):
    """(C, S) float rows of integers in -span .. span with a fraction f of NaN (at least 4 observed per row); the first observed
    entry of every row corrected so that the OBSERVED sum is a multiple of n."""
    X = rng.integers(-span, span + 1, size=(C, S)).astype(np.float64)
    for c in range(C):
        gone = np.flatnonzero(rng.random(S) < f)[:S - 4]
        X[c, gone] = np.nan
        fix_observed_sum(X[c])
    return X


def fix_observed_sum(row):
    o = np.flatnonzero(~np.isnan(row))
    n = len(o)
    r = int(row[o].sum()) % n
    row[o[0]] -= r - n if r > n // 2 else r
    assert int(row[o].sum()) % n == 0
