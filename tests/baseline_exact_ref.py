"""
Exact reference of baseline.group_test and baseline.network_test: rational arithmetic (fractions.Fraction) on the data as
given, ties and degenerate connections included.  Also the named cases of tests/test_gpu_baseline_exact.py and the conditions
under which a device working in doubles must reproduce the reference's counts, bits and p-values exactly.

Why exact tests are possible.  On integer-valued data whose row sums are multiples of S = H + U the row mean is an integer,
so the centred values, Q and every sum A over labelled subjects are integers: exact in doubles, in any summation order, the
MFMA's included.  t^2 = g (S - 2) / (Q - g), g = A^2 S/(U H), evaluated in doubles is then a deterministic function of exact
integers: equal |A| on the same connection give a bit-identical t^2, and a larger |A| gives a strictly larger one (every
step is monotone in A^2, and distinct integers below 1e4 differ by far more than 2^-50 relative).  The reference for the
counts is therefore integer arithmetic, ties included: count_t[c] = #{p : |A_pc| >= |A_c|}.

The documented rules for degenerate connections (fcdiff_amd.baseline.group_test) are restated here, not derived:
    constant (min == max over the S values)  t NaN, 0 to every region sum, no maximum, never suprathreshold, count_t 0,
                                             p_t and p_fwe_t NaN
    SS_w = Q - g = 0 with Q > 0              t^2 = +inf, t = +/-inf with the sign of A; inf >= inf counts
Representation: a t^2 is None (constant), math.inf or a Fraction; a region sum is math.inf or a Fraction.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import baseline_ref as BR
import network_ref as NR
from fcdiff_amd import util

GAP = 1e-9                 # what separates two values that are not an exact tie (tests/test_gpu_baseline.py's GAP)
EPS = 2.0 ** -52
REAL_RTOL = 1e-10          # real-valued rows: the project's bound for its fp64 kernels
THRESHOLDS = (1.5, 2.5)
TAILS = ("both", "greater", "less")


# ---- rational helpers --------------------------------------------------------------------------------------------------------

def _ge(a, b):
    """a >= b for Fractions and math.inf."""
    return a == b or (b != math.inf and (a == math.inf or a > b))


def _rel_gap(a, b):
    """|a - b| / max(|a|, |b|) of two distinct non-negative values, inf if either is infinite."""
    if a == math.inf or b == math.inf:
        return math.inf
    return float(abs(a - b) / max(a, b))


def _root(x):
    """sqrt of a non-negative Fraction, to 2^-64 relative before the one rounding to double."""
    if x == math.inf:
        return math.inf
    (n, d) = (x.numerator, x.denominator)
    return float(Fraction(math.isqrt((n * d) << 128), d << 64))


def _f(x):
    return math.inf if x == math.inf else float(x)


def _sum(terms):
    """Sum of t^2 values: None adds 0, inf makes inf."""
    terms = [v for v in terms if v is not None]
    return math.inf if any(v == math.inf for v in terms) else sum(terms, Fraction(0))


def _max(values):
    return math.inf if any(v == math.inf for v in values) else max(values)


# ---- the exact statistics ----------------------------------------------------------------------------------------------------

class Exact:
    """
    Everything behind the outputs, row 0 = the observed labelling, rows 1 .. P = labels: A[p][c] (Fractions; integers on
    integer rows), Q[c], const[c], integer[c] (the row is integer-valued with an integer mean), t2[p][c], R[p][n], and the
    maxima mt2[p] (0 where every connection is constant), mR[p].  E = baseline_ref.edges_of(N): the device's order of E(n).
    """

    def __init__(self, b, bt, labels):
        (C, H) = b.shape
        U = bt.shape[1]
        (self.C, self.H, self.U, self.S, self.P) = (C, H, U, H + U, labels.shape[0])
        S = self.S
        self.N = N = int(round(util.C_to_N(C)))
        self.E = BR.edges_of(N)
        self.kf = Fraction(S, U * H)
        self.dof = S - 2
        X = [[Fraction(float(v)) for v in row] for row in np.concatenate([b, bt], axis=1)]
        self.const = [min(row) == max(row) for row in X]
        xc = []
        for row in X:
            mean = sum(row) / S
            xc.append([v - mean for v in row])
        self.integer = [all(v.denominator == 1 for v in row) for row in xc]
        self.Q = [sum(v * v for v in row) for row in xc]
        assert all((q == 0) == k for (q, k) in zip(self.Q, self.const))
        self.rows = [np.array([0] * H + [1] * U, dtype=np.uint8)] + [np.asarray(r, dtype=np.uint8) for r in labels]
        on = [np.flatnonzero(r).tolist() for r in self.rows]
        self.A = [[sum((xc[c][s] for s in idx), Fraction(0)) for c in range(C)] for idx in on]
        self.t2 = [[self._t2(self.A[p][c], c) for c in range(C)] for p in range(self.P + 1)]
        self.R = [[_sum(self.t2[p][c] for c in self.E[n]) for n in range(N)] for p in range(self.P + 1)]
        self.mt2 = [_max([Fraction(0)] + [v for v in row if v is not None]) for row in self.t2]
        self.mR = [_max(row) for row in self.R]

    def _t2(self, A, c):
        if self.const[c]:
            return None
        g = A * A * self.kf
        ss_w = self.Q[c] - g
        assert ss_w >= 0
        return math.inf if ss_w == 0 else g * self.dof / ss_w

    def key(self, p, c):
        """Equal keys on integer rows: the device evaluates t^2 on the same doubles, so the results agree bit for bit."""
        return (abs(self.A[p][c]), self.Q[c])

    def same_row(self, p):
        return np.array_equal(self.rows[p], self.rows[0])

    # -- outputs --

    def t(self, p=0):
        out = np.full(self.C, np.nan)
        for c in range(self.C):
            v = self.t2[p][c]
            if v is not None:
                out[c] = math.copysign(_root(v), 1.0 if self.A[p][c] >= 0 else -1.0)
        return out

    def group_test(self):
        """Every key of baseline.group_test(b, bt, labels=labels) but `labels`."""
        (C, N, P) = (self.C, self.N, self.P)
        rows = range(1, P + 1)
        live = [c for c in range(C) if not self.const[c]]
        count_t = np.zeros(C, dtype=np.int64)
        fwe_t = np.zeros(C, dtype=np.int64)
        for c in live:
            count_t[c] = sum(1 for p in rows if _ge(self.t2[p][c], self.t2[0][c]))
            fwe_t[c] = sum(1 for p in rows if _ge(self.mt2[p], self.t2[0][c]))
        count_region = np.array([sum(1 for p in rows if _ge(self.R[p][n], self.R[0][n])) for n in range(N)], dtype=np.int64)
        fwe_region = np.array([sum(1 for p in rows if _ge(self.mR[p], self.R[0][n])) for n in range(N)], dtype=np.int64)
        dead = np.array(self.const)
        return {"t": self.t(), "region": np.array([_f(v) for v in self.R[0]]),
                "null_max_t": np.array([_root(self.mt2[p]) for p in rows]),
                "null_max_region": np.array([_f(self.mR[p]) for p in rows]),
                "count_t": count_t, "count_region": count_region,
                "p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)), "p_region": (1.0 + count_region) / (1.0 + P),
                "p_fwe_t": np.where(dead, np.nan, (1.0 + fwe_t) / (1.0 + P)), "p_fwe_region": (1.0 + fwe_region) / (1.0 + P)}

    def integer_count_t(self):
        """count_t in integers alone, #{p : |A_pc| >= |A_c|}, on the integer rows; -1 elsewhere."""
        return np.array([sum(1 for p in range(1, self.P + 1) if abs(self.A[p][c]) >= abs(self.A[0][c]))
                         if self.integer[c] and not self.const[c] else -1 for c in range(self.C)], dtype=np.int64)

    def bits(self, threshold, tail):
        """(P + 1, C) bool: t^2 > threshold^2 on the side of the tail; row 0 is the observed labelling."""
        thr2 = Fraction(float(threshold)) ** 2
        out = np.zeros((self.P + 1, self.C), dtype=bool)
        for p in range(self.P + 1):
            for c in range(self.C):
                (v, A) = (self.t2[p][c], self.A[p][c])
                side = tail == "both" or (A > 0 if tail == "greater" else A < 0)
                out[p, c] = v is not None and side and (v == math.inf or v > thr2)
        return out

    def network_test(self, threshold, tail="both"):
        """Every key of baseline.network_test(b, bt, threshold, labels=labels, tail=tail) but `labels`."""
        bits = self.bits(threshold, tail)
        (N, P) = (self.N, self.P)
        obs = NR.components(bits[0], N)
        null = [NR.components(bits[p], N) for p in range(1, P + 1)]
        null_max_extent = np.array([r["max_extent"] for r in null], dtype=np.int64)
        p_fwe = np.array([(1.0 + sum(1 for v in null_max_extent if v >= e)) / (1.0 + P) for e in obs["component_edges"]])
        p_of = dict(zip(obs["component_label"].tolist(), p_fwe.tolist()))
        return {"t": self.t(), "edge_mask": bits[0], "component": obs["component"], "component_label": obs["component_label"],
                "component_edges": obs["component_edges"], "component_regions": obs["component_regions"],
                "null_max_extent": null_max_extent,
                "null_max_regions": np.array([r["max_regions"] for r in null], dtype=np.int64),
                "null_n_edges": np.array([r["n_edges"] for r in null], dtype=np.int64), "p_fwe": p_fwe,
                "p_fwe_region": np.array([p_of.get(int(lab), math.nan) for lab in obs["component"]]),
                "threshold": float(threshold), "tail": tail}

    # -- tolerances (relative; derived in the module docstring of tests/test_gpu_baseline_exact.py) --

    def _bound_t2(self, p, c):
        v = self.t2[p][c]
        if v is None or v == math.inf:
            return 0.0
        return 8.0 * (1.0 + float(v) / self.dof) * EPS if self.integer[c] else REAL_RTOL

    def _bound_R(self, p, n):
        return max(self._bound_t2(p, c) for c in self.E[n]) + (self.N - 1) * EPS

    def bounds(self):
        """Relative bounds of t, region, null_max_t, null_max_region."""
        rows = range(1, self.P + 1)
        return {"t": np.array([0.5 * self._bound_t2(0, c) for c in range(self.C)]),
                "region": np.array([self._bound_R(0, n) for n in range(self.N)]),
                "null_max_t": np.array([0.5 * max(self._bound_t2(p, c) for c in range(self.C)) for p in rows]),
                "null_max_region": np.array([max(self._bound_R(p, n) for n in range(self.N)) for p in rows])}

    # -- ties and conditions --

    def ties(self):
        """(ties in count_t, ties in count_region): pairs (p, c) and (p, n) whose statistic equals the observed one exactly."""
        rows = range(1, self.P + 1)
        tt = sum(1 for p in rows for c in range(self.C) if self.t2[p][c] is not None and self.t2[p][c] == self.t2[0][c])
        tr = sum(1 for p in rows for n in range(self.N) if self.R[p][n] == self.R[0][n])
        return tt, tr

    def _terms(self, p, n):
        return [self.key(p, c) for c in self.E[n] if not self.const[c]]

    def _region_tie_is_safe(self, p, n_null, n_obs):
        """Equal (|A|, Q) element by element over E(n), all on integer rows or under the observed labelling itself: the
        device adds the same numbers in the same order (constant connections add 0 at the same positions)."""
        if [self.const[c] for c in self.E[n_null]] != [self.const[c] for c in self.E[n_obs]]:
            return False
        exact = self.same_row(p) or all(self.integer[c] for c in self.E[n_null] + self.E[n_obs])
        return exact and self._terms(p, n_null) == self._terms(0, n_obs)

    def _t_tie_is_safe(self, p, c_null, c_obs):
        exact = (self.same_row(p) and c_null == c_obs) or (self.integer[c_null] and self.integer[c_obs])
        return exact and self.key(p, c_null) == self.key(0, c_obs)

    def check_conditions(self, thresholds=(), boundary=()):
        """
        Raises AssertionError unless exact comparison with a device working in doubles is legitimate:
        1.  every exact tie R_pn == R_n comes from a labelling whose (|A|, Q) over E(n) equal the observed ones element by
            element; every other pair differs by more than relative GAP.  The same for t^2 against the observed t^2 of its
            connection, and for the maxima against every observed value they are compared with (p_fwe_t, p_fwe_region): a tie
            of a maximum must be attained at a term that is safe in this sense.
        2.  every t^2 is farther than relative GAP from threshold^2, or, for a threshold listed in `boundary`, exactly equal.
        """
        rows = range(1, self.P + 1)
        live = [c for c in range(self.C) if not self.const[c]]
        for p in rows:
            for c in live:
                (a, o) = (self.t2[p][c], self.t2[0][c])
                assert (self._t_tie_is_safe(p, c, c) if a == o else _rel_gap(a, o) > GAP), ("t", p, c)
                (a, o) = (self.mt2[p], self.t2[0][c])
                if a == o:
                    assert any(self.t2[p][k] == a and self._t_tie_is_safe(p, k, c) for k in live), ("max t", p, c)
                else:
                    assert _rel_gap(a, o) > GAP, ("max t", p, c)
            for n in range(self.N):
                (a, o) = (self.R[p][n], self.R[0][n])
                assert (self._region_tie_is_safe(p, n, n) if a == o else _rel_gap(a, o) > GAP), ("region", p, n)
                (a, o) = (self.mR[p], self.R[0][n])
                if a == o:
                    assert any(self.R[p][k] == a and self._region_tie_is_safe(p, k, n) for k in range(self.N)), ("max region", p, n)
                else:
                    assert _rel_gap(a, o) > GAP, ("max region", p, n)
        for thr in thresholds:
            thr2 = Fraction(float(thr)) ** 2
            for p in range(self.P + 1):
                for c in live:
                    v = self.t2[p][c]
                    if v == thr2:
                        assert thr in boundary, ("threshold", thr, p, c)
                    else:
                        assert v == math.inf or float(abs(v - thr2) / thr2) > GAP, ("threshold", thr, p, c)


# ---- data and cases ----------------------------------------------------------------------------------------------------------

def integer_rows(C, S, rng):
    """(C, S) integers drawn in -8 .. 8, entry 0 of every row corrected so that the row sum is a multiple of S."""
    X = rng.integers(-8, 9, size=(C, S)).astype(np.int64)
    fix_row_sums(X)
    return X


def fix_row_sums(X, at=0):
    S = X.shape[1]
    r = X.sum(axis=1) % S
    X[:, at] -= np.where(r > S // 2, r - S, r)
    assert (X.sum(axis=1) % S == 0).all()


def random_labels(P, H, U, rng, avoid=()):
    """P drawn rows with exactly U ones, none of them equal to a row of `avoid` (drawn again if so)."""
    labels = np.zeros((P, H + U), dtype=np.uint8)
    for p in range(P):
        while True:
            row = np.zeros(H + U, dtype=np.uint8)
            row[rng.permutation(H + U)[:U]] = 1
            if not any(np.array_equal(row, a) for a in avoid):
                break
        labels[p] = row
    return labels


def observed_row(H, U):
    return np.array([0] * H + [1] * U, dtype=np.uint8)


class Case:
    """b (C, H), bt (C, U), labels (P, S), and what the case's test needs to know about its construction."""

    def __init__(self, X, H, labels, **meta):
        X = np.asarray(X, dtype=np.float64)
        (self.b, self.bt) = (np.ascontiguousarray(X[:, :H]), np.ascontiguousarray(X[:, H:]))
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8)
        (self.H, self.U) = (H, X.shape[1] - H)
        assert (self.labels.sum(axis=1) == self.U).all()
        self.thresholds = THRESHOLDS
        self.boundary = ()
        self.min_ties = None
        self.rounding_c = ()       # connections whose observed t is a matter of rounding (huge or infinite)
        self.rounding_sign = {}    # ... and the sign it must have
        self.__dict__.update(meta)


def _e1(seed=11):
    """E1 (7, 5, 4, 50): S = 9 is not a multiple of 4.  Rows 0, 17 and 49 are the observed labelling, the other 47 are
    drawn.  Integer data in -8 .. 8 tie by themselves in count_t: 131 ties in count_t (63 of them from the three observed
    rows), 21 in count_region (the three observed rows at 7 regions)."""
    (N, H, U, P) = (7, 5, 4, 50)
    rng = np.random.default_rng(seed)
    X = integer_rows(util.N_to_C(N), H + U, rng)
    obs = observed_row(H, U)
    labels = random_labels(P, H, U, rng, avoid=[obs])
    labels[[0, 17, 49]] = obs
    return Case(X, H, labels, min_ties=(20, 3), obs_rows=[0, 17, 49])


def _e2(seed=12):
    """E2 (19, 6, 6, 40) + 4: 18 connections per region cross a 16-tile; H == U, so the complement of the observed labelling
    is a labelling: rows 0, 17 and 43 hold it, row 5 the observed one, the 40 drawn rows fill the rest in order.  Ties:
    1137 in count_t (4 x 171 from the four extra rows, the data's own on top), 76 = 4 x 19 in count_region."""
    (N, H, U, P) = (19, 6, 6, 40)
    rng = np.random.default_rng(seed)
    X = integer_rows(util.N_to_C(N), H + U, rng)
    obs = observed_row(H, U)
    base = random_labels(P, H, U, rng, avoid=[obs, 1 - obs])
    special = {0: 1 - obs, 5: obs, 17: 1 - obs, P + 3: 1 - obs}
    rest = iter(base)
    labels = np.stack([special[i] if i in special else next(rest) for i in range(P + 4)])
    return Case(X, H, labels, min_ties=(20, 3), base_labels=base, comp_rows=[0, 17, P + 3], obs_rows=[5])


def _e3(seed=13):
    """E3 (4, 100, 45, 20): S = 145 takes a second label word.  Subjects 127 and 128 (across the label-word boundary) have
    identical columns, and so have subjects 99 and 100 (across the group boundary).  The 20 rows are 10 pairs (pair_rows)
    that differ only by swapping the two labels inside a duplicate pair: four drawn pairs over (127, 128), four over
    (99, 100), and two pairs made of the observed labelling and its swap over (99, 100): those four rows tie the observed
    statistics everywhere, 24 ties in count_t and 16 in count_region."""
    (N, H, U, P) = (4, 100, 45, 20)
    S = H + U
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(util.N_to_C(N), S)).astype(np.int64)
    X[:, 128] = X[:, 127]
    X[:, H] = X[:, H - 1]
    fix_row_sums(X)
    obs = observed_row(H, U)

    def swapped(row, i, j):
        out = row.copy()
        (out[i], out[j]) = (row[j], row[i])
        return out

    def drawn_pair(i, j):
        while True:
            row = random_labels(1, H, U, rng)[0]
            if row[i] != row[j]:
                return [row, swapped(row, i, j)]

    pairs = [drawn_pair(127, 128) for _ in range(3)] + [drawn_pair(H - 1, H) for _ in range(3)]
    pairs += [[obs, swapped(obs, H - 1, H)], [swapped(obs, H - 1, H), obs]]
    # the two rows of pairs 0 .. 3 at rows i and 16 + i (the second row lies in the second group of 16), the others side by side
    labels = [None] * P
    pair_rows = []
    for (i, (a, b)) in enumerate(pairs):
        (ra, rb) = (i, 16 + i) if i < 4 else (4 + 2 * (i - 4), 5 + 2 * (i - 4))
        (labels[ra], labels[rb]) = (a, b)
        pair_rows.append((ra, rb))
    filler = iter(drawn_pair(127, 128) + drawn_pair(H - 1, H))
    extra = []
    for r in range(P):
        if labels[r] is None:
            labels[r] = next(filler)
            extra.append(r)
    pair_rows += [(extra[0], extra[1]), (extra[2], extra[3])]
    return Case(X, H, np.stack(labels), min_ties=(20, 3), pair_rows=pair_rows)


def _e4(seed=14):
    """E4, the threshold boundary, (4, 4, 4, 12).  Connection 0 holds controls -3, -1, 0, 0 and patients 3, 1, 0, 0:
    kf = 1/2, A = 4, Q = 20, t^2 = 8 * 6 / (20 - 8) = 4.0, every step exact in doubles.  Connection 1 is its mirror
    (A = -4).  Row 3 labels subjects 2 .. 5 (0 + 0 + 3 + 1 = 4): a tie in count_t[0] and count_t[1] by another labelling."""
    (N, H, U, P) = (4, 4, 4, 12)
    rng = np.random.default_rng(seed)
    X = integer_rows(util.N_to_C(N), H + U, rng)
    X[0] = [-3, -1, 0, 0, 3, 1, 0, 0]
    X[1] = -X[0]
    labels = random_labels(P, H, U, rng)
    labels[3] = [0, 0, 1, 1, 1, 1, 0, 0]
    return Case(X, H, labels, thresholds=THRESHOLDS + (2.0,), boundary=(2.0,), tie_row=3)


def _d1():
    """D1, constant connections: E1's data and labels with connection 3 all 0.3 (not dyadic), connection 8 all 0.0, the six
    connections of region 6 (15 .. 20) each constant at another value, and connection 10 constant over the controls only
    (it stays defined)."""
    e1 = _e1()
    X = np.concatenate([e1.b, e1.bt], axis=1)
    X[3] = 0.3
    X[8] = 0.0
    for (c, v) in zip(range(15, 21), (2.0, 0.3, -1.5, 7.0, 0.1, -0.7)):
        X[c] = v
    X[10] = [1, 1, 1, 1, 1, 3, -2, 4, 8]
    return Case(X, e1.H, e1.labels, constant_c=[3, 8] + list(range(15, 21)), dead_region=6, half_constant_c=10,
                obs_rows=e1.obs_rows)


def _d2(seed=15):
    """D2, separation, (7, 6, 3, 50).  Connection 0 holds controls 2 and patients 5: mean 3, Q = 18, A = 6, g = 18 = Q, so
    SS_w = 0 in exact integers and t = +inf.  Connections 5, 9, 12, 14 and 20 hold two values that are not dyadic (controls
    0.3 and patients 0.45, ...; on 14 the patients are the lower): SS_w = 0 in exact arithmetic, in doubles a difference of two
    rounded numbers that comes out negative, zero or positive (about a third each over such pairs).  Row 20 is the observed
    labelling, so inf >= inf is counted."""
    (N, H, U, P) = (7, 6, 3, 50)
    rng = np.random.default_rng(seed)
    X = integer_rows(util.N_to_C(N), H + U, rng).astype(np.float64)
    X[0] = [2.0] * H + [5.0] * U
    two_valued = {5: (0.3, 0.45), 9: (0.1, 0.7), 12: (-0.62, 0.17), 14: (0.81, 0.33), 20: (0.07, 0.93)}
    for (c, (lo, hi)) in two_valued.items():
        X[c] = [lo] * H + [hi] * U
    obs = observed_row(H, U)
    labels = random_labels(P, H, U, rng, avoid=[obs])
    labels[20] = obs
    return Case(X, H, labels, obs_rows=[20], separated_c=0, rounding_c=tuple(two_valued),
                rounding_sign=dict((c, 1.0 if hi > lo else -1.0) for (c, (lo, hi)) in two_valued.items()))


CASES = {"E1": _e1, "E2": _e2, "E3": _e3, "E4": _e4, "D1": _d1, "D2": _d2}
TIED = ("E1", "E2", "E3")


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, Exact) of a named case, made once."""
    k = CASES[name]()
    return k, Exact(k.b, k.bt, k.labels)


@functools.lru_cache(maxsize=None)
def group(name):
    return case(name)[1].group_test()


@functools.lru_cache(maxsize=None)
def network(name, threshold, tail):
    return case(name)[1].network_test(threshold, tail)


def plain_case(shape):
    """baseline_ref's data of a shape (no ties: normal(0.3, 0.1)) as (b, bt, labels, Exact)."""
    (b, bt, labels) = BR.make_data(*shape)
    return b, bt, labels, Exact(b, bt, labels)
