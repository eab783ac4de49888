"""
NumPy reference of fcdiff_amd.baseline: a plain, loop-level restatement of the definitions, with the leave-one-out scores
made by actually deleting the control.  Also the seeded data recipe and the shapes the tests share.
"""
import math

import numpy as np

from fcdiff_amd import util

# (N, H, U, P, seed)
SHAPES = [
    (7, 5, 4, 50, 0),        # S = 9 is not a multiple of 4; 6 connections per region
    (19, 6, 5, 37, 1),       # 18 connections cross one 16-tile; P is not a multiple of 16
    (5, 70, 3, 33, 2),       # more subjects than lanes
    (4, 3, 1, 1, 3),         # smallest legal case: one patient, one permutation
    (18, 9, 8, 64, 4),       # P exactly four 16-tiles
]
MISSING = {1: 0.1, 2: 0.05, 4: 0.2}      # index into SHAPES -> fraction of NaN of the missing-data runs


def make_data(N, H, U, P, seed, f=None):
    """(b, bt, labels) by the recipe: normal(0.3, 0.1), the first N - 1 connections of the patients shifted by 0.15."""
    rng = np.random.default_rng(seed)
    C = util.N_to_C(N)
    b = rng.normal(0.3, 0.1, (C, H))
    bt = rng.normal(0.3, 0.1, (C, U))
    bt[:N - 1] += 0.15
    if f is not None:
        b[rng.random(b.shape) < f] = np.nan
        bt[rng.random(bt.shape) < f] = np.nan
    S = H + U
    labels = np.zeros((P, S), dtype=np.uint8)
    for p in range(P):
        labels[p, rng.permutation(S)[:U]] = 1
    return b, bt, labels


def edges_of(N):
    """E(n) for every region: the connections that touch it."""
    E = [[] for _ in range(N)]
    for c in range(util.N_to_C(N)):
        (n, m) = util.c_to_nm(c)
        E[n].append(c)
        E[m].append(c)
    return E


def _mean_sd(values):
    """Mean and unbiased standard deviation of a list, two passes."""
    k = len(values)
    m = sum(values) / k
    ss = 0.0
    for v in values:
        ss += (v - m) ** 2
    return m, math.sqrt(ss / (k - 1))


def _p_value(null, value):
    """(1 + #{valid null >= value}) / (1 + #valid null); NaN for a NaN value."""
    if math.isnan(value):
        return math.nan
    valid = [v for v in null if not math.isnan(v)]
    return (1.0 + sum(1 for v in valid if v >= value)) / (1.0 + len(valid))


def _region_summary(zs, E, thr):
    (N, K) = (len(E), zs.shape[1])
    msq = np.full((N, K), np.nan)
    n_edges = np.zeros((N, K), dtype=np.int64)
    n_over = np.zeros((N, K), dtype=np.int64)
    for n in range(N):
        for s in range(K):
            vals = [zs[c, s] for c in E[n] if not math.isnan(zs[c, s])]
            n_edges[n, s] = len(vals)
            n_over[n, s] = sum(1 for v in vals if abs(v) > thr)
            if vals:
                msq[n, s] = sum(v * v for v in vals) / len(vals)
    return msq, n_edges, n_over


def normative(b, bt, z_threshold=3.0):
    """Every key of baseline.normative(..., missing_data=True, return_z=True)."""
    (C, H) = b.shape
    U = bt.shape[1]
    N = int(round(util.C_to_N(C)))
    z = np.full((C, U), np.nan)
    z0 = np.full((C, H), np.nan)
    n_controls = np.zeros(C, dtype=np.int64)
    for c in range(C):
        obs = [float(v) for v in b[c] if not math.isnan(v)]
        n_c = len(obs)
        n_controls[c] = n_c
        if n_c < 3:
            continue
        (m, s) = _mean_sd(obs)
        if s > 0:
            for u in range(U):
                if not math.isnan(bt[c, u]):
                    z[c, u] = (bt[c, u] - m) / (s * math.sqrt(1.0 + 1.0 / n_c))
        for h in range(H):
            if math.isnan(b[c, h]):
                continue
            others = [float(v) for (i, v) in enumerate(b[c]) if i != h and not math.isnan(v)]      # control h deleted
            (m1, s1) = _mean_sd(others)
            if s1 > 0:
                z0[c, h] = (b[c, h] - m1) / (s1 * math.sqrt(1.0 + 1.0 / (n_c - 1)))
    E = edges_of(N)
    (msq, n_edges, n_over) = _region_summary(z, E, z_threshold)
    (msq0, n_edges0, n_over0) = _region_summary(z0, E, z_threshold)
    max0 = np.full(H, np.nan)
    for h in range(H):
        vals = [msq0[n, h] for n in range(N) if not math.isnan(msq0[n, h])]
        if vals:
            max0[h] = max(vals)
    p_region = np.array([[_p_value(msq0[n], msq[n, u]) for u in range(U)] for n in range(N)])
    p_fwe = np.array([[_p_value(max0, msq[n, u]) for u in range(U)] for n in range(N)])
    return {"z": z, "z0": z0, "msq": msq, "n_edges": n_edges, "n_over": n_over, "msq0": msq0, "n_edges0": n_edges0,
            "n_over0": n_over0, "max0": max0, "p_region": p_region, "p_fwe": p_fwe, "n_controls": n_controls}


def centre(X):
    """Rows centred on their mean, and their sums of squares.  A constant row (min == max) is exactly 0 with q = 0."""
    (C, S) = X.shape
    xc = np.zeros((C, S))
    q = np.zeros(C)
    for c in range(C):
        if min(X[c]) == max(X[c]):
            continue
        m = sum(float(v) for v in X[c]) / S
        for s in range(S):
            xc[c, s] = X[c, s] - m
            q[c] += xc[c, s] ** 2
    return xc, q


def _t_of(x, q, lab, S, U, H):
    """
    Student's pooled-variance t of one centred row x (sum of squares q) under the labelling lab.  NaN for a constant row
    (q = 0); +/-inf with the sign of A where SS_w, a difference of two rounded numbers, is not > 0.
    """
    if q == 0.0:
        return math.nan
    A = 0.0
    for s in range(S):
        if lab[s]:
            A += x[s]
    k = S / (U * H)
    ss_w = q - A * A * k
    if not ss_w > 0.0:
        return math.copysign(math.inf, A)
    return A * k / math.sqrt(ss_w / (S - 2) * k)


def group_test(b, bt, labels):
    """Every key of baseline.group_test(b, bt, labels=labels) but `labels`; also the (P, C) t and (P, N) R behind them."""
    (C, H) = b.shape
    U = bt.shape[1]
    S = H + U
    N = int(round(util.C_to_N(C)))
    P = labels.shape[0]
    X = np.concatenate([b, bt], axis=1)
    E = edges_of(N)
    (xc, q) = centre(X)
    observed = [0] * H + [1] * U
    live = q != 0.0                                              # a constant connection: t NaN, no part in any sum, maximum or count

    def stats(lab):
        t = np.array([_t_of(xc[c], q[c], lab, S, U, H) for c in range(C)])
        R = np.array([sum(t[c] ** 2 for c in E[n] if live[c]) for n in range(N)])
        return t, R

    (t, region) = stats(observed)
    tp = np.zeros((P, C))
    Rp = np.zeros((P, N))
    for p in range(P):
        (tp[p], Rp[p]) = stats(labels[p])
    null_max_t = np.array([max([0.0] + [abs(tp[p, c]) for c in range(C) if live[c]]) for p in range(P)])
    null_max_region = Rp.max(axis=1)
    count_t = np.array([sum(1 for p in range(P) if live[c] and abs(tp[p, c]) >= abs(t[c])) for c in range(C)], dtype=np.int64)
    count_region = np.array([sum(1 for p in range(P) if Rp[p, n] >= region[n]) for n in range(N)], dtype=np.int64)
    dead = np.isnan(t)
    return {"t": t, "region": region, "null_max_t": null_max_t, "null_max_region": null_max_region, "count_t": count_t,
            "count_region": count_region, "p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)),
            "p_region": (1.0 + count_region) / (1.0 + P),
            "p_fwe_t": np.array([math.nan if dead[c] else (1.0 + sum(1 for v in null_max_t if v >= abs(t[c]))) / (1.0 + P)
                                 for c in range(C)]),
            "p_fwe_region": np.array([(1.0 + sum(1 for v in null_max_region if v >= region[n])) / (1.0 + P) for n in range(N)]),
            "null_t": tp, "null_region": Rp}


def smallest_gap(null, values):
    """Smallest relative gap |a - v| / max(|a|, |v|) between a valid null value and a valid value it is compared with."""
    a = np.asarray(null, dtype=np.float64).reshape(-1)
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    a = a[~np.isnan(a)]
    v = v[~np.isnan(v)]
    if a.size == 0 or v.size == 0:
        return np.inf
    d = np.abs(a[:, None] - v[None, :]) / np.maximum(np.maximum(np.abs(a[:, None]), np.abs(v[None, :])), 1e-300)
    return float(d.min())
