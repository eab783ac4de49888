"""
NumPy reference of the permutation baselines with nuisance covariates (fcdiff_amd.baseline.group_test / network_test with
z_b, z_bt; fcd_baseline_group_glm / fcd_baseline_network_bits_glm): the permutation GLM of Freedman & Lane (1983).
TEST INFRASTRUCTURE ONLY: the product code does not import it.

design        the design by the stated rules, independent of baseline.glm_design: the column choice is
              covariates_ref.design_of's (long double, pivoted Cholesky), the basis a QR factor of the kept unit columns, w_0 the
              least-squares residual of the centred group indicator.
all_t         (t (C,), null_t (P, C)) in one of two forms.  "projection": the definitions as they stand -- residuals on
              [1, Z], d_q = sum_s W[pi[s], q] e_s, t^2 = d_0^2 dof / (Q_e - sum_q d_q^2) -- one permutation at a time.
              "lstsq": the textbook procedure -- the residuals of the nuisance model permuted (e*[pi[s]] = e[s]) and added back
              to its fit, numpy.linalg.lstsq on the full model [1, x, Z] with the RAW covariates, the t of the group
              coefficient from the residual variance and the pseudo-inverse of the normal matrix.
group_test    every key of baseline.group_test(..., z_b=, z_bt=, permutations=) but labels, permutations, design_info; also
              the (P, C) t and (P, N) R behind them.  network_test: the same for the network-based statistic, through
              network_ref's union-find.
Dead connections (both forms): constant rows (min == max), and rows with Q_e <= dead_tol2(S, R) Q_c.
"""
import math

import numpy as np

import baseline_ref as BR
import covariates_ref as CR
import network_ref as NR
from fcdiff_amd import util

# (N, H, U, Q, P, seed): the shapes of the issue, then a Q whose R = 4 lies between the design widths 3 and 5
SHAPES = [
    (5, 4, 3, 1, 40, 0),         # C = 10 < one tile; S = 7 is not a multiple of 4; dof = 4
    (6, 5, 6, 2, 33, 1),         # P is not a multiple of 16
    (18, 20, 13, 4, 48, 2),      # 17 connections per region: a tile of 16 crossed
    (33, 40, 37, 8, 150, 23),    # R = 9; more subjects than lanes; a second block of 128 permutations
    (8, 70, 75, 5, 32, 4),       # S = 145: a second stretch of 128 subjects
    (4, 512, 512, 3, 16, 5),     # S = 1024, the limit
    (7, 9, 8, 3, 20, 6),         # R = 4 between the widths 3 and 5: a zero-padded column
    (7, 9, 8, 5, 20, 7),         # R = 6 between the widths 5 and 9: three zero-padded columns
    (4, 512, 512, 8, 16, 8),     # both limits: W is 72 KB of LDS (the raised limit), the centre kernel's columns 64 KB
]


def dead_tol2(S, R):
    """(8 S R 2^-52)^2: Q_e <= this multiple of Q_c makes a connection dead (DESIGN.md has the derivation)."""
    return (8.0 * S * R * 2.0 ** -52) ** 2


def make_data(N, H, U, Q, P, seed):
    """(b, bt, z_b, z_bt, permutations): baseline_ref's recipe, covariates that differ between the groups and load on the
    data (a slope on every connection), P drawn permutations."""
    rng = np.random.default_rng(1000 + seed)
    C = util.N_to_C(N)
    S = H + U
    Z = rng.normal(0.0, 1.0, (S, Q))
    Z[H:, 0] += 0.7                                               # the first covariate is shifted in the patients
    if Q >= 2:
        Z[:, 1] = (rng.random(S) < 0.5).astype(np.float64)       # a binary one (sex)
        if Z[:, 1].min() == Z[:, 1].max():
            Z[0, 1] = 1.0 - Z[0, 1]
    X = rng.normal(0.3, 0.1, (C, S)) + 0.05 * rng.normal(0.0, 1.0, (C, Q)).dot(Z.T)
    X[:N - 1, H:] += 0.15
    perms = np.stack([rng.permutation(S) for _ in range(P)]).astype(np.int64)
    return X[:, :H].copy(), X[:, H:].copy(), Z[:H].copy(), Z[H:].copy(), perms


def design(z_b, z_bt):
    """(W (S, R), used (Q,) bool, dof) by the rules, see the module docstring."""
    Z = np.concatenate([z_b, z_bt], axis=0).astype(np.float64)               # (Q = 0: the two-sample design)
    (H, U) = (z_b.shape[0], z_bt.shape[0])
    S = H + U
    d = CR.design_of(Z, np.ones(S, dtype=bool))
    used = np.zeros(Z.shape[1], dtype=bool)
    used[d["piv"]] = True
    if d["rank"]:
        (basis, _r) = np.linalg.qr(np.asarray(d["Vp"], dtype=np.float64))
    else:
        basis = np.zeros((S, 0))
    xc = np.array([0.0] * H + [1.0] * U) - U / S
    full = np.concatenate([np.ones((S, 1)), basis], axis=1)
    xr = xc - full.dot(np.linalg.lstsq(full, xc, rcond=None)[0])
    W = np.concatenate([(xr / math.sqrt(xr.dot(xr)))[:, None], basis], axis=1)
    return W, used, S - d["rank"] - 2


def _t_from(d, qe, dof):
    """t of one connection from d (R,) and Q_e: the definitions with their guards."""
    if qe == 0.0:
        return math.nan
    ss = 0.0
    for v in d:
        ss += v * v
    den = qe - ss
    if not den > 0.0:
        return math.copysign(math.inf, d[0])
    return math.copysign(math.sqrt(d[0] * d[0] * dof / den), d[0])


def residuals(X, W):
    """(E (C, S), Q_e (C,)) on [1, w_1 ..]: dead rows are exactly 0 with Q_e = 0."""
    (C, S) = X.shape
    R = W.shape[1]
    E = np.zeros((C, S))
    qe = np.zeros(C)
    for c in range(C):
        if X[c].min() == X[c].max():
            continue
        xc = X[c] - X[c].sum() / S
        e = xc.copy()
        for q in range(1, R):
            e = e - W[:, q] * W[:, q].dot(xc)
        if not e.dot(e) > dead_tol2(S, R) * xc.dot(xc):
            continue
        E[c] = e
        qe[c] = e.dot(e)
    return E, qe


def _projection_t(X, W, dof, perms):
    (E, qe) = residuals(X, W)
    C = X.shape[0]

    def one(pi):
        D = E.dot(W[pi])                                          # (C, R): d_q = sum_s W[pi[s], q] e_s
        return np.array([_t_from(D[c], qe[c], dof) for c in range(C)])

    S = X.shape[1]
    return one(np.arange(S)), np.array([one(pi) for pi in perms]).reshape(len(perms), C)


def _lstsq_t(X, Zraw, H, U, perms):
    """The textbook Freedman-Lane fit; the dead rows by the same two rules, from the nuisance fit's own residuals."""
    (C, S) = X.shape
    x = np.array([0.0] * H + [1.0] * U)
    nuis = np.concatenate([np.ones((S, 1)), Zraw], axis=1)
    full = np.concatenate([np.ones((S, 1)), x[:, None], Zraw], axis=1)
    rank = int(np.linalg.matrix_rank(full))
    dof = S - rank
    vxx = np.linalg.pinv(full.T.dot(full))[1, 1]
    R = rank - 1                                                  # columns of W: the group and the nuisance rank less the constant
    gamma = np.linalg.lstsq(nuis, X.T, rcond=None)[0]
    fit = nuis.dot(gamma).T
    E = X - fit
    dead = np.array([X[c].min() == X[c].max() or
                     not E[c].dot(E[c]) > dead_tol2(S, R) * ((X[c] - X[c].mean()) ** 2).sum() for c in range(C)])

    def one(pi):
        Es = np.empty_like(E)
        Es[:, pi] = E                                             # e*[pi[s]] = e[s]
        Y = fit + Es
        beta = np.linalg.lstsq(full, Y.T, rcond=None)[0]
        res = Y - full.dot(beta).T
        rss = (res * res).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = beta[1] / np.sqrt(rss / dof * vxx)
        return np.where(dead, math.nan, t)

    return one(np.arange(S)), np.array([one(pi) for pi in perms]).reshape(len(perms), C)


def all_t(b, bt, z_b, z_bt, perms, form="projection"):
    X = np.concatenate([b, bt], axis=1)
    (H, U) = (b.shape[1], bt.shape[1])
    if form == "lstsq":
        return _lstsq_t(X, np.concatenate([z_b, z_bt], axis=0), H, U, perms)
    (W, _used, dof) = design(z_b, z_bt)
    return _projection_t(X, W, dof, perms)


def group_from_t(t, tp, N):
    """baseline_ref.group_test's summaries from the observed t (C,) and the permuted t (P, C)."""
    (P, C) = tp.shape
    E = BR.edges_of(N)
    live = ~np.isnan(t)

    def sums(tt):
        return np.array([sum(tt[c] ** 2 for c in E[n] if live[c]) for n in range(N)])

    region = sums(t)
    Rp = np.array([sums(tp[p]) for p in range(P)]).reshape(P, N)
    null_max_t = np.array([max([0.0] + [abs(tp[p, c]) for c in range(C) if live[c]]) for p in range(P)])
    null_max_region = Rp.max(axis=1)
    count_t = np.array([sum(1 for p in range(P) if live[c] and abs(tp[p, c]) >= abs(t[c])) for c in range(C)], dtype=np.int64)
    count_region = np.array([sum(1 for p in range(P) if Rp[p, n] >= region[n]) for n in range(N)], dtype=np.int64)
    dead = ~live
    return {"t": t, "region": region, "null_max_t": null_max_t, "null_max_region": null_max_region, "count_t": count_t,
            "count_region": count_region, "p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)),
            "p_region": (1.0 + count_region) / (1.0 + P),
            "p_fwe_t": np.array([math.nan if dead[c] else (1.0 + sum(1 for v in null_max_t if v >= abs(t[c]))) / (1.0 + P)
                                 for c in range(C)]),
            "p_fwe_region": np.array([(1.0 + sum(1 for v in null_max_region if v >= region[n])) / (1.0 + P) for n in range(N)]),
            "null_t": tp, "null_region": Rp}


def group_test(b, bt, z_b, z_bt, perms, t_pair=None):
    (t, tp) = t_pair if t_pair is not None else all_t(b, bt, z_b, z_bt, perms)
    return group_from_t(t, tp, int(round(util.C_to_N(b.shape[0]))))


def network_test(b, bt, z_b, z_bt, perms, threshold, tail="both", t_pair=None):
    t_pair = t_pair if t_pair is not None else all_t(b, bt, z_b, z_bt, perms)
    return NR.network_test(b, bt, None, threshold, tail, t_pair=t_pair)


def gaps_group(ref, exclude=None):
    """
    Smallest relative gap between a null value and the observed value it is compared with, over the four comparisons, in
    t^2 units for the t's.  exclude (P,) bool: rows that reproduce the observed statistics bit for bit by construction.
    """
    keep = np.ones(ref["null_t"].shape[0], dtype=bool) if exclude is None else ~np.asarray(exclude)
    (t2, n2) = (ref["t"] ** 2, ref["null_t"][keep] ** 2)
    C = t2.shape[0]
    gaps = [BR.smallest_gap(n2[:, c], t2[c]) for c in range(C)]
    gaps += [BR.smallest_gap(ref["null_region"][keep][:, n], ref["region"][n]) for n in range(ref["region"].shape[0])]
    gaps.append(BR.smallest_gap(ref["null_max_t"][keep] ** 2, t2))
    gaps.append(BR.smallest_gap(ref["null_max_region"][keep], ref["region"]))
    return min(gaps)
