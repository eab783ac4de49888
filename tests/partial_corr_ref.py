"""
Oracle of fcd_corr_partial (fcdiff_amd.corr.partial_correlations) in numpy.longdouble: the rules of include/fcdiff_hip.h,
restated per subject over its first n frames.

  1  dead regions: a row that holds a non-finite value or is constant over the n frames -- the rows whose edges
     fcd_corr_edges gives as NaN; a single survivor has no finite edge either and is dead too.  p = number of live regions.
  2  R = Z Z^T / n of the live rows, z_it = (x_it - m_i) / s_i, s_i^2 = sum_t (x_it - m_i)^2 / n.
  3  R_a = (1 - a) R + a I; a given, or Ledoit & Wolf (2004): q_t = sum_i z_it^2, B = sum_t q_t^2, F = ||R||_F^2,
     beta = (B / n - F) / (p n), delta = (F - p) / p, a = 0 if delta <= 0 or beta <= 0 else min(beta, delta) / delta.
  4  Theta = R_a^-1 by Gauss-Jordan without pivoting; a pivot <= 1e-12 is status 1, all NaN.
  5  rho_ij = -Theta_ij / sqrt(Theta_ii Theta_jj), clipped to [-1, 1]; fisher_z: atanh.
"""
import numpy as np

from oracle import fcdiff_oracle as O

LD = np.longdouble
PIVOT_MIN = 1e-12
(OK, SINGULAR, TOO_FEW) = (0, 1, 2)


def live_rows(x):
    """(Nreg,) bool of one subject's (Nreg, n) frames."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = np.isfinite(x).all(axis=1) & (x.min(axis=1) != x.max(axis=1)) if x.shape[1] else np.zeros(x.shape[0], dtype=bool)
    if live.sum() < 2:
        live = np.zeros(x.shape[0], dtype=bool)
    return live


def standardise(x):
    """Z (p, n) longdouble of live rows x (p, n)."""
    x = np.asarray(x).astype(LD)
    n = x.shape[1]
    xc = x - (x.sum(axis=1) / LD(n))[:, None]
    return xc / np.sqrt((xc * xc).sum(axis=1) / LD(n))[:, None]


def ledoit_wolf(Z):
    """(alpha, tol_alpha) for standardised rows Z (p, n).  tol_alpha bounds an fp64 evaluation of the same formula: the
    summation-length bound 8 (p^2 + n p) 2^-53 on B / n and F, times the cancellation factor of B / n - F, over p n delta."""
    (p, n) = Z.shape
    R = Z.dot(Z.T) / LD(n)
    q = (Z * Z).sum(axis=0)
    B = (q * q).sum()
    F = (R * R).sum()
    beta = (B / LD(n) - F) / LD(p * n)
    delta = (F - LD(p)) / LD(p)
    if not delta > 0:
        return (0.0, 0.0)
    tol = float(8.0 * (p * p + n * p) * 2.0 ** -53 * (B / LD(n) + F) / (LD(p * n) * delta))
    return (float(min(beta, delta) / delta) if beta > 0 else 0.0, tol)


def invert_ld(A):
    """(inverse, smallest pivot) of a symmetric positive definite longdouble matrix by Gauss-Jordan without pivoting.  The
    pivots are those of the LDL^T factorisation: whatever the blocking of an implementation, it meets the same ones."""
    A = np.array(A, dtype=LD)
    p = A.shape[0]
    least = LD(np.inf)
    for t in range(p):
        piv = A[t, t]
        least = min(least, piv) if piv == piv else LD(-np.inf)
        if not piv > PIVOT_MIN:
            return (None, float(least))
        d = LD(1) / piv
        row = A[t].copy() * d
        col = A[:, t].copy()
        A -= np.outer(col, row)
        A[t] = row
        A[:, t] = -col * d
        A[t, t] = d
    return (A, float(least))


def partial_corr_subject(x, shrinkage="ledoit_wolf", fisher_z=False):
    """
    x (Nreg, n): the subject's counted frames.  -> dict(edges (C,) fp64, alpha, tol_alpha, n_live, status, cond, live, R_alpha
    (longdouble, live block) or None).  With a number for `shrinkage`, alpha is that number and tol_alpha 0.
    """
    x = np.asarray(x, dtype=np.float64)
    Nreg = x.shape[0]
    ends = O.edge_endpoints(Nreg)
    edges = np.full(ends.shape[0], np.nan)
    live = live_rows(x)
    p = int(live.sum())
    out = dict(edges=edges, alpha=np.nan, tol_alpha=0.0, n_live=p, status=TOO_FEW, cond=np.nan, live=live, R_alpha=None)
    if p < 2:
        return out
    Z = standardise(x[live])
    n = Z.shape[1]
    R = Z.dot(Z.T) / LD(n)
    if isinstance(shrinkage, str):
        assert shrinkage == "ledoit_wolf"
        (a, tol) = ledoit_wolf(Z)
    else:
        (a, tol) = (float(shrinkage), 0.0)
    Ra = (LD(1) - LD(a)) * R + LD(a) * np.eye(p, dtype=LD)
    Ra[np.arange(p), np.arange(p)] = LD(1)
    out.update(alpha=a, tol_alpha=tol, R_alpha=Ra)
    (Th, _least) = invert_ld(Ra)
    if Th is None:
        out.update(status=SINGULAR)
        return out
    d = np.sqrt(np.diagonal(Th))
    rho = np.clip(-Th / d[:, None] / d[None, :], LD(-1), LD(1))
    full = np.full((Nreg, Nreg), np.nan, dtype=LD)
    idx = np.flatnonzero(live)
    full[np.ix_(idx, idx)] = rho
    e = full[ends[:, 0], ends[:, 1]]
    if fisher_z:
        with np.errstate(divide="ignore"):
            e = np.arctanh(e)
    out.update(edges=e.astype(np.float64), status=OK, cond=float(np.linalg.cond(Ra.astype(np.float64))))
    return out


def partial_corr_ld(ts, n_frames=None, shrinkage="ledoit_wolf", fisher_z=False):
    """
    ts (S, Nreg, T); n_frames (S,) or None.  `shrinkage`: "ledoit_wolf", a number, or (S,) numbers (one alpha per subject: the
    device's, so that an error of alpha is not counted again in rho).
    -> dict(out (C, S), alpha (S,), tol_alpha (S,), n_live (S,), status (S,), cond (S,)).
    """
    ts = np.asarray(ts, dtype=np.float64)
    (S, Nreg, T) = ts.shape
    nf = np.full(S, T, dtype=np.int64) if n_frames is None else np.asarray(n_frames, dtype=np.int64)
    res = dict(out=np.full((Nreg * (Nreg - 1) // 2, S), np.nan), alpha=np.full(S, np.nan), tol_alpha=np.zeros(S),
               n_live=np.zeros(S, dtype=np.int64), status=np.zeros(S, dtype=np.int64), cond=np.full(S, np.nan))
    per_subject = not isinstance(shrinkage, str) and np.ndim(shrinkage) == 1
    for s in range(S):
        sh = shrinkage[s] if per_subject else shrinkage
        if not isinstance(sh, str) and not np.isfinite(sh):
            sh = 0.0                    # (the device reports NaN where it inverts nothing: the oracle's status says the same)
        r = partial_corr_subject(ts[s][:, :nf[s]], sh, fisher_z)
        res["out"][:, s] = r["edges"]
        for k in ("alpha", "tol_alpha", "n_live", "status", "cond"):
            res[k][s] = r[k]
    return res


def blocked_gauss_jordan_fp64(A, nb=16):
    """The inversion kernel's steps restated in fp64 NumPy, tile by tile.  The matrix is padded to a multiple of nb with
    identity rows and only its lower tiles (I >= J) are kept (the upper ones are NaN here: never read).  Of the Gauss-Jordan
    state, A_IJ = -A_JI^T where exactly one of I, J has been a pivot block already and +A_JI^T otherwise, which gives every
    operand from the lower tiles.  Step k: the pivot block inverted by unblocked Gauss-Jordan (P), the row panel W_J = P A_kJ,
    the update A_IJ -= A_Ik W_J of the lower tiles, the column panel A_Ik = -A_Ik P (I > k) and the row panel A_kI = W_I
    (I < k).  -> (inverse of the leading block, singular flag)."""
    A = np.asarray(A, dtype=np.float64)
    p = A.shape[0]
    PL = (p + nb - 1) // nb * nb
    RT = PL // nb
    M = np.eye(PL)
    M[:p, :p] = A

    def tile(I, J):
        return M[I * nb:(I + 1) * nb, J * nb:(J + 1) * nb]
    for I in range(RT):
        for J in range(I + 1, RT):
            tile(I, J)[:] = np.nan
    sing = False
    for k in range(RT):
        P = tile(k, k).copy()
        for t in range(nb):
            piv = P[t, t]
            if not piv > PIVOT_MIN:
                (sing, piv) = (True, 1.0)
            d = 1.0 / piv
            row = P[t] * d
            col = P[:, t].copy()
            P -= np.outer(col, row)
            P[t] = row
            P[:, t] = -col * d
            P[t, t] = d
        W = {J: P.dot(tile(k, J) if J < k else tile(J, k).T) for J in range(RT) if J != k}
        for I in range(RT):
            if I == k:
                continue
            minus_col = tile(k, I).T if I < k else -tile(I, k)
            for J in range(I + 1):
                if J != k:
                    tile(I, J)[:] += minus_col.dot(W[J])
        for I in range(RT):
            if I > k:
                tile(I, k)[:] = -tile(I, k).dot(P)
            elif I < k:
                tile(k, I)[:] = W[I]
        tile(k, k)[:] = P
    L = np.tril(M)
    return ((L + np.tril(M, -1).T)[:p, :p], sing)


def rho_bound(cond, p):
    """|rho - oracle| allowed at the device's alpha: kappa (2e-11 + 64 p 2^-53).  1e-11 is what the tests of fcd_corr_edges allow
    its correlations, doubled; 64 p 2^-53 the rounding of the p-term sums of the inversion."""
    return cond * (2e-11 + 64.0 * p * 2.0 ** -53)


def make_series(seed, S, Nreg, T, mix=0.3):
    """Rows A G with A = mix N(0, 1) + I (Nreg x Nreg) and G standard normal (Nreg x T), per subject.  At mix = 0.3 the
    unshrunk R grows ill-conditioned with Nreg (the spectrum of A spreads as 0.3 sqrt(Nreg)); mix = 0.3 / sqrt(Nreg) keeps it
    benign at every size."""
    rs = np.random.RandomState(seed)
    A = mix * rs.standard_normal((S, Nreg, Nreg)) + np.eye(Nreg)[None]
    G = rs.standard_normal((S, Nreg, T))
    return np.einsum("sij,sjt->sit", A, G)


def chain(seed=5, n=4000):
    """x1 -> x2 -> x3 with noise 0.5 per link, (1, 3, n)."""
    rs = np.random.RandomState(seed)
    x1 = rs.standard_normal(n)
    x2 = x1 + 0.5 * rs.standard_normal(n)
    x3 = x2 + 0.5 * rs.standard_normal(n)
    return np.stack([x1, x2, x3])[None]
