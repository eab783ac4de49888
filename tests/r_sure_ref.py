"""
NumPy restatement of the r pass's rule of decided sites (fcd_common.h: R_SURE_T; gibbs_r_bounds_kernel and
gibbs_r_range_kernel in fcd_gibbs_r.hip), operation for operation: the lanes' partial sums over m = lane, lane + 64, ...,
the wave's butterfly and the outward slack come out bit for bit, so a prediction of which sites a sparse pass leaves to its
tables is exact.

The log-odds of r_nu = 1 are  off + sum_{m != n} lMd[u][n][m][f_nm][r_m],  off = ln pi - ln(1 - pi).  With the edge modes k*
(f_sure_ref.edge_modes at the call's starting ln gamma and T - DRIFT), for a row n all of whose edges have a mode,
    lo(n,u) = sum_m min_t lMd[u][n][m][k*][t],   hi(n,u) = sum_m max_t ...,   base(n,u) = sum_m lMd[u][n][m][k*][0].
A site is decided 0 iff hi + off < -T, decided 1 iff lo + off > T; a row with an edge without a mode has no decided site
(its bounds are still made, over all k for such an edge), and bounds that touch a non-finite entry are NaN.

Nothing here is fitted to the kernel's output: the constants are the header's, the arithmetic is the rule's.
"""
import numpy as np

import f_sure_ref as R

T = 16.0                # R_SURE_T
X_LO = 1e-6             # R_SURE_X
MIN_SHARE = 0.9         # R_SURE_MIN_SHARE
KIND_R = 3


def edge_ids(N):
    """(N, N) symmetric edge ids c = n(n-1)/2 + m, n > m; 0 on the diagonal (never used)"""
    (n, m) = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    (a, b) = (np.maximum(n, m), np.minimum(n, m))
    return np.where(n == m, 0, a * (a - 1) // 2 + b)


def region_table(lM, N):
    """lM (C, U, 3 types, 3 cases) -> lMd (U, N, N, 3, 2) (region_tables_kernel, symmetric edge ids), zero on the diagonal"""
    E = edge_ids(N)
    with np.errstate(invalid="ignore"):
        t = np.stack([lM[..., 2] - lM[..., 0], lM[..., 1] - lM[..., 2]], axis=-1)        # (C, U, 3, 2)
    lMd = np.ascontiguousarray(np.moveaxis(t[E], 2, 0))                                   # (U, N, N, 3, 2)
    lMd[:, np.arange(N), np.arange(N)] = 0.0
    return lMd


def mode_matrix(N, mode):
    """edge modes (C,) in -1 .. 2 -> (N, N) in 0 .. 3: 3 = no mode, 0 on the diagonal"""
    km = np.where(mode < 0, 3, mode)[edge_ids(N)]
    km[np.arange(N), np.arange(N)] = 0
    return km


def _wave_rows(x):
    """(U, N, N) terms (zero on the diagonal) -> (U, N): lane l adds m = l, l + 64, ... in turn, then the butterfly"""
    (U, N, _) = x.shape
    nch = (N + 63) // 64
    pad = np.zeros((U, N, nch * 64))
    pad[:, :, :N] = x
    pad = pad.reshape(U, N, nch, 64)
    acc = np.zeros((U, N, 64))
    with np.errstate(invalid="ignore"):
        for c in range(nch):
            acc = acc + pad[:, :, c, :]
        return R.wave_sum(acc)


def site_tables(lMd, km):
    """-> hi, lo, base (N, U) and the row flags (N,): gibbs_r_bounds_kernel.  hi and lo are NaN where an entry they use is
    not finite; base is NaN there and in every flagged row"""
    (U, N) = lMd.shape[:2]
    diag = np.eye(N, dtype=bool)[None]
    known = (km < 3)[None] & ~diag
    kk = np.minimum(km, 2)[None, :, :, None, None]
    with np.errstate(invalid="ignore"):
        pick = np.take_along_axis(lMd, np.broadcast_to(kk, (U, N, N, 1, 2)), axis=3)[:, :, :, 0, :]      # (U, N, N, 2)
        flat = lMd.reshape(U, N, N, 6)
        mx = np.where(known, np.fmax(pick[..., 0], pick[..., 1]), np.fmax.reduce(flat, axis=3))
        mn = np.where(known, np.fmin(pick[..., 0], pick[..., 1]), np.fmin.reduce(flat, axis=3))
        bad = np.where(known, ~np.isfinite(pick).all(axis=3), ~np.isfinite(flat).all(axis=3)) & ~diag
        mx[np.broadcast_to(diag, mx.shape)] = 0.0
        mn[np.broadcast_to(diag, mn.shape)] = 0.0
        mag = np.fmax(np.abs(mx), np.abs(mn))
        t0 = np.where(known, pick[..., 0], 0.0)
        clean = lambda x: np.where(bad, 0.0, x)              # (the sums of rows with a bad entry are replaced below)
        (hi, lo, base, mg) = (_wave_rows(clean(mx)), _wave_rows(clean(mn)), _wave_rows(clean(t0)), _wave_rows(clean(mag)))
        slack = (float(N + 8) * 1.2e-16) * mg
        hi = hi + slack
        lo = lo - slack
    rowbad = bad.any(axis=2)                                  # (U, N)
    rowflag = ((km == 3) & ~np.eye(N, dtype=bool)).any(axis=1)
    hi[rowbad] = np.nan
    lo[rowbad] = np.nan
    base[rowbad | rowflag[None, :]] = np.nan
    return hi.T.copy(), lo.T.copy(), base.T.copy(), rowflag


def decided(hi, lo, off, rowflag):
    """-> d0, d1 (N, U) bool: the rule at this sweep's off = ln pi - ln(1 - pi)"""
    with np.errstate(invalid="ignore"):
        d0 = (hi + off < -T) & ~rowflag[:, None]
        d1 = ~d0 & (lo + off > T) & ~rowflag[:, None]
    return d0, d1


def tables_for_call(N, U, S_B, lM, lng_start):
    """what a call's bound build makes from its tables and its starting ln gamma: km, lMd, hi, lo, base, rowflag"""
    (a, b) = R.edge_bounds(R.edge_table(lM))
    km = mode_matrix(N, R.edge_modes(S_B, lng_start, U, a, b, R.T - R.DRIFT))
    lMd = region_table(lM, N)
    return (km, lMd) + site_tables(lMd, km)


def share(hi, lo, off, rowflag):
    (d0, d1) = decided(hi, lo, off, rowflag)
    return float((d0 | d1).mean())


def uniforms(N, U, chains, sweep, seed):
    """x (N, U, chains) of the r draws of one sweep: counters (n ceil(U/2) + u/2, chain, sweep, KIND_R), halves by u & 1"""
    npair = (U + 1) // 2
    idx = (np.arange(N)[:, None] * npair + np.arange(npair)[None, :])[:, :, None]
    w = R.philox_words(idx, np.asarray(chains)[None, None, :], sweep, KIND_R, seed).astype(np.uint64)      # (N, npair, chains, 4)
    x = np.empty((N, 2 * npair, len(chains)))
    for h in (0, 1):
        x[:, h::2, :] = (((w[..., 2 * h] << np.uint64(32)) | w[..., 2 * h + 1]) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return x[:, :U, :]


def predict_pass(N, U, G, chain0, seed, sweep, off, f, km, hi, lo, rowflag, x_lo=X_LO):
    """one sparse pass: f (G, C) the state its f pass left.  -> (items left to the tables, decided items evaluated in full);
    an item is a (site, word of 64 chains)"""
    (d0, d1) = decided(hi, lo, off, rowflag)
    E = edge_ids(N)
    offdiag = ~np.eye(N, dtype=bool)
    differs = ((f[:, E] != km[None]) & offdiag[None]).any(axis=2)                   # (G, N)
    x = uniforms(N, U, chain0 + np.arange(G), sweep, seed)
    out = np.where(d0[:, :, None], ~(x >= x_lo), ~(x <= 1.0 - x_lo))                # (N, U, G)
    (sure, exc) = (0, 0)
    for w0 in range(0, G, 64):
        sl = slice(w0, min(G, w0 + 64))
        off_modes = differs[sl].any(axis=0) | rowflag                               # (N,)
        e = (d0 | d1) & (off_modes[:, None] | out[:, :, sl].any(axis=2))
        exc += int(e.sum())
        sure += int(((d0 | d1) & ~e).sum())
    return sure, exc


def exact_log_odds(lM, N, n, u, f_row, r_col, off):
    """the oracle's s1 - s0 of site (n, u) from the edge-major table: f_row (N,) the row's f, r_col (N,) the column's r"""
    E = edge_ids(N)
    (s0, s1) = (0.0, 0.0)
    for m in range(N):
        if m == n:
            continue
        p = lM[E[n, m], u, f_row[m]]
        s0 += p[2] if r_col[m] else p[0]
        s1 += p[1] if r_col[m] else p[2]
    return off + (s1 - s0)
