"""
References for the cleaning front-end (fcdiff_amd.corr.clean, correlations(confounds=, frame_mask=)), independent of the
kernels and of numpy.linalg.

clean_ld       the semantics of fcd_corr_clean (include/fcdiff_hip.h) in extended precision (np.longdouble, as
               corr_ref.corr_edges_ld): masked centring, constant confounds dropped, the rest scaled to unit norm and
               orthogonalised by pivoted, twice-applied modified Gram-Schmidt with the drop rule (remaining squared norm
               below 1e-10: not used -- in exact arithmetic the pivots and remainders of diagonally pivoted Cholesky of
               their Gram matrix), projection (twice), the no-residual rule.  Returns the zero-padded residuals, info,
               and what the tests' conditions on their inputs need: the fraction of centred variance every row keeps and
               the condition number of the unit-scaled Gram matrix of the non-constant confounds.
corr_clean_ld  the Pearson correlation of those residuals over the kept frames, rounded to fp64 last: (C, S), info.
clean_fp64     the kernels' pipeline restated in fp64 NumPy: normal equations of the unit-scaled confounds, pivoted
               Cholesky, substitution, zero padding.  Not a reference: corr_fp64 (= corr_ref.shift_form on its output)
               is there so that the CPU suite shows the bound the GPU tests use is fair.
make_input     the inputs of the GPU tests, shared with the CPU tests.
"""
import numpy as np

import corr_ref as R
from oracle import fcdiff_oracle as O

LD = np.longdouble
DROP_TOL = 1e-10
RSS_TOL = 1e-20


def _mask(frame_mask, S, T):
    return np.ones((S, T), dtype=bool) if frame_mask is None else np.asarray(frame_mask).astype(bool)


def _confounds(confounds, S, T):
    return np.zeros((S, 0, T)) if confounds is None else np.asarray(confounds, dtype=np.float64)


def clean_ld(ts, confounds=None, frame_mask=None):
    """-> dict(resid (S, Nreg, T) longdouble, info (S, 3) int, frac (S, Nreg) rss / ss (NaN: no residual), cond (S,))."""
    ts = np.asarray(ts, dtype=np.float64)
    (S, Nreg, T) = ts.shape
    cf = _confounds(confounds, S, T)
    keep = _mask(frame_mask, S, T)
    resid = np.zeros((S, Nreg, T), dtype=LD)
    info = np.zeros((S, 3), dtype=np.int64)
    frac = np.full((S, Nreg), np.nan)
    cond = np.ones(S)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            Y = ts[s][:, keep[s]]
            X = cf[s][:, keep[s]]
            nk = Y.shape[1]
            info[s] = (nk, 0, nk - 1)
            if nk == 0:
                continue
            if not np.isfinite(X).all():
                continue                # a non-finite kept value in a confound: nothing is solved, every row is zero
            Xc = X.astype(LD)
            Xc = Xc - (Xc.sum(axis=1) / LD(nk))[:, None]
            live = X.min(axis=1) != X.max(axis=1) if X.shape[0] else np.zeros(0, dtype=bool)
            V = Xc[live]
            V = V / np.sqrt((V * V).sum(axis=1))[:, None]
            if V.shape[0]:
                cond[s] = np.linalg.cond(V.dot(V.T).astype(np.float64))
            basis = []
            left = list(range(V.shape[0]))
            W = V.copy()
            while left:
                n2 = np.array([(W[j] * W[j]).sum() for j in left])
                p = int(np.argmax(n2))
                if not n2[p] >= DROP_TOL:
                    break
                q = W[left.pop(p)]
                for _ in range(2):
                    for b in basis:
                        q = q - (q * b).sum() * b
                q = q / np.sqrt((q * q).sum())
                basis.append(q)
                for j in left:
                    W[j] = W[j] - (W[j] * q).sum() * q
            rank = len(basis)
            dof = nk - 1 - rank
            info[s] = (nk, rank, dof)
            if dof < 2:
                continue
            for n in range(Nreg):
                y = Y[n]
                if not np.isfinite(y).all() or y.min() == y.max():
                    continue
                yc = y.astype(LD)
                yc = yc - yc.sum() / LD(nk)
                r = yc.copy()
                for _ in range(2):
                    for b in basis:
                        r = r - (r * b).sum() * b
                (rss, ssq) = ((r * r).sum(), (yc * yc).sum())
                if not rss > LD(RSS_TOL) * ssq:
                    continue
                frac[s, n] = float(rss / ssq)
                resid[s, n, :nk] = r
    return dict(resid=resid, info=info, frac=frac, cond=cond)


def _edges_of_rows(X, fisher_z, ends):
    """Pearson correlation of the rows of X (longdouble, any zero-mean padding of zeros allowed) -> edges, NaN for a zero row."""
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
    return e.astype(np.float64)


def corr_clean_ld(ts, confounds=None, frame_mask=None, fisher_z=False, cleaned=None):
    """-> ((C, S) fp64, info (S, 3)); `cleaned` = a clean_ld result of the same input, to spare the second run."""
    c = cleaned if cleaned is not None else clean_ld(ts, confounds, frame_mask)
    (S, Nreg, _T) = c["resid"].shape
    ends = O.edge_endpoints(Nreg)
    out = np.zeros((ends.shape[0], S), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            out[:, s] = _edges_of_rows(c["resid"][s], fisher_z, ends)
    return (out, c["info"])


def clean_fp64(ts, confounds=None, frame_mask=None):
    """The kernels' arithmetic in fp64 -> (resid (S, Nreg, T) fp64, info)."""
    ts = np.asarray(ts, dtype=np.float64)
    (S, Nreg, T) = ts.shape
    cf = _confounds(confounds, S, T)
    keep = _mask(frame_mask, S, T)
    resid = np.zeros((S, Nreg, T))
    info = np.zeros((S, 3), dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for s in range(S):
            Y = ts[s][:, keep[s]]
            X = cf[s][:, keep[s]]
            (Q, nk) = X.shape
            info[s] = (nk, 0, nk - 1)
            if nk == 0 or not np.isfinite(X).all():
                continue
            ok = np.isfinite(Y).all(axis=1) & (Y.min(axis=1) != Y.max(axis=1))
            Ys = np.where(ok[:, None], Y, 0.0)
            Yc = np.where(ok[:, None], Ys - (Ys.sum(axis=1) / nk)[:, None], 0.0)
            Xc = X - (X.sum(axis=1) / nk)[:, None] if Q else X
            ssx = (Xc * Xc).sum(axis=1)
            live = (X.min(axis=1) != X.max(axis=1)) if Q else np.zeros(0, dtype=bool)
            scale = np.where(live, 1.0 / np.sqrt(np.where(live, ssx, 1.0)), 0.0)
            Xs = Xc * scale[:, None]
            A = Xs.dot(Xs.T)
            B = Xs.dot(Yc.T)
            (piv, taken) = ([], np.zeros(Q, dtype=bool))
            for _k in range(Q):
                d = np.where(taken, -1.0, np.diagonal(A))
                p = int(np.argmax(d))
                if not d[p] >= DROP_TOL:
                    break
                lpp = np.sqrt(d[p])
                free = ~taken
                free[p] = False
                A[free, p] = A[free, p] / lpp
                A[np.ix_(free, free)] -= np.outer(A[free, p], A[free, p])
                A[p, p] = lpp
                taken[p] = True
                piv.append(p)
            rank = len(piv)
            info[s] = (nk, rank, nk - 1 - rank)
            if nk - 1 - rank < 2:
                continue
            L = np.tril(A[np.ix_(piv, piv)]) if rank else np.zeros((0, 0))
            y = B[piv].copy()
            for k in range(rank):
                y[k] = (y[k] - L[k, :k].dot(y[:k])) / L[k, k]
            for k in range(rank - 1, -1, -1):
                y[k] = (y[k] - L[k + 1:, k].dot(y[k + 1:])) / L[k, k]
            beta = np.zeros((Q, Nreg))
            beta[piv] = y * scale[piv][:, None]
            r = Yc - beta.T.dot(Xc) if Q else Yc.copy()
            rss = (r * r).sum(axis=1)
            ssq = (Yc * Yc).sum(axis=1)
            r[~(rss > RSS_TOL * ssq) | ~ok] = 0.0
            resid[s, :, :nk] = r
    return (resid, info)


def corr_fp64(ts, confounds=None, frame_mask=None, fisher_z=False):
    (resid, info) = clean_fp64(ts, confounds, frame_mask)
    return (R.shift_form(resid, R.median8_shift(resid), fisher_z=fisher_z), info)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def random_mask(rs, S, T, drop):
    """A different mask per subject, about `drop` of the frames dropped; frame runs, not single frames, half of the time."""
    m = rs.uniform(size=(S, T)) >= drop / 2
    for s in range(S):
        n_runs = max(1, int(round(drop / 2 * T / 4)))
        for a in rs.randint(0, max(1, T - 4), size=n_runs):
            m[s, a:a + 4] = False
    return m


def chunk_masks(S, T, seed):
    """Masks at the seams of clean_index_kernel's 256-frame chunks and clean_resid_kernel's 256-position blocks, S >= 5 and
    T >= 513: subject 0 keeps frames 256 .. 455 only (nothing kept in the first chunk, n_kept = 200), subject 1 exactly
    frames 0 .. 255 (n_kept = 256, nothing behind the first chunk), subject 2 everything but 256 .. 511 (a whole middle
    chunk dropped), subject 3 everything but frame 0 and 254 .. 257 (a dropped run across the chunk edge), the others
    random_mask at 0.3."""
    assert S >= 5 and T >= 513
    m = random_mask(np.random.RandomState(seed), S, T, 0.3)
    m[0] = False
    m[0, 256:456] = True
    m[1] = False
    m[1, :256] = True
    m[2] = True
    m[2, 256:512] = False
    m[3] = True
    m[3, 0] = False
    m[3, 254:258] = False
    return m


def make_input(seed, S, Nreg, T, Q, drop=0.0, level=0.0, scales=False, mask=None):
    """
    ts (S, Nreg, T): unit noise + a shared component + an O(1) combination of the confounds, on `level`;
    confounds (S, Q, T): unit noise times per-column scales (1e-3 .. 1e3 when `scales`) on a level of its own;
    mask: None when drop == 0, else random_mask; mask="chunk": chunk_masks(S, T, Nreg + T) instead.
    """
    rs = np.random.RandomState(seed)
    sc = np.logspace(-3, 3, Q) if (scales and Q > 1) else np.ones(Q)
    z = rs.standard_normal((S, Q, T))
    cf = (z + 0.5) * sc[None, :, None]
    a = rs.standard_normal((S, Nreg, Q)) / np.sqrt(max(Q, 1))
    ts = rs.standard_normal((S, Nreg, T)) + 0.7 * rs.standard_normal((S, 1, T)) + level
    if Q:
        ts = ts + np.einsum("snq,sqt->snt", a, z)
    m = random_mask(rs, S, T, drop) if drop > 0 else None
    if mask is not None:
        assert mask == "chunk" and drop == 0
        m = chunk_masks(S, T, Nreg + T)
    return (ts, cf if Q else None, m)


def assert_conditions(cleaned, collinear=False):
    """The conditions the GPU tests put on their inputs, on the oracle side: every row that has a residual keeps at least
    1e-6 of its centred variance; the unit-scaled Gram matrix of a set that is not deliberately collinear has a condition
    number below 1e3."""
    f = cleaned["frac"]
    assert not (f[np.isfinite(f)] < 1e-6).any(), "a row keeps %.3g of its variance" % np.nanmin(f)
    if not collinear:
        assert cleaned["cond"].max() < 1e3, "confound Gram condition %.3g" % cleaned["cond"].max()


# ---------------------------------------------------------------------------------------------------------------------
# the inputs tests/test_gpu_corr_clean.py and tests/test_gpu_corr_clean_long.py compare against clean_ld;
# tests/test_corr_clean.py runs corr_fp64 on each
# ---------------------------------------------------------------------------------------------------------------------
GPU_INPUTS = (
    [dict(seed=100 + N + T, S=3, Nreg=N, T=T, Q=0, drop=0.2, level=2.0) for N in (5, 16, 17, 33) for T in (37, 64, 65)]
    + [dict(seed=200 + Q + N, S=3, Nreg=N, T=(130 if N == 17 else 131) if Q > 17 else 64 + Q, Q=Q, drop=d, level=1.0)
       for Q in (1, 3, 15, 16, 17, 63, 64) for N in (17, 33) for d in (0.0, 0.15)]
    + [dict(seed=300 + S, S=S, Nreg=17, T=70, Q=3, drop=0.2, level=0.0) for S in (1, 3, 9)]
    + [dict(seed=400 + Q, S=2, Nreg=20, T=130, Q=Q, drop=0.2, level=100.0, scales=True) for Q in (3, 36, 63)]
    + [dict(seed=500, S=2, Nreg=209, T=40, Q=3, drop=0.1, level=1.0)]
)


# Long scans (tests/test_gpu_corr_clean_long.py): every QP instantiation of clean_resid_kernel that GPU_INPUTS leaves out
# (Q = 25 and 32: QP 32; 41 and 48: 48; 49 and 56: 56), T around one block of 256 output positions (one lane in the second
# block at T = 257), several blocks at T = 513 and 700 -- beyond 96 frames K_corr's subject kernel slices the time axis, and
# behind n_kept its slices hold nothing but the zero padding -- and the chunk-mask cases.
CHUNK_INPUTS = [dict(seed=800 + N + T, S=5, Nreg=N, T=T, Q=Q, drop=0.0, level=2.0, mask="chunk")
                for (N, T, Q) in ((17, 513, 5), (33, 700, 9), (17, 700, 0))]
GPU_LONG_INPUTS = (
    [dict(seed=600 + Q, S=2, Nreg=17, T=320, Q=Q, drop=0.15, level=1.0) for Q in (25, 32, 41, 48, 49, 56)]
    + [dict(seed=700 + N + T, S=3, Nreg=N, T=T, Q=Q, drop=0.3, level=2.0)
       for (N, T, Q) in ((5, 255, 3), (5, 256, 3), (5, 257, 3), (33, 513, 5), (70, 700, 9))]
    + CHUNK_INPUTS
)


def input_id(kw):
    return "S%d-N%d-T%d-Q%d-d%g-l%g%s%s" % (kw["S"], kw["Nreg"], kw["T"], kw["Q"], kw["drop"], kw["level"],
                                            "-sc" if kw.get("scales") else "", "-chunk" if kw.get("mask") else "")


def gpu_case(kw):
    """(ts, confounds, mask, clean_ld result) of one entry of GPU_INPUTS or GPU_LONG_INPUTS, the conditions asserted.  The `scales` cases carry a
    duplicated column behind the set whose condition number is checked."""
    (ts, cf, mask) = make_input(**kw)
    cleaned = clean_ld(ts, cf, mask)
    assert_conditions(cleaned)
    if kw.get("scales"):
        cf = np.concatenate([cf, cf[:, 1:2]], axis=1)
        cleaned = clean_ld(ts, cf, mask)
        assert_conditions(cleaned, collinear=True)
        assert (cleaned["info"][:, 1] == kw["Q"]).all()
    return (ts, cf, mask, cleaned)
