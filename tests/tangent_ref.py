"""
Oracle of fcd_sym_eigh, fcd_tangent_fit and fcd_tangent_apply (fcdiff_amd.corr.sym_eigh / fit_tangent / TangentSpace) in NumPy,
written from the rules of include/fcdiff_hip.h.

Two routes for everything that takes a matrix function:
  "ld"   numpy.longdouble throughout; eigen-decompositions by a cyclic Jacobi (round-robin order) run to 2^-70 ||A||_F;
  "f64"  the chain of fp64 steps of the device -- congruence W R_a W, decomposition (numpy.linalg.eigh), V f(L) V^T -- from the
         same R_a rounded to fp64.  It is ONE sample of what fp64 rounding does to the chain, not its bound.

Rules.  Per subject over its first n frames: live rows, R, alpha and R_a = (1 - a) R + a I as tests/partial_corr_ref.py (its
functions are used); status 3 n outside [0, T], 2 fewer than two live regions, 4 a dead region among at least two live ones,
1 lambda_min <= 1e-12 lambda_max (fit: of R_a; apply: of W R_a W).  Fit: used = status 0; G = mean of the used R_a; geometric:
W = G^-1/2, Tbar = mean logm(W R_a W), stop at ||Tbar||_F <= tol sqrt(Nreg) or after max_iter evaluations, else
G <- G^1/2 expm(Tbar) G^1/2 (symmetrised).  Apply: T_s = logm(W R_a,s W), off-diagonals in (C, S), the diagonal apart.

The unit of an error of an entry of T_s is  n eps kappa(M_s)  (the Frechet derivative of log at an SPD matrix is bounded by
1 / lambda_min, a backward-stable decomposition perturbs M by about n eps ||M||_2); of sym_eigh's eigenvalues and residual
n eps ||A||_2, of V^T V - I  n eps.  kappa and the norms come from this module's "ld" route, never from the device.

R_* below: the worst ratio of the "f64" route to the "ld" route in these units over exactly the inputs of
tests/test_gpu_tangent.py (tangent_cases(), eigh_cases()).  Produced on the CPU by
    python -c "import sys; sys.path[:0] = ['.', 'tests']; import tangent_ref as TR; print(TR.measure_r())"
tests/test_tangent.py recomputes them and asserts that they have not grown; the device is held to 16 times these.  The 16:
the device's Jacobi and its MFMA tile sums add in another order than LAPACK and BLAS, and the route is a sample, not a bound.
R_*_EDGE further down: the same over the inputs of tests/test_gpu_tangent_edges.py (tangent_edge_cases(), eigh_edge_cases()).
"""
import numpy as np

import partial_corr_ref as PR
from oracle import fcdiff_oracle as O

LD = np.longdouble
EPS = 2.0 ** -52
EIG_MIN = 1e-12
(OK, SINGULAR, TOO_FEW, BAD_FRAMES, DEAD_REGION, EIG_FAILED) = range(6)
MARGIN = 16.0
# measure_r() on the CPU (see the module docstring); asserted not to have grown by tests/test_tangent.py
R_T = 0.189
R_EIGH_W = 0.583
R_EIGH_RES = 0.603
R_EIGH_ORTH = 1.14


def round_robin(n, r):
    """the pairs (p < q) of step r of a sweep over n indices by the circle method; an odd n gives one index a bye"""
    m = n + (n & 1)
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (r + k) % (m - 1)])
    b = np.concatenate([[r], (r + (m - 1) - k) % (m - 1)])
    (p, q) = (np.minimum(a, b), np.maximum(a, b))
    keep = q < n
    return (p[keep], q[keep])


def jacobi_eigh(A, dtype=LD, rel=None, max_sweeps=60):
    """(w ascending, V, sweeps) of a symmetric matrix by two-sided cyclic Jacobi in `dtype`: an off-diagonal at or below
    rel ||A||_F is not rotated (default 2^-70 in longdouble, 2^-58 in fp64), a sweep without rotation ends the loop."""
    A = np.array(A, dtype=dtype)
    n = A.shape[0]
    A = np.tril(A) + np.tril(A, -1).T
    V = np.eye(n, dtype=dtype)
    if rel is None:
        rel = 2.0 ** -70 if dtype is LD else 2.0 ** -58
    thr = dtype(rel) * np.sqrt((A * A).sum())
    one = dtype(1)
    for sweep in range(max_sweeps):
        rotated = False
        for r in range(max(n + (n & 1) - 1, 1)):
            (p, q) = round_robin(n, r)
            apq = A[p, q]
            on = np.abs(apq) > thr
            if not on.any():
                continue
            (p, q, apq) = (p[on], q[on], apq[on])
            (app, aqq) = (A[p, p], A[q, q])
            theta = (aqq - app) / (2 * apq)
            t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            c = one / np.sqrt(t * t + one)
            s = t * c
            rotated = rotated or bool((s != 0).any())
            (x, y) = (A[:, p].copy(), A[:, q].copy())
            A[:, p] = c * x - s * y
            A[:, q] = s * x + c * y
            (x, y) = (A[p, :].copy(), A[q, :].copy())
            A[p, :] = c[:, None] * x - s[:, None] * y
            A[q, :] = s[:, None] * x + c[:, None] * y
            A[p, p] = app - t * apq
            A[q, q] = aqq + t * apq
            A[p, q] = 0
            A[q, p] = 0
            (x, y) = (V[:, p].copy(), V[:, q].copy())
            V[:, p] = c * x - s * y
            V[:, q] = s * x + c * y
        if not rotated:
            break
    else:
        raise RuntimeError("jacobi_eigh: no convergence in %d sweeps" % max_sweeps)
    w = np.diagonal(A).copy()
    order = np.argsort(w, kind="stable")
    return (w[order], V[:, order], sweep)


_EIGH_LD = {}


def eigh(M, route):
    """(w, V) by the route; the longdouble route remembers its last few matrices (the callers decompose the same M or G for its
    status, its kappa and its function), which changes no value"""
    if route == "ld":
        key = np.asarray(M, dtype=LD).tobytes()
        if key not in _EIGH_LD:
            while len(_EIGH_LD) >= 8:
                del _EIGH_LD[next(iter(_EIGH_LD))]
            _EIGH_LD[key] = jacobi_eigh(M, LD)[:2]
        return _EIGH_LD[key]
    return np.linalg.eigh(np.asarray(M, dtype=np.float64))


def matfun(M, f, route="ld"):
    """V f(L) V^T, symmetric; raises ValueError where f is log or a root and an eigenvalue is <= EIG_MIN times the largest"""
    (w, V) = eigh(M, route)
    if f is not np.exp and not w[0] > EIG_MIN * w[-1]:
        raise ValueError("an eigenvalue <= 1e-12 of the largest")
    F = (V * f(w)).dot(V.T)
    return (F + F.T) / 2 if route == "ld" else np.tril(F) + np.tril(F, -1).T


def isqrt(w):
    return 1 / np.sqrt(w)


def congruence(W, A, route):
    M = W.dot(A).dot(W)
    return (M + M.T) / 2 if route == "ld" else np.tril(M) + np.tril(M, -1).T


def shrunk(x, shrinkage):
    """x (Nreg, n) -> dict(R_alpha (Nreg, Nreg) longdouble or None, alpha, tol_alpha, n_live, status in (0, 2, 4))"""
    x = np.asarray(x, dtype=np.float64)
    Nreg = x.shape[0]
    live = PR.live_rows(x)
    p = int(live.sum())
    out = dict(R_alpha=None, alpha=np.nan, tol_alpha=0.0, n_live=p, status=TOO_FEW)
    if p < 2:
        return out
    Z = PR.standardise(x[live])
    R = Z.dot(Z.T) / LD(Z.shape[1])
    if isinstance(shrinkage, str):
        assert shrinkage == "ledoit_wolf"
        (a, tol) = PR.ledoit_wolf(Z)
    else:
        (a, tol) = (float(shrinkage), 0.0)
    out.update(alpha=a, tol_alpha=tol, status=OK if p == Nreg else DEAD_REGION)
    if p == Nreg:
        Ra = (LD(1) - LD(a)) * R + LD(a) * np.eye(p, dtype=LD)
        Ra[np.arange(p), np.arange(p)] = LD(1)
        out.update(R_alpha=Ra)
    return out


def subjects(ts, n_frames=None, shrinkage="ledoit_wolf"):
    """the per-subject front half: list of shrunk() dicts, status 3 where n_frames is outside [0, T]; `shrinkage` may be (S,)
    numbers (the device's alphas, so that an error of alpha is not counted again)"""
    ts = np.asarray(ts, dtype=np.float64)
    (S, Nreg, T) = ts.shape
    nf = np.full(S, T, dtype=np.int64) if n_frames is None else np.asarray(n_frames, dtype=np.int64)
    per = not isinstance(shrinkage, str) and np.ndim(shrinkage) == 1
    res = []
    for s in range(S):
        if nf[s] < 0 or nf[s] > T:
            res.append(dict(R_alpha=None, alpha=np.nan, tol_alpha=0.0, n_live=int(PR.live_rows(ts[s][:, :0]).sum()), status=BAD_FRAMES))
            continue
        sh = shrinkage[s] if per else shrinkage
        if not isinstance(sh, str) and not np.isfinite(sh):
            sh = 0.0
        res.append(shrunk(ts[s][:, :nf[s]], sh))
    return res


def _as(M, route):
    return np.asarray(M, dtype=LD) if route == "ld" else np.asarray(M).astype(np.float64)


def reference_of(mats, reference="geometric", tol=1e-10, max_iter=50, route="ld", scale=None):
    """(G, G^1/2, G^-1/2, n_iter (negative: cap hit), last norm) of SPD matrices by the rule of the fit; scale = sqrt(p)"""
    scale = np.sqrt(mats[0].shape[0]) if scale is None else scale
    G = mats[0].copy()
    for M in mats[1:]:
        G = G + M
    G = G / len(mats)
    (n_iter, nrm, converged) = (0, np.nan, reference != "geometric")
    while True:
        Gh = matfun(G, np.sqrt, route)
        W = matfun(G, isqrt, route)
        if reference != "geometric":
            break
        n_iter += 1
        Tb = None
        for M in mats:
            T = matfun(congruence(W, M, route), np.log, route)
            Tb = T if Tb is None else Tb + T
        Tb = Tb / len(mats)
        nrm = float(np.sqrt((Tb * Tb).sum()))
        if nrm <= tol * scale:
            converged = True
            break
        if n_iter >= max_iter:
            break
        G = congruence(Gh, matfun(Tb, np.exp, route), route)
    return (G, Gh, W, n_iter if converged else -n_iter, nrm)


def fit(ts, n_frames=None, shrinkage="ledoit_wolf", reference="geometric", tol=1e-10, max_iter=50, route="ld"):
    """-> dict(G, G_half, W (route's dtype), used, alpha, status, n_live, n_iter (negative: cap hit), grad_norm, kappa_G, mats,
    lam_min: the smallest eigenvalue of each used R_a)"""
    subs = subjects(ts, n_frames, shrinkage)
    Nreg = np.shape(ts)[1]
    lam_min = []
    for r in subs:
        if r["status"] == OK:
            w = eigh(_as(r["R_alpha"], route), route)[0]
            if not w[0] > EIG_MIN * w[-1]:
                r["status"] = SINGULAR
            else:
                lam_min.append(float(w[0]))
    used = np.array([r["status"] == OK for r in subs])
    if used.sum() < 2:
        raise ValueError("%d usable controls of %d, at least 2 are needed" % (used.sum(), len(subs)))
    mats = [_as(r["R_alpha"], route) for r in subs if r["status"] == OK]
    (G, Gh, W, n_iter, nrm) = reference_of(mats, reference, tol, max_iter, route, np.sqrt(Nreg))
    converged = n_iter >= 0
    n_iter = abs(n_iter)
    wG = eigh(G, route)[0]
    return dict(G=G, G_half=Gh, W=W, used=used, alpha=np.array([r["alpha"] for r in subs]), status=np.array([r["status"] for r in subs]),
                n_live=np.array([r["n_live"] for r in subs]), n_iter=n_iter if converged else -n_iter, grad_norm=nrm,
                kappa_G=float(wG[-1] / wG[0]), norm_G=float(max(abs(wG[0]), abs(wG[-1]))), mats=mats,
                tol_alpha=np.array([r["tol_alpha"] for r in subs]), lam_min=np.array(lam_min))


def apply(ts, W, n_frames=None, shrinkage="ledoit_wolf", route="ld"):
    """-> dict(out (C, S), diag (Nreg, S) fp64, status, alpha, n_live, kappa (S,): cond of M_s where status is 0, ratio (S,):
    lambda_min / lambda_max of M_s where status is 0 or 1)"""
    subs = subjects(ts, n_frames, shrinkage)
    (S, Nreg) = (len(subs), np.shape(ts)[1])
    ends = O.edge_endpoints(Nreg)
    res = dict(out=np.full((ends.shape[0], S), np.nan), diag=np.full((Nreg, S), np.nan), kappa=np.full(S, np.nan), ratio=np.full(S, np.nan),
               status=np.array([r["status"] for r in subs]), alpha=np.array([r["alpha"] for r in subs]),
               n_live=np.array([r["n_live"] for r in subs]), tol_alpha=np.array([r["tol_alpha"] for r in subs]))
    W = _as(W, route)
    for (s, r) in enumerate(subs):
        if r["status"] != OK:
            continue
        M = congruence(W, _as(r["R_alpha"], route), route)
        w = eigh(M, route)[0]
        res["ratio"][s] = float(w[0] / w[-1])
        if not w[0] > EIG_MIN * w[-1]:
            res["status"][s] = SINGULAR
            continue
        T = matfun(M, np.log, route)
        res["kappa"][s] = float(w[-1] / w[0])
        res["out"][:, s] = T[ends[:, 0], ends[:, 1]].astype(np.float64)
        res["diag"][:, s] = np.diagonal(T).astype(np.float64)
    return res


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------
FIT_SHAPES = ((17, 40, 12), (33, 100, 12), (33, 40, 12))                # (Nreg, T, H)


def make_series(seed, S, Nreg, T, factors=4):
    """`factors` shared factors with subject-independent loadings plus region noise of sd 0.5 .. 1.5: correlated regions whose
    Ledoit-Wolf R_a stays well conditioned ("tight": the oracle asserts kappa(M_s) <= 100 on them)"""
    L = np.random.default_rng([11, Nreg, factors]).standard_normal((Nreg, factors))         # one population for every seed
    rng = np.random.default_rng([seed, S, Nreg, T])
    x = np.einsum("nf,sft->snt", L, rng.standard_normal((S, factors, T)))
    return x + rng.standard_normal((S, Nreg, T)) * (0.5 + rng.random((S, Nreg, 1)))


def tangent_cases():
    """name -> (ts of the controls, ts of the subjects applied, shrinkage): the fit shapes, and the apply batch of 65"""
    cases = {}
    for (Nreg, T, H) in FIT_SHAPES:
        cases["fit_%d_%d_%d" % (Nreg, T, H)] = (make_series(1, H, Nreg, T), make_series(2, 5, Nreg, T), "ledoit_wolf")
    cases["apply_17_40_65"] = (make_series(1, 12, 17, 40), make_series(3, 65, 17, 40), "ledoit_wolf")
    cases["apply_17_40_33_fixed"] = (make_series(1, 12, 17, 40), make_series(3, 33, 17, 40), 0.3)
    return cases


EIGH_SIZES = (2, 3, 15, 16, 17, 33, 47, 64, 65, 130)


def eigh_matrix(kind, n, seed=0):
    rng = np.random.default_rng([7, n, seed])
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    if kind == "spd":
        X = rng.standard_normal((n, 2 * n))
        return X.dot(X.T) / (2 * n)
    if kind == "indefinite":
        X = rng.standard_normal((n, n))
        return (X + X.T) / 2
    if kind == "diagonal":
        return np.diag(rng.standard_normal(n))
    if kind == "identity":
        return np.eye(n)
    if kind == "repeated":
        w = np.where(np.arange(n) < n // 2, 2.0, rng.random(n) + 3.0)
    else:
        assert kind == "cluster"
        w = np.where(np.arange(n) < 3, 1.0 + 1e-9 * np.arange(n), rng.random(n) + 2.0)
    A = (Q * w).dot(Q.T)
    return (A + A.T) / 2


EIGH_KINDS = ("spd", "indefinite", "diagonal", "identity", "repeated", "cluster")


def eigh_cases():
    """name -> (B, n, n): random SPD / indefinite batches of 5 at every size (2 above 100), the special matrices at 17 and 33"""
    cases = {}
    for n in EIGH_SIZES:
        cases["size_%d" % n] = np.stack([eigh_matrix("spd" if b % 2 else "indefinite", n, b) for b in range(5 if n < 100 else 2)])
    for n in (17, 33):
        cases["kinds_%d" % n] = np.stack([eigh_matrix(k, n) for k in EIGH_KINDS])
    return cases


def eigh_errors(A, w, V, w_ref):
    """the three errors of one decomposition in their units: eigenvalues against w_ref, residual, orthogonality"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    norm = float(max(abs(w_ref[0]), abs(w_ref[-1])))
    unit = n * EPS * norm if norm > 0 else n * EPS
    (w, V) = (np.asarray(w, dtype=LD), np.asarray(V, dtype=LD))
    e_w = float(np.abs(w - w_ref).max()) / unit
    e_res = float(np.abs(A.dot(V) - V * w).max()) / unit
    e_orth = float(np.abs(V.T.dot(V) - np.eye(n)).max()) / (n * EPS)
    return (e_w, e_res, e_orth)


_MEMO = {}


def eigh_reference(name):
    """longdouble eigenvalues of every matrix of a case (memo: shared by the tests)"""
    if ("eigh", name) not in _MEMO:
        _MEMO[("eigh", name)] = [jacobi_eigh(A, LD)[0] for A in eigh_cases()[name]]
    return _MEMO[("eigh", name)]


def tangent_reference(name):
    """(fit "ld", apply "ld" of the applied subjects with the oracle's W) of a tangent case (memo: shared by the tests)"""
    if ("tangent", name) not in _MEMO:
        (tc, ta, sh) = tangent_cases()[name]
        f = fit(tc, shrinkage=sh)
        _MEMO[("tangent", name)] = (f, apply(ta, f["W"], shrinkage=sh))
    return _MEMO[("tangent", name)]


def t_ratio(got_out, got_diag, ref):
    """worst |dT| / (n eps kappa(M_s)) over the status-0 subjects of an apply result `ref`"""
    ok = ref["status"] == OK
    n = ref["diag"].shape[0]
    unit = n * EPS * ref["kappa"][ok]
    e_out = (np.abs(got_out[:, ok] - ref["out"][:, ok]).max(axis=0) / unit).max()
    e_diag = (np.abs(got_diag[:, ok] - ref["diag"][:, ok]).max(axis=0) / unit).max()
    return float(max(e_out, e_diag))


def measure_r(names=None, edge=False):
    """the worst ratios of the "f64" route to the "ld" route over the inputs of the GPU tests -> dict(R_T, R_EIGH_*); edge: over
    the inputs of tests/test_gpu_tangent_edges.py (tangent_edge_cases(), eigh_edge_cases()) -> dict(R_T_EDGE, R_EIGH_*_EDGE)"""
    if edge:
        return _measure_r_edge(names)
    r = dict(R_T=0.0, R_EIGH_W=0.0, R_EIGH_RES=0.0, R_EIGH_ORTH=0.0)
    for name in (names if names is not None else list(tangent_cases())):
        (f, a) = tangent_reference(name)
        assert np.nanmax(a["kappa"]) <= 100.0, (name, np.nanmax(a["kappa"]))
        (_tc, ta, sh) = tangent_cases()[name]
        g = apply(ta, f["W"].astype(np.float64), shrinkage=sh, route="f64")
        assert np.array_equal(g["status"], a["status"])
        r["R_T"] = max(r["R_T"], t_ratio(g["out"], g["diag"], a))
    for (name, batch) in eigh_cases().items():
        if names is not None:
            break
        for (A, w_ref) in zip(batch, eigh_reference(name)):
            (w, V) = np.linalg.eigh(A)
            e = eigh_errors(A, w, V, w_ref)
            for (k, v) in zip(("R_EIGH_W", "R_EIGH_RES", "R_EIGH_ORTH"), e):
                r[k] = max(r[k], v)
    return r


# ---- the inputs of tests/test_gpu_tangent_edges.py ----------------------------------------------------------------------------
# Tables and records of their own: tangent_cases(), eigh_cases() and R_* above stay what tests/test_gpu_tangent.py uses.
# R_*_EDGE: the worst "f64" / "ld" ratios over exactly these inputs, in the units of the module docstring, produced on the CPU by
#     python -c "import sys; sys.path[:0] = ['.', 'tests']; import tangent_ref as TR; print(TR.measure_r(edge=True))"
# The device is held to MARGIN * max(R_x, R_x_EDGE) there: R_x is the family's established sample in the same units, and one new
# input on which LAPACK happens to do very well must not tighten what the same algorithm is already allowed.
R_T_EDGE = 0.0717
R_EIGH_W_EDGE = 0.0754
R_EIGH_RES_EDGE = 0.101
R_EIGH_ORTH_EDGE = 0.347

EIGH_EDGE_SIZES = (1, 32, 96, 97)        # the smallest order; 32 | 33 the 256- and the 1024-thread workgroup; 96 | 97 LDS and scratch
SCALE_N = 33
SCALE_EXACT = (-200, -40, 40, 200)       # ldexp(A, k): the device must give ldexp(w, k) and the bytes of V
SCALE_EXTREME = (-520, 500)              # ||A||_F^2 denormal, and near the overflow
SCALE_OVERFLOW = 520                     # ||A||_F^2 overflows: status 1


def scale_matrix():
    return eigh_matrix("spd", SCALE_N, 1)


def graded_matrix():
    """D A D, D = 10^(-i / 4): lambda_max / lambda_min about 2e16, the entries fall by 10^-16 along the diagonal"""
    D = 10.0 ** (-np.arange(SCALE_N) / 4.0)
    return D[:, None] * scale_matrix() * D[None, :]


def eigh_edge_cases():
    """name -> (B, n, n): batches of 3 (indefinite, SPD, indefinite) at the edge sizes, the graded matrix, the extreme scales"""
    cases = {}
    for n in EIGH_EDGE_SIZES:
        cases["size_%d" % n] = np.stack([eigh_matrix("spd" if b % 2 else "indefinite", n, b) for b in range(3)])
    cases["graded_%d" % SCALE_N] = graded_matrix()[None]
    cases["extreme_%d" % SCALE_N] = np.stack([np.ldexp(scale_matrix(), k) for k in SCALE_EXTREME])
    return cases


def eigh_edge_reference(name):
    """longdouble eigenvalues of every matrix of an edge case (memo)"""
    if ("eigh_edge", name) not in _MEMO:
        _MEMO[("eigh_edge", name)] = [jacobi_eigh(A, LD)[0] for A in eigh_edge_cases()[name]]
    return _MEMO[("eigh_edge", name)]


# the fits whose W the edge cases apply: name -> (controls, shrinkage, reference)
LADDER_ALPHAS = (1e-3, 1e-5, 1e-7, 1e-9)
BOUNDARY_ALPHAS = (1e-10, 1e-14)         # either side of EIG_MIN: kappa about 2e10 (status 0), 2e14 (status 1)
LADDER_FRAMES = 12                       # 11 degrees of freedom for 17 regions: R has a null space, lambda_min(R_a) = alpha


def edge_fits():
    return {"97_60_3": (make_series(1, 3, 97, 60), "ledoit_wolf", "euclidean"),
            "32_40_6": (make_series(1, 6, 32, 40), "ledoit_wolf", "geometric"),
            "17_40_12": (make_series(1, 12, 17, 40), "ledoit_wolf", "geometric")}


def edge_fit(name):
    """the "ld" fit of edge_fits()[name] (memo; 17_40_12 is the fit of tangent_cases()["apply_17_40_65"])"""
    if name == "17_40_12":
        return tangent_reference("apply_17_40_65")[0]
    if ("edge_fit", name) not in _MEMO:
        (tc, sh, kind) = edge_fits()[name]
        _MEMO[("edge_fit", name)] = fit(tc, shrinkage=sh, reference=kind)
    return _MEMO[("edge_fit", name)]


def tangent_edge_cases():
    """name -> dict(fit: a name of edge_fits(), ts (S, Nreg, T), n_frames (S,) or None, shrinkage, kappa: the (low, high) that
    kappa(M_s) of every status-0 subject lies in (tests/test_tangent.py asserts it on the "ld" route))"""
    cases = {"apply_97_60_3": dict(fit="97_60_3", ts=make_series(3, 3, 97, 60), n_frames=None, shrinkage="ledoit_wolf", kappa=(1.0, 100.0)),
             "apply_32_40_33": dict(fit="32_40_6", ts=make_series(2, 33, 32, 40), n_frames=None, shrinkage="ledoit_wolf", kappa=(1.0, 100.0))}
    short = make_series(3, 4, 17, 40)
    for a in LADDER_ALPHAS:
        cases["ladder_%g" % a] = dict(fit="17_40_12", ts=np.ascontiguousarray(short[:, :, :LADDER_FRAMES]), n_frames=None, shrinkage=a,
                                      kappa=(1.0 / a, 10.0 / a))
    # subject 0 keeps its 40 frames (well conditioned), the other three their first 12
    nf = np.array([40] + [LADDER_FRAMES] * 3)
    for a in BOUNDARY_ALPHAS:
        cases["boundary_%g" % a] = dict(fit="17_40_12", ts=short, n_frames=nf, shrinkage=a, kappa=(1.0, 10.0 / a))
    return cases


def tangent_edge_reference(name, shrinkage=None, ts=None, n_frames=None):
    """apply "ld" of an edge case with the oracle's W (memo); `shrinkage`, `ts`, `n_frames`: what the device used, not memoised"""
    c = tangent_edge_cases()[name]
    W = edge_fit(c["fit"])["W"]
    if shrinkage is not None or ts is not None:
        return apply(c["ts"] if ts is None else ts, W, c["n_frames"] if n_frames is None else n_frames,
                     shrinkage=c["shrinkage"] if shrinkage is None else shrinkage)
    if ("tangent_edge", name) not in _MEMO:
        _MEMO[("tangent_edge", name)] = apply(c["ts"], W, c["n_frames"], shrinkage=c["shrinkage"])
    return _MEMO[("tangent_edge", name)]


def mean_tangent(ts, W, shrinkage):
    """(Tbar, kappas): the mean over the subjects of logm(W R_a W) on the "ld" route and kappa(M_s) of each, one decomposition a
    subject -- the stationarity of a fitted W without the fixed point"""
    W = _as(W, "ld")
    (Tb, kappa) = (None, [])
    for r in subjects(ts, None, shrinkage):
        assert r["status"] == OK
        (w, V) = eigh(congruence(W, r["R_alpha"], "ld"), "ld")
        assert w[0] > EIG_MIN * w[-1]
        T = (V * np.log(w)).dot(V.T)
        T = (T + T.T) / 2
        Tb = T if Tb is None else Tb + T
        kappa.append(float(w[-1] / w[0]))
    return (Tb / len(kappa), np.array(kappa))


def euclidean_mean(ts, shrinkage):
    """the mean of R_a in the order of the subjects, longdouble (no decomposition: the Euclidean G at given alphas)"""
    mats = [r["R_alpha"] for r in subjects(ts, None, shrinkage)]
    G = mats[0].copy()
    for M in mats[1:]:
        G = G + M
    return G / len(mats)


def _measure_r_edge(names=None):
    r = dict(R_T_EDGE=0.0, R_EIGH_W_EDGE=0.0, R_EIGH_RES_EDGE=0.0, R_EIGH_ORTH_EDGE=0.0)
    cases = tangent_edge_cases()
    for name in (names if names is not None else list(cases)):
        c = cases[name]
        a = tangent_edge_reference(name)
        ok = a["status"] == OK
        assert c["kappa"][0] <= np.nanmin(a["kappa"]) and np.nanmax(a["kappa"]) <= c["kappa"][1], (name, a["kappa"])
        g = apply(c["ts"], edge_fit(c["fit"])["W"].astype(np.float64), c["n_frames"], shrinkage=c["shrinkage"], route="f64")
        assert np.array_equal(g["status"], a["status"]) and ok.any()
        r["R_T_EDGE"] = max(r["R_T_EDGE"], t_ratio(g["out"], g["diag"], a))
    for (name, batch) in eigh_edge_cases().items():
        if names is not None:
            break
        for (A, w_ref) in zip(batch, eigh_edge_reference(name)):
            (w, V) = np.linalg.eigh(A)
            e = eigh_errors(A, w, V, w_ref)
            for (k, v) in zip(("R_EIGH_W_EDGE", "R_EIGH_RES_EDGE", "R_EIGH_ORTH_EDGE"), e):
                r[k] = max(r[k], v)
    return r


# ---- the scenario of README ---------------------------------------------------------------------------------------------------
# 16 regions, 32 controls, 16 patients, 200 frames: every subject's series are 4 shared factors through the population's
# loadings plus region noise (make_series); a region that is anomalous in a patient (each with probability pi) has its row of
# loadings replaced by a fresh draw -- its couplings to all other regions change, nothing else does.  `recorded`: (healthy
# regions flagged, anomalous regions found) at P(r = 1) > 0.5 after `iters` VB iterations with symmetric edge ids, from the
# oracle's fp64 route and the reference VB loop (tests/test_tangent.py); the device's run must reproduce them.  Each input
# gets the model a user would give it (scenario_theta).  `outcome`: tangent() does NOT win here.  Both inputs find the same 27
# of the 28 anomalous regions; tangent() flags 16 of the 228 healthy ones, correlations() 20.
SCENARIO = dict(N=16, H=32, U=16, T=200, pi=0.1, seed=3, iters=8, factors=4,
                recorded=dict(correlation=(0.0877, 0.9643), tangent=(0.0702, 0.9643)), outcome="tie")


def scenario_series():
    """(ts_controls (H, N, T), ts_patients (U, N, T), r (N, U) bool)"""
    s = SCENARIO
    (N, T, F) = (s["N"], s["T"], s["factors"])
    tc = make_series(s["seed"], s["H"], N, T, F)
    L = np.random.default_rng([11, N, F]).standard_normal((N, F))
    rng = np.random.default_rng([s["seed"], 99])
    r = rng.random((N, s["U"])) < s["pi"]
    tp = np.empty((s["U"], N, T))
    for u in range(s["U"]):
        Lu = np.where(r[:, u][:, None], rng.standard_normal((N, F)), L)
        tp[u] = Lu.dot(rng.standard_normal((F, T))) + rng.standard_normal((N, T)) * (0.5 + rng.random((N, 1)))
    return (tc, tp, r)


def scenario_theta(model, b, kind):
    """The model a user would give each input; pi = the scenario's in both.
    "correlation": the model's own defaults (mu = -0.15, 0, 0.3; sigma = 0.025, 0.035, 0.05), which are made for raw
    correlations.  "tangent": tangent values are deviations from the controls' reference centred at 0, for which the defaults
    mean nothing, so mu and sigma are set from the controls' values b: m and s = their mean and standard deviation,
    mu = m + (-3, 0, 3) s, sigma = (s, s, s)."""
    if kind == "tangent":
        (m, s) = (float(np.nanmean(b)), float(np.nanstd(b)))
        model.mu = np.array([m - 3 * s, m, m + 3 * s])
        model.sigma = np.array([s, s, s])
    else:
        assert kind == "correlation"
    model.pi = SCENARIO["pi"]
    return model


def scenario_rates(lq_R, r):
    """(healthy regions flagged, anomalous regions found), flag = P(r = 1) > 0.5"""
    flag = np.exp(lq_R[:, :, 1]) > 0.5
    return (float(flag[~r].mean()), float(flag[r].mean()))
