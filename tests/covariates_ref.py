"""
Reference for the covariate adjustment (fcdiff_amd.covariates, fcd_edge_cov_fit / fcd_edge_cov_apply of include/fcdiff_hip.h),
independent of the kernels and of numpy.linalg.  TEST INFRASTRUCTURE ONLY: the product code does not import it.

fit_ld      per connection, in np.longdouble: the observed controls, columns centred over them, a column with min == max
            dropped, the rest scaled to unit norm, diagonally pivoted Cholesky of their Gram matrix (diagonal exactly 1
            before the first pivot, ties to the lowest index, remaining squared norm below 1e-10: not used), beta from the
            normal equations of the used columns by substitution, the residual variance from the residuals themselves,
            dof < 1: not fitted.  Returns, beside the outputs of the entry point, what the comparisons' conditions need.
apply_ld    x - sum_q beta (z - z_ref) in longdouble, rounded last.
apply_loop  the same in fp64, q ascending from 0.0, one product and one sum per term: what the device gives bit for bit.
assert_conditions   the conditions under which a fitted row is compared to tolerance.
make_design, make_rows   the inputs of the tests.
"""
import numpy as np

LD = np.longdouble
DROP_TOL = 1e-10
MAX_COLUMNS = 16

# beta in scaled units and adjusted values: atol, rtol 0 (RESID of tests/test_gpu_corr_clean.py); resid_var: rtol
BETA = dict(rtol=0, atol=1e-10)
RESID_VAR = dict(rtol=1e-9, atol=0)


def design_of(z, obs):
    """Steps that depend on the set of observed controls alone: centring, the drop rule, the pivoted factor."""
    Q = z.shape[1]
    n = int(obs.sum())
    d = dict(n=n, rank=0, piv=[], pivots=[], rest=0.0, gap=np.inf, cond=1.0)
    if n < 2:
        return d
    Zo = z[obs].astype(LD)
    Zc = Zo - Zo.sum(axis=0) / LD(n)
    live = [q for q in range(Q) if z[obs, q].min() != z[obs, q].max()]
    nrm = np.sqrt((Zc * Zc).sum(axis=0))
    V = np.zeros((n, Q), dtype=LD)
    for q in live:
        V[:, q] = Zc[:, q] / nrm[q]
    G = V.T.dot(V)
    for q in range(Q):
        G[q, q] = LD(1) if q in live else LD(0)
    (piv, taken) = ([], np.zeros(Q, dtype=bool))
    for _k in range(Q):
        dg = np.where(taken, LD(-1), np.diagonal(G))
        p = int(np.argmax(dg))
        if not dg[p] >= DROP_TOL:
            d["rest"] = float(max(dg[p], 0))
            break
        other = np.delete(dg, p)
        other = other[(other >= 0) & (other != dg[p])]
        if other.size:
            d["gap"] = min(d["gap"], float((dg[p] - other.max()) / dg[p]))
        d["pivots"].append(float(dg[p]))
        lpp = np.sqrt(dg[p])
        free = ~taken
        free[p] = False
        G[free, p] = G[free, p] / lpp
        G[np.ix_(free, free)] -= np.outer(G[free, p], G[free, p])
        G[p, p] = lpp
        taken[p] = True
        piv.append(p)
    rank = len(piv)
    d.update(rank=rank, piv=piv, nrm=nrm, Vp=V[:, piv], L=np.tril(G[np.ix_(piv, piv)]) if rank else np.zeros((0, 0), dtype=LD))
    if rank:
        sv = np.linalg.svd(d["Vp"].astype(np.float64), compute_uv=False)
        d["cond"] = float(sv[0] / sv[-1])
    return d


def fit_one(y, z, missing, cache):
    (H, Q) = z.shape
    obs = ~np.isnan(y) if missing else np.ones(H, dtype=bool)
    key = obs.tobytes()
    if key not in cache:
        cache[key] = design_of(z, obs)
    d = cache[key]
    (n, rank, piv) = (d["n"], d["rank"], d["piv"])
    dof = n - 1 - rank
    out = dict(info=[n, 0, dof, 0], beta=np.zeros(Q), norm=np.zeros(Q), resid_var=np.nan, cond=d["cond"], frac=np.nan,
               pivots=d["pivots"], rest=d["rest"], gap=d["gap"], fitted=False)
    if dof < 1:
        return out
    out["info"] = [n, rank, dof, sum(1 << p for p in piv)]
    out["fitted"] = True
    yo = y[obs].astype(LD)
    yc = yo - yo.sum() / LD(n)
    (L, Vp) = (d["L"], d["Vp"])
    t = Vp.T.dot(yc)
    for k in range(rank):
        t[k] = (t[k] - L[k, :k].dot(t[:k])) / L[k, k]
    for k in range(rank - 1, -1, -1):
        t[k] = (t[k] - L[k + 1:, k].dot(t[k + 1:])) / L[k, k]
    r = yc - Vp.dot(t)
    (rss, ss) = ((r * r).sum(), (yc * yc).sum())
    beta = np.zeros(Q, dtype=LD)
    for (k, p) in enumerate(piv):
        beta[p] = t[k] / d["nrm"][p]
        out["norm"][p] = float(d["nrm"][p])
    out["beta"] = beta.astype(np.float64)
    out["resid_var"] = float(rss / LD(dof))
    out["frac"] = float(rss / ss) if ss > 0 else np.nan
    if np.isnan(y[obs]).any():       # a NaN that is not missing data: the whole row of beta
        out["beta"] = np.full(Q, np.nan)
    return out


def fit_ld(b, z, missing=False):
    """-> dict(beta (C, Q), norm (C, Q) norm of the centred column over the observed controls (0: not used), resid_var (C,),
    info (C, 4), fitted (C,) bool, and per row cond, frac (rss / centred ss), pivots, rest, gap)."""
    b = np.asarray(b, dtype=np.float64)
    (C, H) = b.shape
    z = np.asarray(z, dtype=np.float64).reshape(H, -1)
    (rows, cache) = ([], {})
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(C):
            rows.append(fit_one(b[c], z, missing, cache))
    out = {k: np.array([r[k] for r in rows]) for k in ("beta", "norm", "resid_var", "cond", "frac", "rest", "gap", "fitted")}
    out["beta"] = out["beta"].reshape(C, z.shape[1])
    out["norm"] = out["norm"].reshape(C, z.shape[1])
    out["info"] = np.array([r["info"] for r in rows], dtype=np.int64).reshape(C, 4)
    out["pivots"] = [r["pivots"] for r in rows]
    return out


def assert_conditions(ref, rows=None):
    """For the fitted rows among `rows` (default all): design condition < 1e2, no pivot or rest between 1e-12 and 1e-8, the
    residual keeps >= 1e-6 of the centred sum of squares."""
    idx = [c for c in (range(len(ref["fitted"])) if rows is None else rows) if ref["fitted"][c]]
    for c in idx:
        assert ref["cond"][c] < 1e2, "row %d: design condition %.3g" % (c, ref["cond"][c])
        for d in list(ref["pivots"][c]) + [ref["rest"][c]]:
            assert not (1e-12 < d < 1e-8), "row %d: remaining squared norm %.3g" % (c, d)
        assert ref["frac"][c] >= 1e-6, "row %d keeps %.3g of its sum of squares" % (c, ref["frac"][c])
    return idx


def default_z_ref(z_b):
    z_b = np.asarray(z_b, dtype=np.float64)
    return z_b.mean(axis=0) if z_b.shape[0] else np.zeros(z_b.shape[1])


def apply_ld(x, z, z_ref, beta):
    d = np.einsum("cq,sq->cs", np.asarray(beta, dtype=LD), np.asarray(z, dtype=LD) - np.asarray(z_ref, dtype=LD)[None, :])
    return (np.asarray(x, dtype=LD) - d).astype(np.float64)


def apply_loop(x, z, z_ref, beta):
    x = np.asarray(x, dtype=np.float64)
    (z, z_ref, beta) = (np.asarray(z, dtype=np.float64), np.asarray(z_ref, dtype=np.float64), np.asarray(beta, dtype=np.float64))
    d = np.zeros(x.shape)
    for q in range(z.shape[1]):
        d = d + beta[:, q][:, None] * (z[:, q] - z_ref[q])[None, :]
    return x - d


def adjust_ld(b, bt, z_b, z_bt, missing=False):
    """(b_adj, bt_adj, ref): the whole adjustment on the reference alone."""
    ref = fit_ld(b, z_b, missing)
    z_ref = default_z_ref(z_b)
    return apply_ld(b, z_b, z_ref, ref["beta"]), apply_ld(bt, z_bt, z_ref, ref["beta"]), ref


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_design(rng, H, Q):
    """(H, Q) with orthogonal centred columns (condition 1 over all controls, small over most of them), each on a scale
    and a level of its own."""
    if Q == 0:
        return np.zeros((H, 0))
    g = rng.standard_normal((H, Q))
    g = g - g.mean(axis=0)
    (o, _r) = np.linalg.qr(g)
    return o * np.sqrt(H) * np.logspace(-1, 1, Q)[None, :] + rng.standard_normal(Q)[None, :]


def make_rows(rng, C, z, nan=0.0):
    """(C, H): level + fitted part + noise, the centred row of norm about 0.7 (values of about 1 / sqrt(H)); `nan`: share of
    entries set to NaN.  The noise lies in the residual space of the all-controls design (of full column rank) and has norm
    0.3 to 0.6, so that a complete row keeps a residual also where that space has one dimension (H = Q + 2)."""
    (H, Q) = z.shape
    zc = z - z.mean(axis=0) if Q else z
    zu = zc / np.sqrt((zc * zc).sum(axis=0)) if Q else zc
    a = rng.standard_normal((C, Q)) * (0.5 / np.sqrt(max(Q, 1)))
    (o, _r) = np.linalg.qr(np.concatenate([np.ones((H, 1)), zu], axis=1), mode="complete")
    e = rng.standard_normal((C, H - 1 - Q)).dot(o[:, Q + 1:].T)
    e = e / np.sqrt((e * e).sum(axis=1, keepdims=True)) * rng.uniform(0.3, 0.6, (C, 1))
    b = 0.3 * rng.standard_normal((C, 1)) + a.dot(zu.T) + e
    if nan > 0:
        b[rng.random((C, H)) < nan] = np.nan
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the scenario of the change's motivation: patients "older" than the controls, connections of regions 0-3 drift with age
# ---------------------------------------------------------------------------------------------------------------------
SCENARIO = dict(N=16, H=32, U=16, seed=7, pi=0.1, zseed=3, shift=1.5, slope=0.06, slope1=0.01, regions=4, iters=8)


def scenario_data(model):
    """(b0, bt0, b, bt, z_b, z_bt, r (N, U) bool): `model` (pi already SCENARIO['pi']) sampled -> (b0, bt0); the covariate
    effect added -> (b, bt)."""
    from oracle import fcdiff_oracle as O
    s = SCENARIO
    (r, _t, _f, _ft, b0, bt0) = model.sample_fast(s["N"], s["H"], s["U"], seed=s["seed"])
    (b0, bt0) = (np.array(b0, dtype=np.float64), np.array(bt0, dtype=np.float64))
    rng = np.random.default_rng(s["zseed"])
    z_b = rng.standard_normal((s["H"], 2))
    z_bt = rng.standard_normal((s["U"], 2))
    z_bt[:, 0] += s["shift"]
    C = b0.shape[0]
    ends = O.edge_endpoints(s["N"])
    touch = (ends < s["regions"]).any(axis=1)
    slopes = np.zeros((C, 2))
    slopes[touch, 0] = s["slope"]
    slopes[:, 1] = s["slope1"] * rng.standard_normal(C)
    return b0, bt0, b0 + slopes.dot(z_b.T), bt0 + slopes.dot(z_bt.T), z_b, z_bt, np.asarray(r, dtype=bool)


def scenario_rates(lq_R, r):
    """(healthy regions flagged: all, healthy regions flagged: regions 0-3, anomalous regions found), flag = P(r = 1) > 0.5."""
    flag = np.exp(lq_R[:, :, 1]) > 0.5
    k = SCENARIO["regions"]
    return float(flag[~r].mean()), float(flag[:k][~r[:k]].mean()), float(flag[r].mean())
