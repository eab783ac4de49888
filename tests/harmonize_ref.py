"""
Reference for the site harmonisation (fcdiff_amd.covariates.fit_harmonization / SiteHarmonization.apply, fcd_site_harmonize_fit
/ fcd_site_harmonize_apply of include/fcdiff_hip.h), independent of the kernels and of the package's host code.  TEST
INFRASTRUCTURE ONLY: the product code does not import it.

design_ld   the design of the within-site fit in np.longdouble: columns centred within each site, a column constant within
            every site dropped, the rest scaled to unit norm, diagonally pivoted Cholesky of their Gram matrix (ties to the
            lowest index, remaining squared norm below 1e-10: not used).
fit_ld      the statistic, definition by definition, in np.longdouble (loops over sites and columns, arrays over the
            connections): within-site residuals, sigma2 = sum e^2 / n, alpha, abar, gamma_hat, delta2_hat, the rules for
            "fitted", the priors in two passes, the empirical-Bayes fixed point with the stopping rule of the header.
apply_ld    ((x - m) - shift) / scale + m in longdouble, rounded last;  apply_loop: the same in fp64, one rounded operation per
            step in the stated order: what the device gives bit for bit.
assert_conditions   what the comparisons' tolerances rest on.
make_sites, make_design, make_rows   the inputs of the tests;  SCENARIO, scenario_data, scenario_rates: the scenario.
"""
import numpy as np

LD = np.longdouble
DROP_TOL = 1e-10
EB_TOL = LD(1e-13)
EB_MAX_STEPS = 1000
SLOW_RATIO = 0.99          # 1e-13 / (1 - 0.99) = 1e-11: a tenth of FIT's rtol
MAX_SITES = 64
MAX_COLUMNS = 8
MAX_CONTROLS = 4096
(FITTED, ST_DOF, ST_CONSTANT, ST_NAN, ST_SITE) = (0, 1, 2, 3, 4)

FIT = dict(rtol=1e-10, atol=1e-12)         # the FIT tolerance of tests/test_gpu_covariates.py


def design_ld(z, idx, B):
    """-> dict(piv, mask, Qp, W (H, Qp) LD orthonormal, nrm (Q,), z_bar (B, Q) LD, pivots, rest): see the module's text."""
    z = np.asarray(z, dtype=np.float64)
    (H, Q) = z.shape
    z_bar = np.zeros((B, Q), dtype=LD)
    zc = np.zeros((H, Q), dtype=LD)
    live = np.zeros(Q, dtype=bool)
    for i in range(B):
        rows = idx == i
        if rows.any():
            z_bar[i] = z[rows].astype(LD).sum(axis=0) / LD(int(rows.sum()))
            zc[rows] = z[rows].astype(LD) - z_bar[i]
            live |= z[rows].min(axis=0) != z[rows].max(axis=0)
    zc[:, ~live] = 0
    nrm = np.sqrt((zc * zc).sum(axis=0))
    V = np.zeros((H, Q), dtype=LD)
    for q in np.flatnonzero(live):
        V[:, q] = zc[:, q] / nrm[q]
    G = V.T.dot(V)
    for q in range(Q):
        G[q, q] = LD(1) if live[q] else LD(0)
    (piv, pivots, rest, taken) = ([], [], 0.0, np.zeros(Q, dtype=bool))
    for _k in range(Q):
        dg = np.where(taken, LD(-1), np.diagonal(G))
        p = int(np.argmax(dg))
        if not dg[p] >= DROP_TOL:
            rest = float(max(dg[p], 0))
            break
        pivots.append(float(dg[p]))
        lpp = np.sqrt(dg[p])
        free = ~taken
        free[p] = False
        G[free, p] = G[free, p] / lpp
        G[np.ix_(free, free)] -= np.outer(G[free, p], G[free, p])
        G[p, p] = lpp
        taken[p] = True
        piv.append(p)
    # an orthonormal basis of the used columns by modified Gram-Schmidt in pivot order (any basis gives the same fit)
    W = np.zeros((H, len(piv)), dtype=LD)
    for (k, p) in enumerate(piv):
        w = V[:, p].copy()
        for _twice in range(2):
            for m in range(k):
                w = w - W[:, m] * (W[:, m] * w).sum()
        W[:, k] = w / np.sqrt((w * w).sum())
    return dict(piv=piv, mask=sum(1 << p for p in piv), Qp=len(piv), W=W, V=V, nrm=nrm, z_bar=z_bar, pivots=pivots, rest=rest)


def _moments(v):
    """(members, mean, variance ddof 1) of the entries of v that exist (not NaN), in two passes."""
    x = v[~np.isnan(v)]
    n = x.size
    mean = x.sum() / LD(n) if n >= 1 else LD(np.nan)
    var = ((x - mean) * (x - mean)).sum() / LD(n - 1) if n >= 2 else LD(np.nan)
    return n, mean, var


def eb_fixed_point(gh, dh, n_i, gbar, tau2, a, b):
    """The fixed point per connection for one site (arrays over the connections, all of them fitted) ->
    (gamma_star, delta2_star, steps, hit the cap, contraction ratio of the last two steps)."""
    K = gh.shape[0]
    nn = n_i.astype(LD)
    ss = np.where(n_i >= 2, (nn - 1) * np.where(n_i >= 2, dh, 0), LD(0))
    g = gh.copy()
    d2 = np.where(n_i >= 2, dh, b / (a - 1))
    steps = np.zeros(K, dtype=np.int64)
    (last, before) = (np.zeros(K, dtype=LD), np.zeros(K, dtype=LD))
    run = n_i >= 1
    g[~run] = gbar
    d2[~run] = b / (a - 1)
    while run.any() and steps.max() < EB_MAX_STEPS:
        k = np.flatnonzero(run)
        g1 = (nn[k] * tau2 * gh[k] + d2[k] * gbar) / (nn[k] * tau2 + d2[k])
        dev = gh[k] - g1
        d1 = ((ss[k] + nn[k] * dev * dev) / 2 + b) / (nn[k] / 2 + a - 1)
        (sg, sd) = (np.abs(g1 - g[k]), np.abs(d1 - d2[k]))
        done = (sg <= EB_TOL * (1 + np.abs(g1))) & (sd <= EB_TOL * d1)
        before[k] = last[k]
        last[k] = np.maximum(sg / (1 + np.abs(g1)), sd / d1)
        (g[k], d2[k]) = (g1, d1)
        steps[k] += 1
        run[k[done]] = False
    ratio = np.where(before > 0, last / np.where(before > 0, before, 1), 0).astype(np.float64)
    return g, d2, steps, run.copy(), ratio


def fit_ld(b, idx, B, z=None, missing=False, eb=True, z_ref=None):
    """
    b (C, H), idx (H,) sites 0..B-1, z (H, Q) or None.  -> dict of fp64 arrays named as SiteHarmonization's (prior: the dict;
    prior_defined (B,) bool; members (B, 2)), beta_scaled (C, Q) = beta times the norm of the centred column, mask, z_ref, and
    for assert_conditions: frac (C,) sigma2 n / the row's centred sum of squares, pivots, rest, ratio (B, C), capped (B, C).
    """
    b = np.asarray(b, dtype=np.float64)
    (C, H) = b.shape
    idx = np.asarray(idx)
    z = np.zeros((H, 0)) if z is None else np.asarray(z, dtype=np.float64).reshape(H, -1)
    Q = z.shape[1]
    assert not (Q and missing)
    z_ref = (z.mean(axis=0) if Q else np.zeros(0)) if z_ref is None else np.asarray(z_ref, dtype=np.float64)
    des = design_ld(z, idx, B)
    (W, Qp, piv) = (des["W"], des["Qp"], des["piv"])
    y = b.astype(LD)
    obs = ~np.isnan(b) if missing else np.ones((C, H), dtype=bool)
    n_obs = np.zeros((B, C), dtype=np.int64)
    ybar = np.full((B, C), np.nan, dtype=LD)
    yc = np.zeros((C, H), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(B):
            cols = np.flatnonzero(idx == i)
            n_obs[i] = obs[:, cols].sum(axis=1)
            tot = np.where(obs[:, cols], y[:, cols], 0).sum(axis=1)
            ybar[i] = np.where(n_obs[i] >= 1, tot / np.maximum(n_obs[i], 1).astype(LD), np.nan)
            yc[:, cols] = y[:, cols] - ybar[i][:, None]
        yc = np.where(obs, yc, 0)                    # a missing control adds 0 (a NaN that is not missing stays NaN)
        d = yc.dot(W)                                # (C, Qp)
        e = yc - d.dot(W.T)
        e = np.where(obs, e, 0)
        sse_site = np.stack([(e[:, idx == i] ** 2).sum(axis=1) for i in range(B)])          # (B, C)
        n = n_obs.sum(axis=0)
        Bc = (n_obs >= 1).sum(axis=0)
        sse = sse_site.sum(axis=0)
        status = np.where(n - Bc - Qp < 1, ST_DOF, np.where(np.isnan(sse), ST_NAN, np.where(sse > 0, FITTED, ST_CONSTANT)))
        fitted = status == FITTED
        sigma2 = np.where(fitted, sse / np.maximum(n, 1).astype(LD), np.nan)
        sigma = np.sqrt(sigma2)
        # slopes: the coefficients t on the unit-norm used columns solve V_p t = W d
        t = np.zeros((C, Q), dtype=LD)
        if Qp:
            R = W.T.dot(des["V"][:, piv])            # V_p = W R, R upper triangular (W is Gram-Schmidt of V_p in this order)
            tp = np.zeros((C, Qp), dtype=LD)
            for k in range(Qp - 1, -1, -1):
                tp[:, k] = (d[:, k] - tp[:, k + 1:].dot(R[k, k + 1:])) / R[k, k]
            t[:, piv] = tp
        nrm = np.where(des["nrm"] > 0, des["nrm"], 1)
        beta = np.where(fitted[:, None], t / nrm[None, :], np.nan)
        alpha = ybar - (des["z_bar"] - z_ref.astype(LD)[None, :]).dot(beta.T)               # (B, C)
        abar = np.where(n_obs >= 1, n_obs.astype(LD) / np.maximum(n, 1).astype(LD)[None, :] * alpha, 0).sum(axis=0)
        abar = np.where(fitted, abar, np.nan)
        gamma_hat = np.where(fitted[None, :] & (n_obs >= 1), (alpha - abar[None, :]) / sigma[None, :], np.nan)
        delta2_hat = np.where(fitted[None, :] & (n_obs >= 2), sse_site / (sigma2[None, :] * (n_obs - 1).astype(LD)), np.nan)
        css = (yc * yc).sum(axis=1)
        frac = np.where(fitted & (css > 0), sse / np.where(css > 0, css, 1), np.nan).astype(np.float64)

    prior = dict((k, np.full(B, np.nan, dtype=LD)) for k in ("gamma_bar", "tau2", "m", "s2", "a", "b"))
    members = np.zeros((B, 2), dtype=np.int64)
    defined = np.zeros(B, dtype=bool)
    gamma_star = np.full((B, C), np.nan, dtype=LD)
    delta2_star = np.full((B, C), np.nan, dtype=LD)
    (shift, scale) = (np.zeros((B, C), dtype=LD), np.ones((B, C), dtype=LD))
    n_iter = np.zeros((B, C), dtype=np.int64)
    (ratio, capped) = (np.zeros((B, C)), np.zeros((B, C), dtype=bool))
    f = np.flatnonzero(fitted)
    for i in range(B):
        if not eb:
            gamma_star[i, f] = gamma_hat[i, f]
            delta2_star[i, f] = delta2_hat[i, f]
            ok = f[(n_obs[i, f] >= 2) & (delta2_hat[i, f] > 0)]
        else:
            (members[i, 0], prior["gamma_bar"][i], prior["tau2"][i]) = _moments(gamma_hat[i, f])
            (members[i, 1], prior["m"][i], prior["s2"][i]) = _moments(delta2_hat[i, f])
            (tau2, m, s2) = (prior["tau2"][i], prior["m"][i], prior["s2"][i])
            defined[i] = bool(members[i].min() >= 2 and tau2 > 0 and np.isfinite(tau2) and s2 > 0 and np.isfinite(s2))
            if not defined[i]:
                continue
            prior["a"][i] = (2 * s2 + m * m) / s2
            prior["b"][i] = (m * s2 + m * m * m) / s2
            (gamma_star[i, f], delta2_star[i, f], n_iter[i, f], capped[i, f], ratio[i, f]) = eb_fixed_point(
                gamma_hat[i, f], delta2_hat[i, f], n_obs[i, f], prior["gamma_bar"][i], tau2, prior["a"][i], prior["b"][i])
            ok = f
        shift[i, ok] = sigma[ok] * gamma_star[i, ok]
        scale[i, ok] = np.sqrt(delta2_star[i, ok])
    out = dict(grand_mean=abar, pooled_sd=sigma, beta=beta, gamma_hat=gamma_hat, delta2_hat=delta2_hat, gamma_star=gamma_star,
               delta2_star=delta2_star, shift=shift, scale=scale)
    out = dict((k, np.asarray(v, dtype=np.float64)) for (k, v) in out.items())
    out["beta_scaled"] = np.asarray(np.where(fitted[:, None], t, np.nan), dtype=np.float64)
    out["norm"] = np.asarray(des["nrm"], dtype=np.float64)
    out.update(n_obs=n_obs, n_iter=n_iter, info=np.stack([n, Bc, np.full(C, Qp), status], axis=1), fitted=fitted,
               prior=dict((k, v.astype(np.float64)) for (k, v) in prior.items()), prior_defined=defined, members=members,
               mask=des["mask"], used=piv, z_ref=z_ref, frac=frac, pivots=des["pivots"], rest=des["rest"], ratio=ratio, capped=capped,
               eb=eb, sites=B)
    return out


def assert_conditions(ref, rows=None):
    """What the tolerances rest on, for the fitted rows among `rows` (default all) -> those rows: no drop decision near 1e-10,
    sigma2 n at least 1e-6 of the row's centred sum of squares, every site's tau2 and s2 > 0 (with eb), no pair at the cap
    and the contraction ratio of the last steps <= 0.5 -- for every pair but those of ref["slow"] (B, C), which this call
    sets: the pairs with a ratio in (0.5, SLOW_RATIO], outlying estimates of sites with two to four controls.  The stopping
    rule leaves at most 1e-13 / (1 - ratio) of the fixed point: 2e-13 of a pair under the first rule, 1e-11 of a slow one,
    both inside FIT's rtol of 1e-10; a ratio above SLOW_RATIO fails here."""
    idx = np.array([c for c in (range(len(ref["fitted"])) if rows is None else rows) if ref["fitted"][c]], dtype=np.int64)
    for d in list(ref["pivots"]) + [ref["rest"]]:
        assert not (1e-12 < d < 1e-8), "remaining squared norm %.3g: a drop decision near the threshold" % d
    if idx.size:
        assert ref["frac"][idx].min() >= 1e-6, "a row keeps %.3g of its sum of squares" % ref["frac"][idx].min()
    if ref["eb"]:
        assert ref["prior_defined"].all(), "sites without a prior: %s" % np.flatnonzero(~ref["prior_defined"])
        assert np.all(ref["prior"]["tau2"] > 0) and np.all(ref["prior"]["s2"] > 0)
        assert not ref["capped"][:, idx].any()
        rows_mask = np.zeros(len(ref["fitted"]), dtype=bool)
        rows_mask[idx] = True
        ref["slow"] = (ref["ratio"] > 0.5) & rows_mask[None, :]
        assert ref["ratio"][:, idx].max(initial=0.0) <= SLOW_RATIO, "contraction ratio %.3g" % ref["ratio"][:, idx].max()
        assert ref["ratio"][~ref["slow"] & rows_mask[None, :]].max(initial=0.0) <= 0.5
    else:
        ref["slow"] = np.zeros(ref["ratio"].shape, dtype=bool)
    return idx


def apply_ld(x, idx, z, ref):
    """x (C, S), idx (S,), z (S, Q) or None, ref = fit_ld's dict (or any dict of grand_mean, beta, shift, scale, z_ref)."""
    x = np.asarray(x, dtype=np.float64)
    (C, S) = x.shape
    Q = ref["beta"].shape[1]
    zz = np.zeros((S, 0)) if z is None else np.asarray(z, dtype=np.float64).reshape(S, Q)
    with np.errstate(invalid="ignore"):
        d = np.nan_to_num(np.asarray(ref["beta"], dtype=LD)).dot((zz.astype(LD) - np.asarray(ref["z_ref"], dtype=LD)[None, :]).T)
        m = np.asarray(ref["grand_mean"], dtype=LD)[:, None] + d
        (sh, sc) = (np.asarray(ref["shift"], dtype=LD)[idx].T, np.asarray(ref["scale"], dtype=LD)[idx].T)          # (C, S)
        out = ((x.astype(LD) - m) - sh) / sc + m
    return np.where((sh == 0) & (sc == 1), x, out.astype(np.float64))


def apply_loop(x, idx, z, grand_mean, beta, shift, scale, z_ref):
    """fp64, q ascending from 0.0, one rounded operation per step: d, m = grand_mean + d, ((x - m) - shift) / scale + m; a pair
    with shift 0 and scale 1 is copied."""
    x = np.asarray(x, dtype=np.float64)
    (C, S) = x.shape
    beta = np.asarray(beta, dtype=np.float64).reshape(C, -1)
    d = np.zeros((C, S))
    with np.errstate(invalid="ignore"):
        for q in range(beta.shape[1]):
            d = d + beta[:, q][:, None] * (np.asarray(z, dtype=np.float64)[:, q] - z_ref[q])[None, :]
        m = np.asarray(grand_mean, dtype=np.float64)[:, None] + d
        (sh, sc) = (np.asarray(shift, dtype=np.float64)[idx].T, np.asarray(scale, dtype=np.float64)[idx].T)
        t = x - m
        t = t - sh
        t = t / sc
        t = t + m
    return np.where((sh == 0.0) & (sc == 1.0), x, t)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_sites(rng, H, B):
    """(H,) uint8: every site has at least two controls (H >= 2 B), the rest spread at random, then shuffled."""
    assert H >= 2 * B
    idx = np.concatenate([np.repeat(np.arange(B), 2), rng.integers(0, B, H - 2 * B)]).astype(np.uint8)
    rng.shuffle(idx)
    return idx


def make_design(rng, H, Q, idx):
    """(H, Q): a level per site and column plus within-site variation on a scale of its own per column."""
    if Q == 0:
        return np.zeros((H, 0))
    B = int(idx.max()) + 1
    return rng.standard_normal((H, Q)) * np.logspace(-0.5, 0.5, Q)[None, :] + rng.standard_normal((B, Q))[idx] + rng.standard_normal(Q)[None, :]


def make_rows(rng, C, idx, z=None, nan=0.0):
    """(C, H): level + site offset + slopes on z + noise whose spread differs by site; values of magnitude below 1."""
    H = idx.shape[0]
    B = int(idx.max()) + 1
    off = 0.05 * rng.standard_normal((C, B))
    spread = rng.uniform(0.6, 1.6, B)[None, :] * rng.uniform(0.85, 1.15, (C, B))
    b = 0.3 * rng.uniform(-1, 1, (C, 1)) + off[:, idx] + 0.1 * spread[:, idx] * rng.standard_normal((C, H))
    if z is not None and z.shape[1]:
        zc = (z - z.mean(axis=0)) / z.std(axis=0)
        b = b + (0.03 * rng.standard_normal((C, z.shape[1]))).dot(zc.T)
    if nan > 0:
        b[rng.random((C, H)) < nan] = np.nan
    return b


# ---------------------------------------------------------------------------------------------------------------------
# the scenario of the change's motivation: covariates_ref.SCENARIO's model, 64 controls in two sites of 32, every patient at
# site 1, whose scanner adds an offset per connection and spreads the correlations 1.5 times as wide
# ---------------------------------------------------------------------------------------------------------------------
SCENARIO = dict(N=16, H=64, U=16, seed=7, pi=0.1, sseed=5, offset=0.04, spread=1.5, iters=8)


def scenario_data(model):
    """(b0, bt0, b, bt, site_b, site_bt, r (N, U) bool): `model` (pi already SCENARIO['pi']) sampled -> (b0, bt0); site 1's
    effect added -> (b, bt): x -> mu_c + offset_c + spread (x - mu_c), mu_c the mean of the connection over the controls."""
    s = SCENARIO
    (r, _t, _f, _ft, b0, bt0) = model.sample_fast(s["N"], s["H"], s["U"], seed=s["seed"])
    (b0, bt0) = (np.array(b0, dtype=np.float64), np.array(bt0, dtype=np.float64))
    rng = np.random.default_rng(s["sseed"])
    C = b0.shape[0]
    site_b = np.repeat([0, 1], s["H"] // 2)
    site_bt = np.ones(s["U"], dtype=np.int64)
    off = s["offset"] * rng.standard_normal(C)
    mu = b0.mean(axis=1)

    def at_site_1(x):
        return mu[:, None] + off[:, None] + s["spread"] * (x - mu[:, None])
    b = b0.copy()
    b[:, site_b == 1] = at_site_1(b0[:, site_b == 1])
    return b0, bt0, b, at_site_1(bt0), site_b, site_bt, np.asarray(r, dtype=bool)


def scenario_rates(lq_R, r):
    """(healthy regions flagged, anomalous regions found), flag = P(r = 1) > 0.5."""
    flag = np.exp(lq_R[:, :, 1]) > 0.5
    return float(flag[~r].mean()), float(flag[r].mean())


def harmonize_ld(b, bt, site_b, site_bt, **kw):
    """(b_h, bt_h, ref): the whole harmonisation on the reference alone (sites as indices 0..B-1)."""
    B = int(np.max(site_b)) + 1
    ref = fit_ld(b, site_b, B, **kw)
    return apply_ld(b, site_b, None, ref), apply_ld(bt, site_bt, None, ref), ref
