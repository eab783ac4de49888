"""
Adjust connections for subject covariates (age, sex, site dummies, mean motion, ...) fitted on the controls: the normative
approach.  Not part of the reference; oracle = tests/covariates_ref.py.

For every connection c, ordinary least squares with an implied intercept over the controls observed at c,
    b[c,h] = alpha_c + sum_q beta[c,q] z_b[h,q] + e,
and the same slopes taken out of everybody at a reference point z_ref (default: the mean of z_b over all controls):
    x_adj[c,s] = x[c,s] - sum_q beta[c,q] (z[s,q] - z_ref[q]).
Patients never enter the fit of the slopes, so a disease effect cannot be regressed out; the intercept is left in, so mu and
sigma keep their meaning, and a subject at the reference point is unchanged.  Both steps run on the device
(fcd_edge_cov_fit, fcd_edge_cov_apply of include/fcdiff_hip.h); the adjusted arrays go into fit.b / fit.bt as any arrays do.
"""
import ctypes

import numpy as np

from . import _lib

MAX_COLUMNS = 16


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _check_z(z, name):
    """z as a finite float64 host array (covariates are small: they are checked and kept on the host)."""
    z = np.ascontiguousarray(_host(z), dtype=np.float64)
    if not np.isfinite(z).all():
        raise ValueError("%s holds a non-finite value" % name)
    return z


def _check_columns(Q):
    if Q > MAX_COLUMNS:
        raise NotImplementedError("%d covariate columns, at most %d" % (Q, MAX_COLUMNS))


def _check_fit(b, z_b, z_ref):
    sh = _shape(b)
    if len(sh) != 2:
        raise ValueError("b must have shape (C, H)")
    zh = _shape(z_b)
    if len(zh) != 2:
        raise ValueError("z_b must have shape (H, Q)")
    if zh[0] != sh[1]:
        raise ValueError("z_b has shape %s, b %s: the number of controls must agree" % (zh, sh))
    if sh[0] < 1 or sh[1] < 1:
        raise ValueError("b must hold at least one connection and one control")
    _check_columns(zh[1])
    z = _check_z(z_b, "z_b")
    if z_ref is None:
        ref = z.mean(axis=0)
    else:
        ref = _check_z(z_ref, "z_ref")
        if ref.shape != (zh[1],):
            raise ValueError("z_ref has shape %s, z_b %s: one value per column" % (ref.shape, zh))
    return z, ref


def _check_apply(x, z, C, Q):
    """Shapes of apply()'s arguments for C connections and Q columns -> (shape of x, z flattened to (S, Q), finite)."""
    sh = _shape(x)
    zh = _shape(z)
    if len(sh) == 2:
        if zh != (sh[1], Q):
            raise ValueError("x has shape %s: z must have shape (%d, %d), not %s" % (sh, sh[1], Q, zh))
    elif len(sh) == 3:
        if zh != (sh[1], Q) and zh != (sh[1], sh[2], Q):
            raise ValueError("x has shape %s: z must have shape (U, Q) or (U, K, Q) with Q = %d, not %s" % (sh, Q, zh))
    else:
        raise ValueError("x must have shape (C, S) or (C, U, K)")
    if sh[0] != C:
        raise ValueError("x has %d connections, the adjustment %d" % (sh[0], C))
    if min(sh) < 1:
        raise ValueError("x must not be empty")
    z = _check_z(z, "z")
    if len(sh) == 3:
        z = np.repeat(z[:, None, :], sh[2], axis=1) if z.ndim == 2 else z
        z = np.ascontiguousarray(z.reshape(sh[1] * sh[2], Q))
    return sh, z


def _device_f64(x, ctx):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=ctx.device)
    return t.to(device=ctx.device, dtype=torch.float64).contiguous()


class EdgeAdjustment(object):
    """
    The slopes of every connection on the covariates, as fit_adjustment() made them.  NumPy arrays:
    beta (C, Q)      slope per unit of the ORIGINAL column; 0 for a column not used at that connection
    resid_var (C,)   residual variance of the controls around the fit (NaN: the connection was left unadjusted)
    info (C, 4) int  n_obs, rank (columns used), dof = n_obs - 1 - rank, bit mask of the columns used.  A connection with
                     dof < 1 is left unadjusted: beta row 0, rank and mask 0
    z_ref (Q,)       the reference point; n_columns = Q
    beta and z_ref are all apply() needs: EdgeAdjustment(beta, resid_var, info, z_ref) from saved arrays adjusts new subjects.
    z_b (H, Q), the controls' covariates, is kept for leverage() alone.
    """

    def __init__(self, beta, resid_var, info, z_ref, z_b=None, ctx=None):
        (self.beta, self.resid_var, self.info) = (beta, resid_var, info)
        self.z_ref = np.array(z_ref, dtype=np.float64)
        self.n_columns = int(self.z_ref.shape[0])
        self.z_b = None if z_b is None else np.array(z_b, dtype=np.float64)
        self._ctx = ctx

    def apply(self, x, z, as_numpy=True, ctx=None):
        """
        x (C, S) with z (S, Q), or sessions x (C, U, K) with z (U, Q) (a patient's covariates hold for all its sessions) or
        (U, K, Q).  Returns x - sum_q beta[c,q] (z[s,q] - z_ref[q]) in the shape of x; NaN stays NaN.  For the controls and
        patients of the fit, and later for `bt_new` of score() and `x_new` of membership(): new subjects are adjusted with
        the slopes of the controls the model was fitted on.
        """
        import torch
        (sh, z) = _check_apply(x, z, self.beta.shape[0], self.n_columns)
        ctx = ctx if ctx is not None else (self._ctx if self._ctx is not None else _lib.Context())
        self._ctx = ctx
        xd = _device_f64(x, ctx)
        out = torch.empty_like(xd)
        (C, S, Q) = (sh[0], int(np.prod(sh[1:])), self.n_columns)
        zd = _device_f64(z, ctx) if Q else None
        rd = _device_f64(self.z_ref, ctx) if Q else None
        bd = _device_f64(self.beta, ctx) if Q else None
        ctx.call("fcd_edge_cov_apply", _lib.dptr(xd), C, S, _lib.dptr(zd), Q, _lib.dptr(rd), _lib.dptr(bd), _lib.dptr(out),
                 _lib.stream_ptr())
        return out.cpu().numpy() if as_numpy else out

    def leverage(self, z):
        """
        (S,): (z - z_ref)^T (Z_c^T Z_c)^-1 (z - z_ref) for z (S, Q), Z_c the centred design of ALL controls (pseudo-inverse
        where columns are collinear).  Host NumPy.  What it is for: the slopes are estimates, so an adjusted value carries the
        extra variance resid_var[c] * leverage on top of its own -- small near z_ref, growing with the distance from the
        controls' covariates.  A user who wants the fit to know can add a typical resid_var (its median, say) times the
        subject's leverage to that subject's entry of bt_noise_var.  Nothing is added automatically.
        """
        if self.z_b is None:
            raise ValueError("leverage() needs the controls' covariates: EdgeAdjustment(..., z_b=...)")
        z = _check_z(z, "z")
        if z.ndim != 2 or z.shape[1] != self.n_columns:
            raise ValueError("z must have shape (S, %d)" % self.n_columns)
        if self.n_columns == 0:
            return np.zeros(z.shape[0])
        zc = self.z_b - self.z_b.mean(axis=0)[None, :]
        d = z - self.z_ref[None, :]
        return np.einsum("sq,qr,sr->s", d, np.linalg.pinv(zc.T.dot(zc)), d)


def _fit_checked(b, z, ref, missing_data, ctx):
    """fit_adjustment() behind its host checks: z (H, Q) and ref (Q,) are _check_fit's."""
    import torch
    ctx = ctx if ctx is not None else _lib.Context()
    bd = _device_f64(b, ctx)
    (C, H) = (int(bd.shape[0]), int(bd.shape[1]))
    Q = int(z.shape[1])
    zd = _device_f64(z, ctx) if Q else None
    beta = torch.empty((C, Q), dtype=torch.float64, device=ctx.device)
    resid_var = torch.empty((C,), dtype=torch.float64, device=ctx.device)
    info = torch.empty((C, 4), dtype=torch.int32, device=ctx.device)
    ctx.call("fcd_edge_cov_fit", _lib.dptr(bd), C, H, _lib.dptr(zd), Q, _lib.FCD_DATA_NAN_MISSING if missing_data else 0,
             _lib.dptr(beta) if Q else _lib.dptr(None), _lib.dptr(resid_var), _lib.dptr(info), _lib.stream_ptr())
    return EdgeAdjustment(beta.cpu().numpy(), resid_var.cpu().numpy(), info.cpu().numpy(), ref, z, ctx)


def fit_adjustment(b, z_b, *, missing_data=False, z_ref=None, ctx=None):
    """
    b (C, H) correlations of the controls, z_b (H, Q) their covariates, 0 <= Q <= 16; categorical covariates are dummy columns
    (a full set of them is collinear with the intercept: one is dropped).  missing_data: a NaN b[c,h] leaves control h out of
    connection c's fit, so every connection has its own design; without it a NaN makes that connection's slopes NaN.
    Per connection: columns centred over its observed controls, a constant one dropped, the others scaled to unit norm,
    collinear ones dropped by pivoted Cholesky (remaining squared norm below 1e-10, ties to the lowest index), slopes from
    the normal equations.  z_ref: the point the adjusted values refer to (default: the mean of z_b over all controls).
    Returns an EdgeAdjustment.
    """
    (z, ref) = _check_fit(b, z_b, z_ref)
    return _fit_checked(b, z, ref, missing_data, ctx)


def adjust(b, bt, z_b, z_bt, *, missing_data=False, z_ref=None, ctx=None):
    """fit_adjustment(b, z_b, ...), then both arrays adjusted: (b_adj, bt_adj, adj).  bt may hold sessions (C, U, K)."""
    (z, ref) = _check_fit(b, z_b, z_ref)
    _check_apply(bt, z_bt, _shape(b)[0], z.shape[1])            # before any context exists
    adj = _fit_checked(b, z, ref, missing_data, ctx)
    return adj.apply(b, z_b), adj.apply(bt, z_bt), adj


# ---------------------------------------------------------------------------------------------------------------------
# Site harmonisation (ComBat) fitted on the controls.  Not part of the reference; oracle = tests/harmonize_ref.py.
#
# Location and scale per site and connection, shrunk by empirical Bayes towards the site's law over all connections
# (Johnson et al. 2007; Fortin et al. 2018 for connectivity).  The site parameters come from the CONTROLS ALONE and are then
# applied to everybody: a disease effect cannot be harmonised away, and new patients for score() and membership() are
# harmonised with the parameters of the controls the model was fitted on.  The statistic, its rules and its refusals are
# written out at fcd_site_harmonize_fit in include/fcdiff_hip.h.  ComBat stops all connections jointly at a change of 1e-4;
# this is the same fixed point per (site, connection), solved to 1e-13.  Covariate effects are KEPT, as ComBat keeps them:
# fit_adjustment() on the harmonised arrays removes them.
# Not provided: a reference site, the non-parametric prior, mean-only mode, covariates together with missing_data, site
# parameters per session, harmonisation inside score() / membership() (call h.apply first), feeding delta2_star into
# b_noise_var.
# ---------------------------------------------------------------------------------------------------------------------
MAX_SITES = 64
MAX_SITE_CONTROLS = 4096
MAX_SITE_COLUMNS = 8
SITE_DROP_TOL = 1e-10
SITE_STATUS = {0: "fitted", 1: "too few controls for the sites and columns", 2: "constant within every site",
               3: "a NaN that is not missing data", 4: "a site id out of range"}


def _site_index(labels, sites, name):
    """labels (n,) of any hashable kind -> their places in the sorted list `sites` (uint8); unseen: ValueError."""
    where = dict((s, i) for (i, s) in enumerate(sites))
    try:
        return np.array([where[s] for s in labels], dtype=np.uint8)
    except KeyError as err:
        raise ValueError("%s holds the site %r, which the fit did not see" % (name, err.args[0]))


def _labels(site, name):
    site = _host(site) if hasattr(site, "detach") else site
    if isinstance(site, (str, bytes)) or (hasattr(site, "ndim") and site.ndim != 1):
        raise ValueError("%s must hold one label per subject" % name)
    return list(site.tolist() if hasattr(site, "tolist") else site)


def site_design(z, idx, B):
    """
    The design of the within-site fit, made once on the host in fp64.  z (H, Q) finite, idx (H,) in 0..B-1.
    Columns are centred within each site; a column that is constant within every site is dropped (it is exactly zero after
    the centring); the rest are scaled to unit norm; collinear ones are dropped by diagonally pivoted Cholesky of their
    Gram matrix (remaining squared norm below 1e-10, ties to the lowest index): fit_adjustment's column rules.
    -> W (H, Q') orthonormal basis of the used columns, T (Q, Q') with beta = T (W^T y) per unit of the original columns,
    z_bar (B, Q) the sites' means, design_info = dict(used: the columns in pivot order, mask, norm (Q,) of the centred columns).
    """
    (H, Q) = z.shape
    z_bar = np.zeros((B, Q))
    zc = np.zeros((H, Q))
    live = np.zeros(Q, dtype=bool)
    for i in range(B):
        rows = idx == i
        if rows.any():
            z_bar[i] = z[rows].mean(axis=0)
            zc[rows] = z[rows] - z_bar[i]
            live |= z[rows].min(axis=0) != z[rows].max(axis=0)
    zc[:, ~live] = 0.0
    nrm = np.sqrt((zc * zc).sum(axis=0))
    live &= nrm > 0
    V = np.zeros((H, Q))
    V[:, live] = zc[:, live] / nrm[live]
    G = V.T.dot(V)
    G[np.diag_indices(Q)] = live.astype(np.float64)
    (piv, taken) = ([], np.zeros(Q, dtype=bool))
    for _k in range(Q):
        dg = np.where(taken, -1.0, np.diagonal(G))
        p = int(np.argmax(dg))
        if not dg[p] >= SITE_DROP_TOL:
            break
        lpp = np.sqrt(dg[p])
        free = ~taken
        free[p] = False
        G[free, p] = G[free, p] / lpp
        G[np.ix_(free, free)] -= np.outer(G[free, p], G[free, p])
        G[p, p] = lpp
        taken[p] = True
        piv.append(p)
    Qp = len(piv)
    W = np.zeros((H, Qp))
    T = np.zeros((Q, Qp))
    if Qp:
        L = np.tril(G[np.ix_(piv, piv)])
        Li = np.linalg.inv(L)                   # W = Vp L^-T: W^T W = L^-1 (L L^T) L^-T = 1
        W = V[:, piv].dot(Li.T)
        T[piv, :] = Li.T / nrm[piv][:, None]    # Vp t = W d  =>  t = L^-T d, beta_p = t / norm_p
    info = dict(used=list(piv), mask=int(sum(1 << p for p in piv)), norm=nrm)
    return np.ascontiguousarray(W), np.ascontiguousarray(T), z_bar, info


def _check_harmonize_fit(b, site_b, z_b, missing_data, z_ref):
    """Every host-side check of fit_harmonization() -> (sites, idx (H,) uint8, z (H, Q), z_ref (Q,))."""
    sh = _shape(b)
    if len(sh) != 2:
        raise ValueError("b must have shape (C, H)")
    if sh[0] < 1 or sh[1] < 1:
        raise ValueError("b must hold at least one connection and one control")
    lab = _labels(site_b, "site_b")
    if len(lab) != sh[1]:
        raise ValueError("site_b has %d labels, b %s: one site per control" % (len(lab), sh))
    if sh[1] > MAX_SITE_CONTROLS:
        raise NotImplementedError("%d controls, at most %d" % (sh[1], MAX_SITE_CONTROLS))
    sites = sorted(set(lab))
    if len(sites) > MAX_SITES:
        raise NotImplementedError("%d sites, at most %d" % (len(sites), MAX_SITES))
    idx = _site_index(lab, sites, "site_b")
    counts = np.bincount(idx, minlength=len(sites))
    if counts.min() < 2:
        raise ValueError("site %r has %d control: every site needs at least two" % (sites[int(np.argmin(counts))], counts.min()))
    if z_b is None:
        z = np.zeros((sh[1], 0))
    else:
        zh = _shape(z_b)
        if len(zh) != 2:
            raise ValueError("z_b must have shape (H, Q)")
        if zh[0] != sh[1]:
            raise ValueError("z_b has shape %s, b %s: the number of controls must agree" % (zh, sh))
        if zh[1] > MAX_SITE_COLUMNS:
            raise NotImplementedError("%d covariate columns, at most %d" % (zh[1], MAX_SITE_COLUMNS))
        z = _check_z(z_b, "z_b")
    Q = z.shape[1]
    if Q and missing_data:
        raise NotImplementedError("covariates together with missing_data: every connection would need its own design")
    if z_ref is None:
        ref = z.mean(axis=0) if Q else np.zeros(0)
    else:
        ref = _check_z(z_ref, "z_ref")
        if ref.shape != (Q,):
            raise ValueError("z_ref has shape %s: one value per column of z_b (%d)" % (ref.shape, Q))
    return sites, idx, z, ref


def _check_harmonize_apply(x, site, z, C, Q, sites):
    """Shapes and values of SiteHarmonization.apply()'s arguments -> (shape of x, idx (S,) uint8, z (S, Q))."""
    sh = _shape(x)
    if len(sh) not in (2, 3):
        raise ValueError("x must have shape (C, S) or (C, U, K)")
    lab = _labels(site, "site")
    if len(lab) != sh[1]:
        raise ValueError("site has %d labels, x %s: one site per subject" % (len(lab), sh))
    if z is None:
        if Q:
            raise ValueError("the harmonisation was fitted with %d covariate columns: z is needed" % Q)
        z = np.zeros((sh[1], 0))
    (sh, zf) = _check_apply(x, z, C, Q)
    idx = _site_index(lab, sites, "site")
    if len(sh) == 3:
        idx = np.repeat(idx, sh[2])
    return sh, np.ascontiguousarray(idx), zf


class SiteHarmonization(object):
    """
    What fit_harmonization() made.  NumPy arrays, C connections, B sites (`sites`: their labels, sorted), Q covariate columns:
    grand_mean (C,)   the common level abar_c;  pooled_sd (C,)  sigma_c;  beta (C, Q) slopes per unit of the original column
    gamma_hat, delta2_hat, gamma_star, delta2_star, shift, scale (B, C)    the site effects, raw and shrunk, and what apply() uses
    n_obs (B, C) controls observed;  n_iter (B, C) steps of the fixed-point iteration, negative where it hit its cap of 1000
    info (C, 4) int   n, sites with a control, columns used, status (SITE_STATUS; 0 = fitted).  A connection that is not fitted
                      has NaN in every real array but shift 0 and scale 1, and apply() returns it unchanged
    prior             dict of gamma_bar, tau2, a, b (B,) each (and m, s2, the moments of delta2_hat; members (B, 2))
    z_ref (Q,), design_info (used, mask, norm)
    grand_mean, beta, shift, scale, sites and z_ref are all apply() needs: SiteHarmonization(sites=..., grand_mean=..., beta=...,
    shift=..., scale=..., z_ref=...) from saved arrays harmonises new subjects.
    """
    FIELDS = ("grand_mean", "pooled_sd", "beta", "gamma_hat", "delta2_hat", "gamma_star", "delta2_star", "shift", "scale", "n_obs",
              "n_iter", "info", "prior", "design_info")

    def __init__(self, sites, grand_mean, beta, shift, scale, z_ref, ctx=None, **more):
        self.sites = list(sites)
        self.grand_mean = np.ascontiguousarray(grand_mean, dtype=np.float64)
        C = self.grand_mean.shape[0]
        self.z_ref = np.array(z_ref, dtype=np.float64).reshape(-1)
        self.n_columns = int(self.z_ref.shape[0])
        self.beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(C, self.n_columns)
        (self.shift, self.scale) = (np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64))
        if self.shift.shape != (len(self.sites), C) or self.scale.shape != self.shift.shape:
            raise ValueError("shift and scale must have shape (sites, connections) = (%d, %d)" % (len(self.sites), C))
        if len(self.sites) > MAX_SITES or self.n_columns > MAX_SITE_COLUMNS:
            raise NotImplementedError("at most %d sites and %d covariate columns" % (MAX_SITES, MAX_SITE_COLUMNS))
        for k in self.FIELDS:
            if k not in ("grand_mean", "beta", "shift", "scale"):
                setattr(self, k, more.pop(k, None))
        if more:
            raise TypeError("unknown arrays: %s" % ", ".join(sorted(more)))
        self._ctx = ctx

    def apply(self, x, site, z=None, as_numpy=True, ctx=None):
        """
        x (C, S) with site (S,) labels and z (S, Q), or sessions x (C, U, K) with site (U,) and z (U, Q) or (U, K, Q).
        Returns ((x - m) - shift[site, c]) / scale[site, c] + m,  m = grand_mean[c] + sum_q beta[c,q] (z[s,q] - z_ref[q]), in
        the shape of x; NaN stays NaN; a connection that was not fitted, and a pair the fit left alone, come back unchanged bit
        for bit.  A label the fit did not see is a ValueError.
        """
        import torch
        (sh, idx, zf) = _check_harmonize_apply(x, site, z, self.grand_mean.shape[0], self.n_columns, self.sites)
        ctx = ctx if ctx is not None else (self._ctx if self._ctx is not None else _lib.Context())
        self._ctx = ctx
        xd = _device_f64(x, ctx)
        out = torch.empty_like(xd)
        (C, S, Q) = (sh[0], int(np.prod(sh[1:])), self.n_columns)
        sd = torch.as_tensor(idx, device=ctx.device)
        zd = _device_f64(zf, ctx) if Q else None
        held = [_device_f64(a, ctx) for a in (self.grand_mean, self.shift, self.scale)] + [_device_f64(self.beta, ctx) if Q else None]
        ref = np.ascontiguousarray(self.z_ref)
        d = _lib.HarmonizeDesc.make(C=C, S=S, B=len(self.sites), Q=Q, stream=_lib.stream_ptr(), x=_lib.dptr(xd), site=_lib.dptr(sd),
                                    z=_lib.dptr(zd), z_ref=ref.ctypes.data if Q else None, grand_mean=_lib.dptr(held[0]),
                                    shift=_lib.dptr(held[1]), scale=_lib.dptr(held[2]), beta=_lib.dptr(held[3]), out=_lib.dptr(out))
        ctx.call("fcd_site_harmonize_apply", ctypes.byref(d))
        return out.cpu().numpy() if as_numpy else out


def _harmonize_checked(b, sites, idx, z, ref, missing_data, eb, ctx):
    """fit_harmonization() behind its host checks."""
    import torch
    ctx = ctx if ctx is not None else _lib.Context()
    bd = _device_f64(b, ctx)
    (C, H) = (int(bd.shape[0]), int(bd.shape[1]))
    (B, Q) = (len(sites), int(z.shape[1]))
    (W, T, z_bar, dinfo) = site_design(z, idx, B)
    Qp = int(W.shape[1])
    sd = torch.as_tensor(idx, device=ctx.device)
    Wd = _device_f64(W, ctx) if Qp else None
    f64 = dict(dtype=torch.float64, device=ctx.device)
    i32 = dict(dtype=torch.int32, device=ctx.device)
    o = dict(grand_mean=torch.empty((C,), **f64), pooled_sd=torch.empty((C,), **f64), beta=torch.empty((C, Q), **f64),
             n_obs=torch.empty((B, C), **i32), n_iter=torch.empty((B, C), **i32), info=torch.empty((C, 4), **i32),
             prior=torch.empty((6, B), **f64), prior_info=torch.empty((B, 3), **i32))
    for k in ("gamma_hat", "delta2_hat", "gamma_star", "delta2_star", "shift", "scale"):
        o[k] = torch.empty((B, C), **f64)
    (T, z_bar, ref) = (np.ascontiguousarray(T), np.ascontiguousarray(z_bar), np.ascontiguousarray(ref))
    flags = (_lib.FCD_DATA_NAN_MISSING if missing_data else 0) | (0 if eb else _lib.FCD_HARMONIZE_NO_EB)
    d = _lib.HarmonizeDesc.make(flags=flags, C=C, H=H, B=B, Q=Q, Qp=Qp, stream=_lib.stream_ptr(), b=_lib.dptr(bd), site=_lib.dptr(sd),
                                W=_lib.dptr(Wd), T=T.ctypes.data if Qp else None, z_bar=z_bar.ctypes.data if Q else None,
                                z_ref=ref.ctypes.data if Q else None,
                                **dict((k, _lib.dptr(v if (k != "beta" or Q) else None)) for (k, v) in o.items()))
    ctx.call("fcd_site_harmonize_fit", ctypes.byref(d))
    r = dict((k, v.cpu().numpy()) for (k, v) in o.items())
    (p, pi) = (r.pop("prior"), r.pop("prior_info"))
    if eb and not pi[:, 2].all():
        i = int(np.argmin(pi[:, 2]))
        raise ValueError("site %r: the empirical-Bayes prior is undefined (%d connections with a location estimate, %d with a "
                         "scale estimate, tau2 = %g, s2 = %g); eb=False harmonises without it"
                         % (sites[i], pi[i, 0], pi[i, 1], p[1, i], p[3, i]))
    prior = dict(gamma_bar=p[0], tau2=p[1], m=p[2], s2=p[3], a=p[4], b=p[5], members=pi[:, :2].copy())
    return SiteHarmonization(sites, r.pop("grand_mean"), r.pop("beta"), r.pop("shift"), r.pop("scale"), ref, ctx, prior=prior,
                             design_info=dinfo, **r)


def fit_harmonization(b, site_b, z_b=None, *, missing_data=False, eb=True, z_ref=None, ctx=None):
    """
    b (C, H) correlations of the controls, site_b (H,) their sites (any hashable labels; at most 64 sites, at least two
    controls at each, H <= 4096), z_b (H, Q) covariates whose effects are to be KEPT (Q <= 8; complete data only).
    missing_data: a NaN b[c,h] leaves control h out of connection c; without it a NaN leaves the connection unfitted.
    eb=False: no shrinkage, the raw site effects.  z_ref as in fit_adjustment.  Returns a SiteHarmonization; raises ValueError
    where a site's prior is undefined (fewer than two fitted connections, or no spread over them).
    """
    (sites, idx, z, ref) = _check_harmonize_fit(b, site_b, z_b, missing_data, z_ref)
    return _harmonize_checked(b, sites, idx, z, ref, missing_data, eb, ctx)


def harmonize(b, bt, site_b, site_bt, z_b=None, z_bt=None, **kw):
    """fit_harmonization(b, site_b, z_b, ...), then both arrays harmonised: (b_h, bt_h, h).  bt may hold sessions (C, U, K)."""
    unknown = set(kw) - set(("missing_data", "eb", "z_ref", "ctx"))
    if unknown:
        raise TypeError("unknown arguments: %s" % ", ".join(sorted(unknown)))
    (sites, idx, z, ref) = _check_harmonize_fit(b, site_b, z_b, kw.get("missing_data", False), kw.get("z_ref"))
    _check_harmonize_apply(bt, site_bt, z_bt, _shape(b)[0], z.shape[1], sites)           # before any context exists
    h =_harmonize_checked(b, sites, idx, z, ref, kw.get("missing_data", False), kw.get("eb", True), kw.get("ctx"))
    return h.apply(b, site_b, z_b), h.apply(bt, site_bt, z_bt), h
