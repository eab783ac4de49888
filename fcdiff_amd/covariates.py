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
