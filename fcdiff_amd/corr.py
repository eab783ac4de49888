"""
Front-end named by BASELINE.json's north_star: region x time series -> the edge-major correlation arrays the
fitter takes.  Not part of the reference (fcdiff/fit.py:20-23 starts from correlations); oracle = numpy.corrcoef.

clean() / correlations(confounds=, frame_mask=) put frame censoring and confound regression in front of the
correlation, on the device (fcd_corr_clean, include/fcdiff_hip.h); their oracle is tests/corr_clean_ref.py.

partial_correlations() / correlations(kind="partial") give partial correlations from a shrunk correlation matrix instead
(fcd_corr_partial); oracle tests/partial_corr_ref.py.
"""
import numpy as np

from . import _lib
from . import util

MAX_CONFOUNDS = 64


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _check_clean_shapes(ts, confounds, frame_mask):
    """Host-side checks of the cleaning path: before any context exists and before anything is uploaded."""
    sh = _shape(ts)
    if len(sh) != 3:
        raise ValueError("ts must have shape (S, Nreg, T)")
    (S, Nreg, T) = sh
    Q = 0
    if confounds is not None:
        ch = _shape(confounds)
        if len(ch) != 3:
            raise ValueError("confounds must have shape (S, Q, T)")
        if ch[0] != S or ch[2] != T:
            raise ValueError("confounds has shape %s, ts %s: S and T must agree" % (ch, sh))
        Q = ch[1]
        if Q > MAX_CONFOUNDS:
            raise NotImplementedError("%d confounds per subject, at most %d" % (Q, MAX_CONFOUNDS))
    if frame_mask is not None:
        mh = _shape(frame_mask)
        if len(mh) != 2:
            raise ValueError("frame_mask must have shape (S, T)")
        if mh != (S, T):
            raise ValueError("frame_mask has shape %s, ts %s: S and T must agree" % (mh, sh))
    return (S, Nreg, Q, T)


def _device_f64(x, ctx):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=ctx.device)
    return _aligned16(t.to(device=ctx.device, dtype=torch.float64).contiguous())


def _aligned16(t):
    """t, or a copy of it where t is a view that starts off a 16-byte boundary (a caller's slice of a flat buffer): the
    correlation kernels read the rows of an even-T series 16 bytes at a time and the library refuses such a pointer."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _clean_device(ts, confounds, frame_mask, ctx):
    """(resid, info) as device tensors; the inputs are copied or read, never written."""
    import torch
    (S, Nreg, Q, T) = _check_clean_shapes(ts, confounds, frame_mask)
    t = _device_f64(ts, ctx)
    cf = _device_f64(confounds, ctx) if Q > 0 else None
    fm = None
    if frame_mask is not None:
        if isinstance(frame_mask, torch.Tensor):
            fm = frame_mask.to(device=ctx.device).to(torch.bool)
        else:
            fm = torch.as_tensor(np.ascontiguousarray(np.asarray(frame_mask).astype(bool)), device=ctx.device)
        fm = fm.to(torch.uint8).contiguous()
    resid = torch.empty((S, Nreg, T), dtype=torch.float64, device=ctx.device)
    info = torch.empty((S, 3), dtype=torch.int32, device=ctx.device)
    ctx.call("fcd_corr_clean", _lib.dptr(t), _lib.dptr(cf), _lib.dptr(fm), S, Nreg, Q, T, _lib.dptr(resid), _lib.dptr(info),
             _lib.stream_ptr())
    return (resid, info)


def clean(ts, *, confounds=None, frame_mask=None, ctx=None, as_numpy=True):
    """
    Frame censoring and confound regression of every subject's series, on the device.
    ts : (S, Nreg, T) float64.  confounds : (S, Q, T) float64 nuisance regressors, 0 <= Q <= 64; an intercept is always
    implied.  frame_mask : (S, T), truthy keeps the frame; a dropped frame is never read into any sum (NaN or inf stored
    there, in ts or in confounds, does not reach the result).  Unequal scan lengths: pad to a common T and mask the padding.
    Returns (resid, info):
    resid (S, Nreg, T): the residuals of the subject's kept frames, in order, at positions 0 .. n_kept - 1, exact 0.0 behind
    them.  A row that is constant over the kept frames, holds a non-finite kept value or lies in the span of the confounds
    is all zeros, and so is every row of a subject with dof < 2 or with a non-finite kept value in a confound.
    info (S, 3) int: n_kept, rank (confound columns used after constant and collinear ones are dropped), dof = n_kept - 1 - rank.
    """
    _check_clean_shapes(ts, confounds, frame_mask)
    ctx = ctx if ctx is not None else _lib.Context()
    (resid, info) = _clean_device(ts, confounds, frame_mask, ctx)
    return (resid.cpu().numpy(), info.cpu().numpy()) if as_numpy else (resid, info)


def _check_shrinkage(shrinkage):
    """(mode, value) of the C entry point; raises before any context exists."""
    if isinstance(shrinkage, str):
        if shrinkage != "ledoit_wolf":
            raise ValueError("shrinkage must be 'ledoit_wolf' or a number in [0, 1], not %r" % (shrinkage,))
        return (1, 0.0)
    if isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float, np.integer, np.floating)):
        raise ValueError("shrinkage must be 'ledoit_wolf' or a number in [0, 1], not %r" % (shrinkage,))
    a = float(shrinkage)
    if not (0.0 <= a <= 1.0):
        raise ValueError("shrinkage %r lies outside [0, 1]" % (shrinkage,))
    return (0, a)


def partial_correlations(ts, shrinkage="ledoit_wolf", fisher_z=False, ctx=None, as_numpy=True, *, confounds=None,
                         frame_mask=None, return_info=False, _max_chunk=None):
    """
    Partial correlations of every subject's regions, from a shrunk correlation matrix, on the device (fcd_corr_partial,
    include/fcdiff_hip.h; oracle tests/partial_corr_ref.py).  ts : (S, Nreg, T) float64, 2 <= Nreg <= 1024.
    Returns (C, S) float64 in the layout of correlations().
    Per subject, over its n frames (T, or n_kept after cleaning): R = the correlation matrix of the live regions,
    R_a = (1 - a) R + a I, Theta = R_a^-1, rho_ij = -Theta_ij / sqrt(Theta_ii Theta_jj), clipped to [-1, 1].
    shrinkage : "ledoit_wolf" (Ledoit & Wolf 2004 on the standardised rows, per subject) or a fixed a in [0, 1].
    A region whose edges correlations() gives as NaN (constant, all-zero residual, non-finite) is dead: it leaves the
    problem and its edges are NaN.  A subject with fewer than two live regions is all NaN (status 2); so is one whose R_a is
    numerically singular (a pivot <= 1e-12: a = 0 with n - 1 < p, or duplicate rows; status 1) -- nothing is regularised
    behind the caller's back.  NaN edges are meant for a fit with `missing_data = True`.
    fisher_z applies atanh.  confounds, frame_mask: as correlations(); the partial correlations are those of clean()'s
    residuals over the kept frames.
    return_info=True returns (out, info): info = {"alpha": (S,) the a used, "n_live": (S,), "status": (S,), "clean": the
    (S, 3) array of clean() or None}.
    Partial correlations are smaller in magnitude than correlations: the model's mu and sigma defaults do not fit them.
    """
    import torch
    (mode, value) = _check_shrinkage(shrinkage)
    cleaning = confounds is not None or frame_mask is not None
    if cleaning:
        _check_clean_shapes(ts, confounds, frame_mask)
    elif len(_shape(ts)) != 3:
        raise ValueError("ts must have shape (S, Nreg, T)")
    ctx = ctx if ctx is not None else _lib.Context()
    (cinfo, nfr) = (None, None)
    if cleaning:
        (t, cinfo) = _clean_device(ts, confounds, frame_mask, ctx)
        nfr = cinfo[:, 0].contiguous()
    else:
        t = _device_f64(ts, ctx)
    (S, Nreg, T) = (int(t.shape[0]), int(t.shape[1]), int(t.shape[2]))
    out = torch.empty((util.N_to_C(Nreg), S), dtype=torch.float64, device=ctx.device)
    alpha = torch.empty((S,), dtype=torch.float64, device=ctx.device)
    pinfo = torch.empty((S, 2), dtype=torch.int32, device=ctx.device)
    if _max_chunk is not None:
        ctx.set_knob("partial_chunk", int(_max_chunk))
    try:
        ctx.call("fcd_corr_partial", _lib.dptr(t), S, Nreg, T, _lib.dptr(nfr), mode, value, 1 if fisher_z else 0, _lib.dptr(out),
                 _lib.dptr(alpha), _lib.dptr(pinfo), _lib.stream_ptr())
    finally:
        if _max_chunk is not None:
            ctx.set_knob("partial_chunk", 0)
    info = {"alpha": alpha, "n_live": pinfo[:, 0], "status": pinfo[:, 1], "clean": cinfo}
    if as_numpy:
        out = out.cpu().numpy()
        info = {k: (v.cpu().numpy() if v is not None else None) for (k, v) in info.items()}
    return (out, info) if return_info else out


def correlations(ts, fisher_z=False, ctx=None, as_numpy=True, *, confounds=None, frame_mask=None, return_info=False,
                 kind="correlation"):
    """
    ts : (S, Nreg, T) float64 time series of S subjects.
    Returns (C, S) float64, row c = n(n-1)/2 + m (n > m, util.c_to_nm order), column = subject:
    `b = out[:, healthy]`, `bt = out[:, patients]` can go straight into UnsharedRegionFit.  The edges of a constant series
    are NaN, as numpy.corrcoef gives them: they are meant to go into a fit with `missing_data = True`, which integrates
    them out.
    fisher_z applies atanh (default off: the model's defaults are on raw correlations, model.py:213, 236).
    confounds (S, Q, T), frame_mask (S, T): the correlations are those of the residuals clean() gives, over the kept frames
    (see clean); a region or subject with nothing left has NaN edges.  return_info=True returns (out, info).
    kind="partial" is partial_correlations(..., shrinkage="ledoit_wolf") with the same arguments (its info is a dict).
    """
    if kind == "partial":
        return partial_correlations(ts, "ledoit_wolf", fisher_z, ctx, as_numpy, confounds=confounds, frame_mask=frame_mask,
                                    return_info=return_info)
    if kind != "correlation":
        raise ValueError("kind must be 'correlation' or 'partial', not %r" % (kind,))
    import torch
    cleaning = confounds is not None or frame_mask is not None or return_info
    if cleaning:
        _check_clean_shapes(ts, confounds, frame_mask)
    ctx = ctx if ctx is not None else _lib.Context()
    info = None
    if cleaning:
        (t, info) = _clean_device(ts, confounds, frame_mask, ctx)
    else:
        t = _device_f64(ts, ctx)
    if t.dim() != 3:
        raise ValueError("ts must have shape (S, Nreg, T)")
    (S, Nreg, T) = (int(t.shape[0]), int(t.shape[1]), int(t.shape[2]))
    out = torch.empty((util.N_to_C(Nreg), S), dtype=torch.float64, device=ctx.device)
    ctx.call("fcd_corr_edges", _lib.dptr(t), S, Nreg, T, 1 if fisher_z else 0, _lib.dptr(out), _lib.stream_ptr())
    if as_numpy:
        (out, info) = (out.cpu().numpy(), info.cpu().numpy() if info is not None else None)
    return (out, info) if cleaning and return_info else out


def sampling_variance(info, fisher_z=False, n_conditioned=0):
    """
    Per-subject sampling variance of a correlation, from the `info` (S, 3) that clean() / correlations(..., return_info=True)
    give (column 2: the residual degrees of freedom dof = n_kept - 1 - rank): what goes into a fit's `b_noise_var` /
    `bt_noise_var` for the subjects' columns.
      fisher_z=True   1 / (dof - 2): the variance of atanh(r), to first order free of rho (1 / (n - 3) without confounds);
      fisher_z=False  1 / dof: the rho = 0 value of var(r) = (1 - rho^2)^2 / dof, its largest, so an UPPER bound for every
                      edge of the subject (a strongly correlated edge is measured better than this says).
    Returns (S,) float64; `inf` where the denominator is <= 0 -- such a subject carries no information: drop it, or give its
    column as NaN under missing_data (a fit refuses an infinite variance).
    Frames of a scan are not independent: temporal autocorrelation lowers the effective degrees of freedom below dof, so
    these variances are lower bounds on the real ones; a user who knows the effective dof of their acquisition passes
    their own variances instead.
    n_conditioned (a number, or (S,)) is subtracted from dof: a partial correlation conditions on the other p - 2 live regions,
    so pass p - 2 for an UNSHRUNK one (partial_correlations(..., shrinkage=0.0)) -- the classical 1 / (dof - (p - 2) - 2) under
    Fisher z.  With shrinkage a > 0 the estimate is biased towards 0 and has less variance than this; the value is then only a
    guide.  The default 0 is the plain correlation's variance.
    """
    info = np.asarray(info)
    if info.ndim != 2 or info.shape[1] != 3:
        raise ValueError("info must have shape (S, 3): n_kept, rank, dof per subject")
    nc = np.asarray(n_conditioned, dtype=np.float64)
    if nc.ndim > 1 or (nc.ndim == 1 and nc.shape[0] != info.shape[0]) or not np.all(nc >= 0):
        raise ValueError("n_conditioned must be a non-negative number or one per subject")
    den = info[:, 2].astype(np.float64) - nc - (2.0 if fisher_z else 0.0)
    out = np.full(den.shape, np.inf)
    np.divide(1.0, den, out=out, where=den > 0)
    return out


# ---- tangent-space connectivity fitted on the controls (fcd_tangent_fit, fcd_tangent_apply, fcd_sym_eigh) -------------------
MAX_TANGENT_REGIONS = 1024
TANGENT_STATUS = {0: "ok", 1: "numerically singular", 2: "fewer than two live regions", 3: "n_frames outside [0, T]",
                  4: "a dead region: drop it for everyone", 5: "the eigensolver gave up (a non-finite matrix, or no convergence)"}


def _check_tangent_ts(ts, confounds, frame_mask):
    """(S, Nreg, T) of a tangent call; raises before any context exists."""
    if confounds is not None or frame_mask is not None:
        (S, Nreg, _Q, T) = _check_clean_shapes(ts, confounds, frame_mask)
    else:
        sh = _shape(ts)
        if len(sh) != 3:
            raise ValueError("ts must have shape (S, Nreg, T)")
        (S, Nreg, T) = sh
    if S < 1 or Nreg < 2 or T < 2:
        raise ValueError("need S >= 1, Nreg >= 2, T >= 2 (ts has shape %s)" % ((S, Nreg, T),))
    if Nreg > MAX_TANGENT_REGIONS:
        raise NotImplementedError("%d regions, at most %d" % (Nreg, MAX_TANGENT_REGIONS))
    return (S, Nreg, T)


def _tangent_series(ts, confounds, frame_mask, ctx):
    """(series on the device, n_frames or None, clean info or None)"""
    if confounds is not None or frame_mask is not None:
        (t, cinfo) = _clean_device(ts, confounds, frame_mask, ctx)
        return (t, cinfo[:, 0].contiguous(), cinfo)
    return (_device_f64(ts, ctx), None, None)


def _check_tangent_fit(ts, shrinkage, reference, tol, max_iter, confounds, frame_mask):
    """(mode, value, H, Nreg, T) of a fit; raises before any context exists."""
    (mode, value) = _check_shrinkage(shrinkage)
    if reference not in ("geometric", "euclidean"):
        raise ValueError("reference must be 'geometric' or 'euclidean', not %r" % (reference,))
    if not (isinstance(tol, (int, float, np.integer, np.floating)) and tol > 0):
        raise ValueError("tol must be a number > 0, not %r" % (tol,))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError("max_iter must be an integer >= 1, not %r" % (max_iter,))
    (H, Nreg, T) = _check_tangent_ts(ts, confounds, frame_mask)
    if H < 2:
        raise ValueError("%d controls, at least 2 are needed" % H)
    return (mode, value, H, Nreg, T)


def sym_eigh(A, ctx=None, as_numpy=True, _max_chunk=None):
    """
    Eigendecomposition of a batch of symmetric matrices on the device (fcd_sym_eigh, include/fcdiff_hip.h): parallel cyclic
    Jacobi, one workgroup per matrix.  A : (B, n, n) or (n, n) float64, n <= 1024, not necessarily definite; only the lower
    triangle is read.  Returns (w, V, status): w (B, n) ascending, V (B, n, n) with the eigenvectors in columns, status (B,)
    int -- 0 ok, 1 a non-finite entry, 2 not converged in 40 sweeps; w and V are NaN where status is not 0.
    """
    import torch
    sh = _shape(A)
    if len(sh) == 2:
        sh = (1,) + sh
    if len(sh) != 3 or sh[1] != sh[2] or sh[0] < 1 or sh[1] < 1:
        raise ValueError("A must have shape (B, n, n) or (n, n), not %s" % (_shape(A),))
    if sh[1] > 1024:
        raise NotImplementedError("n = %d, at most 1024" % sh[1])
    ctx = ctx if ctx is not None else _lib.Context()
    a = _device_f64(A, ctx).reshape(sh)
    (B, n) = (sh[0], sh[1])
    w = torch.empty((B, n), dtype=torch.float64, device=ctx.device)
    V = torch.empty((B, n, n), dtype=torch.float64, device=ctx.device)
    status = torch.empty((B,), dtype=torch.int32, device=ctx.device)
    d = _lib.EighDesc.make(B=B, n=n, stream=_lib.stream_ptr(), A=_lib.dptr(a), w=_lib.dptr(w), V=_lib.dptr(V), status=_lib.dptr(status))
    import ctypes
    if _max_chunk is not None:
        ctx.set_knob("tangent_chunk", int(_max_chunk))
    try:
        ctx.call("fcd_sym_eigh", ctypes.byref(d))
    finally:
        if _max_chunk is not None:
            ctx.set_knob("tangent_chunk", 0)
    if len(_shape(A)) == 2:
        (w, V, status) = (w[0], V[0], status[0])
    return (w.cpu().numpy(), V.cpu().numpy(), status.cpu().numpy()) if as_numpy else (w, V, status)


class TangentSpace(object):
    """
    A reference connectivity and the map into its tangent space.  .reference G (Nreg, Nreg), .whitening W = G^-1/2, .shrinkage,
    .info (dict of the fit: "used", "alpha", "n_live", "status", "n_iter", "grad_norm", "reference_kind", "clean"; empty for
    from_reference), all NumPy.  Made by fit_tangent() or TangentSpace.from_reference().
    """

    def __init__(self, reference, whitening, shrinkage, info, reference_sqrt=None):
        (self.reference, self.whitening, self.shrinkage, self.info) = (reference, whitening, shrinkage, info)
        self.reference_sqrt = reference_sqrt

    @classmethod
    def from_reference(cls, G, shrinkage="ledoit_wolf"):
        """The space of a given symmetric positive definite G (a reference fitted elsewhere): W = G^-1/2 by numpy.linalg.eigh
        on the host.  Refuses a G that is not square, not finite, not symmetric to 1e-12 or has an eigenvalue <= 1e-12 of the
        largest."""
        _check_shrinkage(shrinkage)
        G = np.array(G, dtype=np.float64)
        if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 2:
            raise ValueError("G must be a square matrix of at least 2 regions, not %s" % (G.shape,))
        if G.shape[0] > MAX_TANGENT_REGIONS:
            raise NotImplementedError("%d regions, at most %d" % (G.shape[0], MAX_TANGENT_REGIONS))
        if not np.isfinite(G).all():
            raise ValueError("G holds a non-finite value")
        if np.abs(G - G.T).max() > 1e-12 * np.abs(G).max():
            raise ValueError("G is not symmetric")
        G = (G + G.T) / 2
        (w, V) = np.linalg.eigh(G)
        if not w[0] > 1e-12 * w[-1]:
            raise ValueError("G is not positive definite (smallest eigenvalue %g, largest %g)" % (w[0], w[-1]))
        W = (V / np.sqrt(w)).dot(V.T)
        Gh = (V * np.sqrt(w)).dot(V.T)
        return cls(G, (W + W.T) / 2, shrinkage, {}, (Gh + Gh.T) / 2)

    def apply(self, ts, *, confounds=None, frame_mask=None, as_numpy=True, return_info=False, ctx=None, _max_chunk=None):
        """
        T_s = logm(W R_a,s W) of every subject of ts (S, Nreg, T): (C, S) float64 off-diagonal entries in the layout of
        correlations(), unscaled.  Controls, patients, now or later: the same map.  confounds, frame_mask: as correlations().
        return_info=True returns (out, info): info = {"diag": (Nreg, S) the diagonal of T_s, "alpha", "n_live", "status" (S,)
        (TANGENT_STATUS), "clean"}.  A subject whose status is not 0 is all NaN.  Never synchronises the stream.
        """
        import ctypes
        import torch
        (mode, value) = _check_shrinkage(self.shrinkage)
        (S, Nreg, T) = _check_tangent_ts(ts, confounds, frame_mask)
        W = np.ascontiguousarray(self.whitening, dtype=np.float64)
        if W.shape != (Nreg, Nreg):
            raise ValueError("ts has %d regions, the reference %d" % (Nreg, W.shape[0]))
        if not np.isfinite(W).all():
            raise ValueError("the whitening matrix holds a non-finite value")
        ctx = ctx if ctx is not None else _lib.Context()
        (t, nfr, cinfo) = _tangent_series(ts, confounds, frame_mask, ctx)
        Wd = _device_f64(W, ctx)
        out = torch.empty((util.N_to_C(Nreg), S), dtype=torch.float64, device=ctx.device)
        diag = torch.empty((Nreg, S), dtype=torch.float64, device=ctx.device)
        alpha = torch.empty((S,), dtype=torch.float64, device=ctx.device)
        pinfo = torch.empty((S, 2), dtype=torch.int32, device=ctx.device)
        d = _lib.TangentDesc.make(S=S, Nreg=Nreg, T=T, shrink_mode=mode, shrink_value=value, stream=_lib.stream_ptr(), ts=_lib.dptr(t),
                                  n_frames=_lib.dptr(nfr), alpha=_lib.dptr(alpha), info=_lib.dptr(pinfo), W=_lib.dptr(Wd),
                                  out=_lib.dptr(out), diag=_lib.dptr(diag))
        if _max_chunk is not None:
            ctx.set_knob("tangent_chunk", int(_max_chunk))
        try:
            ctx.call("fcd_tangent_apply", ctypes.byref(d))
        finally:
            if _max_chunk is not None:
                ctx.set_knob("tangent_chunk", 0)
        info = {"diag": diag, "alpha": alpha, "n_live": pinfo[:, 0], "status": pinfo[:, 1], "clean": cinfo}
        if as_numpy:
            out = out.cpu().numpy()
            info = {k: (v.cpu().numpy() if v is not None else None) for (k, v) in info.items()}
        return (out, info) if return_info else out


def fit_tangent(ts_controls, shrinkage="ledoit_wolf", reference="geometric", *, confounds=None, frame_mask=None, tol=1e-10,
                max_iter=50, ctx=None, _max_chunk=None):
    """
    Fit the tangent space of the controls on the device (fcd_tangent_fit, include/fcdiff_hip.h; oracle tests/tangent_ref.py;
    Varoquaux et al. 2010).  ts_controls : (H, Nreg, T) float64, 2 <= Nreg <= 1024.  Returns a TangentSpace.
    Per control R_a = (1 - a) R + a I with the a and the live / dead rule of partial_correlations(); a control with a dead
    region (status 4), with fewer than two live regions (2) or whose R_a has lambda_min <= 1e-12 lambda_max (1) is left out
    and reported in info["used"]; fewer than two usable controls is a ValueError.
    reference="euclidean": G = the mean of the used R_a.  "geometric" (default): the Frechet mean of the affine-invariant
    metric by the fixed point  W = G^-1/2, Tbar = mean logm(W R_a W), G <- G^1/2 expm(Tbar) G^1/2  from the Euclidean mean,
    until ||Tbar||_F <= tol sqrt(Nreg); max_iter evaluations without that raise RuntimeError with the last norm.
    info["n_iter"], info["grad_norm"]: the evaluations of Tbar and the last norm.
    """
    import ctypes
    import torch
    (mode, value, H, Nreg, T) = _check_tangent_fit(ts_controls, shrinkage, reference, tol, max_iter, confounds, frame_mask)
    ctx = ctx if ctx is not None else _lib.Context()
    (t, nfr, cinfo) = _tangent_series(ts_controls, confounds, frame_mask, ctx)
    mats = [torch.empty((Nreg, Nreg), dtype=torch.float64, device=ctx.device) for _ in range(3)]
    alpha = torch.empty((H,), dtype=torch.float64, device=ctx.device)
    pinfo = torch.empty((H, 2), dtype=torch.int32, device=ctx.device)
    used = torch.empty((H,), dtype=torch.uint8, device=ctx.device)
    (n_iter, grad) = (ctypes.c_int32(0), ctypes.c_double(float("nan")))
    d = _lib.TangentDesc.make(flags=_lib.FCD_TANGENT_EUCLIDEAN if reference == "euclidean" else 0, S=H, Nreg=Nreg, T=T, shrink_mode=mode,
                              shrink_value=value, max_iter=int(max_iter), tol=float(tol), stream=_lib.stream_ptr(), ts=_lib.dptr(t),
                              n_frames=_lib.dptr(nfr), alpha=_lib.dptr(alpha), info=_lib.dptr(pinfo), G=_lib.dptr(mats[0]),
                              G_half=_lib.dptr(mats[1]), W=_lib.dptr(mats[2]), used=_lib.dptr(used),
                              n_iter=ctypes.cast(ctypes.pointer(n_iter), ctypes.c_void_p),
                              grad_norm=ctypes.cast(ctypes.pointer(grad), ctypes.c_void_p))
    if _max_chunk is not None:
        ctx.set_knob("tangent_chunk", int(_max_chunk))
    try:
        ctx.call("fcd_tangent_fit", ctypes.byref(d))
    finally:
        if _max_chunk is not None:
            ctx.set_knob("tangent_chunk", 0)
    if n_iter.value < 0:
        raise RuntimeError("fit_tangent: not converged after %d iterations: ||mean tangent vector||_F = %g, wanted <= %g"
                           % (-n_iter.value, grad.value, tol * np.sqrt(Nreg)))
    info = {"used": used.cpu().numpy().astype(bool), "alpha": alpha.cpu().numpy(), "n_live": pinfo[:, 0].cpu().numpy(),
            "status": pinfo[:, 1].cpu().numpy(), "n_iter": int(n_iter.value), "grad_norm": float(grad.value),
            "reference_kind": reference, "clean": cinfo.cpu().numpy() if cinfo is not None else None}
    return TangentSpace(mats[0].cpu().numpy(), mats[2].cpu().numpy(), shrinkage, info, mats[1].cpu().numpy())


def tangent(ts_controls, ts_patients, shrinkage="ledoit_wolf", reference="geometric", *, tol=1e-10, max_iter=50, ctx=None,
            as_numpy=True):
    """
    fit_tangent() on the controls, then the embedding of both groups: returns (b, bt, space), b (C, H) and bt (C, U) in the layout
    of correlations(), for UnsharedRegionFit and its siblings.  A control that the fit left out is a NaN column of b (a fit with
    `missing_data = True` integrates it out).  Tangent values are deviations from the controls' reference, centred near 0: the
    model's mu and sigma defaults do not fit them; set them from b, or fit them.
    """
    (_mode, _value, _H, Nreg, _T) = _check_tangent_fit(ts_controls, shrinkage, reference, tol, max_iter, None, None)
    if _check_tangent_ts(ts_patients, None, None)[1] != Nreg:
        raise ValueError("ts_controls has %d regions, ts_patients %d" % (Nreg, _shape(ts_patients)[1]))
    ctx = ctx if ctx is not None else _lib.Context()
    space = fit_tangent(ts_controls, shrinkage, reference, tol=tol, max_iter=max_iter, ctx=ctx)
    b = space.apply(ts_controls, as_numpy=as_numpy, ctx=ctx)
    bt = space.apply(ts_patients, as_numpy=as_numpy, ctx=ctx)
    return (b, bt, space)
