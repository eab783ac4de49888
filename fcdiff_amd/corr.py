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
    return t.to(device=ctx.device, dtype=torch.float64).contiguous()


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
        t = ts if isinstance(ts, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(ts, dtype=np.float64), device=ctx.device)
        t = t.to(device=ctx.device, dtype=torch.float64).contiguous()
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
