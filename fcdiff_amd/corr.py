"""
Front-end named by BASELINE.json's north_star: region x time series -> the edge-major correlation arrays the
fitter takes.  Not part of the reference (fcdiff/fit.py:20-23 starts from correlations); oracle = numpy.corrcoef.

clean() / correlations(confounds=, frame_mask=) put frame censoring and confound regression in front of the
correlation, on the device (fcd_corr_clean, include/fcdiff_hip.h); their oracle is tests/corr_clean_ref.py.
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


def correlations(ts, fisher_z=False, ctx=None, as_numpy=True, *, confounds=None, frame_mask=None, return_info=False):
    """
    ts : (S, Nreg, T) float64 time series of S subjects.
    Returns (C, S) float64, row c = n(n-1)/2 + m (n > m, util.c_to_nm order), column = subject:
    `b = out[:, healthy]`, `bt = out[:, patients]` can go straight into UnsharedRegionFit.  The edges of a constant series
    are NaN, as numpy.corrcoef gives them: they are meant to go into a fit with `missing_data = True`, which integrates
    them out.
    fisher_z applies atanh (default off: the model's defaults are on raw correlations, model.py:213, 236).
    confounds (S, Q, T), frame_mask (S, T): the correlations are those of the residuals clean() gives, over the kept frames
    (see clean); a region or subject with nothing left has NaN edges.  return_info=True returns (out, info).
    """
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


def sampling_variance(info, fisher_z=False):
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
    """
    info = np.asarray(info)
    if info.ndim != 2 or info.shape[1] != 3:
        raise ValueError("info must have shape (S, 3): n_kept, rank, dof per subject")
    den = info[:, 2].astype(np.float64) - (2.0 if fisher_z else 0.0)
    out = np.full(den.shape, np.inf)
    np.divide(1.0, den, out=out, where=den > 0)
    return out
