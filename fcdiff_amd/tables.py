"""
The two small device blocks every fit and query starts from, each written by ONE host function:
  build        the likelihood tables (S_B, lM) of a theta -- the only caller of the table kernels in the package;
  write_hyper  the hyper block {ln gamma, ln(1 - pi), ln pi}.
A new feature that needs tables or a hyper block calls these; a new table variant is a new argument of build().
"""
import numpy as np

from . import _lib

# fcd_lik_sessions.hip's FCD_NOISE_LDS_RECORDS: up to this many per-subject records (max(H, U K)) the noise tables keep them in
# LDS, above it they are read from global memory.  Tests build on both sides of it.
NOISE_LDS_RECORDS = 768
# fcd_subtype.hip's SUBTYPE_MAX: the most subtypes (columns of the responsibilities) the weighted table and the subtype
# log-likelihood are built for
SUBTYPE_MAX = 8


def build(ctx, b_dev, bt_dev, theta, flags, shared=False, S_B=None, lM=None, lpB=None, pBt=None, n_missing=None, noise=None,
          groups=None, weights=None):
    """
    (S_B (C, 3), lM) of b_dev (C, H) and bt_dev (C, U) at theta, in ONE library call on `ctx`:
      shared=False  fcd_lik_tables_ex: lM (C, U, 3, 3) and, where given, the per-item tables lpB (C, H, 3), pBt (C, U, 3);
      shared=True   fcd_lik_shared_tables: lM is L (C, 1, 3, 3), the sum over patients (no per-item tables).
    A 3-D bt_dev (C, U, K) -- K sessions of every patient, the session index fastest -- selects the sessions form of the same
    call (fcd_lik_tables_sessions / fcd_lik_shared_tables_sessions): the same outputs, an item's density taken over its
    sessions in log form.  pBt is refused there (ValueError): a product of densities underflows, and nothing consumes it.
    S_B and lM are written in place where given (a sampler built on them reads the new tables after refresh_tables()) and
    allocated where not.  flags: 0 or _lib.FCD_DATA_NAN_MISSING; with flags = 0 and n_missing = None the unshared call is
    the plain fcd_lik_tables, argument for argument.  n_missing: (2,) int64 device tensor the kernel adds the NaN counts of
    b and bt to (a counting build waits for its atomics), or None.
    noise: None, or (var_b_dev, var_bt_dev): known measurement variances on top of sigma^2, float64 device tensors (H,) and
    (U,) / (U, K) matching bt_dev, either of them None for all zeros.  It selects fcd_lik_tables_noise /
    fcd_lik_shared_tables_noise for a bt of either rank (a 2-D bt is K = 1); pBt is refused (ValueError), as with sessions.
    The values are the caller's to check (finite, >= 0): nothing here reads them.
    groups: None, or (order_dev, offsets_dev, G): known groups of patients, as fit.group_labels_csr() makes them -- order (U,)
    int32 the patients sorted by group, offsets (G + 1,) int64 each group's span in it, both device tensors.  It selects
    fcd_lik_grouped_tables: lM is L (C, G, 3, 3), the sum of lM over each group's patients, for a bt of either rank (a 2-D bt
    is K = 1) and with or without `noise`.  There are no per-item tables (lpB, pBt: ValueError), and shared=True with groups
    is a ValueError (one group is the shared table).  The contents of the two index tensors are the caller's to check on the
    host (group_labels_csr does): nothing here reads them.
    weights: None, or (lM_patients, resp): the per-patient table (C, U, 3, 3) of an earlier unshared build of the same data and
    responsibilities resp (U, G), 1 <= G <= SUBTYPE_MAX, both float64 device tensors.  It selects fcd_lik_weighted_tables: lM
    is L (C, G, 3, 3), L[c, g] = sum_u resp[u, g] lM_patients[c, u], written in place where given -- the table of the
    subtype-region model at its current responsibilities (`groups` is its one-hot case).  The data is not read again (noise,
    sessions and missing data are in lM_patients already) and S_B is returned as given: b_dev, bt_dev and theta only say the
    shape.  shared=True or groups with weights is a ValueError, and so are per-item tables and n_missing.  The values of resp
    are the caller's to check; a weight that is exactly 0 adds nothing, whatever the entry.
    """
    import torch
    if weights is not None:
        return _build_weighted(ctx, b_dev, bt_dev, shared, S_B, lM, lpB, pBt, n_missing, groups, weights)
    (C, H) = (int(b_dev.shape[0]), int(b_dev.shape[1]))
    if bt_dev.dim() not in (2, 3):
        raise ValueError("bt must be (C, U) or (C, U, K), got shape %s" % (tuple(bt_dev.shape),))
    U = int(bt_dev.shape[1])
    K = int(bt_dev.shape[2]) if bt_dev.dim() == 3 else None
    if K is not None and pBt is not None:
        raise ValueError("p_Bt_g_Ft is not made for sessions data: a product of densities underflows")
    if K is not None and K < 1:
        raise ValueError("bt (C, U, K) needs K >= 1 sessions, got shape %s" % (tuple(bt_dev.shape),))
    if groups is not None:
        if shared:
            raise ValueError("groups and shared=True exclude each other: one group of all patients is the shared table")
        if lpB is not None or pBt is not None:
            raise ValueError("the grouped tables have no per-item tables (lp_B_g_F, p_Bt_g_Ft)")
        (order, offsets, G) = groups
        G = int(G)
        if not 1 <= G <= U:
            raise ValueError("groups: G = %d groups, must be 1 .. U = %d" % (G, U))
        if tuple(order.shape) != (U,) or order.dtype != torch.int32:
            raise ValueError("groups: order must be int32 (U,) = %s" % ((U,),))
        if tuple(offsets.shape) != (G + 1,) or offsets.dtype != torch.int64:
            raise ValueError("groups: offsets must be int64 (G + 1,) = %s" % ((G + 1,),))
        if lM is not None and tuple(lM.shape) != (C, G, 3, 3):
            raise ValueError("groups: lM must be (C, G, 3, 3) = %s, got %s" % ((C, G, 3, 3), tuple(lM.shape)))
    if S_B is None:
        S_B = torch.empty((C, 3), dtype=torch.float64, device=bt_dev.device)
    if lM is None:
        lM = torch.empty((C, (1 if shared else U) if groups is None else G, 3, 3), dtype=torch.float64, device=bt_dev.device)
    (th, _th) = _lib.dbl_array(theta)
    if groups is not None:
        Kn = 1 if K is None else K
        (var_b, var_bt) = (None, None) if noise is None else _noise_checked(noise, H, U, K)
        ctx.call("fcd_lik_grouped_tables", _lib.dptr(b_dev), _lib.dptr(bt_dev.contiguous()), C, H, U, Kn, th, _lib.dptr(var_b),
                 _lib.dptr(var_bt), _lib.dptr(order.contiguous()), _lib.dptr(offsets.contiguous()), G, _lib.dptr(S_B),
                 _lib.dptr(lM), int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
    elif noise is not None:
        if pBt is not None:
            raise ValueError("p_Bt_g_Ft is not made with noise variances: the noise tables are log-form only")
        Kn = 1 if K is None else K
        (var_b, var_bt) = _noise_checked(noise, H, U, K)
        bt_dev = bt_dev.contiguous()
        if shared:
            ctx.call("fcd_lik_shared_tables_noise", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, Kn, th, _lib.dptr(var_b),
                     _lib.dptr(var_bt), _lib.dptr(S_B), _lib.dptr(lM), int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
        else:
            ctx.call("fcd_lik_tables_noise", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, Kn, th, _lib.dptr(var_b),
                     _lib.dptr(var_bt), _lib.dptr(S_B), _lib.dptr(lM), _lib.dptr(lpB), int(flags), _lib.dptr(n_missing),
                     _lib.stream_ptr())
    elif K is not None:
        bt_dev = bt_dev.contiguous()
        if shared:
            ctx.call("fcd_lik_shared_tables_sessions", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, K, th, _lib.dptr(S_B),
                     _lib.dptr(lM), int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
        else:
            ctx.call("fcd_lik_tables_sessions", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, K, th, _lib.dptr(S_B),
                     _lib.dptr(lM), _lib.dptr(lpB), int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
    elif shared:
        ctx.call("fcd_lik_shared_tables", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, th, _lib.dptr(S_B), _lib.dptr(lM),
                 int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
    else:
        ctx.call("fcd_lik_tables_ex", _lib.dptr(b_dev), _lib.dptr(bt_dev), C, H, U, th, _lib.dptr(S_B), _lib.dptr(lM),
                 _lib.dptr(lpB), _lib.dptr(pBt), int(flags), _lib.dptr(n_missing), _lib.stream_ptr())
    return S_B, lM


def _build_weighted(ctx, b_dev, bt_dev, shared, S_B, L, lpB, pBt, n_missing, groups, weights):
    """build()'s `weights` form: (S_B as given, L) through fcd_lik_weighted_tables, after its argument checks."""
    import torch
    if shared or groups is not None:
        raise ValueError("weights excludes shared=True and groups: responsibilities of one column are the shared table, "
                         "one-hot ones the grouped table")
    if lpB is not None or pBt is not None or n_missing is not None:
        raise ValueError("the weighted table reads the per-patient table, not the data: no per-item tables (lp_B_g_F, p_Bt_g_Ft) "
                         "and no NaN counts")
    if bt_dev.dim() not in (2, 3):
        raise ValueError("bt must be (C, U) or (C, U, K), got shape %s" % (tuple(bt_dev.shape),))
    (C, U) = (int(b_dev.shape[0]), int(bt_dev.shape[1]))
    if not isinstance(weights, (tuple, list)) or len(weights) != 2:
        raise ValueError("weights must be (lM_patients (C, U, 3, 3), resp (U, G))")
    (lM_u, resp) = weights
    if tuple(lM_u.shape) != (C, U, 3, 3) or lM_u.dtype != torch.float64:
        raise ValueError("weights: the per-patient table must be float64 (C, U, 3, 3) = %s, got %s"
                         % ((C, U, 3, 3), tuple(lM_u.shape)))
    if resp.dim() != 2 or int(resp.shape[0]) != U or resp.dtype != torch.float64:
        raise ValueError("weights: resp must be float64 (U, G) with U = %d, got %s" % (U, tuple(resp.shape)))
    G = int(resp.shape[1])
    if not 1 <= G <= SUBTYPE_MAX:
        raise ValueError("weights: G = %d subtypes, must be 1 .. %d" % (G, SUBTYPE_MAX))
    if L is None:
        L = torch.empty((C, G, 3, 3), dtype=torch.float64, device=lM_u.device)
    elif tuple(L.shape) != (C, G, 3, 3) or L.dtype != torch.float64 or not L.is_contiguous():
        raise ValueError("weights: lM must be a contiguous float64 (C, G, 3, 3) = %s, got %s" % ((C, G, 3, 3), tuple(L.shape)))
    ctx.call("fcd_lik_weighted_tables", _lib.dptr(lM_u.contiguous()), _lib.dptr(resp.contiguous()), C, U, G, _lib.dptr(L),
             _lib.stream_ptr())
    return S_B, L


def _noise_checked(noise, H, U, K):
    """(var_b, var_bt) of build()'s `noise`, contiguous, after its shape and dtype checks (K: None for a 2-D bt)."""
    import torch
    (var_b, var_bt) = noise
    Kn = 1 if K is None else K
    if var_b is not None and (tuple(var_b.shape) != (H,) or var_b.dtype != torch.float64):
        raise ValueError("noise: var_b must be float64 (H,) = %s" % ((H,),))
    if var_bt is not None and (var_bt.dtype != torch.float64 or tuple(var_bt.shape) not in ((U, Kn),) + (((U,),) if K is None else ())):
        raise ValueError("noise: var_bt must be float64 (U, K) = %s" % ((U, Kn),))
    return (None if var_b is None else var_b.contiguous(), None if var_bt is None else var_bt.contiguous())


def write_hyper(ctx, hyper, gamma, pi2):
    """Writes {ln gamma[3], ln pi2[2]} into the (8,) float64 device block `hyper` (fcd_hyper_set); returns it."""
    (g, _g) = _lib.dbl_array(np.asarray(gamma, dtype=np.float64).reshape(3))
    (p, _p) = _lib.dbl_array(np.asarray(pi2, dtype=np.float64).reshape(2))
    ctx.call("fcd_hyper_set", _lib.dptr(hyper), g, p, _lib.stream_ptr())
    return hyper
