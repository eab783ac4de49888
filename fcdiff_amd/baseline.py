"""
Classical baselines to hold the model-based results against.  Not part of the reference; oracle = tests/baseline_ref.py.

normative()   per patient: "which regions of this patient are abnormal?" -- the z-score of every patient connection against
              the controls, summarised per region, with a null made by treating each control in turn as the patient
              (leave-one-out).  What UnsharedRegionFit answers with a posterior.
group_test()  per population: "which regions are abnormal in this disease?" -- Student's two-sample t per connection, the
              sum of t^2 per region, family-wise error control by the permutation law of the maximum statistic.  What
              SharedRegionFit answers with a posterior.
network_test()  per population: "which sub-network is abnormal in this disease?" -- the network-based statistic: the t of
              group_test() thresholded, the connected components of the suprathreshold graph, family-wise error control by
              the permutation law of the largest component.  graph_components() gives the components of any mask.
              Oracle = tests/network_ref.py; fcd_baseline_network_bits, fcd_graph_components.
              statistic="intensity" sizes a component by the sum of |t| - threshold over its connections instead of their
              number, graph_components(mask, weights) by any weights.  Oracle = tests/network_intensity_ref.py;
              fcd_baseline_network_excess, fcd_graph_components_weighted.

group_test() and network_test() take missing_data=True (a NaN is an unobserved value) and variance="welch"; a call with
either goes through fcd_baseline_group_perm_opt / fcd_baseline_network_bits_opt, the default call through the entry points
it always used.  Oracle = tests/baseline_missing_ref.py.

group_test() and network_test() take nuisance covariates z_b (H, Q), z_bt (U, Q) (the covariates module's names and shapes):
the permutation GLM of Freedman & Lane, whole permutations of the subjects in place of labellings, through
fcd_baseline_group_glm / fcd_baseline_network_bits_glm.  glm_design() makes the design on the host, draw_permutations() the
permutations.  Oracle = tests/baseline_glm_ref.py.

b (C, H) controls and bt (C, U) patients, NumPy arrays or torch tensors, float64, connections in util.c_to_nm order;
E(n) = the N - 1 connections that touch region n.  Both run on the device (fcd_baseline_normative,
fcd_baseline_group_perm of include/fcdiff_hip.h) and have no CPU fallback; the p-values are made on the host from what the
device returns, with the conventions >= and (1 + count) / (1 + number of valid null values).
"""
import numpy as np

from . import _lib

MAX_CONTROLS = 1024       # normative(): a control row lives in one wave's LDS
MAX_SUBJECTS = 1024       # group_test(): the labels of a permutation are 8 words per lane
_U_CHUNK = 1 << 16        # patients per call of normative()


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _has_nan(x):
    if hasattr(x, "detach"):
        import torch
        return bool(torch.isnan(x).any().item())
    return bool(np.isnan(np.asarray(x, dtype=np.float64)).any())


def _has_inf(x):
    if hasattr(x, "detach"):
        import torch
        return bool(torch.isinf(x).any().item())
    return bool(np.isinf(np.asarray(x, dtype=np.float64)).any())


def _refuse_nonfinite(b, bt, who, tail):
    """ValueError for a NaN or an infinite value in b or bt."""
    if _has_nan(b) or _has_nan(bt) or _has_inf(b) or _has_inf(bt):
        raise ValueError("%s: NaN or infinite value in b or bt; %s" % (who, tail))


def _n_regions(C):
    N = int(round((np.sqrt(8.0 * C + 1.0) - 1.0) / 2.0)) + 1
    if C < 1 or N * (N - 1) // 2 != C:
        raise ValueError("%d connections: not a triangular number N (N - 1) / 2" % C)
    return N


def _check_pair(b, bt, who):
    """Shapes of (b, bt) -> (C, N, H, U); sessions and a non-triangular C are refused."""
    (sb, st) = (_shape(b), _shape(bt))
    if len(st) == 3:
        raise NotImplementedError("%s: bt of shape (C, U, K): sessions are not provided here" % who)
    if len(sb) != 2 or len(st) != 2:
        raise ValueError("%s: b must have shape (C, H) and bt (C, U)" % who)
    if sb[0] != st[0]:
        raise ValueError("%s: b has %d connections, bt %d" % (who, sb[0], st[0]))
    if sb[1] < 1 or st[1] < 1:
        raise ValueError("%s: at least one control and one patient" % who)
    return sb[0], _n_regions(sb[0]), sb[1], st[1]


def _device_f64(x, ctx):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=ctx.device)
    return t.to(device=ctx.device, dtype=torch.float64).contiguous()


def _count_ge(null, values):
    """#{valid null >= value} per value, and the number of valid (not NaN) null values."""
    srt = np.sort(null[~np.isnan(null)])
    return srt.shape[0] - np.searchsorted(srt, values, side="left"), srt.shape[0]


def _p_against(null, values):
    """(1 + #{valid null >= value}) / (1 + #valid null), NaN where the value is NaN.  null (M,) against values of any shape."""
    (ge, n_valid) = _count_ge(null, values)
    return np.where(np.isnan(values), np.nan, (1.0 + ge) / (1.0 + n_valid))


def normative_pvalues(msq, msq0):
    """
    The host half of normative(): (max0, p_region, p_fwe) from msq (N, U) and the leave-one-out msq0 (N, H).
    max0[h] = max over n of msq0[n,h], ignoring NaN (NaN if a control has no defined region).
    """
    with np.errstate(invalid="ignore"):
        max0 = np.where(np.isnan(msq0).all(axis=0), np.nan, np.fmax.reduce(msq0, axis=0))
    p_region = np.stack([_p_against(msq0[n], msq[n]) for n in range(msq.shape[0])])
    p_fwe = _p_against(max0, msq)
    return max0, p_region, p_fwe


def normative(b, bt, *, missing_data=False, z_threshold=3.0, return_z=False, ctx=None, as_numpy=True):
    """
    Normative z-scores of the patients against the controls, per region.  b (C, H), bt (C, U).

    Per connection c over the controls observed there: n_c, mean m_c, s_c^2 = sum (x - m_c)^2 / (n_c - 1).
        z[c,u]  = (bt[c,u] - m_c) / (s_c sqrt(1 + 1/n_c))
        z0[c,h] = (b[c,h] - m_-h) / (s_-h sqrt(1 + 1/(n_c - 1)))     mean and deviation of the OTHER observed controls,
                                                                    their sums taken directly, never by downdating
    A score is NaN where n_c < 3, where the deviation is not > 0, or where the value itself is unobserved.
    Per region n and subject: n_edges = defined scores over E(n), msq = mean of z^2 over them (NaN if none), n_over = those
    with |z| > z_threshold.  p_region[n,u] is taken against the controls' msq0[n,:], p_fwe[n,u] against max0[h] = max_n
    msq0[n,h].

    The leave-one-out null has one degree of freedom fewer than the patient score (n_c - 1 controls stand behind a z0, n_c
    behind a z): its tails are a little heavier than the patients' own null, so the p-values err on the conservative side.

    Returns a dict: msq, n_edges, n_over (N, U); msq0, n_edges0, n_over0 (N, H); max0 (H,); p_region, p_fwe (N, U);
    n_controls (C,); with return_z also z (C, U) and z0 (C, H).  NumPy arrays, or device tensors with as_numpy=False.
    missing_data=False: a NaN or an infinite value anywhere is a ValueError; with it a NaN is unobserved and an infinite
    value is still refused.  At most 1024 controls
    (NotImplementedError above); any number of patients, walked in chunks.  Sessions (C, U, K) are not provided.
    """
    import torch
    (C, N, H, U) = _check_pair(b, bt, "normative")
    if H > MAX_CONTROLS:
        raise NotImplementedError("normative: %d controls, at most %d" % (H, MAX_CONTROLS))
    if not missing_data:
        _refuse_nonfinite(b, bt, "normative", "pass missing_data=True to treat NaN as unobserved")
    elif _has_inf(b) or _has_inf(bt):
        raise ValueError("normative: infinite value in b or bt; missing_data=True admits NaN (unobserved) only")
    ctx = ctx if ctx is not None else _lib.Context()
    (bd, btd) = (_device_f64(b, ctx), _device_f64(bt, ctx))
    dev = ctx.device

    def f64(*sh):
        return torch.empty(sh, dtype=torch.float64, device=dev)

    def i32(*sh):
        return torch.empty(sh, dtype=torch.int32, device=dev)

    (msq0, ne0, no0, n_controls) = (f64(N, H), i32(N, H), i32(N, H), i32(C))
    (msq, ne, no) = (f64(N, U), i32(N, U), i32(N, U))
    z0 = f64(C, H) if return_z else None
    z = f64(C, U) if return_z else None
    for u0 in range(0, U, _U_CHUNK):
        nu = min(_U_CHUNK, U - u0)
        whole = nu == U
        bt_c = btd if whole else btd[:, u0:u0 + nu].contiguous()
        (m_c, e_c, o_c) = (msq, ne, no) if whole else (f64(N, nu), i32(N, nu), i32(N, nu))
        z_c = z if (whole or z is None) else f64(C, nu)
        ctx.call("fcd_baseline_normative", _lib.dptr(bd), _lib.dptr(bt_c), C, H, nu, float(z_threshold), _lib.dptr(msq0),
                 _lib.dptr(ne0), _lib.dptr(no0), _lib.dptr(m_c), _lib.dptr(e_c), _lib.dptr(o_c), _lib.dptr(n_controls),
                 _lib.dptr(z0), _lib.dptr(z_c), _lib.stream_ptr())
        if not whole:
            msq[:, u0:u0 + nu] = m_c
            ne[:, u0:u0 + nu] = e_c
            no[:, u0:u0 + nu] = o_c
            if z is not None:
                z[:, u0:u0 + nu] = z_c
    out = {"msq": msq, "n_edges": ne.long(), "n_over": no.long(), "msq0": msq0, "n_edges0": ne0.long(), "n_over0": no0.long(),
           "n_controls": n_controls.long()}
    if return_z:
        out["z"] = z
        out["z0"] = z0
    (max0, p_region, p_fwe) = normative_pvalues(msq.cpu().numpy(), msq0.cpu().numpy())
    if as_numpy:
        out = dict((k, v.cpu().numpy()) for (k, v) in out.items())
        out.update(max0=max0, p_region=p_region, p_fwe=p_fwe)
    else:
        out.update(max0=torch.as_tensor(max0, device=dev), p_region=torch.as_tensor(p_region, device=dev),
                   p_fwe=torch.as_tensor(p_fwe, device=dev))
    return out


def draw_labels(n_perm, H, U, seed=0):
    """(n_perm, H + U) uint8 rows with exactly U ones: numpy.random.default_rng(seed), rng.permutation(H + U)[:U] per row."""
    rng = np.random.default_rng(seed)
    S = H + U
    labels = np.zeros((int(n_perm), S), dtype=np.uint8)
    for p in range(int(n_perm)):
        labels[p, rng.permutation(S)[:U]] = 1
    return labels


def _check_labels(labels, S, U):
    lab = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
    if lab.ndim != 2 or lab.shape[1] != S or lab.shape[0] < 1:
        raise ValueError("group_test: labels must have shape (P, %d) with P >= 1, not %s" % (S, lab.shape))
    if not np.isin(lab, (0, 1)).all():
        raise ValueError("group_test: labels must hold 0 and 1 only")
    lab = np.ascontiguousarray(lab.astype(np.uint8))
    if not (lab.sum(axis=1, dtype=np.int64) == U).all():
        raise ValueError("group_test: every row of labels must hold exactly U = %d ones" % U)
    return lab


FLAG_MISSING = 1          # FCD_BASELINE_MISSING, FCD_BASELINE_WELCH of include/fcdiff_hip.h
FLAG_WELCH = 2


def _options(who, b, bt, H, U, missing_data, variance):
    """The host checks of missing_data and variance -> flags of the calls with options (0: the default call)."""
    if variance not in ("pooled", "welch"):
        raise ValueError("%s: variance must be 'pooled' or 'welch', not %r" % (who, variance))
    if variance == "welch" and (H < 2 or U < 2):
        raise ValueError("%s: variance='welch' needs two controls and two patients, not H = %d and U = %d" % (who, H, U))
    if not missing_data:
        _refuse_nonfinite(b, bt, who, "the data must be complete and finite (pass missing_data=True to treat NaN as unobserved)")
    elif _has_inf(b) or _has_inf(bt):
        raise ValueError("%s: infinite value in b or bt; missing_data=True admits NaN (unobserved) only" % who)
    return (FLAG_MISSING if missing_data else 0) | (FLAG_WELCH if variance == "welch" else 0)


# ---- nuisance covariates: the permutation GLM ----------------------------------------------------------------------------------

GLM_MAX_COLUMNS = 8       # covariate columns kept: the design has at most 9 columns (fcd_baseline_group_glm)
GLM_DROP_TOL = 1e-10      # covariates.fit_adjustment's rule: remaining squared norm of a unit column below this -> dropped
GLM_CONTRAST_TOL = 1e-10  # ||x_r||^2 must be > this multiple of ||x_c||^2: the group is not a function of the covariates


def draw_permutations(n_perm, S, seed=0):
    """(n_perm, S) int64 rows, each a permutation of 0 .. S - 1: numpy.random.default_rng(seed), one rng.permutation(S) per row."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(int(S)) for _ in range(int(n_perm))]).astype(np.int64).reshape(int(n_perm), int(S))


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _sweep(v, basis):
    """v minus its mean and its components along the orthonormal basis, twice (the second pass takes the first's rounding)."""
    for _ in range(2):
        v = v - v.mean()
        for w in basis:
            v = v - w * w.dot(v)
    return v


def glm_design(z_b, z_bt):
    """
    The design of the permutation GLM from the covariates z_b (H, Q) of the controls and z_bt (U, Q) of the patients.  Host
    only, NumPy float64.  The rules are covariates.fit_adjustment's: the columns of Z = [z_b; z_bt] are centred over the
    S = H + U subjects, a constant one (min == max) is dropped, the others are scaled to unit norm, collinear ones are dropped
    by diagonally pivoted Cholesky of their Gram matrix (remaining squared norm below 1e-10, ties to the lowest index).  The
    Q' columns kept give an orthonormal basis w_1 .. w_Q' of the centred nuisance space (Gram-Schmidt in pivot order, twice);
    x = the group indicator (1 on the last U subjects), x_c = x - U/S, x_r = x_c - sum_q w_q (w_q^T x_c), w_0 = x_r / ||x_r||.

    Returns (W, info): W (S, Q' + 1) = [w_0, w_1, .., w_Q'], columns orthonormal and orthogonal to the constant; info a dict
    with used (Q,) bool, the columns kept, in the order of the columns of z; rank = Q'; dof = S - Q' - 2.
    ValueError: shapes that do not agree, a NaN or an infinite value, S < Q' + 3, or ||x_r||^2 not > 1e-10 ||x_c||^2 (the
    group is a function of the covariates).  NotImplementedError: Q' > 8.
    """
    (zb, zt) = (np.asarray(_host(z_b), dtype=np.float64), np.asarray(_host(z_bt), dtype=np.float64))
    if zb.ndim != 2 or zt.ndim != 2 or zb.shape[1] != zt.shape[1] or zb.shape[0] < 1 or zt.shape[0] < 1:
        raise ValueError("glm_design: z_b must have shape (H, Q) and z_bt (U, Q), not %s and %s" % (zb.shape, zt.shape))
    if not (np.isfinite(zb).all() and np.isfinite(zt).all()):
        raise ValueError("glm_design: NaN or infinite value in z_b or z_bt")
    (H, U, Q) = (zb.shape[0], zt.shape[0], zb.shape[1])
    S = H + U
    Z = np.concatenate([zb, zt], axis=0)
    Zc = Z - Z.mean(axis=0)[None, :]
    live = [q for q in range(Q) if Z[:, q].min() != Z[:, q].max()]
    V = np.zeros((S, Q))
    for q in live:
        V[:, q] = Zc[:, q] / np.sqrt(Zc[:, q].dot(Zc[:, q]))
    G = V.T.dot(V)
    for q in range(Q):
        G[q, q] = 1.0 if q in live else 0.0
    (piv, taken) = ([], np.zeros(Q, dtype=bool))
    for _k in range(Q):
        dg = np.where(taken, -1.0, np.diagonal(G))
        p = int(np.argmax(dg))                                   # (ties to the lowest index)
        if not dg[p] >= GLM_DROP_TOL:
            break
        lpp = np.sqrt(dg[p])
        free = ~taken
        free[p] = False
        G[free, p] = G[free, p] / lpp
        G[np.ix_(free, free)] -= np.outer(G[free, p], G[free, p])
        taken[p] = True
        piv.append(p)
    rank = len(piv)
    if rank > GLM_MAX_COLUMNS:
        raise NotImplementedError("glm_design: %d covariate columns kept, at most %d" % (rank, GLM_MAX_COLUMNS))
    if S < rank + 3:
        raise ValueError("glm_design: %d subjects, %d covariate columns need %d" % (S, rank, rank + 3))
    basis = []
    for p in piv:
        v = _sweep(V[:, p], basis)
        basis.append(v / np.sqrt(v.dot(v)))
    x = np.concatenate([np.zeros(H), np.ones(U)])
    xc = x - float(U) / float(S)
    xr = _sweep(xc, basis)
    if not xr.dot(xr) > GLM_CONTRAST_TOL * xc.dot(xc):
        raise ValueError("glm_design: the group is a linear function of the covariates (||x_r||^2 = %.3g ||x_c||^2)"
                         % (xr.dot(xr) / xc.dot(xc)))
    W = np.ascontiguousarray(np.stack([xr / np.sqrt(xr.dot(xr))] + basis, axis=1))
    used = np.zeros(Q, dtype=bool)
    used[piv] = True
    return W, {"used": used, "rank": rank, "dof": S - rank - 2}


def _check_permutations(who, permutations, S):
    perm = _host(permutations)
    if perm.ndim != 2 or perm.shape[1] != S or perm.shape[0] < 1:
        raise ValueError("%s: permutations must have shape (P, %d) with P >= 1, not %s" % (who, S, perm.shape))
    if perm.dtype.kind not in "iu":
        raise ValueError("%s: permutations must hold integers" % who)
    perm = np.ascontiguousarray(perm.astype(np.int64))
    if not (np.sort(perm, axis=1) == np.arange(S, dtype=np.int64)[None, :]).all():
        raise ValueError("%s: every row of permutations must be a permutation of 0 .. %d" % (who, S - 1))
    return perm


def _glm_setup(who, b, bt, H, U, z_b, z_bt, permutations, labels, missing_data, variance, n_perm, seed):
    """
    The host checks of a call with covariates, all before a context exists -> (W, info, permutations (P, S) int64), or None
    for a call without them.
    """
    if (z_b is None) != (z_bt is None):
        raise ValueError("%s: z_b and z_bt must be given together" % who)
    if z_b is None:
        if permutations is not None:
            raise ValueError("%s: permutations belong to a call with covariates (z_b, z_bt); without them pass labels" % who)
        return None
    if labels is not None:
        raise ValueError("%s: labels with covariates: a labelling does not say whose covariates go where; pass permutations" % who)
    if variance not in ("pooled", "welch"):
        raise ValueError("%s: variance must be 'pooled' or 'welch', not %r" % (who, variance))
    if missing_data or variance == "welch":
        raise NotImplementedError("%s: covariates with missing_data=True or variance='welch' are not provided: every "
                                  "connection would have its own design" % who)
    (sb, st) = (_shape(z_b), _shape(z_bt))
    if len(sb) != 2 or len(st) != 2 or sb[0] != H or st[0] != U or sb[1] != st[1]:
        raise ValueError("%s: z_b must have shape (%d, Q) and z_bt (%d, Q), not %s and %s" % (who, H, U, sb, st))
    _refuse_nonfinite(b, bt, who, "the data must be complete and finite")
    (W, info) = glm_design(z_b, z_bt)
    if permutations is None:
        if int(n_perm) < 1:
            raise ValueError("%s: n_perm must be >= 1" % who)
        perm = draw_permutations(n_perm, H + U, seed)
    else:
        perm = _check_permutations(who, permutations, H + U)
    return W, info, perm


def _device_perms(perm, dev):
    """(P, S) int64 on the host -> the uint16 the device reads, as an int16 tensor (the same bits)."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(perm.astype(np.uint16)).view(np.int16), device=dev)


def group_test(b, bt, n_perm=10000, *, missing_data=False, variance="pooled", seed=0, labels=None, z_b=None, z_bt=None,
               permutations=None, ctx=None, as_numpy=True):
    """
    Mass-univariate two-sample test of patients against controls with permutation inference.  b (C, H), bt (C, U), complete
    unless missing_data=True.  What follows first describes the default call (missing_data=False, variance="pooled").

    X = [b | bt] (C, S), S = H + U, rows centred on their mean over all subjects, Q_c = sum x^2.  For a labelling l in
    {0,1}^S with exactly U ones: A = sum l_s x_s, SS_w = Q_c - A^2 S/(U H), Student's t with pooled variance
    t = A (S/(U H)) / sqrt(SS_w/(S - 2) * S/(U H)), and per region R[n] = sum over E(n) of t^2.  The observed labelling has
    its ones on the last U subjects.  labels: (P, S) of 0/1 with U ones per row; not given, n_perm rows are drawn on the
    host (draw_labels(n_perm, H, U, seed)).  A row equal to the observed labelling counts, and gives the observed statistics
    bit for bit; results repeat bit for bit from call to call.

    Returns a dict: t (C,), region (N,) observed; null_max_t (P,) = max_c |t|, null_max_region (P,) = max_n R;
    count_t (C,) int64 = #{p: |t_pc| >= |t_c|}, count_region (N,) int64 = #{p: R_pn >= R_n}; p_t, p_region =
    (1 + count) / (1 + P); p_fwe_t, p_fwe_region = the same against the maxima; labels (P, S) uint8 as used.

    Degenerate connections.  A connection whose S values are all equal (min == max, the rule of the covariate fit) is
    constant: its centred values and Q_c are exactly 0.  Its t is NaN; it adds exactly 0 to every region sum, observed and
    permuted, and enters no maximum; count_t[c] = 0 and p_t[c], p_fwe_t[c] are NaN.  A region whose connections are all
    constant has region = 0, count_region = P and p_region = 1.  No other input gives a NaN, and no region sum ever sees a
    negative term: where SS_w, a difference of two rounded numbers, is not > 0 with Q_c > 0 (complete separation of the two
    groups), t^2 = +inf and t = +/-inf with the sign of A, and inf >= inf counts as IEEE arithmetic has it.

    missing_data=True: a NaN is an unobserved value (an infinite value stays a ValueError).  Per connection, O = the subjects
    observed there, n = |O|; the row is centred on its mean over O, x_s = 0 for a missing subject, Q = sum x^2; it is constant
    where all observed values are equal.  The labellings are what they are without it: U ones over all S subjects, observed
    or not.  Per labelling n1 = the labelled subjects in O, n0 = n - n1, A = sum l_s x_s, B = sum l_s x_s^2, k = n / (n1 n0);
    the mean difference is A k.  The pooled t^2 = g (n - 2) / (Q - g), g = A^2 k, is defined iff the connection is not constant,
    n >= 3, n1 >= 1 and n0 >= 1; on complete data it is the default call bit for bit.  Two keys are added: n_controls,
    n_patients (C,) int64, the observed values per connection under the observed labelling.
    variance="welch": Welch's unequal-variance t (no degrees of freedom are needed: the inference is by permutation).
    SS1 = max(B - A^2/n1, 0), SS0 = max((Q - B) - A^2/n0, 0), v = SS1/(n1 (n1 - 1)) + SS0/(n0 (n0 - 1)), t^2 = (A k)^2 / v with
    the sign of A; defined iff the connection is not constant, n1 >= 2 and n0 >= 2; where v is not > 0, t^2 = +inf if A != 0
    and 0 if A = 0.  H < 2 or U < 2 is a ValueError.
    A value that is undefined under a labelling adds exactly 0 to every region sum and enters no maximum, but counts as an
    exceedance in count_t: the conservative choice, a labelling that cannot be evaluated never makes a p-value smaller.  A
    connection that is undefined under the observed labelling is dead exactly as a constant one is: t NaN, count_t 0, p_t and
    p_fwe_t NaN, no part in region or in any permuted sum or maximum.  The identity-row property and the repeatability hold
    with either option.

    z_b (H, Q), z_bt (U, Q): nuisance covariates (age, sex, site dummies, motion, ...) by the permutation GLM of Freedman &
    Lane (1983; Winkler et al. 2014), what FSL randomise, PALM and the NBS toolbox run.  glm_design(z_b, z_bt) gives the
    orthonormal W = [w_0, w_1 .. w_Q'] (w_0 the group indicator residualised on the Q' covariate columns kept) and
    dof = S - Q' - 2.  Per connection e = the residuals of the row on the nuisance model [1, Z], Q_e = sum e^2.  A
    permutation pi of 0 .. S - 1 gives subject s the design row pi[s] (the residuals permuted by its inverse under the fixed
    design): d_q = sum_s W[pi[s], q] e_s, t^2 = d_0^2 dof / (Q_e - sum_q d_q^2), t with the sign of d_0 (t > 0: patients
    above controls).  The observed statistics are those of the identity.  permutations: (P, S) integers, every row a
    permutation; not given, draw_permutations(n_perm, S, seed).  labels= is refused: a labelling does not say whose
    covariates go where.  A row equal to the identity counts and gives the observed statistics bit for bit.  The rules for
    constant and separated connections hold unchanged; dead too (t NaN and all that follows) is a connection with
    Q_e <= (8 S (Q' + 1) 2^-52)^2 Q_c: a linear function of the covariates to rounding.  The dict gains permutations (P, S)
    int64 as used and design_info (glm_design's: used, rank, dof); labels is (pi >= H).  Where every column is dropped
    (Q' = 0) the call is the default call with those labels, bit for bit.  ValueError before any context exists: z_b without
    z_bt, shapes that do not agree, a NaN or an infinite covariate, S < Q' + 3, a group that is a linear function of the
    covariates, a row that is no permutation.  NotImplementedError: Q' > 8.
    Not provided with covariates: missing_data or Welch's t (every connection would have its own design: NotImplementedError),
    more than 8 columns, contrasts other than the group (the C entry point tests column 0 of any orthonormal design), F-tests,
    exchangeability blocks (permuting within site), sessions, noise variances.

    Without missing_data a NaN or an infinite value is a ValueError; more than 1024 subjects a NotImplementedError.
    Not provided: sessions, noise variances, cluster statistics.  The network-based statistic is network_test().
    """
    import torch
    (C, N, H, U) = _check_pair(b, bt, "group_test")
    S = H + U
    if S > MAX_SUBJECTS:
        raise NotImplementedError("group_test: %d subjects, at most %d" % (S, MAX_SUBJECTS))
    if S < 3:
        raise ValueError("group_test: %d subjects, a pooled variance needs 3" % S)
    glm = _glm_setup("group_test", b, bt, H, U, z_b, z_bt, permutations, labels, missing_data, variance, n_perm, seed)
    if glm is not None and glm[1]["rank"] == 0:                  # every column dropped: the default call with those labels
        out = group_test(b, bt, labels=(glm[2] >= H).astype(np.uint8), ctx=ctx, as_numpy=as_numpy)
        out["permutations"] = glm[2] if as_numpy else torch.as_tensor(glm[2], device=out["t"].device)
        out["design_info"] = glm[1]
        return out
    if glm is not None:
        flags = 0
        lab = (glm[2] >= H).astype(np.uint8)
    else:
        flags = _options("group_test", b, bt, H, U, missing_data, variance)
        if labels is None:
            if int(n_perm) < 1:
                raise ValueError("group_test: n_perm must be >= 1")
            lab = draw_labels(n_perm, H, U, seed)
        else:
            lab = _check_labels(labels, S, U)
    P = int(lab.shape[0])
    ctx = ctx if ctx is not None else _lib.Context()
    (bd, btd) = (_device_f64(b, ctx), _device_f64(bt, ctx))
    dev = ctx.device
    labd = torch.as_tensor(lab, device=dev)
    out = dict((k, torch.empty((n,), dtype=dt, device=dev)) for (k, n, dt) in (
        ("t", C, torch.float64), ("region", N, torch.float64), ("null_max_t", P, torch.float64),
        ("null_max_region", P, torch.float64), ("count_t", C, torch.int64), ("count_region", N, torch.int64)))
    counts = [torch.empty((C,), dtype=torch.int64, device=dev) for _ in range(2)] if missing_data else [None, None]

    def call(name, *rows, tail=()):
        ctx.call(name, _lib.dptr(bd), _lib.dptr(btd), C, H, U, *rows, *[_lib.dptr(v) for v in out.values()],
                 *[_lib.dptr(v) for v in tail], _lib.stream_ptr())

    if glm is not None:
        (designd, permd) = (_device_f64(glm[0], ctx), _device_perms(glm[2], dev))
        call("fcd_baseline_group_glm", _lib.dptr(designd), int(designd.shape[1]), _lib.dptr(permd), P)
    elif flags == 0:
        call("fcd_baseline_group_perm", _lib.dptr(labd), P)
    else:
        call("fcd_baseline_group_perm_opt", _lib.dptr(labd), P, flags, tail=counts)
        if missing_data:
            out.update(n_controls=counts[0], n_patients=counts[1])
    host = dict((k, v.cpu().numpy()) for (k, v) in out.items())
    pv = group_pvalues(host["t"], host["region"], host["null_max_t"], host["null_max_region"], host["count_t"],
                       host["count_region"])
    if as_numpy:
        out = host
        out.update(pv)
    else:
        out.update(dict((k, torch.as_tensor(v, device=dev)) for (k, v) in pv.items()))
    out["labels"] = lab if as_numpy else labd
    if glm is not None:
        out["permutations"] = glm[2] if as_numpy else torch.as_tensor(glm[2], device=dev)
        out["design_info"] = glm[1]
    return out


def group_pvalues(t, region, null_max_t, null_max_region, count_t, count_region):
    """
    The host half of group_test(): p_t, p_region, p_fwe_t, p_fwe_region, each (1 + count) / (1 + P).  p_t and p_fwe_t are NaN
    where t is NaN (a constant connection); an infinite value is counted by >= like any other (inf >= inf).
    """
    P = null_max_t.shape[0]
    dead = np.isnan(t)
    return {"p_t": np.where(dead, np.nan, (1.0 + count_t) / (1.0 + P)),
            "p_region": (1.0 + count_region) / (1.0 + P),
            "p_fwe_t": np.where(dead, np.nan, (1.0 + _count_ge(null_max_t, np.abs(t))[0]) / (1.0 + P)),
            "p_fwe_region": (1.0 + _count_ge(null_max_region, region)[0]) / (1.0 + P)}


# ---- network-based statistic -------------------------------------------------------------------------------------------------

MAX_REGIONS = 1024        # graph_components(), network_test(): a row of bits lives in one workgroup's LDS (64 KB at 1024)
_P_CHUNK = 1 << 14        # labellings per call of network_test(): bounds the bit workspace (W words each)
_X_BYTES = 256 << 20      # statistic="intensity": the (n, 32 W) doubles of a chunk's excess values (partial_correlations' dense-chunk figure)
TAILS = {"both": 0, "greater": 1, "less": 2}
STATISTICS = ("extent", "intensity")


def _excess_chunk(W):
    """Labellings whose excess values, 32 W doubles each, fit in _X_BYTES; at least 1."""
    return max(1, _X_BYTES // (8 * 32 * W))


def _pair_index(N):
    """(n, m) of every connection, in util.c_to_nm order."""
    (n, m) = np.tril_indices(N, -1)
    return n.astype(np.int64), m.astype(np.int64)


def _component_tables(component, edge_mask):
    """(label, edges, regions) of the components of one graph, by decreasing extent and then by label."""
    N = component.shape[0]
    n_of = _pair_index(N)[0]
    edges = np.bincount(component[n_of[edge_mask]], minlength=N)
    regions = np.bincount(component[component >= 0], minlength=N)
    label = np.flatnonzero(edges > 0)
    label = label[np.lexsort((label, -edges[label]))].astype(np.int64)
    return label, edges[label].astype(np.int64), regions[label].astype(np.int64)


def network_pvalues(component_edges, null_max_extent):
    """The host half of network_test(): p_fwe[k] = (1 + #{p: null_max_extent[p] >= component_edges[k]}) / (1 + P)."""
    (ge, P) = _count_ge(np.asarray(null_max_extent, dtype=np.float64).reshape(-1),
                        np.asarray(component_edges, dtype=np.float64).reshape(-1))
    return (1.0 + ge) / (1.0 + P)


def network_intensity_pvalues(component_intensity, null_max_intensity):
    """The same by intensity: p_fwe[k] = (1 + #{p: null_max_intensity[p] >= component_intensity[k]}) / (1 + P); inf >= inf counts."""
    (ge, P) = _count_ge(np.asarray(null_max_intensity, dtype=np.float64).reshape(-1),
                        np.asarray(component_intensity, dtype=np.float64).reshape(-1))
    return (1.0 + ge) / (1.0 + P)


def _components_call(ctx, bits, B, C, N, component, n_edges, max_extent, max_regions):
    ctx.call("fcd_graph_components", _lib.dptr(bits), B, C, _lib.dptr(component), _lib.dptr(n_edges), _lib.dptr(max_extent),
             _lib.dptr(max_regions), _lib.stream_ptr())


def _weighted_components_call(ctx, bits, weights, B, C, component, n_edges, max_extent, max_regions, intensity, max_intensity):
    import ctypes
    d = _lib.ComponentsDesc.make(B=B, C=C, stream=_lib.stream_ptr(), bits=_lib.dptr(bits), weights=_lib.dptr(weights),
                                 component=_lib.dptr(component), n_edges=_lib.dptr(n_edges), max_extent=_lib.dptr(max_extent),
                                 max_regions=_lib.dptr(max_regions), intensity=_lib.dptr(intensity),
                                 max_intensity=_lib.dptr(max_intensity))
    ctx.call("fcd_graph_components_weighted", ctypes.byref(d))


def _check_weights(mask, weights, sh):
    """weights as a float64 torch tensor of the mask's shape, >= 0 and not NaN where the mask is set (checked where it lies)."""
    import torch
    w = weights if isinstance(weights, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(weights))
    if tuple(w.shape) != tuple(sh):
        raise ValueError("graph_components: weights must have the mask's shape %s, not %s" % (sh, tuple(w.shape)))
    if w.dtype != torch.float64:
        raise ValueError("graph_components: weights must be float64, not %s" % (w.dtype,))
    m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(mask))
    at = w[(m != 0).to(w.device)]
    if bool((torch.isnan(at) | (at < 0.0)).any().item()):
        raise ValueError("graph_components: weights must be >= 0 and not NaN where the mask is set")
    return w


def graph_components(mask, weights=None, *, ctx=None, as_numpy=True):
    """
    Connected components of the graphs on N regions whose edges are the set entries of mask, (C,) or (B, C), bool or 0/1,
    NumPy or torch, connections in util.c_to_nm order.  On the device (fcd_graph_components), one workgroup per graph.

    A component's label is the smallest region in it, its extent its number of connections; a region without a connection
    belongs to none and has label -1.  Returns a dict: component (B, N) int64; n_edges, max_extent, max_regions (B,) int64 =
    set connections, extent of the largest component, regions of the component with the most regions.  For a 1-D mask the
    leading axis is dropped and component_label, component_edges, component_regions (K,) list the K >= 0 components by
    decreasing extent, then by label.  NumPy arrays, or device tensors with as_numpy=False.
    weights, float64 of the mask's shape: a weight per connection, read only where the mask is set, >= 0 and not NaN there
    (+inf is allowed; ValueError otherwise) -- t excesses, or the posterior mass of a thresholded connection_posterior().  The
    call (fcd_graph_components_weighted) then adds max_weight (B,) float64, the largest sum of weights over a component (0.0
    for an empty graph), and for a 1-D mask component_weight (K,), the sum of each listed component.  The sums are taken in
    a fixed order without floating-point atomics: they repeat exactly and do not depend on B or on a graph's place.
    A non-triangular C is a ValueError, more than 1024 regions a NotImplementedError.
    """
    import torch
    sh = _shape(mask)
    if len(sh) not in (1, 2) or (len(sh) == 2 and sh[0] < 1):
        raise ValueError("graph_components: mask must have shape (C,) or (B, C) with B >= 1, not %s" % (sh,))
    C = sh[-1]
    N = _n_regions(C)
    if N > MAX_REGIONS:
        raise NotImplementedError("graph_components: %d regions, at most %d" % (N, MAX_REGIONS))
    if weights is not None:
        weights = _check_weights(mask, weights, sh)
    ctx = ctx if ctx is not None else _lib.Context()
    dev = ctx.device
    m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(mask))
    m = m.to(device=dev).reshape(-1, C)
    if not bool(((m == 0) | (m == 1)).all().item()):
        raise ValueError("graph_components: mask must hold 0 and 1 (or booleans) only")
    B = int(m.shape[0])
    W = (C + 31) // 32
    # bit c & 31 of word c >> 5, as bytes: bit c & 7 of byte c >> 3
    padded = torch.zeros((B, 32 * W), dtype=torch.int32, device=dev)
    padded[:, :C] = m.to(torch.int32)
    place = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    bits = (padded.view(B, 4 * W, 8) * place).sum(dim=2).to(torch.uint8).contiguous()
    component = torch.empty((B, N), dtype=torch.int32, device=dev)
    (n_edges, max_extent, max_regions) = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    if weights is None:
        _components_call(ctx, bits, B, C, N, component, n_edges, max_extent, max_regions)
    else:
        wd = torch.zeros((B, 32 * W), dtype=torch.float64, device=dev)
        wd[:, :C] = weights.to(device=dev).reshape(-1, C)
        intensity = torch.empty((B, N), dtype=torch.float64, device=dev)
        max_weight = torch.empty((B,), dtype=torch.float64, device=dev)
        _weighted_components_call(ctx, bits, wd, B, C, component, n_edges, max_extent, max_regions, intensity, max_weight)
    out = {"component": component.long(), "n_edges": n_edges.long(), "max_extent": max_extent.long(),
           "max_regions": max_regions.long()}
    if weights is not None:
        out["max_weight"] = max_weight
    if len(sh) == 1:
        out = dict((k, v[0]) for (k, v) in out.items())
        tables = _component_tables(out["component"].cpu().numpy(), m[0].cpu().numpy().astype(bool))
        names = ("component_label", "component_edges", "component_regions")
        if weights is not None:
            tables = tables + (intensity[0].cpu().numpy()[tables[0]],)
            names = names + ("component_weight",)
        if as_numpy:
            out = dict((k, v.cpu().numpy()) for (k, v) in out.items())
            out.update(zip(names, tables))
        else:
            out.update((k, torch.as_tensor(v, device=dev)) for (k, v) in zip(names, tables))
        return out
    return dict((k, v.cpu().numpy()) for (k, v) in out.items()) if as_numpy else out


def network_test(b, bt, threshold, n_perm=10000, *, tail="both", missing_data=False, variance="pooled", seed=0, labels=None,
                 z_b=None, z_bt=None, permutations=None, ctx=None, as_numpy=True, statistic="extent"):
    """
    The network-based statistic (Zalesky, Fornito & Bullmore 2010): which sub-networks differ between patients and controls?
    b (C, H), bt (C, U), complete unless missing_data=True.

    Data, labellings, centring and the t are group_test()'s, its options missing_data and variance ("pooled" or "welch")
    with their rules included: a value that is undefined under a labelling is never suprathreshold, a connection that is
    undefined under the observed labelling has t = NaN and is never suprathreshold under any labelling, and
    missing_data=True adds the keys n_controls and n_patients (C,) int64.  In the default call the t is the pooled-variance
    t; the observed labelling has its ones on the last U subjects.  A connection is suprathreshold where |t| > threshold
    (tail="both"), t > threshold ("greater": patients above controls, the sign of group_test's t) or t < -threshold
    ("less"); threshold > 0 in t units.  The components are those of the graph on the N regions whose edges are the
    suprathreshold connections: a component's extent is its number of connections, its label the smallest region in it; a
    region without a suprathreshold connection has label -1.  The family-wise error is controlled by the permutation law of
    the largest extent.  labels as in group_test(); a row equal to the observed labelling counts, and gives the observed bits
    exactly.  Labellings are walked in chunks; the results do not depend on the chunk size and repeat exactly from call to
    call.  Degenerate connections as in group_test(): a constant connection has t = NaN and is never suprathreshold, under
    any labelling; a completely separated one has t = +/-inf and is suprathreshold on its side.

    Returns a dict: t (C,); edge_mask (C,) bool; component (N,) int64; component_label, component_edges, component_regions
    (K,) int64, the K >= 0 observed components by decreasing extent, then by label; null_max_extent, null_max_regions,
    null_n_edges (P,) int64 = per labelling the largest extent, the regions of the component with the most regions, the
    suprathreshold connections; p_fwe (K,) = (1 + #{p: null_max_extent[p] >= extent}) / (1 + P); p_fwe_region (N,) = the p of
    the region's component, NaN at label -1; labels (P, S) uint8 as used; threshold, tail.
    z_b (H, Q), z_bt (U, Q), permutations: nuisance covariates exactly as in group_test() -- its permutation GLM, its t
    (the side of "greater" / "less" is the sign of d_0), its refusals (labels=, missing_data and Welch's t included) and its
    keys permutations and design_info; labels is (pi >= H).  A row equal to the identity gives the observed bits exactly;
    permutations are walked in chunks as labellings are.  Where every column is dropped the call is the default call.
    statistic="intensity": the other component size of the NBS toolbox, for effects that are strong but confined to few
    connections.  The excess of a suprathreshold connection is e = max(|t| - threshold, 0) (+inf at t = +/-inf), a
    component's intensity the sum of e over its connections, and the family-wise error is controlled by the permutation law
    of the largest intensity (0.0 for an empty graph).  Every key above keeps its value bit for bit -- the component tables
    stay ordered by decreasing extent, then by label -- except that p_fwe and p_fwe_region are by intensity,
    (1 + #{p: null_max_intensity[p] >= intensity}) / (1 + P), inf >= inf counting as in group_test().  Added:
    component_intensity (K,) float64; null_max_intensity (P,) float64; p_fwe_extent (K,), the p_fwe of the extent call;
    statistic.  All three forms of the t are served, with their rules; a value exists only where a bit is set, and the sums
    are taken in a fixed order without floating-point atomics, so the results repeat exactly, a row equal to the observed
    labelling (the identity) gives the observed intensities bit for bit, and neither chunk length (the second keeps a
    chunk's excess values within 256 MB) changes a bit.
    Refused: everything group_test() refuses; a threshold that is not finite and > 0, an unknown tail or an unknown
    statistic (ValueError); more than 1024 regions (NotImplementedError).  Not provided: TFCE, sessions, noise variances;
    with covariates also what group_test() lists.
    """
    import torch
    (C, N, H, U) = _check_pair(b, bt, "network_test")
    S = H + U
    if S > MAX_SUBJECTS:
        raise NotImplementedError("network_test: %d subjects, at most %d" % (S, MAX_SUBJECTS))
    if N > MAX_REGIONS:
        raise NotImplementedError("network_test: %d regions, at most %d" % (N, MAX_REGIONS))
    if S < 3:
        raise ValueError("network_test: %d subjects, a pooled variance needs 3" % S)
    thr = float(threshold)
    if not np.isfinite(thr) or thr <= 0.0:
        raise ValueError("network_test: threshold must be finite and > 0, not %r" % (threshold,))
    if tail not in TAILS:
        raise ValueError("network_test: tail must be one of 'both', 'greater', 'less', not %r" % (tail,))
    if statistic not in STATISTICS:
        raise ValueError("network_test: statistic must be one of 'extent', 'intensity', not %r" % (statistic,))
    glm = _glm_setup("network_test", b, bt, H, U, z_b, z_bt, permutations, labels, missing_data, variance, n_perm, seed)
    if glm is not None and glm[1]["rank"] == 0:                  # every column dropped: the default call with those labels
        out = network_test(b, bt, thr, tail=tail, labels=(glm[2] >= H).astype(np.uint8), ctx=ctx, as_numpy=as_numpy,
                           statistic=statistic)
        out["permutations"] = glm[2] if as_numpy else torch.as_tensor(glm[2], device=out["t"].device)
        out["design_info"] = glm[1]
        return out
    if glm is not None:
        flags = 0
        lab = (glm[2] >= H).astype(np.uint8)
    else:
        flags = _options("network_test", b, bt, H, U, missing_data, variance)
        if labels is None:
            if int(n_perm) < 1:
                raise ValueError("network_test: n_perm must be >= 1")
            lab = draw_labels(n_perm, H, U, seed)
        else:
            lab = _check_labels(labels, S, U)
    P = int(lab.shape[0])
    ctx = ctx if ctx is not None else _lib.Context()
    (bd, btd) = (_device_f64(b, ctx), _device_f64(bt, ctx))
    dev = ctx.device
    labd = torch.as_tensor(lab, device=dev)
    W = (C + 31) // 32
    if glm is not None:
        (designd, rows) = (_device_f64(glm[0], ctx), _device_perms(glm[2], dev))
    else:
        rows = labd

    def i32(*sh):
        return torch.empty(sh, dtype=torch.int32, device=dev)

    intensity = statistic == "intensity"

    def f64(*sh):
        return torch.empty(sh, dtype=torch.float64, device=dev)

    def bits_call(lab_c, n, bits, t, excess=None):
        if excess is not None:                                 # one entry point for the three statistics
            import ctypes
            d = _lib.NetworkExcessDesc.make(flags=flags, C=C, H=H, U=U, P=n, threshold=thr, tail=TAILS[tail], stream=_lib.stream_ptr(),
                                            b=_lib.dptr(bd), bt=_lib.dptr(btd), bits=_lib.dptr(bits), excess=_lib.dptr(excess),
                                            t=_lib.dptr(t))
            if glm is not None:
                (d.design, d.R, d.perms) = (_lib.dptr(designd), int(designd.shape[1]), _lib.dptr(lab_c))
            else:
                d.labels = _lib.dptr(lab_c)
            ctx.call("fcd_baseline_network_excess", ctypes.byref(d))
        elif glm is not None:
            ctx.call("fcd_baseline_network_bits_glm", _lib.dptr(bd), _lib.dptr(btd), C, H, U, _lib.dptr(designd),
                     int(designd.shape[1]), _lib.dptr(lab_c), n, thr, TAILS[tail], _lib.dptr(bits), _lib.dptr(t), _lib.stream_ptr())
        elif flags == 0:
            ctx.call("fcd_baseline_network_bits", _lib.dptr(bd), _lib.dptr(btd), C, H, U, _lib.dptr(lab_c), n, thr, TAILS[tail],
                     _lib.dptr(bits), _lib.dptr(t), _lib.stream_ptr())
        else:
            ctx.call("fcd_baseline_network_bits_opt", _lib.dptr(bd), _lib.dptr(btd), C, H, U, _lib.dptr(lab_c), n, thr,
                     TAILS[tail], flags, _lib.dptr(bits), _lib.dptr(t), _lib.stream_ptr())

    # the observed labelling: the same kernels at P = 1
    t = torch.empty((C,), dtype=torch.float64, device=dev)
    bits_obs = i32(1, W)
    (component, obs_edges, obs_extent, obs_regions) = (i32(1, N), i32(1), i32(1), i32(1))
    (null_n_edges, null_max_extent, null_max_regions) = (i32(P), i32(P), i32(P))
    if intensity:
        # a value only where a bit is set: the buffers are never initialised, and only read at set bits
        (obs_sums, obs_max, null_max_intensity) = (f64(1, N), f64(1), f64(P))
        excess_obs = f64(1, 32 * W)
        bits_call(None, 1, bits_obs, t, excess_obs)
        _weighted_components_call(ctx, bits_obs, excess_obs, 1, C, component, obs_edges, obs_extent, obs_regions, obs_sums, obs_max)
        chunk = min(_P_CHUNK, _excess_chunk(W))
    else:
        bits_call(None, 1, bits_obs, t)
        _components_call(ctx, bits_obs, 1, C, N, component, obs_edges, obs_extent, obs_regions)
        chunk = _P_CHUNK
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        bits = i32(n, W)
        if intensity:
            excess = f64(n, 32 * W)
            bits_call(rows[p0:p0 + n], n, bits, None, excess)
            _weighted_components_call(ctx, bits, excess, n, C, None, null_n_edges[p0:p0 + n], null_max_extent[p0:p0 + n],
                                      null_max_regions[p0:p0 + n], None, null_max_intensity[p0:p0 + n])
        else:
            bits_call(rows[p0:p0 + n], n, bits, None)
            _components_call(ctx, bits, n, C, N, None, null_n_edges[p0:p0 + n], null_max_extent[p0:p0 + n],
                             null_max_regions[p0:p0 + n])
    host = {"t": t.cpu().numpy(), "component": component[0].long().cpu().numpy(),
            "null_max_extent": null_max_extent.long().cpu().numpy(), "null_max_regions": null_max_regions.long().cpu().numpy(),
            "null_n_edges": null_n_edges.long().cpu().numpy()}
    host["edge_mask"] = np.unpackbits(bits_obs.cpu().numpy().view(np.uint8).reshape(-1), bitorder="little")[:C].astype(bool)
    (label, edges, regions) = _component_tables(host["component"], host["edge_mask"])
    host.update(component_label=label, component_edges=edges, component_regions=regions)
    host["p_fwe"] = network_pvalues(edges, host["null_max_extent"])
    if intensity:
        host["component_intensity"] = obs_sums[0].cpu().numpy()[label]
        host["null_max_intensity"] = null_max_intensity.cpu().numpy()
        host["p_fwe_extent"] = host["p_fwe"]
        host["p_fwe"] = network_intensity_pvalues(host["component_intensity"], host["null_max_intensity"])
    p_of = np.full(N + 1, np.nan)                            # (label -1 reads the last entry)
    p_of[label] = host["p_fwe"]
    host["p_fwe_region"] = p_of[host["component"]]
    if missing_data:
        host["n_controls"] = (~torch.isnan(bd)).sum(dim=1).cpu().numpy()
        host["n_patients"] = (~torch.isnan(btd)).sum(dim=1).cpu().numpy()
    out = host if as_numpy else dict((k, torch.as_tensor(v, device=dev)) for (k, v) in host.items())
    out["labels"] = lab if as_numpy else labd
    if glm is not None:
        out["permutations"] = glm[2] if as_numpy else torch.as_tensor(glm[2], device=dev)
        out["design_info"] = glm[1]
    out["threshold"] = thr
    out["tail"] = tail
    if intensity:
        out["statistic"] = statistic
    return out
