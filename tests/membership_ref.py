"""
NumPy restatement of membership() (fcdiff_amd/membership.py, fcd_member.hip), written from the model's definitions:
  control_loglik   lc[g, u] = sum_c log N(x_cu; mu_k, sigma_k), k = f[g, c]
  patient_loglik   lp[g, u] = sum_c log M_{k, l}(x_cu), M_{k, l} = eps_l N_k + (1 - eps_l) / 2 (N_j + N_j'), l the mixture case
                   of (r[g, n], r[g, m]) at the endpoints of c = n (n - 1) / 2 + m
and the exact predictive laws of tiny models by enumeration (shared: over the states of shared_region_ref; unshared: the
template f enumerated, every patient's r summed out).  Used by tests/test_membership.py and tests/test_gpu_membership.py.
"""
import itertools

import numpy as np

import shared_region_ref as SR


def endpoints(Nreg):
    (n, m) = np.tril_indices(Nreg, -1)          # c = n(n-1)/2 + m, n > m: the fitter's edge order
    return n, m


def eps_l(theta):
    """(3,) weight of the template's own type in mixture case l = 0 both typical, 1 both anomalous, 2 discordant."""
    (eta, eps) = (theta[1], theta[2])
    return np.array([1.0 - eps, eps, eta * eps + (1.0 - eta) * (1.0 - eps)])


def normal_logs(x, theta, missing=False):
    """(C, U, 3) log N(x_cu; mu_k, sigma_k); a NaN x gives 0 with `missing`."""
    th = np.asarray(theta, dtype=np.float64)
    out = np.stack([SR._nlogpdf(x, th[6 + k], th[9 + k]) for k in range(3)], axis=2)
    if missing:
        out[np.isnan(x)] = 0.0
    return out


def mixture_logs(x, theta, missing=False):
    """(C, U, 3, 3) log M_{k, l}(x_cu); a NaN x gives 0 with `missing`."""
    th = np.asarray(theta, dtype=np.float64)
    dens = np.stack([SR._npdf(x, th[6 + k], th[9 + k]) for k in range(3)], axis=2)           # (C, U, 3)
    others = dens.sum(axis=2, keepdims=True) - dens
    e = eps_l(th)
    with np.errstate(divide="ignore"):
        out = np.log(e[None, None, None, :] * dens[..., None] + ((1.0 - e) * 0.5)[None, None, None, :] * others[..., None])
    if missing:
        out[np.isnan(x)] = 0.0
    return out


def control_loglik(x, theta, f, missing=False):
    """(G, U) from x (C, U) and plain states f (G, C) in {0, 1, 2}."""
    ln = normal_logs(x, theta, missing)                              # (C, U, 3)
    f = np.asarray(f, dtype=np.int64)
    C = ln.shape[0]
    return ln[np.arange(C)[None, :], :, f].sum(axis=1)              # (G, C, U) -> (G, U)


def mix_cases(r, Nreg):
    """(G, C) or (G, C, U) mixture case of every edge from r (G, Nreg) or (G, Nreg, U)."""
    (n, m) = endpoints(Nreg)
    (a, b) = (np.asarray(r)[:, n].astype(bool), np.asarray(r)[:, m].astype(bool))
    return np.where(a & b, 1, np.where(a ^ b, 2, 0))


def patient_loglik(x, theta, f, r, missing=False):
    """(G, U) from x (C, U), f (G, C) and r (G, Nreg): one column for every subject, or (G, Nreg, U): one per subject."""
    lm = mixture_logs(x, theta, missing)                             # (C, U, 3, 3)
    f = np.asarray(f, dtype=np.int64)
    (C, U) = lm.shape[:2]
    r = np.asarray(r)
    l = mix_cases(r, r.shape[1])
    if l.ndim == 2:
        l = np.broadcast_to(l[:, :, None], l.shape + (U,))
    out = np.zeros((f.shape[0], U))
    for c0 in range(0, C, 256):
        cs = np.arange(c0, min(C, c0 + 256))
        out += lm[cs[None, :, None], np.arange(U)[None, None, :], f[:, cs, None], l[:, cs, :]].sum(axis=1)
    return out


def pooled(l, P):
    """
    For per-state log-likelihoods l (S, U) and the states' posterior P (S,): (log E_P e^l (U,), rel (U,)) with
    rel = sqrt(Var_P[e^l]) / E_P[e^l] -- the exact standard error of the log-mean-exp over G draws is rel / sqrt(G).
    """
    mx = l.max(axis=0)
    e = np.exp(l - mx[None, :])
    m1 = (P[:, None] * e).sum(axis=0)
    m2 = (P[:, None] * e * e).sum(axis=0)
    return mx + np.log(m1), np.sqrt(np.maximum(m2 / (m1 * m1) - 1.0, 0.0))


def exact_shared(b, bt, theta, x_new, missing=False):
    """
    The shared-region model at small N by enumeration: the posterior of (f, r) from shared_region_ref.enumerate_posterior's
    logjoint and states, and with it log p(x_u | data, patient) = log E_post exp lp, log p(x_u | data, control) =
    log E_post exp lc and the relative standard deviations of exp lp / exp lc under the posterior.
    """
    ex = SR.enumerate_posterior(b, bt, theta, missing=missing)
    lj = ex["logjoint"]                                               # (3^C, 2^N)
    P = np.exp(lj - ex["log_evidence"])
    (Fa, Ra) = (ex["states_f"], ex["states_r"])
    lc = control_loglik(x_new, theta, Fa, missing)                    # (nF, U): the control side does not see r
    (log_c, rel_c) = pooled(lc, P.sum(axis=1))
    (nF, nR) = lj.shape
    f_all = np.repeat(Fa, nR, axis=0)
    r_all = np.tile(Ra, (nF, 1))
    lp = patient_loglik(x_new, theta, f_all, r_all, missing)          # (nF nR, U)
    (log_p, rel_p) = pooled(lp, P.reshape(-1))
    return {"log_patient": log_p, "rel_patient": rel_p, "log_control": log_c, "rel_control": rel_c}


def exact_unshared(b, bt, theta, x_new, missing=False):
    """
    The unshared model at small N: p(f | data) with every patient's r summed out (all 3^C templates, 2^N configurations of
    r per patient), then log p(x_u | data, group) = log E_{f | data} p(x_u | f, group) and the relative standard deviation of
    p(x_u | f, group) over the posterior of f (for the patient side: the part of the estimator's variance that is not AIS
    noise).
    """
    th = np.asarray(theta, dtype=np.float64)
    (pi, gamma) = (th[0], th[3:6])
    C = b.shape[0]
    N = int(round((1 + np.sqrt(1 + 8 * C)) / 2))
    F = np.array(list(itertools.product(range(3), repeat=C)))
    R = np.array(list(itertools.product((0, 1), repeat=N)))
    lr = np.where(R > 0, np.log(pi), np.log(1 - pi)).sum(axis=1)      # (nR,)
    L = mix_cases(R, N)                                               # (nR, C)

    def log_pred(x):
        """(nF, U) log p(x_u | f, patient) = log sum_r p(r) prod_c M_{f_c, l}(x_cu)."""
        lm = mixture_logs(x, th, missing)                             # (C, U, 3, 3)
        U = lm.shape[1]
        out = np.zeros((len(F), U))
        for (i, f) in enumerate(F):
            t = lm[np.arange(C)[None, :], :, f[None, :], L].sum(axis=1) + lr[:, None]      # (nR, C, U) -> (nR, U)
            mx = t.max(axis=0)
            out[i] = mx + np.log(np.exp(t - mx[None, :]).sum(axis=0))
        return out

    S_B = normal_logs(b, th, missing).sum(axis=1)                     # (C, 3)
    lpost = (np.log(gamma)[None, :] + S_B)[np.arange(C)[None, :], F].sum(axis=1) + log_pred(bt).sum(axis=1)
    P = np.exp(lpost - lpost.max())
    P /= P.sum()
    (log_p, rel_p) = pooled(log_pred(x_new), P)
    (log_c, rel_c) = pooled(control_loglik(x_new, th, F, missing), P)
    return {"log_patient": log_p, "rel_patient": rel_p, "log_control": log_c, "rel_control": rel_c}
