"""
NumPy reference of the measurement-noise tables, for test_noise.py and test_gpu_noise.py.  TEST INFRASTRUCTURE ONLY: the
product code does not import it.

Every control h and every session k of every patient u carries a known variance on top of the population spread:
    b_ch    | F_c = k    ~ N(mu_k, sigma_k^2 + var_b[h])
    bt_cuk  | F~_cu = j  ~ N(mu_j, sigma_j^2 + var_bt[u, k])          (sessions conditionally independent)
in the log form of sessions_ref.py and with its summation order: a_j = sum_k ln N_j (ascending k, one addition at a time),
m = max_j a_j, lM = m + ln M_kl(exp(a - m)) (sessions_ref.log_M).  A 2-D bt is one session.  None is all zeros.
"""
import numpy as np

import missing_data_ref as MD
import sessions_ref as SR
from oracle import fcdiff_oracle as O


def as_sessions(bt):
    bt = np.asarray(bt, dtype=np.float64)
    return bt[:, :, None] if bt.ndim == 2 else bt


def bt_variances(bt, var_bt):
    """(U, K) float64 of var_bt None, (U,) or (U, K) for bt (C, U, K)."""
    (U, K) = bt.shape[1:]
    if var_bt is None:
        return np.zeros((U, K))
    v = np.asarray(var_bt, dtype=np.float64)
    if v.ndim == 1:
        v = np.repeat(v[:, None], K, axis=1)
    assert v.shape == (U, K)
    return v


def spread(sigma_j, v):
    """s = sqrt(sigma_j^2 + v)"""
    return np.sqrt(sigma_j * sigma_j + v)


def session_log_sums(bt, mu, sigma, var_bt=None, missing=False):
    """(a (C, U, 3), n_observed (C, U)): a[..., j] = sum_k ln N(bt[..., k]; mu_j, sigma_j^2 + var_bt[u, k]) in ascending k."""
    bt = as_sessions(bt)
    v = bt_variances(bt, var_bt)
    a = np.zeros(bt.shape[:2] + (3,))
    nan = np.isnan(bt)
    for k in range(bt.shape[2]):
        for j in range(3):
            with np.errstate(invalid="ignore"):
                l = O.norm_logpdf(bt[:, :, k], mu[j], spread(sigma[j], v[None, :, k]))
            if missing:
                l = np.where(nan[:, :, k], 0.0, l)
            a[:, :, j] = a[:, :, j] + l
    n_obs = (~nan).sum(axis=2) if missing else np.full(bt.shape[:2], bt.shape[2])
    return a, n_obs


def lp_B_g_F(b, mu, sigma, var_b=None, missing=False):
    """(C, H, 3) ln N(b_ch; mu_k, sigma_k^2 + var_b[h]); missing: 0 at a NaN."""
    b = np.asarray(b, dtype=np.float64)
    v = np.zeros(b.shape[1]) if var_b is None else np.asarray(var_b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lpB = np.stack([O.norm_logpdf(b, mu[k], spread(sigma[k], v[None, :])) for k in range(3)], axis=2)
    return np.where(np.isnan(b)[:, :, None], 0.0, lpB) if missing else lpB


def lik_tables(b, bt, mu, sigma, eta, epsilon, var_b=None, var_bt=None, missing=False):
    """(S_B (C, 3), lM (C, U, 3, 3)) of b (C, H) and bt (C, U) or (C, U, K) with the variances var_b (H,), var_bt (U,) / (U, K)."""
    S_B = O.sum_lp_B(lp_B_g_F(b, mu, sigma, var_b, missing))
    (a, n_obs) = session_log_sums(bt, mu, sigma, var_bt, missing)
    return S_B, SR.log_M(a, n_obs, eta, epsilon)


def max_abs_log_sum(bt, mu, sigma, var_bt=None, missing=False):
    (a, _n) = session_log_sums(bt, mu, sigma, var_bt, missing)
    a = a[np.isfinite(a)]
    return float(np.abs(a).max()) if a.size else 0.0


def tolerance(bt, mu, sigma, var_bt=None, missing=False, scale=1.0):
    """sessions_ref.tolerance's rule: rtol 1e-12, atol = 1e-14 max(1, max |sum_k ln N|) (times `scale`)."""
    return dict(rtol=1e-12, atol=1e-14 * max(1.0, max_abs_log_sum(bt, mu, sigma, var_bt, missing)) * scale)


def product_like(x, mu, sigma, v, missing=False):
    """(3,) prod_k N(x_k; mu_j, sigma_j^2 + v_k) of one item's sessions x (K,): the plain product of densities written out
    here, exp(-(x - mu)^2 / (2 s2)) / sqrt(2 pi s2) with s2 = sigma^2 + v (small K only: it underflows)."""
    out = np.ones(3)
    for (xk, vk) in zip(np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)):
        if missing and np.isnan(xk):
            continue
        s2 = np.asarray(sigma, dtype=np.float64) ** 2 + vk
        out = out * np.exp(-(xk - np.asarray(mu)) ** 2 / (2.0 * s2)) / np.sqrt(2.0 * np.pi * s2)
    return out


def enumerated_posterior(W, bt, theta, var_bt=None, missing=False):
    """{p_T, p_F_tilde, p_changed} from missing_data_ref.enumerate_law with like = prod_k N_j (relative to its largest),
    contracted over the weights W (C, U, 3, 3)."""
    theta = np.asarray(theta, dtype=np.float64)
    bt = as_sessions(bt)
    (a, n_obs) = session_log_sums(bt, theta[6:9], theta[9:12], var_bt, missing)
    like = np.exp(a - a.max(axis=2, keepdims=True))
    (C, U) = bt.shape[:2]
    out = {"p_T": np.zeros((C, U)), "p_F_tilde": np.zeros((C, U, 3)), "p_changed": np.zeros((C, U))}
    for c in range(C):
        for u in range(U):
            (_M, pT, pF, pch) = MD.enumerate_law(theta[1], theta[2], like=like[c, u])
            w = W[c, u] / W[c, u].sum()
            out["p_T"][c, u] = (w * pT).sum()
            out["p_F_tilde"][c, u] = np.einsum("kl,klj->j", w, pF)
            out["p_changed"][c, u] = (w * pch).sum()
    return out


def vb_fit(b, bt, theta, iters, mode, shared=False, var_b=None, var_bt=None, lq_F=None, update_theta=True):
    """
    sessions_ref.vb_fit's loop on the noise tables: the oracle's VB iterations without the convergence test; shared: the
    shared-region model, the same loop at one patient on the patient-summed table.  theta as the oracle's dict.
    lq_F given and update_theta False: q_F and theta held, only q_R iterated (the loop of score()).
    Returns dict(energy (iters + 1,), lq_F, lq_R, theta, S_B, lM).
    """
    (C, _H) = b.shape
    N = int(O.C_to_N(C))
    U = 1 if shared else bt.shape[1]
    th = dict(theta)
    lq_R = np.full((N, U, 2), -np.log(2))
    hold_F = lq_F is not None
    if not hold_F:
        lq_F = np.full((C, 1, 3), -np.log(3))

    def tables():
        (S_B, lM) = lik_tables(b, bt, th["mu"], th["sigma"], th["eta"], th["epsilon"], var_b, var_bt)
        return S_B, (lM.sum(axis=1, keepdims=True) if shared else lM)

    def pi2():
        return [1 - th["pi"], th["pi"]]
    (S_B, lM) = tables()
    energy = [O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2())]
    for _ in range(iters):
        if not hold_F:
            lq_F = O.update_lq_F(lq_R, S_B, lM, th["gamma"])
        lq_R = O.update_lq_R(lq_R, lq_F, lM, pi2(), mode)
        if update_theta:
            th["pi"] = O.update_pi(lq_R)
            th["gamma"] = O.update_gamma(lq_F)
            (S_B, lM) = tables()
        energy.append(O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2()))
    return dict(energy=np.array(energy), lq_F=lq_F, lq_R=lq_R, theta=th, S_B=S_B, lM=lM)


# ------------------------------------------------------------------------------------------------
# the scenario of the change's motivation: half the patients measured with more noise
# ------------------------------------------------------------------------------------------------
SCENARIO = dict(N=16, H=20, U=16, seed=5, pi=0.15, first_noisy=8, v=0.01, iters=8)


def scenario_data(model):
    """(b, bt, r (N, U) bool, var_bt (U,)): `model` (pi already SCENARIO['pi']) sampled, then Gaussian noise of variance v
    added to the patients from `first_noisy` on."""
    s = SCENARIO
    (r, _t, _f, _ft, b, bt) = model.sample_fast(s["N"], s["H"], s["U"], seed=s["seed"])
    bt = np.array(bt, dtype=np.float64)
    z = np.random.default_rng(0).standard_normal(bt.shape)
    bt[:, s["first_noisy"]:] += np.sqrt(s["v"]) * z[:, s["first_noisy"]:]
    var_bt = np.zeros(s["U"])
    var_bt[s["first_noisy"]:] = s["v"]
    return b, bt, np.asarray(r, dtype=bool), var_bt


def scenario_rates(lq_R, r):
    """(false-positive share, hit share): the healthy regions of the noisy patients that are flagged (P(r = 1) > 0.5), and the
    truly anomalous regions of the noisy patients that are."""
    k = SCENARIO["first_noisy"]
    flag = np.exp(lq_R[:, k:, 1]) > 0.5
    truth = r[:, k:]
    return float(flag[~truth].mean()), float(flag[truth].mean())


def tolerance_b(b, mu, sigma, var_b=None, missing=False):
    """tolerance()'s rule for the control sums S_B: rtol 1e-12, atol = 1e-14 max(1, max |sum_h ln N|)."""
    S = O.sum_lp_B(lp_B_g_F(b, mu, sigma, var_b, missing))
    S = S[np.isfinite(S)]
    return dict(rtol=1e-12, atol=1e-14 * max(1.0, float(np.abs(S).max()) if S.size else 0.0))
