"""
NumPy reference of the sessions tables: bt (C, U, K), K scans of every patient, for the tests of test_sessions.py and
test_gpu_sessions.py.  TEST INFRASTRUCTURE ONLY: the product code does not import it.

F~_cu is the patient's latent state of the connection and its K sessions are conditionally independent measurements of it:
    P_j(c,u)  = prod_k N(bt[c,u,k]; mu_j, sigma_j)                (a NaN session contributes 1 when `missing`)
    M_kl(c,u) = e_l P_k + (1 - e_l)/2 sum_{j != k} P_j            (e_l = the oracle's eval_M_eps)
taken in log form, a_j = sum_k ln N_j (ascending k, one addition at a time), m = max_j a_j, lM = m + ln M_kl(exp(a - m)).
product_like() gives prod_k N_j itself, for the brute-force law of missing_data_ref.enumerate_law.
"""
import numpy as np

from oracle import fcdiff_oracle as O


def session_log_sums(bt, mu, sigma, missing=False):
    """(a (C, U, 3), n_observed (C, U)): a[..., j] = sum_k ln N(bt[..., k]; mu_j, sigma_j) in ascending k."""
    bt = np.asarray(bt, dtype=np.float64)
    assert bt.ndim == 3
    a = np.zeros(bt.shape[:2] + (3,))
    nan = np.isnan(bt)
    for k in range(bt.shape[2]):
        for j in range(3):
            with np.errstate(invalid="ignore"):
                l = O.norm_logpdf(bt[:, :, k], mu[j], sigma[j])
            if missing:
                l = np.where(nan[:, :, k], 0.0, l)
            a[:, :, j] = a[:, :, j] + l
    n_obs = (~nan).sum(axis=2) if missing else np.full(bt.shape[:2], bt.shape[2])
    return a, n_obs


def log_M(a, n_obs, eta, epsilon):
    """lM (C, U, 3, 3) = m + ln M_kl(exp(a - m)); 0 where no session was observed, -inf where m = -inf."""
    m = a.max(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.exp(a - m[:, :, None])
        lM = np.zeros(a.shape[:2] + (3, 3))
        for k in range(3):
            for l in range(3):
                lM[:, :, k, l] = m + np.log(O.eval_M(p, eta, epsilon, k, l))
    lM[np.isneginf(m)] = -np.inf
    lM[n_obs == 0] = 0.0
    return lM


def lik_tables(b, bt, mu, sigma, eta, epsilon, missing=False):
    """(S_B (C, 3), lM (C, U, 3, 3)) of b (C, H) and bt (C, U, K); missing: NaN of b or bt is unobserved."""
    with np.errstate(invalid="ignore"):
        lpB = np.stack([O.norm_logpdf(b, mu[k], sigma[k]) for k in range(3)], axis=2)
    S_B = np.nansum(lpB, axis=1) if missing else O.sum_lp_B(lpB)
    (a, n_obs) = session_log_sums(bt, mu, sigma, missing)
    return S_B, log_M(a, n_obs, eta, epsilon)


def max_abs_log_sum(bt, mu, sigma, missing=False):
    """max |sum_k ln N_j| over the case: the magnitude the session sum rounds in (the atol of the tests' tolerance rule)."""
    (a, _n) = session_log_sums(bt, mu, sigma, missing)
    a = a[np.isfinite(a)]
    return float(np.abs(a).max()) if a.size else 0.0


def tolerance(bt, mu, sigma, missing=False, scale=1.0):
    """rtol 1e-12 (the project's table tolerance), atol = 1e-14 max(1, max |sum_k ln N|) (times `scale`)."""
    return dict(rtol=1e-12, atol=1e-14 * max(1.0, max_abs_log_sum(bt, mu, sigma, missing)) * scale)


def product_like(x, mu, sigma, missing=False):
    """(3,) prod_k N(x_k; mu_j, sigma_j) of one item's sessions x (K,): the plain product (it underflows; small K only)."""
    out = np.ones(3)
    for xk in np.asarray(x, dtype=np.float64):
        if missing and np.isnan(xk):
            continue
        out = out * np.array([O.norm_pdf(xk, mu[j], sigma[j]) for j in range(3)])
    return out


def vb_fit(b, bt, theta, iters, mode, shared=False):
    """
    The NumPy oracle's VB iterations (fcdiff_oracle.vb_fit's loop, without the convergence test) on the sessions tables;
    shared: the shared-region model, the same loop at one patient on the patient-summed table.  theta as the oracle's dict.
    Returns dict(energy (iters + 1,), lq_F, lq_R, theta, S_B, lM).
    """
    (C, _H) = b.shape
    N = int(O.C_to_N(C))
    U = 1 if shared else bt.shape[1]
    th = dict(theta)
    lq_R = np.full((N, U, 2), -np.log(2))
    lq_F = np.full((C, 1, 3), -np.log(3))

    def tables():
        (S_B, lM) = lik_tables(b, bt, th["mu"], th["sigma"], th["eta"], th["epsilon"])
        return S_B, (lM.sum(axis=1, keepdims=True) if shared else lM)

    def pi2():
        return [1 - th["pi"], th["pi"]]
    (S_B, lM) = tables()
    energy = [O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2())]
    for _ in range(iters):
        lq_F = O.update_lq_F(lq_R, S_B, lM, th["gamma"])
        lq_R = O.update_lq_R(lq_R, lq_F, lM, pi2(), mode)
        th["pi"] = O.update_pi(lq_R)
        th["gamma"] = O.update_gamma(lq_F)
        (S_B, lM) = tables()
        energy.append(O.eval_energy(lq_F, lq_R, S_B, lM, th["gamma"], pi2()))
    return dict(energy=np.array(energy), lq_F=lq_F, lq_R=lq_R, theta=th, S_B=S_B, lM=lM)
