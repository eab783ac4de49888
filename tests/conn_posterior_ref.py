"""
NumPy restatement of the connection-level posteriors (fcd_conn_posterior, fcd_gibbs_pair_tally) for the tests.
TEST INFRASTRUCTURE ONLY: the product code does not import it.

Given f_c = k, the mixture case l of (r_n, r_m) (0 both typical, 1 both anomalous, 2 discordant) and bt, with
N_j = Normal(bt; mu_j, sigma_j), e_l = _eval_M_eps(eta, epsilon, l), S_k = sum_{j != k} N_j:
    M_kl              = e_l N_k + (1 - e_l)/2 S_k
    P(T = 1 | k,l)    = pT_l (eps N_k + (1 - eps)/2 S_k) / M_kl,      pT = (0, 1, eta)
    P(F~ = j | k,l)   = (e_l if j == k else (1 - e_l)/2) N_j / M_kl
    P(F~ != F | k,l)  = (1 - e_l)/2 S_k / M_kl
The densities enter through ratios only and are taken relative to the largest of the three (exp(ln N_j - max)).
"""
import numpy as np


def eps_l(eta, epsilon):
    return np.array([1 - epsilon, epsilon, eta * epsilon + (1 - eta) * (1 - epsilon)])


def rel_densities(bt, mu, sigma):
    """(..., 3): N_j / max_j N_j at every bt."""
    bt = np.asarray(bt, dtype=np.float64)
    a = np.stack([-((bt - mu[j]) / sigma[j]) ** 2 / 2.0 - np.log(sigma[j]) for j in range(3)], axis=-1)
    return np.exp(a - a.max(axis=-1, keepdims=True))


def tables(bt, theta):
    """Closed forms at every bt: pT (..., 3k, 3l), pF (..., 3k, 3l, 3j), pch (..., 3k, 3l)."""
    theta = np.asarray(theta, dtype=np.float64)
    (eta, epsilon, mu, sigma) = (theta[1], theta[2], theta[6:9], theta[9:12])
    N = rel_densities(bt, mu, sigma)
    e = eps_l(eta, epsilon)
    pTl = np.array([0.0, 1.0, eta])
    shp = N.shape[:-1]
    pT = np.zeros(shp + (3, 3))
    pF = np.zeros(shp + (3, 3, 3))
    pch = np.zeros(shp + (3, 3))
    for k in range(3):
        (j1, j2) = [j for j in range(3) if j != k]
        S = N[..., j1] + N[..., j2]             # (not sum - N_k: that cancels where N_k dominates)
        for l in range(3):
            off = (1 - e[l]) * 0.5
            M = e[l] * N[..., k] + off * S
            pT[..., k, l] = pTl[l] * (epsilon * N[..., k] + (1 - epsilon) * 0.5 * S) / M
            pch[..., k, l] = off * S / M
            for j in range(3):
                pF[..., k, l, j] = (e[l] if j == k else off) * N[..., j] / M
    return pT, pF, pch


def contract(W, bt, theta):
    """{p_T, p_F_tilde, p_changed} for weights W (C, U, 3, 3) >= 0, normalised per (c, u)."""
    W = np.asarray(W, dtype=np.float64)
    (pT, pF, pch) = tables(bt, theta)
    tot = W.sum(axis=(2, 3))
    return {"p_T": np.einsum("cukl,cukl->cu", W, pT) / tot,
            "p_F_tilde": np.einsum("cukl,cuklj->cuj", W, pF) / tot[..., None],
            "p_changed": np.einsum("cukl,cukl->cu", W, pch) / tot}


def endpoints(Nreg):
    """(n, m) of every edge c = n(n-1)/2 + m, n > m (the fitter's lower-triangular order)."""
    (n, m) = np.tril_indices(Nreg, -1)
    return n, m


def vb_weights(lq_F, lq_R):
    """W[c,u,k,l] = q_F[c,k] w_l(c,u) with w of the TRUE endpoints of c (fit.py:382-406)."""
    q_F = np.exp(np.asarray(lq_F, dtype=np.float64))[:, 0, :]
    q_R = np.exp(np.asarray(lq_R, dtype=np.float64))
    (n, m) = endpoints(q_R.shape[0])
    w = np.stack([q_R[n, :, 0] * q_R[m, :, 0], q_R[n, :, 1] * q_R[m, :, 1],
                  q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]], axis=2)
    return q_F[:, None, :, None] * w[:, :, None, :]


def mix_cases(r):
    """(G, C, U) mixture case of every chain, edge and patient from r (G, Nreg, U)."""
    r = np.asarray(r).astype(bool)
    (n, m) = endpoints(r.shape[1])
    (rn, rm) = (r[:, n, :], r[:, m, :])
    return np.where(rn & rm, 1, np.where(rn != rm, 2, 0)).astype(np.uint8)


def pair_counts(f, r, chunk=512):
    """(C, U, 3, 3) int64: number of chains with f_c = k and mixture case l at (c, u) (chains f (G, C), r (G, Nreg, U))."""
    f = np.asarray(f)
    r = np.asarray(r).astype(bool)
    (G, C) = f.shape
    U = r.shape[2]
    (n, m) = endpoints(r.shape[1])
    out = np.zeros((C, U, 3, 3), dtype=np.int64)
    for c0 in range(0, C, chunk):
        sl = slice(c0, min(C, c0 + chunk))
        (rn, rm) = (r[:, n[sl], :], r[:, m[sl], :])
        L = [~(rn | rm), rn & rm, rn ^ rm]
        for k in range(3):
            fk = (f[:, sl] == k)[:, :, None]
            for l in range(3):
                out[sl, :, k, l] = np.count_nonzero(fk & L[l], axis=0)
    return out
