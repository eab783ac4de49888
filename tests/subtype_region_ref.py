"""
NumPy reference of the subtype-region model (latent patient subtypes, mean-field VB) and the exact evidence of tiny cases.
TEST INFRASTRUCTURE ONLY: the product code does not import it.

Model: GroupedRegionModel with the labels drawn -- rho ~ Dirichlet(alpha, ..., alpha), z_u ~ Categorical(rho), r_ng ~
Bernoulli(pi) per region and subtype, patient u reads column z_u.  Family q(f) q(r) q(z) q(rho), s[u, g] = q(z_u = g),
q(rho) = Dirichlet(alpha + n), n_g = sum_u s[u, g].  The expected collapsed log-likelihood is the unshared model's E_lM term
at G pseudo-patients with L[c, g] = sum_u s[u, g] lM[c, u], so the loop below runs the oracle's vectorised updates
(update_lq_F_vec, update_lq_R_vec with symmetric edge ids, update_pi, update_gamma, eval_energy) at extent G on L:
    L(s);  q_F;  q_R;  pi, gamma;  E[u, g] = sum_c sum_k q_F[c,k] sum_l w_l^g(c) lM[c,u,k,l];
    s[u, :] = softmax_g(E[u, g] + psi(alpha + n_g) - psi(G alpha + U))  (n of the s before the step);
    energy = eval_energy at L(s) - sum s (E ln rho - ln s) + KL(Dir(alpha + n) || Dir(alpha)),  0 ln 0 = 0.
"""
import itertools

import numpy as np
import scipy.special as sp

import grouped_region_ref as GR
import sessions_ref as SR
from oracle import fcdiff_oracle as O


def tables(b, bt, theta, missing=False):
    """(S_B (C, 3), lM (C, U, 3, 3)): the oracle's lik_tables for a plain bt (C, U), sessions_ref's for sessions or NaN."""
    if np.ndim(bt) == 3 or missing:
        bt3 = bt if np.ndim(bt) == 3 else np.asarray(bt)[:, :, None]
        return SR.lik_tables(b, bt3, theta["mu"], theta["sigma"], theta["eta"], theta["epsilon"], missing=missing)
    (lpB, _pBt, lM) = O.lik_tables(b, bt, theta["mu"], theta["sigma"], theta["eta"], theta["epsilon"])
    return O.sum_lp_B(lpB), lM


def default_init(U, G, seed, restart):
    """The fit's default start of restart i: z0 = default_rng(seed + i).permutation(U) % G, s = 0.1/G + 0.9 onehot(z0)."""
    z0 = np.random.default_rng(seed + restart).permutation(U) % G
    s = np.full((U, G), 0.1 / G)
    s[np.arange(U), z0] += 0.9
    return s


def weighted_table(lM, s):
    """L (C, G, 3, 3) = sum_u s[u, g] lM[c, u]; a weight that is exactly 0 adds nothing."""
    with np.errstate(invalid="ignore"):
        terms = np.where(s.T[None, :, :, None, None] == 0, 0.0, s.T[None, :, :, None, None] * lM[:, None, :, :, :])
    return terms.sum(axis=2)


def expected_loglik(lq_F, lq_R, lM):
    """E (U, G): sum_c sum_k q_F[c,k] sum_l w_l^g(c) lM[c,u,k,l], the mixture-case weights of subtype g at c's endpoints."""
    ep = O.edge_endpoints(lq_R.shape[0])
    (n, m) = (ep[:, 0], ep[:, 1])
    q_R = np.exp(lq_R)
    q_F = np.exp(lq_F)[:, 0, :]
    w = np.stack([q_R[n, :, 0] * q_R[m, :, 0], q_R[n, :, 1] * q_R[m, :, 1],
                  q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]], axis=2)          # (C, G, 3)
    return np.einsum("ck,cgl,cukl->ug", q_F, w, lM)


def E_ln_rho(n, alpha):
    return sp.digamma(alpha + n) - sp.digamma(len(n) * alpha + n.sum())


def softmax(a):
    a = a - a.max(axis=1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(axis=1, keepdims=True)


def z_rho_terms(s, alpha):
    """- sum s (E ln rho - ln s) + KL(Dir(alpha + n) || Dir(alpha)) with n = sum_u s, 0 ln 0 = 0."""
    (U, G) = s.shape
    n = s.sum(axis=0)
    el = E_ln_rho(n, alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(s > 0, s * np.log(s), 0.0).sum()
    kl = (sp.gammaln(G * alpha + n.sum()) - sp.gammaln(alpha + n).sum() - sp.gammaln(G * alpha) + G * sp.gammaln(alpha)
          + (n * el).sum())
    return -((s * el[None, :]).sum() - ent) + kl


def energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha):
    return O.eval_energy(lq_F, lq_R, S_B, weighted_table(lM, s), gamma, [1 - pi, pi]) + z_rho_terms(s, alpha)


def vb_fit(S_B, lM, s0, pi, gamma, alpha=1.0, iters=30, update_theta=True):
    """
    The loop of the module docstring from responsibilities s0 (U, G) on the tables (S_B, lM (C, U, 3, 3)), `iters`
    iterations, no convergence test.  Returns a dict: energy (iters + 1,), lq_F, lq_R, pi, gamma, resp, hist (per iteration
    (lq_F, lq_R, pi, gamma, resp)), and steps (iters, 5): the energy at the start of an iteration and after each of its
    four steps (q_F, q_R, pi and gamma, the responsibilities).
    """
    (C, U) = lM.shape[:2]
    G = s0.shape[1]
    N = int(O.C_to_N(C))
    s = np.array(s0, dtype=np.float64)
    gamma = np.array(gamma, dtype=np.float64)
    pi = float(pi)
    lq_R = np.full((N, G, 2), -np.log(2))
    lq_F = np.full((C, 1, 3), -np.log(3))
    energies = [energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha)]
    (hist, steps) = ([], [])
    for _ in range(iters):
        row = [energies[-1]]
        L = weighted_table(lM, s)
        lq_F = O.update_lq_F_vec(lq_R, S_B, L, gamma)
        row.append(energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha))
        lq_R = O.update_lq_R_vec(lq_R, lq_F, L, [1 - pi, pi], O.EDGE_SYMMETRIC)
        row.append(energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha))
        if update_theta:
            pi = float(O.update_pi(lq_R))
            gamma = O.update_gamma(lq_F)
        row.append(energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha))
        E = expected_loglik(lq_F, lq_R, lM)
        s = softmax(E + E_ln_rho(s.sum(axis=0), alpha)[None, :])
        energies.append(energy(lq_F, lq_R, S_B, lM, s, gamma, pi, alpha))
        row.append(energies[-1])
        steps.append(row)
        hist.append((lq_F.copy(), lq_R.copy(), pi, gamma.copy(), s.copy()))
    return dict(energy=np.array(energies), lq_F=lq_F, lq_R=lq_R, pi=pi, gamma=gamma, resp=s, hist=hist, steps=np.array(steps))


def renumbered(out):
    """The result with its subtypes by decreasing n_g (ties by index), as the fit leaves them: resp and lq_R permuted."""
    order = np.argsort(-out["resp"].sum(axis=0), kind="stable")
    new = dict(out)
    new["resp"] = out["resp"][:, order]
    new["lq_R"] = out["lq_R"][:, order]
    new["order"] = order
    return new


def log_p_z(z, G, alpha):
    """ln of the Dirichlet-multinomial probability of the labels z (U,) under rho ~ Dirichlet(alpha, ..., alpha)."""
    n = np.bincount(np.asarray(z), minlength=G).astype(np.float64)
    return float(sp.gammaln(G * alpha) - sp.gammaln(G * alpha + n.sum()) + (sp.gammaln(alpha + n) - sp.gammaln(alpha)).sum())


def exact_log_evidence(b, bt, G, theta12, alpha=1.0):
    """
    ln p(b, bt | theta) of a tiny case: logsumexp over the G^U label vectors z of ln p(z) + the grouped model's exact
    log evidence at those labels (grouped_region_ref.enumerate_posterior; a subtype nobody has sums out to 1).
    """
    U = bt.shape[1]
    terms = []
    for z in itertools.product(range(G), repeat=U):
        terms.append(log_p_z(z, G, alpha) + GR.enumerate_posterior(b, bt, list(z), theta12)["log_evidence"])
    terms = np.array(terms)
    return float(terms.max() + np.log(np.exp(terms - terms.max()).sum()))
