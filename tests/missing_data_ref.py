"""
What an unobserved b or bt means under the fitter's model, for the tests of `missing_data = True`.
TEST INFRASTRUCTURE ONLY: the product code does not import it.

The fitter's densities of b and bt are plain Normals (no clip to [-1, 1]), so integrating an unobserved value out is
integrating a density to 1:
    b[c,h] missing   ->  ln N(b; mu_k, sigma_k) is replaced by ln 1 = 0 in S_B[c,k]
    bt[c,u] missing  ->  N_j = 1 for every j, so M_kl = sum_j P(F~ = j | k, l) = 1 and lM[c,u,k,l] = 0
Given f = k and the mixture case l, the generative model draws T ~ Bernoulli(pT_l), pT = (0, 1, eta), then F~ = k with
probability 1 - epsilon (T = 0) or epsilon (T = 1), else one of the other two types with equal probability.
"""
import itertools

import numpy as np

from oracle import fcdiff_oracle as O


def enumerate_law(eta, epsilon, like=(1.0, 1.0, 1.0)):
    """
    Explicit enumeration of (T, F~) given (k, l), weighted by the likelihood like[F~] of bt:
    M (3k, 3l), P(T = 1 | k, l, bt) (3k, 3l), P(F~ = j | k, l, bt) (3k, 3l, 3j), P(F~ != k | k, l, bt) (3k, 3l).
    """
    pT = (0.0, 1.0, eta)
    M = np.zeros((3, 3))
    t1 = np.zeros((3, 3))
    fj = np.zeros((3, 3, 3))
    for (k, l, t, j) in itertools.product(range(3), range(3), range(2), range(3)):
        p_t = pT[l] if t == 1 else 1.0 - pT[l]
        keep = epsilon if t == 1 else 1.0 - epsilon
        p_j = keep if j == k else (1.0 - keep) / 2.0
        w = p_t * p_j * like[j]
        M[k, l] += w
        t1[k, l] += w * t
        fj[k, l, j] += w
    pT1 = t1 / M
    pF = fj / M[:, :, None]
    pch = np.stack([pF[k, :, [j for j in range(3) if j != k]].sum(axis=0) for k in range(3)])
    return M, pT1, pF, pch


def prior_law(theta):
    """(pT (3k,3l), pF (3k,3l,3j), pch (3k,3l)): the law of T and F~ given (k, l) when bt is unobserved."""
    theta = np.asarray(theta, dtype=np.float64)
    (_M, pT, pF, pch) = enumerate_law(theta[1], theta[2])
    return pT, pF, pch


def contract_prior(W, theta):
    """{p_T, p_F_tilde, p_changed} of the prior law averaged over weights W (..., 3, 3), normalised per item."""
    (pT, pF, pch) = prior_law(theta)
    W = np.asarray(W, dtype=np.float64)
    tot = W.sum(axis=(-2, -1))
    return {"p_T": np.einsum("...kl,kl->...", W, pT) / tot,
            "p_F_tilde": np.einsum("...kl,klj->...j", W, pF) / tot[..., None],
            "p_changed": np.einsum("...kl,kl->...", W, pch) / tot}


def masked_lik_tables(b, bt, mu, sigma, eta, epsilon):
    """
    The NumPy oracle's tables with the rule applied test-side: (S_B (C,3) as a nansum, lp_B_g_F (C,H,3) with 0 at a NaN
    b, p_Bt_g_Ft (C,U,3) with 1 at a NaN bt, lM (C,U,3,3) with 0 at a NaN bt).
    """
    with np.errstate(invalid="ignore", divide="ignore"):
        (lpB, pBt, lM) = O.lik_tables(b, bt, mu, sigma, eta, epsilon)
    S_B = np.nansum(lpB, axis=1)
    lpB = np.where(np.isnan(b)[:, :, None], 0.0, lpB)
    pBt = np.where(np.isnan(bt)[:, :, None], 1.0, pBt)
    lM = np.where(np.isnan(bt)[:, :, None, None], 0.0, lM)
    return S_B, lpB, pBt, lM
