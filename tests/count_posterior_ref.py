"""
NumPy restatement of the anomalous-region counts (fcd_count.hip): the histograms over chains of sum_n r_nu and sum_u r_nu,
and their mean-field law under q_R (Poisson-binomial, the convolution recursion in the kernel's order of operations).
Used by tests/test_count_posterior.py and tests/test_gpu_count_posterior.py.
"""
import numpy as np


def histograms(r):
    """
    r (G, Nreg, U) of 0 / 1 -> (hist_patient (U, Nreg+1), hist_region (Nreg, U+1)) int64:
    hist_patient[u, k] = #{g : sum_n r[g, n, u] = k},  hist_region[n, k] = #{g : sum_u r[g, n, u] = k}.
    """
    r = np.asarray(r, dtype=np.int64)
    (_G, N, U) = r.shape
    per_patient = r.sum(axis=1)                     # (G, U)
    per_region = r.sum(axis=2)                      # (G, N)
    hp = np.bincount((np.arange(U)[None, :] * (N + 1) + per_patient).reshape(-1), minlength=U * (N + 1))
    hr = np.bincount((np.arange(N)[None, :] * (U + 1) + per_region).reshape(-1), minlength=N * (U + 1))
    return hp.reshape(U, N + 1), hr.reshape(N, U + 1)


def q_of(lq_R, dtype=np.float64):
    """(q0, q1) = (P(r = 0), P(r = 1)) from log-weights lq_R (..., 2), normalised in log space, computed in `dtype`."""
    lq_R = np.asarray(lq_R, dtype=dtype)
    (l0, l1) = (lq_R[..., 0], lq_R[..., 1])
    mx = np.maximum(l0, l1)
    (e0, e1) = (np.exp(l0 - mx), np.exp(l1 - mx))
    s = e0 + e1
    return e0 / s, e1 / s


def poisson_binomial(q0, q1, dtype=np.float64):
    """Law of the number of successes of independent sites with P(0) = q0[i], P(1) = q1[i]: (len + 1,) of `dtype`."""
    P = np.zeros(len(q0) + 1, dtype=dtype)
    P[0] = 1.0
    for (i, (a, b)) in enumerate(zip(q0, q1)):
        nxt = P[:i + 2] * a
        nxt[1:] = nxt[1:] + P[:i + 1] * b
        P[:i + 2] = nxt
    return P


def count_posterior(lq_R, dtype=np.float64):
    """lq_R (Nreg, U, 2) -> (p_patient (U, Nreg+1), p_region (Nreg, U+1)) under independent sites; the whole recursion runs in
    `dtype` (np.longdouble: a reference with more digits than the kernel's fp64)."""
    (q0, q1) = q_of(lq_R, dtype)
    (N, U) = q0.shape
    p_patient = np.stack([poisson_binomial(q0[:, u], q1[:, u], dtype) for u in range(U)])
    p_region = np.stack([poisson_binomial(q0[n, :], q1[n, :], dtype) for n in range(N)])
    return p_patient, p_region
