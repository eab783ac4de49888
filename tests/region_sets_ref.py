"""
NumPy restatement of the region-set counts (fcd_region_sets.hip): for sets S_j of regions the histograms over chains of
sum_{n in S_j} r_nu and of the number of patients with an anomalous region in S_j, and the mean-field law of both under
q_R (Poisson-binomial, on count_posterior_ref.poisson_binomial).  Used by tests/test_region_sets.py and
tests/test_gpu_region_sets.py.
"""
import numpy as np

import count_posterior_ref as R


def histograms(r, sets):
    """
    r (G, Nreg, U) of 0 / 1, sets: a list of index sequences -> (hist_set (J, U, S_max+1), hist_prev (J, U+1)) int64:
    hist_set[j, u, k] = #{g : sum_{n in S_j} r[g, n, u] = k},  hist_prev[j, k] = #{g : #{u : some n in S_j has r[g, n, u] = 1} = k}.
    """
    r = np.asarray(r, dtype=np.int64)
    (_G, _N, U) = r.shape
    J = len(sets)
    s_max = max(len(s) for s in sets)
    hist_set = np.zeros((J, U, s_max + 1), dtype=np.int64)
    hist_prev = np.zeros((J, U + 1), dtype=np.int64)
    for (j, s) in enumerate(sets):
        per_patient = r[:, np.asarray(s, dtype=np.int64), :].sum(axis=1)            # (G, U)
        hist_set[j] = np.bincount((np.arange(U)[None, :] * (s_max + 1) + per_patient).reshape(-1),
                                  minlength=U * (s_max + 1)).reshape(U, s_max + 1)
        hist_prev[j] = np.bincount((per_patient > 0).sum(axis=1), minlength=U + 1)
    return hist_set, hist_prev


def independent_laws(lq_R, sets):
    """
    lq_R (Nreg, U, 2), sets -> (p_count (J, U, S_max+1), p_prevalence (J, U+1)) under independent sites: the count of set j
    in patient u is Poisson-binomial over the set's rows, the prevalence Poisson-binomial over u with
    p_u = 1 - prod_{n in S_j} (1 - q1[n, u]), taken as -expm1(sum log(1 - q1)) so that a small p_u keeps its digits.
    """
    (q0, q1) = R.q_of(lq_R)
    (_N, U) = q0.shape
    J = len(sets)
    s_max = max(len(s) for s in sets)
    p_count = np.zeros((J, U, s_max + 1))
    p_prev = np.zeros((J, U + 1))
    with np.errstate(divide="ignore"):
        l0 = np.where(q1 < 0.5, np.log1p(-q1), np.log(q0))
    for (j, s) in enumerate(sets):
        s = np.asarray(s, dtype=np.int64)
        for u in range(U):
            p_count[j, u, :len(s) + 1] = R.poisson_binomial(q0[s, u], q1[s, u])
        none = l0[s].sum(axis=0)                     # log P(no region of the set is anomalous in u)
        p_u = -np.expm1(none)
        p_prev[j] = R.poisson_binomial(1.0 - p_u, p_u)
    return p_count, p_prev
