"""
NumPy restatement of the co-anomaly matrices (fcd_coanomaly.hip) on exported chain states r (G, Nreg, U) of 0 / 1: how
often two regions are anomalous together, how many anomalous regions two patients share, their mean-field (independent
sites) form from lq_R, and the exact second moments of an enumerable model.
Used by tests/test_coanomaly.py and tests/test_gpu_coanomaly.py.
"""
import numpy as np

from count_posterior_ref import q_of


def pair_counts(r):
    """
    r (G, Nreg, U) of 0 / 1 -> (region_pairs (Nreg, Nreg), patient_pairs (U, U)) int64:
    region_pairs[n, m] = #{(g, u): r[g,n,u] = r[g,m,u] = 1},  patient_pairs[u, v] = #{(g, n): r[g,n,u] = r[g,n,v] = 1}.
    (In float64 so that einsum contracts through BLAS: every count is an integer far below 2^53, so the sums are exact.)
    """
    r = np.asarray(r, dtype=np.float64)
    region = np.einsum("gnu,gmu->nm", r, r, optimize=True)
    patient = np.einsum("gnu,gnv->uv", r, r, optimize=True)
    return np.rint(region).astype(np.int64), np.rint(patient).astype(np.int64)


def independent_q(q1):
    """
    q1 (Nreg, U) = P(r_nu = 1) -> (region (Nreg, Nreg), patient (U, U)) float64 under independent sites:
    sum_u q_nu q_mu and sum_n q_nu q_nv off the diagonals, sum_u q_nu and sum_n q_nu on them (r^2 = r).
    """
    q1 = np.asarray(q1, dtype=np.float64)
    region = q1 @ q1.T
    patient = q1.T @ q1
    np.fill_diagonal(region, q1.sum(axis=1))
    np.fill_diagonal(patient, q1.sum(axis=0))
    return region, patient


def independent(lq_R):
    """independent_q with q1 from log-weights lq_R (Nreg, U, 2), normalised in log space."""
    return independent_q(q_of(lq_R)[1])


def posterior_from_counts(region_pairs, patient_pairs, states):
    """The four joint entries of coanomaly_posterior() from pair counts over `states` chain states."""
    rp = np.asarray(region_pairs, dtype=np.float64)
    pp = np.asarray(patient_pairs, dtype=np.float64)
    (N, U) = (rp.shape[0], pp.shape[0])
    return {"p_region_pair": rp / (float(states) * U), "expected_patients": rp / float(states),
            "p_patient_pair": pp / (float(states) * N), "expected_regions": pp / float(states)}


def exact_moments(ec):
    """
    From an ExactChain: (p_region_pair (N, N), p_patient_pair (U, U), marginals (N, U)) under its exact law pi:
    p_region_pair[n, m] = (1/U) sum_u P(r_nu = 1, r_mu = 1),  p_patient_pair[u, v] = (1/N) sum_n P(r_nu = 1, r_nv = 1).
    """
    pi = np.exp(ec.L - ec.L.max()).reshape(-1)
    pi /= pi.sum()
    (_f, r) = ec.all_states()
    r = r.astype(np.float64)                                   # (S, N, U)
    (_S, N, U) = r.shape
    region = np.einsum("s,snu,smu->nm", pi, r, r) / U
    patient = np.einsum("s,snu,snv->uv", pi, r, r) / N
    return region, patient, np.einsum("s,snu->nu", pi, r)


def independent_from_marginals(q1):
    """(p_region_pair, p_patient_pair) of independent sites with marginals q1 (N, U), on the scale of exact_moments."""
    (N, U) = np.shape(q1)
    (region, patient) = independent_q(q1)
    return region / U, patient / N
