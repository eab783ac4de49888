"""
NumPy restatement of the patient-group counts (fcd_patient_groups.hip): for groups g_j of patients and rows rho (the regions,
then the region sets with the indicator "patient u has an anomalous region in S") the histograms over chains of
k_j = #{u in g_j : the row's indicator is 1}, per contrast (a, b) the joint histograms of (k_a, k_b), the mean-field law of
both under q_R (Poisson-binomial, on count_posterior_ref.poisson_binomial), and the derived quantities of
patient_group_posterior() from a joint table, in exact rational arithmetic on the rates.  Used by
tests/test_patient_groups.py and tests/test_gpu_patient_groups.py.
"""
from fractions import Fraction

import numpy as np

import count_posterior_ref as R


def row_indicators(r, sets=None):
    """r (G, Nreg, U) of 0 / 1 -> (G, R, U) int64: the regions' rows, then one row per set, 1 where some member is 1."""
    r = np.asarray(r, dtype=np.int64)
    if not sets:
        return r
    hit = [(r[:, np.asarray(s, dtype=np.int64), :].sum(axis=1) > 0).astype(np.int64) for s in sets]
    return np.concatenate([r, np.stack(hit, axis=1)], axis=1)


def histograms(r, groups, contrasts, sets=None):
    """
    r (G, Nreg, U), groups: a list of index sequences, contrasts: a list of pairs of group indices ->
    (hist_group (J, R, Umax+1) int64, [hist_joint_p (R, |a|+1, |b|+1) int64 for every contrast]):
    hist_group[j, rho, k] = #{g : k_j(g, rho) = k},  hist_joint_p[rho, i, l] = #{g : k_a(g, rho) = i and k_b(g, rho) = l}.
    """
    x = row_indicators(r, sets)
    (_G, rows, _U) = x.shape
    umax = max(len(g) for g in groups)
    k = [x[:, :, np.asarray(g, dtype=np.int64)].sum(axis=2) for g in groups]                 # each (G, R)
    hist_group = np.zeros((len(groups), rows, umax + 1), dtype=np.int64)
    for (j, kj) in enumerate(k):
        hist_group[j] = np.bincount((np.arange(rows)[None, :] * (umax + 1) + kj).reshape(-1),
                                    minlength=rows * (umax + 1)).reshape(rows, umax + 1)
    joints = []
    for (a, b) in contrasts:
        (na, nb) = (len(groups[a]) + 1, len(groups[b]) + 1)
        cell = (np.arange(rows)[None, :] * na + k[a]) * nb + k[b]
        joints.append(np.bincount(cell.reshape(-1), minlength=rows * na * nb).reshape(rows, na, nb))
    return hist_group, joints


def flat_joint(joints):
    """The per-contrast joint histograms as the flat buffer of include/fcdiff_hip.h (one placeholder word without contrasts)."""
    return np.concatenate([j.reshape(-1) for j in joints]) if joints else np.zeros(1, dtype=np.int64)


def split_joint(flat, groups, contrasts, rows):
    """The inverse of flat_joint() for a device buffer."""
    (out, at) = ([], 0)
    for (a, b) in contrasts:
        (na, nb) = (len(groups[a]) + 1, len(groups[b]) + 1)
        out.append(np.asarray(flat[at:at + rows * na * nb]).reshape(rows, na, nb))
        at += rows * na * nb
    return out


def independent_laws(lq_R, groups, contrasts, sets=None):
    """
    lq_R (Nreg, U, 2) -> (p_count (J, R, Umax+1), [p_joint_p (R, |a|+1, |b|+1)]) under independent sites: k_j at a region row is
    Poisson-binomial over the group's columns of q1, at a set row with p_u = 1 - prod_{n in S} (1 - q1[n, u]) (taken as
    -expm1(sum log(1 - q1))); the joint of a contrast of disjoint groups is the outer product of its marginals.
    """
    (q0, q1) = R.q_of(lq_R)
    if sets:
        with np.errstate(divide="ignore"):
            l0 = np.where(q1 < 0.5, np.log1p(-q1), np.log(q0))
        none = np.stack([l0[np.asarray(s, dtype=np.int64)].sum(axis=0) for s in sets])       # (J_S, U)
        q0 = np.concatenate([q0, np.exp(none)], axis=0)
        q1 = np.concatenate([q1, -np.expm1(none)], axis=0)
    rows = q0.shape[0]
    umax = max(len(g) for g in groups)
    p_count = np.zeros((len(groups), rows, umax + 1))
    for (j, g) in enumerate(groups):
        g = np.asarray(g, dtype=np.int64)
        for rho in range(rows):
            p_count[j, rho, :len(g) + 1] = R.poisson_binomial(q0[rho, g], q1[rho, g])
    joints = [p_count[a, :, :len(groups[a]) + 1, None] * p_count[b, :, None, :len(groups[b]) + 1] for (a, b) in contrasts]
    return p_count, joints


def summaries(p_count, p_joint, sizes, contrasts, level=0.95):
    """
    The derived quantities from the laws, cell by cell: prevalence (J, R); per contrast p_greater, p_less, p_equal, diff_mean
    (P, R) and diff_interval (P, R, 2).  The rates k_a/|a| and k_b/|b| are compared as Fractions; the interval's ends are the
    smallest differences whose cumulative probability reaches (1 - level)/2 and (1 + level)/2 (to within 1e-12).
    """
    p_count = np.asarray(p_count, dtype=np.float64)
    (J, rows, _K) = p_count.shape
    out = {"prevalence": np.zeros((J, rows))}
    for j in range(J):
        for rho in range(rows):
            out["prevalence"][j, rho] = sum(k * p_count[j, rho, k] for k in range(sizes[j] + 1)) / sizes[j]
    P = len(contrasts)
    for key in ("p_greater", "p_less", "p_equal", "diff_mean"):
        out[key] = np.zeros((P, rows))
    out["diff_interval"] = np.zeros((P, rows, 2))
    for (p, (a, b)) in enumerate(contrasts):
        (na, nb) = (int(sizes[a]), int(sizes[b]))
        cells = sorted((Fraction(i, na) - Fraction(l, nb), i, l) for i in range(na + 1) for l in range(nb + 1))
        for rho in range(rows):
            pj = p_joint[p][rho]
            for (d, i, l) in cells:
                key = "p_greater" if d > 0 else ("p_less" if d < 0 else "p_equal")
                out[key][p, rho] += pj[i, l]
                out["diff_mean"][p, rho] += float(d) * pj[i, l]
            for (side, q) in enumerate(((1.0 - level) / 2.0, (1.0 + level) / 2.0)):
                (cum, end) = (0.0, float(cells[-1][0]))
                for (d, i, l) in cells:
                    cum += pj[i, l]
                    if cum >= q - 1e-12:
                        end = float(d)
                        break
                out["diff_interval"][p, rho, side] = end
    return out
