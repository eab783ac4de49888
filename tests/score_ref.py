"""
NumPy restatement of scoring new patients (fcdiff_amd/score.py, fcd_score.hip): the per-patient split of the variational
energy terms, the exact predictive likelihood p(bt_u | f) and the posterior of r given f by enumerating r, and the
variational target sum_F q_F(F) log p(bt_u | F) by enumerating F.  Used by tests/test_score.py and tests/test_gpu_score.py.
"""
import itertools

import numpy as np

from oracle import fcdiff_oracle as O


def patient_elbo(lq_F, lq_R, lM, pi2):
    """
    (U, 4) {E_lM, E_lp_R, E_lq_R, elbo} per patient: the oracle's energy terms E_lM (fit.py:489-511), E_lp_R (:486) and
    E_lq_R (:539) evaluated on patient u's slice alone; elbo = E_lM + E_lp_R - E_lq_R.
    """
    lq_R = np.asarray(lq_R, dtype=np.float64)
    q_F = np.exp(np.asarray(lq_F, dtype=np.float64))
    q_R = np.exp(lq_R)
    U = lq_R.shape[1]
    out = np.zeros((U, 4))
    for u in range(U):
        sl = slice(u, u + 1)
        out[u, 0] = O.eval_E_lM(q_F, q_R[:, sl], lM[:, sl])
        out[u, 1] = O.eval_E_lp_R(q_R[:, sl], pi2)
        out[u, 2] = O.eval_E_lq_R(q_R[:, sl], lq_R[:, sl])
    out[:, 3] = out[:, 0] + out[:, 1] - out[:, 2]
    return out


def mix_case(rn, rm):
    """Mixture case of an edge from its endpoints' states: 0 both typical, 1 both anomalous, 2 discordant."""
    return 1 if (rn and rm) else (2 if rn != rm else 0)


def r_configs(Nreg):
    return [np.array(r, dtype=np.int64) for r in itertools.product((0, 1), repeat=Nreg)]


def log_joint_r(lM_u, f, r, pi):
    """log p(r; pi) + sum_c lM[c, f_c, l(r_n, r_m)] for one patient: lM_u (C, 3, 3), f (C,), r (Nreg,)."""
    C = lM_u.shape[0]
    e = float(np.sum(np.where(r == 1, np.log(pi), np.log1p(-pi))))
    for c in range(C):
        (n, m) = O.c_to_nm(c)
        e += lM_u[c, int(f[c]), mix_case(r[n], r[m])]
    return e


def _logsumexp(a):
    a = np.asarray(a, dtype=np.float64)
    mx = np.max(a)
    if not np.isfinite(mx):
        return mx
    return float(mx + np.log(np.sum(np.exp(a - mx))))


def exact_log_pred(lM_u, f, pi):
    """log p(bt_u | f) = log sum_r p(r; pi) prod_c exp lM[c, f_c, l(r_n, r_m)], all 2^Nreg configurations of r."""
    C = lM_u.shape[0]
    Nreg = int(O.C_to_N(C))
    return _logsumexp([log_joint_r(lM_u, f, r, pi) for r in r_configs(Nreg)])


def exact_p_r(lM_u, f, pi):
    """(Nreg,) P(r_n = 1 | f, bt_u) by enumeration."""
    C = lM_u.shape[0]
    Nreg = int(O.C_to_N(C))
    rs = r_configs(Nreg)
    lj = np.array([log_joint_r(lM_u, f, r, pi) for r in rs])
    p = np.exp(lj - np.max(lj))
    p /= p.sum()
    return np.sum(p[:, None] * np.stack(rs), axis=0)


def expected_log_pred_qF(lq_F, lM_u, pi):
    """sum_F q_F(F) log p(bt_u | F), q_F(F) = prod_c q_F[c, F_c]: every one of the 3^C templates (small C only)."""
    q_F = np.exp(np.asarray(lq_F, dtype=np.float64))[:, 0, :]
    C = q_F.shape[0]
    tot = 0.0
    for F in itertools.product(range(3), repeat=C):
        w = float(np.prod([q_F[c, F[c]] for c in range(C)]))
        if w > 0.0:
            tot += w * exact_log_pred(lM_u, np.array(F), pi)
    return tot


def ais_parts(w):
    """(U, 4) {max, sum exp(w - max), sum exp(2 (w - max)), G} of weights w (G, U): fcd_score_ais_finish's numbers."""
    w = np.asarray(w, dtype=np.float64)
    mx = np.max(w, axis=0)
    e = np.exp(w - mx[None, :])
    return np.stack([mx, e.sum(axis=0), (e * e).sum(axis=0), np.full(w.shape[1], float(w.shape[0]))], axis=1)
