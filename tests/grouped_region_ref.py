"""
Exact posterior of the grouped-region model by enumeration (test-side reference; small N, H, U, G only).

Model: r_ng ~ Bernoulli(pi) once per region and GROUP of patients; f_c ~ Categorical(gamma); for every patient u
independently, with g = the patient's group, T_cu | r_ng, r_mg (both typical -> 0, both anomalous -> 1, discordant ->
Bernoulli(eta)), F~_cu | f_c, T_cu (keeps f_c w.p. 1-eps when T = 0 and eps when T = 1, else one of the other two types with
equal probability), b_ch ~ N(mu_f, sigma_f), bt_cu ~ N(mu_F~, sigma_F~).  As in shared_region_ref.py, T and F~ are summed
EXPLICITLY from these definitions per patient (not through M or lM), with r indexed by the patient's group, over every f in
3^C and r in 2^(N G).  Plain Normal densities, as the fitter's.  missing: a NaN b / bt has density 1.
"""
import itertools

import numpy as np

from shared_region_ref import _nlogpdf, _npdf, edges, p_ft, p_t1


def group_index(labels):
    """(names, group_of (U,) int64): the sorted unique labels and every patient's index into them."""
    names = sorted(set(labels))
    return names, np.array([names.index(v) for v in labels], dtype=np.int64)


def enumerate_posterior(b, bt, labels, theta, missing=False):
    """
    theta[12] = pi, eta, epsilon, gamma[3], mu[3], sigma[3]; labels: one per patient (column of bt).  Returns a dict:
      names, log_evidence, logjoint (3^C, 2^(N G)) over states (f in itertools.product order, r likewise, r[n, g] row-major),
      p_r (N, G), p_f (C, 3), p_T (C, U), p_Ft (C, U, 3), p_changed (C, U),
      p_group_count (G, N+1)  P(sum_n r_ng = k),  p_region_count (N, G+1)  P(sum_g r_ng = k),
      p_pair (G, G, N, 2, 2)  P(r_na = i, r_nb = j): the per-region joint of two groups.
    """
    th = np.asarray(theta, dtype=np.float64)
    pi, eta, eps = th[0], th[1], th[2]
    gamma, mu, sigma = th[3:6], th[6:9], th[9:12]
    (C, H) = b.shape
    U = bt.shape[1]
    (names, gof) = group_index(list(labels))
    assert len(gof) == U
    G = len(names)
    N = int(round((1 + np.sqrt(1 + 8 * C)) / 2))
    ends = edges(N)
    assert len(ends) == C
    lpb = np.stack([_nlogpdf(b, mu[k], sigma[k]) for k in range(3)], axis=2)          # (C,H,3)
    dens = np.stack([_npdf(bt, mu[j], sigma[j]) for j in range(3)], axis=2)            # (C,U,3)
    if missing:
        lpb[np.isnan(b)] = 0.0
        dens[np.isnan(bt)] = 1.0
    SB = lpb.sum(axis=1)                                                                # (C,3)
    # per (c, k, r_n, r_m): joint weights of (t, j) for every patient, summed explicitly
    wtj = np.zeros((C, 3, 2, 2, U, 2, 3))
    for c in range(C):
        for k in range(3):
            for rn in (0, 1):
                for rm in (0, 1):
                    pt1 = p_t1(rn, rm, eta)
                    for t in (0, 1):
                        pt = pt1 if t else 1.0 - pt1
                        for j in range(3):
                            wtj[c, k, rn, rm, :, t, j] = pt * p_ft(j, k, t, eps) * dens[c, :, j]
    lbt = np.log(wtj.sum(axis=(5, 6)))                                                  # (C,3,2,2,U)
    F = list(itertools.product(range(3), repeat=C))
    R = list(itertools.product((0, 1), repeat=N * G))
    Fa = np.array(F)
    Ra = np.array(R).reshape(len(R), N, G)
    lj = np.zeros((len(F), len(R)))
    us = np.arange(U)
    for ir in range(len(R)):
        r = Ra[ir]
        lr = np.where(r > 0, np.log(pi), np.log(1 - pi)).sum()
        per_edge = np.array([[np.log(gamma[k]) + SB[c, k] + lbt[c, k, r[n, gof], r[m, gof], us].sum() for k in range(3)]
                             for c, (n, m) in enumerate(ends)])                          # (C,3)
        lj[:, ir] = lr + per_edge[np.arange(C)[None, :], Fa].sum(axis=1)
    mx = lj.max()
    log_ev = mx + np.log(np.exp(lj - mx).sum())
    P = np.exp(lj - log_ev)
    Pr = P.sum(axis=0)                                                                  # (2^(N G),)
    p_r = (Pr[:, None, None] * Ra).sum(axis=0)
    pf_marg = P.sum(axis=1)
    p_f = np.stack([(pf_marg[:, None] * (Fa == k)).sum(axis=0) for k in range(3)], axis=1)
    p_group_count = np.stack([np.bincount(Ra[:, :, g].sum(axis=1), weights=Pr, minlength=N + 1) for g in range(G)], axis=0)
    p_region_count = np.stack([np.bincount(Ra[:, n, :].sum(axis=1), weights=Pr, minlength=G + 1) for n in range(N)], axis=0)
    p_pair = np.zeros((G, G, N, 2, 2))
    for a in range(G):
        for bb in range(G):
            for n in range(N):
                for i in (0, 1):
                    for j in (0, 1):
                        p_pair[a, bb, n, i, j] = Pr[(Ra[:, n, a] == i) & (Ra[:, n, bb] == j)].sum()
    # connection posteriors: average the conditional law of (t, j) given (f_c, r_n, r_m, bt) with the patient's group's r
    cond = wtj / wtj.sum(axis=(5, 6), keepdims=True)                                    # (C,3,2,2,U,2,3)
    p_T = np.zeros((C, U))
    p_Ft = np.zeros((C, U, 3))
    p_ch = np.zeros((C, U))
    for c, (n, m) in enumerate(ends):
        for u in range(U):
            g = gof[u]
            for k in range(3):
                for rn in (0, 1):
                    for rm in (0, 1):
                        w = P[np.ix_(Fa[:, c] == k, (Ra[:, n, g] == rn) & (Ra[:, m, g] == rm))].sum()
                        q = cond[c, k, rn, rm, u]                                       # (2,3)
                        p_T[c, u] += w * q[1, :].sum()
                        p_Ft[c, u] += w * q.sum(axis=0)
                        p_ch[c, u] += w * (1.0 - q.sum(axis=0)[k])
    return dict(names=names, log_evidence=log_ev, logjoint=lj, p_r=p_r, p_f=p_f, p_T=p_T, p_Ft=p_Ft, p_changed=p_ch,
                p_group_count=p_group_count, p_region_count=p_region_count, p_pair=p_pair, states_f=Fa, states_r=Ra)
