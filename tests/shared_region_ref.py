"""
Exact posterior of the shared-region model by enumeration (test-side reference; small N, H, U only).

Model: r_n ~ Bernoulli(pi) once per region; f_c ~ Categorical(gamma); for every patient u independently
T_cu | r_n, r_m (both typical -> 0, both anomalous -> 1, discordant -> Bernoulli(eta)), F~_cu | f_c, T_cu (keeps f_c
w.p. 1-eps when T = 0 and eps when T = 1, else one of the other two types with equal probability), b_ch ~ N(mu_f, sigma_f),
bt_cu ~ N(mu_F~, sigma_F~).  Here T and F~ are summed EXPLICITLY from these definitions (not through M or lM), over
every f in 3^C and r in 2^N.  Plain Normal densities, as the fitter's.  missing: a NaN b / bt has density 1.
"""
import itertools

import numpy as np


def _npdf(x, mu, sigma):
    return np.exp(-((x - mu) / sigma) ** 2 / 2.0) / np.sqrt(2 * np.pi) / sigma


def _nlogpdf(x, mu, sigma):
    return -((x - mu) / sigma) ** 2 / 2.0 - np.log(np.sqrt(2 * np.pi)) - np.log(sigma)


def edges(N):
    """(n, m) of every edge in the fitter's order c = n(n-1)/2 + m, n > m."""
    return [(n, m) for n in range(1, N) for m in range(n)]


def p_t1(rn, rm, eta):
    if rn and rm:
        return 1.0
    if not rn and not rm:
        return 0.0
    return eta


def p_ft(j, k, t, eps):
    keep = eps if t else 1.0 - eps
    return keep if j == k else (1.0 - keep) * 0.5


def enumerate_posterior(b, bt, theta, missing=False):
    """
    theta[12] = pi, eta, epsilon, gamma[3], mu[3], sigma[3].  Returns a dict:
      log_evidence, logjoint (3^C, 2^N) over states (f in itertools.product order, r likewise),
      p_r (N,), p_f (C,3), p_T (C,U), p_Ft (C,U,3), p_changed (C,U), p_count (N+1,).
    """
    th = np.asarray(theta, dtype=np.float64)
    pi, eta, eps = th[0], th[1], th[2]
    gamma, mu, sigma = th[3:6], th[6:9], th[9:12]
    (C, H) = b.shape
    U = bt.shape[1]
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
    R = list(itertools.product((0, 1), repeat=N))
    lj = np.zeros((len(F), len(R)))
    for ir, r in enumerate(R):
        lr = sum(np.log(pi) if x else np.log(1 - pi) for x in r)
        per_edge = np.array([[np.log(gamma[k]) + SB[c, k] + lbt[c, k, r[n], r[m]].sum() for k in range(3)]
                             for c, (n, m) in enumerate(ends)])                          # (C,3)
        for i_f, f in enumerate(F):
            lj[i_f, ir] = lr + per_edge[np.arange(C), f].sum()
    mx = lj.max()
    log_ev = mx + np.log(np.exp(lj - mx).sum())
    P = np.exp(lj - log_ev)
    Fa, Ra = np.array(F), np.array(R)
    p_r = (P.sum(axis=0)[:, None] * Ra).sum(axis=0)
    pf_marg = P.sum(axis=1)
    p_f = np.stack([(pf_marg[:, None] * (Fa == k)).sum(axis=0) for k in range(3)], axis=1)
    p_count = np.bincount(Ra.sum(axis=1), weights=P.sum(axis=0), minlength=N + 1)
    # connection posteriors: average the conditional law of (t, j) given (f_c, r_n, r_m, bt)
    cond = wtj / wtj.sum(axis=(5, 6), keepdims=True)                                    # (C,3,2,2,U,2,3)
    p_T = np.zeros((C, U))
    p_Ft = np.zeros((C, U, 3))
    p_ch = np.zeros((C, U))
    for c, (n, m) in enumerate(ends):
        for k in range(3):
            for rn in (0, 1):
                for rm in (0, 1):
                    w = P[np.ix_(Fa[:, c] == k, (Ra[:, n] == rn) & (Ra[:, m] == rm))].sum()
                    q = cond[c, k, rn, rm]                                              # (U,2,3)
                    p_T[c] += w * q[:, 1, :].sum(axis=1)
                    p_Ft[c] += w * q.sum(axis=1)
                    p_ch[c] += w * (1.0 - q.sum(axis=1)[:, k])
    return dict(log_evidence=log_ev, logjoint=lj, p_r=p_r, p_f=p_f, p_T=p_T, p_Ft=p_Ft, p_changed=p_ch, p_count=p_count,
                states_f=Fa, states_r=Ra)


def collapsed_logjoint(S_B, L, theta, N):
    """ln p(b, bt, f, r) over the same states from S_B (C,3) and L (C,3,3) (the unshared model at one patient)."""
    th = np.asarray(theta, dtype=np.float64)
    pi, gamma = th[0], th[3:6]
    C = S_B.shape[0]
    ends = edges(N)
    F = np.array(list(itertools.product(range(3), repeat=C)))
    R = np.array(list(itertools.product((0, 1), repeat=N)))
    lj = np.zeros((len(F), len(R)))
    for ir, r in enumerate(R):
        lr = np.where(r > 0, np.log(pi), np.log(1 - pi)).sum()
        lcase = np.array([0 if (r[n] == 0 and r[m] == 0) else (1 if (r[n] and r[m]) else 2) for (n, m) in ends])
        per_edge = np.log(gamma)[None, :] + S_B + L[np.arange(C), :, lcase]              # (C,3)
        lj[:, ir] = lr + per_edge[np.arange(C)[None, :], F].sum(axis=1)
    return lj
