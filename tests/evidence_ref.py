"""
NumPy reference of the model evidence (fcdiff_amd/evidence.py), and the stand-in engine that lets the CPU tests drive the
annealing loop over the C oracle.  TEST INFRASTRUCTURE ONLY.

chain_energy is written from the formula

    E(f, r) = sum_c S_B[c, f_c] + sum_{c,u} lM[c, u, f_c, l(r_nu, r_mu)],   (n, m) the endpoints of c = n (n - 1) / 2 + m,
    l = 0 both typical, 1 both anomalous, 2 discordant,

independently of the oracle's conditionals and of oracle/exact_chain.py; exact_log_evidence is the logsumexp of the
enumerated joint of oracle/exact_chain.py (which includes the priors of f and r).
"""
import numpy as np

from oracle.exact_chain import ExactChain


def endpoints(Nreg):
    """(n (C,), m (C,)) with c = n (n - 1) / 2 + m, n > m."""
    (n, m) = np.tril_indices(Nreg, -1)
    return n, m


def chain_energy(S_B, lM, f, r):
    """E (G,) float64 of chains f (G, C) in {0,1,2}, r (G, Nreg, U) in {0,1}."""
    S_B = np.asarray(S_B, dtype=np.float64)
    lM = np.asarray(lM, dtype=np.float64)
    f = np.asarray(f, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    (G, Nreg, U) = r.shape
    (C, U2) = lM.shape[0:2]
    assert U2 == U and f.shape == (G, C) and C == Nreg * (Nreg - 1) // 2
    (n, m) = endpoints(Nreg)
    rn = r[:, n, :]                         # (G, C, U)
    rm = r[:, m, :]
    l = np.where((rn == 1) & (rm == 1), 1, np.where(rn != rm, 2, 0))
    c = np.arange(C)[None, :, None]
    u = np.arange(U)[None, None, :]
    terms = lM[c, u, f[:, :, None], l]      # (G, C, U)
    return S_B[np.arange(C)[None, :], f].sum(axis=1) + terms.reshape(G, -1).sum(axis=1)


def chain_energy_abs(S_B, lM, f, r):
    """sum of |terms| of chain_energy: the scale of its rounding error."""
    return chain_energy(np.abs(S_B), np.abs(lM), f, r)


def logsumexp(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    m = np.max(a)
    return float(m + np.log(np.sum(np.exp(a - m))))


def exact_log_evidence(S_B, lM, gamma, pi2):
    """log sum_{f,r} of the enumerated joint (small models only)."""
    return logsumexp(ExactChain(S_B, lM, gamma, pi2).L)


def exact_log_evidence_shared(S_B, lM, gamma, pi2):
    """The shared-region model: the unshared one at U = 1 on the patient-summed table."""
    return exact_log_evidence(S_B, np.asarray(lM).sum(axis=1, keepdims=True), gamma, pi2)


class OracleEngine(object):
    """The engine surface of evidence.anneal (temper, sweep, energy_step, host) over the C oracle's f and r steps."""

    def __init__(self, S_B, lM, gamma, pi2, G, seed, chain0=0):
        from oracle import fcdiff_oracle as O
        self.S_B = np.ascontiguousarray(S_B, dtype=np.float64)
        self.lM = np.ascontiguousarray(lM, dtype=np.float64)
        (C, U) = self.lM.shape[0:2]
        Nreg = int(round(O.C_to_N(C)))
        (self.lng, self.lnpi2) = (np.log(np.asarray(gamma, dtype=np.float64)), np.log(np.asarray(pi2, dtype=np.float64)))
        (self.seed, self.chain0, self.mode) = (int(seed), int(chain0), O.EDGE_SYMMETRIC)
        self.f = np.zeros((G, C), dtype=np.uint8)
        self.r = np.zeros((G, Nreg, U), dtype=np.uint8)
        self.w = np.zeros(G)
        (self.S_Bw, self.lMw) = (np.zeros_like(self.S_B), np.zeros_like(self.lM))

    def temper(self, beta):
        if beta == 0.0:
            (self.S_Bw, self.lMw) = (np.zeros_like(self.S_B), np.zeros_like(self.lM))
        else:
            (self.S_Bw, self.lMw) = (beta * self.S_B, beta * self.lM)

    def sweep(self, number):
        from oracle import c_oracle as CO
        CO.gibbs_f_step(self.f, self.r, self.S_Bw, self.lMw, self.lng, self.seed, number, self.chain0)
        CO.gibbs_r_step(self.f, self.r, self.lMw, self.lnpi2, self.seed, number, self.mode, self.chain0)

    def energy_step(self, beta_prev, beta):
        self.w += (beta - beta_prev) * chain_energy(self.S_B, self.lM, self.f, self.r)

    def host(self):
        return self.w
