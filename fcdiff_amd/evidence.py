"""
Model evidence by annealed importance sampling (UnsharedRegionFit.log_evidence, inherited by SharedRegionFit): the host side.

Both region models have the same collapsed joint in terms of their tables (the shared model is the unshared one at U = 1 on
the patient-summed table L):

    log Z = log sum_{f,r} p(f; gamma) p(r; pi) exp(E(f, r)) = log p(b, bt | theta),
    E(f, r) = sum_c S_B[c, f_c] + sum_{c,u} lM[c, u, f_c, l(r_nu, r_mu)]        (symmetric edge ids).

For G chains and a ladder 0 = beta_0 < ... < beta_T = 1 (score.ais_schedule):
  1. working tables all zero, one sweep: the f pass then draws f ~ gamma and the r pass r ~ Bernoulli(pi), an exact draw from
     the prior (fcd_gibbs_init alone draws f uniformly);
  2. for t = 1 .. T:  w_g += (beta_t - beta_{t-1}) E_g at the current state (fcd_evidence_energy), working tables = beta_t x
     the base tables (fcd_evidence_temper, one launch), one sweep on them (fcd_gibbs_sweeps, sweep number t);
  3. log_evidence = log mean_g exp(w_g) (unbiased on the exp scale) with its delta-method standard error and ESS as
     score.pool_ais defines them, and lower = mean_g w_g with its standard error: E[w] <= log Z by Jensen, a stochastic lower
     bound that stays meaningful when the ESS collapses.
The loop (anneal) is written against four methods of an engine -- temper, sweep, energy_step, host -- so that the CPU tests
drive the very same loop with a stand-in over the C oracle.  Every device step is a kernel of libfcdiff_hip.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import util
from .score import ais_schedule, pool_ais, score_key, gather_rows

# The annealing sampler's Philox key: score_key of the seed with this constant mixed in, so that for one seed it differs from
# the fit's key (the seed itself) and from score()'s (score_key(seed)).  Sweeps are numbered 0 (the prior draw) to n_anneal.
EVIDENCE_SALT = 0xE71DE9CE5A17ED01
MAX_ANNEAL = (1 << 32) - 2
_MASK64 = (1 << 64) - 1


def evidence_key(seed):
    return score_key((int(seed) ^ EVIDENCE_SALT) & _MASK64)


def anneal(engine, betas):
    """
    The ladder on `engine` (temper(beta), sweep(number), energy_step(beta_prev, beta), host()); returns the chains'
    log-weights (G,) as a NumPy array.  betas[0] must be 0 and betas[-1] 1.
    """
    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim != 1 or betas.size < 2 or betas[0] != 0.0 or betas[-1] != 1.0 or np.any(np.diff(betas) <= 0):
        raise ValueError("the ladder must rise from 0 to 1")
    engine.temper(0.0)               # zero tables: the sweep is a draw from the prior
    engine.sweep(0)
    for t in range(1, betas.size):
        engine.energy_step(float(betas[t - 1]), float(betas[t]))
        engine.temper(float(betas[t]))
        engine.sweep(t)
    return np.asarray(engine.host(), dtype=np.float64)


def weight_parts(w):
    """(6,) of one rank's log-weights: {m = max w, sum exp(w - m), sum exp(2 (w - m)), n, mean w, sum (w - mean)^2}."""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    n = w.size
    m = np.max(w)
    with np.errstate(invalid="ignore"):
        e = np.exp(w - m) if np.isfinite(m) else np.zeros(n)
        mean = np.mean(w)
        m2 = np.sum((w - mean) ** 2)
    return np.array([m, e.sum(), (e * e).sum(), float(n), mean, m2])


def pool(parts, n_anneal):
    """
    parts (R, 6): weight_parts of every rank -> the result dict of log_evidence().  The first four columns pool as
    score.pool_ais pools them; mean and sum of squares combine rank by rank (Chan et al.), so the numbers are those of all
    chains at once.
    """
    parts = np.asarray(parts, dtype=np.float64).reshape(-1, 6)
    (le, se, ess) = pool_ais(parts[:, None, :4])
    (n, mean, m2) = (0.0, 0.0, 0.0)
    with np.errstate(invalid="ignore"):
        for (nb, mb, m2b) in parts[:, 3:6]:
            d = mb - mean
            tot = n + nb
            m2 = m2 + m2b + d * d * n * nb / tot
            mean = mean + d * nb / tot
            n = tot
        lower_se = float(np.sqrt(m2 / (n - 1.0) / n)) if n > 1 else float("nan")
    return {"log_evidence": float(le[0]), "log_evidence_se": float(se[0]), "ess": float(ess[0]), "lower": float(mean),
            "lower_se": lower_se, "n_chains": int(n), "n_anneal": int(n_anneal)}


class EvidenceEngine(object):
    """
    The device side of the ladder: base tables (S_B, lM and the two difference tables the sweep reads, built once -- they
    are linear in lM, so a rung scales them instead of rebuilding them), working copies a GibbsEngine sweeps on, and the
    log-weights.  S_B (C, 3) and lM (C, U, 3, 3) are float64 device tensors and are only read.
    """

    def __init__(self, ctx, S_B, lM, Nreg, U, n_chains, chain0, key, gamma, pi2):
        import torch
        from .gibbs import GibbsEngine
        self.ctx = ctx
        (self.Nreg, self.U, self.G) = (int(Nreg), int(U), int(n_chains))
        Cn = util.N_to_C(self.Nreg)
        dev = lM.device
        sym = _lib.EDGE_MODES["symmetric"]
        (self.S_B, self.lM) = (S_B.contiguous(), lM.contiguous())
        lMd = torch.empty((self.U, self.Nreg, self.Nreg, 3, 2), dtype=torch.float64, device=dev)
        lMf = torch.empty((Cn, self.U, 3, 2), dtype=torch.float64, device=dev)
        ctx.call("fcd_gibbs_region_tables", _lib.dptr(self.lM), self.Nreg, self.U, sym, _lib.dptr(lMd), _lib.stream_ptr())
        ctx.call("fcd_gibbs_edge_tables", _lib.dptr(self.lM), self.Nreg, self.U, _lib.dptr(lMf), _lib.stream_ptr())
        self.base = [self.S_B, self.lM, lMf, lMd]
        self.work = [torch.zeros_like(t) for t in self.base]
        eng = GibbsEngine(self.work[0], self.work[1], self.Nreg, self.U, self.G, chain0=chain0, seed=key,
                          edge_index="symmetric", ctx=ctx, region_major=False)
        (eng.lMf, eng.lMd) = (self.work[2], self.work[3])
        eng.set_hyper(np.asarray(gamma, dtype=np.float64).reshape(3), np.asarray(pi2, dtype=np.float64).reshape(2))
        self.eng = eng
        self.w = torch.zeros(self.G, dtype=torch.float64, device=dev)
        n = len(self.base)
        self._src = (_lib._p * n)(*[t.data_ptr() for t in self.base])
        self._dst = (_lib._p * n)(*[t.data_ptr() for t in self.work])
        self._n = (C.c_int64 * n)(*[t.numel() for t in self.base])

    def temper(self, beta):
        if beta == 0.0:
            for t in self.work:
                t.zero_()            # (never 0 * table: 0 * -inf is NaN)
            return
        self.ctx.call("fcd_evidence_temper", float(beta), len(self.base), self._src, self._dst, self._n, _lib.stream_ptr())

    def sweep(self, number):
        self.eng.sweeps(int(number), 1)

    def energy_step(self, beta_prev, beta):
        self.ctx.call("fcd_evidence_energy", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.eng.f_state),
                      _lib.dptr(self.eng.r_bits), self.Nreg, self.U, self.G, float(beta_prev), float(beta), _lib.dptr(self.w),
                      _lib.stream_ptr())

    def host(self):
        return self.eng.host(self.w)


def log_evidence(ctx, S_B, lM, Nreg, U, gamma, pi2, n_anneal, n_chains, chain0, key):
    """The estimate for tables (S_B, lM) on context `ctx`: this rank's chains annealed, every rank's sums pooled."""
    import torch
    engine = EvidenceEngine(ctx, S_B, lM, Nreg, U, n_chains, chain0, key, gamma, pi2)
    w = anneal(engine, ais_schedule(n_anneal))
    parts = gather_rows(torch.as_tensor(weight_parts(w), device=lM.device))
    return pool(parts, n_anneal)
