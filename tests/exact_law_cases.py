"""
Models, seeds and the verdict shared by tests/test_exact_law.py (C oracle) and tests/test_gpu_exact_law.py (kernels):
the sampler's chains after k sweeps against the exact law P_k of oracle/exact_chain.py.

Every case is deterministic (fixed data, Philox seed and chain ids), and the C oracle is bit-exact with the kernels, so
the outcome on the GPU is the outcome measured with the C oracle.
"""
import math

import numpy as np

from oracle import fcdiff_oracle as O
from oracle.exact_chain import ExactChain, g_test, histogram, marginal_tests

G_CHAINS = 1 << 18          # 4 096 chain words
SWEEPS = (1, 2, 3, 6)
PI0 = 0.3                   # gibbs_init's pi (the model's own pi is also 0.3, its other parameters are not)
P_JOINT = 1e-6              # joint G-test: fail below this p-value (only where states <= JOINT_MAX_STATES)
JOINT_MAX_STATES = 11664
Z_MAX = 5.5                 # marginal cells: fail where the two-sided tail is below that of |z| > 5.5, i.e. P_CELL
P_CELL = math.erfc(Z_MAX / math.sqrt(2.0))     # 3.8e-8 per cell: Bonferroni over <= 226 cells x 4 sweeps leaves 3.4e-5

# name: (Nreg, U, data)
CASES = {
    "3x1": (3, 1, "broad"),
    "3x2": (3, 2, "broad"),
    "4x1": (4, 1, "broad"),
    "4x2": (4, 2, "broad"),
    "3x2-strong": (3, 2, "strong"),
}


def model(data):
    """broad: H = 2 subjects, sigma 0.2-0.3 (every edge type keeps posterior mass, lead 1.3-3.7 nats), epsilon small enough
    that neighbouring r sites are coupled (the scan order shows); strong: sigma 0.05 and types 0.5 apart (the leading type
    of every edge is ahead by far more than e^15: the exponential-free f draw)."""
    from fcdiff_amd.model import UnsharedRegionModel
    m = UnsharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.3, 0.02
    m.gamma = np.array([0.3, 0.4, 0.3])
    if data == "strong":
        m.mu, m.sigma = np.array([-0.5, 0.0, 0.5]), np.array([0.05, 0.05, 0.05])
    else:
        m.mu, m.sigma = np.array([-0.3, 0.0, 0.3]), np.array([0.2, 0.25, 0.3])
    return m


def problem(name):
    """(Nreg, U, S_B, lM, gamma, pi2, seed) of one case; tables by the NumPy oracle (pinned to the reference by G2)."""
    (N, U, data) = CASES[name]
    m = model(data)
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 2, U, seed=10 * N + U)
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    return N, U, O.sum_lp_B(lpB), lM, np.asarray(m.gamma, dtype=np.float64), m.pi2(), 1234 + 10 * N + U


def exact(name, **kw):
    (N, U, S_B, lM, gamma, pi2, _seed) = problem(name)
    return ExactChain(S_B, lM, gamma, pi2, **kw)


def failures(ec, hists, laws):
    """Every reason to reject `laws` ({k: P_k}) given the chains' histograms ({k: counts}); empty = accepted."""
    out = []
    for k in sorted(hists):
        if ec.n_states <= JOINT_MAX_STATES:
            (G2, dof, p) = g_test(hists[k], laws[k])
            if p < P_JOINT:
                out.append("k=%d joint G=%.1f dof=%d p=%.2e" % (k, G2, dof, p))
        (names, z, p) = marginal_tests(ec, hists[k], laws[k])
        bad = np.flatnonzero(p < P_CELL)
        if bad.size:
            j = bad[np.argmin(p[bad])]
            out.append("k=%d %d marginal cells with p < %.1e, worst %s z=%.2f p=%.1e" % (k, bad.size, P_CELL, names[j], z[j],
                                                                                       p[j]))
    return out


def oracle_histograms(name, G=G_CHAINS):
    """Histograms of the C oracle's chains after every k of SWEEPS (and the final state)."""
    from oracle import c_oracle as CO
    (N, U, S_B, lM, gamma, pi2, seed) = problem(name)
    ec = ExactChain(S_B, lM, gamma, pi2)
    (f, r) = CO.gibbs_init(G, N, U, PI0, seed)
    hists = {}
    for s in range(max(SWEEPS)):
        CO.gibbs_f_step(f, r, S_B, lM, np.log(gamma), seed, s)
        CO.gibbs_r_step(f, r, lM, np.log(pi2), seed, s, O.EDGE_SYMMETRIC)
        if s + 1 in SWEEPS:
            hists[s + 1] = histogram(ec, f, r)
    return ec, hists, (f, r)
