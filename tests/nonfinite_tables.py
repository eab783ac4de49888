"""
Table sets with -inf entries and zero gamma / pi for the sampler (tests/test_nonfinite_tables.py pins the builder on the CPU,
tests/test_gpu_nonfinite_tables.py runs the kernels on what it builds).

Every draw of the device kernels is the draw of the oracle's fp64 formulas from the ABSOLUTE log-weights: draw_f(a0, a1, a2, x),
draw_r(s0, s1, x).  The table kernels return lM = -inf where a density underflows, fcd_hyper_set writes ln 0 = -inf for a zero
gamma or pi, and the fast forms of the f pass work on log-odds against type 0: with a0 = -inf those are +inf or NaN.  The sets
made here put such values where the kernels' paths divide.  Inputs hold finite values and -inf only: never a NaN, never +inf.

Sources (the first part of a set's name):
  item          about 1 % of the (c, u) items, and the placement edges, have all nine entries -inf
  plant-all-l   chosen (c, u): lM[c, u, k, :] = -inf for k in one of the six proper non-empty subsets of {0, 1, 2} -- the edge's
                pattern holds whatever the state
  plant-one-l   the same subsets at ONE mixture case l: the chains of a wave differ in whether their logit is finite
  gamma0/1/2    finite tables, one gamma exactly 0, the other two 0.5
  pi0 / pi1     pi2 = (1, 0) / (0, 1), finite tables; pi0+item the first together with `item`
  from-data     b, bt and a model with epsilon = 0 (M[k, typical] = N_k exactly) and sigma_0 well below sigma_1,2: at a few
                outlying bt only N_0 underflows, lM[c, u, 0, 0] = -inf; through the oracle's lik_tables (the GPU test builds
                the same table with the library's kernel)
  firm          all nine entries -inf at one patient of each placement edge and nowhere else; on every edge without such an
                item S_B of type c % 3 is raised until the f pass's rule of decided edges (tests/f_sure_ref.py) decides the
                edge with FIRM_MARGIN nats in hand.  The tiles around the -inf edges are then on the decided-tile path while
                those edges -- their bounds are NaN -- stay open: the decided forms meet non-finite log-odds inside live tiles

Placement.  `item` and `plant-*` touch the edges PLACE: row 0 and row 15 of a full block of 16 regions, region 32 of
Nreg = 33 (the one-row last block), partners inside the block (the non-finite value is an in-block term of the r pass) and
in another block (it arrives through the panel value e).

Base tables are those of the "model" regime of boundary_probes.  S_B of the edges that carry a planted item (and of every
third edge of the gamma sets) is re-centred so that the finite log-weights of the first compared sweep have mean 0 over the
chains: the types that stay possible are then comparable, and a kernel that answers a constant cannot pass.

Each set carries the C oracle's state after one and after two sweeps and the oracle's conditionals BEFORE each compared draw
(cond_f[s] (G, C, 3), cond_r[s] (G, Nreg, U, 2), s = 0, 1).  Nothing in this module needs a GPU.
"""
import functools

import numpy as np

import boundary_probes as BP
import f_sure_ref as R
from oracle import c_oracle as CO

NINF = -np.inf
FIRM_MARGIN = 40.0                                                 # nats over 0 of the decided mode's comparisons of `firm` (the rule asks for 16)
SUBSETS = ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2))               # the six proper non-empty subsets of the types
PATTERNS = SUBSETS + ((0, 1, 2),)                                  # ... and all three: the seven patterns of -inf among (a0, a1, a2)
ONE_L = (0, 2, 1)                                                  # mixture cases of plant-one-l, in turn (at pi = 0.3: 49, 42, 9 % of the chains)
N_SWEEPS = 2


def place_edges(Nreg):
    """(n, m), n > m: the edges every `item` / `plant-*` set touches.  Same block: (15, 0) rows 15 and 0, (1, 0), (8, 7),
    (15, 14); with a second block (16, 3), (20, 17), (31, 30); region 32 / 16 alone in the last block against partners of
    other blocks."""
    e = [(15, 0), (1, 0), (8, 7), (15, 14)]
    if Nreg == 17:
        e += [(16, 0), (16, 15)]
    if Nreg >= 33:
        e += [(16, 3), (20, 17), (31, 30), (32, 0), (32, 15), (32, 31)]
    return [(n, m) for (n, m) in e if n < Nreg]


def edge_id(n, m):
    return n * (n - 1) // 2 + m


class Tables:
    """Tables, hyper, initial state, the oracle's states and conditionals; .planted: dict of equal-length arrays."""


def _planted(Nreg, U, rng, n_per_subset):
    """Edges (distinct), patients and subsets of the planted items: the placement edges first, then random ones."""
    C = Nreg * (Nreg - 1) // 2
    want = 6 * n_per_subset
    first = [edge_id(n, m) for (n, m) in place_edges(Nreg)]
    rest = [c for c in rng.permutation(C) if c not in set(first)]
    edges = np.array((first + rest)[:min(want, C)], dtype=np.int64)
    k = np.arange(len(edges))
    return dict(edge=edges, u=(k * 5 + 1) % U, subset=k % 6, l=np.array(ONE_L)[(k // 6) % 3])


def _recentre(S_B, lM, lng, r0, edges, seed, sweep, chain0):
    """S_B[c, k] of `edges` moved so that the finite a_k of the f pass from r0 average 0 over the chains."""
    f = np.zeros((r0.shape[0], S_B.shape[0]), dtype=np.uint8)
    a = CO.gibbs_f_step(f, r0, S_B, lM, lng, seed, sweep, chain0, want_cond=True, draw=False)
    for c in edges:
        for k in range(3):
            v = a[:, c, k]
            ok = np.isfinite(v)
            if ok.any():
                S_B[c, k] -= v[ok].mean()


def from_data(Nreg, U, seed):
    """(b, bt, theta): epsilon = 0, sigma_0 = 0.015.  N_0 underflows beyond 38.6 sigma_0 of mu_0: ordinary bt is kept below
    36 sigma_0 (no entry in the band where exp is subnormal and two libraries may round differently), outliers sit at 43 to
    50 sigma_0 on the placement edges and on 2 % of the items.  N_1 and N_2 stay far from underflow there."""
    import fcdiff_amd
    m = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(Nreg, 3, U, seed=seed)
    m.epsilon = 0.0
    m.sigma = np.array([0.015, 0.035, 0.05])
    rng = np.random.default_rng([seed, 9])
    bt = np.clip(np.array(bt, dtype=np.float64), m.mu[0] - 36 * 0.015, m.mu[0] + 36 * 0.015)
    out = rng.random(bt.shape) < 0.02
    for (i, (n, mm)) in enumerate(place_edges(Nreg)):
        out[edge_id(n, mm), (i * 3) % U] = True
    bt[out] = m.mu[0] + rng.uniform(43, 50, size=int(out.sum())) * 0.015
    return np.ascontiguousarray(b, dtype=np.float64), np.ascontiguousarray(bt), m.theta(), out


def build(source, Nreg, U, G, seed, sweep=0, chain0=0):
    rng = np.random.default_rng([seed, Nreg, U, G, 91])
    C = Nreg * (Nreg - 1) // 2
    T = Tables()
    (T.source, T.Nreg, T.U, T.G, T.seed, T.sweep, T.chain0, T.C) = (source, Nreg, U, G, seed, sweep, chain0, C)
    parts = source.split("+")
    (gamma, pi2) = (BP.GAMMA.copy(), BP.PI2.copy())
    T.data = None
    if "from-data" in parts:
        (b, bt, theta, outl) = from_data(Nreg, U, seed)
        (S_B, lM) = CO.lik_tables(b, bt, theta)
        T.data = (b, bt, theta, outl)
    else:
        (S_B, lM) = BP.base_tables("model", Nreg, U, seed)
    S_B = np.ascontiguousarray(S_B, dtype=np.float64).copy()
    lM = np.ascontiguousarray(lM, dtype=np.float64).copy()
    for k in range(3):
        if "gamma%d" % k in parts:
            gamma = np.full(3, 0.5)
            gamma[k] = 0.0
    if "pi0" in parts:
        pi2 = np.array([1.0, 0.0])
    if "pi1" in parts:
        pi2 = np.array([0.0, 1.0])
    with np.errstate(divide="ignore"):
        (lng, lnpi2) = (np.log(gamma), np.log(pi2))
    (f0, r0) = CO.gibbs_init(G, Nreg, U, 0.3, seed, chain0)
    T.planted = dict(edge=np.zeros(0, dtype=np.int64))
    recentre = []
    if "item" in parts or "firm" in parts:
        hit = rng.random((C, U)) < 0.01 if "item" in parts else np.zeros((C, U), dtype=bool)
        for (i, (n, m)) in enumerate(place_edges(Nreg)):
            hit[edge_id(n, m), (i * 3 + 1) % U] = True
        lM[hit] = NINF
        T.items = hit
    if "firm" in parts:
        with np.errstate(invalid="ignore"):
            (_a, bounds) = R.edge_bounds(R.edge_table(lM))
            short = FIRM_MARGIN - R.margins(S_B, lng, bounds)
        for c in np.nonzero(~hit.any(axis=1))[0]:
            S_B[c, c % 3] += short[c, c % 3]
    if "plant-all-l" in parts or "plant-one-l" in parts:
        P = _planted(Nreg, U, rng, 6 if Nreg < 33 else 8)
        for (c, u, s, l) in zip(P["edge"], P["u"], P["subset"], P["l"]):
            for k in SUBSETS[s]:
                if "plant-all-l" in parts:
                    lM[c, u, k, :] = NINF
                else:
                    lM[c, u, k, l] = NINF
        T.planted = P
        recentre = list(P["edge"])
    if any(p.startswith("gamma") for p in parts):
        recentre = list(range(0, C, 3))
    if recentre:
        _recentre(S_B, lM, lng, r0, recentre, seed, sweep, chain0)
    assert not np.isnan(lM).any() and not (lM == np.inf).any() and np.isfinite(S_B).all()
    (T.S_B, T.lM, T.gamma, T.pi2, T.lng, T.lnpi2, T.f0, T.r0) = (S_B, lM, gamma, pi2, lng, lnpi2, f0, r0)

    # the C oracle: N_SWEEPS sweeps, the conditionals before every draw
    (f, r) = (f0.copy(), r0.copy())
    (T.cond_f, T.cond_r, T.f_after, T.r_after) = ([], [], [], [])
    for s in range(N_SWEEPS):
        T.cond_f.append(CO.gibbs_f_step(f, r, S_B, lM, lng, seed, sweep + s, chain0, want_cond=True))
        T.cond_r.append(CO.gibbs_r_step(f, r, lM, lnpi2, seed, sweep + s, BP.EDGE_SYMMETRIC, chain0, want_cond=True))
        T.f_after.append(f.copy())
        T.r_after.append(r.copy())
    (T.f1, T.r1, T.f2, T.r2) = (T.f_after[0], T.r_after[0], T.f_after[1], T.r_after[1])
    return T


def f_pattern(a):
    """Index into PATTERNS of the -inf set of (a0, a1, a2) along the last axis, -1 where all three are finite."""
    bits = (a == NINF).astype(np.int64) @ np.array([1, 2, 4])
    code = np.full(8, -1)
    for (i, p) in enumerate(PATTERNS):
        code[sum(1 << k for k in p)] = i
    return code[bits]


def r_pattern(s):
    """0 finite, 1 s0 = -inf alone, 2 s1 = -inf alone, 3 both, of cond_r (.., 2)."""
    return (s[..., 0] == NINF).astype(np.int64) + 2 * (s[..., 1] == NINF).astype(np.int64)


def decided_rule(T):
    """What the f pass's rule of decided edges says of the set's table at its hyper (tests/f_sure_ref.py, on the CPU):
    -> (the record build's hint: some tile is decided with FCD_F_SURE_DRIFT nats in hand, the mode of every edge at the
    hint's threshold, -1 where open, the edges whose bounds are NaN)."""
    assert T.U <= 64
    with np.errstate(invalid="ignore", over="ignore"):
        (a, b) = R.edge_bounds(R.edge_table(T.lM))
        mode = R.edge_modes(T.S_B, T.lng, T.U, a, b, R.T - R.DRIFT)
        return R.hint(T.Nreg, T.S_B, T.lng, T.U, a, b), mode, np.nonzero(np.isnan(b).any(axis=1))[0]


def f_uniforms(T, s=0):
    """(G, C) float64: the uniform of every f draw of compared sweep s."""
    return BP.f_words(T.seed, T.C, T.chain0 + np.arange(T.G), T.sweep + s).astype(np.float64) * (1.0 / 4294967296.0)


def diff_form_draw(a, x):
    """fcd_draw_f(0, a1 - a0, a2 - a0, x) in NumPy, as the fast f forms' exact repeat makes it from log-odds against type 0:
    fmax ignores a NaN, every comparison with a NaN is false."""
    with np.errstate(invalid="ignore", over="ignore"):
        (b1, b2) = (a[..., 1] - a[..., 0], a[..., 2] - a[..., 0])
        mx = np.fmax(0.0, np.fmax(b1, b2))
        (e0, e1, e2) = (np.exp(0.0 - mx), np.exp(b1 - mx), np.exp(b2 - mx))
        t = x * ((e0 + e1) + e2)
        return np.where(t < e0, 0, np.where(t < e0 + e1, 1, 2))


# ------------------------------------------------------------------------------------------------
# the sets: (source, Nreg, U, G, seed).  Shapes: three blocks of 16 regions with one region in the last and 16 chain words;
# one block and one pair of patients; a one-row second block at the full U <= 64 kernel; the any-U kernel; one patient
# ------------------------------------------------------------------------------------------------
BIG = (33, 7, 1024)
SETS = {
    "item-33-7": ("item",) + BIG + (101,), "item-16-2": ("item", 16, 2, 128, 102), "item-17-64": ("item", 17, 64, 128, 103),
    "item-33-70": ("item", 33, 70, 128, 104),
    "gamma0-33-7": ("gamma0",) + BIG + (111,), "gamma0-16-2": ("gamma0", 16, 2, 128, 112), "gamma0-17-64": ("gamma0", 17, 64, 128, 113),
    "gamma0-33-70": ("gamma0", 33, 70, 128, 114), "gamma0-16-1": ("gamma0", 16, 1, 128, 115),
    "plant-all-l-33-7": ("plant-all-l",) + BIG + (121,), "plant-all-l-17-64": ("plant-all-l", 17, 64, 128, 122),
    "plant-one-l-33-7": ("plant-one-l",) + BIG + (131,), "plant-one-l-16-2": ("plant-one-l", 16, 2, 128, 132),
    "plant-one-l-33-70": ("plant-one-l", 33, 70, 128, 133),
    "gamma1-33-7": ("gamma1",) + BIG + (141,), "gamma1-16-1": ("gamma1", 16, 1, 128, 142),
    "gamma2-33-7": ("gamma2",) + BIG + (151,), "gamma2-33-70": ("gamma2", 33, 70, 128, 152),
    "pi0-33-7": ("pi0",) + BIG + (161,), "pi0-16-2": ("pi0", 16, 2, 128, 162),
    "pi1-33-7": ("pi1",) + BIG + (171,), "pi1-17-64": ("pi1", 17, 64, 128, 172),
    "pi0+item-33-7": ("pi0+item",) + BIG + (181,), "pi0+item-33-70": ("pi0+item", 33, 70, 128, 182),
    "from-data-33-7": ("from-data",) + BIG + (191,), "from-data-16-2": ("from-data", 16, 2, 128, 192),
    "firm-33-7": ("firm",) + BIG + (201,), "firm-17-64": ("firm", 17, 64, 128, 203),
}


@functools.lru_cache(maxsize=None)
def build_set(name, G=None):
    (source, Nreg, U, G0, seed) = SETS[name]
    return build(source, Nreg, U, G0 if G is None else G, seed)
