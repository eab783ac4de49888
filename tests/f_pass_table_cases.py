"""
Tables of every model the fits hand the sampler, for the f pass's record, decided-tile and run forms
(tests/test_f_pass_table_cases.py pins the premises on the CPU, tests/test_gpu_f_pass_model_tables.py runs the kernels on
them).  TEST INFRASTRUCTURE ONLY: NumPy and the in-repo references, no GPU, no torch.

Every builder returns (S_B (C, 3), lM (C, U', 3, 3), Nreg, U', premise) for the hyper-parameters of the default
UnsharedRegionModel; `ladder` returns a list of four of them and `weighted` two.  The tables come from the references the
suite already has -- oracle.fcdiff_oracle.lik_tables, sessions_ref.lik_tables, noise_ref.lik_tables,
missing_data_ref.masked_lik_tables, subtype_region_ref.weighted_table -- and sums over patients are taken in fp64.

The premise (premise()) is what tests/f_sure_ref.py, the NumPy restatement of the rule of decided edges, says of the table
at ln gamma of the default model: which forms of the f pass a call on it must take.

    tiles          pair-aligned tiles with at least one edge
    decided_T      of them, those with every edge decided at FCD_F_SURE_T (what a pass at this gamma skips)
    decided_hint   ... at T - FCD_F_SURE_DRIFT (what the record build's hint word counts)
    any, all       the hint word: some tile decided, and no tile open (the auto choice of the run form)
    capped         edges whose margin exceeds T while their fp32 error bound exceeds FCD_F_SURE_DELTA_CAP: open by the cap alone
    mode_T         the decided mode of every edge at T, -1 where open
    ninf           (C, U') the items with a -inf entry
    nan_bounds     edges whose bounds the record build leaves NaN (a non-finite log-odds in some patient)

Why these tables: an unshared one-scan table decides its edges through S_B alone, since a patient's log-odds are bounded by
ln((1 - epsilon) / (epsilon / 2)) and change sign over the mixture cases.  Summing patients (shared, grouped) multiplies the
bound `a` and the error bound delta by the group size; masked tables hold rows that are exactly 0.0; sessions and noise
tables are log-form sums whose linear products underflow; a weighted table carries 0 * -inf = 0 entries; a scaled table
pushes delta over its cap inside live tiles.
"""
import numpy as np

import f_sure_ref as R
import missing_data_ref as MD
import noise_ref as NR
import sessions_ref as SR
import subtype_region_ref as ST
from oracle import fcdiff_oracle as O


def model():
    import fcdiff_amd
    return fcdiff_amd.UnsharedRegionModel()


def edge_id(n, m):
    return n * (n - 1) // 2 + m


def premise(N, S_B, lM, U, lng=None):
    lng = np.log(model().gamma) if lng is None else lng
    with np.errstate(invalid="ignore"):
        lMf = R.edge_table(lM)
        (a, b) = R.edge_bounds(lMf)
        mode_T = R.edge_modes(S_B, lng, U, a, b)
        mode_h = R.edge_modes(S_B, lng, U, a, b, R.T - R.DRIFT)
        c1 = (lng[1] - lng[0]) + (S_B[:, 1] - S_B[:, 0])
        c2 = (lng[2] - lng[0]) + (S_B[:, 2] - S_B[:, 0])
        delta = R.edge_delta(c1, c2, U, a)
        margin = np.fmax.reduce(R.margins(S_B, lng, b), axis=1)
        capped = np.nonzero((margin > R.T) & (delta > R.F32(R.DELTA_CAP)))[0]
    n_tiles = sum(len(t) > 0 for t in R.tiles(N))
    (d_T, d_h) = (len(R.decided_tiles(N, mode_T)), len(R.decided_tiles(N, mode_h)))
    return dict(tiles=n_tiles, decided_T=d_T, decided_hint=d_h, any=d_h > 0, all=0 < d_h == n_tiles, capped=capped,
                mode_T=mode_T, mode_hint=mode_h, ninf=np.isneginf(lM).any(axis=(2, 3)), nan_bounds=np.nonzero(np.isnan(b).any(axis=1))[0])


def tile_of(N, c):
    """the edges of the pair-aligned tile that holds edge c"""
    return next(t for t in R.tiles(N) if c in t)


def _case(N, S_B, lM, extra=None):
    S_B = np.ascontiguousarray(S_B, dtype=np.float64)
    lM = np.ascontiguousarray(lM, dtype=np.float64)
    U = lM.shape[1]
    assert S_B.shape == (N * (N - 1) // 2, 3) and lM.shape == (S_B.shape[0], U, 3, 3)
    p = premise(N, S_B, lM, U)
    p.update(extra or {})
    return S_B, lM, N, U, p


def data(N, H, U, seed, sessions=None):
    m = model()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed, sessions=sessions)
    return m, np.array(b, dtype=np.float64), np.array(bt, dtype=np.float64)


def one_scan_tables(m, b, bt):
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    return O.sum_lp_B(lpB), lM


def group_sums(lM, sizes):
    """(C, len(sizes), 3, 3): consecutive patients summed group by group, in fp64"""
    assert sum(sizes) == lM.shape[1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.stack([lM[:, off[i]:off[i + 1]].sum(axis=1) for i in range(len(sizes))], axis=1)


def shared(N, H, U0, seed):
    """SharedRegionFit's table: L[:, None], the sum over all U0 patients -- one pseudo-patient"""
    (m, b, bt) = data(N, H, U0, seed)
    (S_B, lM) = one_scan_tables(m, b, bt)
    return _case(N, S_B, lM.sum(axis=1, keepdims=True))


def grouped(N, H, U0, seed, sizes=None):
    """GroupedRegionFit's table: one pseudo-patient per group; sizes None = (1, 2, U0 - 3)"""
    sizes = (1, 2, U0 - 3) if sizes is None else tuple(sizes)
    (m, b, bt) = data(N, H, U0, seed)
    (S_B, lM) = one_scan_tables(m, b, bt)
    return _case(N, S_B, group_sums(lM, sizes))


def grouped64(N, H, seed):
    """64 groups of 70 patients (six pairs, 58 singletons): U' = 64, the pair kernel's limit"""
    return grouped(N, H, 70, seed, sizes=(2,) * 6 + (1,) * 58)


OUTLYING_SCANS = (0.9, 0.95, 0.85)


def _plant_outlier(N, bt):
    """one patient's three scans of edge (3, 1) far above every mean: prod_k N_0 and prod_k N_1 are 0.0 in fp64"""
    bt = bt.copy()
    bt[edge_id(3, 1), 0, :] = OUTLYING_SCANS
    return bt


def _underflowing(m, bt, lM, var_bt=None):
    """the items one of whose linear products of densities is exactly 0.0 while their log-form entries are finite"""
    out = []
    for (c, u) in np.ndindex(bt.shape[:2]):
        p = SR.product_like(bt[c, u], m.mu, m.sigma) if var_bt is None else NR.product_like(bt[c, u], m.mu, m.sigma, var_bt[u])
        if (p == 0.0).any() and np.isfinite(lM[c, u]).all():
            out.append((c, u))
    return out


def sessions(N, H, U, seed, K=3):
    """the sessions table, bt (C, U, K) in log form; one item is planted whose linear products underflow"""
    (m, b, bt) = data(N, H, U, seed, sessions=K)
    bt = _plant_outlier(N, bt)
    (S_B, lM) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    return _case(N, S_B, lM, dict(underflow=_underflowing(m, bt, lM)))


def noise(N, H, U, seed, K=3):
    """sessions with a sampling variance of its own on every control and every scan"""
    (m, b, bt) = data(N, H, U, seed, sessions=K)
    bt = _plant_outlier(N, bt)
    rng = np.random.default_rng([seed, 77])
    var_b = rng.uniform(0.0, 4e-4, size=H)
    var_bt = rng.uniform(0.0, 9e-4, size=(U, K))
    (S_B, lM) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, var_b=var_b, var_bt=var_bt)
    return _case(N, S_B, lM, dict(underflow=_underflowing(m, bt, lM, var_bt), var_b=var_b, var_bt=var_bt))


LONE_CONTROL = -0.095    # between mu_0 and mu_1: ln gamma_1 N_1 - ln gamma_0 N_0 = 0.5, so the edge is open and its draws go both ways


def missing(N, H, U, seed):
    """masked tables: about 20 % of bt NaN, U odd with its last patient all NaN, a region (2) none of whose edges any patient
    has, an edge (zero_lM = (4, 3)) no patient has -- its lM is exactly 0.0 -- and which one control observed, at a value that
    leaves it open (with H controls S_B alone would decide it), and an edge (zero_SB = (N - 1, 0)) no control has: S_B = 0.0"""
    assert U % 2 == 1 and N >= 6
    (m, b, bt) = data(N, H, U, seed)
    rng = np.random.default_rng([seed, 78])
    bt[rng.random(bt.shape) < 0.2] = np.nan
    bt[:, U - 1] = np.nan
    dead = [edge_id(max(n, 2), min(n, 2)) for n in range(N) if n != 2]
    bt[dead, :] = np.nan
    (z_lM, z_SB) = (edge_id(4, 3), edge_id(N - 1, 0))
    bt[z_lM, :] = np.nan
    b[z_lM, :] = np.nan
    b[z_lM, 0] = LONE_CONTROL
    b[z_SB, :] = np.nan
    (S_B, _lpB, _pBt, lM) = MD.masked_lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    return _case(N, S_B, lM, dict(zero_lM=z_lM, zero_SB=z_SB, dead_edges=np.array(dead), nan_fraction=float(np.isnan(bt).mean())))


FAR_SCAN = 3.0           # every N_j(3.0) underflows: the item's nine entries are -inf


def weighted(N, H, U0, seed):
    """the subtype model's tables of two subtypes, sum_u s[u, g] lM[c, u]: patient 1's item of edge (5, 2) is -inf, subtype 0
    has responsibility exactly 0 for that patient (0 * -inf adds nothing) and subtype 1 has 1.  -> (finite table, table
    with -inf), U' = 1 each"""
    assert N >= 6 and U0 >= 3
    (m, b, bt) = data(N, H, U0, seed)
    c0 = edge_id(5, 2)
    bt[c0, 1] = FAR_SCAN
    with np.errstate(divide="ignore"):
        (S_B, lM) = one_scan_tables(m, b, bt)
    assert np.isneginf(lM[c0, 1]).all() and np.isfinite(np.delete(lM.reshape(lM.shape[0] * U0, 9), c0 * U0 + 1, axis=0)).all()
    s = np.random.default_rng([seed, 79]).uniform(0.1, 0.9, size=U0)
    s[1] = 0.0
    L = ST.weighted_table(lM, np.stack([s, 1.0 - s], axis=1))
    return [_case(N, S_B, L[:, g:g + 1], dict(ninf_edge=c0)) for g in range(2)]


def scaled_premise_holds(N, p):
    """an edge over the cap with margin > T in a tile whose other edges are decided, and a decided tile"""
    lone = [c for c in p["capped"] if (np.delete(p["mode_T"][tile_of(N, c)], np.nonzero(tile_of(N, c) == c)[0]) >= 0).all()]
    return len(lone) >= 1 and p["decided_T"] >= 1 and p["any"]


def scaled(N, H, U0, seed, factors=(100.0, 50.0, 200.0, 25.0, 400.0)):
    """a shared table with S_B and L multiplied by the first of `factors` at which scaled_premise_holds"""
    (S_B, L, _N, _U, _p) = shared(N, H, U0, seed)
    for k in factors:
        case = _case(N, k * S_B, k * L, dict(factor=k))
        if scaled_premise_holds(N, case[4]):
            return case
    raise AssertionError("no factor of %s puts an edge over the cap inside a live tile" % (factors,))


LADDER_STATES = ("all", "none", "some", "all")


def hint_state(p):
    return "all" if p["all"] else "some" if p["any"] else "none"


def ladder(N, H, U0, seed, betas=tuple(2.0 ** -k for k in range(1, 12))):
    """(beta S_B, beta L) of a shared table for beta = 1, the largest beta of `betas` at which no tile is decided at the hint,
    the largest at which some but not all are, and 1 again: four successive calls on one engine"""
    (S_B, L, _N, _U, _p) = shared(N, H, U0, seed)
    found = {}
    for beta in betas:
        case = _case(N, beta * S_B, beta * L, dict(beta=beta))
        found.setdefault(hint_state(case[4]), case)
    first = _case(N, S_B, L, dict(beta=1.0))
    return [first, found["none"], found["some"], _case(N, S_B.copy(), L.copy(), dict(beta=1.0))]


# ------------------------------------------------------------------------------------------------
# The cases: name -> (builder, arguments, what the premise must say, chains of the GPU run).
# Nreg = 5 (an empty and a diagonal-only tile), 13 (short last blocks), 18 (a second 16-column block of one partial tile),
# 34 (three blocks); G = 65 (a partial chain word), 1100 (two groups of 16 chain words).
# Kinds: "all" every tile decided at the hint; "mixed" some and not all; "scaled", "missing", "ninf" as
# tests/test_f_pass_table_cases.py states them; "finite" no condition of its own (the twin of "ninf").
# ------------------------------------------------------------------------------------------------
CASES = {
    "shared-5": (shared, (5, 16, 11, 5), "all", 65),
    "shared-13": (shared, (13, 16, 11, 5), "all", 1100),
    "shared-18": (shared, (18, 16, 11, 5), "all", 65),
    "shared-34": (shared, (34, 16, 11, 5), "all", 1100),
    "shared-mixed-13": (shared, (13, 3, 11, 5), "mixed", 65),
    "shared-mixed-34": (shared, (34, 3, 11, 6), "mixed", 65),
    "grouped-13": (grouped, (13, 16, 11, 5), "all", 65),
    "grouped-mixed-18": (grouped, (18, 3, 11, 5), "mixed", 1100),
    "grouped64-5": (grouped64, (5, 32, 6), "all", 1100),
    "grouped64-mixed-13": (grouped64, (13, 16, 5), "mixed", 65),
    "sessions-13": (sessions, (13, 16, 7, 5), "all", 65),
    "sessions-mixed-18": (sessions, (18, 3, 7, 5), "mixed", 65),
    "noise-13": (noise, (13, 16, 6, 5), "all", 1100),
    "noise-mixed-5": (noise, (5, 3, 6, 5), "mixed", 65),
    "missing-13": (missing, (13, 16, 7, 5), "missing", 65),
    "missing-34": (missing, (34, 16, 5, 6), "missing", 1100),
    "weighted-finite-13": (lambda *a: weighted(*a)[0], (13, 16, 11, 5), "finite", 65),
    "weighted-ninf-13": (lambda *a: weighted(*a)[1], (13, 16, 11, 5), "ninf", 65),
    "scaled-13": (scaled, (13, 16, 11, 5), "scaled", 65),
}
LADDER = (ladder, (13, 16, 11, 5), 65)

_built = {}


def build(name):
    """the case, built once (callers leave the arrays unchanged)"""
    if name not in _built:
        (fn, args, _kind, _G) = CASES[name]
        _built[name] = fn(*args)
    return _built[name]


def build_ladder():
    if "ladder" not in _built:
        _built["ladder"] = LADDER[0](*LADDER[1])
    return _built["ladder"]
