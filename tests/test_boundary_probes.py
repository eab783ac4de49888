"""
Conditions on the INPUTS of tests/test_gpu_draw_boundaries.py, checked without a GPU: the tables tests/boundary_probes.py
builds really put the target draws where it says, the C oracle resolves every one of them, and there are enough of them.

Smallest distances.  The issue's ranges start at |d| = 1e-10 (f, relative) and 1e-9 (r, absolute).  A regime keeps that only
where the oracle's own fp64 sums resolve it: boundary_probes.f_resolution / r_resolution bound what ANY order of the fp64
additions can move a distance (the 1e-13 / 1e-11 of test_gibbs_cfg3_size_properties, worked out for the tables at hand), and
the smallest probe of a table set stays three decades above that bound.  With S_B up to ~650 (model), sums of 64 - 70 terms
(U = 64, 70), entries of tens to thousands of nats (heavy, shared) the bound is larger and the set's smallest |d| is RAISED
accordingly -- up to 1.8e-7 (f, heavy at U = 64) and 1.1e-6 (r, shared at 33 regions); P.f_min / P.r_min hold the values and
test_rounding_cannot_move_a_probe checks them on the final tables.  Nothing is compared at a distance the oracle cannot
resolve.
"""
import numpy as np
import pytest

import boundary_probes as BP
from oracle import c_oracle as CO
from oracle import fcdiff_oracle as O

ALL_SETS = list(BP.SETS) + list(BP.FAR_SETS) + list(BP.SCAN_SETS)


def test_vectorised_uniforms_equal_the_scalar_oracle_functions():
    seed = 0xA4093822299F31D0
    chains = [0, 5, 64, 129, 2 ** 32 - 1]
    w = BP.f_words(seed, 11, chains, 3)
    for (g, ch) in enumerate(chains):
        for c in range(11):
            assert w[g, c] * (1.0 / 4294967296.0) == O.site_uniform32(seed, c >> 2, ch, 3, O.KIND_F, c & 3)
    for U in (1, 2, 7):
        x = BP.r_uniforms(seed, 5, U, chains, 1)
        for (g, ch) in enumerate(chains):
            for n in range(5):
                for u in range(U):
                    assert x[g, n, u] == O.site_uniform(seed, n * ((U + 1) >> 1) + (u >> 1), ch, 1, O.KIND_R, u & 1)


def oracle_sweep(P):
    """The C oracle's f and r step of the probed sweep on the final tables, with the smallest tie margin of each."""
    (f, r) = (P.f0.copy(), P.r0.copy())
    mf = CO.gibbs_f_step_margin(f, r, P.S_B, P.lM, P.lng, P.seed, P.sweep, P.chain0)
    mr = CO.gibbs_r_step_margin(f, r, P.lM, P.lnpi2, P.seed, P.sweep, BP.EDGE_SYMMETRIC, P.chain0)
    return f, r, mf, mr


@pytest.mark.parametrize("name", ALL_SETS)
def test_probe_outcomes_match_the_oracle(name):
    P = BP.build_set(name)
    (f, r, _mf, _mr) = oracle_sweep(P)
    assert np.array_equal(f, P.f1) and np.array_equal(r, P.r1)
    (pf, pr) = (P.f, P.r)
    # the oracle's draw is the prescribed outcome ...
    assert np.array_equal(f[pf["chain"], pf["edge"]], pf["outcome"])
    assert np.array_equal(r[pr["chain"], pr["n"], pr["u"]], pr["outcome"])
    # ... the long-double distance on the final tables has the prescribed sign, threshold and (within 1 %) magnitude
    assert np.array_equal(np.sign(pf["d_final"]), np.sign(pf["d"])) and np.array_equal(pf["thr_final"], pf["thr"])
    assert np.array_equal(pf["outcome_final"], pf["outcome"])
    assert np.max(np.abs(pf["d_final"] / pf["d"] - 1.0)) < 1e-2
    assert np.array_equal(np.sign(pr["d_final"]), np.sign(pr["d"]))
    assert np.max(np.abs(pr["d_final"] / pr["d"] - 1.0)) < 1e-2
    # both thresholds, both signs, both r outcomes
    plain = pf["kind"] == 0
    for thr in (0, 1):
        for sg in (-1, 1):
            assert ((pf["thr"][plain] == thr) & (np.sign(pf["d"][plain]) == sg)).sum() >= 10
    assert 0.3 < pr["outcome"].mean() < 0.7 or len(pr["n"]) < 40
    assert np.abs(P.lM).max() <= BP.LM_MAX and P.Nreg <= 70


@pytest.mark.parametrize("name", ALL_SETS)
def test_rounding_cannot_move_a_probe(name):
    P = BP.build_set(name)
    (_f, _r, mf, mr) = oracle_sweep(P)
    (f_res, r_res) = (BP.f_resolution(P.S_B, P.lM, P.lng), BP.r_resolution(P.lM, P.lnpi2, P.Nreg))
    # no draw of the sweep, probe or bystander, is closer to a tie than fp64 re-ordering could move it ...
    assert mf >= max(0.5e-10, f_res), (mf, P.f_min, f_res)
    assert mr >= max(0.5e-9, r_res), (mr, P.r_min, r_res)
    # ... and that bound stays three decades below the smallest probe
    assert P.f_min >= BP.F_DMIN and P.r_min >= BP.R_DMIN
    assert np.abs(P.f["d"][P.f["kind"] != 1]).min() >= P.f_min * (1 - 1e-9) >= 1e3 * f_res * (1 - 1e-9) or name in BP.SCAN_SETS
    assert np.abs(P.r["d"]).min() >= P.r_min * (1 - 1e-9) >= 1e3 * r_res * (1 - 1e-9)
    if name in BP.SCAN_SETS:
        k = P.f["kind"]
        assert np.abs(P.f["d"][k == 0]).min() >= P.f_min >= 1e3 * f_res
        assert np.abs(P.f["d"][k == 2]).min() >= BP.F_DMIN >= 1e3 * f_res


@pytest.mark.parametrize("name", ALL_SETS)
def test_coverage_and_unchanged_f_step(name):
    P = BP.build_set(name)
    sites = (P.Nreg - 1) * P.U
    far = name in BP.FAR_SETS            # (|d| >= 1e-3 of a threshold leaves no room next to x < 1e-3: fewer edges there)
    assert len(P.f["edge"]) >= (0.90 if far else 0.95) * P.C and len(set(P.f["edge"])) == len(P.f["edge"])
    assert len(P.r["n"]) >= 0.90 * sites and P.r["n"].max() <= P.Nreg - 2
    assert (P.r["partner"] > P.r["n"]).all()
    assert P.dropped["f"] == P.C - len(P.f["edge"]) and P.dropped["r"] == sites - len(P.r["n"])
    # the target chains rotate over every lane and every chain word, the partial last word included
    lanes = set(P.f["chain"] % 64) | set(P.r["chain"] % 64)
    words = set(P.f["chain"] // 64)
    assert len(lanes) == 64 and words == set(range((P.G + 63) // 64))
    assert (P.f["chain"] >= 128).any() or P.G != 130
    # a tenth of the r probes sit on the most extreme uniforms of the scan
    assert P.r["extreme"].sum() >= len(P.r["n"]) // 10 - 2
    with np.errstate(divide="ignore"):
        lg = np.abs(np.log(P.r["x"] / (1 - P.r["x"])))
    if sites >= 40:
        assert np.median(lg[P.r["extreme"]]) > np.quantile(lg[~P.r["extreme"]], 0.95)
    # the r offsets (the same on all three k) left every f draw where it was
    assert P.f_step_unchanged
    f = P.f0.copy()
    CO.gibbs_f_step(f, P.r0, P.S_B_base, P.lM_before_r, P.lng, P.seed, P.sweep, P.chain0)
    assert np.array_equal(f, P.f1)


def decades(lo, hi):
    """The whole decades [10^k, 10^(k+1)] inside [lo, hi]."""
    k0 = int(np.ceil(np.log10(lo) - 1e-9))
    return [(10.0 ** k, 10.0 ** (k + 1)) for k in range(k0, -1) if 10.0 ** (k + 1) <= hi * (1 + 1e-9)]


@pytest.mark.parametrize("regime", BP.REGIMES)
def test_every_decade_of_distance_is_populated(regime):
    """At least 40 f probes and, for U > 1, 40 r probes in every whole decade of distance some table set of the regime spans."""
    sets = [BP.build_set(n) for (n, s) in BP.SETS.items() if s[0] == regime]
    df = np.concatenate([np.abs(P.f["d"]) for P in sets])
    for (lo, hi) in decades(min(P.f_min for P in sets), BP.F_DMAX):
        assert ((df >= lo) & (df < hi)).sum() >= 40, (regime, "f", lo)
    assert len(decades(min(P.f_min for P in sets), BP.F_DMAX)) >= 6
    sets = [P for P in sets if P.U > 1]
    if sets:
        dr = np.concatenate([np.abs(P.r["d"]) for P in sets])
        dec = decades(min(P.r_min for P in sets), BP.R_DMAX)
        assert len(dec) >= 5
        for (lo, hi) in dec:
            assert ((dr >= lo) & (dr < hi)).sum() >= 40, (regime, "r", lo)


@pytest.mark.parametrize("name", list(BP.SCAN_SETS))
def test_extreme_uniform_scan(name):
    """The short-cut probes straddle 15.01 nats and both bounds on x; among them the exact outcome is sometimes not the
    argmax; the floor probes are all but one-hot with x next to 1."""
    P = BP.build_set(name)
    f = P.f
    assert 100 <= P.n_extreme <= 400
    sure = f["kind"] == 1
    tail = np.minimum(f["x"], 1 - f["x"])
    assert (tail[sure] < 1e-4).all() and sure.sum() >= 100
    assert (f["lead"][sure] >= 12).all() and (f["lead"][sure] <= 18).all()
    assert (f["lead"][sure] > 15.2).sum() >= 20 and (f["lead"][sure] < 14.8).sum() >= 20
    hand = sure & (tail > 1e-6) & (tail < 5e-6)
    assert hand.sum() >= 4 and (sure & (tail < 1e-6)).sum() >= 1
    # a lead between 12.5 and 15 with the draw on the far side of the small mass: what a too small 15.01 would get wrong
    flip = sure & (f["outcome"] != f["argmax"])
    assert (flip & (f["lead"] > 12.5) & (f["lead"] < 15.0)).sum() >= 3
    assert (sure & (f["outcome"] == f["argmax"]) & (f["lead"] > 15.2) & (tail > 1e-6) & (tail < 1e-5)).sum() >= 1
    floor = f["kind"] == 2
    assert floor.sum() >= 30 and (f["x"][floor] > 1 - 1e-4).all() and (f["argmax"][floor] == 0).all()
    assert (np.abs(f["d"][floor]) < 3e-8).sum() >= 10 and (np.abs(f["d"][floor]) <= 1e-6).all()
