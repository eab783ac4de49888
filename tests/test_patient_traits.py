"""
Patient traits without a GPU: the rank transform patient_traits_scores() and its refusals, the NumPy restatement of
tests/patient_traits_ref.py against brute-force pair counting, the integer AUC bin rule, the arithmetic of
patient_trait_posterior() on hand-made histograms, the host refusals of the query, what GibbsEngine.run() sends to a shared
context on stand-ins, and header against binding.
"""
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import patient_traits_ref as PT
from engine_stand_in import stand_in_engine
from conftest import ROOT
from fcdiff_amd import _lib
from fcdiff_amd import gibbs

NEW_SYMBOLS = {"fcd_patient_traits_set": 6, "fcd_gibbs_patient_trait_tally": 8, "fcd_gibbs_set_patient_trait_accumulator": 6}
NAN = float("nan")


# ---- the rank transform ----

def test_scores_of_ties_nan_and_a_binary_trait():
    (names, scores, known, n_known) = gibbs.patient_traits_scores(
        {"severity": [3.5, -1.0, 7.0, 0.25], "tied": [1, 5, 5, 9], "binary": [True, False, True, True],
         "partly": [NAN, 2.0, 2.0, 1.0]}, 4)
    assert names == ["severity", "tied", "binary", "partly"] and scores.dtype == np.int32 and known.dtype == np.bool_
    assert scores.tolist() == [[1, -3, 3, -1], [-3, 0, 0, 3], [1, -3, 1, 1], [0, 1, 1, -2]]
    assert known.tolist() == [[True] * 4] * 3 + [[False, True, True, True]] and n_known.tolist() == [4, 4, 4, 3]
    assert n_known.dtype == np.int64 and not scores.sum(axis=1).any()


@pytest.mark.parametrize("U,seed", [(2, 0), (7, 1), (70, 2), (512, 3)])
def test_scores_equal_pair_counting_and_keep_their_range(U, seed):
    rng = np.random.default_rng(seed)
    y = np.stack([rng.normal(size=U), rng.integers(0, 3, U).astype(np.float64), (np.arange(U) % 2).astype(np.float64)])
    y[1, :2] = (0.0, 2.0)                            # (never all equal)
    if U > 4:
        y[0, rng.choice(U, U // 3, replace=False)] = NAN
        y[1, [0, U - 1]] = NAN
    (names, scores, known, n_known) = gibbs.patient_traits_scores(y, U)
    assert names == ["0", "1", "2"]
    for q in range(3):
        (a, kn) = PT.scores(y[q])
        nptest.assert_array_equal(scores[q], a)
        nptest.assert_array_equal(known[q], kn)
        assert n_known[q] == kn.sum() and scores[q].sum() == 0 and np.abs(scores[q]).max() <= n_known[q] - 1
        assert not scores[q][~kn].any()
    # a binary trait: -n1 on the zeros and n0 on the ones
    (n1, n0) = (int(y[2].sum()), int(U - y[2].sum()))
    assert set(scores[2][y[2] == 0].tolist()) == {-n1} and set(scores[2][y[2] == 1].tolist()) == {n0}
    # the same vectors as a sequence
    nptest.assert_array_equal(gibbs.patient_traits_scores([row for row in y], U)[1], scores)


@pytest.mark.parametrize("traits,U,match", [
    ({"flat": [2.0, 2.0, 2.0, NAN]}, 4, "all equal"),
    ({"one": [NAN, NAN, 1.0, NAN]}, 4, "known for 1 patients"),
    ({"none": [NAN] * 4}, 4, "known for 0 patients"),
    ({"inf": [1.0, float("inf"), 0.0, 2.0]}, 4, "infinite"),
    ({"minf": [1.0, -float("inf"), 0.0, 2.0]}, 4, "infinite"),
    ({"short": [1.0, 2.0, 3.0]}, 4, "vector of U=4"),
    ({"words": ["a", "b", "c", "d"]}, 4, "must hold numbers"),
    ({}, 4, "holds no trait"),
    (np.arange(4.0), 4, "must be"),
    (np.tile(np.arange(4.0), (17, 1)), 4, "17 traits"),
    (np.arange(513.0)[None, :], 513, "at most 512 patients"),
], ids=["all-equal", "one-known", "none-known", "inf", "minus-inf", "length", "strings", "empty", "1-d", "Q=17", "U=513"])
def test_scores_refusals(traits, U, match):
    with pytest.raises(ValueError, match=match):
        gibbs.patient_traits_scores(traits, U)


def test_scores_at_the_limits():
    (names, scores, _known, n_known) = gibbs.patient_traits_scores(np.tile(np.arange(512.0), (16, 1)), 512)
    assert len(names) == 16 and n_known.tolist() == [512] * 16
    assert (gibbs.PATIENT_TRAIT_MAX_U, gibbs.PATIENT_TRAIT_MAX_TRAITS, gibbs.PATIENT_TRAIT_BINS) == (512, 16, PT.NB)
    nptest.assert_array_equal(scores[5], 2 * np.arange(512) - 511)


# ---- the reference against brute force, the bin rule ----

@pytest.mark.parametrize("G,N,U", [(40, 3, 5), (25, 4, 9), (10, 2, 70)])
def test_reference_auc_equals_pair_counting(G, N, U):
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.2, 0.8)).astype(np.uint8)
    traits = [rng.normal(size=U), rng.integers(0, 3, U).astype(np.float64), (rng.random(U) < 0.4).astype(np.float64)]
    traits[1][0] = 0.0
    traits[1][1] = 1.0                               # (never all equal)
    traits[2][:2] = (0.0, 1.0)
    traits[0][rng.choice(U, U // 3, replace=False)] = NAN
    sets = [[0, N - 1], list(range(N))]
    x = PT.row_indicators(r, sets)
    (hist, total) = PT.tally(r, traits, sets)
    umax = max(int((~np.isnan(y)).sum()) for y in traits)
    assert hist.shape == (3, N + 2, umax + 1 + PT.NB + 3) and total.shape == (3, N + 2, umax + 1)
    n_defined = 0
    for (q, y) in enumerate(traits):
        (a, kn) = PT.scores(y)
        n = int(kn.sum())
        aucs = PT.state_aucs(r, y, sets)
        want = np.zeros_like(hist[q])
        for g in range(G):
            for rho in range(N + 2):
                brute = PT.brute_auc(y, x[g, rho])
                (k, A) = PT.k_and_A(x[g, rho], a, kn)
                want[rho, k] += 1
                if brute is None:
                    assert k in (0, n) and np.isnan(aucs[g, rho])
                    continue
                n_defined += 1
                (wins2, pairs) = brute                   # AUC = wins2 / (2 pairs), compared on integers
                assert pairs == k * (n - k) and wins2 == A + pairs and abs(aucs[g, rho] - wins2 / (2.0 * pairs)) < 1e-15
                want[rho, umax + 1 + PT.auc_bin(int(A), int(k), n)] += 1
                want[rho, umax + 1 + PT.NB + (0 if wins2 < pairs else (1 if wins2 == pairs else 2))] += 1
        nptest.assert_array_equal(hist[q], want)
        assert not hist[q, :, n + 1:umax + 1].any()
    assert n_defined > G
    # auc_mean from trait_sum is the mean of the per-state AUCs
    n_known = [int((~np.isnan(y)).sum()) for y in traits]
    out = PT.summaries(hist, total, n_known)
    for (q, y) in enumerate(traits):
        aucs = PT.state_aucs(r, y, sets)
        for rho in range(N + 2):
            ok = ~np.isnan(aucs[:, rho])
            if ok.any():
                nptest.assert_allclose(out["auc_mean"][q, rho], aucs[ok, rho].mean(), rtol=1e-13)
            else:
                assert np.isnan(out["auc_mean"][q, rho])


def test_the_integer_bin_rule():
    (n, k) = (10, 4)
    d = k * (n - k)                                  # 24
    assert PT.auc_bin(-d, k, n) == 0                 # AUC = 0
    assert PT.auc_bin(0, k, n) == 64                 # AUC = 1/2: the lower edge of bin 64
    assert PT.auc_bin(d, k, n) == 127                # AUC = 1 falls into the last bin
    assert PT.auc_bin(d - 1, k, n) == (128 * (2 * d - 1)) // (2 * d) == 125
    # a bin edge hit exactly: AUC = 3/4 = 96/128 belongs to bin 96, one step of A below it to bin 95 or lower
    assert PT.auc_bin(d // 2, k, n) == 96 and PT.auc_bin(d // 2 - 1, k, n) == 93
    # d = 64 (n = 16, k = 8): A + d = 1 is AUC = 1/128, exactly the edge between bins 0 and 1
    assert PT.auc_bin(1 - 64, 8, 16) == 1 and PT.auc_bin(-64, 8, 16) == 0
    # every reachable (k, A) of a small trait: the rule equals the float rule where the float is not at an edge
    for n in (2, 3, 7):
        for k in range(1, n):
            d = k * (n - k)
            for A in range(-d, d + 1):
                auc = 0.5 + A / (2.0 * d)
                b = PT.auc_bin(A, k, n)
                assert b / 128.0 <= auc and (auc < (b + 1) / 128.0 or (b == 127 and auc == 1.0))


# ---- the posterior's arithmetic on hand-made histograms ----

def hand_made_fit(n_known, rows, seed, total=4000):
    """A gibbs fit's results filled in by hand: per (q, row) random states (k, A) with A of the right parity and range."""
    import fcdiff_amd
    rng = np.random.default_rng(seed)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model = fcdiff_amd.UnsharedRegionModel()
    fit.method = "gibbs"
    K = max(n_known) + 1
    hist = np.zeros((len(n_known), rows, K + PT.NB + 3), dtype=np.int64)
    sums = np.zeros((len(n_known), rows, K), dtype=np.int64)
    for (q, n) in enumerate(n_known):
        for rho in range(rows):
            k = rng.integers(0, n + 1, total)
            d = k * (n - k)
            A = np.where(d > 0, rng.integers(-d, d + 1), 0)
            np.add.at(hist[q, rho], k, 1)
            np.add.at(sums[q, rho], k, A)
            ok = d > 0
            np.add.at(hist[q, rho], K + np.minimum(PT.NB - 1, (PT.NB * (A[ok] + d[ok])) // (2 * d[ok])), 1)
            np.add.at(hist[q, rho], K + PT.NB + np.sign(A[ok]) + 1, 1)
    (fit.patient_trait_hist, fit.patient_trait_sum, fit.patient_trait_sweeps) = (hist, sums, 4)
    (fit.patient_trait_names, fit.patient_trait_n_known) = (["t%d" % q for q in range(len(n_known))], np.asarray(n_known))
    fit.patient_trait_rows = [str(n) for n in range(rows)]
    return fit, hist, sums


@pytest.mark.parametrize("level", [0.95, 0.5])
def test_posterior_arithmetic_on_hand_made_histograms(level):
    n_known = [5, 12, 2]
    (fit, hist, sums) = hand_made_fit(n_known, 3, seed=5)
    out = fit.patient_trait_posterior(level=level)
    assert out["names"] == ["t0", "t1", "t2"] and out["n_known"].tolist() == n_known and out["rows"] == ["0", "1", "2"]
    assert out["sweeps"] == 4
    want = PT.summaries(hist, sums, n_known, level)
    for key in ("p_count", "p_defined", "p_greater", "p_less", "p_equal", "auc_mean", "auc_hist"):
        nptest.assert_allclose(out[key], want[key], rtol=1e-13, atol=1e-15, err_msg=key)
    nptest.assert_array_equal(out["auc_interval"], want["auc_interval"])
    nptest.assert_array_equal(out["auc_edges"], np.arange(129) / 128.0)
    assert out["p_count"].shape == (3, 3, 13) and out["auc_hist"].shape == (3, 3, 128) and out["auc_interval"].shape == (3, 3, 2)
    nptest.assert_allclose(out["p_count"].sum(axis=2), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(out["p_greater"] + out["p_less"] + out["p_equal"], 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(out["auc_hist"].sum(axis=2), 1.0, rtol=0, atol=1e-13)
    assert not out["p_count"][0, :, 6:].any() and not out["p_count"][2, :, 3:].any()
    assert np.all(out["auc_interval"][:, :, 0] <= out["auc_mean"]) and np.all(out["auc_mean"] <= out["auc_interval"][:, :, 1])


def test_posterior_of_point_masses_and_undefined_rows():
    (fit, hist, sums) = hand_made_fit([4], 3, seed=1)
    K = 5
    hist[:] = 0
    sums[:] = 0
    # row 0: ten states, all k = 2 (d = 4) with A = 2: AUC = 3/4
    hist[0, 0, 2] = 10
    sums[0, 0, 2] = 20
    hist[0, 0, K + 96] = 10
    hist[0, 0, K + PT.NB + 2] = 10
    # row 1: never defined (k = 0 in 6 states, k = 4 in 4)
    hist[0, 1, 0] = 6
    hist[0, 1, 4] = 4
    # row 2: 4 undefined, 2 at AUC = 0 (k = 1, A = -3), 3 at AUC = 1/2 (k = 2, A = 0), 1 at AUC = 1 (k = 3, A = 3)
    hist[0, 2, :K] = (4, 2, 3, 1, 0)
    sums[0, 2, :K] = (0, -6, 0, 3, 0)
    hist[0, 2, [K + 0, K + 64, K + 127]] = (2, 3, 1)
    hist[0, 2, K + PT.NB:] = (2, 3, 1)
    out = fit.patient_trait_posterior()
    assert out["p_defined"][0].tolist() == [1.0, 0.0, 0.6]
    assert out["p_greater"][0, 0] == 1.0 and out["p_less"][0, 0] == 0.0 and out["auc_mean"][0, 0] == 0.75
    assert out["auc_interval"][0, 0].tolist() == [0.75, 0.75 + 1 / 128.0]
    for key in ("p_greater", "p_less", "p_equal", "auc_mean"):
        assert np.isnan(out[key][0, 1])
    assert np.isnan(out["auc_interval"][0, 1]).all() and np.isnan(out["auc_hist"][0, 1]).all()
    assert out["p_count"][0, 1].tolist() == [0.6, 0, 0, 0, 0.4]
    nptest.assert_allclose([out["p_less"][0, 2], out["p_equal"][0, 2], out["p_greater"][0, 2]], [2 / 6.0, 3 / 6.0, 1 / 6.0], rtol=1e-15)
    nptest.assert_allclose(out["auc_mean"][0, 2], (2 * 0.0 + 3 * 0.5 + 1 * 1.0) / 6.0, rtol=1e-15)
    assert out["auc_interval"][0, 2].tolist() == [0.0, 1.0]
    # level 0.5: a quarter from either side lies in the bins of AUC = 0 (mass 1/3) and AUC = 1/2 (mass from above 1/6 + 1/2)
    assert fit.patient_trait_posterior(level=0.5)["auc_interval"][0, 2].tolist() == [0.0, 65 / 128.0]


def test_posterior_refusals_touch_no_context():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    assert fit.patient_traits is None and fit.patient_traits_every == 1
    assert fit.patient_trait_hist is None and fit.patient_trait_sum is None and fit.patient_trait_sweeps == 0
    assert fit.patient_trait_names is None and fit.patient_trait_n_known is None and fit.patient_trait_rows is None
    with pytest.raises(ValueError, match="needs the sampler's chains"):
        fit.patient_trait_posterior()                            # the default method is 'vb'
    fit.patient_traits = {"dose": [1.0, 2.0, 3.0, 4.0]}
    with pytest.raises(ValueError, match="needs the sampler's chains"):
        fit.patient_trait_posterior()
    fit.method = "gibbs"
    with pytest.raises(ValueError, match="call run"):
        fit.patient_trait_posterior()                            # before run()
    fit.patient_traits = None
    with pytest.raises(ValueError, match="set patient_traits before run"):
        fit.patient_trait_posterior()
    (fit2, hist, _sums) = hand_made_fit([3], 2, seed=2)
    with pytest.raises(ValueError, match="level"):
        fit2.patient_trait_posterior(level=0.0)
    hist[:] = 0
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        fit2.patient_trait_posterior()
    shared = fcdiff_amd.fit.SharedRegionFit()
    with pytest.raises(ValueError, match="population-level r"):
        shared.patient_trait_posterior()
    shared.model = fcdiff_amd.SharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fcdiff_amd.UnsharedRegionModel().sample_fast(5, 3, 4, seed=1)
    (shared.b, shared.bt, shared.patient_traits) = (b, bt, [[1.0, 2.0, 3.0, 4.0]])
    for method in ("vb", "gibbs"):
        shared.method = method
        with pytest.raises(ValueError, match="population-level r"):
            shared.run()                                         # before any context or table is made
    assert fit._ctx is None and fit2._ctx is None and shared._ctx is None and shared._d == {}


@pytest.mark.parametrize("knobs", [
    {"patient_traits": [[1.0, 2.0, 3.0, 4.0]], "patient_traits_every": 0},
    {"patient_traits": [[1.0, 2.0, 3.0, 4.0]], "patient_traits_every": 1.5},
    {"patient_traits": [[1.0, 2.0, 3.0]]},
    {"patient_traits": [[2.0, 2.0, 2.0, 2.0]]},
    {"patient_traits": [[1.0, 2.0, 3.0, 4.0]], "n_chains": 1 << 22, "n_sweeps": 2000, "burn_in": 0},     # would overflow uint32
], ids=["every-0", "every-1.5", "length", "all-equal", "overflow"])
def test_fit_refuses_before_the_run(knobs):
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    for (k, v) in knobs.items():
        setattr(fit, k, v)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 4)                                      # refused before any engine or device state is made
    assert fit._ctx is None


# ---- header, binding, and the shared context on stand-in engines ----

def test_header_and_binding_agree_on_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for (name, n_args) in NEW_SYMBOLS.items():
        decl = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    lib = _lib.load()
    assert lib.fcd_abi_version() == _lib.ABI_VERSION == 4
    assert lib.fcd_patient_traits_set(None, None, None, 0, 0, 0) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_trait_tally(None, None, 4, 2, 64, None, None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_trait_accumulator(None, None, None, 4, 2, 1) == _lib.FCD_ERR_ARG


def test_a_shared_context_gets_this_engine_s_traits_and_sets_first():
    setter = "fcd_gibbs_set_patient_trait_accumulator"
    eng = stand_in_engine(64, 7, 6, attached=("patient_trait",), traits={"dose": [1, 2, 3, NAN, 5, 5]}, sets=[[0, 1], [6]])
    eng.patient_trait_every = 2
    assert eng.patient_trait_rows() == 9
    assert eng.patient_trait_row_names() == [str(n) for n in range(7)] + ["set:0", "set:1"]
    eng.run(0, 5, accumulate_from=1)
    assert [c[0] for c in eng.ctx.calls] == ["fcd_region_sets_set", "fcd_patient_traits_set", setter, setter]
    assert eng.ctx.calls[1][1] == (1, 6, 1)                           # Q = 1, U = 6, with the sets as rows
    assert eng.ctx.calls[2][1] == (7, 6, 2)
    eng.run(5, 2, accumulate_from=1)                                  # now the context holds this engine's
    assert [c[0] for c in eng.ctx.calls[4:]] == [setter, setter]
    assert eng.patient_trait_sweeps == 2 + 1                          # sweeps 1, 3 and 5
    with pytest.raises(ValueError, match="detach the patient-trait accumulator"):
        eng.set_region_sets([[0]])                                    # the sets are rows of the attached buffers
    with pytest.raises(ValueError, match="detach the patient-trait accumulator"):
        eng.set_patient_traits([[1, 2, 3, 4, 5, 6]])
    plain = stand_in_engine(64, 7, 6, attached=("patient_trait",), traits=[[1, 2, 3, 4, 5, 6]])    # without sets: the regions alone
    assert plain.patient_trait_rows() == 7
    plain.run(0, 2, accumulate_from=0)
    assert [c[0] for c in plain.ctx.calls] == ["fcd_patient_traits_set", setter, setter]
    assert plain.ctx.calls[0][1] == (1, 6, 0)

