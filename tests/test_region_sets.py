"""
Region-set counts without a GPU: the NumPy restatement of tests/region_sets_ref.py against brute force, the three input
forms of `region_sets` and their refusals, what GibbsEngine.run() sends to a shared context on a stand-in, and the
defaults and refusals of region_set_posterior().
"""
import itertools

import numpy as np
import numpy.testing as nptest
import pytest

import region_sets_ref as RS
from engine_stand_in import stand_in_engine
from fcdiff_amd import _lib
from fcdiff_amd import gibbs


@pytest.mark.parametrize("G,N,U", [(1, 2, 1), (37, 6, 4), (70, 9, 5)])
def test_histograms_equal_explicit_loops(G, N, U):
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.1, 0.6)).astype(np.uint8)
    sets = [list(range(N)), [0], [N - 1], [0, N - 1], [0], sorted(rng.choice(N, size=max(1, N // 2), replace=False))]
    (hs, hv) = RS.histograms(r, sets)
    s_max = N
    want_s = np.zeros((len(sets), U, s_max + 1), dtype=np.int64)
    want_v = np.zeros((len(sets), U + 1), dtype=np.int64)
    for (j, s) in enumerate(sets):
        for g in range(G):
            hit = 0
            for u in range(U):
                k = int(sum(r[g, n, u] for n in s))
                want_s[j, u, k] += 1
                hit += 1 if k else 0
            want_v[j, hit] += 1
    assert np.array_equal(hs, want_s) and np.array_equal(hv, want_v)
    assert np.all(hs.sum(axis=2) == G) and np.all(hv.sum(axis=1) == G)
    for (j, s) in enumerate(sets):
        assert not hs[j, :, len(s) + 1:].any()


def test_independent_laws_equal_enumeration():
    rng = np.random.default_rng(5)
    (N, U) = (5, 3)
    q1 = rng.uniform(0.05, 0.95, (N, U))
    q1[1, :] = 0.0
    q1[3, 1] = 1.0
    with np.errstate(divide="ignore"):
        lq = np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 2, (N, U, 1))
    sets = [[0, 1, 2, 3, 4], [1], [0, 3], [2, 3, 4]]
    (pc, pv) = RS.independent_laws(lq, sets)
    want_c = np.zeros_like(pc)
    want_v = np.zeros_like(pv)
    for bits in itertools.product((0, 1), repeat=N * U):
        b = np.array(bits).reshape(N, U)
        w = np.prod(np.where(b == 1, q1, 1.0 - q1))
        if w == 0.0:
            continue
        for (j, s) in enumerate(sets):
            k = b[s].sum(axis=0)
            for u in range(U):
                want_c[j, u, k[u]] += w
            want_v[j, int((k > 0).sum())] += w
    nptest.assert_allclose(pc, want_c, rtol=1e-11, atol=1e-15)
    nptest.assert_allclose(pv, want_v, rtol=1e-11, atol=1e-15)
    nptest.assert_allclose(pc.sum(axis=2), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(pv.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(pc[1], np.tile(np.eye(6)[0], (U, 1)))          # q = 0 everywhere: a point mass at 0
    assert np.array_equal(pv[1], np.eye(U + 1)[0])


def test_three_input_forms_parse_to_the_same_csr():
    N = 9
    as_dict = {"dmn": [7, 0, 3], "salience": (2,), "rest": np.array([8, 1, 4, 5, 6])}
    as_lists = [[7, 0, 3], (2,), np.array([8, 1, 4, 5, 6])]
    mask = np.zeros((3, N), dtype=bool)
    for (j, s) in enumerate(as_lists):
        mask[j, np.asarray(s)] = True
    (n_d, o_d, m_d) = gibbs.region_sets_csr(as_dict, N)
    (n_l, o_l, m_l) = gibbs.region_sets_csr(as_lists, N)
    (n_m, o_m, m_m) = gibbs.region_sets_csr(mask, N)
    assert n_d == ["dmn", "salience", "rest"] and n_l == n_m == ["0", "1", "2"]
    for (o, m) in ((o_d, m_d), (o_l, m_l), (o_m, m_m)):
        assert o.dtype == np.int32 and m.dtype == np.int32
        assert o.tolist() == [0, 3, 4, 9] and m.tolist() == [0, 3, 7, 2, 1, 4, 5, 6, 8]
    # overlaps and repeats of whole sets are fine
    (_n, o, m) = gibbs.region_sets_csr([[1, 2], [2, 1], [2]], N)
    assert o.tolist() == [0, 2, 4, 5] and m.tolist() == [1, 2, 1, 2, 2]


@pytest.mark.parametrize("sets", [
    [],                                        # no set
    {},
    [[1, 2], []],                              # an empty set
    np.zeros((2, 9), dtype=bool),              # ... as a mask row
    [[1, 2, 1]],                               # a duplicate
    [[0, 9]],                                  # outside [0, Nreg)
    [[-1, 3]],
    np.zeros((2, 8), dtype=bool),              # a mask of another width
    [[0.5, 1.0]],                              # not indices
    [[i] for i in range(9)] * 114,             # 1026 sets
], ids=["none", "none-dict", "empty", "empty-mask", "duplicate", "too-large", "negative", "mask-width", "floats", "too-many"])
def test_region_sets_refusals(sets):
    with pytest.raises(ValueError):
        gibbs.region_sets_csr(sets, 9)


def test_region_sets_size_limits():
    with pytest.raises(ValueError, match="at most 1023"):
        gibbs.region_sets_csr([list(range(1024))], 2000)
    (_n, o, _m) = gibbs.region_sets_csr([list(range(1023))] * 1024, 2000)
    assert len(o) == 1025
    with pytest.raises(ValueError, match="at most 1024"):
        gibbs.region_sets_csr([[0]] * 1025, 2000)


def test_new_symbols_load_and_abi_stays_4():
    lib = _lib.load()
    for name in ("fcd_region_sets_set", "fcd_gibbs_region_set_tally", "fcd_gibbs_set_region_set_accumulator"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert lib.fcd_abi_version() == _lib.ABI_VERSION == 4
    assert lib.fcd_region_sets_set(None, None, None, 0) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_region_set_tally(None, None, 4, 2, 64, None, None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_region_set_accumulator(None, None, None, 4, 2, 1) == _lib.FCD_ERR_ARG


def test_a_context_that_holds_other_sets_gets_this_engine_s_first():
    """The context is shared between engines: run() sends the engine's own sets before it attaches its buffers."""
    setter = "fcd_gibbs_set_region_set_accumulator"
    eng = stand_in_engine(64, 7, 3, attached=("region_set",), sets=[[0, 1], [6]])
    assert (eng.region_J, eng.region_smax) == (2, 2)
    eng.region_set_every = 2
    eng.run(0, 5, accumulate_from=1)
    assert [c[0] for c in eng.ctx.calls] == ["fcd_region_sets_set", setter, setter]
    assert eng.ctx.calls[0][1][-1] == 2 and eng.ctx.calls[1][1] == (7, 3, 2)
    eng.run(5, 2, accumulate_from=1)                                  # now the context's sets are this engine's
    assert [c[0] for c in eng.ctx.calls[3:]] == [setter, setter]
    assert eng.region_set_sweeps == 2 + 1                             # sweeps 1, 3 and 5


def test_fit_defaults_and_refusals_without_a_run():
    import fcdiff_amd
    for cls in (fcdiff_amd.fit.UnsharedRegionFit, fcdiff_amd.fit.SharedRegionFit):
        fit = cls()
        assert fit.region_sets is None and fit.region_sets_every == 1
        assert fit.region_set_hist is None and fit.region_set_prevalence_hist is None and fit.region_set_sweeps == 0
        with pytest.raises(ValueError, match="call run"):
            fit.region_set_posterior()                           # no model, no data
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fit.model.sample_fast(5, 3, 2, seed=1)
    (fit.b, fit.bt) = (b, bt)
    with pytest.raises(ValueError, match="no region sets"):
        fit.region_set_posterior()                               # vb, no sets
    with pytest.raises(ValueError, match="no region sets"):
        fit.region_set_posterior(independent=True)
    fit.region_sets = {"a": [0, 1], "b": [4]}
    with pytest.raises(ValueError):
        fit.region_set_posterior()                               # vb without a run: no _lq_R
    fit.method = "gibbs"
    with pytest.raises(ValueError, match="set region_sets before run"):
        fit.region_set_posterior()                               # a gibbs run that did not set them left no histograms
    (fit.region_set_names, fit.region_set_sizes) = (["a", "b"], np.array([2, 1]))
    fit.region_set_hist = np.zeros((2, 2, 3), dtype=np.int64)
    fit.region_set_prevalence_hist = np.zeros((2, 3), dtype=np.int64)
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        fit.region_set_posterior()
    fit.region_set_hist[0, :, 2] = 6
    fit.region_set_hist[1, :, 0] = 6
    fit.region_set_prevalence_hist[0, 2] = 6
    fit.region_set_prevalence_hist[1, 0] = 6
    out = fit.region_set_posterior()
    assert out["names"] == ["a", "b"] and out["sizes"].tolist() == [2, 1]
    assert np.array_equal(out["p_count"][0], np.eye(3)[[2, 2]]) and np.array_equal(out["p_count"][1], np.eye(3)[[0, 0]])
    assert np.array_equal(out["p_any"], [[1.0, 1.0], [0.0, 0.0]]) and np.array_equal(out["expected"], [[2.0, 2.0], [0.0, 0.0]])
    assert np.array_equal(out["p_prevalence"], np.eye(3)[[2, 0]]) and np.array_equal(out["p_none"], [0.0, 1.0])
    fit.method = "mcmc"
    with pytest.raises(ValueError, match="method"):
        fit.region_set_posterior()


@pytest.mark.parametrize("knobs", [
    {"region_sets": [[0, 1]], "region_sets_every": 0},
    {"region_sets": [[0, 1]], "region_sets_every": 1.5},
    {"region_sets": [[0, 5]]},                                    # outside the 5 regions
    {"region_sets": [[]]},
    {"region_sets": [[0, 1]], "n_chains": 1 << 22, "n_sweeps": 2000, "burn_in": 0},       # would overflow uint32
], ids=["every-0", "every-1.5", "index", "empty", "overflow"])
def test_fit_refuses_before_the_run(knobs):
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    for (k, v) in knobs.items():
        setattr(fit, k, v)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 2)                                      # refused before any engine or device state is made
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.region_sets = [[0, 1]]
    with pytest.raises(ValueError, match="at most 512 patients"):
        fit._run_gibbs(5, 513)
