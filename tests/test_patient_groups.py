"""
Patient groups and contrasts without a GPU: the NumPy restatement of tests/patient_groups_ref.py against explicit loops, the
three input forms of `patient_groups` and the refusals of groups and contrasts, the arithmetic of patient_group_posterior() on
hand-made histograms, the knobs of the fit on a stand-in engine, what GibbsEngine.run() sends to a shared context on
stand-ins, the shared fit's refusal, and header against binding.
"""
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import patient_groups_ref as PG
from engine_stand_in import stand_in_engine
from conftest import ROOT
from fcdiff_amd import _lib
from fcdiff_amd import gibbs

NEW_SYMBOLS = {"fcd_patient_groups_set": 7, "fcd_gibbs_patient_group_tally": 8, "fcd_gibbs_set_patient_group_accumulator": 6}


@pytest.mark.parametrize("G,N,U", [(1, 2, 1), (37, 6, 5), (70, 4, 9)])
def test_histograms_equal_explicit_loops(G, N, U):
    rng = np.random.default_rng(G + N + U)
    r = (rng.random((G, N, U)) < rng.uniform(0.1, 0.7)).astype(np.uint8)
    groups = [[0], [U - 1], list(range(U)), list(range(0, U, 2))] + ([list(range(1, U, 2))] if U > 1 else [])
    contrasts = [(3, 4), (4, 0)] if U > 2 else []
    sets = [[0], list(range(N)), [0, N - 1]]
    (hg, hj) = PG.histograms(r, groups, contrasts, sets)
    rows = N + len(sets)
    want_g = np.zeros((len(groups), rows, U + 1), dtype=np.int64)
    want_j = [np.zeros((rows, len(groups[a]) + 1, len(groups[b]) + 1), dtype=np.int64) for (a, b) in contrasts]
    for g in range(G):
        for rho in range(rows):
            ind = [int(r[g, rho, u]) if rho < N else int(any(r[g, n, u] for n in sets[rho - N])) for u in range(U)]
            k = [sum(ind[u] for u in grp) for grp in groups]
            for (j, kj) in enumerate(k):
                want_g[j, rho, kj] += 1
            for (p, (a, b)) in enumerate(contrasts):
                want_j[p][rho, k[a], k[b]] += 1
    assert np.array_equal(hg, want_g) and all(np.array_equal(x, y) for (x, y) in zip(hj, want_j))
    assert np.all(hg.sum(axis=2) == G)
    for (j, grp) in enumerate(groups):
        assert not hg[j, :, len(grp) + 1:].any()
    for (p, (a, b)) in enumerate(contrasts):                          # the joint's marginals are the groups' histograms
        assert np.array_equal(hj[p].sum(axis=2), hg[a, :, :len(groups[a]) + 1])
        assert np.array_equal(hj[p].sum(axis=1), hg[b, :, :len(groups[b]) + 1])
    back = PG.split_joint(PG.flat_joint(hj), groups, contrasts, rows)
    assert all(np.array_equal(x, y) for (x, y) in zip(back, hj)) and PG.flat_joint([]).shape == (1,)
    (hg0, _hj0) = PG.histograms(r, groups, [], None)                  # without sets: the region rows alone
    assert np.array_equal(hg0, hg[:, :N])


def test_three_input_forms_parse_to_the_same_csr():
    U = 9
    as_dict = {"treated": [7, 0, 3], "one": (2,), "rest": np.array([8, 1, 4, 5, 6])}
    as_lists = [[7, 0, 3], (2,), np.array([8, 1, 4, 5, 6])]
    mask = np.zeros((3, U), dtype=bool)
    for (j, s) in enumerate(as_lists):
        mask[j, np.asarray(s)] = True
    (n_d, o_d, m_d) = gibbs.patient_groups_csr(as_dict, U)
    (n_l, o_l, m_l) = gibbs.patient_groups_csr(as_lists, U)
    (n_m, o_m, m_m) = gibbs.patient_groups_csr(mask, U)
    assert n_d == ["treated", "one", "rest"] and n_l == n_m == ["0", "1", "2"]
    for (o, m) in ((o_d, m_d), (o_l, m_l), (o_m, m_m)):
        assert o.dtype == np.int32 and m.dtype == np.int32
        assert o.tolist() == [0, 3, 4, 9] and m.tolist() == [0, 3, 7, 2, 1, 4, 5, 6, 8]
    (_n, o, m) = gibbs.patient_groups_csr([[1, 2], [2, 1], [2]], U)   # overlapping groups are fine
    assert o.tolist() == [0, 2, 4, 5] and m.tolist() == [1, 2, 1, 2, 2]
    # contrasts by name and by index
    (pairs, bins) = gibbs.patient_group_contrasts([("treated", "rest"), (1, 0), ("one", 2)], n_d, o_d, m_d)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 2], [1, 0], [1, 2]]
    assert bins.dtype == np.int64 and bins.tolist() == [0, 24, 32, 44]
    (pairs, bins) = gibbs.patient_group_contrasts(None, n_d, o_d, m_d)
    assert pairs.shape == (0, 2) and bins.tolist() == [0]


@pytest.mark.parametrize("groups", [
    [],                                        # no group
    {},
    [[1, 2], []],                              # an empty group
    np.zeros((2, 9), dtype=bool),              # ... as a mask row
    [[1, 2, 1]],                               # a duplicate
    [[0, 9]],                                  # outside [0, U)
    [[-1, 3]],
    np.zeros((2, 8), dtype=bool),              # a mask of another width
    [[0.5, 1.0]],                              # not indices
    [[i % 9] for i in range(65)],              # 65 groups
], ids=["none", "none-dict", "empty", "empty-mask", "duplicate", "too-large", "negative", "mask-width", "floats", "too-many"])
def test_patient_groups_refusals(groups):
    with pytest.raises(ValueError):
        gibbs.patient_groups_csr(groups, 9)


def test_patient_groups_limits():
    with pytest.raises(ValueError, match="at most 512 patients"):
        gibbs.patient_groups_csr([[0]], 513)
    (_n, o, _m) = gibbs.patient_groups_csr([list(range(512))] * 64, 512)
    assert len(o) == 65


@pytest.mark.parametrize("contrasts,match", [
    ([("a", "nobody")], "unknown patient group"),
    ([(0, 4)], "not a name or an index"),
    ([(-1, 0)], "not a name or an index"),
    ([(0.0, 1)], "not a name or an index"),
    ([("a", "a")], "twice"),
    ([(1, 1)], "twice"),
    ([("a", "ab")], "overlap"),
    ([("a", "b", "c")], "pair"),
    ([("a", "b")] * 65, "at most 64"),
], ids=["unknown-name", "index", "negative", "float", "twice", "twice-index", "overlap", "triple", "too-many"])
def test_contrast_refusals(contrasts, match):
    csr = gibbs.patient_groups_csr({"a": [0, 1], "b": [2, 3, 4], "ab": [1, 2], "c": [5]}, 9)
    with pytest.raises(ValueError, match=match):
        gibbs.patient_group_contrasts(contrasts, *csr)


def test_contrast_bin_cap():
    csr = gibbs.patient_groups_csr([list(range(127)), list(range(127, 254)), list(range(254, 382))], 400)
    (_pairs, bins) = gibbs.patient_group_contrasts([(0, 1)], *csr)
    assert bins.tolist() == [0, 128 * 128] and 128 * 128 == gibbs.PATIENT_GROUP_MAX_BINS
    with pytest.raises(ValueError, match="contrast 1 .* 16512 joint bins"):
        gibbs.patient_group_contrasts([(0, 1), (0, 2)], *csr)


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
    assert lib.fcd_patient_groups_set(None, None, None, 0, None, 0, 0) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_patient_group_tally(None, None, 4, 2, 64, None, None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_gibbs_set_patient_group_accumulator(None, None, None, 4, 2, 1) == _lib.FCD_ERR_ARG


def test_a_shared_context_gets_this_engine_s_groups_and_sets_first():
    setter = "fcd_gibbs_set_patient_group_accumulator"
    eng = stand_in_engine(64, 7, 6, attached=("patient_group",), groups={"a": [0, 1], "b": [2, 5]}, contrasts=[("a", "b")],
                          sets=[[0, 1], [6]])
    eng.patient_group_every = 2
    assert eng.patient_group_rows() == 9
    assert eng.patient_group_row_names() == [str(n) for n in range(7)] + ["set:0", "set:1"]
    eng.run(0, 5, accumulate_from=1)
    assert [c[0] for c in eng.ctx.calls] == ["fcd_region_sets_set", "fcd_patient_groups_set", setter, setter]
    assert eng.ctx.calls[1][1][1:] == (1, 1)                          # P = 1, with the sets as rows
    assert eng.ctx.calls[2][1] == (7, 6, 2)
    eng.run(5, 2, accumulate_from=1)                                  # now the context holds this engine's
    assert [c[0] for c in eng.ctx.calls[4:]] == [setter, setter]
    assert eng.patient_group_sweeps == 2 + 1                          # sweeps 1, 3 and 5
    with pytest.raises(ValueError, match="detach the patient-group accumulator"):
        eng.set_region_sets([[0]])                                    # the sets are rows of the attached buffers
    with pytest.raises(ValueError, match="detach the patient-group accumulator"):
        eng.set_patient_groups([[0]])
    plain = stand_in_engine(64, 7, 6, attached=("patient_group",), groups=[[0, 1]])     # without sets: the regions alone, no contrast
    assert plain.patient_group_rows() == 7
    plain.run(0, 2, accumulate_from=0)
    assert [c[0] for c in plain.ctx.calls] == ["fcd_patient_groups_set", setter, setter]
    assert plain.ctx.calls[0][1][1:] == (0, 0)


# ---- the posterior's arithmetic on hand-made histograms ----

def hand_made_fit(sizes, contrasts, rows, seed):
    """A gibbs fit's results filled in by hand: random histograms whose joints have the groups' histograms as marginals."""
    import fcdiff_amd
    rng = np.random.default_rng(seed)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model = fcdiff_amd.UnsharedRegionModel()
    fit.bt = np.zeros((3, int(sum(sizes))))
    fit.method = "gibbs"
    total = 5000
    joints = []
    hg = np.zeros((len(sizes), rows, max(sizes) + 1), dtype=np.int64)
    for (a, b) in contrasts:
        cells = rng.integers(0, (sizes[a] + 1) * (sizes[b] + 1), size=(rows, total))
        h = np.stack([np.bincount(c, minlength=(sizes[a] + 1) * (sizes[b] + 1)) for c in cells])
        joints.append(h.reshape(rows, sizes[a] + 1, sizes[b] + 1))
        hg[a, :, :sizes[a] + 1] = joints[-1].sum(axis=2)
        hg[b, :, :sizes[b] + 1] = joints[-1].sum(axis=1)
    (fit.patient_group_hist, fit.patient_group_joint_hist, fit.patient_group_sweeps) = (hg, joints, 5)
    (fit.patient_group_names, fit.patient_group_sizes) = (["g%d" % j for j in range(len(sizes))], np.asarray(sizes))
    (fit.patient_group_rows, fit.patient_group_pairs) = ([str(n) for n in range(rows)], np.asarray(contrasts, dtype=np.int32))
    return fit, hg, joints, total


@pytest.mark.parametrize("level", [0.95, 0.5])
def test_posterior_arithmetic_on_hand_made_histograms(level):
    (sizes, contrasts, rows) = ([2, 4, 3, 7], [(0, 1), (2, 3)], 4)      # unequal sizes: 1/2 = 2/4, and 3 against 7 never tie inside
    (fit, hg, joints, total) = hand_made_fit(sizes, contrasts, rows, seed=11)
    out = fit.patient_group_posterior(level=level)
    assert out["names"] == ["g0", "g1", "g2", "g3"] and out["sizes"].tolist() == sizes
    assert out["row_names"] == ["0", "1", "2", "3"] and out["contrasts"] == [("g0", "g1"), ("g2", "g3")]
    nptest.assert_allclose(out["p_count"], hg / float(total), rtol=1e-15)
    nptest.assert_allclose(out["p_count"].sum(axis=2), 1.0, rtol=0, atol=1e-14)
    for (p, j) in enumerate(joints):
        nptest.assert_allclose(out["p_joint"][p], j / float(total), rtol=1e-15)
    want = PG.summaries(out["p_count"], out["p_joint"], sizes, contrasts, level)
    for key in ("prevalence", "p_greater", "p_less", "p_equal", "diff_mean"):
        nptest.assert_allclose(out[key], want[key], rtol=1e-13, atol=1e-15, err_msg=key)
    nptest.assert_array_equal(out["diff_interval"], want["diff_interval"])
    nptest.assert_allclose(out["p_greater"] + out["p_less"] + out["p_equal"], 1.0, rtol=0, atol=1e-14)
    assert out["p_equal"].shape == (2, rows) and out["diff_interval"].shape == (2, rows, 2)
    assert np.all(out["diff_interval"][:, :, 0] <= out["diff_mean"]) and np.all(out["diff_mean"] <= out["diff_interval"][:, :, 1])
    # the ties of the first contrast are (0, 0), (1, 2) and (2, 4), those of the second (0, 0) and (3, 7)
    nptest.assert_allclose(out["p_equal"][0], (joints[0][:, 0, 0] + joints[0][:, 1, 2] + joints[0][:, 2, 4]) / float(total), rtol=1e-13)
    nptest.assert_allclose(out["p_equal"][1], (joints[1][:, 0, 0] + joints[1][:, 3, 7]) / float(total), rtol=1e-13)


def test_posterior_of_point_masses_and_equal_rates_of_unequal_groups():
    """Sizes 3 and 9, every chain at (1, 3): the rates are equal -- 1/3 and 3/9 -- though the counts are not."""
    (fit, hg, joints, _total) = hand_made_fit([3, 9], [(0, 1)], 2, seed=3)
    joints[0][:] = 0
    joints[0][0, 1, 3] = 10                                           # row 0: equal rates
    joints[0][1, 2, 3] = 4                                            # row 1: 2/3 > 3/9 in 4 of 10, 0 < 1/9 in 6
    joints[0][1, 0, 1] = 6
    hg[:] = 0
    hg[0, :, :4] = joints[0].sum(axis=2)
    hg[1, :, :10] = joints[0].sum(axis=1)
    out = fit.patient_group_posterior()
    assert np.array_equal(out["p_equal"], [[1.0, 0.0]]) and np.array_equal(out["p_greater"], [[0.0, 0.4]])
    assert np.array_equal(out["p_less"], [[0.0, 0.6]])
    nptest.assert_allclose(out["prevalence"], [[1 / 3.0, 0.4 * 2 / 3.0], [1 / 3.0, (0.4 * 3 + 0.6) / 9.0]], rtol=1e-15)
    nptest.assert_allclose(out["diff_mean"], [[0.0, 0.4 * (2 / 3.0 - 3 / 9.0) - 0.6 / 9.0]], rtol=1e-14, atol=1e-17)
    assert np.array_equal(out["diff_interval"][0, 0], [0.0, 0.0])
    nptest.assert_array_equal(out["diff_interval"][0, 1], [-1 / 9.0, (2 * 9 - 3 * 3) / 27.0])
    nptest.assert_array_equal(fit.patient_group_posterior(level=0.1)["diff_interval"][0, 1], [-1 / 9.0, -1 / 9.0])


def test_fit_defaults_and_refusals_without_a_run():
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    assert fit.patient_groups is None and fit.patient_group_contrasts is None and fit.patient_groups_every == 1
    assert fit.patient_group_hist is None and fit.patient_group_joint_hist is None and fit.patient_group_sweeps == 0
    with pytest.raises(ValueError, match="call run"):
        fit.patient_group_posterior()                            # no model, no data
    fit.model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fit.model.sample_fast(5, 3, 4, seed=1)
    (fit.b, fit.bt) = (b, bt)
    with pytest.raises(ValueError, match="no patient groups"):
        fit.patient_group_posterior()                            # vb, no groups
    with pytest.raises(ValueError, match="no patient groups"):
        fit.patient_group_posterior(independent=True)
    fit.patient_groups = {"a": [0, 1], "b": [3]}
    with pytest.raises(ValueError):
        fit.patient_group_posterior()                            # vb without a run: no _lq_R
    with pytest.raises(ValueError, match="level"):
        fit.patient_group_posterior(level=1.0)
    fit.method = "gibbs"
    with pytest.raises(ValueError, match="set patient_groups before run"):
        fit.patient_group_posterior()                            # a gibbs run that did not set them left no histograms
    (fit.patient_group_names, fit.patient_group_sizes) = (["a", "b"], np.array([2, 1]))
    (fit.patient_group_rows, fit.patient_group_pairs) = (["0", "1"], np.zeros((0, 2), dtype=np.int32))
    (fit.patient_group_hist, fit.patient_group_joint_hist) = (np.zeros((2, 2, 3), dtype=np.int64), [])
    with pytest.raises(ValueError, match="no sweep was accumulated"):
        fit.patient_group_posterior()
    fit.patient_group_hist[0, :, 2] = 6
    fit.patient_group_hist[1, :, 0] = 6
    out = fit.patient_group_posterior()                          # no contrast: the per-group laws alone
    assert np.array_equal(out["prevalence"], [[1.0, 1.0], [0.0, 0.0]]) and out["p_joint"] == [] and out["contrasts"] == []
    assert out["p_greater"].shape == (0, 2) and out["diff_interval"].shape == (0, 2, 2)
    fit.method = "mcmc"
    with pytest.raises(ValueError, match="method"):
        fit.patient_group_posterior()


@pytest.mark.parametrize("knobs", [
    {"patient_groups": [[0, 1]], "patient_groups_every": 0},
    {"patient_groups": [[0, 1]], "patient_groups_every": 1.5},
    {"patient_groups": [[0, 4]]},                                                   # outside the 4 patients
    {"patient_groups": [[]]},
    {"patient_groups": [[0, 1], [1, 2]], "patient_group_contrasts": [(0, 1)]},      # overlapping
    {"patient_groups": {"a": [0], "b": [1]}, "patient_group_contrasts": [("a", "c")]},
    {"patient_groups": [[0, 1]], "n_chains": 1 << 22, "n_sweeps": 2000, "burn_in": 0},      # would overflow uint32
], ids=["every-0", "every-1.5", "index", "empty", "overlap", "unknown-name", "overflow"])
def test_fit_refuses_before_the_run(knobs):
    import fcdiff_amd
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    for (k, v) in knobs.items():
        setattr(fit, k, v)
    with pytest.raises(ValueError):
        fit._run_gibbs(5, 4)                                      # refused before any engine or device state is made


def test_shared_fit_refuses_patient_groups():
    import fcdiff_amd
    fit = fcdiff_amd.fit.SharedRegionFit()
    assert fit.patient_groups is None
    with pytest.raises(ValueError, match="population-level r"):
        fit.patient_group_posterior()                            # the query, with or without groups
    fit.model = fcdiff_amd.SharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = fcdiff_amd.UnsharedRegionModel().sample_fast(5, 3, 4, seed=1)
    (fit.b, fit.bt, fit.patient_groups) = (b, bt, [[0, 1], [2, 3]])
    for method in ("vb", "gibbs"):
        fit.method = method
        with pytest.raises(ValueError, match="population-level r"):
            fit.run()                                            # before any context or table is made
    assert fit._ctx is None and fit._d == {}


# ---- the knobs of the fit on a stand-in engine ----

class StubContext(object):
    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def check_device(self):
        pass


class PlainEngine(object):
    """What _run_gibbs needs of a sampler that has never heard of patient groups."""
    made = []

    def __init__(self, S_B, lM, N, U, n_chains, chain0=0, seed=0, edge_index="symmetric", ctx=None):
        import torch
        (self.Nreg, self.U, self.G, self.ctx) = (N, U, n_chains, ctx)
        self.cnt_f = torch.ones((N * (N - 1) // 2, 3), dtype=torch.int32)
        self.cnt_r = torch.ones((N, U), dtype=torch.int32)
        self.n_accumulated = 3
        (self.pair_acc, self.count_hist, self.coanomaly_acc, self.region_set_acc) = (None, None, None, None)
        self.log = []
        PlainEngine.made.append(self)

    def set_hyper(self, gamma, pi2):
        self.log.append("set_hyper")

    def init(self, pi):
        self.log.append("init")

    def hyper_values(self):
        return np.array([0.3, 0.4, 0.3]), 0.25


class GroupEngine(PlainEngine):
    """... and of one that has: the buffers hold known numbers, 'uint32' ones above 2^31 among them."""

    def set_patient_groups(self, groups, contrasts=None):
        self.log.append("set_patient_groups")
        (self.group_names, self.group_offsets, self.group_members) = gibbs.patient_groups_csr(groups, self.U)
        (self.group_contrasts, self.group_bin_offsets) = gibbs.patient_group_contrasts(contrasts, self.group_names,
                                                                                       self.group_offsets, self.group_members)

    def attach_patient_group_accumulator(self, every=1):
        import torch
        self.log.append(("attach_patient_group_accumulator", every))
        sizes = np.diff(self.group_offsets)
        rng = np.random.default_rng(1)
        hg = rng.integers(0, 1 << 32, size=(len(sizes), self.Nreg, int(sizes.max()) + 1), dtype=np.uint64).astype(np.uint32)
        hj = rng.integers(0, 1 << 32, size=max(1, self.Nreg * int(self.group_bin_offsets[-1])), dtype=np.uint64).astype(np.uint32)
        self.patient_group_acc = (torch.as_tensor(hg.view(np.int32)), torch.as_tensor(hj.view(np.int32)))
        self.patient_group_sweeps = 7

    def patient_group_row_names(self):
        return [str(n) for n in range(self.Nreg)]


def run_on(monkeypatch, engine, **knobs):
    import fcdiff_amd
    monkeypatch.setattr(fcdiff_amd.fit, "GibbsEngine", engine)
    monkeypatch.setattr(fcdiff_amd.fit, "run_chains", lambda eng, *args, **kw: eng.log.append("run_chains"))
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    (fit.model, fit.method, fit._ctx) = (fcdiff_amd.UnsharedRegionModel(), "gibbs", StubContext())
    (fit._d, fit.bt) = ({"S_B": None, "lM": None}, np.zeros((10, 6)))
    for (k, v) in knobs.items():
        setattr(fit, k, v)
    fit._run_gibbs(5, 6)
    return fit, engine.made[-1]


def test_fit_calls_nothing_while_patient_groups_is_none(monkeypatch):
    (fit, eng) = run_on(monkeypatch, PlainEngine)
    assert eng.log == ["set_hyper", "init", "run_chains"] and not hasattr(eng, "patient_group_acc")
    assert fit.patient_group_hist is None and fit.patient_group_joint_hist is None and fit.patient_group_sweeps == 0
    assert fit.patient_group_names is None and fit.patient_group_rows is None
    with pytest.raises(ValueError, match="set patient_groups before run"):
        fit.patient_group_posterior()


def test_fit_knobs_attach_pool_and_count_the_sweeps(monkeypatch):
    groups = {"treated": [0, 1, 2], "untreated": [3, 4], "all": list(range(6))}
    (fit, eng) = run_on(monkeypatch, GroupEngine, patient_groups=groups, patient_groups_every=3,
                        patient_group_contrasts=[("treated", "untreated"), (1, 0)])
    assert eng.log == ["set_patient_groups", ("attach_patient_group_accumulator", 3), "set_hyper", "init", "run_chains"]
    (hg, hj) = (b.numpy().view(np.uint32).astype(np.int64) for b in eng.patient_group_acc)
    assert fit.patient_group_hist.dtype == np.int64 and np.array_equal(fit.patient_group_hist, hg)     # uint32 values, not int32
    assert hg.max() > (1 << 31)
    assert [j.shape for j in fit.patient_group_joint_hist] == [(5, 4, 3), (5, 3, 4)]
    assert np.array_equal(fit.patient_group_joint_hist[0].reshape(-1), hj[:60])
    assert np.array_equal(fit.patient_group_joint_hist[1].reshape(-1), hj[60:])
    assert fit.patient_group_sweeps == 7
    assert fit.patient_group_names == ["treated", "untreated", "all"] and fit.patient_group_sizes.tolist() == [3, 2, 6]
    assert fit.patient_group_rows == ["0", "1", "2", "3", "4"] and fit.patient_group_pairs.tolist() == [[0, 1], [1, 0]]
    fit.patient_groups = None                                        # a second run of the same fit without the knob forgets them
    fit._run_gibbs(5, 6)
    assert fit.patient_group_hist is None and fit.patient_group_joint_hist is None and fit.patient_group_sweeps == 0
    assert GroupEngine.made[-1].log == ["set_hyper", "init", "run_chains"]
    (fit, eng) = run_on(monkeypatch, GroupEngine, patient_groups=[[0], [5]])               # no contrast: a placeholder word
    assert eng.patient_group_acc[1].numel() == 1 and fit.patient_group_joint_hist == []
