"""
The grouped-region model on the host: the label rules of group_labels_csr, the law of GroupedRegionModel.sample, the
enumeration of tests/grouped_region_ref.py against its two degenerate forms, the binding of fcd_lik_grouped_tables, the
arguments tables.build(groups=...) passes (through a context that records its calls, as test_host_plumbing.py) and what
GroupedRegionFit refuses before any context exists.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest
import torch

import fcdiff_amd
from fcdiff_amd import _lib, tables, util
from fcdiff_amd.fit import GroupedRegionFit, group_labels_csr
from oracle import fcdiff_oracle as O

import evidence_ref as ER
import grouped_region_ref as GR
import shared_region_ref as SR

# argument positions of fcd_lik_grouped_tables after the entry point's name (include/fcdiff_hip.h, without the context)
GP = {"C": 2, "H": 3, "U": 4, "K": 5, "theta": 6, "var_b": 7, "var_bt": 8, "order": 9, "offsets": 10, "G": 11, "S_B": 12,
      "lM": 13, "flags": 14, "n_missing": 15, "n_args": 17}


# ------------------------------------------------------------------------------------------------ labels
def test_group_labels_csr_rules():
    (names, offsets, order) = group_labels_csr([2, 0, 1, 0, 2, 2, 0], 7)
    assert names == [0, 1, 2]
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 3, 4, 7]
    assert order.dtype == np.int32 and order.tolist() == [1, 3, 6, 2, 0, 4, 5]          # members in ascending patient index
    (names, offsets, order) = group_labels_csr(np.array(["b", "a", "b"]), 3)
    assert names == ["a", "b"] and offsets.tolist() == [0, 1, 3] and order.tolist() == [1, 0, 2]
    (names, offsets, order) = group_labels_csr(np.arange(5)[::-1], 5)
    assert names == [0, 1, 2, 3, 4] and offsets.tolist() == [0, 1, 2, 3, 4, 5] and order.tolist() == [4, 3, 2, 1, 0]
    (names, offsets, order) = group_labels_csr(["x"] * 4, 4)
    assert names == ["x"] and offsets.tolist() == [0, 4] and order.tolist() == [0, 1, 2, 3]
    assert sorted(order.tolist()) == list(range(4))


@pytest.mark.parametrize("labels,U", [([0, 1], 3), ([0, 1, 2, 3], 3), ([[0, 1], [1, 0]], 2), ("ab", 2), (3, 1),
                                      ([0, None, 1], 3), ([0.0, np.nan, 1.0], 3), ([0, "a", 1], 3), ([0.5, 1.5], 2),
                                      ([True, False], 2)])
def test_group_labels_csr_refusals(labels, U):
    with pytest.raises(ValueError):
        group_labels_csr(labels, U)


# ------------------------------------------------------------------------------------------------ the model's sample
def grouped_model():
    m = fcdiff_amd.GroupedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.gamma, m.mu, m.sigma = np.array([0.2, 0.5, 0.3]), np.array([-0.5, 0, 0.5]), np.ones(3) * 0.05
    return m


def test_sample_columns_of_a_group_share_r():
    m = grouped_model()
    (N, H) = (120, 3)
    labels = ["b", "a", "c", "a", "b", "b", "c", "a"] * 6
    U = len(labels)
    (r, t, f, ft, b, bt) = m.sample(N, H, labels, seed=5)
    Ce = util.N_to_C(N)
    assert r.shape == (N, 3) and r.dtype == bool and t.shape == (Ce, U) and f.shape == (Ce, 3) and ft.shape == (Ce, U, 3)
    assert b.shape == (Ce, H) and bt.shape == (Ce, U)
    nptest.assert_allclose(r.mean(), 0.3, atol=5 * np.sqrt(0.21 / (3 * N)))
    assert not np.array_equal(r[:, 0], r[:, 1]) and not np.array_equal(r[:, 1], r[:, 2])
    ends = np.array([util.c_to_nm(c) for c in range(Ce)])
    gof = np.array(["abc".index(v) for v in labels])
    ru = r[:, gof]                                                   # the patients read their group's column
    (rn, rm) = (ru[ends[:, 0]], ru[ends[:, 1]])
    assert t[rn & rm].all() and not t[~rn & ~rm].any()               # concordant pairs follow the GROUP's r in every patient
    nptest.assert_allclose(t[rn ^ rm].mean(), 0.4, atol=0.01)
    (fk, ftk) = (np.argmax(f, axis=1), np.argmax(ft, axis=2))
    same = ftk == fk[:, None]
    nptest.assert_allclose(same[~t].mean(), 0.8, atol=0.01)
    nptest.assert_allclose(same[t].mean(), 0.2, atol=0.01)
    for k in range(3):
        nptest.assert_allclose(bt[ftk == k].mean(), m.mu[k], atol=0.01)
    again = m.sample(N, H, labels, seed=5)
    assert all(np.array_equal(x, y) for (x, y) in zip(again, (r, t, f, ft, b, bt)))


def test_sample_with_one_label_is_the_shared_models_sample():
    (m, s) = (grouped_model(), fcdiff_amd.SharedRegionModel())
    for k in ("pi", "eta", "epsilon", "gamma", "mu", "sigma"):
        setattr(s, k, getattr(m, k))
    got = m.sample(30, 4, [7] * 9, seed=11)
    want = s.sample(30, 4, 9, seed=11)
    assert got[0].shape == (30, 1)
    nptest.assert_array_equal(got[0][:, 0], want[0])
    for (x, y) in zip(got[1:], want[1:]):
        nptest.assert_array_equal(x, y)


def test_sample_with_sessions():
    m = grouped_model()
    labels = [0, 1, 1, 0, 2]
    (r, t, f, ft, b, bt) = m.sample(6, 2, labels, seed=2, sessions=4)
    assert bt.shape == (15, 5, 4) and ft.shape == (15, 5, 3) and r.shape == (6, 3) and b.shape == (15, 2)
    one = m.sample(6, 2, labels, seed=2)
    for (x, y) in zip((r, t, f, ft, b), one[:5]):                    # the sessions are drawn last
        nptest.assert_array_equal(x, y)
    assert one[5].shape == (15, 5)
    with pytest.raises(ValueError):
        m.sample(6, 2, labels, sessions=0)


# ------------------------------------------------------------------------------------------------ the enumeration
def small_case(N, H, U, seed, missing=False):
    m = fcdiff_amd.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.1
    m.sigma = np.array([0.06, 0.06, 0.08])
    (_r, _t, _f, _ft, b, bt) = m.sample(N, H, U, seed=seed)
    if missing:
        bt = bt.copy()
        bt[0, 0] = np.nan
    return m, b, bt


@pytest.mark.parametrize("missing", [False, True])
def test_enumeration_with_one_label_is_the_shared_enumeration(missing):
    (m, b, bt) = small_case(3, 2, 3, 31, missing)
    got = GR.enumerate_posterior(b, bt, ["g"] * 3, m.theta(), missing=missing)
    want = SR.enumerate_posterior(b, bt, m.theta(), missing=missing)
    nptest.assert_allclose(got["logjoint"], want["logjoint"], rtol=0, atol=1e-12 * np.abs(want["logjoint"]).max())
    assert abs(got["log_evidence"] - want["log_evidence"]) < 1e-12 * abs(want["log_evidence"])
    nptest.assert_allclose(got["p_r"][:, 0], want["p_r"], atol=1e-13)
    nptest.assert_allclose(got["p_group_count"][0], want["p_count"], atol=1e-13)
    for key in ("p_f", "p_T", "p_Ft", "p_changed"):
        nptest.assert_allclose(got[key], want[key], atol=1e-13, err_msg=key)


def test_enumeration_with_distinct_labels_is_the_unshared_enumeration():
    (m, b, bt) = small_case(3, 2, 2, 17)
    got = GR.enumerate_posterior(b, bt, [0, 1], m.theta())
    (lpB, _pBt, lM) = O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    want = ER.exact_log_evidence(lpB.sum(axis=1), lM, np.asarray(m.gamma, dtype=np.float64), m.pi2())
    assert abs(got["log_evidence"] - want) < 1e-12 * abs(want)
    # the laws are laws, and the per-region joint of two groups has the marginals
    nptest.assert_allclose(got["p_group_count"].sum(axis=1), 1.0, atol=1e-12)
    nptest.assert_allclose(got["p_region_count"].sum(axis=1), 1.0, atol=1e-12)
    nptest.assert_allclose(got["p_pair"][0, 1].sum(axis=(1, 2)), 1.0, atol=1e-12)
    nptest.assert_allclose(got["p_pair"][0, 1][:, 1, :].sum(axis=1), got["p_r"][:, 0], atol=1e-12)
    nptest.assert_allclose(got["p_pair"][0, 1][:, :, 1].sum(axis=1), got["p_r"][:, 1], atol=1e-12)
    nptest.assert_allclose((got["p_group_count"] * np.arange(4)).sum(axis=1), got["p_r"].sum(axis=0), atol=1e-12)


def test_enumeration_of_a_permuted_cohort_permutes_the_patients():
    (m, b, bt) = small_case(3, 2, 3, 23)
    a = GR.enumerate_posterior(b, bt, ["x", "y", "x"], m.theta())
    perm = [1, 2, 0]
    p = GR.enumerate_posterior(b, bt[:, perm], ["y", "x", "x"], m.theta())
    assert abs(a["log_evidence"] - p["log_evidence"]) < 1e-12 * abs(a["log_evidence"])
    nptest.assert_allclose(p["p_r"], a["p_r"], atol=1e-13)
    nptest.assert_allclose(p["p_T"], a["p_T"][:, perm], atol=1e-13)


# ------------------------------------------------------------------------------------------------ the binding
def test_entry_point_is_declared_exported_and_bound():
    assert "fcd_lik_grouped_tables" in _lib.SIGNATURES
    (res, args) = _lib.SIGNATURES["fcd_lik_grouped_tables"]
    assert res is C.c_int and len(args) == GP["n_args"] + 1          # the context in front
    assert args[GP["G"] + 1] is C.c_int64 and args[GP["flags"] + 1] is C.c_int
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "fcd_lik_grouped_tables")
    assert _lib.ABI_VERSION == 4
    assert "GroupedRegionModel" in fcdiff_amd.__all__ and fcdiff_amd.fit.GroupedRegionFit is GroupedRegionFit


class Recorder(object):
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))

    def take(self):
        (calls, self.calls) = (self.calls, [])
        return calls


@pytest.fixture()
def no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "stream_ptr", lambda: C.c_void_p(0))


def address(arg):
    return arg.value or 0


def csr_tensors(labels):
    (names, offsets, order) = group_labels_csr(labels, len(labels))
    return torch.as_tensor(order), torch.as_tensor(offsets), len(names)


@pytest.mark.parametrize("sessions", [None, 3])
@pytest.mark.parametrize("noise", [False, True])
def test_build_with_groups_argument_positions(no_stream, sessions, noise):
    rec = Recorder()
    labels = [2, 0, 1, 0, 2, 2, 0]
    (_r, _t, _f, _ft, b, bt) = fcdiff_amd.GroupedRegionModel().sample(5, 3, labels, seed=3, sessions=sessions)
    (b, bt) = (torch.as_tensor(b), torch.as_tensor(bt))
    (order, offsets, G) = csr_tensors(labels)
    theta = fcdiff_amd.GroupedRegionModel().theta()
    (vb, vbt) = (torch.full((3,), 0.01, dtype=torch.float64), torch.full((7, sessions or 1), 0.02, dtype=torch.float64))
    n = torch.zeros(2, dtype=torch.int64)
    kw = {"noise": (vb, vbt)} if noise else {}
    (S_B, lM) = tables.build(rec, b, bt, theta, _lib.FCD_DATA_NAN_MISSING, n_missing=n, groups=(order, offsets, G), **kw)
    assert tuple(S_B.shape) == (10, 3) and tuple(lM.shape) == (10, 3, 3, 3) and lM.dtype == torch.float64
    ((name, args),) = rec.take()
    assert name == "fcd_lik_grouped_tables" and len(args) == GP["n_args"]
    assert (address(args[0]), address(args[1])) == (b.data_ptr(), bt.data_ptr())
    assert args[GP["C"]:GP["K"] + 1] == (10, 3, 7, sessions or 1)
    assert [float(x) for x in args[GP["theta"]][0:12]] == [float(x) for x in theta]
    assert (address(args[GP["var_b"]]), address(args[GP["var_bt"]])) == ((vb.data_ptr(), vbt.data_ptr()) if noise else (0, 0))
    assert (address(args[GP["order"]]), address(args[GP["offsets"]]), args[GP["G"]]) == (order.data_ptr(), offsets.data_ptr(), 3)
    assert (address(args[GP["S_B"]]), address(args[GP["lM"]])) == (S_B.data_ptr(), lM.data_ptr())
    assert args[GP["flags"]] == _lib.FCD_DATA_NAN_MISSING and address(args[GP["n_missing"]]) == n.data_ptr()
    # buffers given are written in place
    (S2, lM2) = tables.build(rec, b, bt, theta, 0, S_B=S_B, lM=lM, groups=(order, offsets, G), **kw)
    assert S2 is S_B and lM2 is lM and address(rec.take()[0][1][GP["n_missing"]]) == 0


def test_build_with_groups_refusals(no_stream):
    rec = Recorder()
    labels = [0, 1, 0, 1]
    (_r, _t, _f, _ft, b, bt) = fcdiff_amd.GroupedRegionModel().sample(5, 3, labels, seed=3)
    (b, bt) = (torch.as_tensor(b), torch.as_tensor(bt))
    (order, offsets, G) = csr_tensors(labels)
    theta = fcdiff_amd.GroupedRegionModel().theta()
    bad = [dict(shared=True), dict(lpB=torch.empty((10, 3, 3), dtype=torch.float64)),
           dict(pBt=torch.empty((10, 4, 3), dtype=torch.float64)), dict(lM=torch.empty((10, 4, 3, 3), dtype=torch.float64))]
    for kw in bad:
        with pytest.raises(ValueError):
            tables.build(rec, b, bt, theta, 0, groups=(order, offsets, G), **kw)
    for groups in ((order, offsets, 0), (order, offsets, 5), (order.to(torch.int64), offsets, G), (order[:3], offsets, G),
                   (order, offsets.to(torch.int32), G), (order, offsets[:2], G)):
        with pytest.raises(ValueError):
            tables.build(rec, b, bt, theta, 0, groups=groups)
    assert rec.take() == []


def test_fit_issues_the_grouped_call_and_keeps_its_buffers(no_stream):
    (N, H) = (5, 3)
    labels = ["b", "a", "b", "c"]
    fit = GroupedRegionFit()
    rec = fit._ctx = Recorder()
    fit.model = fcdiff_amd.GroupedRegionModel()
    (_r, _t, _f, _ft, fit.b, fit.bt) = fit.model.sample(N, H, labels, seed=3)
    fit.group_labels = labels
    fit._init_lps(N, H, 4)
    assert rec.take() == []
    assert tuple(fit._d["lM"].shape) == (10, 3, 3, 3) and tuple(fit._d["lq_R"].shape) == (N, 3, 2)
    kept = (fit._d["S_B"].data_ptr(), fit._d["lM"].data_ptr())
    for _ in range(2):
        fit._update_lps()
        ((name, args),) = rec.take()
        assert name == "fcd_lik_grouped_tables" and args[GP["C"]:GP["K"] + 1] == (10, H, 4, 1) and args[GP["G"]] == 3
        assert (address(args[GP["S_B"]]), address(args[GP["lM"]])) == kept
    fit._tables(full=True)                                        # no per-item tables: still the one call
    assert [c[0] for c in rec.take()] == ["fcd_lik_grouped_tables"] and fit._d["lpB"] is None and fit._d["pBt"] is None
    (order, offsets, group_of, G) = fit._groups_dev()
    assert order.tolist() == [1, 0, 2, 3] and offsets.tolist() == [0, 1, 3, 4] and group_of.tolist() == [1, 0, 1, 2] and G == 3
    W = torch.arange(10 * 3 * 9, dtype=torch.float64).reshape(10, 3, 3, 3)
    nptest.assert_array_equal(fit._expand_weights(W).numpy(), W.numpy()[:, [1, 0, 1, 2]])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture()
def no_context(monkeypatch):
    def refuse(*_a, **_k):
        raise AssertionError("a context was made before the refusal")
    monkeypatch.setattr(_lib, "Context", refuse)


def grouped_fit(labels=(0, 1, 0, 1), **kw):
    fit = GroupedRegionFit()
    fit.model = fcdiff_amd.GroupedRegionModel()
    (_r, _t, _f, _ft, fit.b, fit.bt) = fit.model.sample(4, 2, list(labels), seed=1)
    fit.group_labels = list(labels)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


@pytest.mark.parametrize("kw", [
    dict(group_labels=None), dict(group_labels=[0, 1, 0]), dict(group_labels=[0, None, 0, 1]),
    dict(group_labels=[0.0, np.nan, 0.0, 1.0]), dict(edge_index="reference"), dict(edge_index="other"),
    dict(patient_groups=[[0], [1]]), dict(patient_group_contrasts=[(0, 1)]), dict(patient_traits=[[0.0, 1.0]]),
    dict(group_contrasts=[(0, 2)]), dict(group_contrasts=[(0, 0)]), dict(group_contrasts=[(0, 1), (0, 1)]),
    dict(group_contrasts=[(0, 1, 0)]),
    dict(group_labels=list(range(4)), group_contrasts=[(a, b) for a in range(4) for b in range(4) if a != b] * 6),
    dict(method="gibbs", group_contrasts=[(0, 2)]), dict(bt_noise_var=[-1.0, 0, 0, 0]),
])
def test_run_refuses_on_the_host_before_a_context_exists(no_context, kw):
    fit = grouped_fit(**kw)
    with pytest.raises(ValueError):
        fit.run()
    assert fit._ctx is None


def test_theta_sub_stays_refused_with_sessions_and_noise(no_context):
    fit = grouped_fit(update_theta_sub=True, bt_noise_var=np.zeros(4))
    with pytest.raises(NotImplementedError, match="noise"):
        fit.run()
    fit = grouped_fit(update_theta_sub=True)
    fit.bt = np.repeat(fit.bt[:, :, None], 2, axis=2)
    with pytest.raises(NotImplementedError, match="sessions"):
        fit.run()


def test_score_and_membership_are_not_provided(no_context):
    fit = grouped_fit()
    with pytest.raises(NotImplementedError, match="separate question"):
        fit.score(fit.bt)
    with pytest.raises(NotImplementedError, match="separate question"):
        fit.membership(fit.bt)
    with pytest.raises(ValueError):
        fit.patient_group_posterior()
    with pytest.raises(ValueError):
        fit.patient_trait_posterior()
    with pytest.raises(ValueError):
        fit.group_contrast_posterior()                               # before run()
    with pytest.raises(ValueError):
        fit.region_posterior()
    assert fit._edge_mode() == "symmetric"


def test_the_other_fits_keep_their_patient_extent():
    assert fcdiff_amd.fit.UnsharedRegionFit()._patient_extent(7) == 7
    assert fcdiff_amd.fit.SharedRegionFit()._patient_extent(7) == 1
    assert grouped_fit()._patient_extent(4) == 2
    assert fcdiff_amd.fit.UnsharedRegionFit()._groups_kw() == {} and fcdiff_amd.fit.SharedRegionFit()._groups_kw() == {}
