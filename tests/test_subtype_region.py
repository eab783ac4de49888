"""
The subtype-region model without a GPU: the NumPy reference of tests/subtype_region_ref.py on a planted case (labels
recovered from every restart, the energy never rises -- neither over the loop nor over the responsibility step alone), its
bound against the exact evidence of a tiny model, its invariance under a permutation of the starting labels, and the host
side of the product: SubtypeRegionModel.sample, the refusals of SubtypeRegionFit, the `weights` argument of tables.build and
the binding of the two entry points.
"""
import ctypes as C

import numpy as np
import numpy.testing as nptest
import pytest
import torch

import fcdiff_amd
import subtype_region_ref as R
from conftest import theta_dict
from fcdiff_amd import _lib, tables
from fcdiff_amd.fit import SubtypeRegionFit

PLANTED_LABELS = [0] * 12 + [1] * 12


@pytest.fixture(scope="module")
def planted():
    """The planted case: 12 regions, 24 controls, two subtypes of 12 patients; four seeded restarts of 30 iterations."""
    m = fcdiff_amd.GroupedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample(12, 24, PLANTED_LABELS, seed=0)
    th = theta_dict(m.theta())
    (S_B, lM) = R.tables(b, bt, th)
    fits = [R.vb_fit(S_B, lM, R.default_init(24, 2, 0, i), th["pi"], th["gamma"], alpha=1.0, iters=30) for i in range(4)]
    return dict(S_B=S_B, lM=lM, theta=th, fits=fits)


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_recovers_the_planted_labels_from_every_restart(planted):
    truth = np.array(PLANTED_LABELS)
    for out in planted["fits"]:
        labels = out["resp"].argmax(axis=1)
        assert max((labels == truth).sum(), (labels == 1 - truth).sum()) == 24
    finals = np.array([out["energy"][-1] for out in planted["fits"]])
    nptest.assert_allclose(finals, finals[0], rtol=1e-9)               # one optimum, whatever the start
    nptest.assert_allclose(finals[0], -5327.1261, atol=1e-3)


def test_reference_energy_never_rises(planted):
    for out in planted["fits"]:
        e = out["energy"]
        assert np.all(np.diff(e) <= 1e-9 * np.abs(e[:-1]))              # slack for rounding only
        steps = out["steps"]                                            # (iters, 5): every step of every iteration
        assert np.all(np.diff(steps, axis=1) <= 1e-9 * np.abs(steps[:, :-1]))


def test_responsibility_step_alone_never_raises_the_energy(planted):
    for out in planted["fits"]:
        (before, after) = (out["steps"][:, 3], out["steps"][:, 4])
        assert np.all(after - before <= 1e-9 * np.abs(before))
    # ... and from states the loop does not visit: the step at random q_R and responsibilities
    rng = np.random.default_rng(5)
    (S_B, lM, th) = (planted["S_B"], planted["lM"], planted["theta"])
    out = planted["fits"][0]
    for _ in range(3):
        p = rng.random((12, 2, 1))
        lq_R = np.log(np.concatenate([1 - p, p], axis=2))
        s = rng.dirichlet(np.ones(2), size=24)
        e0 = R.energy(out["lq_F"], lq_R, S_B, lM, s, th["gamma"], th["pi"], 1.0)
        s1 = R.softmax(R.expected_loglik(out["lq_F"], lq_R, lM) + R.E_ln_rho(s.sum(axis=0), 1.0)[None, :])
        e1 = R.energy(out["lq_F"], lq_R, S_B, lM, s1, th["gamma"], th["pi"], 1.0)
        assert e1 - e0 <= 1e-9 * abs(e0)


def test_reference_elbo_is_below_the_exact_evidence():
    """N = 3, H = 3, U = 4, G = 2: 27 x 64 x 16 states."""
    m = fcdiff_amd.GroupedRegionModel()
    m.pi = 0.3
    (_r, _t, _f, _ft, b, bt) = m.sample(3, 3, [0, 0, 1, 1], seed=4)
    th = theta_dict(m.theta())
    (S_B, lM) = R.tables(b, bt, th)
    # pi and gamma are held: with three edges the gamma step puts a type at exactly 0, the 0 ln 0 of the inherited energy.
    # With theta held every iterate of every restart bounds the same number.
    exact = R.exact_log_evidence(b, bt, 2, m.theta(), alpha=1.0)
    for i in range(4):
        out = R.vb_fit(S_B, lM, R.default_init(4, 2, 0, i), th["pi"], th["gamma"], alpha=1.0, iters=20, update_theta=False)
        assert np.all(np.isfinite(out["energy"]))
        assert np.all(-out["energy"] <= exact + 1e-9 * abs(exact))
        assert exact + out["energy"][-1] < 0.5 * abs(exact)             # ... and is not a trivial one


def test_permuted_start_gives_the_permuted_result_and_the_same_one_after_renumbering():
    labels = [0] * 10 + [1] * 14                                         # unequal sizes: no tie in the renumbering
    m = fcdiff_amd.GroupedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample(12, 24, labels, seed=0)
    th = theta_dict(m.theta())
    (S_B, lM) = R.tables(b, bt, th)
    s0 = R.default_init(24, 2, 3, 0)
    a = R.vb_fit(S_B, lM, s0, th["pi"], th["gamma"], iters=12)
    p = R.vb_fit(S_B, lM, s0[:, ::-1], th["pi"], th["gamma"], iters=12)
    tol = dict(rtol=1e-9, atol=1e-12)                                    # the sums over subtypes run in the other order
    nptest.assert_allclose(p["resp"], a["resp"][:, ::-1], **tol)
    nptest.assert_allclose(p["lq_R"], a["lq_R"][:, ::-1], **tol)
    nptest.assert_allclose(p["energy"], a["energy"], rtol=1e-12)
    (ra, rp) = (R.renumbered(a), R.renumbered(p))
    assert list(ra["order"]) == list(rp["order"])[::-1]
    nptest.assert_allclose(rp["resp"], ra["resp"], **tol)
    nptest.assert_allclose(rp["lq_R"], ra["lq_R"], **tol)
    n = ra["resp"].sum(axis=0)
    assert n[0] >= n[1] and list(ra["resp"].argmax(axis=1)) == [1] * 10 + [0] * 14


# ------------------------------------------------------------------------------------------------ the model
def test_sample_with_one_subtype_is_the_shared_draw():
    m = fcdiff_amd.SubtypeRegionModel()
    m.n_subtypes = 1
    out = m.sample(5, 3, 6, seed=9)
    want = fcdiff_amd.SharedRegionModel().sample(5, 3, 6, seed=9)
    assert len(out) == 7 and list(out[0]) == [0] * 6
    nptest.assert_array_equal(out[1][:, 0], want[0])
    for (got, ref) in zip(out[2:], want[1:]):
        nptest.assert_array_equal(got, ref)


def test_sample_is_the_grouped_draw_of_its_labels():
    m = fcdiff_amd.SubtypeRegionModel()
    (m.n_subtypes, m.rho, m.pi) = (3, [0.5, 0.25, 0.25], 0.2)
    out = m.sample(6, 4, 30, seed=2, sessions=2)
    z = out[0]
    assert z.shape == (30,) and z.dtype == np.int64 and set(z.tolist()) == {0, 1, 2}
    g = fcdiff_amd.GroupedRegionModel()
    g.pi = 0.2
    want = g.sample(6, 4, z.tolist(), seed=2, sessions=2)
    for (got, ref) in zip(out[1:], want):
        nptest.assert_array_equal(got, ref)
    assert out[6].shape == (15, 30, 2)
    for bad in ([0.5, 0.5], [0.5, 0.6, -0.1], [0.2, 0.2, 0.2]):
        m.rho = bad
        with pytest.raises(ValueError):
            m.sample(6, 4, 30)
    assert "SubtypeRegionModel" in fcdiff_amd.__all__ and "n_subtypes = 3" in str(m)


# ------------------------------------------------------------------------------------------------ the fit's refusals
def new_fit(U=6, **kw):
    fit = SubtypeRegionFit()
    fit.model = fcdiff_amd.SubtypeRegionModel()
    (_z, _r, _t, _f, _ft, fit.b, fit.bt) = fit.model.sample(5, 3, U, seed=1)
    fit.n_subtypes = 2
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


def test_defaults():
    fit = SubtypeRegionFit()
    assert (fit.rho_concentration, fit.n_restarts, fit.init_responsibilities, fit.seed) == (1.0, 4, None, 0)
    assert fit.edge_index == "symmetric" and fit.method == "vb" and fit.n_subtypes is None
    assert fcdiff_amd.fit.SUBTYPE_MAX == tables.SUBTYPE_MAX == 8


@pytest.mark.parametrize("kw, exc, match", [
    (dict(method="gibbs"), NotImplementedError, "sampler"),
    (dict(update_theta_sub=True), NotImplementedError, "theta_sub"),
    (dict(edge_index="reference"), ValueError, "symmetric"),
    (dict(patient_groups=[[0, 1]]), ValueError, "patient_groups"),
    (dict(patient_traits=[[0.0] * 6]), ValueError, "patient_traits"),
    (dict(n_subtypes=0), ValueError, "n_subtypes"),
    (dict(n_subtypes=7), ValueError, "n_subtypes"),                    # more than U = 6
    (dict(n_subtypes=None), ValueError, "n_subtypes"),
    (dict(n_subtypes=2.5), ValueError, "n_subtypes"),
    (dict(rho_concentration=0.0), ValueError, "rho_concentration"),
    (dict(n_restarts=0), ValueError, "n_restarts"),
    (dict(init_responsibilities=np.full((6, 3), 1 / 3)), ValueError, "shape"),
    (dict(init_responsibilities=np.array([[1.5, -0.5]] * 6)), ValueError, ">= 0"),
    (dict(init_responsibilities=np.array([[np.nan, 0.5]] * 6)), ValueError, "finite"),
    (dict(init_responsibilities=np.array([[0.5, 0.4]] * 6)), ValueError, "sum to 1"),
])
def test_run_refusals_come_before_any_device_work(kw, exc, match):
    fit = new_fit(**kw)
    with pytest.raises(exc, match=match):
        fit.run()
    assert fit._ctx is None


def test_more_than_eight_subtypes_are_refused():
    fit = new_fit(U=12, n_subtypes=9)
    with pytest.raises(ValueError, match="n_subtypes"):
        fit.run()


def test_queries_that_are_not_provided_say_why():
    fit = new_fit()
    for (call, word) in ((lambda: fit.score(fit.bt), "assign"), (lambda: fit.membership(fit.bt), "sampler"),
                         (fit.log_evidence, "ELBO")):
        with pytest.raises(NotImplementedError, match=word):
            call()
    for call in (fit.patient_group_posterior, fit.patient_trait_posterior):
        with pytest.raises(ValueError, match="subtypes"):
            call()
    for call in (fit.subtype_posterior, fit.region_posterior, fit.connection_posterior, lambda: fit.assign(fit.bt)):
        with pytest.raises(ValueError, match="run"):
            call()


# ------------------------------------------------------------------------------------------------ the binding
def test_entry_points_are_declared_exported_and_bound():
    for (name, n_args) in (("fcd_lik_weighted_tables", 7), ("fcd_vb_subtype_loglik", 8)):
        (res, args) = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args + 1                # the context in front
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    assert _lib.SIGNATURES["fcd_lik_weighted_tables"][1][3:6] == [C.c_int64] * 3
    assert _lib.SIGNATURES["fcd_vb_subtype_loglik"][1][4:7] == [C.c_int64] * 3
    assert _lib.ABI_VERSION == 4 and fcdiff_amd.fit.SubtypeRegionFit is SubtypeRegionFit


class Recorder(object):
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))


@pytest.fixture()
def no_stream(monkeypatch):
    monkeypatch.setattr(_lib, "stream_ptr", lambda: C.c_void_p(0))


def weights_case(sessions=None):
    (_z, _r, _t, _f, _ft, b, bt) = fcdiff_amd.SubtypeRegionModel().sample(5, 3, 7, seed=3, sessions=sessions)
    lM_u = torch.zeros((10, 7, 3, 3), dtype=torch.float64)
    resp = torch.full((7, 3), 1 / 3, dtype=torch.float64)
    return torch.as_tensor(b), torch.as_tensor(bt), lM_u, resp, fcdiff_amd.SubtypeRegionModel().theta()


@pytest.mark.parametrize("sessions", [None, 2])
def test_build_with_weights_argument_positions(no_stream, sessions):
    rec = Recorder()
    (b, bt, lM_u, resp, theta) = weights_case(sessions)
    S_in = torch.zeros((10, 3), dtype=torch.float64)
    (S_B, L) = tables.build(rec, b, bt, theta, 0, S_B=S_in, weights=(lM_u, resp))
    assert S_B is S_in and tuple(L.shape) == (10, 3, 3, 3) and L.dtype == torch.float64
    ((name, args),) = rec.calls                                          # ONE call: the data is not read again
    assert name == "fcd_lik_weighted_tables" and len(args) == 7
    assert (args[0].value, args[1].value, args[5].value) == (lM_u.data_ptr(), resp.data_ptr(), L.data_ptr())
    assert args[2:5] == (10, 7, 3)
    (_S, L2) = tables.build(rec, b, bt, theta, 0, lM=L, weights=(lM_u, resp))          # written in place where given
    assert L2 is L and rec.calls[1][1][5].value == L.data_ptr()


def test_build_with_weights_refusals(no_stream):
    rec = Recorder()
    (b, bt, lM_u, resp, theta) = weights_case()
    order = torch.arange(7, dtype=torch.int32)
    offsets = torch.as_tensor([0, 7], dtype=torch.int64)
    f64 = torch.float64
    bad = [dict(shared=True), dict(groups=(order, offsets, 1)), dict(lpB=torch.empty((10, 3, 3), dtype=f64)),
           dict(pBt=torch.empty((10, 7, 3), dtype=f64)), dict(n_missing=torch.zeros(2, dtype=torch.int64)),
           dict(lM=torch.empty((10, 7, 3, 3), dtype=f64)), dict(lM=torch.empty((10, 3, 3, 3), dtype=torch.float32)),
           dict(weights=(lM_u[:, :6], resp)), dict(weights=(lM_u.float(), resp)), dict(weights=(lM_u, resp[:6])),
           dict(weights=(lM_u, resp.float())), dict(weights=(lM_u, torch.full((7, 9), 1 / 9, dtype=f64))),
           dict(weights=(lM_u, torch.empty((7, 0), dtype=f64))), dict(weights=(lM_u,)), dict(weights=(lM_u, resp[:, 0]))]
    for kw in bad:
        kw.setdefault("weights", (lM_u, resp))
        with pytest.raises(ValueError):
            tables.build(rec, b, bt, theta, 0, **kw)
    assert rec.calls == []
