"""
The oracle of the partial correlations (tests/partial_corr_ref.py) against independent routes, the rules it restates, the
argument checks of fcdiff_amd.corr that need no device, and sampling_variance(n_conditioned=).  No GPU.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import partial_corr_ref as PR
from fcdiff_amd import corr
from oracle import fcdiff_oracle as O

SHAPES = [(5, 40), (17, 30), (33, 20)]


def independent(x, alpha):
    """rho of one subject by numpy.corrcoef and numpy.linalg.inv (all rows live)."""
    R = np.corrcoef(x)
    p = R.shape[0]
    Th = np.linalg.inv((1.0 - alpha) * R + alpha * np.eye(p))
    d = np.sqrt(np.diag(Th))
    rho = -Th / d[:, None] / d[None, :]
    ends = O.edge_endpoints(p)
    return rho[ends[:, 0], ends[:, 1]]


@pytest.mark.parametrize("pn", SHAPES, ids=lambda v: "p%d-n%d" % v)
def test_oracle_against_numpy_inv(pn):
    (p, n) = pn
    x = PR.make_series(10 + p, 1, p, n)[0]
    for sh in ("ledoit_wolf", 0.1, 0.5, 1.0) + ((0.0,) if n >= 4 * p else ()):
        r = PR.partial_corr_subject(x, sh)
        assert r["status"] == PR.OK and r["n_live"] == p
        exp = independent(x, r["alpha"])
        # numpy.linalg.inv in fp64: its own error is a few ulp times the condition number
        nptest.assert_allclose(r["edges"], exp, rtol=0, atol=r["cond"] * 64 * p * 2.0 ** -53)
        if sh == 1.0:
            assert (r["edges"] == 0.0).all()
        nptest.assert_allclose(PR.partial_corr_subject(x, sh, fisher_z=True)["edges"], np.arctanh(r["edges"]), rtol=1e-14, atol=0)


@pytest.mark.parametrize("pn", SHAPES + [(40, 300)], ids=lambda v: "p%d-n%d" % v)
def test_oracle_shrinkage_against_sklearn(pn):
    cov = pytest.importorskip("sklearn.covariance")
    (p, n) = pn
    x = PR.make_series(20 + p, 1, p, n)[0]
    Z = PR.standardise(x)
    (a, tol) = PR.ledoit_wolf(Z)
    (_c, exp) = cov.ledoit_wolf(Z.astype(np.float64).T, assume_centered=True)
    assert 0.0 < a < 1.0 and abs(a - exp) <= 1e-12
    assert 0.0 < tol < 1e-9


def test_chain_example():
    x = PR.chain()
    full = np.corrcoef(x[0])
    r = PR.partial_corr_subject(x[0], 0.0)
    rho13 = r["edges"][O.edge_endpoints(3).tolist().index([2, 0])]
    assert abs(full[0, 2]) > 0.7 and abs(rho13) < 0.05
    assert abs(r["edges"][0]) > 0.5 and abs(r["edges"][2]) > 0.5        # the direct links stay


def test_edge_order_of_the_chain():
    # c = n(n-1)/2 + m: (1,0), (2,0), (2,1)
    assert O.edge_endpoints(3).tolist() == [[1, 0], [2, 0], [2, 1]]


def test_dead_region_rule():
    (p, n) = (9, 60)
    x = PR.make_series(31, 1, p, n)[0]
    bad = x.copy()
    bad[0] = 3.5
    bad[4] = 0.0
    bad[8, 7] = np.nan
    r = PR.partial_corr_subject(bad, "ledoit_wolf")
    keep = np.array([1, 2, 3, 5, 6, 7])
    assert r["n_live"] == 6 and r["status"] == PR.OK and r["live"].tolist() == [i in keep for i in range(p)]
    by_hand = PR.partial_corr_subject(x[keep], "ledoit_wolf")
    assert r["alpha"] == by_hand["alpha"]
    ends = O.edge_endpoints(p)
    inside = np.isin(ends[:, 0], keep) & np.isin(ends[:, 1], keep)
    assert np.isnan(r["edges"][~inside]).all()
    assert np.array_equal(r["edges"][inside], by_hand["edges"])
    # one survivor has no finite edge: it is dead as well
    one = np.zeros((4, 30))
    one[2] = np.arange(30.0)
    r1 = PR.partial_corr_subject(one, 0.1)
    assert r1["n_live"] == 0 and r1["status"] == PR.TOO_FEW and np.isnan(r1["edges"]).all() and np.isnan(r1["alpha"])


def test_singular_rule():
    (p, n) = (12, 6)
    x = PR.make_series(32, 1, p, n)[0]
    r = PR.partial_corr_subject(x, 0.0)
    assert r["status"] == PR.SINGULAR and np.isnan(r["edges"]).all() and r["alpha"] == 0.0
    r = PR.partial_corr_subject(x, "ledoit_wolf")
    assert r["status"] == PR.OK and np.isfinite(r["edges"]).all() and r["alpha"] > 0.0
    dup = PR.make_series(33, 1, 5, 80)[0]
    dup[3] = 2.0 * dup[1] + 1.0
    assert PR.partial_corr_subject(dup, 0.0)["status"] == PR.SINGULAR
    assert PR.partial_corr_subject(dup, 0.05)["status"] == PR.OK


@pytest.mark.parametrize("p", [2, 3, 15, 16, 17, 33, 64, 65, 130])
def test_blocked_gauss_jordan_restated(p):
    """The inversion kernel's steps, in fp64 NumPy, inside the bound the device is held to."""
    n = 4 * p + 3
    x = PR.make_series(40 + p, 1, p, n)[0]
    r = PR.partial_corr_subject(x, 0.1)
    (Th, sing) = PR.blocked_gauss_jordan_fp64(r["R_alpha"].astype(np.float64))
    assert not sing
    d = 1.0 / np.sqrt(np.diag(Th))
    rho = np.clip(-Th * d[:, None] * d[None, :], -1.0, 1.0)
    ends = O.edge_endpoints(p)
    err = np.abs(rho[ends[:, 0], ends[:, 1]] - r["edges"]).max()
    assert err <= PR.rho_bound(r["cond"], p) and PR.rho_bound(r["cond"], p) < 1e-9
    (_Th, sing) = PR.blocked_gauss_jordan_fp64(np.ones((p, p)))
    assert sing


def test_batch_form_and_alpha_per_subject():
    ts = PR.make_series(50, 3, 6, 40)
    a = PR.partial_corr_ld(ts)
    b = PR.partial_corr_ld(ts, shrinkage=a["alpha"])
    assert np.array_equal(a["out"], b["out"]) and a["out"].shape == (15, 3) and (a["status"] == 0).all()
    c = PR.partial_corr_ld(np.concatenate([ts, np.full((3, 6, 5), 1e300)], axis=2), n_frames=[40, 40, 40])
    assert np.array_equal(a["out"], c["out"])


# ---------------------------------------------------------------------------------------------------------------------
# fcdiff_amd.corr without a device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["oas", "", -0.1, 1.5, float("nan"), None, True, [0.1]])
def test_bad_shrinkage_raises_before_any_context(bad):
    with pytest.raises(ValueError):
        corr.partial_correlations(np.zeros((1, 3, 10)), shrinkage=bad)


def test_bad_shapes_and_kind_raise_before_any_context():
    with pytest.raises(ValueError):
        corr.partial_correlations(np.zeros((3, 10)))
    with pytest.raises(ValueError):
        corr.partial_correlations(np.zeros((1, 3, 10)), frame_mask=np.ones((2, 10)))
    with pytest.raises(ValueError):
        corr.correlations(np.zeros((1, 3, 10)), kind="covariance")
    with pytest.raises(ValueError):
        corr.correlations(np.zeros((3, 10)), kind="partial")


def test_sampling_variance_n_conditioned():
    info = np.array([[100, 3, 96], [50, 0, 49], [12, 2, 9], [5, 0, 4]])
    for fz in (False, True):
        base = corr.sampling_variance(info, fisher_z=fz)
        assert np.array_equal(base, corr.sampling_variance(info, fisher_z=fz, n_conditioned=0))
        den = info[:, 2] - (2.0 if fz else 0.0)
        assert np.array_equal(base, np.where(den > 0, 1.0 / np.where(den > 0, den, 1.0), np.inf))
    p = 10
    v = corr.sampling_variance(info, fisher_z=True, n_conditioned=p - 2)
    assert v.tolist() == [1.0 / (96 - 8 - 2), 1.0 / (49 - 8 - 2), np.inf, np.inf]
    v = corr.sampling_variance(info, fisher_z=False, n_conditioned=np.array([8, 0, 8, 3]))
    assert v.tolist() == [1.0 / 88, 1.0 / 49, 1.0, 1.0]
    for bad in (-1, [1, 2], [[1]]):
        with pytest.raises(ValueError):
            corr.sampling_variance(info, n_conditioned=bad)
