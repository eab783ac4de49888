"""
Covariate adjustment without a GPU: the reference (covariates_ref.py) against numpy.linalg.lstsq, the host-side argument checks
of fcdiff_amd.covariates (they run before any context exists, so they raise here, where there is no device), leverage
against the hat matrix, and the scenario that motivates the feature on the reference alone.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import covariates_ref as CV
import noise_ref as NR
import fcdiff_amd
from conftest import theta_dict
from fcdiff_amd import covariates
from oracle import fcdiff_oracle as O


@pytest.mark.parametrize("H,Q", [(5, 1), (17, 3), (40, 16), (64, 0)])
def test_reference_against_lstsq(H, Q):
    rng = np.random.default_rng(10 * H + Q)
    z = CV.make_design(rng, H, Q)
    b = CV.make_rows(rng, 7, z)
    ref = CV.fit_ld(b, z)
    CV.assert_conditions(ref)
    X = np.concatenate([np.ones((H, 1)), z], axis=1)
    (coef, _res, rank, _sv) = np.linalg.lstsq(X, b.T, rcond=None)
    assert rank == Q + 1
    nptest.assert_allclose(ref["beta"], coef[1:].T, rtol=1e-9, atol=1e-12)
    resid = b.T - X.dot(coef)
    nptest.assert_allclose(ref["resid_var"], (resid * resid).sum(axis=0) / (H - 1 - Q), rtol=1e-9)
    assert np.array_equal(ref["info"], np.tile([H, Q, H - 1 - Q, (1 << Q) - 1], (7, 1)))
    # a subject at the reference point is unchanged, and the controls' adjusted values keep their mean
    z_ref = CV.default_z_ref(z)
    nptest.assert_array_equal(CV.apply_ld(b[:, :1], z_ref[None, :], z_ref, ref["beta"]), b[:, :1])
    nptest.assert_allclose(CV.apply_ld(b, z, z_ref, ref["beta"]).mean(axis=1), b.mean(axis=1), rtol=0, atol=1e-14)
    nptest.assert_allclose(CV.apply_loop(b, z, z_ref, ref["beta"]), CV.apply_ld(b, z, z_ref, ref["beta"]), rtol=0, atol=1e-14)


def test_reference_missing_rows_and_drop_rule():
    rng = np.random.default_rng(5)
    (H, Q) = (20, 3)
    z = CV.make_design(rng, H, Q)
    z = np.concatenate([z, z[:, :1]], axis=1)                  # column 3 = column 0: the lower index is used
    b = CV.make_rows(rng, 4, z[:, :3])
    b[1, 3:9] = np.nan
    b[2, :] = np.nan
    b[3, 4:] = np.nan                                          # n_obs = 4 = rank + 1
    ref = CV.fit_ld(b, z, missing=True)
    assert ref["info"].tolist() == [[20, 3, 16, 0b0111], [14, 3, 10, 0b0111], [0, 0, -1, 0], [4, 0, 0, 0]]
    assert np.all(ref["beta"][:2, 3] == 0) and np.all(ref["beta"][2:] == 0) and np.isnan(ref["resid_var"][2:]).all()
    keep = ~np.isnan(b[1])
    X = np.concatenate([np.ones((keep.sum(), 1)), z[keep, :3]], axis=1)
    nptest.assert_allclose(ref["beta"][1, :3], np.linalg.lstsq(X, b[1, keep], rcond=None)[0][1:], rtol=1e-9, atol=1e-12)
    # without the flag the NaN is a value: the whole row of beta
    plain = CV.fit_ld(b[:2], z)
    assert np.isnan(plain["beta"][1]).all() and plain["info"][1].tolist() == [20, 3, 16, 0b0111]


def test_host_checks_run_before_any_context():
    rng = np.random.default_rng(0)
    (b, z) = (rng.standard_normal((6, 5)), rng.standard_normal((5, 2)))
    with pytest.raises(ValueError, match="controls must agree"):
        covariates.fit_adjustment(b, z[:4])
    with pytest.raises(ValueError, match=r"\(C, H\)"):
        covariates.fit_adjustment(b[0], z)
    with pytest.raises(ValueError, match=r"\(H, Q\)"):
        covariates.fit_adjustment(b, z[:, 0])
    bad = z.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        covariates.fit_adjustment(b, bad)
    with pytest.raises(ValueError, match="non-finite"):
        covariates.fit_adjustment(b, z, z_ref=[0.0, np.inf])
    with pytest.raises(ValueError, match="one value per column"):
        covariates.fit_adjustment(b, z, z_ref=[0.0, 0.0, 0.0])
    with pytest.raises(NotImplementedError, match="at most 16"):
        covariates.fit_adjustment(b, rng.standard_normal((5, 17)))
    with pytest.raises(ValueError, match="z must have shape"):
        covariates.adjust(b, rng.standard_normal((6, 3)), z, rng.standard_normal((4, 2)))
    adj = covariates.EdgeAdjustment(np.zeros((6, 2)), np.zeros(6), np.zeros((6, 4), dtype=np.int32), z.mean(axis=0), z)
    assert adj.n_columns == 2
    for (x, zz) in [(np.zeros((6, 3)), np.zeros((3, 1))), (np.zeros((6, 3, 2)), np.zeros((2, 2))),
                    (np.zeros((6, 3, 2)), np.zeros((3, 3, 2))), (np.zeros((5, 3)), np.zeros((3, 2))), (np.zeros(6), np.zeros((6, 2)))]:
        with pytest.raises(ValueError):
            adj.apply(x, zz)
    with pytest.raises(ValueError, match="non-finite"):
        adj.apply(np.zeros((6, 3)), np.full((3, 2), np.nan))


def test_leverage_is_the_hat_matrix_diagonal():
    rng = np.random.default_rng(2)
    (H, Q) = (12, 3)
    z = rng.standard_normal((H, Q)) * [1.0, 10.0, 0.1] + [3.0, -2.0, 0.0]
    adj = covariates.EdgeAdjustment(np.zeros((1, Q)), np.zeros(1), np.zeros((1, 4), dtype=np.int32), z.mean(axis=0), z)
    X = np.concatenate([np.ones((H, 1)), z], axis=1)
    hat = X.dot(np.linalg.solve(X.T.dot(X), X.T))
    nptest.assert_allclose(adj.leverage(z), np.diagonal(hat) - 1.0 / H, rtol=1e-10, atol=1e-13)
    assert adj.leverage(z.mean(axis=0)[None, :])[0] == 0.0
    with pytest.raises(ValueError):
        adj.leverage(z[:, :2])


def scenario_fits():
    """Rates of the scenario on the reference alone: no covariate effect, effect not adjusted, adjusted on the controls."""
    s = CV.SCENARIO
    m = fcdiff_amd.UnsharedRegionModel()
    m.pi = s["pi"]
    (b0, bt0, b, bt, z_b, z_bt, r) = CV.scenario_data(m)
    start = theta_dict(m.theta())
    (b_adj, bt_adj, ref) = CV.adjust_ld(b, bt, z_b, z_bt)
    CV.assert_conditions(ref)
    rates = [CV.scenario_rates(NR.vb_fit(x, xt, start, s["iters"], O.EDGE_SYMMETRIC)["lq_R"], r)
             for (x, xt) in ((b0, bt0), (b, bt), (b_adj, bt_adj))]
    return rates, r


def test_scenario_effect_looks_anomalous_until_adjusted():
    """
    covariates_ref.SCENARIO on the reference alone, 8 VB iterations, symmetric edge ids: patients 1.5 units "older" than the
    controls, 0.06 per unit on every connection of regions 0-3.  Healthy regions flagged (all / regions 0-3) and anomalous
    regions found (25): no effect 0.0043 / 0.018 and 0.92; effect not adjusted 0.147 / 0.509 and 0.84; adjusted on the
    controls 0.0043 / 0.018 and 0.92.
    """
    (rates, r) = scenario_fits()
    assert int(r.sum()) == 25
    for (name, v) in zip(("no effect", "not adjusted", "adjusted"), rates):
        print("%s: flagged %.4f / %.3f found %.2f" % ((name,) + v))
    assert rates[1][0] >= 0.10
    assert rates[2][0] <= 0.02
    assert rates[2][2] >= 0.80
    # the figures quoted in README.md
    assert [(round(a, 4), round(b, 3), round(c, 2)) for (a, b, c) in rates] == [(0.0043, 0.018, 0.92), (0.1472, 0.509, 0.84),
                                                                                (0.0043, 0.018, 0.92)]
