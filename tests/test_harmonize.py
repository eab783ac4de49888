"""
Site harmonisation without a GPU: the reference (harmonize_ref.py) against closed forms and numpy.linalg.lstsq, the fixed point
against its two equations, the host-side argument checks of fcdiff_amd.covariates (they run before any context exists, so they
raise here, where there is no device), the package's host-side design against the reference's, and the scenario that
motivates the feature on the reference alone.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import harmonize_ref as HR
import noise_ref as NR
import fcdiff_amd
from conftest import theta_dict
from fcdiff_amd import covariates
from oracle import fcdiff_oracle as O

LD = np.longdouble


@pytest.mark.parametrize("B,H", [(1, 9), (2, 4), (3, 17), (16, 65)])
def test_reference_without_shrinkage_against_closed_forms(B, H):
    """eb=False, no covariates: the harmonised controls of every site have mean abar_c and ddof-1 variance sigma2_c."""
    rng = np.random.default_rng(100 * B + H)
    idx = HR.make_sites(rng, H, B)
    b = HR.make_rows(rng, 12, idx)
    ref = HR.fit_ld(b, idx, B, eb=False)
    assert len(HR.assert_conditions(ref)) == 12 and np.all(ref["info"] == [H, B, 0, 0])
    out = HR.apply_ld(b, idx, None, ref)
    for i in range(B):
        cols = idx == i
        nptest.assert_allclose(out[:, cols].mean(axis=1), ref["grand_mean"], rtol=0, atol=1e-12)
        nptest.assert_allclose(out[:, cols].var(axis=1, ddof=1), ref["pooled_sd"] ** 2, rtol=1e-12, atol=0)
    # the common level is the mean of all controls, sigma2 the pooled within-site variance divided by n
    nptest.assert_allclose(ref["grand_mean"], b.mean(axis=1), rtol=0, atol=1e-14)
    within = sum(((b[:, idx == i] - b[:, idx == i].mean(axis=1, keepdims=True)) ** 2).sum(axis=1) for i in range(B))
    nptest.assert_allclose(ref["pooled_sd"] ** 2, within / H, rtol=1e-12)
    nptest.assert_allclose(HR.apply_loop(b, idx, np.zeros((H, 0)), ref["grand_mean"], ref["beta"], ref["shift"], ref["scale"], ref["z_ref"]),
                           out, rtol=0, atol=1e-14)


@pytest.mark.parametrize("B,H,Q", [(2, 12, 1), (3, 40, 3), (16, 130, 8)])
def test_reference_slopes_against_lstsq(B, H, Q):
    rng = np.random.default_rng(10 * H + Q)
    idx = HR.make_sites(rng, H, B)
    z = HR.make_design(rng, H, Q, idx)
    b = HR.make_rows(rng, 9, idx, z)
    ref = HR.fit_ld(b, idx, B, z)
    HR.assert_conditions(ref)
    assert ref["mask"] == (1 << Q) - 1 and np.all(ref["info"] == [H, B, Q, 0])
    X = np.concatenate([(idx[:, None] == np.arange(B)[None, :]).astype(np.float64), z], axis=1)
    (coef, _res, rank, _sv) = np.linalg.lstsq(X, b.T, rcond=None)
    assert rank == B + Q
    nptest.assert_allclose(ref["beta"], coef[B:].T, rtol=1e-9, atol=1e-12)
    resid = b.T - X.dot(coef)
    nptest.assert_allclose(ref["pooled_sd"] ** 2, (resid * resid).sum(axis=0) / H, rtol=1e-9)
    # alpha_i is the fitted value of site i at z_ref: abar their weighted mean
    at_ref = coef[:B] + ref["z_ref"].dot(coef[B:])[None, :]
    nptest.assert_allclose(ref["grand_mean"], (np.bincount(idx, minlength=B)[:, None] * at_ref).sum(axis=0) / H, rtol=1e-9, atol=1e-12)
    # the covariate effects are kept: the slopes of the harmonised controls are beta again wherever shift and scale are mild
    ref0 = HR.fit_ld(b, idx, B, z, eb=False)
    out = HR.apply_ld(b, idx, z, ref0)
    for i in range(B):
        nptest.assert_allclose(out[:, idx == i].mean(axis=1) - (z[idx == i].mean(axis=0) - ref0["z_ref"]).dot(ref0["beta"].T),
                               ref0["grand_mean"], rtol=0, atol=1e-12)


def test_reference_design_rules():
    """A column constant within every site is dropped, a copy of a column loses to the lower index, and neither gets a slope."""
    rng = np.random.default_rng(3)
    (B, H) = (3, 30)
    idx = HR.make_sites(rng, H, B)
    z = HR.make_design(rng, H, 2, idx)
    z = np.concatenate([z, rng.standard_normal(B)[idx][:, None], z[:, :1] * 2.0 + 1.0], axis=1)      # 2: site level; 3: column 0 again
    b = HR.make_rows(rng, 5, idx, z[:, :2])
    ref = HR.fit_ld(b, idx, B, z)
    assert sorted(ref["used"]) == [0, 1] and ref["mask"] == 0b0011 and np.all(ref["info"][:, 2] == 2)
    assert np.all(ref["beta"][:, 2:] == 0.0) and ref["norm"][2] == 0.0
    (W, T, z_bar, info) = covariates.site_design(z, idx, B)
    assert info["mask"] == 0b0011 and info["used"] == ref["used"] and W.shape == (H, 2) and T.shape == (4, 2) and np.all(T[2:] == 0.0)
    nptest.assert_allclose(W.T.dot(W), np.eye(2), rtol=0, atol=1e-14)
    for i in range(B):
        nptest.assert_allclose(W[idx == i].sum(axis=0), 0.0, atol=1e-14)
    nptest.assert_allclose(z_bar, np.stack([z[idx == i].mean(axis=0) for i in range(B)]), rtol=0, atol=1e-15)
    # the package's basis spans the reference's columns: the same slopes
    yc = b - np.stack([b[:, idx == i].mean(axis=1) for i in range(B)])[idx].T
    nptest.assert_allclose(yc.dot(W).dot(T.T), ref["beta"], rtol=1e-10, atol=1e-13)


def test_fixed_point_and_sufficient_statistics():
    """(gamma_star, delta2_star) satisfies both equations of the map, and the bracket of the second,
    (n_i - 1) delta2_hat + n_i (gamma_hat - gamma)^2, is the direct sum over the site's standardised controls."""
    rng = np.random.default_rng(8)
    (B, H, C) = (3, 21, 40)
    idx = HR.make_sites(rng, H, B)
    b = HR.make_rows(rng, C, idx, nan=0.1)
    b[0, idx == 1] = np.nan
    b[0, np.flatnonzero(idx == 1)[0]] = 0.2            # a lone control
    b[1, idx == 2] = np.nan                            # a site missing entirely
    ref = HR.fit_ld(b, idx, B, missing=True)
    rows = HR.assert_conditions(ref)
    assert ref["n_obs"][1, 0] == 1 and ref["n_obs"][2, 1] == 0 and ref["fitted"][:2].all()
    p = ref["prior"]
    for i in range(B):
        for c in rows:
            (n, gh, dh, g, d2) = (int(ref["n_obs"][i, c]), ref["gamma_hat"][i, c], ref["delta2_hat"][i, c], ref["gamma_star"][i, c],
                                  ref["delta2_star"][i, c])
            if n == 0:
                assert g == p["gamma_bar"][i] and np.isnan(gh) and ref["n_iter"][i, c] == 0
                nptest.assert_allclose(d2, p["b"][i] / (p["a"][i] - 1.0), rtol=1e-15)
                continue
            ss = (n - 1) * dh if n >= 2 else 0.0
            assert np.isnan(dh) == (n < 2)
            nptest.assert_allclose(g, (n * p["tau2"][i] * gh + d2 * p["gamma_bar"][i]) / (n * p["tau2"][i] + d2), rtol=1e-12, atol=1e-13)
            nptest.assert_allclose(d2, (0.5 * (ss + n * (gh - g) ** 2) + p["b"][i]) / (n / 2.0 + p["a"][i] - 1.0), rtol=1e-12)
            # the standardised controls of the site: Z_h = (y_h - abar) / sigma
            cols = (idx == i) & ~np.isnan(b[c])
            Z = (b[c, cols].astype(LD) - LD(ref["grand_mean"][c])) / LD(ref["pooled_sd"][c])
            direct = ((Z - LD(g)) ** 2).sum()
            nptest.assert_allclose(float(direct), ss + n * (gh - g) ** 2, rtol=1e-10)
    assert ref["n_iter"][:, rows].max() < 200


def test_reference_rules_for_connections_that_are_not_fitted():
    rng = np.random.default_rng(4)
    (B, H) = (2, 8)
    idx = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.uint8)
    b = HR.make_rows(rng, 30, idx)
    b[0] = 0.25                                        # constant
    b[1] = np.where(idx == 0, 0.1, -0.2)               # constant within each site
    b[2, [1, 2, 3, 5, 6, 7]] = np.nan                  # n - B_c = 0
    b[3, 2] = np.nan                                   # one NaN
    ref = HR.fit_ld(b, idx, B, missing=True)
    assert ref["info"][:4].tolist() == [[8, 2, 0, HR.ST_CONSTANT], [8, 2, 0, HR.ST_CONSTANT], [2, 2, 0, HR.ST_DOF], [7, 2, 0, 0]]
    plain = HR.fit_ld(b[[3, 4]], idx, B)
    assert plain["info"].tolist() == [[8, 2, 0, HR.ST_NAN], [8, 2, 0, 0]] and np.isnan(plain["grand_mean"][0])
    for k in ("grand_mean", "pooled_sd"):
        assert np.isnan(ref[k][:3]).all() and np.isfinite(ref[k][3:]).all()
    assert np.all(ref["shift"][:, :3] == 0.0) and np.all(ref["scale"][:, :3] == 1.0)
    x = rng.standard_normal((30, 5))
    out = HR.apply_ld(x, np.array([0, 1, 1, 0, 1]), None, ref)
    assert out[:3].tobytes() == x[:3].tobytes() and not np.array_equal(out[3:], x[3:])
    # identical rows: no spread of gamma_hat over the connections, the prior is undefined
    same = HR.fit_ld(np.tile(b[5], (4, 1)), idx, B)
    assert not same["prior_defined"].any() and same["fitted"].all() and np.all(same["shift"] == 0.0)


def test_host_checks_run_before_any_context():
    rng = np.random.default_rng(0)
    (C, H) = (6, 8)
    b = rng.standard_normal((C, H))
    site = ["a", "b"] * 4
    z = rng.standard_normal((H, 2))
    fit = covariates.fit_harmonization
    with pytest.raises(ValueError, match=r"\(C, H\)"):
        fit(b[0], site)
    with pytest.raises(ValueError, match="one site per control"):
        fit(b, site[:7])
    with pytest.raises(ValueError, match="at least two"):
        fit(b, ["a"] * 7 + ["b"])
    with pytest.raises(ValueError, match="controls must agree"):
        fit(b, site, z[:7])
    with pytest.raises(ValueError, match=r"\(H, Q\)"):
        fit(b, site, z[:, 0])
    bad = z.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        fit(b, site, bad)
    with pytest.raises(ValueError, match="one value per column"):
        fit(b, site, z, z_ref=[0.0])
    with pytest.raises(NotImplementedError, match="at most 8"):
        fit(b, site, rng.standard_normal((H, 9)))
    with pytest.raises(NotImplementedError, match="own design"):
        fit(b, site, z, missing_data=True)
    with pytest.raises(NotImplementedError, match="at most 64"):
        fit(rng.standard_normal((2, 130)), list(range(65)) * 2)
    with pytest.raises(NotImplementedError, match="at most 4096"):
        fit(np.zeros((1, 4097)), [0, 1] * 2048 + [0])
    # harmonize(): the patients' arguments too
    with pytest.raises(ValueError, match="did not see"):
        covariates.harmonize(b, rng.standard_normal((C, 3)), site, ["a", "c", "b"])
    with pytest.raises(ValueError, match="one site per subject"):
        covariates.harmonize(b, rng.standard_normal((C, 3)), site, ["a", "b"])
    with pytest.raises(ValueError, match="z is needed"):
        covariates.harmonize(b, rng.standard_normal((C, 3)), site, ["a", "b", "b"], z)
    with pytest.raises(ValueError, match="z must have shape"):
        covariates.harmonize(b, rng.standard_normal((C, 3)), site, ["a", "b", "b"], z, rng.standard_normal((3, 1)))
    with pytest.raises(TypeError, match="unknown"):
        covariates.harmonize(b, rng.standard_normal((C, 3)), site, ["a", "b", "b"], reference_site="a")
    # apply() of an object made from saved arrays
    h = covariates.SiteHarmonization(["a", "b"], np.zeros(C), np.zeros((C, 2)), np.zeros((2, C)), np.ones((2, C)), z.mean(axis=0))
    assert h.n_columns == 2 and h.sites == ["a", "b"] and h.info is None
    for (x, s, zz) in [(np.zeros((C, 3)), ["a", "b", "x"], np.zeros((3, 2))), (np.zeros((C, 3)), ["a", "b"], np.zeros((3, 2))),
                       (np.zeros((C, 3)), ["a", "b", "b"], None), (np.zeros((C, 3)), ["a", "b", "b"], np.zeros((3, 1))),
                       (np.zeros((C + 1, 3)), ["a", "b", "b"], np.zeros((3, 2))), (np.zeros(C), ["a"], np.zeros((1, 2))),
                       (np.zeros((C, 3, 2)), ["a", "b", "b"], np.zeros((2, 2)))]:
        with pytest.raises(ValueError):
            h.apply(x, s, zz)
    with pytest.raises(ValueError, match="non-finite"):
        h.apply(np.zeros((C, 3)), ["a", "b", "b"], np.full((3, 2), np.nan))
    with pytest.raises(ValueError, match="sites, connections"):
        covariates.SiteHarmonization(["a", "b"], np.zeros(C), np.zeros((C, 0)), np.zeros((3, C)), np.ones((3, C)), np.zeros(0))


def scenario_fits():
    """Rates of the scenario on the reference alone: no site effect, effect present, harmonised on the controls."""
    s = HR.SCENARIO
    m = fcdiff_amd.UnsharedRegionModel()
    m.pi = s["pi"]
    (b0, bt0, b, bt, site_b, site_bt, r) = HR.scenario_data(m)
    start = theta_dict(m.theta())
    (b_h, bt_h, ref) = HR.harmonize_ld(b, bt, site_b, site_bt)
    HR.assert_conditions(ref)
    fits = [NR.vb_fit(x, xt, start, s["iters"], O.EDGE_SYMMETRIC) for (x, xt) in ((b0, bt0), (b, bt), (b_h, bt_h))]
    return fits, r, ref


def test_scenario_site_effect_looks_anomalous_until_harmonised():
    """
    harmonize_ref.SCENARIO on the reference alone, 8 VB iterations, symmetric edge ids: 64 controls in two sites of 32, every
    patient at site 1, which adds N(0, 0.04^2) per connection and spreads the correlations 1.5 times as wide.  Healthy
    regions flagged and anomalous regions found (25): no site effect 0.0043 and 0.92; effect present, not harmonised 0.0390
    and 0.92; harmonised on the controls 0.0087 and 0.92.
    """
    (fits, r, ref) = scenario_fits()
    rates = [HR.scenario_rates(f["lq_R"], r) for f in fits]
    assert int(r.sum()) == 25 and ref["fitted"].all()
    for (name, v) in zip(("no effect", "not harmonised", "harmonised"), rates):
        print("%s: flagged %.4f found %.2f" % ((name,) + v))
    print("largest n_iter %d" % ref["n_iter"].max())
    assert rates[1][0] >= 5.0 * rates[0][0] > 0.0            # the effect looks anomalous ...
    assert rates[2][0] < rates[1][0]                         # ... and harmonising takes most of that away
    assert rates[2][0] <= 0.02
    assert rates[2][2 - 1] >= 0.80                           # the bound the covariates scenario allows itself
    # the figures quoted in README.md
    assert [(round(a, 4), round(c, 2)) for (a, c) in rates] == [(0.0043, 0.92), (0.0390, 0.92), (0.0087, 0.92)]
