"""
The permutation baselines with nuisance covariates without a GPU: the two forms of the reference (baseline_glm_ref.py)
against each other, against baseline_ref's two-sample t where no column is kept, and against three regions worked by hand;
glm_design() and draw_permutations(); the host-side refusals (they run before any context exists); and that header, binding
and library agree on the two entry points.
"""
import math
import os
import re

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_glm_ref as GR
import baseline_ref as BR
from fcdiff_amd import _lib, baseline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", GR.SHAPES[:7])
def test_projection_form_against_direct_freedman_lane(shape):
    """rtol 1e-9 on t^2 over all connections and permutations.  A relative bound needs a t away from 0 (its error is
    absolute, about S 2^-53 in t units): |t| >= 1e-5 is asserted first, and the seeds of the shapes were chosen for it."""
    (b, bt, z_b, z_bt, perms) = GR.make_data(*shape)
    (t, tp) = GR.all_t(b, bt, z_b, z_bt, perms)
    (t2, tp2) = GR.all_t(b, bt, z_b, z_bt, perms, "lstsq")
    a = np.concatenate([t[None, :], tp]) ** 2
    d = np.concatenate([t2[None, :], tp2]) ** 2
    assert np.isfinite(a).all() and a.min() >= 1e-10
    nptest.assert_allclose(a, d, rtol=1e-9, atol=0)
    assert np.array_equal(np.sign(t), np.sign(t2)) and np.array_equal(np.sign(tp), np.sign(tp2))


def test_lstsq_form_with_a_full_set_of_site_dummies():
    """Three site dummies sum to the constant: the raw design is rank deficient, one column is dropped, the t's agree."""
    (N, H, U, Q, P, seed) = (6, 9, 8, 2, 12, 11)
    (b, bt, z_b, z_bt, perms) = GR.make_data(N, H, U, Q, P, seed)
    site = np.arange(H + U) % 3
    dummies = (site[:, None] == np.arange(3)[None, :]).astype(np.float64)
    (z_b, z_bt) = (np.concatenate([z_b, dummies[:H]], axis=1), np.concatenate([z_bt, dummies[H:]], axis=1))
    (W, used, dof) = GR.design(z_b, z_bt)
    assert used[:2].all() and used[2:].sum() == 2 and dof == H + U - 4 - 2 and W.shape == (H + U, 5)
    assert used.tolist() == baseline.glm_design(z_b, z_bt)[1]["used"].tolist()
    (t, tp) = GR.all_t(b, bt, z_b, z_bt, perms)
    (t2, tp2) = GR.all_t(b, bt, z_b, z_bt, perms, "lstsq")
    assert min(np.abs(t).min(), np.abs(tp).min()) >= 1e-5
    nptest.assert_allclose(np.concatenate([t[None, :], tp]) ** 2, np.concatenate([t2[None, :], tp2]) ** 2, rtol=1e-9)


@pytest.mark.parametrize("shape", BR.SHAPES[:3])
def test_no_column_kept_is_the_two_sample_t(shape):
    (N, H, U, P, seed) = shape
    (b, bt, _labels) = BR.make_data(*shape)
    perms = baseline.draw_permutations(P, H + U, seed)
    none = np.zeros((H + U, 0))
    ref = GR.group_test(b, bt, none[:H], none[H:], perms)
    two = BR.group_test(b, bt, (perms >= H).astype(np.uint8))
    for k in ("t", "region", "null_max_t", "null_max_region", "null_t"):
        nptest.assert_allclose(ref[k], two[k], rtol=1e-10, err_msg=k)
    # constant covariate columns are the same thing
    const = np.full((H + U, 2), 4.0)
    (W, used, dof) = GR.design(const[:H], const[H:])
    assert not used.any() and dof == H + U - 2 and W.shape == (H + U, 1)
    kf = math.sqrt(U * H / (H + U))
    nptest.assert_allclose(W[:, 0], np.array([-U / (H + U)] * H + [H / (H + U)] * U) / kf, rtol=1e-14)


def hand_case():
    """Three regions, H = 3, U = 2, one covariate z = (-2, -1, 0, 1, 2).  w_1 = z / sqrt(10); x_c = (-.4, -.4, -.4, .6, .6),
    w_1 . x_c = 3 / sqrt(10), x_r = x_c - .3 z = (.2, -.1, -.4, .3, 0), ||x_r||^2 = .3; dof = 2.
    Connection 0 = (1, 2, 0, 4, 3): centred (-1, 0, -2, 2, 1), w_1 . y = 6 / sqrt(10), e = y_c - .6 z = (.2, .6, -2, 1.4, -.2),
    Q_e = 6.4; x_r . e = 1.2, d_0^2 = 1.44 / .3 = 4.8, d_1 = 0; t^2 = 4.8 * 2 / 1.6 = 6.
    Permutation (1, 0, 2, 3, 4): x_r[pi] . e = 1.32, d_0^2 = 5.808; z[pi] . e = -.4, d_1^2 = .016; t^2 = 11.616 / .576 = 121/6.
    Connection 1 is constant; connection 2 = 10 - connection 0: the same with the other sign."""
    y = np.array([1.0, 2.0, 0.0, 4.0, 3.0])
    X = np.stack([y, np.full(5, 5.0), 10.0 - y])
    z = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])[:, None]
    perms = np.array([[1, 0, 2, 3, 4]], dtype=np.int64)
    return X[:, :3].copy(), X[:, 3:].copy(), z[:3].copy(), z[3:].copy(), perms


def test_three_regions_by_hand():
    (b, bt, z_b, z_bt, perms) = hand_case()
    for (W, dof) in (GR.design(z_b, z_bt)[::2], (baseline.glm_design(z_b, z_bt)[0], baseline.glm_design(z_b, z_bt)[1]["dof"])):
        assert dof == 2
        nptest.assert_allclose(W[:, 0], np.array([.2, -.1, -.4, .3, 0.0]) / math.sqrt(.3), rtol=0, atol=1e-15)
        nptest.assert_allclose(np.abs(W[:, 1]), np.abs(np.array([-2.0, -1, 0, 1, 2])) / math.sqrt(10.0), rtol=0, atol=1e-15)
    for form in ("projection", "lstsq"):
        (t, tp) = GR.all_t(b, bt, z_b, z_bt, perms, form)
        nptest.assert_allclose(t[[0, 2]], [math.sqrt(6.0), -math.sqrt(6.0)], rtol=1e-12)
        nptest.assert_allclose(tp[0, [0, 2]], [11.0 / math.sqrt(6.0), -11.0 / math.sqrt(6.0)], rtol=1e-12)
        assert math.isnan(t[1]) and math.isnan(tp[0, 1])
    ref = GR.group_test(b, bt, z_b, z_bt, perms)
    nptest.assert_allclose(ref["region"], [6.0, 12.0, 6.0], rtol=1e-12)             # E(0) = {0, 1}, E(1) = {0, 2}, E(2) = {1, 2}
    nptest.assert_allclose(ref["null_region"][0], [121.0 / 6, 121.0 / 3, 121.0 / 6], rtol=1e-12)
    nptest.assert_allclose(ref["null_max_t"], [11.0 / math.sqrt(6.0)], rtol=1e-12)
    assert ref["count_t"].tolist() == [1, 0, 1] and ref["count_region"].tolist() == [1, 1, 1]
    assert ref["p_t"][0] == 1.0 and math.isnan(ref["p_t"][1]) and math.isnan(ref["p_fwe_t"][1])
    net = GR.network_test(b, bt, z_b, z_bt, perms, 2.0, "greater")
    assert net["edge_mask"].tolist() == [True, False, False] and net["null_max_extent"].tolist() == [1]


def test_reference_treats_a_row_in_the_covariates_span_as_dead():
    (b, bt, z_b, z_bt, perms) = GR.make_data(*GR.SHAPES[2])
    (b, bt) = (b.copy(), bt.copy())
    (b[4], bt[4]) = (z_b[:, 0] + 0.3, z_bt[:, 0] + 0.3)
    (b[7], bt[7]) = (z_b[:, 0] + 0.3, z_bt[:, 0] + 0.3)
    bt[7, 0] += 1e-9                                              # nine digits away from the span: alive
    for form in ("projection", "lstsq"):
        (t, tp) = GR.all_t(b, bt, z_b, z_bt, perms, form)
        assert np.flatnonzero(np.isnan(t)).tolist() == [4] and np.isnan(tp[:, 4]).all() and not np.isnan(np.delete(tp, 4, axis=1)).any()
    S = b.shape[1] + bt.shape[1]
    assert GR.dead_tol2(S, 5) == (8 * S * 5 * 2.0 ** -52) ** 2 and math.sqrt(GR.dead_tol2(1024, 9)) < 2e-11


# ---- glm_design, draw_permutations ---------------------------------------------------------------------------------------------

def test_glm_design_rules():
    rng = np.random.default_rng(3)
    (H, U) = (9, 7)
    S = H + U
    age = rng.normal(50.0, 10.0, S)
    site = np.arange(S) % 3
    dummies = (site[:, None] == np.arange(3)[None, :]).astype(np.float64)
    Z = np.column_stack([age, np.full(S, 2.0), 3.0 * age + 1.0, dummies])        # a constant, a duplicate (rescaled), a full set of dummies
    (W, info) = baseline.glm_design(Z[:H], Z[H:])
    # `used` is in the order of the columns of z: the constant, the duplicate behind its original and one dummy are dropped
    assert info["used"].dtype == bool and info["used"][:3].tolist() == [True, False, False] and info["used"][3:].sum() == 2
    assert info["rank"] == 3 and info["dof"] == S - 3 - 2 and W.shape == (S, 4) and W.dtype == np.float64 and W.flags.c_contiguous
    nptest.assert_allclose(W.T.dot(W), np.eye(4), rtol=0, atol=1e-14)             # orthonormal ...
    nptest.assert_allclose(W.sum(axis=0), 0.0, atol=1e-14)                         # ... and centred
    # columns 1 .. span the centred kept covariates; column 0 is the group residualised on them
    kept = Z[:, info["used"]] - Z[:, info["used"]].mean(axis=0)
    nptest.assert_allclose(W[:, 1:].dot(W[:, 1:].T.dot(kept)), kept, atol=1e-12)
    x = np.array([0.0] * H + [1.0] * U)
    full = np.column_stack([np.ones(S), kept])
    xr = x - full.dot(np.linalg.lstsq(full, x, rcond=None)[0])
    nptest.assert_allclose(W[:, 0], xr / np.linalg.norm(xr), atol=1e-13)
    (Wr, used, dof) = GR.design(Z[:H], Z[H:])
    assert used.tolist() == info["used"].tolist() and dof == info["dof"]
    nptest.assert_allclose(W[:, 0], Wr[:, 0], atol=1e-13)
    # no column at all, and columns that are all constant: the two-sample design
    for z in (np.zeros((S, 0)), np.full((S, 3), 1.5)):
        (W0, info0) = baseline.glm_design(z[:H], z[H:])
        assert W0.shape == (S, 1) and info0["rank"] == 0 and info0["dof"] == S - 2 and info0["used"].shape == (z.shape[1],)
        nptest.assert_allclose(W0[:, 0], (x - U / S) / math.sqrt(U * H / S), rtol=1e-14)
    # torch tensors are taken
    import torch
    (Wt, _i) = baseline.glm_design(torch.as_tensor(Z[:H]), torch.as_tensor(Z[H:]))
    assert np.array_equal(Wt, W)


def test_draw_permutations():
    perms = baseline.draw_permutations(5, 9, seed=4)
    rng = np.random.default_rng(4)
    want = np.stack([rng.permutation(9) for _ in range(5)])
    assert perms.dtype == np.int64 and perms.shape == (5, 9) and np.array_equal(perms, want)
    assert (np.sort(perms, axis=1) == np.arange(9)[None, :]).all()
    assert np.array_equal(baseline.draw_permutations(5, 9, seed=4), perms) and not np.array_equal(baseline.draw_permutations(5, 9, seed=5), perms)


# ---- refusals, before any context exists ---------------------------------------------------------------------------------------

def calls():
    return ((baseline.group_test, ()), (baseline.network_test, (2.0,)))


def test_refusals_before_a_context_exists():
    (b, bt, z_b, z_bt, perms) = GR.make_data(*GR.SHAPES[1])
    (H, U) = (b.shape[1], bt.shape[1])
    S = H + U
    rng = np.random.default_rng(0)
    for (fn, args) in calls():
        def call(bb=b, tt=bt, **kw):
            kw.setdefault("z_b", z_b)
            kw.setdefault("z_bt", z_bt)
            kw.setdefault("permutations", perms)
            return fn(bb, tt, *args, **kw)
        with pytest.raises(ValueError, match="together"):
            call(z_bt=None)
        with pytest.raises(ValueError, match="together"):
            call(z_b=None)
        with pytest.raises(ValueError, match="labels"):
            call(labels=(perms >= H).astype(np.uint8))
        with pytest.raises(ValueError, match="covariates"):
            fn(b, bt, *args, permutations=perms)
        with pytest.raises(NotImplementedError, match="own design"):
            call(missing_data=True)
        with pytest.raises(NotImplementedError, match="own design"):
            call(variance="welch")
        for (zb, zt) in ((z_b[:-1], z_bt), (z_b, z_bt[:, :1]), (z_b[:, 0], z_bt[:, 0]), (z_bt, z_b)):
            with pytest.raises(ValueError, match="shape"):
                call(z_b=zb, z_bt=zt)
        for bad in (math.nan, math.inf, -math.inf):
            z = z_bt.copy()
            z[1, 0] = bad
            with pytest.raises(ValueError, match="NaN or infinite"):
                call(z_bt=z)
        nan_b = b.copy()
        nan_b[0, 0] = math.nan
        with pytest.raises(ValueError, match="NaN or infinite"):
            call(bb=nan_b)
        # more than 8 columns kept; 8 of 9 kept is fine up to the device
        big = rng.normal(size=(40, 9))
        (b40, bt40) = (np.tile(b[:, :1], (1, 25)), np.tile(bt[:, :1], (1, 15)))
        with pytest.raises(NotImplementedError, match="at most 8"):
            fn(b40, bt40, *args, z_b=big[:25], z_bt=big[25:])
        # S < Q' + 3: 10 subjects carry 7 columns at most
        with pytest.raises(ValueError, match="need"):
            fn(b[:, :5], bt[:, :5], *args, z_b=rng.normal(size=(5, 8)), z_bt=rng.normal(size=(5, 8)))
        # the group is a function of the covariates
        g = np.array([0.0] * H + [1.0] * U)[:, None]
        with pytest.raises(ValueError, match="linear function"):
            call(z_b=g[:H], z_bt=g[H:])
        two = np.column_stack([z_b[:, 0].tolist() + z_bt[:, 0].tolist(), 2.0 * g[:, 0] - np.array(z_b[:, 0].tolist() + z_bt[:, 0].tolist())])
        with pytest.raises(ValueError, match="linear function"):
            call(z_b=two[:H], z_bt=two[H:])
        # permutations
        for bad in (perms[:, :-1], perms[0], perms.astype(np.float64), np.zeros((0, S), dtype=np.int64)):
            with pytest.raises(ValueError, match="permutations"):
                call(permutations=bad)
        twice = perms.copy()
        twice[3, 0] = twice[3, 1]
        with pytest.raises(ValueError, match="permutation of"):
            call(permutations=twice)
        with pytest.raises(ValueError, match="n_perm"):
            fn(b, bt, *args, z_b=z_b, z_bt=z_bt, n_perm=0)
        # as today
        wide = np.zeros((b.shape[0], 1020))
        with pytest.raises(NotImplementedError, match="at most 1024"):
            fn(wide, bt, *args, z_b=np.zeros((1020, 1)), z_bt=z_bt[:, :1])
        with pytest.raises(NotImplementedError, match="sessions"):
            call(tt=np.zeros((b.shape[0], U, 2)))


def test_a_valid_call_reaches_the_device():
    """Past the host checks the call reaches for the device (and fails here without one)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    (b, bt, z_b, z_bt, perms) = GR.make_data(*GR.SHAPES[1])
    for (fn, args) in calls():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b, bt, *args, z_b=z_b, z_bt=z_bt, permutations=perms)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(b, bt, *args, z_b=np.ones_like(z_b), z_bt=np.ones_like(z_bt), n_perm=5)


# ---- header, binding, library --------------------------------------------------------------------------------------------------

def test_header_binding_and_library_agree():
    names = ("fcd_baseline_group_glm", "fcd_baseline_network_bits_glm")
    text = open(os.path.join(ROOT, "include", "fcdiff_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, "%s is not declared in the header" % name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
        assert "const double *design" in m.group(1) and "const uint16_t *perms" in m.group(1)
        assert hasattr(lib, name)
    # design, R and perms take the place of labels
    assert len(_lib.SIGNATURES[names[0]][1]) == len(_lib.SIGNATURES["fcd_baseline_group_perm"][1]) + 2
    assert len(_lib.SIGNATURES[names[1]][1]) == len(_lib.SIGNATURES["fcd_baseline_network_bits"][1]) + 2
    assert lib.fcd_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert baseline.GLM_MAX_COLUMNS == 8


def test_docstrings_state_the_rules():
    for fn in (baseline.group_test, baseline.network_test):
        assert "z_b" in fn.__doc__ and "permutations" in fn.__doc__ and "design_info" in fn.__doc__
    doc = baseline.group_test.__doc__
    for word in ("Freedman", "exchangeability", "F-tests", "more than 8 columns", "own design"):
        assert word in doc, word
