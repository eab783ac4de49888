"""
The variational path's reductions at the sizes where their grids wrap (run with -m gpu on an MI355X).

test_gpu_parity.py checks the variational kernels at fixture sizes and at cfg2, where every grid-stride loop of
fcd_vb.hip / fcd_theta.hip runs one trip, the energy's (region, patient) loop runs in a handful of blocks and the theta
folds see a few partials.  Here the shapes are chosen so that the code that only runs at real sizes runs: each loop past
its first trip, the block cap of 8 x CU count, the folds over more than 256 partials.  `geometry()` restates the launch
formulas of the .hip files and every shape asserts the regime it was picked for, so that a change of the geometry fails
here instead of silently retiring the coverage.

Expected values come from the C oracle (oracle/c_oracle.py) and the NumPy oracle (oracle/fcdiff_oracle.py), both
pinned to the reference fixtures.  Sums over many terms are held to a tolerance set by their conditioning:
|got - exp| <= 1e-11 * sum |summands|, the sum of magnitudes taken on the host in long double.
"""
import math

import numpy as np
import numpy.testing as nptest
import pytest

from conftest import theta_dict

pytestmark = pytest.mark.gpu

TAB = dict(rtol=1e-12, atol=1e-14)
QF = dict(rtol=1e-9, atol=1e-10)
COND = 1e-11                    # |got - exp| <= COND * sum |summands|


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from oracle import c_oracle as CO
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.CO, e.O = torch, fcdiff_amd, _lib, CO, O
    e.ctx = _lib.Context()
    e.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return e


def new_fit(env, model=None):
    f = env.pkg.fit.UnsharedRegionFit()
    f._ctx = env.ctx
    f.model = env.pkg.UnsharedRegionModel() if model is None else model
    return f


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


# ------------------------------------------------------------------------------------------------
# launch geometry of fcd_vb.hip / fcd_theta.hip
# ------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def geometry(Nreg, U, H, n_cu):
    """
    Trip counts of the reduction loops for (Nreg, U, H) on a device with n_cu CUs, from the launches of fcd_vb.hip
    (fcd_vb_energy, fcd_vb_theta_step, fcd_vb_update_qF) and fcd_theta.hip (fcd_theta_sub_objective_ex,
    fcd_theta_full_objective_ex; H = 0: no b).
    """
    C = Nreg * (Nreg - 1) // 2
    NU = Nreg * U
    cap = 8 * n_cu
    g = dict(C=C, NU=NU, cap=cap)
    # vb_energy_edges: min(ceil(C/4), cap) blocks of 4 waves; a wave per edge, 256 threads per (region, patient) item
    nb = min(_cdiv(C, 4), cap)
    g.update(energy_blocks=nb, edge_passes=_cdiv(C, 4 * nb), nu_passes=_cdiv(NU, 256 * nb),
             nu_blocks=min(nb, _cdiv(NU, 256)))
    # vb_qF_kernel / edge_weighted_sums: lanes over patients
    g["lane_passes"] = _cdiv(U, 64)
    # vb_theta_part_kernel: TH_PARTS = 64 blocks of 256 threads
    g.update(part_c_passes=_cdiv(C, 64 * 256), part_nu_passes=_cdiv(NU, 64 * 256))
    # theta_sub_kernel: min(ceil(C U / 256), cap) blocks
    sb = min(_cdiv(C * U, 256), cap)
    g.update(sub_blocks=sb, sub_passes=_cdiv(C * U, 256 * sb))
    # theta_full_kernel: min(ceil(C max(U, H) / 256), cap) blocks; bt loop over C U, b loop over C H
    fb = min(_cdiv(C * max(U, H), 256), cap)
    g.update(full_blocks=fb, full_bt_passes=_cdiv(C * U, 256 * fb), full_b_passes=_cdiv(C * H, 256 * fb))
    return g


# the regimes a shape is chosen for: name -> test on geometry()
REGIMES = {
    "one edge": lambda g: g["C"] == 1 and g["energy_blocks"] == 1,
    "C ragged": lambda g: g["C"] % 4 != 0,
    "lanes wrap": lambda g: g["lane_passes"] >= 2,
    "lanes exact": lambda g: g["lane_passes"] == 1 and g["NU"] % 64 == 0,
    "NU loop wraps over blocks": lambda g: g["nu_passes"] >= 2 and g["nu_blocks"] > 1,
    "part NU loop wraps": lambda g: g["part_nu_passes"] >= 4,
    "edge loop wraps": lambda g: g["edge_passes"] >= 2 and g["energy_blocks"] == g["cap"],
    "edge loop 3 passes": lambda g: g["edge_passes"] == 3,
    "part C loop wraps": lambda g: g["part_c_passes"] >= 2,
    "fold > 256 partials": lambda g: g["energy_blocks"] > 256,
}

# (Nreg, U, regimes): tiny and ragged, tall and thin, wide
SHAPES = [
    (2, 1, ("one edge",)),
    (3, 65, ("C ragged", "lanes wrap")),
    (5, 64, ("lanes exact",)),
    (7, 63, ("C ragged",)),
    (11, 129, ("C ragged", "lanes wrap")),
    (40, 2000, ("NU loop wraps over blocks", "part NU loop wraps", "lanes wrap")),
    (200, 50, ("edge loop wraps", "edge loop 3 passes", "part C loop wraps", "fold > 256 partials")),
    (131, 67, ("edge loop wraps", "C ragged", "lanes wrap", "fold > 256 partials")),
]
SHAPE_IDS = ["%dx%d" % (s[0], s[1]) for s in SHAPES]


def check_regimes(env, Nreg, U, H, regimes):
    g = geometry(Nreg, U, H, env.n_cu)
    for r in regimes:
        assert REGIMES[r](g), "shape (Nreg=%d, U=%d, H=%d) is no longer in regime %r: %s" % (Nreg, U, H, r, g)
    return g


def test_geometry_of_the_named_shapes():
    """The table the shapes were chosen from, at 256 CUs (MI355X): independent of the device."""
    g = geometry(200, 50, 50, 256)                      # cfg3
    assert (g["energy_blocks"], g["edge_passes"], g["nu_passes"], g["nu_blocks"]) == (2048, 3, 1, 40)
    assert (g["part_c_passes"], g["sub_blocks"], g["sub_passes"], g["full_bt_passes"], g["full_b_passes"]) == (2, 2048, 2, 2, 2)
    g = geometry(40, 2000, 0, 256)
    assert (g["energy_blocks"], g["nu_passes"], g["nu_blocks"], g["part_nu_passes"]) == (195, 2, 195, 5)
    g = geometry(200, 3, 500, 256)
    assert (g["full_blocks"], g["full_bt_passes"], g["full_b_passes"]) == (2048, 1, 19)
    g = geometry(64, 16, 16, 256)                       # cfg2: one trip of everything
    assert (g["energy_blocks"], g["edge_passes"], g["nu_passes"], g["nu_blocks"]) == (504, 1, 1, 4)


# ------------------------------------------------------------------------------------------------
# inputs and host references
# ------------------------------------------------------------------------------------------------
def random_state(Nreg, U, seed):
    """
    lM (C,U,3,3), S_B (C,3), lq_F (C,1,3), lq_R (Nreg,U,2), gamma (3,), pi2 (2,): random, with exact zeros among the
    probabilities (lq = -inf) -- one-hot q_R sites and q_F rows, and q_F rows with a single zero.
    """
    rng = np.random.default_rng(seed)
    C = Nreg * (Nreg - 1) // 2
    lM = rng.normal(size=(C, U, 3, 3)) * 2.0 - 1.0
    S_B = rng.normal(size=(C, 3)) * 10.0
    q_R = rng.dirichlet([1.0, 1.0], size=(Nreg, U))
    hot = rng.random((Nreg, U)) < 0.1
    hot[0, 0] = True
    q_R[hot] = np.eye(2)[rng.integers(0, 2, size=int(hot.sum()))]
    q_F = rng.dirichlet([1.0, 1.0, 1.0], size=(C, 1))
    row = rng.random(C)
    row[0] = 0.15                                       # (a zero on every shape, the single edge of Nreg = 2 included)
    one = row < 0.1
    q_F[one, 0] = np.eye(3)[rng.integers(0, 3, size=int(one.sum()))]
    zero = (row >= 0.1) & (row < 0.2)
    k0 = rng.integers(0, 3, size=int(zero.sum()))
    q_F[zero, 0, k0] = 0.0
    q_F[zero, 0] /= q_F[zero, 0].sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        lq_F, lq_R = np.log(q_F), np.log(q_R)
    return dict(lM=lM, S_B=S_B, lq_F=lq_F, lq_R=lq_R, gamma=np.array([0.2, 0.5, 0.3]), pi2=np.array([0.7, 0.3]))


def load_state(env, st):
    """A fit whose device state is `st` (S_B through the (C,1,3) lp_B_g_F its H-sum is made from)."""
    fit = new_fit(env)
    fit.model.gamma, fit.model.pi = st["gamma"], st["pi2"]
    fit._lq_F, fit._lq_R, fit._lM = st["lq_F"], st["lq_R"], st["lM"]
    fit._lp_B_g_F = st["S_B"][:, None, :]
    return fit


def _lsum(x):
    return float(np.sum(np.abs(np.asarray(x, dtype=np.longdouble))))


def _pair_w(q_R, c0, c1):
    """w_l(c, u) for edges c0 <= c < c1: (q0n q0m, q1n q1m, q0n q1m + q1n q0m), fit.py:382-406."""
    from oracle import fcdiff_oracle as O
    ep = O.edge_endpoints(q_R.shape[0])[c0:c1]
    (qn, qm) = (q_R[ep[:, 0]], q_R[ep[:, 1]])
    return np.stack([qn[:, :, 0] * qm[:, :, 0], qn[:, :, 1] * qm[:, :, 1], qn[:, :, 0] * qm[:, :, 1] + qn[:, :, 1] * qm[:, :, 0]],
                    axis=2)


def energy_scales(lq_F, lq_R, S_B, lM, gamma, pi2, chunk=4096):
    """sum |summands| of each of the six energy terms (fit.py:447-539), in the order of _energy_terms()."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q_F, q_R = np.exp(lq_F)[:, 0, :], np.exp(lq_R)
        xF = np.where(q_F == 0, 0.0, q_F * lq_F[:, 0, :])
        xR = np.where(q_R == 0, 0.0, q_R * lq_R)
    C = q_F.shape[0]
    eM = np.longdouble(0)
    for c0 in range(0, C, chunk):
        c1 = min(C, c0 + chunk)
        w = _pair_w(q_R, c0, c1)
        eM += _lsum(q_F[c0:c1] * np.einsum("cul,cukl->ck", w, np.abs(lM[c0:c1])))
    return np.array([_lsum(q_F * np.log(gamma)), _lsum(q_F * S_B), _lsum(q_R * np.log(pi2)), float(eM), _lsum(xF), _lsum(xR)])


def assert_conditioned(got, exp, scale, what):
    got, exp, scale = np.asarray(got), np.asarray(exp), np.asarray(scale)
    err = np.abs(got - exp)
    bad = ~(err <= COND * scale)
    assert not bad.any(), "%s: |got - exp| %s > %g * sum|summands| %s (got %s, exp %s)" % (
        what, err[bad], COND, scale[bad], got[bad], exp[bad])


def fsum_mean(a):
    a = np.asarray(a).ravel()
    return math.fsum(a.tolist()) / a.size


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------------------------------------
# q_F update, energy, theta step, VB weights: every shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nreg,U,regimes", SHAPES, ids=SHAPE_IDS)
def test_update_lq_F_against_c_oracle(env, Nreg, U, regimes):
    """vb_qF_kernel (one wave per edge, lanes over patients) against the C oracle's update_lq_F."""
    check_regimes(env, Nreg, U, 0, regimes)
    st = random_state(Nreg, U, seed=Nreg * 7919 + U)
    fit = load_state(env, st)
    fit._update_lq_F()
    exp = env.CO.update_lq_F(st["lq_R"], st["S_B"], st["lM"], st["gamma"])
    got = fit._lq_F
    assert np.isfinite(exp).all()
    nptest.assert_allclose(got, exp, **QF)


@pytest.mark.parametrize("Nreg,U,regimes", SHAPES, ids=SHAPE_IDS)
def test_energy_terms_against_c_oracle(env, Nreg, U, regimes):
    """
    vb_energy_edges + vb_energy_fold: the six terms one by one against the C oracle's energy_terms, each to its
    conditioning; bitwise the same on a second call, and again after a q_R update in between, which grows or overwrites
    the shared workspace the partials live in (a partial slot left stale would show).
    """
    check_regimes(env, Nreg, U, 0, regimes)
    st = random_state(Nreg, U, seed=Nreg * 104729 + U)
    assert np.isneginf(st["lq_R"]).any() and np.isneginf(st["lq_F"]).any()        # xlogy0 is exercised
    fit = load_state(env, st)
    got = fit._energy_terms()
    exp = env.CO.energy_terms(st["lq_F"], st["lq_R"], st["S_B"], st["lM"], st["gamma"], st["pi2"])
    scale = energy_scales(st["lq_F"], st["lq_R"], st["S_B"], st["lM"], st["gamma"], st["pi2"])
    assert np.isfinite(exp).all() and (scale > 0).all()
    assert_conditioned(got, exp, scale, "energy terms [E_lp_F, E_lp_B, E_lp_R, E_lM, E_lq_F, E_lq_R]")
    assert bits(fit._energy_terms()) == bits(got)
    lq_R = fit._d["lq_R"]
    fit.edge_index = "symmetric"                        # (reference edge ids need three regions)
    fit._update_lq_R()
    fit._d["lq_R"] = lq_R
    assert bits(fit._energy_terms()) == bits(got)


def hyper_theta_step(env, fit):
    """fcd_vb_theta_step with a hyper block: (out4, hyper8); slots 5-7 of hyper start as a sentinel."""
    t = env.torch
    (N, U) = (int(fit._d["lq_R"].shape[0]), int(fit._d["lq_R"].shape[1]))
    out = t.empty(4, dtype=t.float64, device="cuda")
    hyper = t.full((8,), 12345.0, dtype=t.float64, device="cuda")
    env.ctx.call("fcd_vb_theta_step", env.lib.dptr(fit._d["lq_F"]), env.lib.dptr(fit._d["lq_R"]), N, U, env.lib.dptr(out),
                 env.lib.dptr(hyper), env.lib.stream_ptr())
    return out.cpu().numpy(), hyper.cpu().numpy()


def check_theta_step(env, fit, lq_F, lq_R):
    with np.errstate(divide="ignore"):
        pi = fsum_mean(np.exp(lq_R[:, :, 1]))
        gamma = np.array([fsum_mean(np.exp(lq_F[:, 0, k])) for k in range(3)])
    fit._update_theta()
    nptest.assert_allclose(fit.model.pi, pi, rtol=1e-13, atol=0)
    nptest.assert_allclose(fit.model.gamma, gamma, rtol=1e-13, atol=0)
    (out4, hyper) = hyper_theta_step(env, fit)
    assert bits(out4) == bits(np.concatenate([[fit.model.pi], fit.model.gamma]))
    with np.errstate(divide="ignore"):
        want = np.concatenate([np.log(out4[1:4]), [np.log(1 - out4[0]), np.log(out4[0])]])
    got = hyper[:5]
    assert not np.isnan(got).any()
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    nptest.assert_allclose(got[fin], want[fin], rtol=4e-15, atol=0)
    assert (hyper[5:] == 12345.0).all()                 # the step writes ln gamma, ln(1 - pi), ln pi and nothing else
    return out4, hyper


@pytest.mark.parametrize("Nreg,U,regimes", SHAPES, ids=SHAPE_IDS)
def test_theta_step_against_fsum(env, Nreg, U, regimes):
    """
    vb_theta_part_kernel + vb_theta_kernel (one launch pair): pi and gamma against math.fsum means of exp(lq), and the
    hyper block the step writes against np.log of its own pi and gamma (the device log and libm's agree to an ulp or
    two: rtol 4e-15, some 18 ulp).
    """
    check_regimes(env, Nreg, U, 0, regimes)
    st = random_state(Nreg, U, seed=Nreg * 31 + U)
    fit = load_state(env, st)
    check_theta_step(env, fit, st["lq_F"], st["lq_R"])


@pytest.mark.parametrize("which", ["pi0", "pi1"])
@pytest.mark.parametrize("Nreg,U", [(5, 64), (200, 50), (40, 2000)])
def test_theta_step_one_hot_everywhere(env, Nreg, U, which):
    """
    q_R one-hot at every site (pi = 0 exactly, or pi = 1) and q_F one-hot in one class (two gammas exactly 0): the
    hyper block holds -inf exactly where np.log gives -inf, and no NaN.
    """
    C = Nreg * (Nreg - 1) // 2
    q_R = np.zeros((Nreg, U, 2))
    q_R[:, :, 0 if which == "pi0" else 1] = 1.0
    q_F = np.zeros((C, 1, 3))
    q_F[:, 0, 1] = 1.0
    with np.errstate(divide="ignore"):
        (lq_F, lq_R) = (np.log(q_F), np.log(q_R))
    fit = new_fit(env)
    fit._lq_F, fit._lq_R = lq_F, lq_R
    (out4, hyper) = check_theta_step(env, fit, lq_F, lq_R)
    assert out4[0] == (0.0 if which == "pi0" else 1.0) and list(out4[1:]) == [0.0, 1.0, 0.0]
    assert np.isneginf(hyper[[0, 2]]).all() and hyper[1] == 0.0
    assert (hyper[3], hyper[4]) == ((0.0, -np.inf) if which == "pi0" else (-np.inf, 0.0))


@pytest.mark.parametrize("Nreg,U,regimes", SHAPES, ids=SHAPE_IDS)
def test_vb_weights_against_oracle(env, Nreg, U, regimes):
    """weights_vb_kernel (one thread per (c, u); C U not a multiple of 256) against the oracle's vb_weights."""
    check_regimes(env, Nreg, U, 0, regimes)
    assert (Nreg * (Nreg - 1) // 2 * U) % 256 != 0          # the last block is partly idle
    st = random_state(Nreg, U, seed=Nreg * 17 + U)
    fit = load_state(env, st)
    W = fit._theta_sub_weights().cpu().numpy()
    with np.errstate(divide="ignore"):
        exp = env.O.vb_weights(np.exp(st["lq_F"]), np.exp(st["lq_R"]))
    assert (exp == 0).any()
    nptest.assert_allclose(W, exp, rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------
# theta objectives at the multi-pass shapes
# ------------------------------------------------------------------------------------------------
def _theta_terms(b, bt, W, mu, sigma, eta, epsilon):
    """
    sum |summands| of the nine outputs of fcd_theta_full_objective (S, dS/d eta, dS/d epsilon, dS/d mu, dS/d sigma^2):
    the per-item terms theta_full_kernel adds (a NaN b or bt -- missing -- and a zero weight add nothing).
    """
    from oracle import fcdiff_oracle as O
    scale = np.zeros(9, dtype=np.longdouble)
    ok = ~np.isnan(bt)
    x = np.where(ok, bt, 0.0)
    s2 = sigma * sigma
    N = np.stack([O.norm_pdf(x, mu[k], sigma[k]) for k in range(3)], axis=2)
    d = x[:, :, None] - mu
    dNm = N * (d / s2)
    dNs = N * ((d * d - s2) / (2.0 * s2 * s2))
    deps_de = (-1.0, 1.0, 2 * eta - 1)
    deps_dh = 2 * epsilon - 1
    for k in range(3):
        others = N.sum(axis=2) - N[:, :, k]
        slope = N[:, :, k] - 0.5 * others
        for l in range(3):
            w = W[:, :, k, l]
            nz = (w != 0) & ok
            e = O.eval_M_eps(eta, epsilon, l)
            M = np.where(nz, e * N[:, :, k] + (1 - e) * 0.5 * others, 1.0)
            wz = np.where(nz, w, 0.0)
            r = wz / M
            scale[0] += _lsum(wz * np.log(M))
            scale[2] += _lsum(deps_de[l] * r * slope)
            if l == 2:
                scale[1] += _lsum(deps_dh * r * slope)
            for j in range(3):
                cf = e if j == k else 0.5 * (1 - e)
                scale[3 + j] += _lsum(r * cf * dNm[:, :, j])
                scale[6 + j] += _lsum(r * cf * dNs[:, :, j])
    if b is not None:
        wF = W[:, 0, :, :].sum(axis=2)
        for k in range(3):
            db = b - mu[k]
            z = db / sigma[k]
            lp = -(z * z) / 2.0 - 0.91893853320467274178 - np.log(sigma[k])
            wk = np.where(np.isnan(b), 0.0, wF[:, k:k + 1])
            scale[0] += _lsum(np.where(wk != 0, wk * lp, 0.0))
            scale[3 + k] += _lsum(np.where(wk != 0, wk * db / s2[k], 0.0))
            scale[6 + k] += _lsum(np.where(wk != 0, wk * (db * db - s2[k]) / (2.0 * s2[k] * s2[k]), 0.0))
    return scale.astype(np.float64)


def _b_term_missing(b, W, mu, sigma):
    """The healthy-subject term of the full objective with NaN b integrated out (a NaN adds nothing): (S, dm, ds)."""
    from oracle import fcdiff_oracle as O
    wF = np.sum(W[:, 0, :, :], axis=2)
    S, dm, ds = 0.0, np.zeros(3), np.zeros(3)
    for k in range(3):
        S += np.sum(wF[:, k] * np.nansum(O.norm_logpdf(b, mu[k], sigma[k]), axis=1))
        dm[k] += np.sum(wF[:, k] * np.nansum(O.eval_dlN_dm(b, mu[k], sigma[k]), axis=1))
        ds[k] += np.sum(wF[:, k] * np.nansum(O.eval_dlN_ds(b, mu[k], sigma[k]), axis=1)) / (sigma[k] * sigma[k])
    return S, dm, ds


def expected_full(env, b, bt, W, m, missing):
    """O.theta_full_objective; missing data: a NaN bt item enters with zero weight, a NaN b through _b_term_missing."""
    args = (m.mu, m.sigma, m.eta, m.epsilon)
    if not missing:
        (S, dh, de, dm, ds) = env.O.theta_full_objective(b, bt, W, *args)
        return np.concatenate([[S, dh, de], dm, ds])
    nan_bt = np.isnan(bt)
    Wm = np.where(nan_bt[:, :, None, None], 0.0, W)
    (S, dh, de, dm, ds) = env.O.theta_full_objective(None, np.where(nan_bt, 0.0, bt), Wm, *args)
    if b is not None:
        (Sb, dmb, dsb) = _b_term_missing(b, W, m.mu, m.sigma)
        (S, dm, ds) = (S + Sb, dm + dmb, ds + dsb)
    return np.concatenate([[S, dh, de], dm, ds])


@pytest.mark.parametrize("Nreg,H,U,regimes", [
    (200, 50, 50, ("sub 2 passes", "full bt 2 passes", "full b 2 passes")),      # cfg3: C U > 2048 x 256
    (200, 500, 3, ("b loop sets the grid",)),                                      # H > U
], ids=["cfg3", "H500xU3"])
def test_theta_objectives_multi_pass(env, Nreg, H, U, regimes):
    """
    theta_sub_kernel / theta_full_kernel and their folds over 2048 partials, against the oracle's
    theta_full_objective: with and without the b term, with VB weights and with chain counts (zeros among them),
    with and without missing data (NaN in b and bt).  The first three numbers without b equal
    fcd_theta_sub_objective's to 1e-12.
    """
    from fcdiff_amd.fit import theta_full_objective, theta_sub_objective
    g = geometry(Nreg, U, H, env.n_cu)
    g0 = geometry(Nreg, U, 0, env.n_cu)
    for r in regimes:
        ok = {"sub 2 passes": g["sub_passes"] >= 2 and g["sub_blocks"] == g["cap"],
              "full bt 2 passes": g["full_bt_passes"] >= 2 and g0["full_bt_passes"] >= 2,
              "full b 2 passes": g["full_b_passes"] >= 2,
              "b loop sets the grid": H > U and g["full_blocks"] == g["cap"] and g["full_b_passes"] >= 2
                                      and g["full_b_passes"] > g["full_bt_passes"]}[r]
        assert ok, "shape (%d, %d, %d) is no longer in regime %r: %s" % (Nreg, H, U, r, g)
    m = env.pkg.UnsharedRegionModel()
    m.eta, m.epsilon = 0.29, 0.07
    m.mu, m.sigma = np.array([-0.2, 0.01, 0.33]), np.array([0.06, 0.08, 0.11])
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(Nreg, H, U, seed=Nreg + H + U)
    C = Nreg * (Nreg - 1) // 2
    rs = np.random.RandomState(11)
    q_F = rs.uniform(1e-7, 1, (C, 1, 3))
    q_F /= q_F.sum(axis=2, keepdims=True)
    q_R = rs.uniform(1e-7, 1, (Nreg, U, 2))
    q_R /= q_R.sum(axis=2, keepdims=True)
    W_vb = env.O.vb_weights(q_F, q_R)
    f = rs.randint(0, 3, (6, C)).astype(np.uint8)
    r = (rs.rand(6, Nreg, U) < 0.3).astype(np.uint8)
    W_ct = env.O.pair_counts(f, r)
    assert (W_ct == 0).any()
    b_nan, bt_nan = b.copy(), bt.copy()
    b_nan[rs.rand(*b.shape) < 0.03] = np.nan
    bt_nan[rs.rand(*bt.shape) < 0.03] = np.nan
    th = m.theta()
    for (wname, W) in (("vb", W_vb), ("counts", W_ct)):
        W_d = up(env, W)
        for missing in (False, True):
            (bb, bbt) = (b_nan, bt_nan) if missing else (b, bt)
            (b_d, bt_d) = (up(env, bb), up(env, bbt))
            for with_b in (True, False):
                got = theta_full_objective(env.ctx, b_d if with_b else None, bt_d, W_d, th, missing_data=missing)
                exp = expected_full(env, bb if with_b else None, bbt, W, m, missing)
                scale = _theta_terms(bb if with_b else None, bbt, W, m.mu, m.sigma, m.eta, m.epsilon)
                assert np.isfinite(exp).all() and (scale > 0).all()
                assert_conditioned(got, exp, scale, "theta_full W=%s missing=%s b=%s" % (wname, missing, with_b))
                if not with_b:
                    sub = theta_sub_objective(env.ctx, bt_d, W_d, th, missing_data=missing)
                    nptest.assert_allclose(got[:3], sub, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------
# one full variational iteration at cfg3, the cfg5 kernels, tables with -inf entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reference", "symmetric"])
def test_vb_iteration_cfg3_against_oracles(env, mode):
    """
    BASELINE cfg3 (Nreg 200, H = U = 50): tables, q_F, q_R, theta, tables again, energy -- each step against the C
    oracle (q_R and the energy from the oracle's own chain of steps, hence q_F's tolerance for both); the final energy
    against the NumPy oracle's vb_iteration (vectorised) to 1e-9 relative: bench.py's `energies_agree`, asserted.
    """
    (N, H, U) = (200, 50, 50)
    check_regimes(env, N, U, H, ("edge loop wraps", "part C loop wraps", "fold > 256 partials"))
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    th0 = theta_dict(m.theta())
    fit = new_fit(env, m)
    fit.edge_index = mode
    fit.b, fit.bt = b, bt
    fit._init_lps(N, H, U)
    fit._update_lps()
    S_B, lM = env.CO.lik_tables(b, bt, m.theta())
    nptest.assert_allclose(fit._lM, lM, **TAB)
    nptest.assert_allclose(fit._d["S_B"].cpu().numpy(), S_B, rtol=1e-12)
    (lq_R0, lq_F0) = (fit._lq_R, fit._lq_F)
    fit._update_lq_F()
    lq_F = env.CO.update_lq_F(lq_R0, S_B, lM, m.gamma)
    nptest.assert_allclose(fit._lq_F, lq_F, **QF)
    fit._update_lq_R()
    lq_R = env.CO.update_lq_R(lq_R0, lq_F, lM, m.pi2(), 0 if mode == "reference" else 1)
    nptest.assert_allclose(fit._lq_R, lq_R, **QF)
    (lq_F_d, lq_R_d) = (fit._lq_F, fit._lq_R)
    fit._update_theta()
    nptest.assert_allclose(fit.model.pi, fsum_mean(np.exp(lq_R_d[:, :, 1])), rtol=1e-13)
    nptest.assert_allclose(fit.model.gamma, [fsum_mean(np.exp(lq_F_d[:, 0, k])) for k in range(3)], rtol=1e-13)
    nptest.assert_allclose(fit.model.pi, env.O.update_pi(lq_R), rtol=1e-9)
    nptest.assert_allclose(fit.model.gamma, env.O.update_gamma(lq_F), rtol=1e-9)
    fit._update_lps()
    S_B2, lM2 = env.CO.lik_tables(b, bt, m.theta())
    nptest.assert_allclose(fit._lM, lM2, **TAB)
    nptest.assert_allclose(fit._d["S_B"].cpu().numpy(), S_B2, rtol=1e-12)
    terms = fit._energy_terms()
    exp = env.CO.energy_terms(lq_F, lq_R, S_B2, lM2, env.O.update_gamma(lq_F), [1 - env.O.update_pi(lq_R), env.O.update_pi(lq_R)])
    nptest.assert_allclose(terms, exp, rtol=1e-9)
    (_F, _R, th1, e_np) = env.O.vb_iteration(lq_F0, lq_R0, b, bt, th0,
                                             mode=env.O.EDGE_REFERENCE if mode == "reference" else env.O.EDGE_SYMMETRIC,
                                             vectorised=True)
    e = fit._eval_energy()
    nptest.assert_allclose(e, e_np, rtol=1e-9)
    nptest.assert_allclose(fit.model.pi, th1["pi"], rtol=1e-9)


def test_cfg5_kernels_against_c_oracle_on_device_tables(env):
    """
    BASELINE cfg5 (Nreg 400, H = U = 500): q_F, energy and the theta step against the C oracle applied to the device's
    own tables copied back (one 2.9 GB lM on the host, not two).  q_R is random with exact zeros.
    """
    (N, H, U) = (400, 500, 500)
    g = check_regimes(env, N, U, H, ("edge loop wraps", "lanes wrap", "part C loop wraps", "fold > 256 partials"))
    assert g["edge_passes"] >= 9 and g["part_nu_passes"] >= 10
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=5)
    fit = new_fit(env, m)
    fit.b, fit.bt = b, bt
    fit._init_lps(N, H, U)
    fit._update_lps()
    del b, bt, _r, _t, _f, _ft
    rng = np.random.default_rng(55)
    q_R = rng.dirichlet([1.0, 1.0], size=(N, U))
    hot = rng.random((N, U)) < 0.05
    q_R[hot] = np.eye(2)[rng.integers(0, 2, size=int(hot.sum()))]
    with np.errstate(divide="ignore"):
        lq_R = np.log(q_R)
    fit._lq_R = lq_R
    S_B, lM = fit._d["S_B"].cpu().numpy(), fit._lM
    fit._update_lq_F()
    lq_F = fit._lq_F
    nptest.assert_allclose(lq_F, env.CO.update_lq_F(lq_R, S_B, lM, m.gamma), **QF)
    pi2 = m.pi2()
    got = fit._energy_terms()
    exp = env.CO.energy_terms(lq_F, lq_R, S_B, lM, m.gamma, pi2)
    scale = energy_scales(lq_F, lq_R, S_B, lM, m.gamma, pi2)
    assert_conditioned(got, exp, scale, "cfg5 energy terms")
    del lM
    check_theta_step(env, fit, lq_F, lq_R)


def test_minus_inf_tables_through_q_F_and_energy(env):
    """
    Tables with -inf entries (densities that underflow, built as test_lik_tables_underflow_gives_minus_inf_like_reference
    builds them) through the q_F update and the energy, U > 64: the NaN and -inf pattern of the outputs equals the
    oracles' (NumPy and C) exactly, and the finite entries meet the usual tolerances.  A zero gamma makes lq_F = -inf;
    zero q_R beside -inf lM make the 0 * (-inf) = NaN of the reference.
    """
    (N, H, U) = (12, 3, 70)
    C = N * (N - 1) // 2
    m = env.pkg.UnsharedRegionModel()
    m.sigma = np.array([1e-3, 1e-3, 1e-3])
    rng = np.random.default_rng(12)
    b = rng.normal(size=(C, H)) * 1e-3
    bt = m.mu[rng.integers(0, 3, size=(C, U))] + rng.normal(size=(C, U)) * 1e-3
    far = rng.random((C, U)) < 0.005             # about a third of the edges meet one
    bt[far] = 1.0                                       # every density underflows: lM = -inf for all (k, l)
    fit = new_fit(env, m)
    fit.b, fit.bt = b, bt
    fit._init_lps(N, H, U)
    fit._update_lps()
    with np.errstate(divide="ignore"):
        (lpB, _pBt, lM) = env.O.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon)
    got_lM = fit._lM
    assert np.array_equal(np.isneginf(got_lM), np.isneginf(lM)) and np.isneginf(lM).any()
    S_B = env.O.sum_lp_B(lpB)
    q_R = rng.dirichlet([1.0, 1.0], size=(N, U))
    hot = rng.random((N, U)) < 0.1
    q_R[hot] = np.eye(2)[rng.integers(0, 2, size=int(hot.sum()))]
    for gamma in (np.array([0.1, 0.8, 0.1]), np.array([0.5, 0.5, 0.0])):
        with np.errstate(divide="ignore", invalid="ignore"):
            lq_R = np.log(q_R)
            exp_F = env.O.update_lq_F(lq_R, S_B, lM, gamma)
            exp_Fc = env.CO.update_lq_F(lq_R, S_B, lM, gamma)
        fit.model.gamma = gamma
        fit._lq_R = lq_R
        fit._update_lq_F()
        got_F = fit._lq_F
        for (name, e) in (("numpy", exp_F), ("C", exp_Fc)):
            for test in (np.isnan, np.isneginf, np.isposinf):
                assert np.array_equal(test(got_F), test(e)), (name, test.__name__)
        assert np.isnan(exp_F).any() and np.isfinite(exp_F).any()
        fin = np.isfinite(exp_F)
        nptest.assert_allclose(got_F[fin], exp_F[fin], **QF)
        nptest.assert_allclose(got_F[fin], exp_Fc[fin], **QF)
        # energy on a q_F without NaN (the update's NaN rows replaced by a finite distribution; -inf kept)
        lq_F = np.where(np.isnan(got_F), np.log(1 / 3), got_F)
        fit._lq_F = lq_F
        got = fit._energy_terms()
        with np.errstate(divide="ignore", invalid="ignore"):
            exp = env.O.energy_terms(lq_F, lq_R, S_B, lM, gamma, m.pi2())
            exp_c = env.CO.energy_terms(lq_F, lq_R, S_B, lM, gamma, m.pi2())
            scale = energy_scales(lq_F, lq_R, S_B, np.where(np.isinf(lM), 0.0, lM), gamma, m.pi2())
        for (name, e) in (("numpy", exp), ("C", exp_c)):
            for test in (np.isnan, np.isneginf, np.isposinf):
                assert np.array_equal(test(got), test(e)), (name, test.__name__, got, e)
        assert not np.isfinite(exp).all()
        fin = np.isfinite(exp)
        assert_conditioned(got[fin], exp[fin], scale[fin], "energy terms with -inf tables")
        assert_conditioned(got[fin], exp_c[fin], scale[fin], "energy terms with -inf tables (C)")
