"""
Site harmonisation on the device (fcd_site_harmonize_fit, fcd_site_harmonize_apply, fcdiff_amd.covariates) against
tests/harmonize_ref.py.

Tolerances.  Everything the fit makes per connection -- grand_mean, pooled_sd, gamma_hat, delta2_hat, beta in scaled units
(times the norm of the centred column) -- and the priors are fixed-order sums of at most H (priors: C) terms of magnitude
about 1, compared at FIT (rtol 1e-10, atol 1e-12) under the conditions harmonize_ref.assert_conditions checks on the oracle's
side; info, n_obs and the design's mask exactly.  gamma_star, delta2_star, shift and scale at the same tolerance: the stopping
rule leaves at most 1e-13 / (1 - ratio) of the fixed point, ratio the contraction of the last steps, <= 0.5 for all pairs
but the few "slow" ones assert_conditions names (<= 0.99: 1e-11).  apply is compared bit for bit with a NumPy loop of the
stated operation order on the device's own parameters.

Shapes are the edges of the kernels: B = 16 / 17 (a tile of 16 columns in the product form the header leaves open), 64 (every
lane owns a site), H = 2 B (two controls a site), 65 / 130 (lanes wrap), 600 and 1100 (more than the 256 controls a wave
stages at once; 1100 x 8 columns is also more than the 2048 doubles of W a workgroup stages), C = 2016 (more connections
than one pass of a small grid's waves would take is left to profiles/harmonize_cost.py's 19 900).
"""
import ctypes

import numpy as np
import numpy.testing as nptest
import pytest

import caller_stream_cases as R
import harmonize_ref as HR
import noise_ref as NR
from conftest import theta_dict
from oracle import fcdiff_oracle as O

pytestmark = pytest.mark.gpu

FIT = HR.FIT
CS = (3, 10, 2016)
REAL = ("grand_mean", "pooled_sd", "gamma_hat", "delta2_hat", "gamma_star", "delta2_star", "shift", "scale")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, covariates

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.cov = torch, fcdiff_amd, _lib, covariates
    e.ctx = _lib.Context()
    return e


def up(env, a, dtype=None):
    return None if a is None else env.torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


FIT_OUT = dict(grand_mean=("C", np.float64), pooled_sd=("C", np.float64), beta=("CQ", np.float64), gamma_hat=("BC", np.float64),
               delta2_hat=("BC", np.float64), gamma_star=("BC", np.float64), delta2_star=("BC", np.float64), shift=("BC", np.float64),
               scale=("BC", np.float64), n_obs=("BC", np.int32), n_iter=("BC", np.int32), info=("C4", np.int32),
               prior=("6B", np.float64), prior_info=("B3", np.int32))


def out_shapes(C, B, Q):
    sh = {"C": (C,), "CQ": (C, max(Q, 1)), "BC": (B, C), "C4": (C, 4), "6B": (6, B), "B3": (B, 3)}
    return dict((k, (sh[s], dt)) for (k, (s, dt)) in FIT_OUT.items())


def raw_fit(env, b, idx, B, z=None, flags=0, ctx=None, override=None):
    """fcd_site_harmonize_fit through the C ABI on host arrays, the design by the package's host code -> dict of NumPy arrays
    (outputs pre-filled with 7); override: members of the descriptor set last (a wrong size, extents past the limits)."""
    t = env.torch
    (C, H) = b.shape
    z = np.zeros((H, 0)) if z is None else z
    Q = z.shape[1]
    (W, T, z_bar, _info) = env.cov.site_design(z, np.asarray(idx), B) if Q else (np.zeros((H, 0)), np.zeros((0, 0)), np.zeros((B, 0)), None)
    Qp = W.shape[1]
    ref = np.ascontiguousarray(z.mean(axis=0)) if Q else np.zeros(0)
    held = [up(env, b, np.float64), up(env, idx, np.uint8), up(env, W, np.float64) if Qp else None]
    outs = dict((k, t.full(sh, 7, dtype=getattr(t, np.dtype(dt).name), device="cuda")) for (k, (sh, dt)) in out_shapes(C, B, Q).items())
    p = env.lib.dptr
    members = dict(flags=flags, C=C, H=H, B=B, Q=Q, Qp=Qp, stream=env.lib.stream_ptr(), b=p(held[0]), site=p(held[1]), W=p(held[2]),
                   T=T.ctypes.data if Qp else None, z_bar=z_bar.ctypes.data if Q else None, z_ref=ref.ctypes.data if Q else None)
    members.update((k, p(v)) for (k, v) in outs.items())
    members.update(override or {})
    d = env.lib.HarmonizeDesc.make(**members)
    (ctx or env.ctx).call("fcd_site_harmonize_fit", ctypes.byref(d))
    got = dict((k, v.cpu().numpy()) for (k, v) in outs.items())
    got["beta"] = got["beta"][:, :Q]
    got["_inputs"] = held
    return got


def raw_apply(env, xd, sd, zd, par, z_ref, outd, B, ctx=None, override=None):
    """fcd_site_harmonize_apply on device tensors (xd, outd (C, S) may be views); par: dict of device tensors."""
    (C, S) = (int(xd.shape[0]), int(xd.shape[1]))
    Q = int(z_ref.shape[0])
    p = env.lib.dptr
    z_ref = np.ascontiguousarray(z_ref, dtype=np.float64)
    members = dict(C=C, S=S, B=B, Q=Q, stream=env.lib.stream_ptr(), x=p(xd), site=p(sd), z=p(zd) if Q else None,
                   z_ref=z_ref.ctypes.data if Q else None, grand_mean=p(par["grand_mean"]), beta=p(par["beta"]) if Q else None,
                   shift=p(par["shift"]), scale=p(par["scale"]), out=p(outd))
    members.update(override or {})
    d = env.lib.HarmonizeDesc.make(**members)
    (ctx or env.ctx).call("fcd_site_harmonize_apply", ctypes.byref(d))


def compare(got, ref, rows, what=REAL, with_prior=True, label=""):
    """got: a SiteHarmonization or a dict of arrays over the first C connections of the reference's."""
    g = (lambda k: getattr(got, k)) if not isinstance(got, dict) else (lambda k: got[k])
    C = g("grand_mean").shape[0]
    rows = np.asarray([c for c in rows if c < C], dtype=np.int64)
    assert np.array_equal(g("info"), ref["info"][:C]), "info"
    assert np.array_equal(g("n_obs"), ref["n_obs"][:, :C]), "n_obs"
    worst = {}
    for k in what:
        (a, w) = (g(k), ref[k][..., :C])
        assert np.array_equal(np.isnan(a), np.isnan(w)), k
        sel = (a[..., rows], w[..., rows])
        with np.errstate(invalid="ignore"):
            worst[k] = float(np.nanmax(np.abs(sel[0] - sel[1]) / (1e-12 / 1e-10 + np.abs(sel[1])), initial=0.0))
        # a connection that is not among the rows compared to tolerance is not fitted: NaN or (0, 1), checked above / below
    beta = g("beta") * ref["norm"][None, :]
    worst["beta"] = float(np.nanmax(np.abs(beta[rows] - ref["beta_scaled"][rows]), initial=0.0))
    print("%s C=%d: %d rows; largest deviation relative to (1e-2 + |ref|): %s" % (label, C, rows.size, ", ".join("%s %.2g" % kv for kv in sorted(worst.items()))))
    for k in what:
        nptest.assert_allclose(g(k)[..., rows], ref[k][..., :C][..., rows], err_msg=k, **FIT)
    nptest.assert_allclose(beta[rows], ref["beta_scaled"][rows], err_msg="beta", **FIT)
    unfit = np.flatnonzero(~ref["fitted"][:C])
    assert np.all(g("shift")[:, unfit] == 0.0) and np.all(g("scale")[:, unfit] == 1.0) and np.isnan(g("grand_mean")[unfit]).all()
    if with_prior:
        p = g("prior")
        for k in ("gamma_bar", "tau2", "m", "s2", "a", "b"):
            nptest.assert_allclose(p[k], ref["prior"][k], err_msg="prior " + k, **FIT)
        assert np.array_equal(p["members"], ref["members"])


# ------------------------------------------------------------------------------------------------
# 1. the fit against the reference
# ------------------------------------------------------------------------------------------------
# (B, H, Q, share of NaN, eb).  B = 1 has gamma_hat = 0 everywhere, so no prior: eb=False there.
FIT_CASES = [(1, 17, 0, 0.0, False), (2, 4, 0, 0.0, True), (3, 17, 1, 0.0, True), (2, 64, 3, 0.0, True), (16, 65, 0, 0.06, True),
             (17, 130, 0, 0.0, True), (16, 130, 8, 0.0, True), (64, 130, 0, 0.06, True), (3, 600, 3, 0.0, True),
             (2, 1100, 8, 0.0, True), (3, 65, 0, 0.06, False), (12, 64, 8, 0.0, True), (64, 128, 0, 0.0, True)]
_cases = {}


def fit_case(key):
    """the inputs of a case and ONE run of the reference on its 2016 rows, shared by the tests"""
    if key not in _cases:
        (B, H, Q, nan, eb) = key
        rng = np.random.default_rng([B, H, Q, int(nan * 100), int(eb)])
        idx = HR.make_sites(rng, H, B)
        z = HR.make_design(rng, H, Q, idx) if Q else None
        b = HR.make_rows(rng, CS[-1], idx, z, nan)
        ref = HR.fit_ld(b, idx, B, z, missing=nan > 0, eb=eb)
        rows = HR.assert_conditions(ref)
        ref_hats = HR.fit_ld(b, idx, B, z, missing=nan > 0, eb=False) if eb else ref
        _cases[key] = (idx, z, b, ref, rows, ref_hats)
    return _cases[key]


@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: "B%d-H%d-Q%d-nan%g-eb%d" % c)
def test_fit_against_the_reference(env, case):
    """The device at C = 2016 with everything compared; at C = 3 and 10 on the first rows with eb=False (the priors depend on
    all connections, the rest does not)."""
    (B, H, Q, nan, eb) = case
    (idx, z, b, ref, rows, ref_hats) = fit_case(case)
    assert rows.size >= 0.9 * CS[-1]
    h = env.cov.fit_harmonization(b, idx.tolist(), z, missing_data=nan > 0, eb=eb, ctx=env.ctx)
    assert h.sites == list(range(B)) and h.design_info["mask"] == ref["mask"] and sorted(h.design_info["used"]) == sorted(ref["used"])
    assert h.z_ref.tobytes() == ref["z_ref"].tobytes()
    compare(h, ref, rows, with_prior=eb, label="eb=%d" % eb)
    if not eb:
        assert np.isnan(h.prior["tau2"]).all() and np.all(h.prior["members"] == 0) and np.all(h.n_iter == 0)
    capped = h.n_iter < 0
    print("largest n_iter %d (reference %d), pairs at the cap %d, slow pairs %d of %d" % (np.abs(h.n_iter).max(), ref["n_iter"].max(), capped.sum(),
                                                                                     ref["slow"].sum(), ref["slow"].size))
    assert not capped.any()
    for C in CS[:2]:
        got = raw_fit(env, b[:C], idx, B, z, (env.lib.FCD_DATA_NAN_MISSING if nan else 0) | env.lib.FCD_HARMONIZE_NO_EB)
        compare(got, ref_hats, rows, with_prior=False, label="eb=0")


# ------------------------------------------------------------------------------------------------
# 2. apply, bit for bit
# ------------------------------------------------------------------------------------------------
def random_parameters(rng, C, B, Q):
    par = dict(grand_mean=0.3 * rng.standard_normal(C), beta=0.1 * rng.standard_normal((C, Q)), shift=0.05 * rng.standard_normal((B, C)),
               scale=rng.uniform(0.5, 1.7, (B, C)))
    par["shift"][:, 3] = 0.0
    par["scale"][:, 3] = 1.0                          # a connection that was not fitted ...
    par["grand_mean"][3] = np.nan
    par["beta"][3] = np.nan
    par["shift"][B - 1, 5] = 0.0                      # ... and a pair the fit left alone
    par["scale"][B - 1, 5] = 1.0
    par["shift"][0, 6] = 0.0                          # (shift 0 alone, scale 1 alone: harmonised)
    par["scale"][0, 7] = 1.0
    return par


@pytest.mark.parametrize("S", [1, 2, 255, 256, 257])
@pytest.mark.parametrize("B,Q", [(1, 0), (3, 3), (64, 8)])
def test_apply_is_the_numpy_loop_bit_for_bit(env, S, B, Q):
    """S odd: 8 bytes per lane; S even: 16; 257: two blocks of columns.  37 rows: two blocks of rows.  Then the same through
    views that start 8 bytes off a 16-byte boundary (x, out, both)."""
    C = 37
    rng = np.random.default_rng(1000 * S + 10 * B + Q)
    x = rng.standard_normal((C, S))
    x[rng.random((C, S)) < 0.1] = np.nan
    site = rng.integers(0, B, S)
    site[0] = B - 1
    z = rng.standard_normal((S, Q)) * 3.0 + 1.0
    z_ref = rng.standard_normal(Q)
    par = random_parameters(rng, C, B, Q)
    h = env.cov.SiteHarmonization(list(range(B)), par["grand_mean"], par["beta"], par["shift"], par["scale"], z_ref, env.ctx)
    out = h.apply(x, site, z if Q else None)
    want = HR.apply_loop(x, site, z, par["grand_mean"], par["beta"], par["shift"], par["scale"], z_ref)
    assert np.array_equal(np.isnan(out), np.isnan(x))
    assert out.tobytes() == want.tobytes()
    assert out[3].tobytes() == x[3].tobytes() and out[5, 0].tobytes() == x[5, 0].tobytes()       # (subject 0 is at site B - 1)
    assert (~np.isnan(x) & (out != x))[[0, 1, 2, 4, 6, 7]].any()
    t = env.torch
    dpar = dict((k, up(env, v, np.float64)) for (k, v) in par.items())
    (sd, zd) = (up(env, site, np.uint8), up(env, z, np.float64))
    for (off_x, off_out) in ((1, 0), (0, 1), (1, 1)):
        (xb, ob) = (t.zeros(C * S + 2, dtype=t.float64, device="cuda"), t.full((C * S + 2,), 7.0, dtype=t.float64, device="cuda"))
        xv = xb[off_x:off_x + C * S].view(C, S)
        ov = ob[off_out:off_out + C * S].view(C, S)
        assert xv.data_ptr() % 16 == 8 * off_x and ov.data_ptr() % 16 == 8 * off_out
        xv.copy_(up(env, x, np.float64))
        raw_apply(env, xv, sd, zd, dpar, z_ref, ov, B)
        assert ov.cpu().numpy().tobytes() == want.tobytes(), (off_x, off_out)
        guard = ob.cpu().numpy()
        assert guard[:off_out].tolist() == [7.0] * off_out and guard[off_out + C * S:].tolist() == [7.0] * (2 - off_out)
        assert xv.cpu().numpy().tobytes() == x.tobytes()


def test_apply_takes_sessions_and_labels(env):
    (C, U, K, Q, B) = (10, 3, 2, 3, 3)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((C, U, K))
    x[2, 1, 0] = np.nan
    (z_u, z_uk) = (rng.standard_normal((U, Q)), rng.standard_normal((U, K, Q)))
    par = random_parameters(rng, C, B, Q)
    sites = ["leuven", "nyu", "ucla"]
    lab = ["ucla", "leuven", "ucla"]
    idx = np.array([2, 0, 2])
    z_ref = rng.standard_normal(Q)
    h = env.cov.SiteHarmonization(sites, par["grand_mean"], par["beta"], par["shift"], par["scale"], z_ref, env.ctx)

    def loop(xx, ii, zz):
        return HR.apply_loop(xx, ii, zz, par["grand_mean"], par["beta"], par["shift"], par["scale"], z_ref)
    got = h.apply(x, lab, z_u)
    assert got.shape == (C, U, K)
    assert got.tobytes() == loop(x.reshape(C, U * K), np.repeat(idx, K), np.repeat(z_u, K, axis=0)).tobytes()
    got = h.apply(x, np.array(lab), z_uk, as_numpy=False)
    assert tuple(got.shape) == (C, U, K) and got.is_cuda
    assert got.cpu().numpy().tobytes() == loop(x.reshape(C, U * K), np.repeat(idx, K), z_uk.reshape(U * K, Q)).tobytes()
    assert h.apply(x[:, :, 0], lab, z_u).tobytes() == loop(x[:, :, 0], idx, z_u).tobytes()
    with pytest.raises(ValueError, match="did not see"):
        h.apply(x, ["ucla", "leuven", "oslo"], z_u)


# ------------------------------------------------------------------------------------------------
# 3. degenerate rows, exactly; refusals
# ------------------------------------------------------------------------------------------------
def degenerate_rows(rng):
    (B, H, C) = (3, 15, 40)
    idx = np.repeat(np.arange(B), 5).astype(np.uint8)
    b = HR.make_rows(rng, C, idx)
    b[0] = 0.25                                        # constant
    b[1] = np.array([0.1, -0.2, 0.05])[idx]            # constant within each site
    b[2] = np.nan
    b[2, [0, 5, 10]] = [0.1, 0.2, 0.3]                 # n - B_c = 0
    b[3, idx == 1] = np.nan                            # a site missing entirely: the prior's values
    b[4, 6:10] = np.nan                                # n_i = 1
    b[5, idx == 2] = -0.125                            # delta2_hat = 0 at one site
    b[6, 7] = np.nan                                   # one NaN
    b[7] = np.nan                                      # nothing observed
    return B, idx, b


def test_degenerate_rows_exactly(env):
    rng = np.random.default_rng(11)
    (B, idx, b) = degenerate_rows(rng)
    C = b.shape[0]
    ref = HR.fit_ld(b, idx, B, missing=True)
    rows = HR.assert_conditions(ref)
    assert ref["info"][:8, 3].tolist() == [HR.ST_CONSTANT, HR.ST_CONSTANT, HR.ST_DOF, 0, 0, 0, 0, HR.ST_DOF]
    assert ref["info"][2].tolist() == [3, 3, 0, HR.ST_DOF] and ref["info"][7].tolist() == [0, 0, 0, HR.ST_DOF]
    h = env.cov.fit_harmonization(b, idx, missing_data=True, ctx=env.ctx)
    compare(h, ref, rows, label="missing")
    # n_i = 0: exactly the prior; n_i = 1: no delta2_hat, a location from one control
    p = h.prior
    assert h.n_obs[1, 3] == 0 and h.gamma_star[1, 3] == p["gamma_bar"][1] and h.delta2_star[1, 3] == p["b"][1] / (p["a"][1] - 1.0)
    assert h.n_iter[1, 3] == 0 and np.isnan(h.gamma_hat[1, 3]) and h.shift[1, 3] == h.pooled_sd[3] * p["gamma_bar"][1]
    assert h.n_obs[1, 4] == 1 and np.isnan(h.delta2_hat[1, 4]) and np.isfinite(h.gamma_hat[1, 4]) and h.n_iter[1, 4] > 0
    assert h.delta2_hat[2, 5] == 0.0 and h.delta2_star[2, 5] > 0.0
    x = rng.standard_normal((C, 6))
    x[9, 2] = np.nan
    site = np.array([0, 1, 2, 2, 1, 0])
    out = h.apply(x, site)
    for c in (0, 1, 2, 7):
        assert out[c].tobytes() == x[c].tobytes()
    assert out.tobytes() == HR.apply_loop(x, site, np.zeros((6, 0)), h.grand_mean, h.beta, h.shift, h.scale, h.z_ref).tobytes()
    nptest.assert_allclose(out[rows], HR.apply_ld(x, site, None, ref)[rows], **FIT)
    # eb=False: a pair with n_i < 2 or delta2_hat = 0 is left alone
    ref0 = HR.fit_ld(b, idx, B, missing=True, eb=False)
    h0 = env.cov.fit_harmonization(b, idx, missing_data=True, eb=False, ctx=env.ctx)
    compare(h0, ref0, rows, with_prior=False, label="missing, eb=0")
    for (i, c) in ((1, 3), (1, 4), (2, 5)):
        assert h0.shift[i, c] == 0.0 and h0.scale[i, c] == 1.0
    assert h0.gamma_star[1, 4] == h0.gamma_hat[1, 4] and h0.delta2_star[2, 5] == 0.0 and h0.shift[0, 3] != 0.0
    out0 = h0.apply(x, site)
    for (s, c) in ((1, 3), (4, 4), (2, 5), (3, 5)):
        assert out0[c, s] == x[c, s]
    assert out0[3, 0] != x[3, 0]
    # without missing_data a NaN leaves the connection unfitted, every control counts
    plain = env.cov.fit_harmonization(b[[6, 8, 9]], idx, eb=False, ctx=env.ctx)
    assert plain.info.tolist() == [[15, 3, 0, HR.ST_NAN], [15, 3, 0, 0], [15, 3, 0, 0]] and np.all(plain.n_obs == 5)
    for k in REAL[:6]:
        assert np.isnan(getattr(plain, k)[..., 0]).all() and np.isfinite(getattr(plain, k)[..., 1:]).all(), k
    assert np.all(plain.shift[:, 0] == 0.0) and np.all(plain.scale[:, 0] == 1.0)


def test_undefined_prior_and_host_refusals(env):
    rng = np.random.default_rng(12)
    idx = np.repeat(np.arange(2), 4).astype(np.uint8)
    b = np.tile(HR.make_rows(rng, 1, idx), (4, 1))      # identical rows (four: their sum is exact in any order): tau2 = 0
    with pytest.raises(ValueError, match=r"site 1.*eb=False|site 0.*eb=False"):
        env.cov.fit_harmonization(b, idx, ctx=env.ctx)
    h = env.cov.fit_harmonization(b, idx, eb=False, ctx=env.ctx)
    assert np.all(h.info[:, 3] == 0) and np.all(h.gamma_hat == h.gamma_hat[:, :1])
    with pytest.raises(NotImplementedError, match="own design"):
        env.cov.fit_harmonization(b, idx, rng.standard_normal((8, 1)), missing_data=True, ctx=env.ctx)
    env.ctx.check_device()


def test_entry_point_refusals(env):
    rng = np.random.default_rng(13)
    (B, H, C) = (2, 8, 9)
    idx = np.repeat(np.arange(B), 4).astype(np.uint8)
    b = HR.make_rows(rng, C, idx)
    z = HR.make_design(rng, H, 2, idx)
    n_alloc = env.ctx.stat("n_alloc")
    size = ctypes.sizeof(env.lib.HarmonizeDesc)
    for bad in (0, size - 8, size + 8):
        with pytest.raises(ValueError, match="descriptor of"):
            raw_fit(env, b, idx, B, override=dict(size=bad))
    with pytest.raises(NotImplementedError, match="unknown flags"):
        raw_fit(env, b, idx, B, override=dict(flags=4))
    with pytest.raises(NotImplementedError, match="at most 64"):
        raw_fit(env, b, idx, B, override=dict(B=65))
    with pytest.raises(NotImplementedError, match="at most 8"):
        raw_fit(env, b, idx, B, override=dict(Q=9, Qp=0))
    with pytest.raises(NotImplementedError, match="at most 4096"):
        raw_fit(env, b, idx, B, override=dict(H=4097))
    with pytest.raises(NotImplementedError, match="own design"):
        raw_fit(env, b, idx, B, z, flags=env.lib.FCD_DATA_NAN_MISSING)
    for members in (dict(C=0), dict(B=0), dict(H=0), dict(b=None), dict(site=None), dict(info=None), dict(scale=None), dict(Q=-1), dict(Qp=1)):
        with pytest.raises(ValueError):
            raw_fit(env, b, idx, B, override=members)
    with pytest.raises(ValueError, match="null"):
        env.ctx.call("fcd_site_harmonize_fit", None)
    t = env.torch
    par = dict((k, up(env, v, np.float64)) for (k, v) in random_parameters(rng, C, B, 0).items())
    (xd, sd, od) = (up(env, rng.standard_normal((C, 4)), np.float64), up(env, [0, 1, 1, 0], np.uint8), t.full((C, 4), 7.0, dtype=t.float64, device="cuda"))
    for members in (dict(size=12), dict(S=0), dict(C=0), dict(B=0), dict(x=None), dict(out=None), dict(shift=None)):
        with pytest.raises(ValueError):
            raw_apply(env, xd, sd, None, par, np.zeros(0), od, B, override=members)
    with pytest.raises(NotImplementedError, match="at most 64"):
        raw_apply(env, xd, sd, None, par, np.zeros(0), od, B, override=dict(B=65))
    with pytest.raises(NotImplementedError, match="at most 8"):
        raw_apply(env, xd, sd, None, par, np.zeros(0), od, B, override=dict(Q=9))
    t.cuda.synchronize()
    assert np.all(od.cpu().numpy() == 7.0) and env.ctx.stat("n_alloc") == n_alloc and env.ctx.stat("dev_err") == 0
    raw_fit(env, b, idx, B, z)                         # the context is still usable
    env.ctx.check_device()


def test_a_site_id_out_of_range_is_reported(env):
    """checked on the device: status 4 in every row of info, NaN out of apply, the context's error word until it is cleared"""
    rng = np.random.default_rng(14)
    (B, H, C) = (3, 12, 7)
    ctx = env.lib.Context()
    try:
        idx = np.repeat(np.arange(B), 4).astype(np.uint8)
        b = HR.make_rows(rng, C, idx)
        bad = idx.copy()
        bad[5] = B
        got = raw_fit(env, b, bad, B, ctx=ctx)
        assert np.all(got["info"][:, 3] == HR.ST_SITE) and np.isnan(got["grand_mean"]).all() and np.isnan(got["gamma_hat"]).all()
        assert np.all(got["shift"] == 0.0) and np.all(got["scale"] == 1.0) and np.all(got["prior_info"] == 0)
        assert ctx.stat("dev_err") == 2
        with pytest.raises(env.lib.FcdiffHipError, match="site id"):
            ctx.check_device()
        ctx.clear_error()
        ctx.check_device()
        good = raw_fit(env, b, idx, B, ctx=ctx)
        assert np.all(good["info"][:, 3] == 0) and ctx.stat("dev_err") == 0
        t = env.torch
        par = dict((k, up(env, good[k], np.float64)) for k in ("grand_mean", "shift", "scale"))
        x = rng.standard_normal((C, 4))
        od = t.full((C, 4), 7.0, dtype=t.float64, device="cuda")
        raw_apply(env, up(env, x, np.float64), up(env, [0, 200, 2, 1], np.uint8), None, par, np.zeros(0), od, B, ctx=ctx)
        out = od.cpu().numpy()
        assert np.isnan(out[:, 1]).all() and np.isfinite(out[:, [0, 2, 3]]).all() and ctx.stat("dev_err") == 2
        ctx.clear_error()
        ctx.check_device()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 4. determinism, chunking, inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(16, 130, 8, 0.0, True), (64, 130, 0, 0.06, True), (3, 600, 3, 0.0, True)], ids=str)
def test_deterministic_chunked_and_inputs_unchanged(env, case):
    (B, H, Q, nan, _eb) = case
    (idx, z, b, _ref, _rows, _hats) = fit_case(case)
    flags = env.lib.FCD_DATA_NAN_MISSING if nan else 0
    first = raw_fit(env, b, idx, B, z, flags)
    second = raw_fit(env, b, idx, B, z, flags)
    for k in FIT_OUT:
        assert first[k].tobytes() == second[k].tobytes(), k
    (bd, sd, Wd) = first["_inputs"]
    assert bd.cpu().numpy().tobytes() == b.tobytes() and sd.cpu().numpy().tobytes() == idx.tobytes()
    # what does not depend on other connections: the first rows alone give the same bits (the priors do: eb=False)
    whole = raw_fit(env, b, idx, B, z, flags | env.lib.FCD_HARMONIZE_NO_EB)
    for k in ("grand_mean", "pooled_sd", "gamma_hat", "delta2_hat", "n_obs", "info", "beta"):
        assert whole[k].tobytes() == first[k].tobytes(), k
    for C in CS[:2] + (1001,):
        part = raw_fit(env, b[:C], idx, B, z, flags | env.lib.FCD_HARMONIZE_NO_EB)
        for k in FIT_OUT:
            if k in ("prior", "prior_info"):
                continue
            w = whole[k][:C] if FIT_OUT[k][0][0] == "C" else whole[k][:, :C]
            assert part[k].tobytes() == np.ascontiguousarray(w).tobytes(), (C, k)


# ------------------------------------------------------------------------------------------------
# 5. end to end: the scenario through the fit, new patients
# ------------------------------------------------------------------------------------------------
def new_fit(env, model, b, bt, **kw):
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    (fit.model, fit.b, fit.bt) = (model, b, bt)
    for (k, v) in kw.items():
        setattr(fit, k, v)
    return fit


def scenario_model(env):
    m = env.pkg.UnsharedRegionModel()
    m.pi = HR.SCENARIO["pi"]
    return m


def test_scenario_through_the_fit(env):
    """
    test_harmonize.py's scenario: harmonize() on the device, then UnsharedRegionFit (vb, 8 iterations, symmetric edge ids).
    lq_R is the reference loop's on the REFERENCE's harmonised arrays at FIT, the flagged sets are the same, and score() takes
    new patients that went through h.apply.
    """
    s = HR.SCENARIO
    (_b0, _bt0, b, bt, site_b, site_bt, r) = HR.scenario_data(scenario_model(env))
    start = theta_dict(scenario_model(env).theta())
    (b_ref, bt_ref, ref) = HR.harmonize_ld(b, bt, site_b, site_bt)
    rows = HR.assert_conditions(ref)
    assert rows.size == b.shape[0]
    (b_h, bt_h, h) = env.cov.harmonize(b, bt, site_b, site_bt, ctx=env.ctx)
    compare(h, ref, rows, label="scenario")
    nptest.assert_allclose(b_h, b_ref, **FIT)
    nptest.assert_allclose(bt_h, bt_ref, **FIT)
    fit = new_fit(env, scenario_model(env), b_h, bt_h, max_iters=s["iters"], rel_tol=-np.inf, edge_index="symmetric")
    fit.run()
    want = NR.vb_fit(b_ref, bt_ref, start, s["iters"], O.EDGE_SYMMETRIC)
    rates = HR.scenario_rates(fit._lq_R, r)
    print("harmonised: flagged %.4f found %.2f; max |d lq_R| %.3g" % (rates + (np.abs(fit._lq_R - want["lq_R"]).max(),)))
    nptest.assert_allclose(fit._lq_R, want["lq_R"], **FIT)
    assert np.array_equal(np.exp(fit._lq_R[:, :, 1]) > 0.5, np.exp(want["lq_R"][:, :, 1]) > 0.5)
    assert rates == HR.scenario_rates(want["lq_R"], r) and rates[0] <= 0.02 and rates[1] >= 0.80
    # new patients of site 1 and of site 0
    (_r, _t, _f, _ft, _b, bt_new) = scenario_model(env).sample_fast(s["N"], s["H"], 3, seed=9)
    bt_new = np.array(bt_new, dtype=np.float64)
    new_h = h.apply(bt_new, [1, 0, 1])
    assert new_h.tobytes() == HR.apply_loop(bt_new, np.array([1, 0, 1]), np.zeros((3, 0)), h.grand_mean, h.beta, h.shift, h.scale, h.z_ref).tobytes()
    got = fit.score(new_h, max_iters=6, tol=0.0)
    assert got["p_R"].shape == (s["N"], 3) and np.all(np.isfinite(got["p_R"]))


# ------------------------------------------------------------------------------------------------
# 6. the two protocols of tests/caller_stream_cases.py for the two entry points
#
# Their prototypes carry the stream inside the descriptor, so the registry's parser does not see them and its list holds no
# case for them.  The cases are built here with the constructor (the case() decorator appends to the shared list) and
# driven the way tests/test_gpu_caller_stream.py and tests/test_gpu_context_reuse.py drive theirs.
# ------------------------------------------------------------------------------------------------
HARM_DIMS = {17: dict(H=12, B=3, Q=2, S=5), 33: dict(H=40, B=5, Q=3, S=9)}          # by the registry's N: small, large


def _harm_build(eb, missing):
    def build(d):
        from fcdiff_amd import covariates
        e = HARM_DIMS[d["N"]]
        (C, H, B, S) = (R.tri(d["N"]), e["H"], e["B"], e["S"])
        Q = 0 if missing else e["Q"]
        rng = np.random.default_rng([91, d["N"], int(eb), int(missing)])
        idx = HR.make_sites(rng, H, B)
        z = HR.make_design(rng, H, Q, idx)
        b = HR.make_rows(rng, C, idx, z, 0.1 if missing else 0.0)
        (W, T, z_bar, _info) = covariates.site_design(z, idx, B)
        assert W.shape[1] == Q
        inputs = dict(b=b, site=idx, x=0.3 * rng.standard_normal((C, S)), site_x=rng.integers(0, B, S).astype(np.uint8))
        if Q:
            inputs.update(W=W, z=HR.make_design(rng, S, Q, inputs["site_x"]))
        outs = out_shapes(C, B, Q)
        if not Q:
            del outs["beta"]
        outs["out"] = ((C, S), np.float64)
        flags = (R.MISSING if missing else 0) | (0 if eb else 2)
        return dict(inputs=inputs, outputs=outs, host=dict(C=C, H=H, B=B, Q=Q, S=S, flags=flags, T=T, z_bar=z_bar, z_ref=np.ascontiguousarray(z.mean(axis=0))))
    return build


def _harm_call(ctx, i, o, h):
    L = R._lib()
    Q = h["Q"]
    host = dict(T=h["T"].ctypes.data if Q else None, z_bar=h["z_bar"].ctypes.data if Q else None, z_ref=h["z_ref"].ctypes.data if Q else None)
    outs = dict((k, R.P(v)) for (k, v) in o.items() if k != "out")
    d = L.HarmonizeDesc.make(flags=h["flags"], C=h["C"], H=h["H"], B=h["B"], Q=Q, Qp=Q, stream=R.ST(), b=R.P(i["b"]), site=R.P(i["site"]),
                             W=R.P(i.get("W")), **dict(host, **outs))
    ctx.call("fcd_site_harmonize_fit", ctypes.byref(d))
    d = L.HarmonizeDesc.make(C=h["C"], S=h["S"], B=h["B"], Q=Q, stream=R.ST(), x=R.P(i["x"]), site=R.P(i["site_x"]), z=R.P(i.get("z")),
                             z_ref=host["z_ref"], grand_mean=R.P(o["grand_mean"]), beta=R.P(o.get("beta")), shift=R.P(o["shift"]),
                             scale=R.P(o["scale"]), out=R.P(o["out"]))
    ctx.call("fcd_site_harmonize_apply", ctypes.byref(d))


def _harm_conditions(s):
    h = s["host"]
    z = None
    if h["Q"]:
        # the covariates the design was made from are not an input of the call: the reference takes the basis itself, which
        # spans the same columns
        z = s["inputs"]["W"]
    ref = HR.fit_ld(s["inputs"]["b"], s["inputs"]["site"], h["B"], z, missing=bool(h["flags"] & R.MISSING), eb=not h["flags"] & 2)
    assert len(HR.assert_conditions(ref)) >= 0.9 * h["C"]


EPS = ["fcd_site_harmonize_fit", "fcd_site_harmonize_apply"]
HARM_CASES = [R.Case("site_harmonize_eb", EPS, _harm_build(True, False), _harm_call, conditions=_harm_conditions),
              R.Case("site_harmonize_missing_no_eb", EPS, _harm_build(False, True), _harm_call, conditions=_harm_conditions)]


def test_the_cases_are_what_the_registry_asks_of_a_case():
    """(needs no device beyond the mark of this file) deterministic, larger at "large", not in the shared list"""
    for case in HARM_CASES:
        assert case not in R.CASES and case.name not in R.BY_NAME
        for size in R.SIZES:
            (a, b) = (case.make(size), case.make(size))
            for k in a:
                assert a[k].tobytes() == b[k].tobytes() and a[k].flags["C_CONTIGUOUS"]
            case.conditions(size)
        (small, large) = (case.extents("small"), case.extents("large"))
        assert sorted(small) == sorted(large) and all(np.prod(large[k]) >= np.prod(small[k]) for k in small) and small != large


@pytest.fixture(scope="module")
def stream_gpu(env):
    import test_gpu_caller_stream as CSM
    dev = env.torch.device("cuda", 0)
    delay = CSM.Delay(env.torch, dev)
    return dict(torch=env.torch, lib=env.lib, device=dev, delay=delay, streams=CSM.independent_streams(env.torch, delay, 2))


@pytest.mark.parametrize("case", HARM_CASES, ids=lambda c: c.name)
def test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case):
    """the protocol of tests/test_gpu_caller_stream.py, by its own function: the inputs are poison (NaN, site ids 0xFF) until
    the producer has run, the host is through the calls before that, and the outputs are those of a plain run byte for byte"""
    import test_gpu_caller_stream as CSM
    CSM.test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case)


@pytest.mark.parametrize("case", HARM_CASES, ids=lambda c: c.name)
def test_on_a_context_that_other_families_have_used(env, case):
    """the protocol of tests/test_gpu_context_reuse.py: after fcd_edge_cov_fit, fcd_baseline_group_perm and fcd_gibbs_run at
    another shape, and those again after it; every output equals that of a fresh context byte for byte"""
    dev = env.torch.device("cuda", 0)
    others = [R.BY_NAME[n] for n in ("edge_cov_fit_apply", "baseline_group_perm", "gibbs_run_run_form")]
    ctx = env.lib.Context()

    def check(c, size, where):
        (want, want_stats) = R.fresh(c, size, dev)
        (got, stats) = R.run_once(ctx, c, size, dev, stats=True)
        bad = R.differing(got, want)
        assert not bad, "%s: %s/%s differs from a fresh context in %s" % (where, c.name, size, bad)
        assert stats == want_stats and ctx.stat("dev_err") == 0, (where, c.name, size)
    try:
        for (mine, theirs) in (("small", "large"), ("large", "small")):
            for c in others:
                check(c, theirs, "before %s" % mine)
            check(case, mine, "after the others at %s" % theirs)
            n_alloc = ctx.stat("n_alloc")
            desc = env.lib.HarmonizeDesc.make()
            assert getattr(ctx.lib, EPS[0])(ctx.handle, ctypes.byref(desc)) < 0 and ctx.stat("n_alloc") == n_alloc      # a refused call
            check(case, mine, "after a refusal")
        for c in others:
            check(c, "small", "at the end")
        ctx.check_device()
    finally:
        ctx.close()
