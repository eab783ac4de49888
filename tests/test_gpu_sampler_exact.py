"""
The device forward sampler (fcd_sample.hip behind UnsharedRegionModel.sample_gpu and SharedRegionModel.sample_gpu)
against its NumPy restatement tests/sampler_ref.py, element for element.

The sampler is counter-based, so nothing here is statistical: r, t, f and f~ must be EQUAL to the reference's (their
uniforms are exact 53-bit values and every comparison is of two doubles), b and b~ must agree to sigma_k 1e-13 with k
the reference's component.  That bound is reasoned, not measured: z = sqrt(-2 log u1) cos(2 pi u2) with |z| <= 8.57 (a
53-bit u1), the argument of the cosine up to 2 pi carries a rounding error of a few 2^-53 2 pi = 7e-16 which the
cosine passes on at most as it is, log and sqrt add a few ulp of a value below 8.6 (1e-15 each at most), and mu +
sigma z is one product and one sum (the library is built without contraction; one fused step would change one rounding
of 1 ulp of |sigma z| <= 8.57 sigma 1.1e-16): in all below sigma 1e-14, and 1e-13 leaves a decade.  It is far
below what a wrong uniform, a wrong component or a swapped half of the Philox block would give (of the order of sigma).

What this file cannot reach: the high counter word (index >> 32) is zero for every size that fits a test (C U >= 2^32
items are 34 GB of b~ alone).  tests/test_sampler_ref.py pins the reference's use of it to the oracle's Philox; the
kernel's is read, not run.
"""
import numpy as np
import pytest

import sampler_ref as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib) = (torch, fcdiff_amd, _lib)
    e.ctx = _lib.Context()
    return e


def model(env, shared, theta):
    m = env.pkg.SharedRegionModel() if shared else env.pkg.UnsharedRegionModel()
    (m.pi, m.eta, m.epsilon) = (float(theta[0]), float(theta[1]), float(theta[2]))
    (m.gamma, m.mu, m.sigma) = (theta[3:6].copy(), theta[6:9].copy(), theta[9:12].copy())
    assert np.array_equal(m.theta(), theta)
    return m


_ref = {}


def reference(name, N, H, U, seed, shared):
    key = (name, N, H, U, seed, shared)
    if key not in _ref:
        _ref[key] = SR.sample(SR.THETAS[name], N, H, U, seed, shared=shared)
    return _ref[key]


@pytest.mark.parametrize("seed", SR.SEEDS)
@pytest.mark.parametrize("name", sorted(SR.THETAS))
@pytest.mark.parametrize("N,H,U", SR.SHAPES)
@pytest.mark.parametrize("shared", [False, True])
def test_sampler_equals_its_restatement(env, shared, N, H, U, name, seed):
    theta = SR.THETAS[name]
    (r, t, f, ft, b, bt) = model(env, shared, theta).sample_gpu(N, H, U, seed=seed, ctx=env.ctx)
    ref = reference(name, N, H, U, seed, shared)
    C = N * (N - 1) // 2
    assert r.shape == ((N,) if shared else (N, U)) and r.dtype == bool and t.shape == (C, U) and t.dtype == bool
    assert f.shape == (C, 3) and ft.shape == (C, U, 3) and b.shape == (C, H) and bt.shape == (C, U)
    assert (f.sum(axis=1) == 1).all() and (ft.sum(axis=2) == 1).all()
    assert np.array_equal(r, ref["r"]), "r"
    assert np.array_equal(np.argmax(f, axis=1), ref["f"]), "f"
    assert np.array_equal(t, ref["t"]), "t"
    assert np.array_equal(np.argmax(ft, axis=2), ref["ft"]), "f~"
    sigma = theta[9:12]
    for (what, got, exp, k) in (("b", b, ref["b"], np.broadcast_to(ref["f"][:, None], b.shape)), ("b~", bt, ref["bt"], ref["ft"])):
        assert np.isfinite(got).all() and np.abs(got).max() <= 1.0, what
        err = np.abs(got - exp) / sigma[k]
        assert err.max() <= 1e-13, "%s: worst |error| / sigma %.3e" % (what, err.max())
        clipped = np.abs(exp) == 1.0
        assert np.array_equal(got[clipped], exp[clipped]), "%s at the clip" % what


def test_edge_parameters_reach_the_clip_on_the_device(env):
    """The equality at the clip bound is not vacuous: the edge set's components put a few per cent of b and b~ there."""
    ref = reference("edge", 40, 6, 50, SR.SEEDS[0], False)
    assert (np.abs(ref["b"]) == 1.0).mean() > 0.01 and (np.abs(ref["bt"]) == 1.0).mean() > 0.01
    (_r, _t, _f, _ft, b, bt) = model(env, False, SR.THETA_EDGE).sample_gpu(40, 6, 50, seed=SR.SEEDS[0], ctx=env.ctx)
    assert np.array_equal(np.abs(b) == 1.0, np.abs(ref["b"]) == 1.0) and np.array_equal(np.abs(bt) == 1.0, np.abs(ref["bt"]) == 1.0)
