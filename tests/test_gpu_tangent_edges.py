"""
The tangent-space kernels (fcd_corr_tangent.hip) where tests/test_gpu_tangent.py does not take them: region counts above the 96
up to which the eigensolver keeps its matrices in LDS and region counts that are whole tiles, the two switch points of the
solver's launch, its batch loop, matrices that are graded, tiny, huge, infinite or overflowing, and subjects whose M_s has a
condition number of 1e3 to 2e10, up to and across the 1e-12 of status 1.

  1  fcd_sym_eigh at n = 1, 32 (the last 256-thread workgroup; 33 is in the neighbour), 96 (the last LDS form: ld = 97, 146 KB)
     and 97 (the first in scratch), batches of 3
  2  n = 33: a matrix graded over 16 decades; ldexp(A, k) must give ldexp(w, k) and the bytes of V (every step of the kernel,
     the threshold included, is exactly covariant under a power of two); k = -520 and +500, where ||A||_F^2 is denormal or close
     to the overflow; +inf, -inf and an overflowing ||A||_F^2 give status 1 and leave their neighbours' bits alone
  3  the batch loop of fcd_sym_eigh, bounded by the knob "tangent_chunk": the bits and the status words of the unchunked call,
     in LDS (n = 17) and in the scratch that successive chunks reuse (n = 130)
  4  apply and both fits at 97 regions (the pipeline's own call of the solver -- padded leading dimensions, status stride 2,
     the chunk's scratch slot -- on the scratch form) and at 32 regions (PL = Nreg: no padding, no zero rows of V)
  5  apply on 12 frames of 17 regions with a fixed alpha of 1e-3 .. 1e-9: kappa(M_s) = 1.7e3 .. 2e9; alpha = 1e-10 (kappa 2e10,
     status 0) and 1e-14 (status 1) beside a well-conditioned subject

Bounds: the units of tests/tangent_ref.py; the device is held to MARGIN * max(R_x, R_x_EDGE), R_x_EDGE = the worst ratio of the
oracle's fp64 route to its longdouble route over exactly the inputs used here (tangent_ref.tangent_edge_cases(),
eigh_edge_cases(); tests/test_tangent.py asserts that the record has not grown, and that the inputs have the kappa claimed here).
The max: R_x is the family's established sample in the same units, and an input on which LAPACK does very well (0.006 at 97
regions) must not tighten what the same algorithm is already allowed.

Not tested, on purpose.  Status 2 (no convergence in 40 sweeps) cannot be produced honestly: cyclic Jacobi converges
quadratically on every finite symmetric matrix, the graded one here takes 4 sweeps on the oracle's fp64 run.  The branch
fabs(theta) > 1e150 of the rotation cannot be reached.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tangent_ref as TR  # noqa: E402
from test_gpu_tangent import check_apply, check_eigh, env  # noqa: E402,F401

pytestmark = pytest.mark.gpu

K_T = TR.MARGIN * max(TR.R_T, TR.R_T_EDGE)
K_EIGH = (TR.MARGIN * max(TR.R_EIGH_W, TR.R_EIGH_W_EDGE), TR.MARGIN * max(TR.R_EIGH_RES, TR.R_EIGH_RES_EDGE),
          TR.MARGIN * max(TR.R_EIGH_ORTH, TR.R_EIGH_ORTH_EDGE))
TOL = 1e-10


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ------------------------------------------------------------------------------------------------
# 1. the sizes at which the launch changes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TR.EIGH_EDGE_SIZES)
def test_sym_eigh_at_the_switch_points(env, n):
    batch = TR.eigh_edge_cases()["size_%d" % n]
    ref = TR.eigh_edge_reference("size_%d" % n)
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert w.shape == (3, n) and V.shape == (3, n, n) and np.array_equal(st, np.zeros(3))
    for b in range(3):
        check_eigh(batch[b], w[b], V[b], ref[b], "n = %d, matrix %d" % (n, b), K_EIGH)
    (w1, V1, st1) = env.corr.sym_eigh(batch[-1], ctx=env.ctx)
    assert st1 == 0 and same(w1, w[-1]) and same(V1, V[-1])
    if n == 1:
        assert same(w[:, 0], batch[:, 0, 0]) and np.array_equal(V, np.ones((3, 1, 1)))


# ------------------------------------------------------------------------------------------------
# 2. scale
# ------------------------------------------------------------------------------------------------
def test_sym_eigh_graded_matrix(env):
    A = TR.eigh_edge_cases()["graded_%d" % TR.SCALE_N][0]
    (w, V, st) = env.corr.sym_eigh(A, ctx=env.ctx)
    assert st == 0
    check_eigh(A, w, V, TR.eigh_edge_reference("graded_%d" % TR.SCALE_N)[0], "graded over 16 decades", K_EIGH)


def test_sym_eigh_is_covariant_under_powers_of_two(env):
    A = TR.scale_matrix()
    (w0, V0, st0) = env.corr.sym_eigh(A, ctx=env.ctx)
    assert st0 == 0
    (w, V, st) = env.corr.sym_eigh(np.stack([np.ldexp(A, k) for k in TR.SCALE_EXACT]), ctx=env.ctx)
    assert np.array_equal(st, np.zeros(len(TR.SCALE_EXACT)))
    for (i, k) in enumerate(TR.SCALE_EXACT):
        d = np.abs(np.ldexp(w[i], -k) - w0).max() / np.abs(w0).max()
        print("2^%d: |2^-k w - w0| / |w0| = %.3g (0 wanted), V differs in %d of %d entries" % (k, d, (V[i] != V0).sum(), V0.size))
        assert same(w[i], np.ldexp(w0, k)) and same(V[i], V0), k


def test_sym_eigh_extreme_scales(env):
    name = "extreme_%d" % TR.SCALE_N
    batch = TR.eigh_edge_cases()[name]
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert np.array_equal(st, np.zeros(len(batch)))
    for (b, k) in enumerate(TR.SCALE_EXTREME):
        check_eigh(batch[b], w[b], V[b], TR.eigh_edge_reference(name)[b], "scaled by 2^%d" % k, K_EIGH)


def test_sym_eigh_infinities_and_overflow(env):
    good = TR.eigh_cases()["size_33"][:3]
    (w0, V0, st0) = env.corr.sym_eigh(good, ctx=env.ctx)
    assert np.array_equal(st0, np.zeros(3))
    (plus, minus) = (good[1].copy(), good[1].copy())
    (plus[20, 7], minus[32, 32]) = (np.inf, -np.inf)
    huge = np.ldexp(TR.scale_matrix(), TR.SCALE_OVERFLOW)
    assert np.isfinite(huge).all()
    batch = np.stack([good[0], plus, good[1], minus, huge, good[2]])
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert list(st) == [0, 1, 0, 1, 1, 0]
    for b in (1, 3, 4):
        assert np.isnan(w[b]).all() and np.isnan(V[b]).all(), b
    for (b, g) in ((0, 0), (2, 1), (5, 2)):
        assert same(w[b], w0[g]) and same(V[b], V0[g]), b


# ------------------------------------------------------------------------------------------------
# 3. the batch loop
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, chunks", ((17, (2, 1)), (130, (1,))))
def test_sym_eigh_chunks_change_no_bit(env, n, chunks):
    batch = TR.eigh_cases()["size_%d" % n]
    B = len(batch)
    assert B == (5 if n == 17 else 2)
    (w0, V0, st0) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert np.array_equal(st0, np.zeros(B))
    for chunk in chunks:
        (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx, _max_chunk=chunk)
        assert same(w, w0) and same(V, V0) and same(st, st0), chunk
    # a NaN matrix in the second chunk: its status word at its index, nothing else moves
    bad = batch.copy()
    at = B - 2 if n == 17 else 1
    bad[at, n - 1, 2] = np.nan
    (w, V, st) = env.corr.sym_eigh(bad, ctx=env.ctx, _max_chunk=chunks[0])
    assert list(st) == [1 if b == at else 0 for b in range(B)]
    assert np.isnan(w[at]).all() and np.isnan(V[at]).all()
    keep = np.arange(B) != at
    assert same(w[keep], w0[keep]) and same(V[keep], V0[keep])
    # the knob is back at 0: a later call is unchunked and equal
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert same(w, w0) and same(V, V0) and same(st, st0)


# ------------------------------------------------------------------------------------------------
# 4. the pipeline above 96 regions and at whole tiles
# ------------------------------------------------------------------------------------------------
def space_of(env, fit_name, shrinkage):
    """the oracle's G on the host: no error of the device's fit enters apply"""
    return env.corr.TangentSpace.from_reference(TR.edge_fit(fit_name)["G"].astype(np.float64), shrinkage)


def check_identities(sp, Nreg, kappa_G, norm_G, what):
    """W G W = I and G^1/2 G^1/2 = G at the rounding of two products at kappa(G), as test_fit_reference"""
    unit = K_T * Nreg * TR.EPS * kappa_G
    e1 = np.abs(sp.whitening.dot(sp.reference).dot(sp.whitening) - np.eye(Nreg)).max()
    e2 = np.abs(sp.reference_sqrt.dot(sp.reference_sqrt) - sp.reference).max()
    print("%s: |W G W - I| %.3g of %.3g, |Gh Gh - G| %.3g of %.3g" % (what, e1, 4 * unit, e2, 4 * unit * norm_G))
    assert np.array_equal(sp.reference, sp.reference.T) and np.array_equal(sp.whitening, sp.whitening.T)
    assert e1 <= 4 * unit and e2 <= 4 * unit * norm_G, what


def test_apply_at_97_regions(env):
    c = TR.tangent_edge_cases()["apply_97_60_3"]
    sp = space_of(env, c["fit"], c["shrinkage"])
    (out, info) = sp.apply(c["ts"], ctx=env.ctx, return_info=True)
    assert out.shape == (97 * 96 // 2, 3) and info["diag"].shape == (97, 3)
    ref0 = check_apply(out, info, c["ts"], sp.whitening, None, "97 regions, S = 3, Ledoit-Wolf", c["kappa"][1], K_T)
    assert np.all(np.abs(info["alpha"] - ref0["alpha"]) <= ref0["tol_alpha"])
    # a chunk of 2 and a chunk of 1 in the same scratch slot
    (o, i) = sp.apply(c["ts"], ctx=env.ctx, return_info=True, _max_chunk=2)
    assert same(o, out) and same(i["diag"], info["diag"]) and same(i["alpha"], info["alpha"]) and np.array_equal(i["status"], info["status"])


def test_euclidean_fit_at_97_regions(env):
    (tc, sh, kind) = TR.edge_fits()["97_60_3"]
    (H, Nreg, T) = tc.shape
    ref = TR.edge_fit("97_60_3")
    sp = env.corr.fit_tangent(tc, sh, kind, ctx=env.ctx)
    assert sp.info["used"].all() and np.array_equal(sp.info["status"], ref["status"]) and np.array_equal(sp.info["n_live"], ref["n_live"])
    assert np.all(np.abs(sp.info["alpha"] - ref["alpha"]) <= ref["tol_alpha"]) and sp.info["n_iter"] == 0
    dG = np.abs(sp.reference - TR.euclidean_mean(tc, sp.info["alpha"]).astype(np.float64)).max()
    bound = (T + 4 + H + 2) * TR.EPS
    print("euclidean fit at 97 regions: |dG| %.3g of %.3g" % (dG, bound))
    assert dG <= bound
    check_identities(sp, Nreg, ref["kappa_G"], ref["norm_G"], "euclidean fit at 97 regions")


def test_geometric_fit_at_97_regions_is_stationary(env):
    """The longdouble fixed point costs 50 s at this size; what it would pin is that the device's W makes the mean tangent vector
    of the controls vanish, and that the oracle can check at the device's W and alpha with one decomposition a control.
    ||Tbar||_F <= tol sqrt(p) is the stopping rule on the device's own Tbar; each of its p^2 entries is within
    K_T p eps max_s kappa(M_s) of the oracle's, so the oracle's norm is within p times that.
    kappa and the norm of the geometric G for the two identities: harmonic <= geometric <= arithmetic mean in the Loewner
    order, so lambda_max(G) <= lambda_max of the Euclidean mean and lambda_min(G) >= the smallest lambda_min of the R_a."""
    (tc, sh, _kind) = TR.edge_fits()["97_60_3"]
    p = tc.shape[1]
    ref = TR.edge_fit("97_60_3")
    sp = env.corr.fit_tangent(tc, sh, "geometric", ctx=env.ctx, tol=TOL)
    assert sp.info["used"].all() and np.array_equal(sp.info["status"], np.zeros(3))
    assert np.all(np.abs(sp.info["alpha"] - ref["alpha"]) <= ref["tol_alpha"])
    assert sp.info["n_iter"] > 0 and sp.info["grad_norm"] <= TOL * np.sqrt(p)
    (Tbar, kappa) = TR.mean_tangent(tc, sp.whitening, sp.info["alpha"])
    nrm = float(np.sqrt((Tbar * Tbar).sum()))
    bound = TOL * np.sqrt(p) + p * K_T * p * TR.EPS * kappa.max()
    print("geometric fit at 97 regions: %d iterations, device norm %.3g, oracle's norm at the device's W %.3g of %.3g; kappa <= %.3g"
          % (sp.info["n_iter"], sp.info["grad_norm"], nrm, bound, kappa.max()))
    assert nrm <= bound
    check_identities(sp, p, ref["norm_G"] / ref["lam_min"].min(), ref["norm_G"], "geometric fit at 97 regions")


@pytest.mark.parametrize("kind", ("euclidean", "geometric"))
def test_fit_at_32_regions(env, kind):
    """test_fit_reference of the neighbour at PL = Nreg, against the longdouble fit"""
    (tc, sh, _kind) = TR.edge_fits()["32_40_6"]
    (H, Nreg, T) = tc.shape
    sp = env.corr.fit_tangent(tc, sh, kind, ctx=env.ctx, tol=TOL)
    ref = TR.edge_fit("32_40_6") if kind == "geometric" else TR.fit(tc, shrinkage=sh, reference=kind)
    assert sp.info["used"].all() and np.array_equal(sp.info["status"], ref["status"]) and np.array_equal(sp.info["n_live"], ref["n_live"])
    assert np.all(np.abs(sp.info["alpha"] - ref["alpha"]) <= ref["tol_alpha"])
    if kind == "euclidean":
        dG = np.abs(sp.reference - TR.euclidean_mean(tc, sp.info["alpha"]).astype(np.float64)).max()
        bound = (T + 4 + H + 2) * TR.EPS
        assert sp.info["n_iter"] == 0
    else:
        dG = np.abs(sp.reference - ref["G"].astype(np.float64)).max()
        bound = ref["norm_G"] * (2 * TOL * np.sqrt(Nreg) + K_T * Nreg * TR.EPS * ref["kappa_G"])
        assert abs(sp.info["n_iter"] - ref["n_iter"]) <= 2 and ref["n_iter"] > 0
        assert sp.info["grad_norm"] <= TOL * np.sqrt(Nreg)
    print("32 regions, %s: |dG| %.3g of %.3g, n_iter %d (oracle %d), norm %.3g" % (kind, dG, bound, sp.info["n_iter"], ref["n_iter"], sp.info["grad_norm"]))
    assert dG <= bound
    check_identities(sp, Nreg, ref["kappa_G"], ref["norm_G"], "32 regions, %s" % kind)
    if kind == "geometric":
        (out, info) = sp.apply(tc, ctx=env.ctx, return_info=True)
        nrm = np.sqrt(2 * (out.mean(axis=1) ** 2).sum() + (info["diag"].mean(axis=1) ** 2).sum())
        assert nrm <= TOL * np.sqrt(Nreg) * (1 + 1e-3)


def test_apply_at_32_regions(env):
    c = TR.tangent_edge_cases()["apply_32_40_33"]
    sp = space_of(env, c["fit"], c["shrinkage"])
    (out, info) = sp.apply(c["ts"], ctx=env.ctx, return_info=True)
    assert out.shape == (32 * 31 // 2, 33) and info["diag"].shape == (32, 33)
    ref0 = check_apply(out, info, c["ts"], sp.whitening, None, "32 regions, S = 33, Ledoit-Wolf", c["kappa"][1], K_T)
    assert np.all(np.abs(info["alpha"] - ref0["alpha"]) <= ref0["tol_alpha"])


# ------------------------------------------------------------------------------------------------
# 5. conditioning
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", TR.LADDER_ALPHAS)
def test_apply_on_the_conditioning_ladder(env, alpha):
    c = TR.tangent_edge_cases()["ladder_%g" % alpha]
    sp = space_of(env, c["fit"], alpha)
    (out, info) = sp.apply(c["ts"], ctx=env.ctx, return_info=True)
    assert np.array_equal(info["alpha"], np.full(4, alpha)) and np.array_equal(info["status"], np.zeros(4))
    check_apply(out, info, c["ts"], sp.whitening, None, "12 frames of 17 regions, alpha = %g" % alpha, c["kappa"][1], K_T)


def test_apply_on_either_side_of_the_singular_status(env):
    """alpha = 1e-10: lambda_min / lambda_max = 5e-11, status 0; alpha = 1e-14: 5e-15, status 1 and NaN columns.  Subject 0 keeps
    all its frames and is well conditioned; in both batches it has the bits it has alone."""
    for (alpha, want) in zip(TR.BOUNDARY_ALPHAS, ([0, 0, 0, 0], [0, 1, 1, 1])):
        c = TR.tangent_edge_cases()["boundary_%g" % alpha]
        sp = space_of(env, c["fit"], alpha)
        mask = np.arange(40)[None, :] < c["n_frames"][:, None]
        (out, info) = sp.apply(c["ts"], frame_mask=mask, ctx=env.ctx, return_info=True)
        assert list(info["status"]) == want, alpha
        bad = np.array(want) != 0
        assert np.isnan(out[:, bad]).all() and np.isnan(info["diag"][:, bad]).all() and np.isfinite(out[:, ~bad]).all()
        (resid, cinfo) = env.corr.clean(c["ts"], frame_mask=mask, ctx=env.ctx)
        assert np.array_equal(cinfo[:, 0], c["n_frames"])
        check_apply(out, info, resid, sp.whitening, cinfo[:, 0], "alpha = %g beside a well-conditioned subject" % alpha, c["kappa"][1], K_T)
        (o1, i1) = sp.apply(c["ts"][:1], frame_mask=mask[:1], ctx=env.ctx, return_info=True)
        assert i1["status"][0] == 0 and same(o1[:, 0], out[:, 0]) and same(i1["diag"][:, 0], info["diag"][:, 0])
