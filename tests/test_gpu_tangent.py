"""
fcd_sym_eigh, fcd_tangent_fit and fcd_tangent_apply (fcdiff_amd.corr.sym_eigh, fit_tangent, TangentSpace, tangent) against the
oracle of tests/tangent_ref.py.

Bounds.  The units are the oracle's (its module docstring): an entry of T_s in n eps kappa(M_s), sym_eigh's eigenvalues and
residual in n eps ||A||_2, V^T V - I in n eps; kappa and the norms are the oracle's.  The device is held to
K = 16 r, r = tangent_ref.R_* = the worst ratio of the oracle's own fp64 route to its longdouble route over exactly the inputs
used here (tests/test_tangent.py asserts that the recorded r has not grown).  T_s is compared with the oracle EVALUATED AT THE
DEVICE'S alpha (one error is not counted twice); alpha itself within the oracle's tol_alpha, as tests/test_gpu_partial_corr.py.
The reference G:
  euclidean   a running sum of H correlation matrices with entries <= 1, each entry a normalised sum of T products, then one
              division: |dG| <= (T + 4 + H + 2) eps;
  geometric   the fit is defined up to its stopping rule: ||Tbar||_F <= tol sqrt(p) leaves G within a factor exp(+-tol sqrt(p))
              of the Frechet mean in the affine-invariant metric, for the device and for the oracle alike, so
              |dG| <= ||G||_2 (2 tol sqrt(p) + K n eps kappa(G)) -- the second term is the rounding of one evaluation of the
              chain, propagated through G^1/2 . G^1/2 at the oracle's kappa(G).
Shapes: the eigensolver at n = 2, 3 (one pair; the bye), 15 / 16 / 17 and 47 / 64 / 65 (tile and padding edges), 33, and 130
(above the 96 up to which the matrices stay in LDS); the embedding at S = 1, 31, 32, 33, 65 (the 32-subject tiles of the emit
kernel) and in chunks of 7, 32, 33.
"""
import ctypes

import numpy as np
import pytest

import caller_stream_cases as R
import tangent_ref as TR

pytestmark = pytest.mark.gpu

K_T = TR.MARGIN * TR.R_T
(K_W, K_RES, K_ORTH) = (TR.MARGIN * TR.R_EIGH_W, TR.MARGIN * TR.R_EIGH_RES, TR.MARGIN * TR.R_EIGH_ORTH)


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd import corr
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib, e.corr) = (torch, fcdiff_amd, _lib, corr)
    e.ctx = _lib.Context()
    return e


# ------------------------------------------------------------------------------------------------
# 1, 2. the eigensolver
# ------------------------------------------------------------------------------------------------
def check_eigh(A, w, V, w_ref, what, bounds=None):
    """bounds: (K_W, K_RES, K_ORTH) of a caller with inputs and recorded ratios of its own (tests/test_gpu_tangent_edges.py)"""
    (k_w, k_res, k_orth) = (K_W, K_RES, K_ORTH) if bounds is None else bounds
    (e_w, e_res, e_orth) = TR.eigh_errors(A, w, V, w_ref)
    print("%s: eigenvalues %.3g of %.3g, residual %.3g of %.3g, orthogonality %.3g of %.3g" % (what, e_w, k_w, e_res, k_res, e_orth, k_orth))
    assert np.all(np.diff(w) >= 0), what
    assert e_w <= k_w and e_res <= k_res and e_orth <= k_orth, what


@pytest.mark.parametrize("n", TR.EIGH_SIZES)
def test_sym_eigh_sizes_and_batches(env, n):
    batch = TR.eigh_cases()["size_%d" % n]
    ref = TR.eigh_reference("size_%d" % n)
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert w.shape == batch.shape[:2] and V.shape == batch.shape and np.array_equal(st, np.zeros(len(batch)))
    for b in range(len(batch)):
        check_eigh(batch[b], w[b], V[b], ref[b], "n = %d, matrix %d" % (n, b))
    # B = 1, and a matrix alone has the bits it has inside the batch
    (w1, V1, st1) = env.corr.sym_eigh(batch[-1], ctx=env.ctx)
    assert st1 == 0 and w1.tobytes() == w[-1].tobytes() and V1.tobytes() == V[-1].tobytes()


@pytest.mark.parametrize("n", (17, 33))
def test_sym_eigh_special_matrices(env, n):
    batch = TR.eigh_cases()["kinds_%d" % n]
    ref = TR.eigh_reference("kinds_%d" % n)
    (w, V, st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    assert np.array_equal(st, np.zeros(len(batch)))
    kinds = dict((k, i) for (i, k) in enumerate(TR.EIGH_KINDS))
    for (k, i) in kinds.items():
        check_eigh(batch[i], w[i], V[i], ref[i], "%s at %d" % (k, n))
        # V f(L) V^T with f = identity gives A back: A - V L V^T = (A V - V L) V^T + A (I - V V^T), entry-wise at most
        # n (residual bound) + n ||A||_2 (orthogonality bound)
        norm = float(np.abs(ref[i]).max())
        bound = n * (K_RES * n * TR.EPS * norm) + n * norm * (K_ORTH * n * TR.EPS)
        assert np.abs((V[i] * w[i]).dot(V[i].T) - batch[i]).max() <= bound, k
    # no rotation: the diagonal matrix comes back sorted and exact, its eigenvectors are unit vectors; the identity as it is
    d = np.diagonal(batch[kinds["diagonal"]])
    assert np.array_equal(w[kinds["diagonal"]], np.sort(d))
    assert np.array_equal(V[kinds["diagonal"]], np.eye(n)[:, np.argsort(d, kind="stable")])
    assert np.array_equal(w[kinds["identity"]], np.ones(n)) and np.array_equal(V[kinds["identity"]], np.eye(n))
    # the repeated eigenvalue and the cluster: the invariant subspace, through a function that separates it from the rest
    for k in ("repeated", "cluster"):
        i = kinds[k]
        want = TR.matfun(batch[i], np.exp, "ld")
        got = (V[i] * np.exp(w[i])).dot(V[i].T)
        scale = float(np.exp(ref[i][-1]))
        assert np.abs(got - want).max() <= 2 * n * scale * (K_RES + K_ORTH) * n * TR.EPS, k


def test_sym_eigh_nan_and_only_the_lower_triangle(env):
    batch = TR.eigh_cases()["size_33"][:3].copy()
    (w0, V0, _st) = env.corr.sym_eigh(batch, ctx=env.ctx)
    bad = batch.copy()
    bad[1, 20, 7] = np.nan
    (w, V, st) = env.corr.sym_eigh(bad, ctx=env.ctx)
    assert list(st) == [0, 1, 0] and np.isnan(w[1]).all() and np.isnan(V[1]).all()
    for b in (0, 2):
        assert w[b].tobytes() == w0[b].tobytes() and V[b].tobytes() == V0[b].tobytes()
    upper = batch.copy()
    upper[:, np.triu_indices(33, 1)[0], np.triu_indices(33, 1)[1]] = np.nan
    (w, V, st) = env.corr.sym_eigh(upper, ctx=env.ctx)
    assert list(st) == [0, 0, 0] and w.tobytes() == w0.tobytes() and V.tobytes() == V0.tobytes()


# ------------------------------------------------------------------------------------------------
# 3. the fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TR.FIT_SHAPES, ids=lambda s: "%d_%d_%d" % s)
@pytest.mark.parametrize("kind", ("euclidean", "geometric"))
def test_fit_reference(env, shape, kind):
    (Nreg, T, H) = shape
    name = "fit_%d_%d_%d" % shape
    (tc, _ta, sh) = TR.tangent_cases()[name]
    tol = 1e-10
    sp = env.corr.fit_tangent(tc, sh, kind, ctx=env.ctx, tol=tol)
    ref = TR.tangent_reference(name)[0] if kind == "geometric" else TR.fit(tc, shrinkage=sh, reference=kind)
    assert sp.info["used"].all() and np.array_equal(sp.info["status"], ref["status"]) and np.array_equal(sp.info["n_live"], ref["n_live"])
    assert np.all(np.abs(sp.info["alpha"] - ref["alpha"]) <= ref["tol_alpha"])
    ref_a = ref if kind == "geometric" else TR.fit(tc, shrinkage=sp.info["alpha"], reference=kind)
    dG = np.abs(sp.reference - ref_a["G"].astype(np.float64)).max()
    if kind == "euclidean":
        bound = (T + 4 + H + 2) * TR.EPS
        assert sp.info["n_iter"] == 0
    else:
        # (the oracle's own alpha: an error of alpha of tol_alpha ~ 1e-15 is far inside the stopping rule's term)
        bound = ref["norm_G"] * (2 * tol * np.sqrt(Nreg) + K_T * Nreg * TR.EPS * ref["kappa_G"])
        assert abs(sp.info["n_iter"] - ref["n_iter"]) <= 2 and ref["n_iter"] > 0
        assert sp.info["grad_norm"] <= tol * np.sqrt(Nreg)
    print("%s %s: |dG| %.3g of %.3g, n_iter %d (oracle %d), norm %.3g" % (name, kind, dG, bound, sp.info["n_iter"], ref["n_iter"], sp.info["grad_norm"]))
    assert dG <= bound
    assert np.array_equal(sp.reference, sp.reference.T) and np.array_equal(sp.whitening, sp.whitening.T)
    # W G W = I and G^1/2 G^1/2 = G at the rounding of two products at kappa(G)
    unit = K_T * Nreg * TR.EPS * ref["kappa_G"]
    assert np.abs(sp.whitening.dot(sp.reference).dot(sp.whitening) - np.eye(Nreg)).max() <= 4 * unit
    assert np.abs(sp.reference_sqrt.dot(sp.reference_sqrt) - sp.reference).max() <= 4 * unit * ref["norm_G"]
    if kind == "geometric":
        # the mean tangent vector of the controls, through apply: the same kernels on the same matrices
        (out, info) = sp.apply(tc, ctx=env.ctx, return_info=True)
        nrm = np.sqrt(2 * (out.mean(axis=1) ** 2).sum() + (info["diag"].mean(axis=1) ** 2).sum())
        assert nrm <= tol * np.sqrt(Nreg) * (1 + 1e-3)


def test_fit_leaves_out_and_refuses(env):
    (tc, _ta, sh) = TR.tangent_cases()["fit_17_40_12"]
    tc = tc.copy()
    tc[4, 9, :] = 2.5                                    # a dead region in control 4
    sp = env.corr.fit_tangent(tc, sh, ctx=env.ctx)
    ref = TR.fit(tc, shrinkage=sh)
    assert list(np.flatnonzero(~sp.info["used"])) == [4] and sp.info["status"][4] == TR.DEAD_REGION and sp.info["n_live"][4] == 16
    assert np.array_equal(sp.info["used"], ref["used"]) and np.array_equal(sp.info["status"], ref["status"])
    assert np.abs(sp.reference - ref["G"].astype(np.float64)).max() <= ref["norm_G"] * (2e-10 * np.sqrt(17) + K_T * 17 * TR.EPS * ref["kappa_G"])
    # chunks of controls change no bit
    sp7 = env.corr.fit_tangent(tc, sh, ctx=env.ctx, _max_chunk=5)
    assert sp7.reference.tobytes() == sp.reference.tobytes() and sp7.whitening.tobytes() == sp.whitening.tobytes()
    assert sp7.info["n_iter"] == sp.info["n_iter"] and sp7.info["grad_norm"] == sp.info["grad_norm"]
    with pytest.raises(ValueError, match="1 usable controls of 2"):
        env.corr.fit_tangent(tc[[4, 5]], sh, ctx=env.ctx)
    with pytest.raises(RuntimeError, match="not converged after 1 iterations"):
        env.corr.fit_tangent(tc, sh, ctx=env.ctx, max_iter=1)
    # alpha = 0 with n - 1 < p: every control is singular
    with pytest.raises(ValueError, match="0 usable controls"):
        env.corr.fit_tangent(tc[:, :, :12], 0.0, ctx=env.ctx)


# ------------------------------------------------------------------------------------------------
# 4. apply, with the oracle's G so that no error of the fit enters
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch65(env):
    """the batch of 65 on the device, Ledoit-Wolf: (space, ts, out, info)"""
    (_tc, ta, sh) = TR.tangent_cases()["apply_17_40_65"]
    G = TR.tangent_reference("apply_17_40_65")[0]["G"].astype(np.float64)
    sp = env.corr.TangentSpace.from_reference(G, sh)
    (out, info) = sp.apply(ta, ctx=env.ctx, return_info=True)
    return (sp, ta, out, info)


def check_apply(out, info, ts, W, n_frames, what, kappa_cap=100.0, k_t=None):
    """kappa_cap, k_t: of a caller with inputs off the "tight" ones and a recorded ratio of its own, whose CPU test pins the
    kappa of its inputs (tests/test_gpu_tangent_edges.py, tests/test_tangent.py)"""
    k_t = K_T if k_t is None else k_t
    ref0 = TR.apply(ts, W, n_frames)
    ref = TR.apply(ts, W, n_frames, shrinkage=info["alpha"])
    assert np.array_equal(info["status"], ref["status"]) and np.array_equal(info["n_live"], ref["n_live"]), what
    ok = ref["status"] == 0
    assert np.nanmax(ref["kappa"]) <= kappa_cap
    r = TR.t_ratio(out, info["diag"], ref)
    print("%s: |dT| / (n eps kappa) %.3g of %.3g; kappa <= %.3g" % (what, r, k_t, np.nanmax(ref["kappa"])))
    assert r <= k_t, what
    assert np.isnan(out[:, ~ok]).all() and np.isnan(info["diag"][:, ~ok]).all()
    return ref0


def test_apply_batch_of_65_against_the_oracle(env, batch65):
    (sp, ta, out, info) = batch65
    ref0 = check_apply(out, info, ta, sp.whitening, None, "S = 65, Ledoit-Wolf")
    assert np.all(np.abs(info["alpha"] - ref0["alpha"]) <= ref0["tol_alpha"])
    assert out.shape == (136, 65) and info["diag"].shape == (17, 65)
    (out2, info2) = sp.apply(ta, ctx=env.ctx, return_info=True)
    assert out2.tobytes() == out.tobytes() and info2["diag"].tobytes() == info["diag"].tobytes()


@pytest.mark.parametrize("S", (1, 31, 32, 33))
def test_apply_smaller_batches_have_the_bits_of_the_large_one(env, batch65, S):
    (sp, ta, out, info) = batch65
    (o, i) = sp.apply(ta[:S], ctx=env.ctx, return_info=True)
    assert o.tobytes() == np.ascontiguousarray(out[:, :S]).tobytes() and i["diag"].tobytes() == np.ascontiguousarray(info["diag"][:, :S]).tobytes()
    assert i["alpha"].tobytes() == info["alpha"][:S].tobytes()


@pytest.mark.parametrize("s", (0, 31, 32, 64))
def test_apply_a_subject_alone_has_its_bits_of_the_batch(env, batch65, s):
    (sp, ta, out, info) = batch65
    (o, i) = sp.apply(ta[s:s + 1], ctx=env.ctx, return_info=True)
    assert o[:, 0].tobytes() == np.ascontiguousarray(out[:, s]).tobytes() and i["diag"][:, 0].tobytes() == np.ascontiguousarray(info["diag"][:, s]).tobytes()


@pytest.mark.parametrize("chunk", (7, 32, 33))
def test_apply_chunks_change_no_bit(env, batch65, chunk):
    (sp, ta, out, info) = batch65
    (o, i) = sp.apply(ta, ctx=env.ctx, return_info=True, _max_chunk=chunk)
    assert o.tobytes() == out.tobytes() and i["diag"].tobytes() == info["diag"].tobytes() and np.array_equal(i["status"], info["status"])


def test_apply_fixed_alpha(env):
    (_tc, ta, sh) = TR.tangent_cases()["apply_17_40_33_fixed"]
    G = TR.tangent_reference("apply_17_40_33_fixed")[0]["G"].astype(np.float64)
    sp = env.corr.TangentSpace.from_reference(G, sh)
    (out, info) = sp.apply(ta, ctx=env.ctx, return_info=True)
    assert np.array_equal(info["alpha"], np.full(33, sh))
    check_apply(out, info, ta, sp.whitening, None, "S = 33, alpha = %g" % sh)


def test_apply_after_cleaning(env, batch65):
    (sp, ta, _out, _info) = batch65
    ts = ta[:9]
    rng = np.random.default_rng(5)
    mask = rng.random((9, 40)) > 0.2
    conf = rng.standard_normal((9, 2, 40))
    (out, info) = sp.apply(ts, confounds=conf, frame_mask=mask, ctx=env.ctx, return_info=True)
    (resid, cinfo) = env.corr.clean(ts, confounds=conf, frame_mask=mask, ctx=env.ctx)
    assert np.array_equal(info["clean"], cinfo) and np.all(cinfo[:, 0] < 40) and np.array_equal(cinfo[:, 0], mask.sum(axis=1))
    check_apply(out, info, resid, sp.whitening, cinfo[:, 0], "9 subjects after cleaning (2 confounds, censored frames)")


def test_apply_statuses_inside_a_full_tile(env, batch65):
    """alpha = 0; subject 5 has a dead region (status 4), subject 20 keeps 10 frames of 40 for 17 regions (status 1); the other
    30 subjects of the tile have the bits of the call without the two"""
    (sp, ta, _out, _info) = batch65
    sp0 = env.corr.TangentSpace.from_reference(sp.reference, 0.0)
    ts = ta[:32].copy()
    mask = np.ones((32, 40), dtype=bool)
    (o_plain, i_plain) = sp0.apply(ts, frame_mask=mask, ctx=env.ctx, return_info=True)
    assert np.array_equal(i_plain["status"], np.zeros(32))
    ts[5, 3, :] = -1.0
    mask[20, 10:] = False
    (o, i) = sp0.apply(ts, frame_mask=mask, ctx=env.ctx, return_info=True)
    want = np.zeros(32, dtype=int)
    (want[5], want[20]) = (TR.DEAD_REGION, TR.SINGULAR)
    assert np.array_equal(i["status"], want) and i["n_live"][5] == 16
    assert np.isnan(o[:, [5, 20]]).all() and np.isnan(i["diag"][:, [5, 20]]).all()
    keep = want == 0
    assert np.ascontiguousarray(o[:, keep]).tobytes() == np.ascontiguousarray(o_plain[:, keep]).tobytes()
    assert np.ascontiguousarray(i["diag"][:, keep]).tobytes() == np.ascontiguousarray(i_plain["diag"][:, keep]).tobytes()
    (resid, cinfo) = env.corr.clean(ts, frame_mask=mask, ctx=env.ctx)
    ref = TR.apply(resid, sp0.whitening, cinfo[:, 0], shrinkage=0.0)
    assert np.array_equal(ref["status"], want)


# ------------------------------------------------------------------------------------------------
# 5. refusals of the three entry points, through the C ABI
# ------------------------------------------------------------------------------------------------
def test_entry_point_refusals(env):
    t = env.torch
    L = env.lib
    ctx = env.ctx
    dev = ctx.device
    p = L.dptr
    (S, N, T) = (3, 5, 20)
    buf = dict(ts=t.randn((S, N, T), dtype=t.float64, device=dev), alpha=t.empty(S, dtype=t.float64, device=dev),
               info=t.empty((S, 2), dtype=t.int32, device=dev), G=t.empty((N, N), dtype=t.float64, device=dev),
               G_half=t.empty((N, N), dtype=t.float64, device=dev), W=t.eye(N, dtype=t.float64, device=dev),
               used=t.empty(S, dtype=t.uint8, device=dev), out=t.empty((10, S), dtype=t.float64, device=dev),
               diag=t.empty((N, S), dtype=t.float64, device=dev))
    (n_iter, grad) = (ctypes.c_int32(0), ctypes.c_double(0.0))
    host = dict(n_iter=ctypes.cast(ctypes.pointer(n_iter), ctypes.c_void_p), grad_norm=ctypes.cast(ctypes.pointer(grad), ctypes.c_void_p))

    def members(**kw):
        m = dict(S=S, Nreg=N, T=T, shrink_mode=1, max_iter=50, tol=1e-10, stream=L.stream_ptr(), **host)
        m.update((k, p(v)) for (k, v) in buf.items())
        m.update(kw)
        return m

    def refused(name, desc, rc, text):
        n_alloc = ctx.stat("n_alloc")
        got = getattr(ctx.lib, name)(ctx.handle, ctypes.byref(desc) if desc is not None else None)
        msg = ctx.lib.fcd_last_message(ctx.handle).decode()
        assert got == rc and text in msg and msg.startswith(name), (name, got, msg)
        assert ctx.stat("n_alloc") == n_alloc

    both = ("fcd_tangent_fit", "fcd_tangent_apply")
    for name in both:
        refused(name, None, L.FCD_ERR_ARG, "null descriptor")
        d = L.TangentDesc.make(**members())
        d.size -= 8
        refused(name, d, L.FCD_ERR_ARG, "descriptor size")
        refused(name, L.TangentDesc.make(**members(flags=2)), L.FCD_ERR_UNSUPPORTED, "unknown flags")
        for k in ("ts", "alpha", "info", "W"):
            refused(name, L.TangentDesc.make(**members(**{k: None})), L.FCD_ERR_ARG, "null pointer")
        refused(name, L.TangentDesc.make(**members(S=0)), L.FCD_ERR_ARG, "need S, Nreg, T >= 1")
        refused(name, L.TangentDesc.make(**members(Nreg=1)), L.FCD_ERR_SHAPE, "need Nreg >= 2, T >= 2")
        refused(name, L.TangentDesc.make(**members(T=1)), L.FCD_ERR_SHAPE, "need Nreg >= 2, T >= 2")
        refused(name, L.TangentDesc.make(**members(Nreg=1025)), L.FCD_ERR_UNSUPPORTED, "1025 regions, at most 1024")
        refused(name, L.TangentDesc.make(**members(S=65536)), L.FCD_ERR_UNSUPPORTED, "shape too large")
        refused(name, L.TangentDesc.make(**members(T=1 << 31)), L.FCD_ERR_UNSUPPORTED, "shape too large")
        refused(name, L.TangentDesc.make(**members(shrink_mode=2)), L.FCD_ERR_UNSUPPORTED, "unknown shrink_mode")
        for a in (-0.1, 1.5, float("nan")):
            refused(name, L.TangentDesc.make(**members(shrink_mode=0, shrink_value=a)), L.FCD_ERR_ARG, "shrink_value outside [0, 1]")
    for k in ("G", "G_half", "used", "n_iter", "grad_norm"):
        refused(both[0], L.TangentDesc.make(**members(**{k: None})), L.FCD_ERR_ARG, "null pointer")
    refused(both[0], L.TangentDesc.make(**members(tol=0.0)), L.FCD_ERR_ARG, "tol must be > 0")
    # 65535 controls of 1024 regions: their R_a alone are 550 GB (refused before anything is reserved or read)
    refused(both[0], L.TangentDesc.make(**members(S=65535, Nreg=1024)), L.FCD_ERR_UNSUPPORTED, "need more than 64 GiB")
    refused(both[0], L.TangentDesc.make(**members(max_iter=0)), L.FCD_ERR_ARG, "max_iter=0")
    for k in ("out", "diag"):
        refused(both[1], L.TangentDesc.make(**members(**{k: None})), L.FCD_ERR_ARG, "null pointer")
    # a non-finite W is on the device, and apply does not synchronise: every subject gets status 5, the Python layer refuses
    buf["W"][1, 2] = float("nan")
    ctx.call("fcd_tangent_apply", ctypes.byref(L.TangentDesc.make(**members())))
    assert buf["info"][:, 1].tolist() == [5, 5, 5] and bool(t.isnan(buf["out"]).all())
    sp = env.corr.TangentSpace(np.eye(N), buf["W"].cpu().numpy(), 0.5, {})
    with pytest.raises(ValueError, match="non-finite"):
        sp.apply(buf["ts"].cpu().numpy(), ctx=ctx)
    # the eigensolver
    A = t.eye(4, dtype=t.float64, device=dev).repeat(2, 1, 1).contiguous()
    eb = dict(A=A, w=t.empty((2, 4), dtype=t.float64, device=dev), V=t.empty((2, 4, 4), dtype=t.float64, device=dev),
              status=t.empty(2, dtype=t.int32, device=dev))

    def em(**kw):
        m = dict(B=2, n=4, stream=L.stream_ptr())
        m.update((k, p(v)) for (k, v) in eb.items())
        m.update(kw)
        return m
    name = "fcd_sym_eigh"
    refused(name, None, L.FCD_ERR_ARG, "null descriptor")
    d = L.EighDesc.make(**em())
    d.size += 8
    refused(name, d, L.FCD_ERR_ARG, "descriptor size")
    refused(name, L.EighDesc.make(**em(flags=1)), L.FCD_ERR_UNSUPPORTED, "unknown flags")
    for k in eb:
        refused(name, L.EighDesc.make(**em(**{k: None})), L.FCD_ERR_ARG, "null pointer")
    refused(name, L.EighDesc.make(**em(B=0)), L.FCD_ERR_ARG, "need B, n >= 1")
    refused(name, L.EighDesc.make(**em(n=0)), L.FCD_ERR_ARG, "need B, n >= 1")
    refused(name, L.EighDesc.make(**em(n=1025)), L.FCD_ERR_UNSUPPORTED, "n=1025, at most 1024")
    refused(name, L.EighDesc.make(**em(B=(1 << 24) + 1)), L.FCD_ERR_UNSUPPORTED, "at most 2^24")
    assert ctx.lib.fcd_tangent_fit(None, None) == L.FCD_ERR_ARG and ctx.lib.fcd_sym_eigh(None, None) == L.FCD_ERR_ARG


# ------------------------------------------------------------------------------------------------
# 6. the two protocols of tests/caller_stream_cases.py
#
# The prototypes carry the stream inside the descriptor, so the registry's parser does not see them; the cases are built here
# with the constructor and driven the way tests/test_gpu_caller_stream.py and tests/test_gpu_context_reuse.py drive theirs.
# The fit waits for its stream (once for the used controls, once per iteration): syncs_stream.  apply and the eigensolver
# never do.
# ------------------------------------------------------------------------------------------------
TG_DIMS = {17: dict(H=6, S=5, n=47, B=2), 33: dict(H=8, S=9, n=130, B=3)}


def _tangent_build(d):
    e = TG_DIMS[d["N"]]
    (N, T) = (d["N"], d["T"])
    inputs = dict(tc=TR.make_series(21, e["H"], N, T), ts=TR.make_series(22, e["S"], N, T))
    outs = dict(G=((N, N), np.float64), G_half=((N, N), np.float64), W=((N, N), np.float64), used=((e["H"],), np.uint8),
                alpha_c=((e["H"],), np.float64), info_c=((e["H"], 2), np.int32), alpha=((e["S"],), np.float64),
                info=((e["S"], 2), np.int32), out=((R.tri(N), e["S"]), np.float64), diag=((N, e["S"]), np.float64))
    return dict(inputs=inputs, outputs=outs, host=dict(N=N, T=T, H=e["H"], S=e["S"]))


def _tangent_call(ctx, i, o, h):
    L = R._lib()
    (n_iter, grad) = (ctypes.c_int32(0), ctypes.c_double(0.0))
    d = L.TangentDesc.make(S=h["H"], Nreg=h["N"], T=h["T"], shrink_mode=1, max_iter=50, tol=1e-10, stream=R.ST(), ts=R.P(i["tc"]),
                           alpha=R.P(o["alpha_c"]), info=R.P(o["info_c"]), G=R.P(o["G"]), G_half=R.P(o["G_half"]), W=R.P(o["W"]),
                           used=R.P(o["used"]), n_iter=ctypes.cast(ctypes.pointer(n_iter), ctypes.c_void_p),
                           grad_norm=ctypes.cast(ctypes.pointer(grad), ctypes.c_void_p))
    ctx.call("fcd_tangent_fit", ctypes.byref(d))
    assert n_iter.value > 0
    d = L.TangentDesc.make(S=h["S"], Nreg=h["N"], T=h["T"], shrink_mode=1, stream=R.ST(), ts=R.P(i["ts"]), alpha=R.P(o["alpha"]),
                           info=R.P(o["info"]), W=R.P(o["W"]), out=R.P(o["out"]), diag=R.P(o["diag"]))
    ctx.call("fcd_tangent_apply", ctypes.byref(d))


def _apply_build(d):
    e = TG_DIMS[d["N"]]
    (N, T) = (d["N"], d["T"])
    G = TR.fit(TR.make_series(21, e["H"], N, T), reference="euclidean", route="f64")
    A = np.stack([TR.eigh_matrix("indefinite", e["n"], b) for b in range(e["B"])])
    inputs = dict(ts=TR.make_series(22, e["S"], N, T), W=np.ascontiguousarray(G["W"]), A=A)
    outs = dict(alpha=((e["S"],), np.float64), info=((e["S"], 2), np.int32), out=((R.tri(N), e["S"]), np.float64),
                diag=((N, e["S"]), np.float64), w=((e["B"], e["n"]), np.float64), V=((e["B"], e["n"], e["n"]), np.float64),
                status=((e["B"],), np.int32))
    return dict(inputs=inputs, outputs=outs, host=dict(N=N, T=T, S=e["S"], n=e["n"], B=e["B"]))


def _apply_call(ctx, i, o, h):
    L = R._lib()
    d = L.TangentDesc.make(S=h["S"], Nreg=h["N"], T=h["T"], shrink_mode=0, shrink_value=0.25, stream=R.ST(), ts=R.P(i["ts"]),
                           alpha=R.P(o["alpha"]), info=R.P(o["info"]), W=R.P(i["W"]), out=R.P(o["out"]), diag=R.P(o["diag"]))
    ctx.call("fcd_tangent_apply", ctypes.byref(d))
    e = L.EighDesc.make(B=h["B"], n=h["n"], stream=R.ST(), A=R.P(i["A"]), w=R.P(o["w"]), V=R.P(o["V"]), status=R.P(o["status"]))
    ctx.call("fcd_sym_eigh", ctypes.byref(e))


TG_CASES = [R.Case("tangent_fit_apply", ["fcd_tangent_fit", "fcd_tangent_apply"], _tangent_build, _tangent_call, syncs_stream=True),
            R.Case("tangent_apply_sym_eigh", ["fcd_tangent_apply", "fcd_sym_eigh"], _apply_build, _apply_call)]


def test_the_cases_are_what_the_registry_asks_of_a_case():
    for case in TG_CASES:
        assert case not in R.CASES and case.name not in R.BY_NAME
        for size in R.SIZES:
            (a, b) = (case.make(size), case.make(size))
            for k in a:
                assert a[k].tobytes() == b[k].tobytes() and a[k].flags["C_CONTIGUOUS"]
        (small, large) = (case.extents("small"), case.extents("large"))
        assert sorted(small) == sorted(large) and all(np.prod(large[k]) >= np.prod(small[k]) for k in small) and small != large


@pytest.fixture(scope="module")
def stream_gpu(env):
    import test_gpu_caller_stream as CSM
    dev = env.torch.device("cuda", 0)
    delay = CSM.Delay(env.torch, dev)
    return dict(torch=env.torch, lib=env.lib, device=dev, delay=delay, streams=CSM.independent_streams(env.torch, delay, 2))


@pytest.mark.parametrize("case", TG_CASES, ids=lambda c: c.name)
def test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case):
    import test_gpu_caller_stream as CSM
    CSM.test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case)


@pytest.mark.parametrize("case", TG_CASES, ids=lambda c: c.name)
def test_on_a_context_that_other_families_have_used(env, case):
    dev = env.torch.device("cuda", 0)
    others = [R.BY_NAME[n] for n in ("corr_partial_lw", "edge_cov_fit_apply", "gibbs_run_run_form")]
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
            desc = env.lib.TangentDesc.make()
            assert getattr(ctx.lib, case.entry_points[0])(ctx.handle, ctypes.byref(desc)) < 0 and ctx.stat("n_alloc") == n_alloc
            check(case, mine, "after a refusal")
        for c in others:
            check(c, "small", "at the end")
        ctx.check_device()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 7. end to end: the README scenario
# ------------------------------------------------------------------------------------------------
def test_scenario_through_the_fit(env):
    """tangent_ref.SCENARIO: tangent() and correlations() on the same series, each into UnsharedRegionFit (vb, symmetric edge
    ids) with the model tangent_ref.scenario_theta gives each input (the defaults for correlations, mu and sigma from the controls'
    values for tangent values); the rates are README's table."""
    s = TR.SCENARIO
    (tc, tp, r) = TR.scenario_series()
    rates = {}
    for kind in ("correlation", "tangent"):
        if kind == "tangent":
            (b, bt, space) = env.corr.tangent(tc, tp, ctx=env.ctx)
            assert space.info["used"].all() and space.info["n_iter"] > 0
        else:
            b = env.corr.correlations(tc, ctx=env.ctx)
            bt = env.corr.correlations(tp, ctx=env.ctx)
        m = env.pkg.UnsharedRegionModel()
        TR.scenario_theta(m, b, kind)
        fit = env.pkg.fit.UnsharedRegionFit()
        fit._ctx = env.ctx
        (fit.model, fit.b, fit.bt) = (m, b, bt)
        (fit.max_iters, fit.rel_tol, fit.edge_index) = (s["iters"], -np.inf, "symmetric")
        fit.run()
        rates[kind] = TR.scenario_rates(fit._lq_R, r)
        print("%s: healthy regions flagged %.4f, anomalous regions found %.4f" % ((kind,) + rates[kind]))
    # the recorded values to within one region of the 228 healthy and of the 28 anomalous (region, patient) pairs; the outcome
    # is a tie in what is found, with no more healthy regions flagged: tangent() does not win on this scenario
    for kind in rates:
        assert abs(rates[kind][0] - s["recorded"][kind][0]) <= 1.01 / 228 and abs(rates[kind][1] - s["recorded"][kind][1]) <= 1.01 / 28, (kind, rates)
    assert s["outcome"] == "tie" and rates["tangent"][1] >= rates["correlation"][1]
