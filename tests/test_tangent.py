"""
The oracle of the tangent-space front-end (tests/tangent_ref.py) against closed forms, the record of its fp64-route ratios, the
host-side refusals of fcdiff_amd.corr's tangent API, the new symbols of the C ABI, and README's scenario on the oracle alone.
No test here needs a GPU.
"""
import re

import numpy as np
import pytest
import scipy.linalg

import noise_ref as NR
import tangent_ref as TR
from conftest import theta_dict
from oracle import fcdiff_oracle as O

LD = TR.LD


def spd(seed, n, spread=1.0):
    rng = np.random.default_rng([3, seed, n])
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    A = (Q * np.exp(spread * rng.standard_normal(n))).dot(Q.T)
    return ((A + A.T) / 2).astype(LD)


def test_jacobi_against_lapack_and_its_own_residual():
    for n in (1, 2, 3, 8, 17):
        A = np.asarray(spd(n, n) - 1.0, dtype=np.float64)
        (w, V, _sweeps) = TR.jacobi_eigh(A)
        assert np.abs(w.astype(np.float64) - np.linalg.eigvalsh(A)).max() <= 8 * n * TR.EPS * np.abs(w).max()
        assert np.abs(A.astype(LD).dot(V) - V * w).max() <= 1e-17 * np.abs(w).max() * n
        assert np.abs(V.T.dot(V) - np.eye(n)).max() <= 1e-17 * n
    for r in range(7):
        (p, q) = TR.round_robin(7, r)
        assert len(p) == 3 and len(set(p) | set(q)) == 6
    assert sorted((a, b) for r in range(7) for (a, b) in zip(*TR.round_robin(8, r))) == [(a, b) for a in range(8) for b in range(a + 1, 8)]


def test_geometric_mean_of_two_matrices_is_the_closed_form():
    (A, B) = (spd(1, 6), spd(2, 6))
    (G, _Gh, _W, n_iter, nrm) = TR.reference_of([A, B], tol=1e-15)
    Ah = TR.matfun(A, np.sqrt)
    Aih = TR.matfun(A, TR.isqrt)
    want = TR.congruence(Ah, TR.matfun(TR.congruence(Aih, B, "ld"), np.sqrt), "ld")
    assert n_iter > 0 and nrm <= 1e-15 * np.sqrt(6)
    assert np.abs(G - want).max() <= 1e-14 * np.abs(want).max()


def test_commuting_matrices_give_the_log_euclidean_mean():
    rng = np.random.default_rng(4)
    d = np.exp(rng.standard_normal((5, 7)))
    (G, _Gh, W, n_iter, _nrm) = TR.reference_of([np.diag(x).astype(LD) for x in d], tol=1e-15)
    want = np.exp(np.log(d.astype(LD)).mean(axis=0))
    assert n_iter > 0 and np.abs(G - np.diag(want)).max() <= 1e-15 * want.max()
    assert np.abs(W - np.diag(1 / np.sqrt(want))).max() <= 1e-15 * (1 / np.sqrt(want)).max()


def test_affine_invariance_of_the_reference():
    mats = [spd(s, 5, 0.5) for s in range(4)]
    X = np.random.default_rng(6).standard_normal((5, 5)).astype(LD) + 2 * np.eye(5)
    G = TR.reference_of(mats, tol=1e-15)[0]
    moved = [X.dot(M).dot(X.T) for M in mats]
    GX = TR.reference_of([(M + M.T) / 2 for M in moved], tol=1e-15)[0]
    want = X.dot(G).dot(X.T)
    assert np.abs(GX - want).max() <= 1e-13 * np.abs(want).max()


def test_logm_agrees_with_scipy():
    for s in range(5):
        A = spd(s, 9, 0.7)
        got = TR.matfun(A, np.log).astype(np.float64)
        want = scipy.linalg.logm(A.astype(np.float64)).real
        assert np.abs(got - want).max() <= 1e-12
        assert np.abs(TR.matfun(A.astype(np.float64), np.log, "f64") - want).max() <= 1e-12


def test_mean_tangent_vector_is_zero_and_the_reference_embeds_to_zero():
    (tc, _ta, sh) = TR.tangent_cases()["fit_17_40_12"]
    f = TR.tangent_reference("fit_17_40_12")[0]
    assert 0 < f["n_iter"] < 20 and f["grad_norm"] <= 1e-10 * np.sqrt(17) and f["used"].all()
    a = TR.apply(tc, f["W"], shrinkage=sh)
    nrm = np.sqrt(2 * (a["out"].mean(axis=1) ** 2).sum() + (a["diag"].mean(axis=1) ** 2).sum())
    assert nrm <= 1e-10 * np.sqrt(17) * (1 + 1e-6)
    T = TR.matfun(TR.congruence(f["W"], f["G"], "ld"), np.log)
    assert np.abs(T).max() <= 1e-16 * f["kappa_G"]
    # the statuses of the front half
    ts = tc[:4].copy()
    ts[1, 3, :] = 1.0
    ts[2, :, :] = 0.0
    ts[2, 0, :] = np.arange(40)
    subs = TR.subjects(ts, n_frames=[40, 40, 40, 41])
    assert [r["status"] for r in subs] == [TR.OK, TR.DEAD_REGION, TR.TOO_FEW, TR.BAD_FRAMES] and subs[1]["n_live"] == 16
    with pytest.raises(ValueError, match="1 usable controls of 2"):
        TR.fit(ts[:2])
    with pytest.raises(ValueError, match="0 usable controls"):
        TR.fit(tc[:3, :, :12], shrinkage=0.0, route="f64")
    assert TR.fit(tc, max_iter=1, route="f64")["n_iter"] == -1


def test_recorded_ratios_have_not_grown():
    r = TR.measure_r()
    print(r)
    for (k, v) in r.items():
        assert v <= getattr(TR, k), (k, v)
        assert v >= 0.25 * getattr(TR, k), "%s = %g: the record %g is stale" % (k, v, getattr(TR, k))
    assert TR.MARGIN == 16.0


def test_recorded_edge_ratios_have_not_grown():
    r = TR.measure_r(edge=True)
    print(r)
    for (k, v) in r.items():
        assert v <= getattr(TR, k), (k, v)
        assert v >= 0.25 * getattr(TR, k), "%s = %g: the record %g is stale" % (k, v, getattr(TR, k))
    # the tables of tests/test_gpu_tangent.py are not these
    assert not set(TR.tangent_edge_cases()) & set(TR.tangent_cases()) and sorted(r) == sorted(k + "_EDGE" for k in TR.measure_r(names=[]))


def test_edge_inputs_are_what_their_names_say():
    """the conditioning, the scales and the shapes that tests/test_gpu_tangent_edges.py relies on, on the oracle alone"""
    cases = TR.tangent_edge_cases()
    # the ladder: kappa(M_s) of every subject in the decade of 1 / alpha, status 0 on both routes (measure_r asserts the second)
    for a in TR.LADDER_ALPHAS:
        ref = TR.tangent_edge_reference("ladder_%g" % a)
        assert cases["ladder_%g" % a]["kappa"] == (1 / a, 10 / a) and cases["ladder_%g" % a]["ts"].shape == (4, 17, TR.LADDER_FRAMES)
        assert np.array_equal(ref["status"], np.zeros(4)) and np.all(ref["kappa"] >= 1 / a) and np.all(ref["kappa"] < 10 / a), (a, ref["kappa"])
    # either side of EIG_MIN.  The side that fails is more than 100 times below it.  The side that passes is 51 times above it:
    # kappa = 2e10 is 1 / (50 EIG_MIN), and the fp64 chain moves lambda_min / lambda_max by about n eps kappa = 1e-4 of itself,
    # so neither case sits anywhere near the boundary
    (lo, hi) = (TR.tangent_edge_reference("boundary_%g" % a) for a in TR.BOUNDARY_ALPHAS)
    assert list(lo["status"]) == [0, 0, 0, 0] and list(hi["status"]) == [0, 1, 1, 1]
    assert np.all(lo["ratio"][1:] >= 50 * TR.EIG_MIN) and np.all(hi["ratio"][1:] <= TR.EIG_MIN / 100) and np.all(lo["kappa"][1:] > 1.5e10)
    assert lo["kappa"][0] <= 100 and hi["kappa"][0] <= 100
    assert 17 * TR.EPS * np.nanmax(lo["kappa"]) * 16 * TR.R_T < 1e-3
    # no padding: 32 and 96 regions are whole tiles; 97 is past the LDS form, 32 | 33 the two workgroup sizes
    assert cases["apply_32_40_33"]["ts"].shape == (33, 32, 40) and cases["apply_97_60_3"]["ts"].shape == (3, 97, 60)
    assert TR.EIGH_EDGE_SIZES == (1, 32, 96, 97) and all(TR.eigh_edge_cases()["size_%d" % n].shape == (3, n, n) for n in TR.EIGH_EDGE_SIZES)
    # the graded matrix: 16 decades, and the fp64 Jacobi of the device's rule (2^-58 ||A||_F) converges on it in a few sweeps
    G = TR.graded_matrix()
    w_ld = TR.eigh_edge_reference("graded_%d" % TR.SCALE_N)[0]
    assert 1e15 < float(w_ld[-1] / w_ld[0]) < 1e17 and w_ld[0] > 0
    (w, V, sweeps) = TR.jacobi_eigh(G, np.float64)
    (e_w, e_res, e_orth) = TR.eigh_errors(G, w, V, w_ld)
    print("graded: fp64 Jacobi %d sweeps, eigenvalues %.3g, residual %.3g, orthogonality %.3g" % (sweeps, e_w, e_res, e_orth))
    assert sweeps <= 8 and max(e_w, e_res, e_orth) <= TR.MARGIN * TR.R_EIGH_ORTH
    # a power of two scales every step of the fp64 Jacobi exactly: the threshold too (sqrt of an exact 4^k multiple)
    A = TR.scale_matrix()
    (w0, V0, s0) = TR.jacobi_eigh(A, np.float64)
    for k in TR.SCALE_EXACT:
        (wk, Vk, sk) = TR.jacobi_eigh(np.ldexp(A, k), np.float64)
        assert sk == s0 and wk.tobytes() == np.ldexp(w0, k).tobytes() and Vk.tobytes() == V0.tobytes(), k
    # the extreme scales: the squares leave the normal range at one end and stay finite at the other; one step further they overflow
    with np.errstate(over="ignore", under="ignore"):
        sq = [float((np.ldexp(A, k) ** 2).sum()) for k in TR.SCALE_EXTREME + (TR.SCALE_OVERFLOW,)]
    assert sq[0] < 2.0 ** -1022 and np.isfinite(sq[1]) and sq[1] > 2.0 ** 1000 and np.isinf(sq[2]) and np.isfinite(np.ldexp(A, TR.SCALE_OVERFLOW)).all()
    # the private chunk bound of the eigensolver
    import inspect
    from fcdiff_amd import corr
    assert inspect.signature(corr.sym_eigh).parameters["_max_chunk"].default is None


def test_host_side_refusals_need_no_gpu():
    from fcdiff_amd import corr
    ts = np.zeros((3, 5, 20))
    for (call, exc, text) in (
            (lambda: corr.fit_tangent(ts[0]), ValueError, "shape"),
            (lambda: corr.fit_tangent(ts[:1]), ValueError, "at least 2"),
            (lambda: corr.fit_tangent(ts, shrinkage="oas"), ValueError, "shrinkage"),
            (lambda: corr.fit_tangent(ts, shrinkage=1.5), ValueError, "outside"),
            (lambda: corr.fit_tangent(ts, reference="harmonic"), ValueError, "reference"),
            (lambda: corr.fit_tangent(ts, tol=0.0), ValueError, "tol"),
            (lambda: corr.fit_tangent(ts, max_iter=0), ValueError, "max_iter"),
            (lambda: corr.fit_tangent(ts[:, :1]), ValueError, "Nreg >= 2"),
            (lambda: corr.fit_tangent(ts[:, :, :1]), ValueError, "T >= 2"),
            (lambda: corr.fit_tangent(np.zeros((2, 1025, 2))), NotImplementedError, "1025 regions, at most 1024"),
            (lambda: corr.fit_tangent(ts, frame_mask=np.ones((3, 19))), ValueError, "frame_mask"),
            (lambda: corr.fit_tangent(ts, confounds=np.ones((2, 1, 20))), ValueError, "confounds"),
            (lambda: corr.tangent(ts, ts, reference="x"), ValueError, "reference"),
            (lambda: corr.TangentSpace.from_reference(np.eye(5)[:4]), ValueError, "square"),
            (lambda: corr.TangentSpace.from_reference(np.full((5, 5), np.nan)), ValueError, "non-finite"),
            (lambda: corr.TangentSpace.from_reference(np.triu(np.ones((5, 5)))), ValueError, "symmetric"),
            (lambda: corr.TangentSpace.from_reference(np.ones((5, 5))), ValueError, "positive definite"),
            (lambda: corr.TangentSpace.from_reference(np.eye(5), shrinkage=-1), ValueError, "outside"),
            (lambda: corr.TangentSpace.from_reference(np.eye(1025)), NotImplementedError, "at most 1024"),
            (lambda: corr.TangentSpace.from_reference(np.eye(5)).apply(ts[0]), ValueError, "shape"),
            (lambda: corr.TangentSpace.from_reference(np.eye(4)).apply(ts), ValueError, "5 regions, the reference 4"),
            (lambda: corr.sym_eigh(np.zeros((2, 3, 4))), ValueError, "shape"),
            (lambda: corr.sym_eigh(np.zeros(3)), ValueError, "shape"),
            (lambda: corr.sym_eigh(np.zeros((1, 1025, 1025))), NotImplementedError, "at most 1024")):
        with pytest.raises(exc, match=re.escape(text)):
            call()
    sp = corr.TangentSpace.from_reference(np.diag([4.0, 1.0, 0.25]), 0.2)
    assert np.array_equal(sp.whitening, np.diag([0.5, 1.0, 2.0])) and np.array_equal(sp.reference_sqrt, np.diag([2.0, 1.0, 0.5]))
    assert sp.shrinkage == 0.2 and sp.info == {}
    # correlations() keeps its two kinds and its text
    with pytest.raises(ValueError, match=re.escape("kind must be 'correlation' or 'partial', not 'tangent'")):
        corr.correlations(ts, kind="tangent")


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    import os
    from fcdiff_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcdiff_hip.h")).read()
    lib = _lib.load()
    for name in ("fcd_sym_eigh", "fcd_tangent_fit", "fcd_tangent_apply"):
        assert re.search(r"\bint %s\(fcd_ctx \*ctx, const fcd_\w+_desc \*d\);" % name, header)
        assert _lib.SIGNATURES[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]) and hasattr(lib, name)
    assert "#define FCD_ABI_VERSION 4" in header and _lib.ABI_VERSION == 4 and "#define FCD_TANGENT_EUCLIDEAN 1" in header
    # the descriptors member for member: names and order from the header, 8-byte members after two 4-byte pairs
    for (struct, cls) in (("fcd_eigh_desc", _lib.EighDesc), ("fcd_tangent_desc", _lib.TangentDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.search(r"(\w+)$", m.strip()).group(1) for m in body.split(";") if m.strip()]
        assert names == [f[0] for f in cls._fields_], struct
        assert cls.make().size == ctypes.sizeof(cls)
    assert ctypes.sizeof(_lib.EighDesc) == 64 and ctypes.sizeof(_lib.TangentDesc) == 160
    # refusals that need no device: a null context
    assert lib.fcd_sym_eigh(None, None) == _lib.FCD_ERR_ARG and lib.fcd_tangent_fit(None, None) == _lib.FCD_ERR_ARG
    assert lib.fcd_tangent_apply(None, None) == _lib.FCD_ERR_ARG


def test_scenario_on_the_oracle_alone():
    """README's scenario with the oracle's fp64 route in place of the device and the reference VB loop in place of the fit:
    the rates tangent_ref.SCENARIO records."""
    import fcdiff_amd
    s = TR.SCENARIO
    (tc, tp, r) = TR.scenario_series()
    assert r.shape == (16, 16) and tc.shape == (32, 16, 200) and tp.shape == (16, 16, 200) and 10 < r.sum() < 50
    f = TR.fit(tc, route="f64")
    pairs = dict(tangent=(TR.apply(tc, f["W"], route="f64")["out"], TR.apply(tp, f["W"], route="f64")["out"]))
    tril = np.tril_indices(s["N"], -1)
    assert np.array_equal(np.stack(tril, axis=1), O.edge_endpoints(s["N"]))
    pairs["correlation"] = tuple(np.stack([np.corrcoef(x)[tril] for x in ts], axis=1) for ts in (tc, tp))
    rates = {}
    for (kind, (b, bt)) in pairs.items():
        m = TR.scenario_theta(fcdiff_amd.UnsharedRegionModel(), b, kind)
        with np.errstate(divide="ignore", invalid="ignore"):
            lq_R = NR.vb_fit(b, bt, theta_dict(m.theta()), s["iters"], O.EDGE_SYMMETRIC)["lq_R"]
        rates[kind] = TR.scenario_rates(lq_R, r)
        print(kind, rates[kind])
        assert np.allclose(rates[kind], s["recorded"][kind], atol=5e-4), (kind, rates[kind])
    # a tie in what is found, with fewer healthy regions flagged: tangent() does not win on this scenario
    assert s["outcome"] == "tie" and rates["tangent"][1] == rates["correlation"][1] and rates["tangent"][0] <= rates["correlation"][0]
