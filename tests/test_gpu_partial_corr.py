"""
fcd_corr_partial behind fcdiff_amd.corr.partial_correlations against the long-double oracle of tests/partial_corr_ref.py.

Data: rows A G with A = 0.3 N(0, 1) + I and G standard normal (partial_corr_ref.make_series).
alpha against the oracle: |d alpha| <= tol_alpha, which the oracle returns with the value (the summation-length bound
8 (p^2 + n p) 2^-53 times the cancellation factor (B / n + F) / (p n delta) of B / n - F).
rho against the oracle EVALUATED AT THE DEVICE'S alpha (one error is not counted twice): |d rho| <= kappa (2e-11 + 64 p 2^-53),
kappa = cond(R_alpha) from the oracle.  With shrinkage the bound is at most 1.6e-9 on every case here; the unshrunk R of this data
grows ill-conditioned with Nreg (kappa up to 1e7 at 65 regions, the bound with it), so alpha = 0 also runs on a benign mix
(partial_corr_ref.make_series, mix = 0.3 / sqrt(Nreg)) where the bound is asserted to be below 1e-9.
The inversion walks the matrix in blocks of NB = 16 columns and has one form; the shapes sit around NB, 2 NB and the
64-region blocks of the correlation kernels.  The batches sit around the 32-subject tiles of pc_dense_kernel and
pc_emit_kernel (S = 31 .. 70, chunks that cut them), the long cleaned scans around the 256-frame blocks of pc_frame_kernel.
"""
import ctypes as C
import functools

import numpy as np
import numpy.testing as nptest
import pytest

import corr_clean_ref as CR
import partial_corr_ref as PR

pytestmark = pytest.mark.gpu

NB = 16


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd import corr
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    (e.torch, e.pkg, e.lib, e.O, e.corr) = (torch, fcdiff_amd, _lib, O, corr)
    e.ctx = _lib.Context()
    return e


def check(env, ts, shrinkage, n_frames=None, got=None, info=None, what="", tight=False):
    """One device call against the oracle, under the two bounds of the module docstring.  -> (out, info) of the device."""
    if got is None:
        (got, info) = env.corr.partial_correlations(ts, shrinkage=shrinkage, ctx=env.ctx, return_info=True)
    lw = isinstance(shrinkage, str)
    ref_a = PR.partial_corr_ld(ts, n_frames, shrinkage)
    assert np.array_equal(info["status"], ref_a["status"]), what
    assert np.array_equal(info["n_live"], ref_a["n_live"]), what
    ok = ref_a["status"] == 0
    assert np.isnan(info["alpha"][ref_a["status"] >= 2]).all()
    if lw:
        d = np.abs(info["alpha"][ok] - ref_a["alpha"][ok])
        print("%s alpha %s: worst |diff| %.3g, tol %.3g" % (what, np.round(ref_a["alpha"][ok], 3), d.max() if d.size else 0,
                                                              ref_a["tol_alpha"][ok].min() if d.size else 0))
        assert (d <= ref_a["tol_alpha"][ok]).all(), what
    else:
        assert (info["alpha"][ref_a["status"] < 2] == float(shrinkage)).all(), what
    ref = PR.partial_corr_ld(ts, n_frames, info["alpha"]) if lw else ref_a        # (a fixed alpha is the device's, bit for bit)
    assert got.shape == ref["out"].shape
    assert np.array_equal(np.isnan(got), np.isnan(ref["out"])), what
    for s in np.flatnonzero(ok):
        bound = PR.rho_bound(ref["cond"][s], ref["n_live"][s])
        assert bound < 1e-9 or not tight
        fin = ~np.isnan(ref["out"][:, s])
        err = np.abs(got[fin, s] - ref["out"][fin, s]).max()
        print("%s subject %d: p %d cond %.3g worst |diff| %.3g, %.3g of the bound" % (what, s, ref["n_live"][s], ref["cond"][s],
                                                                                  err, err / bound))
        assert err <= bound, what
        assert np.abs(got[fin, s]).max() <= 1.0
    return (got, info)


# Nreg around NB, 2 NB and the correlation kernels' 64-region blocks; S in {1, 3, 9}; T odd and even, n >= 4 p and n < p
CASES = [(2, 1, 9), (2, 3, 40), (3, 9, 41), (NB - 1, 3, 61), (NB - 1, 1, 8), (NB, 9, 64), (NB, 3, 9), (NB + 1, 1, 69), (NB + 1, 9, 10),
         (2 * NB + 1, 3, 133), (2 * NB + 1, 1, 20), (64, 1, 256), (64, 3, 33), (65, 9, 261), (65, 1, 40), (130, 3, 521), (130, 1, 66)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-S%d-T%d" % c)
def test_against_the_oracle(env, case):
    (N, S, T) = case
    ts = PR.make_series(1000 + 7 * N + T, S, N, T)
    modes = [0.1, "ledoit_wolf"] + ([0.0] if T >= 4 * N else [])
    for sh in modes:
        (got, _info) = check(env, ts, sh, what="shrinkage %s" % sh)
        assert np.isfinite(got).all()
        z = env.corr.partial_correlations(ts, shrinkage=sh, fisher_z=True, ctx=env.ctx)
        # the same rho bits, then atanh on the device and in NumPy: both good to a few ulp
        nptest.assert_allclose(z, np.arctanh(got), rtol=1e-13, atol=0)
    if T >= 4 * N:
        check(env, PR.make_series(2000 + 7 * N + T, S, N, T, mix=0.3 / np.sqrt(N)), 0.0, what="benign mix, shrinkage 0", tight=True)
    (one, info) = env.corr.partial_correlations(ts, shrinkage=1.0, ctx=env.ctx, return_info=True)
    assert (one == 0.0).all() and (info["alpha"] == 1.0).all() and (info["status"] == 0).all() and (info["n_live"] == N).all()


def test_above_64_kb_of_lds(env):
    """From 512 regions on the inversion kernel's row panel takes more than 64 KB of LDS and the limit is raised for it; 33
    tile rows are also more than its 16 waves.  One subject, n < p, a fixed alpha (the oracle call takes two seconds)."""
    ts = PR.make_series(81, 1, 520, 64)
    (got, info) = check(env, ts, 0.5, what="520 regions", tight=True)
    assert np.isfinite(got).all() and info["n_live"].tolist() == [520]


def test_dead_regions(env):
    (S, N, T) = (5, 20, 90)
    clean = PR.make_series(71, S, N, T)
    ts = clean.copy()
    ts[0, [0, 7, N - 1]] = np.array([1.5, -2.0, 0.0])[:, None]       # first, a middle and the last region constant
    ts[1, 5, 17] = np.nan                                              # one region NaN
    ts[2] = np.arange(N, dtype=np.float64)[:, None]                    # every region constant
    ts[3] = 4.0
    ts[3, [3, 11]] = clean[3, [3, 11]]                                 # exactly two live regions
    ends = env.O.edge_endpoints(N)
    for sh in (0.1, "ledoit_wolf", 0.0):
        (got, info) = check(env, ts, sh, what="dead regions, shrinkage %s" % sh)
        assert info["n_live"].tolist() == [N - 3, N - 1, 0, 2, N] and info["status"].tolist() == [0, 0, 2, 0, 0]
        touched0 = np.isin(ends, [0, 7, N - 1]).any(axis=1)
        assert np.isnan(got[touched0, 0]).all() and np.isfinite(got[~touched0, 0]).all()
        touched1 = (ends == 5).any(axis=1)
        assert np.isnan(got[touched1, 1]).all() and np.isfinite(got[~touched1, 1]).all()
        assert np.isnan(got[:, 2]).all()
        pair = np.flatnonzero((ends == [11, 3]).all(axis=1))
        assert np.isfinite(got[pair, 3]).all() and np.isnan(np.delete(got[:, 3], pair)).all()
        # the neighbour in the batch does not notice: the call without the defects gives it the same bits
        ref = env.corr.partial_correlations(clean, shrinkage=sh, ctx=env.ctx)
        assert np.array_equal(got[:, 4], ref[:, 4]) and np.isfinite(got[:, 4]).all()


def test_singular(env):
    (S, N) = (3, 2 * NB)
    ts = PR.make_series(72, S, N, N // 2)                              # n = p / 2
    (got, info) = check(env, ts, 0.0, what="singular")
    assert info["status"].tolist() == [1] * S and np.isnan(got).all() and (info["alpha"] == 0.0).all()
    (got, info) = check(env, ts, "ledoit_wolf", what="singular data, Ledoit-Wolf")
    assert info["status"].tolist() == [0] * S and np.isfinite(got).all() and (info["alpha"] > 0.0).all()
    # a singular subject among regular ones: duplicate rows, unshrunk
    ts = PR.make_series(73, S, 5, 80)
    ts[1, 3] = 2.0 * ts[1, 1] + 1.0
    (got, info) = check(env, ts, 0.0, what="duplicate rows")
    assert info["status"].tolist() == [0, 1, 0] and np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2]]).all()


def test_with_cleaning(env):
    (ts, cf, mask) = CR.make_input(74, 3, NB + 1, 90, 3, drop=0.25, level=2.0)
    cleaned = CR.clean_ld(ts, cf, mask)
    CR.assert_conditions(cleaned)
    n_kept = cleaned["info"][:, 0]
    assert len(set(n_kept.tolist())) == 3                              # unequal n_kept per subject
    resid = cleaned["resid"].astype(np.float64)
    for sh in ("ledoit_wolf", 0.1):
        (got, info) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
        assert np.array_equal(info["clean"], cleaned["info"])
        check(env, resid, sh, n_frames=n_kept, got=got, info=info, what="cleaned, shrinkage %s" % sh)
    # Masked-out frames appended behind the scan change no bit, whatever they hold.  (Both calls have the same T: the time
    # slices of fcd_corr_edges' subject kernel follow T.)
    rs = np.random.RandomState(75)
    K = 7
    junk = np.array([np.nan, 1e300, -np.inf])[rs.randint(0, 3, size=(3, NB + 1, K))]
    (ts_a, ts_b) = (np.concatenate([ts, rs.standard_normal((3, NB + 1, K))], axis=2), np.concatenate([ts, junk], axis=2))
    (cf_a, cf_b) = (np.concatenate([cf, rs.standard_normal((3, 3, K))], axis=2), np.concatenate([cf, junk[:, :3]], axis=2))
    mask2 = np.concatenate([mask, np.zeros((3, K), dtype=bool)], axis=1)
    a = env.corr.partial_correlations(ts_a, ctx=env.ctx, confounds=cf_a, frame_mask=mask2)
    b = env.corr.partial_correlations(ts_b, ctx=env.ctx, confounds=cf_b, frame_mask=mask2)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    # mask only
    (got, info) = env.corr.partial_correlations(ts, ctx=env.ctx, frame_mask=mask, return_info=True)
    c = CR.clean_ld(ts, None, mask)
    check(env, c["resid"].astype(np.float64), "ledoit_wolf", n_frames=c["info"][:, 0], got=got, info=info, what="mask only")


def test_deterministic_and_independent_of_the_batch(env):
    # T < 96: fcd_corr_edges' subject kernel then takes one time slice whatever S is, and its bits do not depend on S
    (S, N, T) = (9, 2 * NB + 1, 64)
    ts = PR.make_series(76, S, N, T)
    for sh in ("ledoit_wolf", 0.1):
        (a, ia) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, return_info=True)
        (b, ib) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, return_info=True)
        assert np.isfinite(a).all() and np.array_equal(a, b) and np.array_equal(ia["alpha"], ib["alpha"])
        for s in range(S):
            (one, io) = env.corr.partial_correlations(ts[s:s + 1], shrinkage=sh, ctx=env.ctx, return_info=True)
            assert np.array_equal(one[:, 0], a[:, s]) and io["alpha"][0] == ia["alpha"][s]


@pytest.mark.parametrize("shape", [(9, 2 * NB + 1, 64), (9, 20, 700), (3, 209, 40)], ids=lambda v: "S%d-N%d-T%d" % v)
def test_chunking_changes_no_bit(env, shape):
    """One time slice, several time slices (T = 700), and the 64 x 64 block form of the correlations (Nreg > 208)."""
    (S, N, T) = shape
    ts = PR.make_series(77, S, N, T)
    ts[S - 1, 1] = 2.0                                                 # a dead region in the last chunk
    (a, ia) = env.corr.partial_correlations(ts, ctx=env.ctx, return_info=True)
    assert np.isfinite(a[:, :S - 1]).all() and ia["n_live"].tolist() == [N] * (S - 1) + [N - 1]
    for chunk in (1, 2, 4):
        (b, ib) = env.corr.partial_correlations(ts, ctx=env.ctx, return_info=True, _max_chunk=chunk)
        assert np.array_equal(a, b, equal_nan=True), chunk
        for k in ("alpha", "n_live", "status"):
            assert np.array_equal(ia[k], ib[k]), (chunk, k)


# ---------------------------------------------------------------------------------------------------------------------
# Batches past one 32-subject tile of pc_dense_kernel / pc_emit_kernel (blockIdx.y > 0, tile rows beyond the ninth, a full
# tile, one subject in the last tile), chunks that cut the tiles, and scans whose frame blocks behind n_frames are empty.
# Every case is held to tight=True: its oracle bound is below 1e-9.
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = [(31, 5, 40), (32, 5, 41), (33, 17, 69), (65, 5, 40), (70, 17, 69), (40, 33, 300)]


@functools.lru_cache(maxsize=None)
def batch_series(shape):
    (S, N, T) = shape
    return PR.make_series(3000 + S + N, S, N, T)


@pytest.mark.parametrize("shape", BATCHES, ids=lambda v: "S%d-N%d-T%d" % v)
def test_batches_past_one_tile(env, shape):
    ts = batch_series(shape)
    for sh in (0.1, "ledoit_wolf"):
        (got, info) = check(env, ts, sh, what="S %d, shrinkage %s" % (shape[0], sh), tight=True)
        assert np.isfinite(got).all() and (info["status"] == 0).all()
        z = env.corr.partial_correlations(ts, shrinkage=sh, fisher_z=True, ctx=env.ctx)
        nptest.assert_allclose(z, np.arctanh(got), rtol=1e-13, atol=0)


@pytest.mark.parametrize("chunk", [7, 31, 32, 33])
def test_chunks_that_cut_tiles(env, chunk):
    """s_base = 7, 14, ... in front of partial tiles; 31, 62 one short of a tile; 32, 64 on the tile edge; 33, 66 one past it."""
    shape = (70, 17, 69)
    ts = batch_series(shape)
    (a, ia) = env.corr.partial_correlations(ts, ctx=env.ctx, return_info=True)
    assert np.isfinite(a).all()
    (b, ib) = env.corr.partial_correlations(ts, ctx=env.ctx, return_info=True, _max_chunk=chunk)
    assert np.array_equal(a, b, equal_nan=True), chunk
    for k in ("alpha", "n_live", "status"):
        assert np.array_equal(ia[k], ib[k]), (chunk, k)


def test_a_subject_alone_past_one_tile(env):
    # T < 96: one time slice whatever S is, as in test_deterministic_and_independent_of_the_batch
    shape = (65, 5, 40)
    ts = batch_series(shape)
    for sh in ("ledoit_wolf", 0.1):
        (a, ia) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, return_info=True)
        assert np.isfinite(a).all()
        for s in (0, 31, 32, 33, 63, 64):
            (one, io) = env.corr.partial_correlations(ts[s:s + 1], shrinkage=sh, ctx=env.ctx, return_info=True)
            assert np.array_equal(one[:, 0], a[:, s]) and io["alpha"][0] == ia["alpha"][s], s


def test_statuses_inside_a_full_tile(env):
    (S, N, T, Q) = (40, 5, 60, 2)
    (ts, cf, _m) = CR.make_input(900, S, N, T, Q, level=1.0)
    mask = CR.random_mask(np.random.RandomState(901), S, T, 0.2)
    mask[5] = False                                                    # nothing kept
    mask[33] = False
    mask[33, 10:14] = True                                             # dof 1
    ts[34, 1] = 3.0                                                    # a dead region
    ts[39, 2, 7] = np.nan                                              # a kept NaN: a dead region
    mask[39, 7] = True
    cleaned = CR.clean_ld(ts, cf, mask)
    n_kept = cleaned["info"][:, 0]
    assert cleaned["info"][5].tolist() == [0, 0, -1] and cleaned["info"][33].tolist() == [4, Q, 1]
    resid = cleaned["resid"].astype(np.float64)
    regular = np.array([s for s in range(S) if s not in (5, 33, 34, 39)])
    CR.assert_conditions(CR.clean_ld(ts[regular], cf[regular], mask[regular]))
    for sh in ("ledoit_wolf", 0.1):
        (got, info) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
        assert np.array_equal(info["clean"], cleaned["info"])
        check(env, resid, sh, n_frames=n_kept, got=got, info=info, what="statuses in a tile, shrinkage %s" % sh, tight=True)
        assert np.flatnonzero(info["status"]).tolist() == [5, 33] and info["status"][[5, 33]].tolist() == [2, 2]
        assert np.flatnonzero(info["n_live"] != N).tolist() == [5, 33, 34, 39] and info["n_live"][[5, 33, 34, 39]].tolist() == [0, 0, 4, 4]
        assert np.isnan(got[:, [5, 33]]).all()
        # the neighbours do not notice (36 and 40 subjects have the same slice count at T = 60)
        ref = env.corr.partial_correlations(ts[regular], shrinkage=sh, ctx=env.ctx, confounds=cf[regular], frame_mask=mask[regular])
        for s in (4, 6, 32, 35):
            at = int(np.flatnonzero(regular == s)[0])
            assert np.isfinite(got[:, s]).all() and np.array_equal(got[:, s], ref[:, at]), s


@pytest.mark.parametrize("kw", CR.CHUNK_INPUTS, ids=CR.input_id)
def test_long_cleaned_scans(env, kw):
    """n_frames = 200 and 256 at T = 513 and 700: workgroups of pc_frame_kernel whose 256 frames all lie behind n, exact zeros
    among the NBT partial sums of pc_shrink_kernel; n_frames one past and far past a block for the other subjects."""
    (ts, cf, mask, cleaned) = CR.gpu_case(kw)
    n_kept = cleaned["info"][:, 0]
    assert n_kept[:2].tolist() == [200, 256] and kw["T"] > 512
    resid = cleaned["resid"].astype(np.float64)
    for sh in ("ledoit_wolf", 0.1):
        (got, info) = env.corr.partial_correlations(ts, shrinkage=sh, ctx=env.ctx, confounds=cf, frame_mask=mask, return_info=True)
        assert np.array_equal(info["clean"], cleaned["info"])
        check(env, resid, sh, n_frames=n_kept, got=got, info=info, what="long cleaned scan, shrinkage %s" % sh, tight=True)
        assert np.isfinite(got).all()
        if sh == "ledoit_wolf":
            (same, si) = env.corr.correlations(ts, ctx=env.ctx, kind="partial", confounds=cf, frame_mask=mask, return_info=True)
            assert np.array_equal(same, got) and np.array_equal(si["alpha"], info["alpha"])


def test_end_to_end(env):
    torch = env.torch
    ts = PR.make_series(78, 3, 12, 100)
    (a, ia) = env.corr.correlations(ts, ctx=env.ctx, kind="partial", return_info=True)
    (b, ib) = env.corr.partial_correlations(ts, ctx=env.ctx, return_info=True)
    assert np.array_equal(a, b) and np.array_equal(ia["alpha"], ib["alpha"]) and ib["clean"] is None
    assert np.array_equal(env.corr.correlations(ts, ctx=env.ctx, kind="partial", fisher_z=True),
                          env.corr.partial_correlations(ts, fisher_z=True, ctx=env.ctx))
    # device tensors in, device tensors out; the input is not written
    dts = torch.as_tensor(ts, device=env.ctx.device)
    keep = dts.clone()
    (c, ic) = env.corr.partial_correlations(dts, ctx=env.ctx, as_numpy=False, return_info=True)
    assert c.is_cuda and ic["alpha"].is_cuda and torch.equal(dts, keep) and np.array_equal(c.cpu().numpy(), b)
    # the chain x1 -> x2 -> x3: the indirect connection is there in the correlation and gone from the partial correlation
    x = PR.chain()
    full = env.corr.correlations(x, ctx=env.ctx)
    part = env.corr.partial_correlations(x, shrinkage=0.0, ctx=env.ctx)
    assert abs(full[1, 0]) > 0.7 and abs(part[1, 0]) < 0.05 and abs(part[0, 0]) > 0.5 and abs(part[2, 0]) > 0.5
    check(env, x, 0.0, what="chain")


def test_argument_errors_launch_nothing(env):
    torch = env.torch
    (S, N, T) = (2, 5, 30)
    dev = env.ctx.device
    ts = torch.ones((S, N, T), dtype=torch.float64, device=dev)
    out = torch.full((N * (N - 1) // 2, S), -7.0, dtype=torch.float64, device=dev)
    alpha = torch.full((S,), -7.0, dtype=torch.float64, device=dev)
    info = torch.full((S, 2), -7, dtype=torch.int32, device=dev)
    (p, st) = (env.lib.dptr, env.lib.stream_ptr())
    fn = env.ctx.lib.fcd_corr_partial
    h = env.ctx.handle
    ARG, UNS, SHAPE = env.lib.FCD_ERR_ARG, env.lib.FCD_ERR_UNSUPPORTED, env.lib.FCD_ERR_SHAPE
    assert fn(h, p(None), S, N, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st) == ARG
    assert fn(h, p(ts), S, N, T, p(None), 1, 0.0, 0, p(None), p(alpha), p(info), st) == ARG
    assert fn(h, p(ts), S, N, T, p(None), 1, 0.0, 0, p(out), p(None), p(info), st) == ARG
    assert fn(h, p(ts), S, N, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(None), st) == ARG
    assert fn(C.c_void_p(0), p(ts), S, N, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st) == ARG
    for (s_, n_, t_) in ((0, N, T), (S, 0, T), (S, N, 0), (-1, N, T)):
        assert fn(h, p(ts), s_, n_, t_, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st) == ARG
    for v in (-0.01, 1.01, float("nan"), float("inf")):
        assert fn(h, p(ts), S, N, T, p(None), 0, v, 0, p(out), p(alpha), p(info), st) == ARG
    assert fn(h, p(ts), S, 1025, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st) == UNS
    assert b"1024" in env.ctx.lib.fcd_last_message(h)
    assert fn(h, p(ts), S, N, T, p(None), 2, 0.0, 0, p(out), p(alpha), p(info), st) == UNS
    assert fn(h, p(ts), S, N, T, p(None), -1, 0.0, 0, p(out), p(alpha), p(info), st) == UNS
    assert fn(h, p(ts), S, 1, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st) == SHAPE
    with pytest.raises(NotImplementedError):
        env.ctx.call("fcd_corr_partial", p(ts), S, 1025, T, p(None), 1, 0.0, 0, p(out), p(alpha), p(info), st)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((alpha == -7.0).all()) and bool((info == -7).all())
    # n_frames outside [0, T] is found on the device: status 3, the column NaN, the neighbour untouched
    x = torch.as_tensor(PR.make_series(79, S, N, T), device=dev)
    nf = torch.tensor([T, T + 1], dtype=torch.int32, device=dev)
    assert fn(h, p(x), S, N, T, p(nf), 1, 0.0, 0, p(out), p(alpha), p(info), st) == 0
    assert info.cpu().numpy().tolist() == [[N, 0], [N, 3]]
    o = out.cpu().numpy()
    assert np.isfinite(o[:, 0]).all() and np.isnan(o[:, 1]).all()
    assert env.lib.load().fcd_abi_version() == 4
