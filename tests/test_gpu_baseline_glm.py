"""
The permutation baselines with nuisance covariates on the device (fcd_baseline_group_glm, fcd_baseline_network_bits_glm)
against tests/baseline_glm_ref.py.

Tolerance: rtol 1e-10 on every floating-point output, the bound of the other baseline GPU tests.  Counts, bits, components
and p-values are compared exactly; that is legitimate only where no permuted t^2 (region sum, maximum) lies within relative
GAP = 1e-9 of the observed value it is compared with, and no |t| within GAP of the threshold, which every such test asserts
on the reference arrays first.  The references are made once per shape.
"""
import functools
import math

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_glm_ref as GR
import baseline_ref as BR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GAP = 1e-9
SHAPES = GR.SHAPES
NETWORK_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[6]]
THRESHOLDS = (1.5, 2.0, 2.5)
TAILS = ("both", "greater", "less")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.bl = torch, fcdiff_amd, _lib, baseline
    e.ctx = _lib.Context()
    return e


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def close(got, want, name):
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % name
    assert np.array_equal(np.isinf(got), np.isinf(want)), "%s: infinite positions differ" % name
    nptest.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=name)


@functools.lru_cache(maxsize=None)
def data_of(shape):
    return GR.make_data(*shape)


@functools.lru_cache(maxsize=None)
def t_of(shape):
    return GR.all_t(*data_of(shape))


@functools.lru_cache(maxsize=None)
def group_ref(shape):
    return GR.group_from_t(*t_of(shape), shape[0])


def gaps_network(t, null_t, threshold):
    a = np.abs(np.concatenate([np.asarray(t).reshape(-1), np.asarray(null_t).reshape(-1)]))
    a = a[~np.isnan(a)]
    return float((np.abs(a - threshold) / threshold).min()) if a.size else np.inf


GROUP_KEYS = {"t", "region", "null_max_t", "null_max_region", "count_t", "count_region", "p_t", "p_region", "p_fwe_t",
              "p_fwe_region", "labels", "permutations", "design_info"}
NETWORK_EXTRA = {"labels", "permutations", "design_info"}


def check_group(out, ref, perms, H, rank):
    for k in ("t", "region", "null_max_t", "null_max_region"):
        close(out[k], ref[k], k)
    for k in ("count_t", "count_region"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["permutations"], perms) and out["permutations"].dtype == np.int64
    assert np.array_equal(out["labels"], (perms >= H).astype(np.uint8)) and out["labels"].dtype == np.uint8
    info = out["design_info"]
    assert info["rank"] == rank and info["dof"] == perms.shape[1] - rank - 2 and info["used"].sum() == rank
    assert set(out) == GROUP_KEYS


def check_network(out, ref, perms, H):
    close(out["t"], ref["t"], "t")
    for k in ("edge_mask", "component", "component_label", "component_edges", "component_regions", "null_max_extent",
              "null_max_regions", "null_n_edges", "p_fwe", "p_fwe_region"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert out["threshold"] == ref["threshold"] and out["tail"] == ref["tail"]
    assert np.array_equal(out["permutations"], perms) and np.array_equal(out["labels"], (perms >= H).astype(np.uint8))
    assert set(out) == (set(ref) - {"null_t", "null_components"}) | NETWORK_EXTRA


# ---- against the reference -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_group_test_against_reference(env, shape):
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    ref = group_ref(shape)
    assert GR.gaps_group(ref) > GAP and not np.isnan(ref["t"]).any()
    out = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    check_group(out, ref, perms, shape[1], shape[3])


@pytest.mark.parametrize("shape", NETWORK_SHAPES)
def test_network_test_against_reference(env, shape):
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    (t, null_t) = t_of(shape)
    for thr in THRESHOLDS:
        assert gaps_network(t, null_t, thr) > GAP
        for tail in TAILS:
            ref = GR.network_test(b, bt, z_b, z_bt, perms, thr, tail, t_pair=(t, null_t))
            out = env.bl.network_test(b, bt, thr, z_b=z_b, z_bt=z_bt, permutations=perms, tail=tail, ctx=env.ctx)
            check_network(out, ref, perms, shape[1])


def test_network_reference_covers_empty_and_split_graphs():
    (empty, split, found) = (0, 0, 0)
    for shape in NETWORK_SHAPES:
        (b, bt, z_b, z_bt, perms) = data_of(shape)
        for thr in THRESHOLDS:
            for tail in TAILS:
                ref = GR.network_test(b, bt, z_b, z_bt, perms, thr, tail, t_pair=t_of(shape))
                empty += int((ref["null_n_edges"] == 0).sum()) + int(len(ref["component_label"]) == 0)
                split += int((ref["null_components"] >= 2).sum()) + int(len(ref["component_label"]) >= 2)
                found += int(len(ref["component_label"]) >= 1)
    assert empty >= 1 and split >= 1 and found >= 1


# ---- the identity among the rows -----------------------------------------------------------------------------------------------

def _bits_rows(env, b, bt, W, perms, threshold, tail):
    """(P, C) bool straight from fcd_baseline_network_bits_glm."""
    t = env.torch
    (C, H) = b.shape
    U = bt.shape[1]
    words = (C + 31) // 32
    (bd, btd, Wd) = (t.as_tensor(b, device="cuda"), t.as_tensor(bt, device="cuda"), t.as_tensor(np.ascontiguousarray(W), device="cuda"))
    pd = t.as_tensor(np.ascontiguousarray(perms.astype(np.uint16)).view(np.int16), device="cuda")
    bits = t.zeros((perms.shape[0], words), dtype=t.int32, device="cuda")
    env.ctx.call("fcd_baseline_network_bits_glm", env.lib.dptr(bd), env.lib.dptr(btd), C, H, U, env.lib.dptr(Wd), W.shape[1],
                 env.lib.dptr(pd), perms.shape[0], float(threshold), env.bl.TAILS[tail], env.lib.dptr(bits), env.lib.dptr(None),
                 env.lib.stream_ptr())
    rows = np.unpackbits(bits.cpu().numpy().view(np.uint8).reshape(perms.shape[0], -1), axis=1, bitorder="little")
    return rows[:, :C].astype(bool)


def _rows_reproduce_observed(env, shape, row):
    """`row` at the first place, the last place and place 17 of the permutations: the observed statistics bit for bit."""
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    assert not (perms == row[None, :]).all(axis=1).any()
    kw = dict(z_b=z_b, z_bt=z_bt, ctx=env.ctx)
    base = env.bl.group_test(b, bt, permutations=perms, **kw)
    live = ~np.isnan(base["t"])
    (W, _info) = env.bl.glm_design(z_b, z_bt)
    for where in (0, perms.shape[0], 17):
        rows = np.insert(perms, where, row, axis=0)
        more = env.bl.group_test(b, bt, permutations=rows, **kw)
        assert np.array_equal(more["count_t"], base["count_t"] + live)               # counted by >=
        assert np.array_equal(more["count_region"], base["count_region"] + 1)
        assert more["null_max_t"][where] == np.nanmax(np.abs(more["t"]))
        assert more["null_max_region"][where] == more["region"].max()
        assert same(np.delete(more["null_max_t"], where), base["null_max_t"])
        assert same(np.delete(more["null_max_region"], where), base["null_max_region"])
        assert same(more["t"], base["t"]) and same(more["region"], base["region"])
        for tail in TAILS:
            net = env.bl.network_test(b, bt, 1.5, permutations=rows, tail=tail, **kw)
            got = _bits_rows(env, b, bt, W, rows, 1.5, tail)
            assert np.array_equal(got[where], net["edge_mask"]) and net["null_n_edges"][where] == net["edge_mask"].sum()
            assert net["edge_mask"].any() or tail != "both"
            assert np.array_equal(np.delete(got, where, axis=0), _bits_rows(env, b, bt, W, perms, 1.5, tail))
            assert same(net["t"], more["t"])


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[7]])
def test_identity_row(env, shape):
    _rows_reproduce_observed(env, shape, np.arange(shape[1] + shape[2], dtype=np.int64))


def test_transposition_of_two_controls_with_equal_covariates(env):
    """Controls 1 and 3 have the same covariates: exchanging them exchanges two equal rows of W, so every product is the same."""
    shape = SHAPES[2]
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    z_b = z_b.copy()
    z_b[3] = z_b[1]
    row = np.arange(shape[1] + shape[2], dtype=np.int64)
    row[[1, 3]] = [3, 1]
    (W, _info) = env.bl.glm_design(z_b, z_bt)
    assert same(W[1], W[3]) and not same(b[:, 1], b[:, 3])
    kw = dict(z_b=z_b, z_bt=z_bt, ctx=env.ctx)
    base = env.bl.group_test(b, bt, permutations=perms, **kw)
    for where in (0, perms.shape[0], 17):
        more = env.bl.group_test(b, bt, permutations=np.insert(perms, where, row, axis=0), **kw)
        assert np.array_equal(more["count_t"], base["count_t"] + 1) and np.array_equal(more["count_region"], base["count_region"] + 1)
        assert more["null_max_t"][where] == np.abs(more["t"]).max() and more["null_max_region"][where] == more["region"].max()
        assert same(more["t"], base["t"]) and same(more["region"], base["region"])
        net = env.bl.network_test(b, bt, 1.5, permutations=np.insert(perms, where, row, axis=0), **kw)
        assert net["null_n_edges"][where] == net["edge_mask"].sum() > 0


# ---- degenerate designs and rows -----------------------------------------------------------------------------------------------

def test_all_columns_dropped_is_the_default_call_bit_for_bit(env):
    shape = SHAPES[2]
    (b, bt, _zb, _zt, perms) = data_of(shape)
    (H, U) = shape[1:3]
    (z_b, z_bt) = (np.full((H, 2), 3.0), np.full((U, 2), 3.0))
    labels = (perms >= H).astype(np.uint8)
    base = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    out = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    assert set(out) == set(base) | {"permutations", "design_info"} and out["design_info"]["rank"] == 0
    assert not out["design_info"]["used"].any() and out["design_info"]["dof"] == H + U - 2
    for k in base:
        assert same(out[k], base[k]) and out[k].dtype == base[k].dtype, k
    base = env.bl.network_test(b, bt, 2.0, labels=labels, ctx=env.ctx)
    out = env.bl.network_test(b, bt, 2.0, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    assert set(out) == set(base) | {"permutations", "design_info"}
    for k in base:
        assert same(out[k], base[k]) if isinstance(base[k], np.ndarray) else out[k] == base[k], k


@functools.lru_cache(maxsize=None)
def dead_rows_case():
    """SHAPES[2] with connection 2 constant, connection 4 = the first covariate plus a constant, connection 40 = a combination
    of two covariates plus a constant."""
    (b, bt, z_b, z_bt, perms) = data_of(SHAPES[2])
    (b, bt) = (b.copy(), bt.copy())
    b[2] = 0.25
    bt[2] = 0.25
    b[4] = z_b[:, 0] + 0.3
    bt[4] = z_bt[:, 0] + 0.3
    b[40] = 0.1 * z_b[:, 0] - 0.02 * z_b[:, 2] + 0.3
    bt[40] = 0.1 * z_bt[:, 0] - 0.02 * z_bt[:, 2] + 0.3
    return b, bt, z_b, z_bt, perms


def test_constant_row_and_row_equal_to_a_covariate_are_dead(env):
    (b, bt, z_b, z_bt, perms) = dead_rows_case()
    shape = SHAPES[2]
    (t, null_t) = GR.all_t(b, bt, z_b, z_bt, perms)
    ref = GR.group_from_t(t, null_t, shape[0])
    dead = [2, 4, 40]
    assert np.flatnonzero(np.isnan(ref["t"])).tolist() == dead and GR.gaps_group(ref) > GAP
    out = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    check_group(out, ref, perms, shape[1], shape[3])
    assert (out["count_t"][dead] == 0).all() and np.isnan(out["p_t"][dead]).all() and np.isnan(out["p_fwe_t"][dead]).all()
    # a dead connection takes exactly its term from both its regions: against the data as they were
    (b0, bt0) = data_of(shape)[:2]
    full = env.bl.group_test(b0, bt0, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    assert same(np.delete(out["t"], dead), np.delete(full["t"], dead))
    lost = np.zeros(shape[0])
    for c in dead:
        lost[list(env.pkg.util.c_to_nm(c))] += full["t"][c] ** 2
    nptest.assert_allclose(out["region"], full["region"] - lost, rtol=1e-12)
    for tail in TAILS:
        assert gaps_network(t, null_t, 1.5) > GAP
        net = env.bl.network_test(b, bt, 1.5, z_b=z_b, z_bt=z_bt, permutations=perms, tail=tail, ctx=env.ctx)
        check_network(net, GR.network_test(b, bt, z_b, z_bt, perms, 1.5, tail, t_pair=(t, null_t)), perms, shape[1])
        assert not net["edge_mask"][dead].any()
        (W, _info) = env.bl.glm_design(z_b, z_bt)
        assert not _bits_rows(env, b, bt, W, perms, 1.5, tail)[:, dead].any()


# ---- repeatability, tensors, chunks --------------------------------------------------------------------------------------------

def test_repeatable_second_context_device_tensors_and_chunks(env, monkeypatch):
    shape = SHAPES[2]
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    kw = dict(z_b=z_b, z_bt=z_bt, permutations=perms)
    t = env.torch

    def agree(x, y, k):
        if isinstance(x, np.ndarray):
            assert same(x, y), k
        elif isinstance(x, dict):
            assert set(x) == set(y) and all(same(x[j], y[j]) for j in x), k
        else:
            assert x == y, k

    one = env.bl.group_test(b, bt, ctx=env.ctx, **kw)
    two = env.bl.group_test(b, bt, ctx=env.ctx, **kw)
    other = env.bl.group_test(b, bt, **kw)                      # a context of its own
    dev = env.bl.group_test(t.as_tensor(b, device="cuda"), bt, ctx=env.ctx, as_numpy=False, z_b=t.as_tensor(z_b, device="cuda"),
                            z_bt=z_bt, permutations=t.as_tensor(perms, device="cuda"))
    assert set(dev) == set(one)
    for k in one:
        agree(one[k], two[k], k)
        agree(one[k], other[k], k)
        if k != "design_info":
            assert isinstance(dev[k], t.Tensor) and dev[k].is_cuda and same(dev[k].cpu().numpy(), one[k]), k
    net = env.bl.network_test(b, bt, 1.5, ctx=env.ctx, **kw)
    again = env.bl.network_test(b, bt, 1.5, ctx=env.ctx, **kw)
    other = env.bl.network_test(b, bt, 1.5, **kw)
    devn = env.bl.network_test(b, t.as_tensor(bt, device="cuda"), 1.5, ctx=env.ctx, as_numpy=False, **kw)
    chunked = []
    for size in (16, 7):
        monkeypatch.setattr(env.bl, "_P_CHUNK", size)
        chunked.append(env.bl.network_test(b, bt, 1.5, ctx=env.ctx, **kw))
    assert set(devn) == set(net)
    for k in net:
        for o in [again, other] + chunked:
            agree(net[k], o[k], k)
        if isinstance(net[k], np.ndarray):
            assert isinstance(devn[k], t.Tensor) and devn[k].is_cuda and same(devn[k].cpu().numpy(), net[k]), k
    assert same(net["t"], one["t"])


def test_drawn_permutations_are_the_given_ones(env):
    shape = SHAPES[1]
    (b, bt, z_b, z_bt, _perms) = data_of(shape)
    perms = env.bl.draw_permutations(20, shape[1] + shape[2], seed=5)
    given = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    drawn = env.bl.group_test(b, bt, 20, seed=5, z_b=z_b, z_bt=z_bt, ctx=env.ctx)
    assert all(same(given[k], drawn[k]) for k in given if k != "design_info")


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals(env):
    t = env.torch
    p = env.lib.dptr
    d = t.zeros(16384, dtype=t.float64, device="cuda")
    i = t.zeros(16384, dtype=t.int64, device="cuda")
    s = env.lib.stream_ptr()

    def group(b=d, C=3, H=4, U=4, R=2, P=1, design=d, perms=i, out=d):
        env.ctx.call("fcd_baseline_group_glm", p(b), p(d), C, H, U, p(design), R, p(perms), P, p(out), p(d), p(d), p(d), p(i), p(i), s)

    def bits(b=d, C=3, H=4, U=4, R=2, P=1, design=d, perms=i, out=i, thr=2.0, tail=0):
        env.ctx.call("fcd_baseline_network_bits_glm", p(b), p(d), C, H, U, p(design), R, p(perms), P, thr, tail, p(out), p(None), s)

    for call in (group, bits):
        for R in (0, -1, 10):
            with pytest.raises(NotImplementedError, match="design columns"):
                call(R=R)
        with pytest.raises(NotImplementedError, match="at most 1024"):
            call(H=1000, U=25)
        for kw in ({"b": None}, {"design": None}, {"out": None}):
            with pytest.raises(ValueError, match="null"):
                call(**kw)
        for kw in ({"P": 0}, {"C": 0}, {"H": 0}):
            with pytest.raises(ValueError, match=">= 1"):
                call(**kw)
        with pytest.raises(ValueError, match="R \\+ 2"):
            call(H=2, U=1, R=2)
        with pytest.raises(ValueError, match="R \\+ 2"):
            call(H=5, U=5, R=9)
        with pytest.raises(ValueError, match="triangular"):
            call(C=5)
    with pytest.raises(ValueError, match="null"):
        group(perms=None)
    with pytest.raises(NotImplementedError, match="too large"):
        group(P=65535 * 128 + 1)
    with pytest.raises(NotImplementedError, match="too large"):
        bits(P=65535 * 32 + 1)
    with pytest.raises(ValueError, match="identity"):
        bits(perms=None, P=2)
    with pytest.raises(ValueError, match="threshold"):
        bits(thr=0.0)
    with pytest.raises(ValueError, match="tail"):
        bits(tail=3)
    with pytest.raises(NotImplementedError, match="regions"):
        bits(C=1025 * 1024 // 2)
    # the context is still usable
    shape = SHAPES[0]
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    out = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    close(out["t"], group_ref(shape)["t"], "t")


def test_c_abi_identity_without_permutations(env):
    """perms == NULL with P = 1 is the identity: the observed bits and t."""
    shape = SHAPES[1]
    (b, bt, z_b, z_bt, perms) = data_of(shape)
    (W, _info) = env.bl.glm_design(z_b, z_bt)
    net = env.bl.network_test(b, bt, 1.5, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    ident = np.arange(shape[1] + shape[2], dtype=np.int64)[None, :]
    assert np.array_equal(_bits_rows(env, b, bt, W, ident, 1.5, "both")[0], net["edge_mask"])


# ---- end to end ----------------------------------------------------------------------------------------------------------------

E2E_SEED = 3


@functools.lru_cache(maxsize=None)
def end_to_end_case(seed=E2E_SEED):
    """16 regions, 32 controls, 16 patients, sampled.  One covariate (age, say), 1.5 units higher in the patients; every
    connection of regions 0 .. 3 has a slope on it and no group effect; every connection of regions 8 and 9 has a group effect
    and no slope."""
    (N, H, U, P) = (16, 32, 16, 99)
    rng = np.random.default_rng(seed)
    C = N * (N - 1) // 2
    z = rng.normal(0.0, 1.0, H + U)
    z[H:] += 1.5
    X = rng.normal(0.3, 0.1, (C, H + U))
    for c in range(C):
        (n, m) = (int(v) for v in BR.util.c_to_nm(c))
        if n <= 3 or m <= 3:
            X[c] += 0.06 * z
        elif n in (8, 9) or m in (8, 9):
            X[c, H:] += 0.08
    perms = np.stack([rng.permutation(H + U) for _ in range(P)]).astype(np.int64)
    return X[:, :H].copy(), X[:, H:].copy(), z[:H, None].copy(), z[H:, None].copy(), perms


def test_end_to_end_covariate_confound(env):
    (b, bt, z_b, z_bt, perms) = end_to_end_case()
    (H, U) = (b.shape[1], bt.shape[1])
    none = np.zeros((H + U, 0))
    plain = GR.group_test(b, bt, none[:H], none[H:], perms)          # Q = 0: the two-sample t on the same permutations
    ref = GR.group_test(b, bt, z_b, z_bt, perms)
    assert (plain["p_fwe_region"][:4] <= 0.05).any()                 # the confound passes for a group difference ...
    assert (ref["p_fwe_region"][:4] > 0.05).all()                    # ... and does not with the covariate in the model
    assert (ref["p_fwe_region"][8:10] <= 0.05).all()                 # the planted effect is found with it
    assert GR.gaps_group(ref) > GAP and GR.gaps_group(plain) > GAP
    out = env.bl.group_test(b, bt, z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    check_group(out, ref, perms, H, 1)
    base = env.bl.group_test(b, bt, labels=(perms >= H).astype(np.uint8), ctx=env.ctx)
    for k in ("count_t", "count_region", "p_fwe_region"):
        nptest.assert_array_equal(base[k], plain[k], err_msg=k)
