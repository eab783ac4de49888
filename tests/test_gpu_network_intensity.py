"""
Component intensity of the network-based statistic on the device (fcd_baseline_network_excess, fcd_graph_components_weighted,
baseline.network_test(statistic="intensity"), baseline.graph_components(mask, weights)) against tests/network_intensity_ref.py.

Tolerances.  t is held to RTOL = 1e-10 like every fp64 kernel.  An intensity is sum (|t| - threshold) over a component's
connections, so the same bound carried through the subtraction is |got - ref| <= RTOL (ref + extent threshold) = RTOL sum |t|;
for a null maximum the extent is that of the reference's arg-max component.  Bits, labels, extents, counts and p-values are
compared exactly, which is legitimate only where no |t| lies within 1e-9 of the threshold and no observed intensity within 1e-6
of a null maximum: both are asserted on the reference first (tests/test_network_intensity.py asserts them over the whole list).
graph_components' sums against union-find plus fsum at rtol 1e-12: n 2^-53 for the n <= a few thousand non-negative terms of a
sum.  Everything else -- repeats, chunk lengths, a row alone or in a batch, an inserted observed row -- is compared bit for bit.
"""
import ctypes
import functools
import math

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_glm_ref as GR
import baseline_missing_ref as MR
import baseline_ref as BR
import caller_stream_cases as R
import network_intensity_ref as IR
import network_ref as NR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GAP = 1e-9
GAP_INTENSITY = 1e-6
THRESHOLDS = (1.5, 2.0, 2.5)
CASES = [(shape, thr, "both") for shape in NR.SHAPES for thr in THRESHOLDS] + \
        [(shape, 2.0, tail) for shape in (NR.SHAPES[1], NR.SHAPES[8]) for tail in ("greater", "less")]
EXACT = ("edge_mask", "component", "component_label", "component_edges", "component_regions", "null_max_extent",
         "null_max_regions", "null_n_edges", "p_fwe", "p_fwe_region", "p_fwe_extent")
ADDED = {"component_intensity", "null_max_intensity", "p_fwe_extent", "statistic"}


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


def close(got, ref, extent, thr, what):
    """|got - ref| <= RTOL (ref + extent thr); an infinite sum is infinite on both sides"""
    (got, ref) = (np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64))
    assert got.shape == ref.shape and got.dtype == np.float64, what
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(got), inf) and (got[inf] > 0).all(), what
    err = np.abs(got[~inf] - ref[~inf])
    bound = IR.tolerance(ref[~inf], np.asarray(extent)[~inf], thr, RTOL)
    if err.size:
        print("%s: largest error %.3g of its bound (%d values)" % (what, float((err / np.maximum(bound, 1e-300)).max()), err.size))
    assert (err <= bound).all(), what


def check(out, base, ref, thr, tail, extra=()):
    """an intensity call against the extent call of the same arguments and against the reference"""
    assert NR.threshold_gap(ref["t"][~np.isnan(ref["t"])], ref["null_t"][~np.isnan(ref["null_t"])], thr) > GAP
    assert IR.intensity_gap(ref) >= GAP_INTENSITY
    assert set(out) == set(base) | ADDED and "statistic" not in base
    for k in base:
        if k in ("p_fwe", "p_fwe_region", "threshold", "tail", "design_info"):
            continue
        assert out[k].dtype == base[k].dtype and same(out[k], base[k]), k
    assert same(out["p_fwe_extent"], base["p_fwe"])
    assert (out["threshold"], out["tail"], out["statistic"]) == (thr, tail, "intensity") == (base["threshold"], base["tail"], "intensity")
    nptest.assert_allclose(out["t"], ref["t"], rtol=RTOL, atol=0)
    for k in EXACT + tuple(extra):
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, k
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    close(out["component_intensity"], ref["component_intensity"], ref["component_edges"], thr, "component_intensity")
    close(out["null_max_intensity"], ref["null_max_intensity"], ref["null_arg_extent"], thr, "null_max_intensity")


# ---- 1. against the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,thr,tail", CASES)
def test_against_reference(env, shape, thr, tail):
    (b, bt, labels, ref) = IR.case(shape, thr, tail)
    base = env.bl.network_test(b, bt, thr, labels=labels, tail=tail, ctx=env.ctx)
    out = env.bl.network_test(b, bt, thr, labels=labels, tail=tail, ctx=env.ctx, statistic="intensity")
    check(out, base, ref, thr, tail)
    assert same(env.bl.network_test(b, bt, thr, labels=labels, tail=tail, ctx=env.ctx, statistic="extent")["p_fwe"], base["p_fwe"])


# ---- 2. the other statistics -----------------------------------------------------------------------------------------------

MISSING_SHAPE = BR.SHAPES[4]                                   # (18, 9, 8, 64): P exactly four 16-tiles, a fifth of the values NaN
GLM_SHAPE = GR.SHAPES[2]                                       # (18, 20, 13, 4, 48): R = 5


@functools.lru_cache(maxsize=None)
def missing_case(variance):
    import test_gpu_baseline_missing as TM
    (b, bt, labels) = TM.data_of(MISSING_SHAPE)
    (t, tp) = TM.t_of(MISSING_SHAPE, variance)
    return b, bt, labels, IR.from_t(t, tp, 1.5, "both")


@functools.lru_cache(maxsize=None)
def glm_case(thr=2.0):
    data = GR.make_data(*GLM_SHAPE)
    (t, tp) = GR.all_t(*data)
    return data, IR.from_t(t, tp, thr, "both")


@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_missing_data_and_welch(env, variance):
    (b, bt, labels, ref) = missing_case(variance)
    assert np.isnan(b).any() and np.isnan(bt).any()
    kw = dict(labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    base = env.bl.network_test(b, bt, 1.5, **kw)
    out = env.bl.network_test(b, bt, 1.5, statistic="intensity", **kw)
    check(out, base, ref, 1.5, "both")
    assert "n_controls" in out and len(ref["component_label"]) >= 1 and (ref["null_max_intensity"] > 0).any()


def test_nuisance_covariates(env):
    ((b, bt, z_b, z_bt, perms), ref) = glm_case()
    kw = dict(z_b=z_b, z_bt=z_bt, permutations=perms, ctx=env.ctx)
    base = env.bl.network_test(b, bt, 2.0, **kw)
    out = env.bl.network_test(b, bt, 2.0, statistic="intensity", **kw)
    check(out, base, ref, 2.0, "both")
    assert sorted(out["design_info"]) == sorted(base["design_info"]) and out["design_info"]["rank"] == GLM_SHAPE[3]
    assert all(same(out["design_info"][k], base["design_info"][k]) for k in base["design_info"])
    assert len(ref["component_label"]) >= 1 and (ref["null_max_intensity"] > 0).any()
    # every column dropped: the default call, with the statistic passed on
    flat = np.zeros_like(z_b[:, :1]), np.zeros_like(z_bt[:, :1])
    rank0 = env.bl.network_test(b, bt, 2.0, z_b=flat[0], z_bt=flat[1], permutations=perms, ctx=env.ctx, statistic="intensity")
    plain = env.bl.network_test(b, bt, 2.0, labels=(perms >= b.shape[1]).astype(np.uint8), ctx=env.ctx, statistic="intensity")
    assert rank0["design_info"]["rank"] == 0 and set(rank0) == set(plain) | {"permutations", "design_info"}
    assert all(same(rank0[k], plain[k]) for k in plain if k not in ("threshold", "tail", "statistic")) and rank0["statistic"] == "intensity"


# ---- 3. a row equal to the observed labelling --------------------------------------------------------------------------------

def counts(r):
    return np.rint(r["p_fwe"] * (1.0 + r["null_max_intensity"].shape[0]) - 1.0).astype(np.int64)


def check_inserted(base, more, where):
    top = more["component_intensity"].max()
    assert more["null_max_intensity"][where] == top and more["null_max_extent"][where] == more["component_edges"][0]
    rises = (base["component_intensity"] <= top).astype(np.int64)
    assert rises.all() and np.array_equal(counts(more), counts(base) + rises)
    for k in ("null_max_intensity", "null_max_extent", "null_max_regions", "null_n_edges"):
        assert np.array_equal(np.delete(more[k], where), base[k]), k
    for k in ("t", "edge_mask", "component", "component_label", "component_edges", "component_regions", "component_intensity"):
        assert same(more[k], base[k]), k


def test_observed_row(env):
    (shape, thr) = (NR.SHAPES[1], 2.0)
    (b, bt, labels, ref) = IR.case(shape, thr)
    (H, U) = shape[1:3]
    P = labels.shape[0]
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    base = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx, statistic="intensity")
    assert base["component_edges"].shape[0] >= 2 and len(set(base["component_intensity"].tolist())) >= 2
    for where in (P, 0, 17):                                   # last row, first row, inside a group of 16
        more = env.bl.network_test(b, bt, thr, labels=np.insert(labels, where, observed, axis=0), ctx=env.ctx, statistic="intensity")
        check_inserted(base, more, where)
    # the identity permutation, with covariates
    ((b, bt, z_b, z_bt, perms), _ref) = glm_case()
    kw = dict(z_b=z_b, z_bt=z_bt, ctx=env.ctx, statistic="intensity")
    base = env.bl.network_test(b, bt, 2.0, permutations=perms, **kw)
    ident = np.arange(perms.shape[1], dtype=perms.dtype)
    more = env.bl.network_test(b, bt, 2.0, permutations=np.insert(perms, 17, ident, axis=0), **kw)
    check_inserted(base, more, 17)


# ---- 4. repeatability --------------------------------------------------------------------------------------------------------

def test_chunks_repeatability_and_tensors(env, monkeypatch):
    (shape, thr) = (NR.SHAPES[4], 1.5)                         # P = 64
    (b, bt, labels, _ref) = IR.case(shape, thr)
    kw = dict(labels=labels, statistic="intensity")
    one = env.bl.network_test(b, bt, thr, ctx=env.ctx, **kw)
    two = env.bl.network_test(b, bt, thr, ctx=env.ctx, **kw)
    other = env.bl.network_test(b, bt, thr, **kw)              # a context of its own
    given = env.bl.network_test(env.torch.as_tensor(b, device="cuda"), bt, thr, labels=env.torch.as_tensor(labels, device="cuda"),
                                ctx=env.ctx, as_numpy=False, statistic="intensity")
    arrays = [k for k in one if k not in ("threshold", "tail", "statistic")]
    assert (one["null_max_intensity"] > 0).sum() >= 32
    for k in arrays:
        assert same(one[k], two[k]) and same(one[k], other[k]), k
        assert isinstance(given[k], env.torch.Tensor) and given[k].is_cuda and same(given[k].cpu().numpy(), one[k]), k
    assert set(given) == set(one) and (given["threshold"], given["tail"], given["statistic"]) == (thr, "both", "intensity")
    for (p_chunk, x_chunk) in ((16, 16), (7, 7), (1, 1), (16, 7), (7, 64)):
        monkeypatch.setattr(env.bl, "_P_CHUNK", p_chunk)
        monkeypatch.setattr(env.bl, "_excess_chunk", lambda W, n=x_chunk: n)
        parts = env.bl.network_test(b, bt, thr, ctx=env.ctx, **kw)
        assert set(parts) == set(one) and all(same(parts[k], one[k]) for k in arrays), (p_chunk, x_chunk)
    monkeypatch.undo()


# ---- 5. complete separation --------------------------------------------------------------------------------------------------

def test_complete_separation(env):
    (N, H, U, P, seed) = (7, 6, 3, 40, 21)
    (b, bt, labels) = BR.make_data(N, H, U, P, seed)
    (b[0], bt[0]) = (2.0, 5.0)                                 # connection 0 = (1, 0): mean 3, Q = 18 = g in exact integers, t = +inf
    (b[3], bt[3]) = (0.3, 0.3)                                 # connection 3 = (3, 0): constant, dead under every labelling
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    labels[5] = observed                                       # one labelling that is separated too
    assert sum(1 for p in range(P) if (labels[p] == observed).all() or (labels[p] != observed).all()) == 1
    (t, tp) = NR.group_t(b, bt, labels)
    ref = IR.from_t(t, tp, 2.0, "both")
    assert t[0] == math.inf and math.isnan(t[3]) and np.isinf(tp[:, 0]).sum() == 1
    base = env.bl.network_test(b, bt, 2.0, labels=labels, ctx=env.ctx)
    out = env.bl.network_test(b, bt, 2.0, labels=labels, ctx=env.ctx, statistic="intensity")
    check(out, base, ref, 2.0, "both")
    k = int(np.flatnonzero(out["component_label"] == out["component"][0])[0])
    assert out["t"][0] == math.inf and out["component_intensity"][k] == math.inf
    n_inf = int(np.isinf(out["null_max_intensity"]).sum())
    assert n_inf == 1 and out["null_max_intensity"][5] == math.inf and out["p_fwe"][k] == (1.0 + n_inf) / (1.0 + P)
    assert math.isnan(out["t"][3]) and not out["edge_mask"][3]
    assert np.isfinite(np.delete(out["component_intensity"], k)).all()


# ---- 6. graph_components(mask, weights) --------------------------------------------------------------------------------------

def mask_of(N, edges):
    from fcdiff_amd import util
    m = np.zeros(util.N_to_C(N), dtype=bool)
    for (n, k) in edges:
        m[util.nm_to_c(max(n, k), min(n, k))] = True
    return m


def path(order):
    return [(order[i], order[i + 1]) for i in range(len(order) - 1)]


def random_weights(C, seed):
    """non-negative over nine decades, NaN and negative values sprinkled where nobody may look"""
    rng = np.random.default_rng(seed)
    return rng.random(C) * 10.0 ** rng.integers(-6, 3, C)


def spoil_unset(mask, w):
    w = w.copy()
    off = np.flatnonzero(~mask)
    w[off[0::2]] = np.nan
    w[off[1::2]] = -1.0
    return w


def check_weighted(env, mask, w, N):
    """a 1-D call against union-find plus fsum; returns the call's result"""
    ref = IR.weighted_components(mask, w, N)
    out = env.bl.graph_components(mask, spoil_unset(mask, w), ctx=env.ctx)
    assert set(out) == {"component", "n_edges", "max_extent", "max_regions", "component_label", "component_edges",
                        "component_regions", "max_weight", "component_weight"}
    for k in ("component", "component_label", "component_edges", "component_regions"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in ("n_edges", "max_extent", "max_regions"):
        assert int(out[k]) == ref[k], k
    assert out["component_weight"].dtype == np.float64 and out["component_weight"].shape == ref["component_weight"].shape
    nptest.assert_allclose(out["component_weight"], ref["component_weight"], rtol=1e-12, atol=0)
    nptest.assert_allclose(float(out["max_weight"]), ref["max_weight"], rtol=1e-12, atol=0)
    assert float(out["max_weight"]) == (out["component_weight"].max() if out["component_weight"].size else 0.0)
    plain = env.bl.graph_components(mask, ctx=env.ctx)         # without weights: the pinned keys, the same graph
    assert set(plain) == set(out) - {"max_weight", "component_weight"} and all(same(plain[k], out[k]) for k in plain)
    return out


def test_graph_components_weights_small(env):
    off = check_weighted(env, mask_of(2, []), np.array([3.0]), 2)
    assert float(off["max_weight"]) == 0.0 and off["component_weight"].shape == (0,)
    on = check_weighted(env, mask_of(2, [(1, 0)]), np.array([3.0]), 2)
    assert float(on["max_weight"]) == 3.0 and on["component_weight"].tolist() == [3.0]
    mask = np.random.default_rng(1).random(528) < 0.03          # N = 33: 16.5 words, several components
    w = random_weights(528, 2)
    out = check_weighted(env, mask, w, 33)
    assert out["component_label"].shape[0] >= 3 and (out["component"] == -1).any()
    dev = env.bl.graph_components(env.torch.as_tensor(mask, device="cuda"), env.torch.as_tensor(w, device="cuda"), ctx=env.ctx,
                                  as_numpy=False)
    for k in out:
        assert isinstance(dev[k], env.torch.Tensor) and dev[k].is_cuda and same(dev[k].cpu().numpy(), out[k]), k
    full = check_weighted(env, np.ones(528, dtype=bool), w, 33)   # every row full: the first and last word of every row
    assert full["component_edges"].tolist() == [528]
    with pytest.raises(ValueError, match=">= 0 and not NaN"):
        env.bl.graph_components(env.torch.as_tensor(mask, device="cuda"), env.torch.as_tensor(spoil_unset(~mask, w), device="cuda"),
                                ctx=env.ctx)


def test_graph_components_weights_at_the_lds_limit(env):
    (N, C) = (1024, 1024 * 1023 // 2)
    rng = np.random.default_rng(7)
    order = [int(v) for v in rng.permutation(N)]
    sparse = np.zeros(C, dtype=bool)
    sparse[rng.choice(C, 300, replace=False)] = True
    # about 2000 edges inside 64 blocks of 16 regions: many components (edges drawn over all regions would join nearly all)
    (blk, a_, b_) = (rng.integers(0, 64, 3000), rng.integers(0, 16, 3000), rng.integers(0, 16, 3000))
    many = mask_of(N, [(16 * k + i, 16 * k + j) for (k, i, j) in zip(blk.tolist(), a_.tolist(), b_.tolist()) if i != j])
    assert 1500 <= many.sum() <= 3000
    masks = np.stack([np.zeros(C, dtype=bool), mask_of(N, path(order)) | sparse, many])
    w = np.stack([random_weights(C, 10 + i) for i in range(3)])
    w[2, np.flatnonzero(many)[777]] = math.inf
    spoiled = np.stack([spoil_unset(masks[i], w[i]) for i in range(3)])
    batch = env.bl.graph_components(masks, spoiled, ctx=env.ctx)
    assert set(batch) == {"component", "n_edges", "max_extent", "max_regions", "max_weight"} and batch["max_weight"].shape == (3,)
    for i in range(3):
        alone = check_weighted(env, masks[i], w[i], N)
        assert np.array_equal(batch["component"][i], alone["component"])
        assert batch["max_weight"][i] == float(alone["max_weight"])          # bit for bit: a row alone and in the batch
        assert (batch["n_edges"][i], batch["max_extent"][i], batch["max_regions"][i]) == \
            (alone["n_edges"], alone["max_extent"], alone["max_regions"])
        if i == 1:
            assert alone["component_edges"][0] >= 1023 and alone["component_regions"][0] == 1024
        if i == 2:
            assert alone["component_label"].shape[0] >= 20 and float(alone["max_weight"]) == math.inf
            assert np.isinf(alone["component_weight"]).sum() == 1
    assert batch["max_weight"][0] == 0.0 and batch["n_edges"].tolist()[0] == 0
    # the rows in another order and another batch size: the same bits
    turned = env.bl.graph_components(masks[::-1].copy(), spoiled[::-1].copy(), ctx=env.ctx)
    assert np.array_equal(turned["max_weight"][::-1], batch["max_weight"])
    assert np.array_equal(env.bl.graph_components(masks[1:], spoiled[1:], ctx=env.ctx)["max_weight"], batch["max_weight"][1:])


# ---- 7. through the C ABI ----------------------------------------------------------------------------------------------------

def excess_desc(env, **kw):
    m = dict(stream=env.lib.stream_ptr())
    m.update((k, env.lib.dptr(v) if hasattr(v, "data_ptr") or v is None else v) for (k, v) in kw.items())
    return env.lib.NetworkExcessDesc.make(**m)


def components_desc(env, **kw):
    m = dict(stream=env.lib.stream_ptr())
    m.update((k, env.lib.dptr(v) if hasattr(v, "data_ptr") or v is None else v) for (k, v) in kw.items())
    return env.lib.ComponentsDesc.make(**m)


def test_only_set_entries_are_written_and_read(env):
    """C = 780 over 25 words: 20 entries of a row of excess values, and 20 bits of its last word, lie behind C."""
    t = env.torch
    shape = NR.SHAPES[8]
    (b, bt, labels, ref) = IR.case(shape, 2.0)
    (N, C, P, W) = (shape[0], b.shape[0], labels.shape[0], 25)
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device="cuda")
    (bd, btd, labd) = (dev(b), dev(bt), dev(labels))
    want_bits = t.empty((P, W), dtype=t.int32, device="cuda")
    env.ctx.call("fcd_baseline_network_bits", env.lib.dptr(bd), env.lib.dptr(btd), C, shape[1], shape[2], env.lib.dptr(labd), P, 2.0, 0,
                 env.lib.dptr(want_bits), env.lib.dptr(None), env.lib.stream_ptr())
    got = {}
    for fill in (math.nan, 0.0):
        bits = t.full((P, W), -1, dtype=t.int32, device="cuda")
        excess = t.full((P, 32 * W), fill, dtype=t.float64, device="cuda")
        tt = t.empty((C,), dtype=t.float64, device="cuda")
        env.ctx.call("fcd_baseline_network_excess", ctypes.byref(excess_desc(
            env, C=C, H=shape[1], U=shape[2], P=P, threshold=2.0, tail=0, b=bd, bt=btd, labels=labd, bits=bits, excess=excess, t=tt)))
        assert t.equal(bits, want_bits)
        on = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little").astype(bool)
        e = excess.cpu().numpy()
        assert not on[:, C:].any() and np.array_equal(on[:, :C], NR.suprathreshold(ref["null_t"], 2.0, "both"))
        assert same(e[~on], np.full(int((~on).sum()), fill))                # nothing stored where no bit is set
        want = np.abs(ref["null_t"])[on[:, :C]] - 2.0
        assert (np.abs(e[on] - want) <= RTOL * (want + 2.0)).all()
        outs = dict(component=t.empty((P, N), dtype=t.int32, device="cuda"), intensity=t.empty((P, N), dtype=t.float64, device="cuda"),
                    max_intensity=t.empty((P,), dtype=t.float64, device="cuda"))
        outs.update((k, t.empty((P,), dtype=t.int32, device="cuda")) for k in ("n_edges", "max_extent", "max_regions"))
        env.ctx.call("fcd_graph_components_weighted", ctypes.byref(components_desc(env, B=P, C=C, bits=bits, weights=excess, **outs)))
        got[fill] = dict((k, v.cpu().numpy()) for (k, v) in outs.items())
        dirty = bits.clone()
        dirty[:, W - 1] |= -(1 << (C & 31))                                 # the bits behind C in the last word
        again = dict((k, t.empty_like(v)) for (k, v) in outs.items())
        env.ctx.call("fcd_graph_components_weighted", ctypes.byref(components_desc(env, B=P, C=C, bits=dirty, weights=excess, **again)))
        assert all(same(again[k].cpu().numpy(), got[fill][k]) for k in outs), "bits behind C"
        # intensity and component are optional
        (lone, lone_e) = (t.empty((P,), dtype=t.float64, device="cuda"), t.empty((P,), dtype=t.int32, device="cuda"))
        env.ctx.call("fcd_graph_components_weighted", ctypes.byref(components_desc(
            env, B=P, C=C, bits=bits, weights=excess, n_edges=lone_e, max_extent=again["max_extent"], max_regions=again["max_regions"],
            max_intensity=lone)))
        assert same(lone.cpu().numpy(), got[fill]["max_intensity"]) and same(lone_e.cpu().numpy(), got[fill]["n_edges"])
    (nan, zero) = (got[math.nan], got[0.0])
    assert all(same(nan[k], zero[k]) for k in nan) and np.isfinite(nan["max_intensity"]).all() and np.isfinite(nan["intensity"]).all()
    close(nan["max_intensity"], ref["null_max_intensity"], ref["null_arg_extent"], 2.0, "max_intensity")
    assert np.array_equal(nan["max_extent"], ref["null_max_extent"]) and np.array_equal(nan["n_edges"], ref["null_n_edges"])
    # intensity holds each component's sum at its label and 0.0 elsewhere
    roots = nan["component"] == np.arange(N)[None, :]
    assert (nan["intensity"][~roots] == 0.0).all() and (nan["intensity"][roots] > 0.0).all()
    assert np.array_equal(nan["intensity"].max(axis=1), nan["max_intensity"])


def test_c_abi_refusals(env):
    t = env.torch
    L = env.lib
    d = t.zeros(4096, dtype=t.float64, device="cuda")
    i = t.zeros(4096, dtype=t.int32, device="cuda")
    C1025 = 1025 * 1024 // 2

    def refused(name, desc, rc, text):
        n_alloc = env.ctx.stat("n_alloc")
        got = getattr(env.ctx.lib, name)(env.ctx.handle, ctypes.byref(desc) if desc is not None else None)
        msg = env.ctx.lib.fcd_last_message(env.ctx.handle).decode()
        assert got == rc and text in msg and msg.startswith(name), (name, got, msg)
        assert env.ctx.stat("n_alloc") == n_alloc

    def ex(**kw):
        m = dict(C=3, H=4, U=4, P=1, threshold=2.0, tail=0, b=d, bt=d, labels=i, bits=i, excess=d, t=d)
        m.update(kw)
        return excess_desc(env, **m)

    name = "fcd_baseline_network_excess"
    refused(name, None, L.FCD_ERR_ARG, "null descriptor")
    for delta in (-8, 8):
        x = ex()
        x.size += delta
        refused(name, x, L.FCD_ERR_ARG, "descriptor size")
    for k in ("b", "bt", "bits", "excess"):
        refused(name, ex(**{k: None}), L.FCD_ERR_ARG, "null pointer")
    refused(name, ex(flags=4), L.FCD_ERR_UNSUPPORTED, "unknown flags")
    refused(name, ex(flags=1, design=d, R=2, perms=i), L.FCD_ERR_UNSUPPORTED, "with a design")
    refused(name, ex(P=0), L.FCD_ERR_ARG, "must be >= 1")
    refused(name, ex(labels=None, P=2), L.FCD_ERR_ARG, "P = 1")
    refused(name, ex(design=d, R=2, perms=None, P=2), L.FCD_ERR_ARG, "the identity")
    refused(name, ex(C=5), L.FCD_ERR_SHAPE, "triangular")
    refused(name, ex(H=1, U=1), L.FCD_ERR_ARG, "needs 3")
    refused(name, ex(flags=2, H=1, U=7), L.FCD_ERR_ARG, "welch")
    for bad in (0.0, -1.0, math.inf, math.nan):
        refused(name, ex(threshold=bad), L.FCD_ERR_ARG, "threshold")
    for bad in (-1, 3):
        refused(name, ex(tail=bad), L.FCD_ERR_ARG, "tail")
    refused(name, ex(H=1000, U=25), L.FCD_ERR_UNSUPPORTED, "at most 1024")
    refused(name, ex(C=C1025), L.FCD_ERR_UNSUPPORTED, "regions, at most 1024")
    for R_ in (0, 10):
        refused(name, ex(design=d, R=R_, perms=i), L.FCD_ERR_UNSUPPORTED, "design columns")
    refused(name, ex(design=d, R=7, perms=i), L.FCD_ERR_ARG, "need R + 2")

    def cc(**kw):
        m = dict(B=1, C=3, bits=i, weights=d, component=i, n_edges=i, max_extent=i, max_regions=i, intensity=d, max_intensity=d)
        m.update(kw)
        return components_desc(env, **m)

    name = "fcd_graph_components_weighted"
    refused(name, None, L.FCD_ERR_ARG, "null descriptor")
    for delta in (-8, 8):
        x = cc()
        x.size += delta
        refused(name, x, L.FCD_ERR_ARG, "descriptor size")
    refused(name, cc(flags=1), L.FCD_ERR_UNSUPPORTED, "unknown flags")
    for k in ("bits", "weights", "n_edges", "max_extent", "max_regions", "max_intensity"):
        refused(name, cc(**{k: None}), L.FCD_ERR_ARG, "null pointer")
    refused(name, cc(B=0), L.FCD_ERR_ARG, "must be >= 1")
    refused(name, cc(C=0), L.FCD_ERR_ARG, "must be >= 1")
    refused(name, cc(C=5), L.FCD_ERR_SHAPE, "triangular")
    refused(name, cc(C=C1025), L.FCD_ERR_UNSUPPORTED, "regions, at most 1024")
    assert env.ctx.lib.fcd_baseline_network_excess(None, None) == L.FCD_ERR_ARG
    assert env.ctx.lib.fcd_graph_components_weighted(None, None) == L.FCD_ERR_ARG
    # the context still serves
    out = env.bl.graph_components(np.array([1, 0, 1], dtype=bool), np.array([0.5, 9.0, 0.25]), ctx=env.ctx)
    assert float(out["max_weight"]) == 0.75


# The two protocols of tests/caller_stream_cases.py.  The prototypes carry the stream inside the descriptor, so the registry's
# parser does not see them; the cases are built here with its constructor and driven the way tests/test_gpu_caller_stream.py and
# tests/test_gpu_context_reuse.py drive theirs.  Neither entry point synchronises.

def _weighted_outs(d, P):
    (N, W) = (d["N"], (R.tri(d["N"]) + 31) // 32)
    outs = {"bits": ((P, W), np.uint32), "t": ((R.tri(N),), np.float64), "excess": ((P, 32 * W), np.float64),
            "intensity": ((P, N), np.float64), "max_intensity": ((P,), np.float64)}
    outs.update(R._components_outs(d, P))
    return outs


def _call_weighted(ctx, o, h, P):
    L = R._lib()
    d = L.ComponentsDesc.make(B=P, C=h["C"], stream=R.ST(), bits=R.P(o["bits"]), weights=R.P(o["excess"]), component=R.P(o["component"]),
                              n_edges=R.P(o["n_edges"]), max_extent=R.P(o["max_extent"]), max_regions=R.P(o["max_regions"]),
                              intensity=R.P(o["intensity"]), max_intensity=R.P(o["max_intensity"]))
    ctx.call("fcd_graph_components_weighted", ctypes.byref(d))


def _plain_build(d):
    (b, bt, labels) = R._base_data(d)
    return dict(inputs={"b": b, "bt": bt, "labels": labels}, outputs=_weighted_outs(d, d["P"]), host=R._base_host(d))


def _plain_call(ctx, i, o, h):
    L = R._lib()
    d = L.NetworkExcessDesc.make(C=h["C"], H=h["H"], U=h["U"], P=h["P"], threshold=1.0, tail=0, stream=R.ST(), b=R.P(i["b"]),
                                 bt=R.P(i["bt"]), labels=R.P(i["labels"]), bits=R.P(o["bits"]), excess=R.P(o["excess"]), t=R.P(o["t"]))
    ctx.call("fcd_baseline_network_excess", ctypes.byref(d))
    _call_weighted(ctx, o, h, h["P"])


def _glm_build(d):
    return R._glm_io(d, _weighted_outs(d, d["P"]))


def _glm_call(ctx, i, o, h):
    L = R._lib()
    d = L.NetworkExcessDesc.make(C=h["C"], H=h["H"], U=h["U"], P=h["P"], threshold=1.0, tail=2, R=h["R"], stream=R.ST(), b=R.P(i["b"]),
                                 bt=R.P(i["bt"]), design=R.P(i["design"]), perms=R.P(i["perms"]), bits=R.P(o["bits"]),
                                 excess=R.P(o["excess"]), t=R.P(o["t"]))
    ctx.call("fcd_baseline_network_excess", ctypes.byref(d))
    _call_weighted(ctx, o, h, h["P"])


NI_CASES = [R.Case("network_excess_weighted", ["fcd_baseline_network_excess", "fcd_graph_components_weighted"], _plain_build, _plain_call),
            R.Case("network_excess_glm_weighted", ["fcd_baseline_network_excess", "fcd_graph_components_weighted"], _glm_build, _glm_call)]


def test_the_cases_are_what_the_registry_asks_of_a_case():
    for case in NI_CASES:
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


@pytest.mark.parametrize("case", NI_CASES, ids=lambda c: c.name)
def test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case):
    import test_gpu_caller_stream as CSM
    CSM.test_on_a_side_stream_behind_a_delayed_producer(stream_gpu, case)


@pytest.mark.parametrize("case", NI_CASES, ids=lambda c: c.name)
def test_on_a_context_that_other_families_have_used(env, case):
    dev = env.torch.device("cuda", 0)
    others = [R.BY_NAME[n] for n in ("corr_partial_lw", "baseline_group_glm", "gibbs_run_run_form")]
    ctx = env.lib.Context()

    def run(c, size, where):
        (want, want_stats) = R.fresh(c, size, dev)
        (got, stats) = R.run_once(ctx, c, size, dev, stats=True)
        bad = R.differing(got, want)
        assert not bad, "%s: %s/%s differs from a fresh context in %s" % (where, c.name, size, bad)
        assert stats == want_stats and ctx.stat("dev_err") == 0, (where, c.name, size)
    try:
        for (mine, theirs) in (("small", "large"), ("large", "small")):
            for c in others:
                run(c, theirs, "before %s" % mine)
            run(case, mine, "after the others at %s" % theirs)
            n_alloc = ctx.stat("n_alloc")
            assert case.refuse(ctx) < 0 and ctx.stat("n_alloc") == n_alloc
            run(case, mine, "after a refusal")
        for c in others:
            run(c, "small", "at the end")
        ctx.check_device()
    finally:
        ctx.close()
