"""
The network-based statistic on the device (fcd_baseline_network_bits, fcd_graph_components, baseline.network_test,
baseline.graph_components) against tests/network_ref.py.

t is held to rtol 1e-10 like every fp64 kernel; everything else -- bits, labels, extents, counts, p-values -- is compared exactly.
That is legitimate only where no |t|, observed or permuted, lies within relative 1e-9 of the threshold, which every such
test asserts on the reference's arrays first.  The references are made once per (shape, threshold, tail).
"""
import numpy as np
import numpy.testing as nptest
import pytest

import baseline_ref as BR
import network_ref as NR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GAP = 1e-9
THRESHOLDS = (1.5, 2.0, 2.5)
CASES = [(shape, thr, "both") for shape in NR.SHAPES for thr in THRESHOLDS] + \
        [(shape, 2.0, tail) for shape in (NR.SHAPES[1], NR.SHAPES[8]) for tail in ("greater", "less")]
EXACT = ("edge_mask", "component", "component_label", "component_edges", "component_regions", "null_max_extent",
         "null_max_regions", "null_n_edges", "p_fwe", "p_fwe_region")


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


# ---- graph_components ------------------------------------------------------------------------------------------------------

def mask_of(N, edges):
    from fcdiff_amd import util
    m = np.zeros(util.N_to_C(N), dtype=bool)
    for (n, k) in edges:
        m[util.nm_to_c(max(n, k), min(n, k))] = True
    return m


def clique(regions):
    return [(a, b) for a in regions for b in regions if a > b]


def path(order):
    return [(order[i], order[i + 1]) for i in range(len(order) - 1)]


def shuffled(N, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(N)]


def random_mask(N, density, seed):
    return np.random.default_rng(seed).random(N * (N - 1) // 2) < density


GRAPHS = {
    "n2_off": (2, lambda: mask_of(2, [])),
    "n2_on": (2, lambda: mask_of(2, [(1, 0)])),
    "n33_sparse": (33, lambda: random_mask(33, 0.03, 1)),          # C = 528 = 16.5 words: several components
    "n33_empty": (33, lambda: mask_of(33, [])),
    "n33_complete": (33, lambda: np.ones(528, dtype=bool)),
    "star": (20, lambda: mask_of(20, [(7, k) for k in range(20) if k != 7])),
    "two_cliques": (12, lambda: mask_of(12, clique(range(0, 5)) + clique(range(6, 12)))),
    "two_cliques_bridged": (12, lambda: mask_of(12, clique(range(0, 5)) + clique(range(6, 12)) + [(11, 2)])),
    "path64": (64, lambda: mask_of(64, path(list(range(64))))),
    "path64_renumbered": (64, lambda: mask_of(64, path(shuffled(64, 3)))),      # labels travel against the index order
    "path1024": (1024, lambda: mask_of(1024, path(list(range(1024))))),        # the limit: 64 KB of bits, diameter 1023
    "path1024_renumbered": (1024, lambda: mask_of(1024, path(shuffled(1024, 4)))),
}


def check_components(out, mask, N):
    """A 1-D result of graph_components against the reference and against what the host derives from it."""
    ref = NR.components(mask, N)
    for k in ("component", "component_label", "component_edges", "component_regions"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in ("n_edges", "max_extent", "max_regions"):
        assert int(out[k]) == ref[k], k
    assert int(out["n_edges"]) == int(mask.sum())
    comp = out["component"]
    n_of = np.tril_indices(N, -1)[0]
    extent = np.bincount(comp[n_of[mask]], minlength=N)
    regions = np.bincount(comp[comp >= 0], minlength=N)
    assert int(out["max_extent"]) == extent.max() and int(out["max_regions"]) == regions.max()
    return ref


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_components_against_reference(env, name):
    (N, make) = GRAPHS[name]
    mask = make()
    out = env.bl.graph_components(mask, ctx=env.ctx)
    ref = check_components(out, mask, N)
    assert set(out) == {"component", "n_edges", "max_extent", "max_regions", "component_label", "component_edges",
                        "component_regions"}
    if name == "n33_sparse":
        assert len(ref["component_label"]) >= 3 and (ref["component"] == -1).any()
    if name.startswith("path1024"):
        assert ref["component_edges"].tolist() == [1023] and ref["component_regions"].tolist() == [1024]
    again = env.bl.graph_components(env.torch.as_tensor(mask.astype(np.uint8), device="cuda"), ctx=env.ctx, as_numpy=False)
    for k in out:
        assert isinstance(again[k], env.torch.Tensor) and again[k].is_cuda and same(again[k].cpu().numpy(), out[k]), k


def test_graph_components_rows_of_one_call(env):
    masks = np.stack([random_mask(33, 0.03, 1), mask_of(33, path(shuffled(33, 5))), mask_of(33, [])])
    out = env.bl.graph_components(masks, ctx=env.ctx)
    assert set(out) == {"component", "n_edges", "max_extent", "max_regions"} and out["component"].shape == (3, 33)
    for i in range(3):
        ref = NR.components(masks[i], 33)
        assert np.array_equal(out["component"][i], ref["component"])
        assert (out["n_edges"][i], out["max_extent"][i], out["max_regions"][i]) == (ref["n_edges"], ref["max_extent"],
                                                                                   ref["max_regions"])
    assert len(set(out["n_edges"].tolist())) == 3


def test_bits_behind_the_last_connection_change_nothing(env):
    """C = 528 ends in the middle of word 16: through the C ABI, with those 16 bits set."""
    t = env.torch
    (N, C, W) = (33, 528, 17)
    mask = random_mask(33, 0.03, 1)
    padded = np.zeros(32 * W, dtype=np.uint8)
    padded[:C] = mask
    clean = np.packbits(padded, bitorder="little").view(np.uint32).copy()
    dirty = clean.copy()
    dirty[W - 1] |= np.uint32(0xFFFF0000)
    got = []
    for words in (clean, dirty):
        bits = t.as_tensor(words.view(np.int32), device="cuda")
        comp = t.full((N,), -7, dtype=t.int32, device="cuda")
        (ne, me, mr) = (t.full((1,), -7, dtype=t.int32, device="cuda") for _ in range(3))
        env.ctx.call("fcd_graph_components", env.lib.dptr(bits), 1, C, env.lib.dptr(comp), env.lib.dptr(ne), env.lib.dptr(me),
                     env.lib.dptr(mr), env.lib.stream_ptr())
        got.append((comp.cpu().numpy(), int(ne.item()), int(me.item()), int(mr.item())))
    ref = NR.components(mask, N)
    for (labels, *tallies) in got:
        assert np.array_equal(labels, ref["component"]) and tuple(tallies) == (ref["n_edges"], ref["max_extent"], ref["max_regions"])
    # component is optional
    env.ctx.call("fcd_graph_components", env.lib.dptr(bits), 1, C, env.lib.dptr(None), env.lib.dptr(ne), env.lib.dptr(me),
                 env.lib.dptr(mr), env.lib.stream_ptr())
    assert (int(ne.item()), int(me.item()), int(mr.item())) == got[0][1:]


# ---- network_test ----------------------------------------------------------------------------------------------------------

def test_reference_cases_cover_the_paths():
    """Asserted on the reference: the cases below meet empty graphs, many components, a giant component, a large extent."""
    (empty, many, giant, large) = (0, 0, 0, 0)
    for (shape, thr, tail) in CASES:
        ref = NR.case(shape, thr, tail)[3]
        (ne, mx) = (ref["null_n_edges"], ref["null_max_extent"])
        empty += int((ne == 0).sum())
        many = max(many, int(ref["null_components"].max()))
        giant += int(((ne >= 10) & (mx > 0.9 * ne)).sum())
        large = max(large, int(ref["component_edges"].max()) if ref["component_edges"].size else 0)
    assert empty >= 100 and many >= 5 and giant >= 1 and large >= 25


@pytest.mark.parametrize("shape,thr,tail", CASES)
def test_network_test_against_reference(env, shape, thr, tail):
    (b, bt, labels, ref) = NR.case(shape, thr, tail)
    (H, U) = (shape[1], shape[2])
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    assert not (labels == observed[None, :]).all(axis=1).any()
    assert NR.threshold_gap(ref["t"], ref["null_t"], thr) > GAP
    out = env.bl.network_test(b, bt, thr, labels=labels, tail=tail, ctx=env.ctx)
    nptest.assert_allclose(out["t"], ref["t"], rtol=RTOL, atol=0)
    for k in EXACT:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, k
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert out["threshold"] == thr and out["tail"] == tail
    assert np.array_equal(out["labels"], labels) and out["labels"].dtype == np.uint8
    assert set(out) == (set(ref) - {"null_t", "null_components"}) | {"labels"}


def test_bits_through_the_c_abi(env):
    """The (P, W) words themselves, C = 780 over 25 words: every bit against the reference's t, zeros behind C."""
    t = env.torch
    shape = NR.SHAPES[8]
    (b, bt, labels, ref) = NR.case(shape, 2.0)
    (C, P, W) = (b.shape[0], labels.shape[0], 25)
    assert NR.threshold_gap(ref["t"], ref["null_t"], 2.0) > GAP
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device="cuda")
    (bd, btd, labd) = (dev(b), dev(bt), dev(labels))
    for (tail, code) in (("both", 0), ("greater", 1), ("less", 2)):
        bits = t.full((P, W), -1, dtype=t.int32, device="cuda")
        env.ctx.call("fcd_baseline_network_bits", env.lib.dptr(bd), env.lib.dptr(btd), C, shape[1], shape[2], env.lib.dptr(labd), P,
                     2.0, code, env.lib.dptr(bits), env.lib.dptr(None), env.lib.stream_ptr())
        got = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
        assert np.array_equal(got[:, :C].astype(bool), NR.suprathreshold(ref["null_t"], 2.0, tail)), tail
        assert not got[:, C:].any()


def test_identity_row(env):
    (shape, thr) = (NR.SHAPES[1], 2.0)
    (b, bt, labels, _ref) = NR.case(shape, thr)
    (H, U) = shape[1:3]
    P = labels.shape[0]
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    base = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx)
    assert base["component_edges"].shape[0] >= 2
    for where in (P, 0, 17):                                   # last row, first row, inside a group of 16
        more = env.bl.network_test(b, bt, thr, labels=np.insert(labels, where, observed, axis=0), ctx=env.ctx)
        assert more["null_max_extent"][where] == more["component_edges"][0]
        assert more["null_n_edges"][where] == more["edge_mask"].sum()
        assert more["null_max_regions"][where] == more["component_regions"].max()
        rises = (base["component_edges"] <= more["null_max_extent"][where]).astype(np.int64)
        count = lambda r: np.rint(r["p_fwe"] * (1.0 + r["null_max_extent"].shape[0]) - 1.0).astype(np.int64)
        assert np.array_equal(count(more), count(base) + rises) and rises.all()
        for k in ("null_max_extent", "null_max_regions", "null_n_edges"):
            assert np.array_equal(np.delete(more[k], where), base[k]), k
        for k in ("t", "edge_mask", "component", "component_label", "component_edges", "component_regions"):
            assert same(more[k], base[k]), k


def test_chunks_repeatability_and_tensors(env, monkeypatch):
    (shape, thr) = (NR.SHAPES[4], 2.0)                         # P = 64
    (b, bt, labels, _ref) = NR.case(shape, thr)
    one = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx)
    two = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx)
    other = env.bl.network_test(b, bt, thr, labels=labels)      # a context of its own
    given = env.bl.network_test(env.torch.as_tensor(b, device="cuda"), bt, thr, labels=env.torch.as_tensor(labels, device="cuda"),
                                ctx=env.ctx, as_numpy=False)
    arrays = [k for k in one if k not in ("threshold", "tail")]
    for k in arrays:
        assert same(one[k], two[k]) and same(one[k], other[k]), k
        assert isinstance(given[k], env.torch.Tensor) and given[k].is_cuda and same(given[k].cpu().numpy(), one[k]), k
    assert (given["threshold"], given["tail"]) == (one["threshold"], one["tail"]) == (thr, "both") and set(given) == set(one)
    for chunk in (16, 7):
        monkeypatch.setattr(env.bl, "_P_CHUNK", chunk)
        parts = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx)
        assert set(parts) == set(one) and all(same(parts[k], one[k]) for k in arrays), chunk
    monkeypatch.undo()
    (H, U) = shape[1:3]
    drawn = env.bl.network_test(b, bt, thr, n_perm=23, seed=9, tail="greater", ctx=env.ctx)
    assert np.array_equal(drawn["labels"], env.bl.draw_labels(23, H, U, seed=9)) and drawn["null_max_extent"].shape == (23,)


def test_c_abi_refusals(env):
    t = env.torch
    p = env.lib.dptr
    d = t.zeros(4096, dtype=t.float64, device="cuda")
    i = t.zeros(4096, dtype=t.int32, device="cuda")
    s = env.lib.stream_ptr()
    C1025 = 1025 * 1024 // 2

    def bits(*args):
        env.ctx.call("fcd_baseline_network_bits", *args)

    with pytest.raises(ValueError, match="null"):
        bits(p(d), p(None), 3, 4, 4, p(i), 1, 2.0, 0, p(i), p(d), s)
    with pytest.raises(ValueError, match="null"):
        bits(p(d), p(d), 3, 4, 4, p(i), 1, 2.0, 0, p(None), p(d), s)
    with pytest.raises(ValueError, match="P = 1"):
        bits(p(d), p(d), 3, 4, 4, p(None), 2, 2.0, 0, p(i), p(d), s)
    with pytest.raises(ValueError, match="must be >= 1"):
        bits(p(d), p(d), 3, 4, 4, p(i), 0, 2.0, 0, p(i), p(d), s)
    with pytest.raises(ValueError, match="triangular"):
        bits(p(d), p(d), 5, 4, 4, p(i), 1, 2.0, 0, p(i), p(d), s)
    with pytest.raises(ValueError, match="needs 3"):
        bits(p(d), p(d), 3, 1, 1, p(i), 1, 2.0, 0, p(i), p(d), s)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            bits(p(d), p(d), 3, 4, 4, p(i), 1, bad, 0, p(i), p(d), s)
    for bad in (-1, 3):
        with pytest.raises(ValueError, match="tail"):
            bits(p(d), p(d), 3, 4, 4, p(i), 1, 2.0, bad, p(i), p(d), s)
    with pytest.raises(NotImplementedError, match="at most 1024"):
        bits(p(d), p(d), 3, 1000, 25, p(i), 1, 2.0, 0, p(i), p(d), s)                  # S = 1025
    with pytest.raises(NotImplementedError, match="regions, at most 1024"):
        bits(p(d), p(d), C1025, 4, 4, p(i), 1, 2.0, 0, p(i), p(d), s)                  # refused before anything is read

    def comps(*args):
        env.ctx.call("fcd_graph_components", *args)

    with pytest.raises(ValueError, match="null"):
        comps(p(None), 1, 3, p(i), p(i), p(i), p(i), s)
    with pytest.raises(ValueError, match="null"):
        comps(p(i), 1, 3, p(i), p(i), p(None), p(i), s)
    with pytest.raises(ValueError, match="must be >= 1"):
        comps(p(i), 0, 3, p(i), p(i), p(i), p(i), s)
    with pytest.raises(ValueError, match="triangular"):
        comps(p(i), 1, 5, p(i), p(i), p(i), p(i), s)
    with pytest.raises(NotImplementedError, match="regions, at most 1024"):
        comps(p(i), 1, C1025, p(i), p(i), p(i), p(i), s)


def test_end_to_end_on_sampled_data(env):
    """
    SharedRegionModel.sample at 16 regions, pi = 0.2, seed 3 plants regions {0, 4, 7, 9}; on the reference the largest
    component at threshold 2.5 has 11 connections, holds all four and no labelling of 199 reaches it (p = 1/200).  The same
    recipe with every column drawn from the control law (seed 103) leaves one lone connection, p = 0.875.
    """
    (N, H, U, P, seed) = (16, 20, 20, 199, 3)
    model = env.pkg.SharedRegionModel()
    model.pi = 0.2
    (r, _t, _f, _ft, b, bt) = model.sample(N, H, U, seed=seed)
    planted = np.flatnonzero(r)
    assert planted.tolist() == [0, 4, 7, 9]
    out = env.bl.network_test(b, bt, 2.5, n_perm=P, seed=seed, ctx=env.ctx)
    assert out["p_fwe"].shape[0] >= 1 and out["p_fwe"][0] < 0.05
    top = out["component_label"][0]
    assert (out["component"][planted] == top).all() and (out["p_fwe_region"][planted] < 0.05).all()
    assert out["null_max_extent"].shape == (P,) and out["labels"].shape == (P, H + U)
    (_r, _t, _f, _ft, b0, _bt0) = model.sample(N, H + U, 1, seed=seed + 100)
    null = env.bl.network_test(b0[:, :H], b0[:, H:], 2.5, n_perm=P, seed=seed, ctx=env.ctx)
    assert not (null["p_fwe"] < 0.01).any() and null["p_fwe"].shape[0] >= 1
    assert np.isnan(null["p_fwe_region"]).sum() == N - null["component_regions"].sum()
