"""
The classical baselines on the device (fcd_baseline_normative, fcd_baseline_group_perm, fcdiff_amd.baseline) against
tests/baseline_ref.py.

Tolerance: rtol 1e-10 on every floating-point output, what the project holds its fp64 kernels to against the oracle.  Counts
and p-values are compared exactly; that is legitimate only where no null value lies within relative 1e-9 of a value it is
compared with, which every such test asserts on the reference arrays first.  The references are made once per shape.
"""
import functools

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_ref as BR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GAP = 1e-9
# three more shapes for group_test alone, where the kernel takes another path: a second label word per lane (S > 128), all
# eight of them (S = 1024, the limit), and a second block of 128 permutations whose last group of 16 is partial
GROUP_EXTRA = [(4, 100, 45, 20, 5), (3, 1000, 24, 3, 6), (4, 10, 9, 150, 7)]


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


@functools.lru_cache(maxsize=None)
def norm_case(i, missing):
    (b, bt, _labels) = BR.make_data(*BR.SHAPES[i], f=BR.MISSING[i] if missing else None)
    return b, bt, BR.normative(b, bt)


@functools.lru_cache(maxsize=None)
def group_case(shape):
    (b, bt, labels) = BR.make_data(*shape)
    return b, bt, labels, BR.group_test(b, bt, labels)


NORM_CASES = [(i, False) for i in range(5)] + [(i, True) for i in sorted(BR.MISSING)]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def close(got, want, name):
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN positions differ" % name
    nptest.assert_allclose(got, want, rtol=RTOL, atol=0, err_msg=name)


@pytest.mark.parametrize("i,missing", NORM_CASES)
def test_normative_against_reference(env, i, missing):
    (b, bt, ref) = norm_case(i, missing)
    out = env.bl.normative(b, bt, missing_data=missing, return_z=True, ctx=env.ctx)
    for k in ("z", "z0", "msq", "msq0", "max0"):
        close(out[k], ref[k], k)
    for k in ("n_edges", "n_over", "n_edges0", "n_over0", "n_controls"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    assert set(out) == set(ref)
    plain = env.bl.normative(b, bt, missing_data=missing, ctx=env.ctx)
    assert set(plain) == set(ref) - {"z", "z0"} and all(same(plain[k], out[k]) for k in plain)


@pytest.mark.parametrize("i,missing", NORM_CASES)
def test_normative_pvalues_against_reference(env, i, missing):
    (b, bt, ref) = norm_case(i, missing)
    N = ref["msq"].shape[0]
    assert min(BR.smallest_gap(ref["msq0"][n], ref["msq"][n]) for n in range(N)) > GAP
    assert BR.smallest_gap(ref["max0"], ref["msq"]) > GAP
    out = env.bl.normative(b, bt, missing_data=missing, ctx=env.ctx)
    nptest.assert_array_equal(out["p_region"], ref["p_region"])
    nptest.assert_array_equal(out["p_fwe"], ref["p_fwe"])


def test_normative_threshold_counts(env):
    """n_over at a threshold that many scores pass (at 3.0 few do at these sizes)."""
    (b, bt, _ref) = norm_case(1, False)
    ref = BR.normative(b, bt, z_threshold=1.0)
    zs = np.abs(np.concatenate([ref["z"].reshape(-1), ref["z0"].reshape(-1)]))
    assert np.abs(zs / 1.0 - 1.0).min() > GAP and ref["n_over"].sum() > 50 and ref["n_over0"].sum() > 50
    out = env.bl.normative(b, bt, z_threshold=1.0, ctx=env.ctx)
    assert np.array_equal(out["n_over"], ref["n_over"]) and np.array_equal(out["n_over0"], ref["n_over0"])


def test_connection_with_fewer_than_three_controls(env):
    (b, bt, _ref) = norm_case(1, False)
    c0 = 40
    (n, m) = env.pkg.util.c_to_nm(c0)
    full = env.bl.normative(b, bt, missing_data=True, return_z=True, ctx=env.ctx)
    b2 = b.copy()
    b2[c0, 2:] = np.nan
    out = env.bl.normative(b2, bt, missing_data=True, return_z=True, ctx=env.ctx)
    assert out["n_controls"][c0] == 2
    assert np.isnan(out["z"][c0]).all() and np.isnan(out["z0"][c0]).all()
    touched = np.zeros(full["n_edges"].shape[0], dtype=np.int64)
    touched[[n, m]] = 1
    assert np.array_equal(out["n_edges"], full["n_edges"] - touched[:, None])
    assert np.array_equal(out["n_edges0"], full["n_edges0"] - touched[:, None])
    ref = BR.normative(b2, bt)
    for k in ("z", "z0", "msq", "msq0"):
        close(out[k], ref[k], k)


def test_dominant_control(env):
    """One control 1000 times the others on every connection: a downdated sum of squares would lose the others' spread."""
    (b, bt, _ref) = norm_case(0, False)
    b2 = b.copy()
    b2[:, 1] *= 1000.0
    ref = BR.normative(b2, bt)
    out = env.bl.normative(b2, bt, return_z=True, ctx=env.ctx)
    close(out["z0"], ref["z0"], "z0")
    close(out["msq0"], ref["msq0"], "msq0")


def test_normative_patient_chunks_and_tensors(env, monkeypatch):
    (b, bt, _ref) = norm_case(4, True)
    whole = env.bl.normative(b, bt, missing_data=True, return_z=True, ctx=env.ctx)
    monkeypatch.setattr(env.bl, "_U_CHUNK", 3)
    parts = env.bl.normative(env.torch.as_tensor(b, device="cuda"), env.torch.as_tensor(bt), missing_data=True, return_z=True,
                             ctx=env.ctx, as_numpy=False)
    assert set(parts) == set(whole)
    for k in whole:
        assert isinstance(parts[k], env.torch.Tensor) and parts[k].is_cuda, k
        assert same(parts[k].cpu().numpy(), whole[k]), k


@pytest.mark.parametrize("shape", BR.SHAPES + GROUP_EXTRA)
def test_group_test_against_reference(env, shape):
    (b, bt, labels, ref) = group_case(shape)
    (H, U) = (shape[1], shape[2])
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    assert not (labels == observed[None, :]).all(axis=1).any()
    C = b.shape[0]
    assert min(BR.smallest_gap(np.abs(ref["null_t"][:, c]), np.abs(ref["t"][c])) for c in range(C)) > GAP
    assert min(BR.smallest_gap(ref["null_region"][:, n], ref["region"][n]) for n in range(shape[0])) > GAP
    assert BR.smallest_gap(ref["null_max_t"], np.abs(ref["t"])) > GAP
    assert BR.smallest_gap(ref["null_max_region"], ref["region"]) > GAP
    out = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    for k in ("t", "region", "null_max_t", "null_max_region"):
        close(out[k], ref[k], k)
    for k in ("count_t", "count_region"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["labels"], labels) and out["labels"].dtype == np.uint8
    assert set(out) == (set(ref) - {"null_t", "null_region"}) | {"labels"}


def test_group_test_identity_row(env):
    (b, bt, labels, _ref) = group_case(BR.SHAPES[0])
    (H, U) = BR.SHAPES[0][1:3]
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    base = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    for where in (labels.shape[0], 0, 17):                    # last row, first row, inside a tile of 16
        more = env.bl.group_test(b, bt, labels=np.insert(labels, where, observed, axis=0), ctx=env.ctx)
        assert np.array_equal(more["count_t"], base["count_t"] + 1)
        assert np.array_equal(more["count_region"], base["count_region"] + 1)
        assert more["null_max_t"][where] == np.abs(more["t"]).max()
        assert more["null_max_region"][where] == more["region"].max()
        assert same(np.delete(more["null_max_t"], where), base["null_max_t"]) and same(more["t"], base["t"])


def test_repeatable(env):
    (b, bt, _ref) = norm_case(1, True)
    one = env.bl.normative(b, bt, missing_data=True, return_z=True, ctx=env.ctx)
    two = env.bl.normative(b, bt, missing_data=True, return_z=True, ctx=env.ctx)
    assert all(same(one[k], two[k]) for k in one)
    (b, bt, labels, _ref) = group_case(BR.SHAPES[4])
    one = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    two = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    assert all(same(one[k], two[k]) for k in one)
    other = env.bl.group_test(b, bt, labels=labels)              # a context of its own
    assert all(same(one[k], other[k]) for k in one)


def test_drawn_labels_and_device_tensors(env):
    (b, bt, _labels, _ref) = group_case(BR.SHAPES[1])
    (H, U) = BR.SHAPES[1][1:3]
    out = env.bl.group_test(b, bt, n_perm=23, seed=9, ctx=env.ctx)
    assert np.array_equal(out["labels"], env.bl.draw_labels(23, H, U, seed=9)) and out["null_max_t"].shape == (23,)
    given = env.bl.group_test(env.torch.as_tensor(b, device="cuda"), bt, labels=out["labels"], ctx=env.ctx, as_numpy=False)
    for k in out:
        assert isinstance(given[k], env.torch.Tensor) and given[k].is_cuda and same(given[k].cpu().numpy(), out[k]), k


def test_c_abi_refusals(env):
    t = env.torch
    p = env.lib.dptr
    d = t.zeros(4096, dtype=t.float64, device="cuda")
    i = t.zeros(4096, dtype=t.int64, device="cuda")
    s = env.lib.stream_ptr()
    with pytest.raises(NotImplementedError, match="at most 1024"):
        env.ctx.call("fcd_baseline_normative", p(d), p(d), 3, 1025, 1, 3.0, p(d), p(i), p(i), p(d), p(i), p(i), p(i), p(None), p(None), s)
    with pytest.raises(ValueError, match="triangular"):
        env.ctx.call("fcd_baseline_normative", p(d), p(d), 4, 5, 1, 3.0, p(d), p(i), p(i), p(d), p(i), p(i), p(i), p(None), p(None), s)
    with pytest.raises(ValueError, match="null"):
        env.ctx.call("fcd_baseline_normative", p(d), p(None), 3, 5, 1, 3.0, p(d), p(i), p(i), p(d), p(i), p(i), p(i), p(None), p(None), s)
    with pytest.raises(NotImplementedError, match="at most 1024"):
        env.ctx.call("fcd_baseline_group_perm", p(d), p(d), 3, 1000, 25, p(i), 1, p(d), p(d), p(d), p(d), p(i), p(i), s)
    with pytest.raises(ValueError, match="triangular"):
        env.ctx.call("fcd_baseline_group_perm", p(d), p(d), 5, 4, 4, p(i), 1, p(d), p(d), p(d), p(d), p(i), p(i), s)
    with pytest.raises(ValueError, match="needs 3"):
        env.ctx.call("fcd_baseline_group_perm", p(d), p(d), 3, 1, 1, p(i), 1, p(d), p(d), p(d), p(d), p(i), p(i), s)


def test_end_to_end_on_model_data(env):
    (N, H, U) = (12, 24, 12)
    model = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(N, H, U, seed=5)
    order = env.pkg.util.upper_to_lower_edge_order(N)
    (b, bt) = (np.asarray(b)[order], np.asarray(bt)[order])
    nv = env.bl.normative(b, bt, ctx=env.ctx)
    for k in ("p_region", "p_fwe"):
        assert nv[k].shape == (N, U) and np.isfinite(nv[k]).all() and (nv[k] > 0).all() and (nv[k] <= 1).all()
    assert (nv["p_fwe"] >= nv["p_region"]).all()
    assert (nv["n_edges"] == N - 1).all() and (nv["n_controls"] == H).all()
    gt = env.bl.group_test(b, bt, n_perm=200, ctx=env.ctx)
    for k in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        assert np.isfinite(gt[k]).all() and (gt[k] > 0).all() and (gt[k] <= 1).all()
    assert (gt["p_fwe_t"] >= gt["p_t"]).all() and (gt["p_fwe_region"] >= gt["p_region"]).all()
    assert gt["labels"].shape == (200, H + U)
