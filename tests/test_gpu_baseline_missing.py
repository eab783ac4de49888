"""
The permutation baselines with their options (missing_data=True, variance="welch") on the device
(fcd_baseline_group_perm_opt, fcd_baseline_network_bits_opt) against tests/baseline_missing_ref.py.

Tolerance: rtol 1e-10 on every floating-point output, the project's bound for its fp64 kernels against a loop-level oracle
(the reference evaluates the direct two-sample formulas, the kernel the centred closed forms; they agree to about 1e-12 at
these sizes).  Counts, bits and p-values are compared exactly; that is legitimate only where no null value lies within
relative GAP = 1e-9 of the value it is compared with, or of the threshold, which every such test asserts on the reference
arrays first (gaps_group, gaps_network), or, for the integer cases, where baseline_missing_ref.Exact.check_conditions holds.
The references are made once per case.
"""
import functools
import math

import numpy as np
import numpy.testing as nptest
import pytest

import baseline_missing_ref as MR
import baseline_ref as BR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
GAP = 1e-9
NAN = math.nan
EXTRA = [(4, 100, 45, 20, 5), (3, 1000, 24, 3, 6), (4, 10, 9, 150, 7)]      # test_gpu_baseline.GROUP_EXTRA
SHAPES = BR.SHAPES + EXTRA
# fraction of NaN per shape: baseline_ref.MISSING where it names one, 0.1 elsewhere
FRACTION = dict((s, BR.MISSING.get(i, 0.1)) for (i, s) in enumerate(SHAPES))
REFUSED = ((4, 3, 1, 1, 3), "welch")                                        # one patient: Welch is refused there
CASES = [(s, v) for s in SHAPES for v in MR.VARIANCES if (s, v) != REFUSED]
TAILS = ("both", "greater", "less")
THRESHOLD = 1.5


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


def without_complements(b, bt, labels, seed, keep=()):
    """
    labels with every row drawn again (numpy.random.default_rng(seed), rows of `keep` excepted) that labels the OBSERVED
    subjects of some connection as the complement of the observed labelling does.  Such a row ties |t| with the observed
    value in exact arithmetic, but the device's A is then minus the sum over the other group only up to rounding: a tie the
    doubles do not keep, which an exact comparison of counts must not meet.  (On complete data only H == U has complements.)
    """
    obs = ~np.isnan(np.concatenate([b, bt], axis=1))
    (H, U) = (b.shape[1], bt.shape[1])
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    labels = labels.copy()

    def complement_somewhere(row):
        return bool(((row[None, :] != observed[None, :]) | ~obs).all(axis=1)[obs.sum(axis=1) >= 2].any())

    for p in range(labels.shape[0]):
        while p not in keep and complement_somewhere(labels[p]):
            labels[p] = 0
            labels[p, rng.permutation(H + U)[:U]] = 1
    return labels


@functools.lru_cache(maxsize=None)
def data_of(shape):
    (b, bt, labels) = MR.make_missing(shape, FRACTION[shape])
    return b, bt, without_complements(b, bt, labels, 100 + shape[4])


@functools.lru_cache(maxsize=None)
def t_of(shape, variance):
    (b, bt, labels) = data_of(shape)
    return MR.all_t(b, bt, labels, variance)


@functools.lru_cache(maxsize=None)
def group_ref(shape, variance):
    (b, bt, labels) = data_of(shape)
    return MR.group_test(b, bt, labels, variance, t_pair=t_of(shape, variance))


@functools.lru_cache(maxsize=None)
def network_ref(shape, variance, threshold, tail):
    (b, bt, labels) = data_of(shape)
    return MR.network_test(b, bt, labels, threshold, tail, variance, t_pair=t_of(shape, variance))


def gaps_group(ref, b, bt, labels):
    """
    The smallest relative gap between a null value and the observed value it is compared with, over the four comparisons.
    Left out: the ties that missing data make by themselves.  A labelling that labels the OBSERVED subjects of a connection as
    the observed labelling does differs from it only where the centred value and the mask are 0: the device adds exact zeros
    to the same sums and the reference walks the same two lists, so both reproduce the observed value bit for bit.
    """
    obs = ~np.isnan(np.concatenate([b, bt], axis=1))                                  # (C, S)
    observed = np.array([0] * b.shape[1] + [1] * bt.shape[1], dtype=np.uint8)
    differs = (labels[:, None, :] != observed[None, None, :]) & obs[None, :, :]
    alike = ~differs.any(axis=2)                                                      # (P, C)
    (P, C) = alike.shape
    N = ref["region"].shape[0]
    E = BR.edges_of(N)
    live = ~np.isnan(ref["t"])
    alike_n = np.array([[all(alike[p, c] for c in E[n] if live[c]) for n in range(N)] for p in range(P)])
    (at, nt) = (np.abs(ref["t"]), np.abs(ref["null_t"]))
    gaps = [BR.smallest_gap(nt[~alike[:, c], c], at[c]) for c in range(C)]
    gaps += [BR.smallest_gap(ref["null_region"][~alike_n[:, n], n], ref["region"][n]) for n in range(N)]
    for p in range(P):
        # a maximum attained at a connection (region) labelled alike ties that connection's (region's) observed value
        tied_c = [c for c in range(C) if live[c] and alike[p, c] and nt[p, c] == ref["null_max_t"][p]]
        tied_n = [n for n in range(N) if alike_n[p, n] and ref["null_region"][p, n] == ref["null_max_region"][p]]
        gaps.append(BR.smallest_gap(ref["null_max_t"][p], np.delete(at, tied_c)))
        gaps.append(BR.smallest_gap(ref["null_max_region"][p], np.delete(ref["region"], tied_n)))
    return min(gaps)


def gaps_network(t, null_t, threshold):
    a = np.abs(np.concatenate([np.asarray(t).reshape(-1), np.asarray(null_t).reshape(-1)]))
    a = a[~np.isnan(a)]
    return float((np.abs(a - threshold) / threshold).min()) if a.size else np.inf


GROUP_KEYS = {"t", "region", "null_max_t", "null_max_region", "count_t", "count_region", "p_t", "p_region", "p_fwe_t",
              "p_fwe_region", "labels", "n_controls", "n_patients"}


def check_group(out, ref, labels):
    for k in ("t", "region", "null_max_t", "null_max_region"):
        close(out[k], ref[k], k)
    for k in ("count_t", "count_region", "n_controls", "n_patients"):
        assert out[k].dtype == np.int64 and np.array_equal(out[k], ref[k]), k
    for k in ("p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.array_equal(out["labels"], labels) and set(out) == GROUP_KEYS


def check_network(out, ref, labels):
    close(out["t"], ref["t"], "t")
    for k in ("edge_mask", "component", "component_label", "component_edges", "component_regions", "null_max_extent",
              "null_max_regions", "null_n_edges", "p_fwe", "p_fwe_region", "n_controls", "n_patients"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    assert out["threshold"] == ref["threshold"] and out["tail"] == ref["tail"] and np.array_equal(out["labels"], labels)
    assert set(out) == (set(ref) - {"null_t", "null_components"}) | {"labels"}


# ---- complete data: the option changes nothing ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [BR.SHAPES[0], BR.SHAPES[1], EXTRA[0]])
def test_complete_data_is_the_default_call_bit_for_bit(env, shape):
    (b, bt, labels) = BR.make_data(*shape)
    (C, H, U) = (b.shape[0], shape[1], shape[2])
    base = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, ctx=env.ctx)
    assert set(out) == set(base) | {"n_controls", "n_patients"}
    for k in base:
        assert same(out[k], base[k]) and out[k].dtype == base[k].dtype, k
    for (k, v) in (("n_controls", H), ("n_patients", U)):
        assert out[k].dtype == np.int64 and out[k].shape == (C,) and (out[k] == v).all()
    for thr in (1.5, 2.5):
        base = env.bl.network_test(b, bt, thr, labels=labels, ctx=env.ctx)
        out = env.bl.network_test(b, bt, thr, labels=labels, missing_data=True, ctx=env.ctx)
        assert set(out) == set(base) | {"n_controls", "n_patients"}
        for k in base:
            assert same(out[k], base[k]) if isinstance(base[k], np.ndarray) else out[k] == base[k], k
        assert (out["n_controls"] == H).all() and (out["n_patients"] == U).all() and out["n_controls"].dtype == np.int64


def test_welch_on_complete_data_adds_no_key(env):
    (b, bt, labels) = BR.make_data(*BR.SHAPES[1])
    base = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    out = env.bl.group_test(b, bt, labels=labels, variance="welch", ctx=env.ctx)
    assert set(out) == set(base) and not same(out["t"], base["t"])
    ref = MR.group_test(b, bt, labels, "welch")
    assert gaps_group(ref, b, bt, labels) > GAP
    for k in ("t", "region", "null_max_t", "null_max_region"):
        close(out[k], ref[k], k)
    for k in ("count_t", "count_region", "p_t", "p_region", "p_fwe_t", "p_fwe_region"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    both = env.bl.group_test(b, bt, labels=labels, variance="welch", missing_data=True, ctx=env.ctx)
    assert all(same(both[k], out[k]) for k in out)              # the counted n1 = U and n = S: the same numbers


# ---- against the reference with NaN --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,variance", CASES)
def test_group_test_against_reference(env, shape, variance):
    (b, bt, labels) = data_of(shape)
    ref = group_ref(shape, variance)
    assert np.isnan(b).any() or np.isnan(bt).any()
    assert gaps_group(ref, b, bt, labels) > GAP
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    check_group(out, ref, labels)


@pytest.mark.parametrize("shape,variance", CASES)
def test_network_test_against_reference(env, shape, variance):
    (b, bt, labels) = data_of(shape)
    (t, null_t) = t_of(shape, variance)
    assert gaps_network(t, null_t, THRESHOLD) > GAP
    for tail in TAILS:
        out = env.bl.network_test(b, bt, THRESHOLD, labels=labels, tail=tail, missing_data=True, variance=variance, ctx=env.ctx)
        check_network(out, network_ref(shape, variance, THRESHOLD, tail), labels)


def test_welch_with_one_patient_is_refused(env):
    (b, bt, labels) = data_of(REFUSED[0])
    for kw in ({}, {"missing_data": True}):
        with pytest.raises(ValueError, match="welch"):
            env.bl.group_test(b, bt, labels=labels, variance="welch", ctx=env.ctx, **kw)
        with pytest.raises(ValueError, match="welch"):
            env.bl.network_test(b, bt, THRESHOLD, labels=labels, variance="welch", ctx=env.ctx, **kw)


# ---- engineered rows -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def engineered():
    """baseline_ref.SHAPES[0] = (7, 5, 4, 50), complete, with rows made degenerate by hand; labels[3] has its ones on the four
    missing controls of connection 9 (n1 = 0 there), labels[20] on the four observed subjects of connection 11 (n0 = 0).
    The other rows are without_complements'."""
    (b, bt, labels) = BR.make_data(*BR.SHAPES[0])
    (b, bt, labels) = (b.copy(), bt.copy(), labels.copy())
    bt[2, :] = NAN                                   # missing in every patient: dead
    b[5, 1:] = NAN                                   # n = 2: one control, one patient
    bt[5, 1:] = NAN
    b[7] = [0.3, NAN, 0.3, NAN, NAN]                 # the observed values all equal, NaN elsewhere: constant
    bt[7] = [NAN, 0.3, 0.3, NAN]
    b[9, :4] = NAN                                   # missing in 4 of the 5 controls: n0 = 1 as observed, n1 = 0 under labels[3]
    b[11, :4] = NAN                                  # ... and in one patient too: n = 4, n0 = 0 under labels[20]
    bt[11, 0] = NAN
    b[13, :3] = NAN                                  # two controls left: Welch is defined as observed, not under every labelling;
    bt[13] += 0.5                                    # ... with a large observed t, so that few defined labellings exceed it
    bt[14, 3] = NAN                                  # the last subject (S = 9, inside the zero padding of the last K-step)
    b[0, 0] = NAN                                    # the first value of a row: the comparand of the constant test moves on
    b[17, :] = NAN                                   # observed in nobody: n = 0, dead
    bt[17, :] = NAN
    labels[3] = [1, 1, 1, 1, 0, 0, 0, 0, 0]
    labels[20] = [0, 0, 0, 0, 1, 0, 1, 1, 1]
    labels = without_complements(b, bt, labels, 200, keep=(3, 20))
    return b, bt, labels


@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_engineered_rows(env, variance):
    (b, bt, labels) = engineered()
    (t, null_t) = MR.all_t(b, bt, labels, variance)
    ref = MR.group_test(b, bt, labels, variance, t_pair=(t, null_t))
    assert gaps_group(ref, b, bt, labels) > GAP and gaps_network(t, null_t, THRESHOLD) > GAP
    # what the rows were made for, on the reference: dead connections, and labellings that cannot be evaluated
    dead = sorted([2, 5, 7, 17] + ([9, 11] if variance == "welch" else []))
    assert np.flatnonzero(np.isnan(ref["t"])).tolist() == dead
    probe = 13 if variance == "welch" else 9
    undefined = np.isnan(ref["null_t"][:, probe])
    assert undefined.any() and not undefined.all()
    if variance == "pooled":
        assert undefined[3] and np.isnan(ref["null_t"][20, 11]) and ref["count_t"][9] >= 1 and ref["count_t"][11] >= 1
    assert ref["count_t"][probe] >= undefined.sum() and ref["count_t"][probe] < labels.shape[0]
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    check_group(out, ref, labels)
    assert out["n_controls"][17] == 0 and out["n_patients"][17] == 0 and out["n_patients"][2] == 0 and out["n_controls"][9] == 1
    assert (out["count_t"][dead] == 0).all() and np.isnan(out["p_t"][dead]).all() and np.isnan(out["p_fwe_t"][dead]).all()
    # a dead connection takes exactly its term from both its regions: connection 2 = (2, 1) against the same data with its
    # patients back
    if variance == "pooled":
        (b2, bt2) = (b.copy(), bt.copy())
        bt2[2] = BR.make_data(*BR.SHAPES[0])[1][2]
        full = env.bl.group_test(b2, bt2, labels=labels, missing_data=True, ctx=env.ctx)
        lost = np.zeros(7)
        lost[[1, 2]] = full["t"][2] ** 2
        nptest.assert_allclose(out["region"], full["region"] - lost, rtol=1e-13)
        assert same(np.delete(out["t"], 2), np.delete(full["t"], 2))
    for tail in TAILS:
        net = env.bl.network_test(b, bt, THRESHOLD, labels=labels, tail=tail, missing_data=True, variance=variance, ctx=env.ctx)
        check_network(net, MR.network_test(b, bt, labels, THRESHOLD, tail, variance, t_pair=(t, null_t)), labels)
        assert not net["edge_mask"][dead].any()


@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_nan_only_in_the_row_a_masked_column_rereads(env, variance):
    """At 7 regions a tile has 6 valid columns; the others re-read connection 20 (the last), whose mask words and n they
    then load too."""
    (b, bt, labels) = BR.make_data(*BR.SHAPES[0])
    b = b.copy()
    b[20, 3] = NAN
    (t, null_t) = MR.all_t(b, bt, labels, variance)
    ref = MR.group_test(b, bt, labels, variance, t_pair=(t, null_t))
    assert gaps_group(ref, b, bt, labels) > GAP and gaps_network(t, null_t, THRESHOLD) > GAP
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    check_group(out, ref, labels)
    net = env.bl.network_test(b, bt, THRESHOLD, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    check_network(net, MR.network_test(b, bt, labels, THRESHOLD, "both", variance, t_pair=(t, null_t)), labels)


# ---- the observed labelling among the rows -------------------------------------------------------------------------------------

def _bits_rows(env, b, bt, labels, threshold, tail, flags):
    """(P, C) bool straight from fcd_baseline_network_bits_opt."""
    t = env.torch
    (C, H) = b.shape
    U = bt.shape[1]
    W = (C + 31) // 32
    (bd, btd) = (t.as_tensor(b, device="cuda"), t.as_tensor(bt, device="cuda"))
    lab = t.as_tensor(np.ascontiguousarray(labels), device="cuda")
    bits = t.zeros((labels.shape[0], W), dtype=t.int32, device="cuda")
    env.ctx.call("fcd_baseline_network_bits_opt", env.lib.dptr(bd), env.lib.dptr(btd), C, H, U, env.lib.dptr(lab), labels.shape[0],
                 float(threshold), env.bl.TAILS[tail], flags, env.lib.dptr(bits), env.lib.dptr(None), env.lib.stream_ptr())
    rows = np.unpackbits(bits.cpu().numpy().view(np.uint8).reshape(labels.shape[0], -1), axis=1, bitorder="little")
    return rows[:, :C].astype(bool)


@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_identity_row(env, variance):
    (b, bt, labels) = engineered()
    (H, U) = BR.SHAPES[0][1:3]
    observed = np.array([0] * H + [1] * U, dtype=np.uint8)
    assert not (labels == observed[None, :]).all(axis=1).any()
    kw = dict(missing_data=True, variance=variance, ctx=env.ctx)
    flags = env.bl.FLAG_MISSING | (env.bl.FLAG_WELCH if variance == "welch" else 0)
    base = env.bl.group_test(b, bt, labels=labels, **kw)
    live = ~np.isnan(base["t"])
    assert live.sum() >= 12 and not live.all()
    for where in (labels.shape[0], 0, 17):                    # last row, first row, inside a tile of 16
        rows = np.insert(labels, where, observed, axis=0)
        more = env.bl.group_test(b, bt, labels=rows, **kw)
        assert np.array_equal(more["count_t"], base["count_t"] + live)
        assert np.array_equal(more["count_region"], base["count_region"] + 1)
        assert more["null_max_t"][where] == np.nanmax(np.abs(more["t"]))
        assert more["null_max_region"][where] == more["region"].max()
        assert same(np.delete(more["null_max_t"], where), base["null_max_t"])
        assert same(np.delete(more["null_max_region"], where), base["null_max_region"])
        for k in ("t", "region", "n_controls", "n_patients"):
            assert same(more[k], base[k]), k
        for tail in TAILS:
            net = env.bl.network_test(b, bt, THRESHOLD, labels=rows, tail=tail, **kw)
            got = _bits_rows(env, b, bt, rows, THRESHOLD, tail, flags)
            assert np.array_equal(got[where], net["edge_mask"]) and net["null_n_edges"][where] == net["edge_mask"].sum()
            assert np.array_equal(np.delete(got, where, axis=0), _bits_rows(env, b, bt, labels, THRESHOLD, tail, flags))
            assert same(net["t"], more["t"])


# ---- exact ties ----------------------------------------------------------------------------------------------------------------

BELOW = math.nextafter(2.0, 0.0)


@functools.lru_cache(maxsize=None)
def tied_case(name):
    """T1 (7, 5, 5, 40) + 4: integer rows in -50 .. 50 with 15 % missing whose observed sums are multiples of n.  (The wide
    range leaves few ties between unlike labellings: under Welch two labellings with n1 = n0 and the same |A| tie exactly
    whatever their B, and the device's two variance terms round apart.)  H == U, so the complement of the observed labelling
    is a labelling: rows 5 and 41 hold it, rows 0 and 17 the observed one.
    T2 (5, 5, 4, 12): connections 0 and 1 have t^2 = 4 exactly with one control missing (n = 8, k = 1/2, A = +/-4, Q = 20;
    Welch: B = 10, SS1 = SS0 = 6, v = 1, every step exact in doubles); connections 2 and 3 are completely separated with both
    groups constant, four against four (k = 1/2, g = Q = 72 and SS1 = SS0 = 0 exactly); row 3 labels the subjects 2, 3, 5, 6
    of connection 0: the values 0, 0, 3, 1."""
    if name == "T1":
        (N, H, U, P) = (7, 5, 5, 40)
        rng = np.random.default_rng(35)
        X = MR.integer_rows_missing(21, H + U, rng, 0.15, span=50)
        obs = np.array([0] * H + [1] * U, dtype=np.uint8)
        labels = list(BR.make_data(N, H, U, P, 9)[2])
        for (where, row) in ((0, obs), (5, 1 - obs), (17, obs), (41, 1 - obs)):
            labels.insert(where, row)
        return X[:, :H].copy(), X[:, H:].copy(), np.stack(labels), (1.5, 2.5), ()
    (N, H, U, P) = (5, 5, 4, 12)
    rng = np.random.default_rng(32)
    X = MR.integer_rows_missing(10, H + U, rng, 0.1)
    X[0] = [-3, -1, 0, 0, NAN, 3, 1, 0, 0]
    X[1] = [3, 1, 0, 0, NAN, -3, -1, 0, 0]
    X[2] = [0, 0, NAN, 0, 0, 6, 6, 6, 6]
    X[3] = [6, NAN, 6, 6, 6, 0, 0, 0, 0]
    labels = BR.make_data(N, H, U, P, 10)[2].copy()
    labels[3] = [0, 0, 1, 1, 0, 1, 1, 0, 0]
    return X[:, :H].copy(), X[:, H:].copy(), labels, (1.5, 2.0, 2.5), (2.0,)


@functools.lru_cache(maxsize=None)
def tied_exact(name, variance):
    (b, bt, labels, thresholds, boundary) = tied_case(name)
    ex = MR.Exact(b, bt, labels, variance)
    ex.check_conditions(thresholds=thresholds, boundary=boundary)
    return ex


def boundary_is_the_engineered_one(ex):
    """Every t^2 within GAP of 4 is exactly 4 and has the (|A|, Q, n, n1, B) of the row worked by hand: there the device's t^2
    is 4.0 exactly, above BELOW^2 = 4 - 2^-50 and not above 2.0^2."""
    hits = 0
    for p in range(ex.P + 1):
        for c in ex.live:
            v = ex.t2[p][c]
            if v is not None and v != math.inf and abs(float(v) - 4.0) <= 4.0 * GAP:
                assert v == 4 and ex.key(p, c) == ex.key(0, 0), (p, c)
                hits += 1
    return hits


@pytest.mark.parametrize("name", ["T1", "T2"])
@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_exact_ties(env, name, variance):
    (b, bt, labels, thresholds, _boundary) = tied_case(name)
    ex = tied_exact(name, variance)
    assert all(ex.integer)
    (tt, tr) = ex.ties()
    assert (tt >= 20 and tr >= 7) if name == "T1" else tt >= 1
    ref = ex.group_test()
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
    finite = np.isfinite(ref["t"])
    nptest.assert_allclose(out["t"][finite], ref["t"][finite], rtol=RTOL)
    assert same(out["t"][~finite], ref["t"][~finite])
    for k in ("count_t", "count_region", "p_t", "p_region", "p_fwe_t", "p_fwe_region", "n_controls", "n_patients"):
        nptest.assert_array_equal(out[k], ref[k], err_msg=k)
    if name == "T2":
        # separated with both groups constant: +/-inf with the sign of A, under both variances
        assert out["t"][2] == math.inf and out["t"][3] == -math.inf and out["t"][0] == 2.0 and out["t"][1] == -2.0
        assert boundary_is_the_engineered_one(ex) >= 3
        thresholds = thresholds + (BELOW,)
    flags = env.bl.FLAG_MISSING | (env.bl.FLAG_WELCH if variance == "welch" else 0)
    for thr in thresholds:
        for tail in TAILS:
            want = ex.bits(thr, tail)
            assert np.array_equal(_bits_rows(env, b, bt, labels, thr, tail, flags), want[1:]), (thr, tail)
            net = env.bl.network_test(b, bt, thr, labels=labels, tail=tail, missing_data=True, variance=variance, ctx=env.ctx)
            netx = ex.network_test(thr, tail)
            for k in netx:
                if k not in ("t", "threshold", "tail"):
                    nptest.assert_array_equal(net[k], netx[k], err_msg=k)
    if name == "T2":
        assert ex.bits(BELOW, "both")[0, :2].all() and not ex.bits(2.0, "both")[0, :2].any()


# ---- repeatability, tensors, chunks --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variance", MR.VARIANCES)
def test_repeatable_and_device_tensors(env, variance, monkeypatch):
    shape = BR.SHAPES[4]
    (b, bt, labels) = data_of(shape)
    kw = dict(labels=labels, missing_data=True, variance=variance)
    one = env.bl.group_test(b, bt, ctx=env.ctx, **kw)
    two = env.bl.group_test(b, bt, ctx=env.ctx, **kw)
    other = env.bl.group_test(b, bt, **kw)                      # a context of its own
    dev = env.bl.group_test(env.torch.as_tensor(b, device="cuda"), bt, ctx=env.ctx, as_numpy=False, **kw)
    assert set(dev) == set(one)
    for k in one:
        assert same(one[k], two[k]) and same(one[k], other[k]), k
        assert isinstance(dev[k], env.torch.Tensor) and dev[k].is_cuda and same(dev[k].cpu().numpy(), one[k]), k
    net = env.bl.network_test(b, bt, THRESHOLD, ctx=env.ctx, **kw)
    again = env.bl.network_test(b, bt, THRESHOLD, ctx=env.ctx, **kw)
    other = env.bl.network_test(b, bt, THRESHOLD, **kw)
    devn = env.bl.network_test(b, env.torch.as_tensor(bt, device="cuda"), THRESHOLD, ctx=env.ctx, as_numpy=False, **kw)
    monkeypatch.setattr(env.bl, "_P_CHUNK", 16)
    chunked = env.bl.network_test(b, bt, THRESHOLD, ctx=env.ctx, **kw)
    assert set(devn) == set(net)
    for k in net:
        if isinstance(net[k], np.ndarray):
            assert same(net[k], again[k]) and same(net[k], other[k]) and same(net[k], chunked[k]), k
            assert isinstance(devn[k], env.torch.Tensor) and devn[k].is_cuda and same(devn[k].cpu().numpy(), net[k]), k
        else:
            assert net[k] == again[k] == chunked[k] == devn[k], k


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals(env):
    t = env.torch
    p = env.lib.dptr
    d = t.zeros(4096, dtype=t.float64, device="cuda")
    i = t.zeros(4096, dtype=t.int64, device="cuda")
    s = env.lib.stream_ptr()

    def group(b=d, C=3, H=4, U=4, P=1, flags=1, out=d):
        env.ctx.call("fcd_baseline_group_perm_opt", p(b), p(d), C, H, U, p(i), P, flags, p(out), p(d), p(d), p(d), p(i), p(i),
                     p(None), p(None), s)

    def bits(b=d, C=3, H=4, U=4, P=1, flags=1, out=i, thr=2.0, tail=0):
        env.ctx.call("fcd_baseline_network_bits_opt", p(b), p(d), C, H, U, p(i), P, thr, tail, flags, p(out), p(None), s)

    for call in (group, bits):
        for flags in (4, 8 | 1, -1):
            with pytest.raises(NotImplementedError, match="unknown flags"):
                call(flags=flags)
        for flags in (2, 3):
            with pytest.raises(ValueError, match="welch"):
                call(U=1, flags=flags)
            with pytest.raises(ValueError, match="welch"):
                call(H=1, flags=flags)
        for flags in (0, 1, 2, 3):
            with pytest.raises(ValueError, match="null"):
                call(b=None, flags=flags)
            with pytest.raises(ValueError, match="null"):
                call(out=None, flags=flags)
            with pytest.raises(NotImplementedError, match="at most 1024"):
                call(H=1000, U=25, flags=flags)
            with pytest.raises(ValueError, match="triangular"):
                call(C=5, flags=flags)
            with pytest.raises(ValueError, match=">= 1"):
                call(P=0, flags=flags)
        with pytest.raises(ValueError, match="needs 3"):
            call(H=1, U=1, flags=1)
    with pytest.raises(ValueError, match="threshold"):
        bits(thr=0.0)
    with pytest.raises(ValueError, match="tail"):
        bits(tail=3)
    # the context is still usable
    (b, bt, labels) = data_of(BR.SHAPES[0])
    out = env.bl.group_test(b, bt, labels=labels, missing_data=True, ctx=env.ctx)
    close(out["t"], group_ref(BR.SHAPES[0], "pooled")["t"], "t")


def test_flags_zero_is_the_call_without_options(env):
    (b, bt, labels) = BR.make_data(*BR.SHAPES[1])
    (C, H, U, P) = (b.shape[0], b.shape[1], bt.shape[1], labels.shape[0])
    t = env.torch
    p = env.lib.dptr
    base = env.bl.group_test(b, bt, labels=labels, ctx=env.ctx)
    (bd, btd, lab) = (t.as_tensor(b, device="cuda"), t.as_tensor(bt, device="cuda"), t.as_tensor(labels, device="cuda"))
    f = [t.empty(n, dtype=t.float64, device="cuda") for n in (C, 19, P, P)]
    k = [t.empty(n, dtype=t.int64, device="cuda") for n in (C, 19, C, C)]
    env.ctx.call("fcd_baseline_group_perm_opt", p(bd), p(btd), C, H, U, p(lab), P, 0, p(f[0]), p(f[1]), p(f[2]), p(f[3]), p(k[0]),
                 p(k[1]), p(k[2]), p(k[3]), env.lib.stream_ptr())
    for (got, key) in zip(f + k[:2], ("t", "region", "null_max_t", "null_max_region", "count_t", "count_region")):
        assert same(got.cpu().numpy(), base[key]), key
    assert (k[2].cpu().numpy() == H).all() and (k[3].cpu().numpy() == U).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_end_to_end_on_model_data(env):
    (N, H, U, P) = (16, 20, 12, 40)
    model = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(N, H, U, seed=5)
    order = env.pkg.util.upper_to_lower_edge_order(N)
    (b, bt) = (np.array(b, dtype=np.float64)[order], np.array(bt, dtype=np.float64)[order])
    rng = np.random.default_rng(6)
    b[rng.random(b.shape) < 0.05] = NAN
    bt[rng.random(bt.shape) < 0.05] = NAN
    labels = env.bl.draw_labels(P, H, U, seed=3)
    for variance in MR.VARIANCES:
        ref = MR.group_test(b, bt, labels, variance)
        assert gaps_group(ref, b, bt, labels) > GAP
        out = env.bl.group_test(b, bt, labels=labels, missing_data=True, variance=variance, ctx=env.ctx)
        check_group(out, ref, labels)
        assert (out["n_controls"] < H).any() and (out["n_patients"] < U).any() and np.isfinite(out["p_t"]).all()
    drawn = env.bl.group_test(b, bt, n_perm=P, seed=3, missing_data=True, variance="welch", ctx=env.ctx)
    assert all(same(drawn[k], out[k]) for k in out)
