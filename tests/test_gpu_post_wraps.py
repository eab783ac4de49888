"""
The post-fit kernels where their grids and chunk loops wrap (run with -m gpu on an MI355X).

The count, region-set and patient-group histograms, the connection posteriors, the shared, sessions and noise tables, the
membership fold, evidence tempering and the mean-field count law each cap their grid or walk a per-thread chunk loop.  The
files that test them use shapes at which, on 256 CUs, every one of those loops runs a single trip.  Here each shape is the
smallest that takes the loop into its second trip (or its last chunk), so that a wrong stride, a stale LDS tile, a barrier
missing on the second round or a row left unwritten shows.

`geometry()` restates the launch formulas of the .hip files; every named case lists the regimes it was picked for and
asserts them on the device that runs the suite (check_regimes) and, without a device, at 256 CUs
(test_regimes_of_the_named_shapes): a change of a cap that retires this coverage fails here.

Every output is prefilled before the call -- NaN for fp64, a known non-zero pattern for the uint32 histograms, which add --
so a row that was never written or added to is seen.  The bits of the chains beyond G in the last chain word are set on
purpose.  References and tolerances are those of the files that test the same kernels at small shapes.
"""
import ctypes as C
import itertools

import numpy as np
import numpy.testing as nptest
import pytest

import conn_posterior_ref as CP
import count_posterior_ref as R
import membership_ref as MR
import missing_data_ref as MD
import noise_ref as NR
import patient_groups_ref as PG
import region_sets_ref as RS
import sessions_ref as SR

pytestmark = pytest.mark.gpu

TAB = dict(rtol=1e-12, atol=1e-290)         # test_gpu_conn_posterior.py: the contraction kernel
SESS_POST = dict(rtol=1e-12, atol=1e-14)    # test_gpu_sessions.py: the sessions posterior
SUM = dict(rtol=1e-10, atol=1e-11)          # test_gpu_membership.py: sums of log-densities over edges
PB = dict(rtol=1e-12, atol=1e-300)          # test_gpu_count_posterior.py: the Poisson-binomial kernel


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib, gibbs, tables
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.gibbs, e.tables, e.O = torch, fcdiff_amd, _lib, gibbs, tables, O
    e.ctx = _lib.Context()
    e.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return e


def up(env, a):
    return None if a is None else env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def nan_tensor(env, *shape):
    return env.torch.full(shape, float("nan"), dtype=env.torch.float64, device="cuda")


def report(case, key, got, want, tol):
    """Prints the largest absolute and relative error of `got` against `want` beside the tolerance it is held to."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
        rel = d / np.abs(np.asarray(want, dtype=np.float64))
    d = d[np.isfinite(d)]
    rel = rel[np.isfinite(rel)]
    worst = (float(d.max()) if d.size else 0.0, float(rel.max()) if rel.size else 0.0)
    print("%s %s: max abs err %.3g, max rel err %.3g (rtol %.1g, atol %.3g)" % (case, key, worst[0], worst[1], tol["rtol"], tol["atol"]))


# ------------------------------------------------------------------------------------------------
# launch geometry
# ------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _tri(n):
    return n * (n - 1) // 2


def _grid_stride(n, per_block, cap):
    """(blocks, trips, units past the first trip) of a grid-stride loop over n units, per_block a block and trip."""
    blocks = min(_cdiv(n, per_block), cap)
    return blocks, _cdiv(n, per_block * blocks), max(0, n - per_block * blocks)


def geometry(what, n_cu, **s):
    """
    Blocks and loop trips of one launch on a device with n_cu CUs, restated from the .hip files:
      "count tally"          fcd_count.hip, fcd_count_tally_launch: count_sums_kernel, a workgroup per chain word, at most 8 CU
      "region-set tally"     fcd_region_sets.hip: region_set_sums_kernel over the pairs (set, word), at most 8 CU workgroups
      "patient-group tally"  fcd_patient_groups.hip: patient_group_sums_kernel over the pairs (row, word), at most 8 CU
      "posterior"            fcd_post.hip / fcd_lik_sessions.hip: posterior_kernel and posterior_sessions_kernel, an item per
                             thread, at most 64 CU blocks of 256
      "shared table"         fcd_lik_shared.hip / fcd_lik_sessions.hip: a group of 16, 32 or 64 lanes per edge by U, 256 / group
                             edges per block and pass, at most 16 CU blocks (the record forms: blocks of several tiles)
      "noise records"        fcd_lik_sessions.hip, noise_records: a record per thread, at most 8 CU blocks of 256
      "member fold"          fcd_member.hip: member_fold, an output per thread, at most 8 CU blocks of 256
      "temper"               fcd_evidence.hip: evidence_temper_kernel, at most 16 CU blocks of 256 sized by the largest table;
                             pairs of doubles where source and destination are 16-byte aligned, then a scalar tail
      "count law"            fcd_count.hip: poisson_binomial_kernel, a workgroup of 256 per row, bin k = tid + 256 t, t < 16,
                             the sites in chunks of 256
    """
    g = dict(s)
    if what == "count tally":
        GW = _cdiv(s["G"], 64)
        (blocks, trips, past) = _grid_stride(GW, 1, 8 * n_cu)
        tn = min(4096 // s["U"], s["Nreg"])
        g.update(GW=GW, tail=s["G"] % 64, blocks=blocks, trips=trips, past=past, tiles=_cdiv(s["Nreg"], tn))
    elif what in ("region-set tally", "patient-group tally"):
        GW = _cdiv(s["G"], 64)
        rows = s["J"] if what == "region-set tally" else s["R"]
        (blocks, trips, past) = _grid_stride(rows * GW, 1, 8 * n_cu)
        g.update(GW=GW, tail=s["G"] % 64, pairs=rows * GW, blocks=blocks, trips=trips, past=past, chunks=_cdiv(s["U"], 64))
    elif what == "posterior":
        items = _tri(s["Nreg"]) * s["U"]
        (blocks, trips, past) = _grid_stride(items, 256, 64 * n_cu)
        g.update(items=items, blocks=blocks, trips=trips, past=past)
    elif what == "shared table":
        Cn = _tri(s["Nreg"])
        group = 16 if s["U"] <= 16 else (32 if s["U"] <= 32 else 64)
        epb = 256 // group
        # the record forms keep U K records of 48 bytes in LDS up to 768 of them and give a block a tile per 4096 bytes copied
        n_rec = max(s.get("H", 1), s["U"] * s.get("K", 1))
        per_block = max(1, _cdiv(s["U"] * s.get("K", 1) * 48, 4096)) if s.get("noise") and n_rec <= 768 else 1
        n_l = min(_cdiv(_cdiv(Cn, epb), per_block), 16 * n_cu)
        g.update(C=Cn, group=group, epb=epb, per_block=per_block, blocks=n_l, at_cap=n_l == 16 * n_cu,
                 trips=_cdiv(Cn, n_l * epb), past=max(0, Cn - n_l * epb))
    elif what == "noise records":
        n = s["H_b"] + s["U"] * s["K"]
        (blocks, trips, past) = _grid_stride(n, 256, 8 * n_cu)
        g.update(records=n, blocks=blocks, trips=trips, past=past)
    elif what == "member fold":
        n = s["U"] * s["G"]
        (blocks, trips, past) = _grid_stride(n, 256, 8 * n_cu)
        g.update(outputs=n, blocks=blocks, trips=trips, past=past)
    elif what == "temper":
        blocks = max(1, min(_cdiv(s["largest"] // 2, 256), 16 * n_cu))
        n_pairs = s["n"] // 2 if s["aligned"] else 0
        n_scalar = s["n"] - 2 * n_pairs
        g.update(blocks=blocks, pair_trips=_cdiv(n_pairs, 256 * blocks), scalar_elements=n_scalar,
                 scalar_trips=_cdiv(n_scalar, 256 * blocks))
    elif what == "count law":
        L = max(s["Nreg"], s["U"])
        g.update(L=L, top_bin_slot=L // 256, site_chunks=_cdiv(L, 256), accepted=L <= 256 * 16 - 1)
    else:
        raise KeyError(what)
    return g


# the regimes a case is chosen for: name -> test on geometry()
REGIMES = {
    "second trip": lambda g: g["trips"] >= 2 and g["past"] > 0,
    "second trip of a few units": lambda g: g["trips"] == 2 and 0 < g["past"] <= 64,
    "last word holds one chain": lambda g: g["tail"] == 1,
    "partial last word": lambda g: g["tail"] != 0,
    "one trip": lambda g: g["trips"] == 1,
    "two patient chunks": lambda g: g["chunks"] == 2,
    "every bit plane": lambda g: g["Nreg"] == 1023,
    "several row tiles": lambda g: g["tiles"] >= 2,
    "512 patients": lambda g: g["U"] == 512,
    "lanes 16 at the cap": lambda g: g["group"] == 16 and g["at_cap"] and g["trips"] == 2,
    "lanes 32 at the cap": lambda g: g["group"] == 32 and g["at_cap"] and g["trips"] == 2,
    "lanes 64 at the cap": lambda g: g["group"] == 64 and g["at_cap"] and g["trips"] == 2,
    "a tile per block": lambda g: g["per_block"] == 1,
    "pair loop wraps, scalar tail": lambda g: g["pair_trips"] >= 2 and g["scalar_elements"] == 1,
    "scalar loop only, wraps": lambda g: g["pair_trips"] == 0 and g["scalar_trips"] >= 2,
    "bin slot 15": lambda g: g["top_bin_slot"] == 15 and g["accepted"],
    "bin slots and site chunks 0 to 2": lambda g: g["top_bin_slot"] == 2 and g["site_chunks"] == 3,
    "refused": lambda g: not g["accepted"],
}

# the 1024 sets (the cap): the non-empty subsets with bit masks 1 .. 1024 over the regions 0 .. 10
SETS_1024 = [[n for n in range(11) if (mask >> n) & 1] for mask in range(1, 1025)]

# case -> (launch, shape, regimes)
CASES = {
    "count 2x1x131137": ("count tally", dict(Nreg=2, U=1, G=131137), ("second trip", "last word holds one chain")),
    "sets 1024 12x2x130": ("region-set tally", dict(J=1024, Nreg=12, U=2, G=130), ("second trip", "partial last word")),
    "groups 700x3x192": ("patient-group tally", dict(R=700, Nreg=700, U=3, G=192), ("second trip",)),
    "groups 12+1024x70x130": ("patient-group tally", dict(R=12 + 1024, Nreg=12, U=70, G=130),
                              ("second trip", "two patient chunks", "partial last word")),
    "count 1023x2x70": ("count tally", dict(Nreg=1023, U=2, G=70), ("one trip", "every bit plane", "partial last word")),
    "sets 1 1023x2x70": ("region-set tally", dict(J=1, Nreg=1023, U=2, G=70), ("one trip", "every bit plane")),
    "count 2x512x70": ("count tally", dict(Nreg=2, U=512, G=70), ("one trip", "512 patients", "partial last word")),
    "groups 2x512x70": ("patient-group tally", dict(R=2, Nreg=2, U=512, G=70), ("one trip", "512 patients")),
    "posterior 46x4100": ("posterior", dict(Nreg=46, U=4100), ("second trip",)),
    "shared 363x1": ("shared table", dict(Nreg=363, U=1, H=1, K=2, noise=True), ("lanes 16 at the cap", "a tile per block")),
    "shared 257x17": ("shared table", dict(Nreg=257, U=17, H=1, K=2, noise=True), ("lanes 32 at the cap", "a tile per block")),
    "shared 182x33": ("shared table", dict(Nreg=182, U=33, H=1, K=2, noise=True), ("lanes 64 at the cap", "a tile per block")),
    "records bt 524300": ("noise records", dict(H_b=0, U=524300, K=1), ("second trip of a few units",)),
    "records b 524300": ("noise records", dict(H_b=524300, U=1, K=1), ("second trip of a few units",)),
    "fold 4x70x7552": ("member fold", dict(U=70, G=7552), ("second trip",)),
    "temper aligned": ("temper", dict(n=2500001, aligned=True, largest=2500001), ("pair loop wraps, scalar tail",)),
    "temper odd start": ("temper", dict(n=2500001, aligned=False, largest=2500001), ("scalar loop only, wraps",)),
    "law 4095x2": ("count law", dict(Nreg=4095, U=2), ("bin slot 15",)),
    "law 600x3": ("count law", dict(Nreg=600, U=3), ("bin slots and site chunks 0 to 2",)),
    "law 4096x2": ("count law", dict(Nreg=4096, U=2), ("refused",)),
}


def check_regimes(n_cu, case):
    (what, shape, regimes) = CASES[case]
    g = geometry(what, n_cu, **shape)
    for r in regimes:
        assert REGIMES[r](g), "case %r (%s) is no longer in regime %r at %d CUs: %s" % (case, what, r, n_cu, g)
    return g


def test_regimes_of_the_named_shapes():
    """Every case is in its regimes on an MI355X (256 CUs), whatever device runs the suite; the figures they were chosen from."""
    for case in CASES:
        check_regimes(256, case)
    g = check_regimes(256, "count 2x1x131137")
    assert (g["GW"], g["blocks"], g["trips"], g["past"]) == (2050, 2048, 2, 2)
    g = check_regimes(256, "sets 1024 12x2x130")
    assert (g["pairs"], g["blocks"], g["trips"]) == (3072, 2048, 2)
    assert len(SETS_1024) == 1024 and max(len(s) for s in SETS_1024) == 10 and SETS_1024[-1] == [10]
    assert check_regimes(256, "groups 700x3x192")["pairs"] == 2100
    assert check_regimes(256, "groups 12+1024x70x130")["pairs"] == 3108
    g = check_regimes(256, "posterior 46x4100")
    assert (g["items"], g["blocks"], g["past"]) == (4243500, 16384, 49196)
    for (case, Cn, covered) in (("shared 363x1", 65703, 65536), ("shared 257x17", 32896, 32768), ("shared 182x33", 16471, 16384)):
        g = check_regimes(256, case)
        assert (g["C"], g["blocks"] * g["epb"]) == (Cn, covered)
    assert check_regimes(256, "records bt 524300")["past"] == 12 and check_regimes(256, "records b 524300")["past"] == 13
    g = check_regimes(256, "fold 4x70x7552")
    assert (g["outputs"], g["blocks"], g["past"]) == (528640, 2048, 4352)
    g = check_regimes(256, "temper aligned")
    assert (g["blocks"], g["pair_trips"], g["scalar_trips"]) == (4096, 2, 1)
    assert check_regimes(256, "temper odd start")["scalar_trips"] == 3
    # what the other files reach today: one trip of the same loops
    assert geometry("count tally", 256, Nreg=400, U=500, G=130)["trips"] == 1
    assert geometry("posterior", 256, Nreg=200, U=50)["trips"] == 1
    assert geometry("member fold", 256, U=70, G=1100)["trips"] == 1


# ------------------------------------------------------------------------------------------------
# histogram tallies
# ------------------------------------------------------------------------------------------------
STATE_KINDS = ("random", "all ones", "all zeros", "last word only")


def planted_r(Nreg, U, G, kind, seed):
    """r (G, Nreg, U) uint8."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (rng.random((G, Nreg, U)) < rng.uniform(0.05, 0.95, (1, Nreg, 1))).astype(np.uint8)
    if kind == "all ones":
        return np.ones((G, Nreg, U), dtype=np.uint8)
    r = np.zeros((G, Nreg, U), dtype=np.uint8)
    if kind == "last word only":
        g0 = (G - 1) // 64 * 64
        r[g0:] = (rng.random((G - g0, Nreg, U)) < 0.5).astype(np.uint8)
        r[G - 1, 0, 0] = 1
    return r


def pack_r(env, r):
    """r_bits (GW, Nreg, U) of r (G, Nreg, U), packed on the host (bit j of word w: chain 64 w + j); the bits of the chains
    beyond G in the last word are set on purpose and must never be counted."""
    (G, N, U) = r.shape
    GW = _cdiv(G, 64)
    rp = np.zeros((GW * 64, N, U), dtype=np.uint64)
    rp[:G] = r
    rp[G:] = 1
    shifts = np.arange(64, dtype=np.uint64)[None, :, None, None]
    bits = np.bitwise_or.reduce(rp.reshape(GW, 64, N, U) << shifts, axis=1)
    return up(env, bits.view(np.int64))


def pattern(env, *shape):
    """(device int32 tensor holding a known non-zero uint32 pattern, some above 2^31; the pattern as int64)."""
    n = int(np.prod(shape))
    base = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x9E3779B9)) % np.uint64(1 << 32)).astype(np.int64)
    base[base == 0] = 1
    base = base.reshape(shape)
    return up(env, base.astype(np.uint32).view(np.int32)), base


def added(t, base):
    """What was added to the uint32 buffer `t` on top of `base`, modulo 2^32, as int64."""
    return (t.cpu().numpy().view(np.uint32).astype(np.int64) - base) % (1 << 32)


def tally_twice(env, call, buffers, wants, what):
    """`call()` adds to the prefilled `buffers` [(tensor, base)]: after one call base + want, after two base + 2 want."""
    for times in (1, 2):
        call()
        for ((t, base), want, name) in zip(buffers, wants, what):
            nptest.assert_array_equal(added(t, base), times * want, err_msg="%s after %d call(s)" % (name, times))
    env.ctx.check_device()


def count_tally(env, r, N, U, G):
    r_bits = pack_r(env, r)
    bufs = [pattern(env, U, N + 1), pattern(env, N, U + 1)]
    tally_twice(env, lambda: env.ctx.call("fcd_gibbs_count_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(bufs[0][0]),
                                          env.lib.dptr(bufs[1][0]), env.lib.stream_ptr()),
                bufs, R.histograms(r), ("hist_patient", "hist_region"))


def i32p(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.c_void_p)


def send_sets(env, sets, N):
    """The region sets to the context through the C entry (None: none); (J, S_max)."""
    env.ctx.region_sets_owner = None
    if sets is None:
        env.ctx.call("fcd_region_sets_set", None, None, 0)
        return 0, 0
    (_names, offsets, members) = env.gibbs.region_sets_csr(sets, N)
    env.ctx.call("fcd_region_sets_set", i32p(offsets), i32p(members), len(offsets) - 1)
    return len(offsets) - 1, int(np.diff(offsets).max())


def send_groups(env, groups, contrasts, U, with_sets):
    """The patient groups to the context through the C entry; (J, Umax, joint bins of all contrasts)."""
    (names, offsets, members) = env.gibbs.patient_groups_csr(groups, U)
    (pairs, bins) = env.gibbs.patient_group_contrasts(contrasts, names, offsets, members)
    env.ctx.patient_groups_owner = None
    env.ctx.call("fcd_patient_groups_set", i32p(offsets), i32p(members), len(names), i32p(pairs) if len(pairs) else None,
                 len(pairs), 1 if with_sets else 0)
    return len(names), int(np.diff(offsets).max()), int(bins[-1])


def clear_sets_and_groups(env):
    env.ctx.patient_groups_owner = None
    env.ctx.call("fcd_patient_groups_set", None, None, 0, None, 0, 0)
    send_sets(env, None, 0)


def region_set_tally(env, r, sets, N, U, G):
    (J, s_max) = send_sets(env, sets, N)
    r_bits = pack_r(env, r)
    bufs = [pattern(env, J, U, s_max + 1), pattern(env, J, U + 1)]
    try:
        tally_twice(env, lambda: env.ctx.call("fcd_gibbs_region_set_tally", env.lib.dptr(r_bits), N, U, G, env.lib.dptr(bufs[0][0]),
                                              env.lib.dptr(bufs[1][0]), env.lib.stream_ptr()),
                    bufs, RS.histograms(r, sets), ("hist_set", "hist_prev"))
    finally:
        clear_sets_and_groups(env)


def patient_group_tally(env, r, groups, contrasts, sets, N, U, G):
    (JS, _s) = send_sets(env, sets, N)
    rows = N + JS
    try:
        (J, umax, bins) = send_groups(env, groups, contrasts, U, sets is not None)
        r_bits = pack_r(env, r)
        (want_g, want_j) = PG.histograms(r, groups, contrasts or [], sets)
        want_j = PG.flat_joint(want_j)
        if not contrasts:
            want_j = np.zeros(1, dtype=np.int64)             # the placeholder word: left alone
        bufs = [pattern(env, J, rows, umax + 1), pattern(env, max(1, rows * bins))]
        assert want_g.shape == (J, rows, umax + 1) and want_j.shape == (max(1, rows * bins),)
        tally_twice(env, lambda: env.ctx.call("fcd_gibbs_patient_group_tally", env.lib.dptr(r_bits), N, U, G,
                                              env.lib.dptr(bufs[0][0]), env.lib.dptr(bufs[1][0]), env.lib.stream_ptr()),
                    bufs, (want_g, want_j), ("hist_group", "hist_joint"))
    finally:
        clear_sets_and_groups(env)


@pytest.mark.parametrize("kind", STATE_KINDS)
def test_count_tally_past_the_first_trip(env, kind):
    """fcd_gibbs_count_tally with 2050 chain words: words 2048 and 2049 are the second trip, the last holds one chain."""
    g = check_regimes(env.n_cu, "count 2x1x131137")
    (N, U, G) = (g["Nreg"], g["U"], g["G"])
    count_tally(env, planted_r(N, U, G, kind, seed=11), N, U, G)


@pytest.mark.parametrize("kind", STATE_KINDS)
def test_region_set_tally_past_the_first_trip(env, kind):
    """fcd_gibbs_region_set_tally with the 1024 sets over three chain words: 3072 pairs (set, word)."""
    g = check_regimes(env.n_cu, "sets 1024 12x2x130")
    (N, U, G) = (g["Nreg"], g["U"], g["G"])
    region_set_tally(env, planted_r(N, U, G, kind, seed=12), SETS_1024, N, U, G)


@pytest.mark.parametrize("kind", STATE_KINDS)
@pytest.mark.parametrize("case", ["groups 700x3x192", "groups 12+1024x70x130"])
def test_patient_group_tally_past_the_first_trip(env, case, kind):
    """fcd_gibbs_patient_group_tally over 2100 pairs (row, word) of region rows, and over 3108 with the 1024 sets as rows and a
    second 64-patient chunk; the groups {0}, {1, 2}, all patients (and {62 .. 65}), the contrast {0} against {1, 2}."""
    g = check_regimes(env.n_cu, case)
    (N, U, G) = (g["Nreg"], g["U"], g["G"])
    groups = [[0], [1, 2], list(range(U))] + ([[62, 63, 64, 65]] if U == 70 else [])
    sets = SETS_1024 if g["R"] > N else None
    patient_group_tally(env, planted_r(N, U, G, kind, seed=13), groups, [(0, 1)], sets, N, U, G)


SATURATED = ("all ones", "all ones but region 0", "511 per column", "512 per column")


def saturated_r(N, U, G, kind):
    """r (G, N, U) with the same count in every column of every chain: 1023, 1022, 511 or 512 (the carry into the top plane, in
    every chain at the same row; patient 1 takes its rows from the other end)."""
    r = np.zeros((G, N, U), dtype=np.uint8)
    if kind == "all ones":
        r[:] = 1
    elif kind == "all ones but region 0":
        r[:, 1:] = 1
    else:
        k = 511 if kind.startswith("511") else 512
        r[:, :k, 0::2] = 1
        r[:, N - k:, 1::2] = 1
    return r


@pytest.mark.parametrize("kind", SATURATED)
def test_bit_sliced_counters_saturated(env, kind):
    """The ten bit planes of count_sums_kernel and region_set_sums_kernel (one set of all 1023 regions) at the counts 1023
    (the top bin), 1022, 511 and 512 in every chain at once."""
    g = check_regimes(env.n_cu, "count 1023x2x70")
    check_regimes(env.n_cu, "sets 1 1023x2x70")
    (N, U, G) = (g["Nreg"], g["U"], g["G"])
    r = saturated_r(N, U, G, kind)
    k = {"all ones": 1023, "all ones but region 0": 1022, "511 per column": 511, "512 per column": 512}[kind]
    assert (r.sum(axis=1) == k).all()
    assert R.histograms(r)[0][:, k].tolist() == [G] * U
    count_tally(env, r, N, U, G)
    region_set_tally(env, r, [list(range(N))], N, U, G)


def test_tallies_with_512_patients_all_anomalous(env):
    """Region count 512 (the top bin of hist_region and of the group of all patients) in every chain."""
    g = check_regimes(env.n_cu, "count 2x512x70")
    check_regimes(env.n_cu, "groups 2x512x70")
    (N, U, G) = (g["Nreg"], g["U"], g["G"])
    r = np.ones((G, N, U), dtype=np.uint8)
    assert R.histograms(r)[1][:, 512].tolist() == [G, G]
    count_tally(env, r, N, U, G)
    patient_group_tally(env, r, [list(range(U))], None, None, N, U, G)


# ------------------------------------------------------------------------------------------------
# connection posteriors
# ------------------------------------------------------------------------------------------------
EDGE_CHUNK = 69             # edges per piece of a host reference (1035 = 15 x 69): (69 x 4100 x 27) doubles at most


def in_edge_chunks(Cn, fn):
    """fn(slice of edges) -> dict of arrays, evaluated in pieces and joined along the edges."""
    parts = [fn(slice(c0, min(Cn, c0 + EDGE_CHUNK))) for c0 in range(0, Cn, EDGE_CHUNK)]
    return {k: np.concatenate([p[k] for p in parts], axis=0) for k in parts[0]}


def vb_weights_of(lq_F, lq_R, sl):
    """conn_posterior_ref.vb_weights for the edges of `sl` alone."""
    q_F = np.exp(lq_F)[sl, 0, :]
    q_R = np.exp(lq_R)
    (n, m) = CP.endpoints(q_R.shape[0])
    (n, m) = (n[sl], m[sl])
    w = np.stack([q_R[n, :, 0] * q_R[m, :, 0], q_R[n, :, 1] * q_R[m, :, 1],
                  q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]], axis=2)
    return q_F[:, None, :, None] * w[:, :, None, :]


def contract_with_missing(W, bt, theta, missing):
    """conn_posterior_ref.contract; with `missing` an item whose bt is NaN gets the prior law (missing_data_ref.contract_prior)."""
    nan = np.isnan(bt)
    if not (missing and nan.any()):
        return CP.contract(W, bt, theta)
    out = CP.contract(W, np.where(nan, 0.0, bt), theta)
    prior = MD.contract_prior(W[nan], theta)
    for key in out:
        out[key][nan] = prior[key]
    return out


def enumerate_law_arrays(eta, epsilon, like):
    """missing_data_ref.enumerate_law for an array of items, like (3j, ...): the same enumeration of (T, F~) given (k, l) in the
    same order, every step on whole arrays.  (pT (3k, 3l, ...), pF (3k, 3l, 3j, ...), pch (3k, 3l, ...))."""
    pT = (0.0, 1.0, eta)
    shp = like.shape[1:]
    M = np.zeros((3, 3) + shp)
    t1 = np.zeros((3, 3) + shp)
    fj = np.zeros((3, 3, 3) + shp)
    for (k, l, t, j) in itertools.product(range(3), range(3), range(2), range(3)):
        p_t = pT[l] if t == 1 else 1.0 - pT[l]
        keep = epsilon if t == 1 else 1.0 - epsilon
        p_j = keep if j == k else (1.0 - keep) / 2.0
        w = p_t * p_j * like[j]
        M[k, l] += w
        t1[k, l] += w * t
        fj[k, l, j] += w
    pF = fj / M[:, :, None]
    pch = np.stack([sum(pF[k, :, j] for j in range(3) if j != k) for k in range(3)])
    return t1 / M, pF, pch


def enumerated_posterior_arrays(W, a, theta):
    """noise_ref.enumerated_posterior / test_gpu_sessions.enumerated_posterior on whole arrays: a (C, U, 3) the session log
    sums of the items, W (C, U, 3, 3) their weights."""
    like = np.ascontiguousarray(np.moveaxis(np.exp(a - a.max(axis=2, keepdims=True)), 2, 0))
    (pT, pF, pch) = enumerate_law_arrays(theta[1], theta[2], like)
    w = np.ascontiguousarray(np.moveaxis(W / W.sum(axis=(2, 3), keepdims=True), (2, 3), (0, 1)))
    return {"p_T": (w * pT).sum(axis=(0, 1)), "p_F_tilde": np.moveaxis((w[:, :, None] * pF).sum(axis=(0, 1)), 0, 2),
            "p_changed": (w * pch).sum(axis=(0, 1))}


@pytest.fixture(scope="module")
def post_case(env):
    """Data of the posterior cases, made once and never changed: bt (C, U, 2) with and without NaN, weights, variances."""
    g = check_regimes(env.n_cu, "posterior 46x4100")
    (N, U) = (g["Nreg"], g["U"])
    Cn = _tri(N)
    m = env.pkg.UnsharedRegionModel()
    m.sigma = np.array([0.1, 0.12, 0.15])
    (_r, _t, _f, _ft, _b, bt) = m.sample_fast(N, 1, U, seed=N + U, sessions=2)
    rng = np.random.default_rng(N * U)
    btn = bt.copy()
    btn[rng.random(bt.shape) < 0.05] = np.nan
    first_past = g["blocks"] * 256                                                      # first item of the second trip
    all_nan = [(1, 0), ((first_past - 1) // U, (first_past - 1) % U), (first_past // U, first_past % U), (Cn - 1, U - 1),
               (Cn - 3, 17)]
    for (c, u) in all_nan:
        btn[c, u, :] = np.nan
    one_nan = [(0, 5), (Cn - 1, 0), (Cn - 2, U - 1)]
    for (c, u) in one_nan:
        btn[c, u, :] = [np.nan, 0.05]
    assert all(c * U + u >= first_past for (c, u) in all_nan[2:] + one_nan[1:]) and all_nan[1][0] * U + all_nan[1][1] < first_past
    lq_F = np.log(rng.dirichlet(np.ones(3), Cn))[:, None, :]
    q1 = rng.uniform(0, 1, (N, U))
    q1[0] = 0.0                             # region 0 typical for sure: some weight only in l = 0 / 2
    with np.errstate(divide="ignore"):
        lq_R = np.log(np.stack([1 - q1, q1], axis=2))
    vbt = rng.uniform(0, 0.02, (U, 2))
    vbt[rng.random((U, 2)) < 0.25] = 0.0
    vbt[U - 1] = [0.0, 0.019]
    # the 2-D cases: the first session, with densities that underflow as in test_contraction_kernel_against_numpy
    bt2 = bt[:, :, 0].copy()
    bt2.reshape(-1)[::7] = rng.choice([-40.0, 40.0, -1.0, 1.0, 1e3], size=bt2.reshape(-1)[::7].shape)
    bt2n = np.where(np.isnan(btn[:, :, 0]), np.nan, bt2)

    class P:
        pass
    p = P()
    (p.N, p.U, p.C, p.m, p.theta, p.bt, p.btn, p.lq_F, p.lq_R, p.vbt, p.g) = (N, U, Cn, m, m.theta(), bt, btn, lq_F, lq_R, vbt, g)
    (p.bt2, p.bt2n, p.first_past) = (bt2, bt2n, first_past)
    p.planted = all_nan + one_nan
    return p


def run_posterior(env, p, bt, missing, K=None, var=None, counts=None):
    """The C entry for bt (C, U) or (C, U, K) on NaN-prefilled outputs: {p_T, p_F_tilde, p_changed} on the host."""
    out = (nan_tensor(env, p.C, p.U), nan_tensor(env, p.C, p.U, 3), nan_tensor(env, p.C, p.U))
    (th, _th) = env.lib.dbl_array(p.theta)
    (bt_d, lq_F, lq_R) = (up(env, bt), up(env, p.lq_F), up(env, p.lq_R))
    P = env.lib.dptr
    weights = (P(counts), P(None), P(None)) if counts is not None else (P(None), P(lq_F), P(lq_R))
    flags = env.lib.FCD_DATA_NAN_MISSING if missing else 0
    tail = weights + (flags, P(out[0]), P(out[1]), P(out[2]), env.lib.stream_ptr())
    if var is not None:
        var_d = up(env, var)
        env.ctx.call("fcd_conn_posterior_noise", P(bt_d), p.N, p.U, K, th, P(var_d), *tail)
    elif K is not None:
        env.ctx.call("fcd_conn_posterior_sessions", P(bt_d), p.N, p.U, K, th, *tail)
    else:
        env.ctx.call("fcd_conn_posterior_ex", P(bt_d), p.N, p.U, th, *tail)
    got = {"p_T": out[0].cpu().numpy(), "p_F_tilde": out[1].cpu().numpy(), "p_changed": out[2].cpu().numpy()}
    env.ctx.check_device()
    return got


def check_posterior(case, got, want, tol):
    for key in ("p_T", "p_F_tilde", "p_changed"):
        assert np.all(np.isfinite(got[key])), "%s: %s holds the sentinel or another non-number at %s" % (
            case, key, np.argwhere(~np.isfinite(got[key]))[:4].tolist())
        report(case, key, got[key], want[key], tol)
        nptest.assert_allclose(got[key], want[key], err_msg=key, **tol)
    nptest.assert_allclose(got["p_F_tilde"].sum(axis=2), 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("weights,missing", [("lq", False), ("lq", True), ("counts", True)])
def test_contraction_kernel_past_the_first_trip(env, post_case, weights, missing):
    """fcd_conn_posterior_ex on 4 243 500 items (the last 49 196 are the second trip) against conn_posterior_ref.contract:
    the mean-field weights with and without FCD_DATA_NAN_MISSING, and once counts with zeros among them."""
    p = post_case
    bt = p.bt2n if missing else p.bt2
    if weights == "counts":
        rng = np.random.default_rng(5)
        cnt = rng.integers(0, 50, (p.C, p.U, 3, 3), dtype=np.uint32)
        cnt[rng.random((p.C, p.U, 3, 3)) < 0.4] = 0
        cnt[:, :, 0, 0] += 1
        got = run_posterior(env, p, bt, missing, counts=up(env, cnt.view(np.int32)))
        want = in_edge_chunks(p.C, lambda sl: contract_with_missing(cnt[sl].astype(np.float64), bt[sl], p.theta, missing))
    else:
        got = run_posterior(env, p, bt, missing)
        want = in_edge_chunks(p.C, lambda sl: contract_with_missing(vb_weights_of(p.lq_F, p.lq_R, sl), bt[sl], p.theta, missing))
    check_posterior("posterior_kernel %s%s" % (weights, " missing" if missing else ""), got, want, TAB)
    if missing:
        assert all(np.isnan(bt[c, u]) for (c, u) in p.planted[:5])


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("noise", [False, True], ids=["sessions", "noise"])
def test_sessions_posteriors_past_the_first_trip(env, post_case, noise, missing):
    """fcd_conn_posterior_sessions (the sigma terms) and fcd_conn_posterior_noise (records from global memory) with K = 2 and
    the mean-field weights, against the enumeration of the files that test them: on whole arrays for every item, and the
    looped reference itself on the planted items and their neighbours in both trips."""
    p = post_case
    bt = p.btn if missing else p.bt
    var = p.vbt if noise else None
    got = run_posterior(env, p, bt, missing, K=2, var=var)
    (mu, sigma) = (p.theta[6:9], p.theta[9:12])

    def log_sums(x, v):
        return NR.session_log_sums(x, mu, sigma, v, missing)[0] if noise else SR.session_log_sums(x, mu, sigma, missing)[0]
    tol = NR.tolerance(bt, mu, sigma, var, missing=missing) if noise else SESS_POST
    want = in_edge_chunks(p.C, lambda sl: enumerated_posterior_arrays(vb_weights_of(p.lq_F, p.lq_R, sl), log_sums(bt[sl], var), p.theta))
    case = "posterior_sessions_kernel %s%s" % ("global records" if noise else "sigma", " missing" if missing else "")
    check_posterior(case, got, want, tol)
    # the looped reference on a few edges and patients of both trips
    for c in sorted(set(c for (c, _u) in p.planted)):
        us = sorted(set([u for (cc, u) in p.planted if cc == c] + [0, 1, 2, 3, 4, 5, 6, p.U - 2, p.U - 1]))
        W = vb_weights_of(p.lq_F, p.lq_R, slice(c, c + 1))[:, us]
        x = bt[c:c + 1][:, us]
        if noise:
            loop = NR.enumerated_posterior(W, x, p.theta, var[us], missing)
        else:
            import test_gpu_sessions as TS
            loop = TS.enumerated_posterior(W, x, p.theta, missing)
        for key in loop:
            nptest.assert_allclose(want[key][c:c + 1][:, us], loop[key], rtol=1e-14, atol=1e-16, err_msg="array form: " + key)
            nptest.assert_allclose(got[key][c:c + 1][:, us], loop[key], err_msg=key, **tol)
    if missing:
        prior = MD.contract_prior(vb_weights_of(p.lq_F, p.lq_R, slice(p.C - 1, p.C))[0, p.U - 1], p.theta)
        nptest.assert_allclose(got["p_T"][p.C - 1, p.U - 1], prior["p_T"], rtol=1e-13, atol=1e-15)


# ------------------------------------------------------------------------------------------------
# shared tables
# ------------------------------------------------------------------------------------------------
MISS = 1                    # FCD_DATA_NAN_MISSING (asserted against the library in build_tables)


def build_tables(env, m, b, bt, shared, flags=0, count=False, noise=None, lpB=False):
    """tables.build on host arrays into NaN-prefilled outputs: (S_B, lM, (n_b, n_bt) or None[, lpB])."""
    assert MISS == env.lib.FCD_DATA_NAN_MISSING
    (Cn, H) = b.shape
    U = bt.shape[1]
    S_B = nan_tensor(env, Cn, 3)
    lM = nan_tensor(env, Cn, 1 if shared else U, 3, 3)
    lp = nan_tensor(env, Cn, H, 3) if lpB else None
    n = env.torch.full((2,), -7, dtype=env.torch.int64, device="cuda") if count else None
    kw = {} if noise is None else {"noise": (up(env, noise[0]), up(env, noise[1]))}
    env.tables.build(env.ctx, up(env, b), up(env, bt), m.theta(), flags, shared=shared, S_B=S_B, lM=lM, lpB=lp, n_missing=n, **kw)
    out = (S_B.cpu().numpy(), lM.cpu().numpy(), None if n is None else tuple(n.cpu().tolist()))
    env.ctx.check_device()
    return out + ((lp.cpu().numpy(),) if lpB else ())


def table_reference(env, m, b, bt, form, noise, missing):
    """(S_B, lM (C, U, 3, 3), tolerance of the patient sum) of the form's own reference."""
    if form == "2d":
        obs = ~np.isnan(bt)
        (lpB, _pBt, lM) = env.O.lik_tables(np.where(np.isnan(b), 0.0, b), np.where(obs, bt, 0.0), m.mu, m.sigma, m.eta, m.epsilon)
        lM = lM * obs[:, :, None, None]
        S_B = (lpB * ~np.isnan(b)[:, :, None]).sum(axis=1)
        return S_B, lM, SR.tolerance(bt[:, :, None], m.mu, m.sigma, missing=missing, scale=3)
    if form == "sessions":
        (S_B, lM) = SR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, missing=missing)
        return S_B, lM, SR.tolerance(bt, m.mu, m.sigma, missing=missing, scale=3)
    (S_B, lM) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, noise[0], noise[1], missing=missing)
    return S_B, lM, NR.tolerance(bt, m.mu, m.sigma, noise[1], missing=missing, scale=3)


@pytest.mark.parametrize("form", ["2d", "sessions", "noise"])
@pytest.mark.parametrize("case", ["shared 363x1", "shared 257x17", "shared 182x33"])
def test_shared_tables_past_the_first_trip(env, case, form):
    """
    tables.build(shared=True) with C just past what 16 CU blocks cover in one pass, one case per lane-group width: the 2-D bt
    (lik_shared_kernel), bt (C, U, 2) (lik_shared_sessions_kernel, the sigma terms) and the same with noise variances,
    against the reference summed over patients; S_B bit-equal to the unshared build; with FCD_DATA_NAN_MISSING the NaN
    counts of b and bt, planted in both trips, come back exactly.
    """
    g = check_regimes(env.n_cu, case)
    (N, U, H, Cn) = (g["Nreg"], g["U"], g["H"], g["C"])
    first_past = g["blocks"] * g["epb"]                     # first edge of the second trip
    assert first_past < Cn
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=N + U, sessions=2)
    if form == "2d":
        bt = np.ascontiguousarray(bt[:, :, 0])
    rng = np.random.default_rng(N)
    noise = None
    if form == "noise":
        vbt = rng.uniform(0, 0.02, (U, 2))
        vbt[U - 1, 0] = 0.0
        noise = (np.array([0.004]), vbt)
    (S_ref, lM_ref, tol) = table_reference(env, m, b, bt, form, noise, False)
    (S_B, L, _n) = build_tables(env, m, b, bt, True, noise=noise)
    (S_u, _lM, _n) = build_tables(env, m, b, bt, False, noise=noise)
    assert L.shape == (Cn, 1, 3, 3) and np.all(np.isfinite(L)) and np.all(np.isfinite(S_B))
    report(case + " " + form, "L", L[:, 0], lM_ref.sum(axis=1), tol)
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **tol)
    nptest.assert_array_equal(S_B, S_u)
    nptest.assert_allclose(S_B, S_ref, **(NR.tolerance_b(b, m.mu, m.sigma, noise[0]) if noise else dict(rtol=1e-12)))
    # NaN counts: a known number in b and in bt, in both trips
    (bn, btn) = (b.copy(), bt.copy())
    b_at = [0, 7, first_past - 1, first_past, Cn - 1]
    bn[b_at, 0] = np.nan
    bt_flat = btn.reshape(Cn, -1)
    picks = rng.choice(Cn * bt_flat.shape[1], size=301, replace=False)
    bt_flat.reshape(-1)[picks] = np.nan
    bt_flat[first_past] = np.nan                            # a whole edge of the second trip, and its last item
    bt_flat[Cn - 1, -1] = np.nan
    bt_flat[0, 0] = np.nan
    btn = bt_flat.reshape(bt.shape)
    n_bt = int(np.isnan(btn).sum())
    assert n_bt > 300 and int(np.isnan(btn[first_past:]).sum()) > bt_flat.shape[1]
    (S_ref, lM_ref, tol) = table_reference(env, m, bn, btn, form, noise, True)
    (S_n, L_n, counts) = build_tables(env, m, bn, btn, True, flags=MISS, count=True, noise=noise)
    assert counts == (len(b_at), n_bt), "NaN counts (b, bt) %s, planted %s" % (counts, (len(b_at), n_bt))
    assert np.all(np.isfinite(L_n))
    report(case + " " + form + " missing", "L", L_n[:, 0], lM_ref.sum(axis=1), tol)
    nptest.assert_allclose(L_n[:, 0], lM_ref.sum(axis=1), **tol)
    assert np.all(L_n[first_past, 0] == 0.0) and np.all(S_n[b_at] == 0.0)
    (S_un, _lM, counts_u) = build_tables(env, m, bn, btn, False, flags=MISS, count=True, noise=noise)
    assert counts_u == counts
    nptest.assert_array_equal(S_n, S_un)


# ------------------------------------------------------------------------------------------------
# noise records
# ------------------------------------------------------------------------------------------------
def distinctive(v):
    """The last subjects get variances no other subject has, zero among them: a record in the wrong slot shows."""
    v[-13:] = np.array([0.5, 0.0, 0.31, 0.07, 1.5, 0.0, 0.9, 0.11, 0.23, 0.0, 2.0, 0.41, 0.0])
    return v


def test_noise_records_of_524300_patients(env):
    """var_bt alone, (C 1, H 3, U 524 300, K 1): 12 records past the first trip of noise_records_kernel; unshared and shared."""
    g = check_regimes(env.n_cu, "records bt 524300")
    (U, H) = (g["U"], 3)
    m = env.pkg.UnsharedRegionModel()
    rng = np.random.default_rng(2)
    b = rng.normal(0.0, 0.1, (1, H))
    bt = rng.normal(0.0, 0.15, (1, U))
    vbt = distinctive(rng.uniform(0, 0.02, U))
    (S_ref, lM_ref) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, None, vbt)
    tol = NR.tolerance(bt, m.mu, m.sigma, vbt)
    (S_B, lM, _n) = build_tables(env, m, b, bt, False, noise=(None, vbt))
    assert np.all(np.isfinite(lM))
    report("noise_records_kernel var_bt", "lM", lM, lM_ref, tol)
    nptest.assert_allclose(lM, lM_ref, **tol)
    nptest.assert_allclose(lM[:, -13:], lM_ref[:, -13:], **tol)
    nptest.assert_allclose(S_B, S_ref, **NR.tolerance_b(b, m.mu, m.sigma, None))
    (S_s, L, _n) = build_tables(env, m, b, bt, True, noise=(None, vbt))
    tol3 = NR.tolerance(bt, m.mu, m.sigma, vbt, scale=3)
    report("noise_records_kernel var_bt shared", "L", L[:, 0], lM_ref.sum(axis=1), tol3)
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **tol3)
    nptest.assert_array_equal(S_s, S_B)
    # the variances of the last subjects matter at this tolerance: without them the tables differ
    (_S, lM_0) = NR.lik_tables(b, bt[:, -13:], m.mu, m.sigma, m.eta, m.epsilon, None, None)
    assert not np.allclose(lM[:, -13:][:, vbt[-13:] > 0], lM_0[:, vbt[-13:] > 0], rtol=1e-6)


def test_noise_records_of_524300_controls(env):
    """var_b alone, (C 1, H 524 300, U 1, K 1): the records of b and one of bt, 13 past the first trip; unshared and shared."""
    g = check_regimes(env.n_cu, "records b 524300")
    (H, U) = (g["H_b"], 1)
    m = env.pkg.UnsharedRegionModel()
    rng = np.random.default_rng(3)
    b = rng.normal(0.0, 0.1, (1, H))
    bt = rng.normal(0.0, 0.15, (1, U))
    vb = distinctive(rng.uniform(0, 0.02, H))
    (S_ref, lM_ref) = NR.lik_tables(b, bt, m.mu, m.sigma, m.eta, m.epsilon, vb, None)
    lp_ref = NR.lp_B_g_F(b, m.mu, m.sigma, vb)
    tol_b = NR.tolerance_b(b, m.mu, m.sigma, vb)
    (S_B, lM, _n, lpB) = build_tables(env, m, b, bt, False, noise=(vb, None), lpB=True)
    assert np.all(np.isfinite(lpB))
    report("noise_records_kernel var_b", "lp_B_g_F", lpB, lp_ref, tol_b)
    nptest.assert_allclose(lpB, lp_ref, **tol_b)
    report("noise_records_kernel var_b", "S_B", S_B, S_ref, tol_b)
    nptest.assert_allclose(S_B, S_ref, **tol_b)
    nptest.assert_allclose(lM, lM_ref, **NR.tolerance(bt, m.mu, m.sigma, None))
    (S_s, L, _n) = build_tables(env, m, b, bt, True, noise=(vb, None))
    nptest.assert_array_equal(S_s, S_B)
    nptest.assert_allclose(L[:, 0], lM_ref.sum(axis=1), **NR.tolerance(bt, m.mu, m.sigma, None, scale=3))
    lp_0 = NR.lp_B_g_F(b[:, -13:], m.mu, m.sigma, None)
    assert not np.allclose(lpB[:, -13:][:, vb[-13:] > 0], lp_0[:, vb[-13:] > 0], rtol=1e-6)


# ------------------------------------------------------------------------------------------------
# membership fold
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_cols", ["U", "1"])
def test_member_fold_past_the_first_trip(env, r_cols):
    """fcd_member_loglik at (Nreg 4, U 70, G 7552): 528 640 outputs out[g U + u], 4352 of them in member_fold's second trip;
    the control side alone and both sides, r one column per subject and one for all."""
    g = check_regimes(env.n_cu, "fold 4x70x7552")
    (N, U, G) = (4, g["U"], g["G"])
    rng = np.random.default_rng(G)
    m = env.pkg.SharedRegionModel()
    m.pi, m.eta, m.epsilon = 0.3, 0.4, 0.2
    m.sigma = np.array([0.15, 0.15, 0.2])
    (_r, _t, _f, _ft, _b, x) = m.sample(N, 1, U, seed=N + U)
    theta = m.theta()
    f = rng.integers(0, 3, size=(G, _tri(N)))
    r = (rng.random((G, N, U if r_cols == "U" else 1)) < 0.4).astype(np.uint8)
    t = env.torch
    f_state = t.zeros((_cdiv(G, 64), _tri(N), 64), dtype=t.uint8, device="cuda")
    r_bits = t.zeros((_cdiv(G, 64), N, r.shape[2]), dtype=t.int64, device="cuda")
    (f_d, r_d) = (up(env, f.astype(np.uint8)), up(env, r))
    env.ctx.call("fcd_gibbs_import_state", env.lib.dptr(f_d), env.lib.dptr(r_d), N, r.shape[2], G, env.lib.dptr(f_state),
                 env.lib.dptr(r_bits), env.lib.stream_ptr())
    (th, _th) = env.lib.dbl_array(theta)
    x_d = up(env, x)
    want_c = MR.control_loglik(x, theta, f)
    want_p = MR.patient_loglik(x, theta, f, r if r_cols == "U" else r[:, :, 0])
    for patient in (False, True):
        lc = nan_tensor(env, G, U)
        lp = nan_tensor(env, G, U) if patient else None
        env.ctx.call("fcd_member_loglik", env.lib.dptr(x_d), th, env.lib.dptr(f_state), env.lib.dptr(r_bits if patient else None), N, U,
                     G, r.shape[2], 0, env.lib.dptr(lc), env.lib.dptr(lp), env.lib.stream_ptr())
        got_c = lc.cpu().numpy()
        assert np.all(np.isfinite(got_c)), "out_control still holds the sentinel at %s" % np.argwhere(~np.isfinite(got_c))[:4].tolist()
        report("member_fold r_cols=%s" % r_cols, "control", got_c, want_c, SUM)
        nptest.assert_allclose(got_c, want_c, **SUM)
        if patient:
            got_p = lp.cpu().numpy()
            assert np.all(np.isfinite(got_p)), "out_patient still holds the sentinel at %s" % np.argwhere(~np.isfinite(got_p))[:4].tolist()
            report("member_fold r_cols=%s" % r_cols, "patient", got_p, want_p, SUM)
            nptest.assert_allclose(got_p, want_p, **SUM)
    env.ctx.check_device()


# ------------------------------------------------------------------------------------------------
# evidence tempering
# ------------------------------------------------------------------------------------------------
def temper(env, beta, src, dst):
    n = len(src)
    env.ctx.call("fcd_evidence_temper", float(beta), n, (env.lib._p * n)(*[t.data_ptr() for t in src]),
                 (env.lib._p * n)(*[t.data_ptr() for t in dst]), (C.c_int64 * n)(*[t.numel() for t in src]),
                 env.lib.stream_ptr())


def test_temper_launch_past_the_first_trip(env):
    """test_gpu_evidence.py's test_temper_launch with two tables of 2 500 001 doubles: one 16-byte aligned (the pair loop wraps,
    then a scalar tail of one), one that starts at an odd element (the scalar loop alone, three trips).  beta = 1: the sources
    bit for bit; beta = 0.37: torch's beta * src bit for bit; the words around each table untouched; one call in place."""
    check_regimes(env.n_cu, "temper aligned")
    check_regimes(env.n_cu, "temper odd start")
    t = env.torch
    rng = np.random.default_rng(3)
    n = 2500001
    src = []
    for odd in (False, True):
        a = rng.normal(size=n + 1) * 10.0 ** rng.integers(-5, 6)
        a[rng.integers(0, n + 1)] = -np.inf
        full = up(env, a)
        src.append(full[1:] if odd else full[:n])
    assert src[0].data_ptr() % 16 == 0 and src[1].data_ptr() % 16 == 8
    for beta in (1.0, 0.37):
        store = [t.full((n + 3,), 7.0, dtype=t.float64, device="cuda") for _ in src]
        dst = [store[0][2:n + 2], store[1][1:n + 1]]
        assert dst[0].data_ptr() % 16 == 0 and dst[1].data_ptr() % 16 == 8
        temper(env, beta, src, dst)
        for (s, d, st) in zip(src, dst, store):
            want = s.clone() if beta == 1.0 else beta * s
            assert d.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
            assert float((st == 7.0).sum()) == 3.0                   # nothing written outside the table
    a = src[0].clone()                                               # in place, one table
    temper(env, 0.37, [a], [a])
    assert a.cpu().numpy().tobytes() == (0.37 * src[0]).cpu().numpy().tobytes()
    env.ctx.check_device()


# ------------------------------------------------------------------------------------------------
# mean-field count law
# ------------------------------------------------------------------------------------------------
def count_law_input(N, U):
    """The recipe of test_vb_count_kernel_against_numpy: exact 0 / 1 sites, lq_R not normalised, the two point-mass rows."""
    rng = np.random.default_rng(N * 1000 + U)
    q1 = rng.uniform(0, 1, (N, U))
    q1[rng.random((N, U)) < 0.1] = 0.0
    q1[rng.random((N, U)) < 0.1] = 1.0
    q1[0, :] = 0.0                                   # region 0 typical outside patient 0: a point mass at 1
    q1[:, 0] = 1.0                                   # patient 0 anomalous everywhere: a point mass at N
    with np.errstate(divide="ignore"):
        return np.log(np.stack([1.0 - q1, q1], axis=2)) + rng.normal(0, 3, (N, U, 1))


def count_law(env, lq_R, N, U):
    pp = nan_tensor(env, U, N + 1)
    pr = nan_tensor(env, N, U + 1)
    lq = up(env, lq_R)
    env.ctx.call("fcd_vb_count_posterior", env.lib.dptr(lq), N, U, env.lib.dptr(pp), env.lib.dptr(pr), env.lib.stream_ptr())
    return pp.cpu().numpy(), pr.cpu().numpy()


@pytest.mark.parametrize("case", ["law 4095x2", "law 600x3"])
def test_count_law_with_every_bin_slot(env, case):
    """fcd_vb_count_posterior at the largest row it accepts (4096 bins: slot t = 15 of every thread) and at 600 sites (three
    chunks of sites), against the recursion of count_posterior_ref in long double, at the tolerance of
    test_vb_count_kernel_against_numpy; the rows sum to 1."""
    g = check_regimes(env.n_cu, case)
    (N, U) = (g["Nreg"], g["U"])
    lq_R = count_law_input(N, U)
    (pp, pr) = count_law(env, lq_R, N, U)
    env.ctx.check_device()
    (want_p, want_r) = R.count_posterior(lq_R, dtype=np.longdouble)
    assert want_p.dtype == np.longdouble
    assert np.all(np.isfinite(pp)) and np.all(np.isfinite(pr))
    report(case, "p_patient", pp, want_p.astype(np.float64), PB)
    report(case, "p_region", pr, want_r.astype(np.float64), PB)
    nptest.assert_allclose(pp, want_p.astype(np.float64), **PB)
    nptest.assert_allclose(pr, want_r.astype(np.float64), **PB)
    nptest.assert_allclose(pp.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    nptest.assert_allclose(pr.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(pp[0], np.eye(N + 1)[N])
    assert np.array_equal(pr[0], np.eye(U + 1)[1])


def test_count_law_refuses_4096_sites(env):
    """Nreg = 4096 is one bin more than a workgroup holds: refused, and nothing is launched (the outputs keep the sentinel)."""
    g = check_regimes(env.n_cu, "law 4096x2")
    (N, U) = (g["Nreg"], g["U"])
    pp = nan_tensor(env, U, N + 1)
    pr = nan_tensor(env, N, U + 1)
    lq = up(env, np.zeros((N, U, 2)))
    with pytest.raises(NotImplementedError, match="at most 4095"):
        env.ctx.call("fcd_vb_count_posterior", env.lib.dptr(lq), N, U, env.lib.dptr(pp), env.lib.dptr(pr), env.lib.stream_ptr())
    env.torch.cuda.synchronize()
    assert bool(env.torch.isnan(pp).all()) and bool(env.torch.isnan(pr).all())
    env.ctx.check_device()
