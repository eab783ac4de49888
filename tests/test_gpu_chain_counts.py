"""
The kernels that read the sampler's chains back out, at every chain-word layout (run with -m gpu on an MI355X).

The sweep kernels are pinned to the C oracle bit for bit elsewhere; this file pins the bookkeeping around them -- the
pooled counts of the M-step (fcd_gibbs_stats, the tally), the marginal counters behind _lq_F / _lq_R
(fcd_gibbs_accumulate, the tally, fcd_gibbs_run), the M-step itself, the per-chain log-joint and sum r of diagnostics(),
the (f, mixture case) counts of the MCEM theta step and the connection posteriors (fcd_gibbs_pair_counts,
fcd_gibbs_pair_tally) and import / export of the state -- against a recount on the host that uses none of them.  States
are planted with NumPy and loaded with import_state; the packed layout is then decoded on the host, so import is
checked independently of export.

Chain words: 64 chains per word, GW = ceil(G / 64).  In the last word, lanes >= G % 64 belong to chains that do not
exist.  The sweeps draw real values there, so every counter must mask them: where G % 64 != 0 each result is computed
again after those lanes are poisoned (f byte 2, r bit 1) and must not change.

`geometry()` restates the launch formulas of fcd_gibbs.hip / fcd_gibbs_r.hip / fcd_post.hip and each shape asserts the
regime it was picked for, so that a change of the geometry fails here instead of silently retiring the coverage.  The
host oracles run on every chain; the pair counts (O.pair_counts, a Python loop over chains) skip the two shapes with
more than 2e7 (chain, edge, patient) items.  Two shapes with more than 1024 chain words (PAIR_ROUND_SHAPES) run the pair
counts alone, where pair_tally_kernel takes the f masks of an edge in two rounds.
"""
import numpy as np
import numpy.testing as nptest
import pytest

pytestmark = pytest.mark.gpu

LJ_COND = 1e-12             # |got - exp| <= LJ_COND * sum |terms| of the chain's log-joint
PACK_TALLY_MAX = 600000     # the packing launch carries the f half of the tally while C * GW <= this (fcd_gibbs_r.hip)
PAIR_MAX_ITEMS = 20000000   # O.pair_counts above this many (chain, edge, patient) items is too slow for the suite


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    from oracle import c_oracle as CO
    from oracle import fcdiff_oracle as O
    _lib.load()

    class E:
        pass
    e = E()
    e.torch, e.pkg, e.lib, e.GibbsEngine, e.CO, e.O = torch, fcdiff_amd, _lib, GibbsEngine, CO, O
    e.ctx = _lib.Context()
    e.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return e


def up(env, a):
    return env.torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ------------------------------------------------------------------------------------------------
# launch geometry of the counting kernels
# ------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def geometry(Nreg, U, G, n_cu):
    """
    Blocks and loop trips of the kernels that read the chains, for (Nreg, U, G) on a device with n_cu CUs, from the
    launches of fcd_gibbs.hip (launch_tally, which fcd_gibbs_stats, fcd_gibbs_accumulate, fcd_gibbs_tally and the sweep
    loop run; fcd_gibbs_logjoint, fcd_gibbs_chain_rsum), fcd_gibbs_r.hip (the packing launch's tally rows) and
    fcd_post.hip (fcd_pair_tally_launch, which fcd_gibbs_pair_counts and fcd_gibbs_pair_tally run).
    """
    C = Nreg * (Nreg - 1) // 2
    NU = Nreg * U
    GW = _cdiv(G, 64)
    g = dict(C=C, U=U, NU=NU, G=G, GW=GW, tail=G % 64)
    # gibbs_tally_kernel: min(ceil(C / 64), 2 CU) f blocks of 16 waves x 4 edges; min(ceil(NU / 1024), 64) r blocks, and
    # every f block counts r bits too; with the f half done in the packing launch only the r blocks run
    fb = min(_cdiv(C, 64), 2 * n_cu)
    rb = min(_cdiv(NU, 1024), 64)
    ngrp = _cdiv(GW, 16)
    g.update(tally_f_blocks=fb, tally_f_passes=_cdiv(C, 64 * fb), tally_r_blocks=rb,
             tally_r_passes=_cdiv(NU, 1024 * max(fb, rb)), tally_r_passes_after_pack=_cdiv(NU, 1024 * rb),
             wg_groups=ngrp, wg_last=GW - 16 * (ngrp - 1))
    # gibbs_logjoint_kernel: grid (GW, 64 slices), slice s sums edges s, s + 64, ...
    g.update(lj_idle=max(0, 64 - C), lj_passes=_cdiv(C, 64))
    # gibbs_rsum_kernel: grid (GW, min(NU, 64) slices)
    rs = min(NU, 64)
    g.update(rsum_slices=rs, rsum_passes=_cdiv(NU, rs))
    g["pack_tally"] = C * GW <= PACK_TALLY_MAX
    # pair_tally_kernel: min(C, 64 CU) workgroups, a workgroup per edge; min(U, 256) threads rounded up to a wave, a
    # thread per patient; the f masks of min(GW, 1024) chain words in LDS at a time
    pb = min(C, 64 * n_cu)
    pt = _cdiv(min(U, 256), 64) * 64
    pw = min(GW, 1024)
    g.update(pair_blocks=pb, pair_threads=pt, pair_words=pw, pair_edge_passes=_cdiv(C, pb), pair_u_passes=_cdiv(U, pt),
             pair_word_rounds=_cdiv(GW, pw))
    return g


# the regimes a shape is chosen for: name -> test on geometry()
REGIMES = {
    "one chain": lambda g: g["G"] == 1,
    "one edge": lambda g: g["C"] == 1,
    "partial last word": lambda g: g["tail"] != 0,
    "one full word": lambda g: g["G"] == 64,
    "17 words": lambda g: g["GW"] == 17 and g["wg_groups"] == 2 and g["wg_last"] == 1,
    "3 wg groups, last word partial": lambda g: g["wg_groups"] >= 3 and g["tail"] != 0,
    "lj slices idle": lambda g: g["lj_idle"] > 0,
    "lj slices wrap": lambda g: g["lj_passes"] >= 2,
    "U > 64": lambda g: g["U"] > 64,
    "rsum NU < 64": lambda g: g["rsum_slices"] == g["NU"] < 64,
    "rsum wraps": lambda g: g["rsum_passes"] >= 2,
    "tally f wraps, f half in tally": lambda g: g["tally_f_passes"] >= 2 and not g["pack_tally"],
    "tally r wraps": lambda g: g["tally_r_passes"] >= 2,
    "tally r wraps after pack": lambda g: g["tally_r_passes_after_pack"] >= 2 and g["pack_tally"],
    "pair edges wrap": lambda g: g["pair_edge_passes"] >= 2,
    "pair patients wrap": lambda g: g["pair_u_passes"] >= 2,
    "pair word rounds": lambda g: g["pair_word_rounds"] >= 2,
}

# (Nreg, U, G, regimes)
SHAPES = [
    (2, 1, 1, ("one chain", "one edge", "lj slices idle", "rsum NU < 64")),
    (5, 3, 63, ("partial last word", "lj slices idle", "rsum NU < 64")),
    (7, 4, 64, ("one full word", "lj slices idle")),
    (6, 5, 65, ("partial last word", "rsum NU < 64")),
    (11, 6, 1000, ("partial last word", "lj slices idle", "rsum wraps")),
    (9, 5, 1025, ("17 words", "partial last word")),
    (13, 3, 2113, ("3 wg groups, last word partial",)),
    (3, 70, 130, ("U > 64", "partial last word", "rsum wraps")),
    (300, 3, 1024, ("tally f wraps, f half in tally", "pair edges wrap")),
    (40, 2000, 63, ("tally r wraps", "tally r wraps after pack", "U > 64", "pair patients wrap", "partial last word")),
    # the pair counts where pair_tally_kernel loops, within PAIR_MAX_ITEMS (the two shapes above are not)
    (200, 2, 65, ("pair edges wrap", "partial last word")),
    (4, 300, 65, ("pair patients wrap", "U > 64", "partial last word")),
]
SHAPE_IDS = ["%dx%dx%d" % s[:3] for s in SHAPES]
# more chain words than pair_tally_kernel holds f masks for (1024): GW = 1026, a second round of two words, the last with one
# chain; the second shape has two patient blocks as well, so the masks of every round are rebuilt per block.  The counters
# that walk every chain on the host would take too long at this G: these shapes run the pair counts alone
# (test_pair_counts_over_two_word_rounds), against the vectorised recount of conn_posterior_ref.
PAIR_ROUND_SHAPES = [
    (3, 2, 65601, ("pair word rounds", "partial last word")),
    (2, 300, 65601, ("pair word rounds", "pair patients wrap", "U > 64", "partial last word")),
]
KINDS = ("random", "f2 r1", "last word only")


def check_regimes(n_cu, Nreg, U, G, regimes):
    g = geometry(Nreg, U, G, n_cu)
    for r in regimes:
        assert REGIMES[r](g), "shape (Nreg=%d, U=%d, G=%d) is no longer in regime %r at %d CUs: %s" % (
            Nreg, U, G, r, n_cu, g)
    return g


def test_regimes_of_the_named_shapes():
    """Every shape is in its regimes on an MI355X (256 CUs), whatever device runs the suite."""
    for (Nreg, U, G, regimes) in SHAPES:
        check_regimes(256, Nreg, U, G, regimes)
    for (Nreg, U, G, _missing, regimes) in LJ_SHAPES:
        check_regimes(256, Nreg, U, G, regimes)
    for (Nreg, U, G, _n, _p, regimes) in RUN_SHAPES:
        check_regimes(256, Nreg, U, G, regimes)
    for (Nreg, U, G, regimes) in PAIR_ROUND_SHAPES:
        g = check_regimes(256, Nreg, U, G, regimes)
        assert (g["GW"], g["pair_words"], g["pair_word_rounds"], g["tail"]) == (1026, 1024, 2, 1)
        assert G * g["C"] * U <= PAIR_MAX_ITEMS
    assert geometry(2, 300, 65601, 256)["pair_u_passes"] == 2
    assert all(geometry(*s[:3], 256)["pair_word_rounds"] == 1 for s in SHAPES)
    g = geometry(300, 3, 1024, 256)
    assert (g["tally_f_blocks"], g["tally_f_passes"], g["pair_blocks"], g["pair_edge_passes"]) == (512, 2, 16384, 3)
    g = geometry(200, 2, 65, 256)
    assert (g["pair_blocks"], g["pair_edge_passes"], g["pair_threads"], g["pair_words"]) == (16384, 2, 64, 2)
    assert 65 * g["C"] * 2 <= PAIR_MAX_ITEMS
    g = geometry(4, 300, 65, 256)
    assert (g["pair_blocks"], g["pair_threads"], g["pair_u_passes"], g["pair_word_rounds"]) == (6, 256, 2, 1)
    g = geometry(200, 50, 16384, 256)                   # cfg3: one trip of the tally's f loop, one wg group
    assert (g["tally_f_passes"], g["tally_r_passes"], g["wg_groups"], g["pack_tally"]) == (1, 1, 16, False)


# ------------------------------------------------------------------------------------------------
# planted states and the host recount
# ------------------------------------------------------------------------------------------------
def planted(Nreg, U, G, kind, seed):
    """f (G, C) uint8, r (G, Nreg, U) uint8."""
    rng = np.random.default_rng(seed)
    C = Nreg * (Nreg - 1) // 2
    if kind == "random":
        f = rng.integers(0, 3, size=(G, C), dtype=np.uint8)
        r = (rng.random((G, Nreg, U)) < 0.3).astype(np.uint8)
    elif kind == "f2 r1":
        f = np.full((G, C), 2, dtype=np.uint8)
        r = np.ones((G, Nreg, U), dtype=np.uint8)
    else:
        # zero everywhere but in the chains of the last word
        f = np.zeros((G, C), dtype=np.uint8)
        r = np.zeros((G, Nreg, U), dtype=np.uint8)
        g0 = (G - 1) // 64 * 64
        f[g0:] = rng.integers(1, 3, size=(G - g0, C), dtype=np.uint8)
        r[g0:] = (rng.random((G - g0, Nreg, U)) < 0.5).astype(np.uint8)
        r[G - 1, 0, 0] = 1
    return f, r


def recount(f, r):
    """counts[0..4] = {sum r, #f=0, #f=1, #f=2, G}; cnt_f (C, 3); cnt_r (Nreg, U); per-chain sum r (G,)."""
    G = f.shape[0]
    cnt_f = np.stack([np.count_nonzero(f == k, axis=0) for k in range(3)], axis=1).astype(np.int64)
    cnt_r = r.sum(axis=0, dtype=np.int64)
    counts = np.array([cnt_r.sum(), cnt_f[:, 0].sum(), cnt_f[:, 1].sum(), cnt_f[:, 2].sum(), G], dtype=np.int64)
    return counts, cnt_f, cnt_r, r.reshape(G, -1).sum(axis=1, dtype=np.int64)


def packed_layout(f, r):
    """The device layout of (f, r) built on the host: f_state (GW, C, 64) uint8, r_bits (GW, Nreg, U) uint64."""
    (G, C) = f.shape
    GW = _cdiv(G, 64)
    fp = np.zeros((GW * 64, C), dtype=np.uint8)
    fp[:G] = f
    rp = np.zeros((GW * 64,) + r.shape[1:], dtype=np.uint64)
    rp[:G] = r
    f_state = fp.reshape(GW, 64, C).transpose(0, 2, 1)
    shifts = np.arange(64, dtype=np.uint64)[None, :, None, None]
    r_bits = np.bitwise_or.reduce(rp.reshape((GW, 64) + r.shape[1:]) << shifts, axis=1)
    return f_state, r_bits


def zero_engine(env, Nreg, U, G):
    """An engine for counting only: zero tables, no region-major tables."""
    t = env.torch
    C = Nreg * (Nreg - 1) // 2
    S_B = t.zeros((C, 3), dtype=t.float64, device="cuda")
    lM = t.zeros((C, U, 3, 3), dtype=t.float64, device="cuda")
    return env.GibbsEngine(S_B, lM, Nreg, U, G, ctx=env.ctx, region_major=False)


def poison(env, eng):
    """Non-zero values in the lanes of the last word that hold no chain: f bytes 2, r bits 1."""
    tail = eng.G % 64
    assert tail != 0
    w = eng.GW - 1
    eng.f_state[w, :, tail:] = 2
    mask = np.array([~((1 << tail) - 1) & ((1 << 64) - 1)], dtype=np.uint64).view(np.int64)[0]
    eng.r_bits[w] |= env.torch.tensor(int(mask), dtype=env.torch.int64, device="cuda")


def as_u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def from_u32(env, a):
    return up(env, np.asarray(a, dtype=np.int64).astype(np.uint32).view(np.int32))


# ------------------------------------------------------------------------------------------------
# import / export
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Nreg,U,G,regimes", SHAPES, ids=SHAPE_IDS)
def test_import_layout_and_round_trip(env, Nreg, U, G, regimes, kind):
    """import_state writes the packed layout decoded on the host (lanes without a chain hold 0); export inverts it."""
    check_regimes(env.n_cu, Nreg, U, G, regimes)
    (f, r) = planted(Nreg, U, G, kind, seed=Nreg * 1000 + U + G)
    eng = zero_engine(env, Nreg, U, G)
    eng.f_state.fill_(7)
    eng.r_bits.fill_(-1)
    eng.import_state(f, r)
    (fs, rb) = packed_layout(f, r)
    nptest.assert_array_equal(eng.f_state.cpu().numpy(), fs)
    nptest.assert_array_equal(eng.r_bits.cpu().numpy().view(np.uint64), rb)
    (fe, re_) = eng.export_state()
    nptest.assert_array_equal(fe, f)
    nptest.assert_array_equal(re_, r)


def test_import_refuses_f_above_2(env):
    """f bytes are 0, 1 or 2: import_state refuses any other value before it touches the device state."""
    (Nreg, U, G) = (5, 3, 63)
    (f, r) = planted(Nreg, U, G, "random", seed=5)
    eng = zero_engine(env, Nreg, U, G)
    eng.import_state(f, r)
    (fs, rb) = (eng.f_state.cpu().numpy().copy(), eng.r_bits.cpu().numpy().copy())
    for bad in (3, 255):
        f2 = f.copy()
        f2[G - 1, 0] = bad
        with pytest.raises(ValueError):
            eng.import_state(f2, r)
    nptest.assert_array_equal(eng.f_state.cpu().numpy(), fs)
    nptest.assert_array_equal(eng.r_bits.cpu().numpy(), rb)


# ------------------------------------------------------------------------------------------------
# stats, accumulate, tally, chain sums, pair counts against the recount
# ------------------------------------------------------------------------------------------------
def run_counters(env, eng, rng_seed, k_acc=2):
    """Every counting entry point once on the engine's current state: a dict of host results."""
    t = env.torch
    out = {}
    out["stats"] = eng.stats().cpu().numpy().copy()
    # accumulate k times from non-zero uint32 counters (some above 2^31: the sums are unsigned)
    rng = np.random.default_rng(rng_seed)
    room = (1 << 32) - 1 - k_acc * eng.G
    base_f = rng.integers(0, room, size=(eng.C, 3), dtype=np.int64)
    base_r = rng.integers(0, room, size=(eng.Nreg, eng.U), dtype=np.int64)
    base_f[0, 0] = room
    eng.cnt_f.copy_(from_u32(env, base_f))
    eng.cnt_r.copy_(from_u32(env, base_r))
    for _ in range(k_acc):
        eng.accumulate()
    out["acc_f"] = as_u32(eng.cnt_f) - base_f
    out["acc_r"] = as_u32(eng.cnt_r) - base_r
    # tally: counts only (counters untouched), counters only (counts untouched), both, both again
    eng.cnt_f.copy_(from_u32(env, base_f))
    eng.cnt_r.copy_(from_u32(env, base_r))
    eng.counts.fill_(-5)
    out["tally_counts"] = eng.tally(want_counts=True, accumulate=False).cpu().numpy().copy()
    nptest.assert_array_equal(as_u32(eng.cnt_f), base_f)
    nptest.assert_array_equal(as_u32(eng.cnt_r), base_r)
    eng.counts.fill_(-5)
    eng.tally(want_counts=False, accumulate=True)
    assert (eng.counts.cpu().numpy() == -5).all()
    out["tally_cnt_f"] = as_u32(eng.cnt_f) - base_f
    out["tally_cnt_r"] = as_u32(eng.cnt_r) - base_r
    out["tally_both"] = eng.tally(want_counts=True, accumulate=True).cpu().numpy().copy()
    out["tally_both_cnt_f"] = as_u32(eng.cnt_f) - base_f
    out["tally_both_cnt_r"] = as_u32(eng.cnt_r) - base_r
    out["tally_again"] = eng.tally(want_counts=True, accumulate=False).cpu().numpy().copy()
    out["rsum"] = eng.r_sums().cpu().numpy().astype(np.int64)
    if eng.G * eng.C * eng.U <= PAIR_MAX_ITEMS:
        out["pair"] = eng.pair_counts().cpu().numpy()
        W0 = t.as_tensor(rng.integers(0, 1000, size=(eng.C, eng.U, 3, 3)).astype(np.float64), device="cuda")
        out["pair_acc"] = eng.pair_counts(W0.clone(), accumulate=True).cpu().numpy() - W0.cpu().numpy()
        # uint32 += on top of existing values, some above 2^31
        A0 = rng.integers(0, (1 << 32) - 1 - eng.G, size=(eng.C, eng.U, 3, 3), dtype=np.int64)
        A0.flat[0] = (1 << 32) - 1 - eng.G
        out["pair_tally"] = as_u32(eng.pair_tally(from_u32(env, A0))) - A0
    env.ctx.check_device()
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Nreg,U,G,regimes", SHAPES, ids=SHAPE_IDS)
def test_counters_against_recount(env, Nreg, U, G, regimes, kind):
    """
    stats(), accumulate() x 2 on non-zero uint32 counters, tally() as counts only / counters only / both / again (its
    context accumulators are reset: the same counts), r_sums(), pair_counts() (plain and accumulate=True on top of
    existing values) and pair_tally() (on top of existing uint32 values) against a recount of the planted state; where
    the last word is partial, the same again with its chain-less lanes poisoned, bit for bit.
    Regression (40x2000x63): the tally's grid held only its f blocks where ceil(NU / 1024) r blocks were more; the r
    sites of the missing blocks went uncounted and no block drew the last ticket, so counts were never written.
    """
    check_regimes(env.n_cu, Nreg, U, G, regimes)
    (f, r) = planted(Nreg, U, G, kind, seed=Nreg * 7 + U * 13 + G)
    (counts, cnt_f, cnt_r, rsum) = recount(f, r)
    eng = zero_engine(env, Nreg, U, G)
    eng.import_state(f, r)
    clean = run_counters(env, eng, rng_seed=G)
    nptest.assert_array_equal(clean["stats"][:5], counts, err_msg="stats")
    nptest.assert_array_equal(clean["acc_f"], 2 * cnt_f, err_msg="accumulate: cnt_f")
    nptest.assert_array_equal(clean["acc_r"], 2 * cnt_r, err_msg="accumulate: cnt_r")
    for key in ("tally_counts", "tally_both", "tally_again"):
        nptest.assert_array_equal(clean[key][:5], counts, err_msg=key)
        assert (clean[key][5:] == 0).all(), key
    nptest.assert_array_equal(clean["tally_cnt_f"], cnt_f, err_msg="tally (counters only): cnt_f")
    nptest.assert_array_equal(clean["tally_cnt_r"], cnt_r, err_msg="tally (counters only): cnt_r")
    nptest.assert_array_equal(clean["tally_both_cnt_f"], 2 * cnt_f, err_msg="tally (both): cnt_f")
    nptest.assert_array_equal(clean["tally_both_cnt_r"], 2 * cnt_r, err_msg="tally (both): cnt_r")
    nptest.assert_array_equal(clean["rsum"], rsum, err_msg="r_sums")
    if kind == "f2 r1":
        assert (clean["rsum"] == Nreg * U).all()
    if "pair" in clean:
        W = env.O.pair_counts(f, r)
        nptest.assert_array_equal(clean["pair"], W, err_msg="pair_counts")
        nptest.assert_array_equal(clean["pair_acc"], W, err_msg="pair_counts(accumulate=True)")
        nptest.assert_array_equal(clean["pair_tally"], W, err_msg="pair_tally")
    if G % 64:
        poison(env, eng)
        dirty = run_counters(env, eng, rng_seed=G)
        assert set(dirty) == set(clean)
        for key in clean:
            assert clean[key].tobytes() == dirty[key].tobytes(), "%s changed with the chain-less lanes poisoned" % key


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Nreg,U,G,regimes", PAIR_ROUND_SHAPES, ids=["%dx%dx%d" % s[:3] for s in PAIR_ROUND_SHAPES])
def test_pair_counts_over_two_word_rounds(env, Nreg, U, G, regimes, kind):
    """
    pair_counts() (plain, and accumulate=True on top of existing values) and pair_tally() (on top of existing uint32 values,
    some above 2^31) where the f masks of an edge take two rounds of chain words, against the vectorised recount of
    conn_posterior_ref.pair_counts; bit for bit the same with the chain-less lanes of the last word poisoned.  Every output
    starts from a sentinel or from known values, so an item left unwritten shows.
    """
    import conn_posterior_ref as CPR
    check_regimes(env.n_cu, Nreg, U, G, regimes)
    t = env.torch
    (f, r) = planted(Nreg, U, G, kind, seed=Nreg * 7 + U * 13 + G)
    W = CPR.pair_counts(f, r)
    assert W.sum() == G * W.shape[0] * U
    eng = zero_engine(env, Nreg, U, G)
    eng.import_state(f, r)
    rng = np.random.default_rng(G + U)
    W0 = rng.integers(0, 1000, size=(eng.C, U, 3, 3)).astype(np.float64)
    A0 = rng.integers(1, (1 << 32) - 1 - G, size=(eng.C, U, 3, 3), dtype=np.int64)
    A0.flat[0] = (1 << 32) - 1 - G

    def run():
        plain = eng.pair_counts(t.full((eng.C, U, 3, 3), float("nan"), dtype=t.float64, device="cuda")).cpu().numpy()
        acc = eng.pair_counts(up(env, W0), accumulate=True).cpu().numpy() - W0
        tally = as_u32(eng.pair_tally(from_u32(env, A0))) - A0
        env.ctx.check_device()
        return plain, acc, tally
    clean = run()
    for (got, name) in zip(clean, ("pair_counts", "pair_counts(accumulate=True)", "pair_tally")):
        nptest.assert_array_equal(got, W, err_msg=name)
    poison(env, eng)
    for (a, b, name) in zip(clean, run(), ("pair_counts", "pair_counts(accumulate=True)", "pair_tally")):
        assert a.tobytes() == b.tobytes(), "%s changed with the chain-less lanes poisoned" % name


# ------------------------------------------------------------------------------------------------
# log-joint against the C oracle
# ------------------------------------------------------------------------------------------------
def tables_for(env, Nreg, H, U, seed, missing=False):
    """(S_B, lM) host and device, from sampled data; missing=True: NaN holes in bt and the NaN-missing table kernel."""
    m = env.pkg.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(Nreg, H, U, seed=seed)
    if not missing:
        (S_B, lM) = env.CO.lik_tables(b, bt, m.theta())
        return m, S_B, lM, up(env, S_B), up(env, lM)
    rng = np.random.default_rng(seed)
    bt = bt.copy()
    bt[rng.random(bt.shape) < 0.2] = np.nan
    bt[:, U - 1] = np.nan
    fit = env.pkg.fit.UnsharedRegionFit()
    fit._ctx = env.ctx
    fit.model, fit.b, fit.bt, fit.missing_data = m, b, bt, True
    fit._init_lps(Nreg, H, U)
    fit._update_lps()
    return m, fit._d["S_B"].cpu().numpy(), fit._lM, fit._d["S_B"], fit._d["lM"]


def logjoint_scale(f, r, S_B, lM, lng, lnpi2):
    """sum |terms| of each chain's log-joint, in long double."""
    from oracle import fcdiff_oracle as O
    (G, C) = f.shape
    ends = O.edge_endpoints(r.shape[1])
    cs = np.arange(C)
    out = np.zeros(G, dtype=np.longdouble)
    a = np.abs(np.asarray(lM, dtype=np.longdouble))
    for g in range(G):
        fg = f[g].astype(np.int64)
        l = O.mix_index(r[g][ends[:, 0]], r[g][ends[:, 1]])
        out[g] = (np.abs(np.longdouble(lng[fg])).sum() + np.abs(np.longdouble(S_B[cs, fg])).sum()
                  + np.abs(np.where(r[g] != 0, np.longdouble(lnpi2[1]), np.longdouble(lnpi2[0]))).sum()
                  + a[cs[:, None], np.arange(lM.shape[1])[None, :], fg[:, None], l].sum())
    return out.astype(np.float64)


# (Nreg, U, G, missing, regimes)
LJ_SHAPES = [
    (14, 9, 130, False, ("lj slices wrap", "partial last word")),
    (3, 70, 130, False, ("U > 64", "lj slices idle", "partial last word")),
    (11, 6, 1000, False, ("lj slices idle", "partial last word")),
    (12, 8, 200, True, ("lj slices wrap", "partial last word")),
]


@pytest.mark.parametrize("Nreg,U,G,missing,regimes", LJ_SHAPES, ids=["%dx%dx%d%s" % (s[0], s[1], s[2], "-missing" if s[3] else "")
                                                                     for s in LJ_SHAPES])
def test_logjoint_against_oracle(env, Nreg, U, G, missing, regimes):
    """
    fcd_gibbs_logjoint for every chain against CO.gibbs_logjoint, to the conditioning of the sum
    (|got - exp| <= 1e-12 sum |terms|), at a random state and at f = 2, r = 1 everywhere; bit for bit the same with the
    chain-less lanes poisoned.  missing=True: tables with NaN in bt, so that some lM rows are exactly 0.
    """
    check_regimes(env.n_cu, Nreg, U, G, regimes)
    (m, S_B, lM, S_B_d, lM_d) = tables_for(env, Nreg, 4, U, seed=Nreg * 31 + U, missing=missing)
    if missing:
        assert (lM == 0).all(axis=(2, 3)).any() and not (lM == 0).all()
    eng = env.GibbsEngine(S_B_d, lM_d, Nreg, U, G, ctx=env.ctx, region_major=False)
    eng.set_hyper(m.gamma, m.pi2())
    h = eng.hyper.cpu().numpy()
    (lng, lnpi2) = (h[0:3].copy(), h[3:5].copy())
    for kind in ("random", "f2 r1"):
        (f, r) = planted(Nreg, U, G, kind, seed=G + Nreg)
        eng.import_state(f, r)
        got = eng.logjoint().cpu().numpy()
        exp = env.CO.gibbs_logjoint(f, r, S_B, lM, lng, lnpi2)
        scale = logjoint_scale(f, r, S_B, lM, lng, lnpi2)
        assert np.isfinite(exp).all() and (scale > 0).all()
        err = np.abs(got - exp)
        bad = ~(err <= LJ_COND * scale)
        assert not bad.any(), "%s: chains %s: |got - exp| %s > %g * %s" % (kind, np.nonzero(bad)[0][:8], err[bad][:8],
                                                                           LJ_COND, scale[bad][:8])
        poison(env, eng)
        assert eng.logjoint().cpu().numpy().tobytes() == got.tobytes(), kind


# ------------------------------------------------------------------------------------------------
# fcd_gibbs_run: counts and counters of the sweep loop against the oracle's chains
# ------------------------------------------------------------------------------------------------
# (Nreg, U, G, sweeps, sweeps whose packing launch carries the f half, regimes)
RUN_SHAPES = [
    # U <= 64: the packing launch runs in the first sweep only and carries its f half; the tally counts it afterwards
    (17, 7, 1025, 3, 1, ("17 words", "partial last word")),
    # C GW > 600 000: the packing launch of the first sweep does not carry the f half; the tally's f loop wraps
    (300, 3, 1024, 2, 0, ("tally f wraps, f half in tally",)),
    # U > 64 (any-U f kernel): a packing launch in every sweep, carrying the f half; the tally's r loop then wraps
    (40, 2000, 63, 2, 2, ("tally r wraps after pack", "partial last word")),
]


@pytest.mark.parametrize("Nreg,U,G,n_sweeps,in_pack,regimes", RUN_SHAPES, ids=["%dx%dx%d" % s[:3] for s in RUN_SHAPES])
def test_run_counts_against_oracle_chains(env, Nreg, U, G, n_sweeps, in_pack, regimes):
    """
    fcd_gibbs_run(want_counts, accumulate_from = 0, an M-step after the last sweep) from the device's own init, whose
    chain-less lanes hold real draws: counts of the last sweep, cnt_f / cnt_r summed over all sweeps and the M-step's
    hyper block against a recount of the C oracle's chains after the same sweeps; fcd_gibbs_mstep on the returned counts
    writes the same hyper block, byte for byte.  The context's counters say where the f half of each sweep's tally ran.
    """
    g = check_regimes(env.n_cu, Nreg, U, G, regimes)
    (m, S_B, lM, S_B_d, lM_d) = tables_for(env, Nreg, 3, U, seed=Nreg + U)
    (seed, chain0, pi) = (777 + G, 3, 0.3)
    eng = env.GibbsEngine(S_B_d, lM_d, Nreg, U, G, chain0=chain0, seed=seed, ctx=env.ctx)
    eng.set_hyper(m.gamma, m.pi2())
    h0 = eng.hyper.cpu().numpy()
    eng.init(pi)
    if g["tail"]:
        tail = g["tail"]
        assert int(eng.f_state[-1, :, tail:].count_nonzero()) > 0
        assert (eng.r_bits[-1].cpu().numpy().view(np.uint64) >> np.uint64(tail)).any()
    (f_o, r_o) = env.CO.gibbs_init(G, Nreg, U, pi, seed, chain0)
    sum_f = np.zeros((eng.C, 3), dtype=np.int64)
    sum_r = np.zeros((Nreg, U), dtype=np.int64)
    for s in range(n_sweeps):
        env.CO.gibbs_f_step(f_o, r_o, S_B, lM, h0[0:3], seed, s, chain0)
        env.CO.gibbs_r_step(f_o, r_o, lM, h0[3:5], seed, s, 1, chain0)
        (counts, cnt_f, cnt_r, _rs) = recount(f_o, r_o)
        sum_f += cnt_f
        sum_r += cnt_r
    (n_pack0, n_in0) = (env.ctx.stat("pack_launches"), env.ctx.stat("tally_f_in_pack"))
    cts = eng.run(0, n_sweeps, mstep_every=n_sweeps, accumulate_from=0, want_counts=True)
    got = cts.cpu().numpy()
    n_in = env.ctx.stat("tally_f_in_pack") - n_in0
    assert n_in == in_pack, "the packing launch carried the f half in %d sweeps, expected %d" % (n_in, in_pack)
    assert env.ctx.stat("pack_launches") - n_pack0 >= n_in
    assert env.ctx.stat("dev_err") == 0
    (f_g, r_g) = eng.export_state()
    assert np.array_equal(f_g, f_o) and np.array_equal(r_g, r_o), "chains left the oracle's"
    nptest.assert_array_equal(got[:5], counts, err_msg="counts of the last sweep")
    nptest.assert_array_equal(as_u32(eng.cnt_f), sum_f, err_msg="cnt_f")
    nptest.assert_array_equal(as_u32(eng.cnt_r), sum_r, err_msg="cnt_r")
    (pi_h, gamma_h) = env.O.gibbs_mstep(counts, Nreg, U)
    h = eng.hyper.cpu().numpy()
    nptest.assert_allclose(h[0:3], np.log(gamma_h), rtol=1e-14, atol=0)
    nptest.assert_allclose(h[3:5], [np.log(1.0 - pi_h), np.log(pi_h)], rtol=1e-14, atol=0)
    eng.mstep(cts)
    assert eng.hyper.cpu().numpy().tobytes() == h.tobytes(), "fcd_gibbs_mstep differs from the tally's M-step"
