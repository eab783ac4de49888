"""
Conditions on the INPUTS of tests/test_gpu_nonfinite_tables.py, checked without a GPU: on the table sets of
tests/nonfinite_tables.py (-inf table entries, zero gamma / pi) the Python oracle and the C oracle draw the same chains from
the same conditionals, no conditional of a compared draw is NaN or +inf, every pattern of -inf among the log-weights occurs
often enough and with both of its possible outcomes, and the placements the kernels' paths divide at are hit.  All of it is
evaluated on the oracle alone.

The last test restates the draw the fast f forms made from log-odds against type 0, fcd_draw_f(0, a1 - a0, a2 - a0, x), in
NumPy.  With a0 = -inf the log-odds are +inf or NaN, exp(inf - inf) is NaN, every comparison is false and the answer is 2:
  {0}    -inf  wrong wherever the oracle draws 1 (it draws 1 or 2 by their weights),
  {0, 2} -inf  wrong always (the oracle draws 1 for certain),
  {0, 1} -inf  right by accident (the oracle draws 2 for certain) -- the issue that asked for these sets expected a
               difference here too; the arithmetic above gives none, and the test says so,
  all other patterns (a0 finite, or all three -inf where the oracle's own NaN comparisons answer 2) agree.
The sets therefore catch that form of the draw, which is what the test keeps pinned.
"""
import numpy as np
import pytest

import boundary_probes as BP
import nonfinite_tables as NT
from oracle import fcdiff_oracle as O

SETS = list(NT.SETS)


def source(name):
    return NT.SETS[name][0]


def python_sweeps(T):
    """N_SWEEPS sweeps of the Python oracle from (f0, r0): states after each, conditionals before every draw."""
    (f, r) = (T.f0.copy(), T.r0.copy())
    (G, C) = f.shape
    out = []
    for s in range(NT.N_SWEEPS):
        sw = T.sweep + s
        cf = np.empty((G, C, 3))
        cr = np.empty((G, T.Nreg, T.U, 2))
        for g in range(G):
            for c in range(C):
                a = O.f_conditional_logits(c, r[g], T.S_B, T.lM, T.lng)
                cf[g, c] = a
                (idx, word) = O.f_draw_site(c)
                f[g, c] = O.draw_f(a, O.site_uniform32(T.seed, idx, T.chain0 + g, sw, O.KIND_F, word))
            for n in range(T.Nreg):
                for u in range(T.U):
                    (s0, s1) = O.r_conditional_logits(n, u, f[g], r[g], T.lM, T.lnpi2, O.EDGE_SYMMETRIC)
                    cr[g, n, u] = (s0, s1)
                    (idx, half) = O.r_draw_site(n, u, T.U)
                    r[g, n, u] = O.draw_r(s0, s1, O.site_uniform(T.seed, idx, T.chain0 + g, sw, O.KIND_R, half))
        out.append((f.copy(), r.copy(), cf, cr))
    return out


@pytest.mark.parametrize("name", SETS)
def test_python_and_c_oracle_agree(name):
    """Reduced G: identical chains, identical -inf pattern of the conditionals (no NaN, no +inf in either), finite ones equal
    to rounding.  np.max, the C oracle's ?: maximum and the device's fmax differ on NaN log-weights only, and there are none."""
    T = NT.build_set(name, G=2)
    with np.errstate(invalid="ignore"):                 # (exp(-inf - -inf) where all three types are impossible: both oracles answer 2)
        py = python_sweeps(T)
    for (s, (f, r, cf, cr)) in enumerate(py):
        assert np.array_equal(f, T.f_after[s]) and np.array_equal(r, T.r_after[s]), "%s: chains differ after sweep %d" % (name, s + 1)
        for (a, b) in ((cf, T.cond_f[s]), (cr, T.cond_r[s])):
            assert not np.isnan(a).any() and not np.isnan(b).any() and not (a == np.inf).any() and not (b == np.inf).any()
            assert np.array_equal(a == -np.inf, b == -np.inf)
            fin = np.isfinite(a)
            np.testing.assert_allclose(a[fin], b[fin], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", SETS)
def test_inputs_hold_finite_values_and_minus_inf_only(name):
    """... and so do the conditionals of every compared draw, at the G the GPU test runs."""
    T = NT.build_set(name)
    assert np.isfinite(T.S_B).all()
    for a in (T.lM, T.lng, T.lnpi2) + tuple(T.cond_f) + tuple(T.cond_r):
        assert not np.isnan(a).any() and not (a == np.inf).any()
    src = source(name)
    assert np.isfinite(T.lM).all() == (not any(p in src for p in ("item", "plant", "from-data", "firm")))
    if "from-data" in src:
        # only N_0 underflows, only at the outliers, only in the typical case: M[0, typical] = N_0 at epsilon = 0
        bad = T.lM == -np.inf
        assert np.array_equal(bad[:, :, 0, 0], T.data[3]) and bad.sum() == T.data[3].sum() and T.data[3].sum() >= 8


def census(T):
    p = NT.f_pattern(T.cond_f[0])
    rp = NT.r_pattern(T.cond_r[0])
    return p, rp, np.array([(p == i).sum() for i in range(7)]), np.array([(rp == i).sum() for i in range(4)])


def test_pattern_census_covers_every_case():
    """First compared sweep, oracle alone.  Printed per set (-s): draws per pattern of -inf among (a0, a1, a2), outcomes of the
    single-type patterns, r draws by which of (s0, s1) is -inf."""
    tot = np.zeros(7, dtype=np.int64)
    rtot = np.zeros(4, dtype=np.int64)
    outcomes = np.zeros((3, 3), dtype=np.int64)
    r_fin = np.zeros(2, dtype=np.int64)
    for name in SETS:
        T = NT.build_set(name)
        (p, rp, cnt, rc) = census(T)
        tot += cnt
        rtot += rc
        single = np.array([np.bincount(T.f1[p == i], minlength=3) for i in range(3)])
        outcomes += single
        if rc[1:].sum():
            r_fin += np.bincount(T.r1[rp == 0], minlength=2)
        print("%-20s f %s  outcomes of {0},{1},{2} %s  r (finite, s0, s1, both) %s" % (name, cnt.tolist(), single.tolist(), rc.tolist()))
        src = source(name)
        # the pattern a set targets
        if src.startswith("plant"):
            assert (cnt[:6] >= 64).all(), name
        for k in range(3):
            if src == "gamma%d" % k:
                assert cnt[k] == T.G * T.C
        if src == "item":
            assert cnt[6] >= 64
    print("all sets: f %s  r %s" % (tot.tolist(), rtot.tolist()))
    assert (tot >= 200).all()
    # each single-type pattern leaves two types: both are drawn (a kernel that answers a constant fails)
    for k in range(3):
        assert outcomes[k, k] == 0 and (np.delete(outcomes[k], k) >= 20).all()
    assert (rtot[1:] >= 64).all() and (r_fin > 0).all()


def test_one_l_sets_mix_finite_and_non_finite_lanes():
    """plant-one-l: the chains of one wave (64 consecutive chains) differ in whether the edge's log-weights are finite."""
    for name in SETS:
        if source(name) != "plant-one-l":
            continue
        T = NT.build_set(name)
        p = NT.f_pattern(T.cond_f[0]) >= 0                              # (G, C)
        w = p.reshape(T.G // 64, 64, T.C)
        mixed = int((w.any(axis=1) & ~w.all(axis=1)).sum())
        print(name, "mixed (chain word, edge) pairs:", mixed)
        assert mixed >= 32


def test_placements_are_hit():
    for name in SETS:
        src = source(name)
        if not ("item" in src or src.startswith("plant")):
            continue
        T = NT.build_set(name)
        (en, em) = BP.edge_pairs(T.Nreg)
        bad = (T.lM == -np.inf).any(axis=(1, 2, 3))
        touched = set(en[bad]) | set(em[bad])
        rows = {0, 15} | ({32} if T.Nreg == 33 else set()) | ({16} if T.Nreg == 17 else set())
        assert rows <= touched, name
        assert (bad & (en // 16 == em // 16)).any()
        if T.Nreg > 16:
            assert (bad & (en // 16 != em // 16)).any()
        # ... and the draws there see it: f draws of the placement edges, and (where the r pass can meet the value at all:
        # after a plant-all-l f pass no chain holds an impossible type) r draws of both regions of each
        p = NT.f_pattern(T.cond_f[0])
        rp = NT.r_pattern(T.cond_r[0])
        for (n, m) in NT.place_edges(T.Nreg):
            assert (p[:, NT.edge_id(n, m)] >= 0).any(), (name, n, m)
            if "item" in src:
                assert (rp[:, n, :] != 0).any() and (rp[:, m, :] != 0).any(), (name, n, m)
        if src == "plant-one-l":
            assert len({n for n in rows if (rp[:, n, :] != 0).any()}) >= 2


def test_firm_sets_put_the_minus_inf_edges_inside_decided_tiles():
    """`firm`: the rule of decided edges (tests/f_sure_ref.py) decides every edge but the placement edges, whose bounds are
    NaN; so the record build's hint says "some tile, not every tile", each -inf edge is the open edge of a tile whose other
    edges are decided, and the oracle draws the decided mode on every decided edge in both compared sweeps."""
    import f_sure_ref as R
    names = [n for n in SETS if source(n) == "firm"]
    assert {NT.SETS[n][1:3] for n in names} == {(33, 7), (17, 64)}
    for name in names:
        T = NT.build_set(name)
        (hint, mode, nan_bounds) = NT.decided_rule(T)
        place = sorted(NT.edge_id(n, m) for (n, m) in NT.place_edges(T.Nreg))
        rest = np.setdiff1d(np.arange(T.C), place)
        assert hint and nan_bounds.tolist() == place == np.nonzero(T.items.any(axis=1))[0].tolist(), name
        assert (mode[place] == -1).all() and np.array_equal(mode[rest], rest % 3), name
        n_tiles = sum(len(t) > 0 for t in R.tiles(T.Nreg))
        decided = R.decided_tiles(T.Nreg, mode)
        assert 0 < len(decided) == n_tiles - len({min(t) for t in R.tiles(T.Nreg) if len(t) and (mode[t] < 0).any()}) < n_tiles, name
        assert any(len(t) > 1 and (mode[t] < 0).sum() == 1 for t in R.tiles(T.Nreg) if len(t)), name
        for s in range(NT.N_SWEEPS):
            assert (NT.f_pattern(T.cond_f[s])[:, place] == 6).all(), name
            assert np.array_equal(T.f_after[s][:, rest], np.broadcast_to(mode[rest], (T.G, len(rest)))), name
        print("%s: %d of %d tiles decided at the hint, %d edges with NaN bounds" % (name, len(decided), n_tiles, len(place)))


def test_difference_form_draw_fails_on_these_sets():
    """See the header: the draw from log-odds against type 0 differs from the oracle on {0} and {0, 2}, nowhere else."""
    diff = np.zeros(7, dtype=np.int64)
    want = np.zeros(7, dtype=np.int64)
    for name in SETS:
        T = NT.build_set(name)
        p = NT.f_pattern(T.cond_f[0])
        emu = NT.diff_form_draw(T.cond_f[0], NT.f_uniforms(T))
        assert np.array_equal(emu[p == -1], T.f1[p == -1]), name
        for i in range(7):
            diff[i] += (emu != T.f1)[p == i].sum()
        want[0] += ((p == 0) & (T.f1 == 1)).sum()
        want[4] += (p == 4).sum()
    print("draws that differ, per pattern %s: %s" % (list(NT.PATTERNS), diff.tolist()))
    assert np.array_equal(diff, want) and want[0] >= 200 and want[4] >= 200
