"""
The rule of decided edges of the f pass (fcd_common.h: fcd_f_edge_mode), through its NumPy restatement tests/f_sure_ref.py:
an edge it calls decided with mode m draws m in the oracle -- for the r states that attain each of its six bounds and for
random ones, for uniforms at both ends of fcd_draw_f_sure's range and random ones.  Tables with -inf or NaN entries are
never decided; an edge whose margin is placed at T + 1e-3 is decided, at T - 1e-3 it is not.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f_sure_ref as R  # noqa: E402

from oracle import c_oracle as CO  # noqa: E402
from oracle import fcdiff_oracle as O  # noqa: E402


def tables_for(N, H, U, seed):
    import fcdiff_amd
    m = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    S_B, lM = CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def test_constants_are_the_headers():
    src = open(os.path.join(HERE, "..", "fcdiff_amd", "csrc", "fcd_common.h")).read()

    def val(name):
        return float(re.search(r"#define\s+%s\s+([0-9.eE+-]+)f?\b" % name, src).group(1))
    assert (val("FCD_F_SURE_T"), val("FCD_F_SURE_DELTA_CAP"), val("FCD_F_SURE_DRIFT")) == (R.T, R.DELTA_CAP, R.DRIFT)
    assert R.T >= 15.01 + 0.065 + 7.1 * R.DELTA_CAP          # the derivation next to the rule


def words_at_the_range_ends():
    """the smallest and the largest Philox word inside fcd_draw_f_sure's range (fp32 test), found by bisection"""
    (lo, hi) = (0, 1 << 16)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        (lo, hi) = (lo, mid) if R.in_range(mid) else (mid, hi)
    first = hi
    (lo, hi) = ((1 << 32) - (1 << 16), (1 << 32) - 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        (lo, hi) = (mid, hi) if R.in_range(mid) else (lo, mid)
    last = lo
    assert R.in_range(first) and not R.in_range(first - 1) and R.in_range(last) and not R.in_range(last + 1)
    return first, last


def r_state_for(N, U, n, m, z):
    """an r state (N, U) whose mixture case for edge (n, m) is z[u] for patient u: 0 typical, 1 both, 2 discordant"""
    r = np.zeros((N, U), dtype=np.uint8)
    r[n, :] = (z != 0)
    r[m, :] = (z == 1)
    return r


@pytest.mark.parametrize("N,H,U,seed", [(8, 16, 1, 1), (8, 16, 5, 2), (9, 3, 3, 3), (9, 3, 7, 4), (7, 6, 64, 5), (6, 2, 2, 6)])
def test_decided_edges_draw_their_mode(N, H, U, seed):
    (m, S_B, lM) = tables_for(N, H, U, seed)
    lMf = R.edge_table(lM)
    (a, b) = R.edge_bounds(lMf)
    rng = np.random.RandomState(seed)
    (first, last) = words_at_the_range_ends()
    n_checked = 0
    for gamma in (m.gamma, np.array([1e-40, 1.0, 1e-40]), np.array([0.3, 1e-20, 0.7])):
        lng = np.log(gamma)
        mode = R.edge_modes(S_B, lng, U, a, b)
        for c in np.nonzero(mode >= 0)[0]:
            (n, mm) = O.c_to_nm(int(c))
            v = np.stack([lMf[c, :, :, 0], lMf[c, :, :, 1], lMf[c, :, :, 0] - lMf[c, :, :, 1]], axis=-1)      # (U, case, 3)
            states = [v[:, :, q].argmin(axis=1) for q in range(3)] + [v[:, :, q].argmax(axis=1) for q in range(3)]
            states += [rng.randint(0, 3, size=U) for _ in range(3)]
            for z in states:
                logits = O.f_conditional_logits(int(c), r_state_for(N, U, n, mm, z), S_B, lM, lng)
                lead = np.sort(logits)[-1] - np.sort(logits)[-2]
                assert lead > 15.0 and int(np.argmax(logits)) == mode[c], (c, z, logits, mode[c])
                for xw in (first, last, int(rng.randint(first, last))):
                    assert O.draw_f(logits, xw * (1.0 / 4294967296.0)) == mode[c], (c, z, xw)
                n_checked += 1
    assert n_checked > 0


def test_bounds_enclose_every_state():
    """lo <= sum_u d(z_u) <= hi for random states, on tables without any structure"""
    rng = np.random.RandomState(0)
    (C, U) = (20, 9)
    lMf = rng.normal(scale=30.0, size=(C, U, 3, 2))
    (a, b) = R.edge_bounds(lMf)
    bd = b.astype(np.float64)
    for _ in range(200):
        z = rng.randint(0, 3, size=(C, U))
        d = np.take_along_axis(lMf, z[:, :, None, None], axis=2)[:, :, 0, :].sum(axis=1)      # (C, 2)
        s = np.stack([d[:, 0], d[:, 1], d[:, 0] - d[:, 1]], axis=1)
        assert (bd[:, 0::2] <= s).all() and (s <= bd[:, 1::2]).all()
    assert (a >= np.abs(lMf).max(axis=(2, 3)).sum(axis=1)).all()


@pytest.mark.parametrize("bad", (-np.inf, np.nan, np.inf))
def test_tables_with_entries_that_are_not_finite_are_never_decided(bad):
    (m, S_B, lM) = tables_for(8, 16, 5, 2)
    lMf = R.edge_table(lM)
    (a, b) = R.edge_bounds(lMf)
    lng = np.log(m.gamma)
    before = R.edge_modes(S_B, lng, 5, a, b)
    assert (before >= 0).all()
    rng = np.random.RandomState(1)
    hit = rng.choice(len(before), size=6, replace=False)
    for (i, c) in enumerate(hit):
        lMf[c, rng.randint(5), i % 3, i % 2] = bad
    (a2, b2) = R.edge_bounds(lMf)
    after = R.edge_modes(S_B, lng, 5, a2, b2)
    assert (after[hit] == -1).all()
    assert (np.delete(after, hit) == np.delete(before, hit)).all()
    # ... and neither with S_B or gamma not finite
    S2 = S_B.copy()
    S2[hit[0], 1] = bad
    assert R.edge_modes(S2, lng, 5, a, b)[hit[0]] == -1
    with np.errstate(divide="ignore"):
        assert (R.edge_modes(S_B, np.log(np.array([0.5, 0.0, 0.5])), 5, a, b) == -1).all()


def test_delta_above_its_cap_is_never_decided():
    (m, S_B, lM) = tables_for(8, 16, 5, 2)
    (a, b) = R.edge_bounds(R.edge_table(lM))
    lng = np.log(m.gamma)
    S2 = S_B.copy()
    S2[:, 1] += 3e5                      # c1 = 3e5: type 1 leads by far, but delta = 1.2e-7 (cm + a) > 1/32
    assert (R.edge_modes(S2, lng, 5, a, b) == -1).all()
    S2 = S_B.copy()
    S2[:, 1] += 1e5
    assert (R.edge_modes(S2, lng, 5, a, b) == 1).all()


@pytest.mark.parametrize("want", (0, 1, 2))
def test_margin_at_the_threshold(want):
    (m, S_B, lM) = tables_for(9, 3, 3, 3)
    (a, b) = R.edge_bounds(R.edge_table(lM))
    lng = np.log(m.gamma)
    mode = R.edge_modes(S_B, lng, 3, a, b)
    c = int(np.nonzero(mode == want)[0][0])
    up = R.edge_modes(R.place_margin(S_B, c, want, lng, b, R.T + 1e-3), lng, 3, a, b)
    down = R.edge_modes(R.place_margin(S_B, c, want, lng, b, R.T - 1e-3), lng, 3, a, b)
    assert up[c] == want and down[c] == -1
    assert (np.delete(up, c) == np.delete(mode, c)).all() and (np.delete(down, c) == np.delete(mode, c)).all()


def test_tiles_cover_every_edge_once():
    for N in (2, 3, 5, 13, 18, 45):
        ids = np.concatenate(R.tiles(N))
        assert sorted(ids.tolist()) == list(range(N * (N - 1) // 2))
        assert len(R.tiles(N)) == (lambda i: (i // 2) * (i // 2 + 1) if i % 2 == 0 else (i // 2 + 1) ** 2)((N + 1) // 2)
