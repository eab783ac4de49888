"""
The r pass's rule of decided sites (tests/r_sure_ref.py, the NumPy restatement of fcd_common.h's R_SURE_T rule and of
gibbs_r_bounds_kernel) against the model itself, on the CPU:

  * brute force at Nreg <= 8, U = 2: for every r configuration of the other regions (and every f on an edge without a mode,
    where a decided row had one), a decided site's exact log-odds -- from the edge-major table, as the oracle sums them -- lie
    beyond +-16;
  * oracle chains at Nreg 64, H 16, U 16: no decided site whose row is at its modes and whose uniform lies in
    [1e-6, 1 - 1e-6] is ever drawn against the rule;
  * the decided share on the benchmark's tables (Nreg 200, H 50, U 50) is at least 0.9.
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_sure_ref as R  # noqa: E402
import r_sure_ref as RS  # noqa: E402


def tables_for(N, H, U, seed):
    import fcdiff_amd
    from oracle import c_oracle as CO
    m = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=seed)
    (S_B, lM) = CO.lik_tables(b, bt, m.theta())
    return m, S_B, lM


def off_of(m):
    return float(np.log(m.pi) - np.log(1.0 - m.pi))


def test_region_table_is_the_difference_of_the_oracles_sums():
    (N, U) = (5, 2)
    (m, S_B, lM) = tables_for(N, 16, U, seed=1)
    lMd = RS.region_table(lM, N)
    rng = np.random.default_rng(4)
    for _ in range(20):
        (n, u) = (int(rng.integers(N)), int(rng.integers(U)))
        (f_row, r_col) = (rng.integers(0, 3, size=N), rng.integers(0, 2, size=N))
        want = RS.exact_log_odds(lM, N, n, u, f_row, r_col, 0.25)
        got = 0.25 + sum(lMd[u, n, mm, f_row[mm], r_col[mm]] for mm in range(N) if mm != n)
        assert abs(want - got) < 1e-9 * (1.0 + abs(want))


def test_brute_force_small_tables():
    """every r state of the other regions: a decided site's exact log-odds are beyond the threshold; its base sum is the
    all-healthy state's.  Factors 4 and 16 on the tables put the share between none and all."""
    seen = 0
    for (N, factor, seed) in ((8, 4.0, 3), (8, 16.0, 3), (6, 8.0, 5), (3, 16.0, 7)):
        U = 2
        (m, S_B, lM) = tables_for(N, 16, U, seed=seed)
        (S_B, lM) = (factor * S_B, factor * lM)
        off = off_of(m)
        (km, lMd, hi, lo, base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
        (d0, d1) = RS.decided(hi, lo, off, rowflag)
        for n in range(N):
            if rowflag[n]:
                assert not (d0[n] | d1[n]).any()
                continue
            others = [mm for mm in range(N) if mm != n]
            for u in range(U):
                vs = []
                for bits in itertools.product((0, 1), repeat=N - 1):
                    r_col = np.zeros(N, dtype=np.int64)
                    r_col[others] = bits
                    vs.append(RS.exact_log_odds(lM, N, n, u, km[n], r_col, off))
                vs = np.array(vs)
                assert lo[n, u] - 1e-9 <= vs.min() - off and vs.max() - off <= hi[n, u] + 1e-9
                assert abs((vs[0] - off) - base[n, u]) < 1e-9 * (1.0 + abs(base[n, u]))
                if d0[n, u]:
                    assert vs.max() < -RS.T
                    seen += 1
                if d1[n, u]:
                    assert vs.min() > RS.T
                    seen += 1
    assert seen > 10


def test_a_row_with_an_open_edge_has_no_decided_site():
    """weak S_B on one edge leaves it without a mode: both its rows are flagged, their bounds take the extreme over all k"""
    (N, U) = (6, 2)
    (m, S_B, lM) = tables_for(N, 16, U, seed=5)
    (S_B, lM) = (16.0 * S_B, 16.0 * lM)
    c = 4 * 3 // 2 + 1
    S_B[c] = 0.0
    lM[c] *= 1e-3
    (km, lMd, hi, lo, base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
    assert km[4, 1] == 3 and km[1, 4] == 3 and rowflag[4] and rowflag[1] and rowflag.sum() == 2
    (d0, d1) = RS.decided(hi, lo, off_of(m), rowflag)
    assert not (d0 | d1)[[1, 4]].any() and (d0 | d1).any()
    assert np.isnan(base[[1, 4]]).all() and np.isfinite(hi).all()
    for f41 in range(3):
        f_row = km[4].copy()
        f_row[1] = f41
        for r1 in (0, 1):
            r_col = np.zeros(N, dtype=np.int64)
            r_col[1] = r1
            v = RS.exact_log_odds(lM, N, 4, 0, f_row, r_col, 0.0)
            assert lo[4, 0] - 1e-9 <= v <= hi[4, 0] + 1e-9


def test_non_finite_entries_make_nan_bounds():
    (N, U) = (6, 2)
    (m, S_B, lM) = tables_for(N, 16, U, seed=5)
    (S_B, lM) = (16.0 * S_B, 16.0 * lM)
    c = 3 * 2 // 2 + 0
    lM[c, 1] = -np.inf
    with np.errstate(invalid="ignore"):
        (km, lMd, hi, lo, base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
        (d0, d1) = RS.decided(hi, lo, off_of(m), rowflag)
    assert np.isnan(hi[3, 1]) and np.isnan(lo[0, 1]) and np.isnan(base[3, 1])
    assert not (d0 | d1)[[0, 3], 1].any()


def test_oracle_chains_never_draw_a_decided_site_against_the_rule():
    from oracle import c_oracle as CO
    (N, H, U, G, seed, chain0) = (64, 16, 16, 64, 11, 2)
    (m, S_B, lM) = tables_for(N, H, U, seed=3)
    (lng, lnpi2) = (np.log(m.gamma), np.log(m.pi2()))
    off = float(lnpi2[1] - lnpi2[0])
    (km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S_B, lM, lng)
    (d0, d1) = RS.decided(hi, lo, off, rowflag)
    assert 0.5 < (d0 | d1).mean() < 0.8
    E = RS.edge_ids(N)
    offdiag = ~np.eye(N, dtype=bool)
    (f, r) = CO.gibbs_init(G, N, U, 0.3, seed, chain0)
    checked = 0
    for s in range(4):
        CO.gibbs_f_step(f, r, S_B, lM, lng, seed, s, chain0)
        at_modes = ~((f[:, E] != km[None]) & offdiag[None]).any(axis=2)             # (G, N)
        CO.gibbs_r_step(f, r, lM, lnpi2, seed, s, 1, chain0)
        x = RS.uniforms(N, U, chain0 + np.arange(G), s, seed)                       # (N, U, G)
        ok = at_modes.T[:, None, :] & (x >= RS.X_LO) & (x <= 1.0 - RS.X_LO)
        rr = np.moveaxis(np.asarray(r).reshape(G, N, U), 0, 2).astype(bool)         # (N, U, G)
        assert not (rr & d0[:, :, None] & ok).any()
        assert not (~rr & d1[:, :, None] & ok).any()
        checked += int(((d0 | d1)[:, :, None] & ok).sum())
    assert checked > 0.5 * 4 * G * N * U * 0.6


def test_share_on_the_benchmarks_tables():
    (N, H, U) = (200, 50, 50)
    (m, S_B, lM) = tables_for(N, H, U, seed=0)
    (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
    assert not rowflag.any()
    s = RS.share(hi, lo, off_of(m), rowflag)
    print("decided share at Nreg 200, H 50, U 50:", s)
    assert s >= 0.9
