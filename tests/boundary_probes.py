"""
Probe builder for the sampler's fast draws (tests/test_boundary_probes.py pins it on the CPU, tests/test_gpu_draw_boundaries.py
runs the kernels on what it builds).

The device kernels promise the draws of the exact fp64 formulas (fcd_draw_f / fcd_draw_r of fcd_common.h, draw_f / draw_r of the
oracle) although their hot paths decide most draws in fp32 and repeat only the "ambiguous" ones.  The tables made here put
draws ON PURPOSE at known distances inside and outside those margins:

  f probes     one per edge c, for ONE target chain: S_B[c, 1] and S_B[c, 2] are set so that the nearer threshold of the inverse
               CDF (0|1 or 1|2) lies at a prescribed signed distance d = (x sum(w) - T) / sum(w) from the target's own uniform
               x -- the quantity oracle_gibbs_f_step_m reports.  The other chains of the edge see the same tables at other r
               states: ordinary draws.
  sure probes  (the extreme-uniform scan) edges whose target draw has x < 1e-4 or x > 1 - 1e-4: the mode leads the runner-up by
               12 .. 18 nats, straddling the 15.01 + eta of fcd_draw_f_sure, with the small mass on the side of x -- the
               exact outcome is then sometimes NOT the argmax.
  floor probes (same scan) x > 1 - 1e-4, mode 0 with p0 = x - d, |d| in [1e-10, 1e-6]: the conditional is all but one-hot, so
               the eta term of the margin vanishes and only FCD_DRAW_F_MARGIN covers the fp32 roundings of x, sum and product.
  r probes     one per site (n, u) outside the last region, for one target chain, built in the order of the pass: an offset t
               on lM[c(n, m*), u, :, l(1, r_m*)] for one partner m* > n makes v - logit(x) the prescribed value.  The same t
               on all three k leaves every f log-odds unchanged in exact arithmetic, so both kinds live in one pair of tables.

All distances are evaluated in long double (64-bit mantissa) from the FINAL fp64 tables.  Uniforms are the sampler's own
(the Philox counters of oracle/fcdiff_oracle.py's site_uniform32 / site_uniform, vectorised here).  Nothing in this module needs a GPU.
"""
import functools

import numpy as np

from oracle import c_oracle as CO

LD = np.longdouble
KIND_F, KIND_R = 2, 3
EDGE_SYMMETRIC = 1
U64 = np.uint64
_M32 = U64(0xFFFFFFFF)

F_DMAX, R_DMAX = 3e-2, 1e-2          # largest prescribed distances of the issue's ranges
F_DMIN, R_DMIN = 1e-10, 1e-9         # smallest ones, where the oracle's own fp64 sums resolve them (see f_/r_resolution)
LM_MAX = 3000.0


# ------------------------------------------------------------------------------------------------
# the sampler's uniforms, vectorised
# ------------------------------------------------------------------------------------------------
def philox_vec(c0, c1, c2, c3, seed):
    """Philox4x32-10 on broadcastable counter arrays; returns four uint64 arrays holding 32-bit words."""
    (c0, c1, c2, c3) = np.broadcast_arrays(*[np.asarray(c, dtype=U64) & _M32 for c in (c0, c1, c2, c3)])
    (k0, k1) = (U64(seed & 0xFFFFFFFF), U64((seed >> 32) & 0xFFFFFFFF))
    (m0, m1, w0, w1) = (U64(0xD2511F53), U64(0xCD9E8D57), U64(0x9E3779B9), U64(0xBB67AE85))
    s32 = U64(32)
    for _ in range(10):
        p0 = m0 * c0
        p1 = m1 * c2
        (c0, c1, c2, c3) = ((p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + w0) & _M32
        k1 = (k1 + w1) & _M32
    return (c0, c1, c2, c3)


def f_words(seed, C, chains, sweep):
    """(G, C) uint64: the 32-bit word edge c of each chain draws in the f pass of `sweep` (x = word * 2^-32)."""
    chains = np.asarray(chains, dtype=U64)
    blk = np.arange((C + 3) // 4, dtype=U64)
    w = philox_vec(blk[None, :], chains[:, None], sweep, KIND_F, seed)
    return np.stack(w, axis=2).reshape(len(chains), -1)[:, :C]


def r_uniforms(seed, Nreg, U, chains, sweep):
    """(G, Nreg, U) float64: the 53-bit uniform site (n, u) of each chain draws in the r pass of `sweep`."""
    chains = np.asarray(chains, dtype=U64)
    U2 = (U + 1) >> 1
    idx = np.arange(Nreg * U2, dtype=U64)
    (x0, x1, x2, x3) = philox_vec(idx[None, :], chains[:, None], sweep, KIND_R, seed)
    s11 = U64(11)
    h0 = (((x0 << U64(32)) | x1) >> s11).astype(np.float64) * (1.0 / 9007199254740992.0)
    h1 = (((x2 << U64(32)) | x3) >> s11).astype(np.float64) * (1.0 / 9007199254740992.0)
    both = np.stack([h0, h1], axis=2).reshape(len(chains), Nreg, 2 * U2)
    return np.ascontiguousarray(both[:, :, :U])


# ------------------------------------------------------------------------------------------------
# exact (long double) evaluations
# ------------------------------------------------------------------------------------------------
def edge_pairs(Nreg):
    """n[c], m[c] of c = n (n - 1) / 2 + m, n > m."""
    n = np.repeat(np.arange(Nreg), np.arange(Nreg))
    m = np.concatenate([np.arange(k) for k in range(Nreg)]) if Nreg > 1 else np.zeros(0, dtype=np.int64)
    return n.astype(np.int64), m.astype(np.int64)


def mix_index(rn, rm):
    """0: neither region anomalous, 1: both, 2: exactly one."""
    return np.where((rn & rm) != 0, 1, np.where((rn ^ rm) != 0, 2, 0))


def f_logits_ld(S_B, lM, lng, r_rows, edges):
    """Long-double log-weights a_k of `edges` (array of c) at the r states r_rows (len(edges), Nreg, U)."""
    (en, em) = edge_pairs(r_rows.shape[1])
    U = lM.shape[1]
    k = np.arange(len(edges))
    l = mix_index(r_rows[k, en[edges], :], r_rows[k, em[edges], :])                        # (E, U)
    terms = lM[edges[:, None], np.arange(U)[None, :], :, l].astype(LD)                     # (E, U, 3)
    return lng.astype(LD)[None, :] + (S_B[edges].astype(LD) + terms.sum(axis=1))


def f_distance_ld(a, x):
    """For log-weights a (E, 3) and uniforms x (E,): signed relative distance to the NEARER threshold, which threshold
    (0: 0|1, 1: 1|2), the exact outcome, and the distance to the farther threshold."""
    a = a.astype(LD)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    s = e.sum(axis=1)
    d0 = (x.astype(LD) * s - e[:, 0]) / s
    d1 = (x.astype(LD) * s - (e[:, 0] + e[:, 1])) / s
    near1 = np.abs(d1) < np.abs(d0)
    out = np.where(d0 < 0, 0, np.where(d1 < 0, 1, 2))
    return np.where(near1, d1, d0), near1.astype(np.int64), out, np.where(near1, d0, d1)


def sym_edge(n, m):
    (a, b) = (np.maximum(n, m), np.minimum(n, m))
    return a * (a - 1) // 2 + b


def r_v_ld(lM, lnpi2, f_row, r_col, n, u):
    """Exact v = s1 - s0 of site (n, u) for one chain: f_row (C,), r_col (Nreg,) = the r_{m,u} as they stand."""
    Nreg = len(r_col)
    m = np.array([q for q in range(Nreg) if q != n], dtype=np.int64)
    c = sym_edge(n, m)
    rm = r_col[m]
    l1 = np.where(rm != 0, 1, 2)
    l0 = np.where(rm != 0, 2, 0)
    p = lM[c, u, f_row[c], :].astype(LD)                                                  # (Nreg - 1, 3)
    k = np.arange(len(m))
    return (LD(lnpi2[1]) - LD(lnpi2[0])) + (p[k, l1] - p[k, l0]).sum()


def logit_ld(x):
    x = LD(x)
    return np.log(x / (LD(1) - x))


# ------------------------------------------------------------------------------------------------
# what fp64 re-ordering can move (the smallest distance a regime may prescribe is 1000 x this)
# ------------------------------------------------------------------------------------------------
def f_resolution(S_B, lM, lng):
    """Bound on what any order of fp64 additions can move a relative f distance: each of the U + 2 additions of a_k errs by
    at most 2^-53 times a partial sum <= B_c = |ln gamma| + |S_B| + sum_u max |lM|; a log-odds b_k = a_k - a_0 then moves by
    at most 2 (U + 2) 2^-53 B, and a threshold p (1 - p) <= 1/4 times that."""
    B = np.abs(lng).max() + np.abs(S_B).max(axis=1) + np.abs(lM).max(axis=(2, 3)).sum(axis=1)
    return 0.5 * (lM.shape[1] + 2) * 2.0 ** -53 * float(B.max())


def r_resolution(lM, lnpi2, Nreg):
    """The same for v = s1 - s0: two sums of Nreg terms, partial sums <= B = |ln pi| + sum_m max |lM| of the worst site."""
    A = np.abs(lM).max(axis=(2, 3))                                                       # (C, U)
    worst = 0.0
    for n in range(Nreg):
        m = np.array([q for q in range(Nreg) if q != n])
        worst = max(worst, float(A[sym_edge(n, m)].sum(axis=0).max()))
    return 2.0 * (Nreg + 1) * 2.0 ** -53 * (np.abs(lnpi2).max() + worst)


# ------------------------------------------------------------------------------------------------
# base tables of the four regimes
# ------------------------------------------------------------------------------------------------
GAMMA = np.array([0.1, 0.8, 0.1])
PI2 = np.array([0.95, 0.05])
REGIMES = ("weak", "model", "heavy", "shared")


def base_tables(regime, Nreg, U, seed):
    """(S_B (C, 3), lM (C, U, 3, 3)) before any probe."""
    C = Nreg * (Nreg - 1) // 2
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    if regime == "weak":
        return rng.normal(size=(C, 3)), rng.normal(size=(C, U, 3, 3)) * 0.05
    if regime == "model":
        import fcdiff_amd
        m = fcdiff_amd.UnsharedRegionModel()
        (_r, _t, _f, _ft, b, bt) = m.sample_fast(Nreg, 3, U, seed=seed)
        return CO.lik_tables(b, bt, m.theta())
    if regime == "heavy":
        # large entries of both signs: the sums over the patients nearly cancel, the fp32 error is largest against the log-odds
        return rng.normal(size=(C, 3)), rng.uniform(0.0, 40.0, size=(C, U, 3, 3)) * rng.choice([-1.0, 1.0], size=(C, U, 3, 3))
    if regime == "shared":
        # patient-summed tables of the shared-region fit (U = 1, L of 100 - 1000 patients): every entry in -[100, 3000].
        # The level differs by hundreds to thousands of nats between the three types k (what the f pass subtracts in fp32);
        # between the mixture cases l of one type it differs by tens, so that ONE offset within |lM| <= 3000 can carry an r
        # site to its threshold.
        assert U == 1
        level = rng.uniform(200.0, 2800.0, size=(C, 1, 3, 1))
        return rng.normal(size=(C, 3)), -(level + rng.uniform(-60.0, 60.0, size=(C, 1, 3, 3)))
    raise ValueError(regime)


# ------------------------------------------------------------------------------------------------
# the builder
# ------------------------------------------------------------------------------------------------
class Probes:
    """Tables, initial state, the oracle's state after the probed sweep, and the probe lists (dicts of equal-length arrays)."""


def _log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))


def _place_f(S_B, lM, lng, r0, edges, chains, p):
    """Set S_B[c, 1:3] of `edges` so that the target chains' conditional is p (E, 3), in long double; rounded to fp64."""
    S_B[edges, 1:] = 0.0
    a = f_logits_ld(S_B, lM, lng, r0[chains], edges)               # with S_B[c, 1:] = 0
    p = p.astype(LD)
    for k in (1, 2):
        S_B[edges, k] = (np.log(p[:, k] / p[:, 0]) - (a[:, k] - a[:, 0])).astype(np.float64)


def _build_once(regime, Nreg, U, G, seed, sweep, f_range, r_range, scan, chain0):
    """
    Tables with one f probe per edge and one r probe per site outside the last region, for the sweep `sweep` from the state
    gibbs_init(pi = 0.3) leaves.  scan=True: the edges whose draw has an extreme uniform in some chain carry a sure / floor
    probe for that chain instead (the extreme-uniform scan; meant for G = 2048).  A probe that cannot be placed (a zero
    word, a threshold outside (0, 1), the other threshold not farther than 2 |d|, no partner whose entry stays within
    |lM| <= 3000) is dropped and counted in .dropped, never forced.
    """
    rng = np.random.default_rng([seed, Nreg, U, G, 77])
    C = Nreg * (Nreg - 1) // 2
    (S_B, lM) = base_tables(regime, Nreg, U, seed)
    S_B = np.ascontiguousarray(S_B, dtype=np.float64).copy()
    lM = np.ascontiguousarray(lM, dtype=np.float64).copy()
    assert np.isfinite(lM).all() and np.abs(lM).max() <= LM_MAX
    (lng, lnpi2) = (np.log(GAMMA), np.log(PI2))
    chains = chain0 + np.arange(G)
    (f0, r0) = CO.gibbs_init(G, Nreg, U, 0.3, seed, chain0)
    P = Probes()
    (P.regime, P.Nreg, P.U, P.G, P.seed, P.sweep, P.chain0, P.C) = (regime, Nreg, U, G, seed, sweep, chain0, C)
    (P.gamma, P.pi2, P.lng, P.lnpi2, P.f0, P.r0) = (GAMMA, PI2, lng, lnpi2, f0, r0)
    P.dropped = {"f": 0, "r": 0}

    # the smallest distances this regime may prescribe: three decades above what fp64 re-ordering can move.  The S_B
    # shifts and r offsets about double the magnitudes of the base tables: bounded with a factor 2 here, checked on the
    # final tables by the tests
    S_est = np.abs(S_B) + np.abs(lM).max(axis=(2, 3)).sum(axis=1)[:, None] + 40.0
    f_min = max(f_range[0], 1e3 * f_resolution(S_est, lM, lng))
    r_min = max(r_range[0], 1e3 * (2.0 * r_resolution(lM, lnpi2, Nreg) + 2.0 * (Nreg + 1) * 2.0 ** -53 * 40.0))
    (P.f_min, P.r_min) = (f_min, r_min)

    # ---- f probes -------------------------------------------------------------------------------
    words = f_words(seed, C, chains, sweep)                          # (G, C)
    xs = words.astype(np.float64) * (1.0 / 4294967296.0)
    edges = np.arange(C)
    tgt = (edges * 37 + 5 + seed) % G                                # rotates over every lane of every word, the partial last one too
    kind = np.zeros(C, dtype=np.int64)                               # 0 f, 1 sure, 2 floor
    if scan:
        ext = np.argwhere((xs < 1e-4) | (xs > 1 - 1e-4))            # (g, c), a few hundred
        xe = xs[ext[:, 0], ext[:, 1]]
        tail = np.minimum(xe, 1.0 - xe)
        # one probe per edge: the draw nearest the 1e-6 bound of fcd_draw_f_sure wins its edge
        order = np.argsort(np.abs(np.log(np.maximum(tail, 1e-12) / 1e-6)))
        seen = set()
        for i in order:
            (g, c) = ext[i]
            if c in seen:
                continue
            seen.add(c)
            tgt[c] = g
            # above 1 - 1e-4 every other edge tests the floor of the margin instead of the short-cut; the handful next to
            # the 1e-6 bound always tests the short-cut
            near = 5e-7 < tail[i] < 6e-6
            kind[c] = 2 if (xe[i] > 0.5 and not near and (len(seen) & 1)) else 1
        P.n_extreme = len(ext)
    x = xs[tgt, edges]
    thr = rng.integers(0, 2, size=C)
    sign = rng.choice([-1.0, 1.0], size=C)
    dmag = _log_uniform(rng, f_min, f_range[1], C)
    d = sign * dmag
    # the split of the mass on the far side of the probed threshold: comparable weights for one half of the edges, one
    # weight small (down to 1e-4 of that mass) for the other
    alpha = np.where(rng.random(C) < 0.5, rng.uniform(0.2, 0.8, size=C), 10.0 ** -rng.uniform(1.0, 4.0, size=C))
    alpha = np.where(rng.random(C) < 0.5, alpha, 1.0 - alpha)
    q = x.astype(LD) - d.astype(LD)                                  # the threshold T / sum(w)

    def far_side(al):                                                # distance to the threshold that is not probed
        return np.where(thr == 0, (1 - q) * al - d, q * (1 - al) + d)
    # (a split that would bring the other threshold within 2 |d| gives way to an even one: the probe keeps its distance)
    alpha = np.where(np.abs(far_side(alpha).astype(np.float64)) > 2.0 * dmag, alpha, 0.5)
    p = np.zeros((C, 3), dtype=LD)
    p[:, 0] = np.where(thr == 0, q, q * alpha)
    p[:, 1] = np.where(thr == 0, (1 - q) * alpha, q * (1 - alpha))
    p[:, 2] = 1 - p[:, 0] - p[:, 1]
    other = far_side(alpha)
    lead = np.zeros(C)
    # sure probes: mode leads the runner-up by L nats, the third weight 5 nats further down; runner-up on the side of x
    ks = np.flatnonzero(kind == 1)
    if len(ks):
        xk = x[ks]
        low = xk < 0.5
        L = _log_uniform(rng, 12.0, 18.0, len(ks))
        tailk = np.where(low, xk, 1.0 - xk)
        near = (tailk > 5e-7) & (tailk < 6e-6)
        # the handful next to the bound: the lead is placed about the draw's own flip point -ln(tail), inside [12.6, 18]
        # (0.6 nats above 12, so that the other chains of the wave -- same S_B, other r -- lead by more than 12 as well),
        # so that both outcomes (argmax and not) occur among them
        nn = int(near.sum())
        if nn:
            off = np.linspace(-1.0, 1.5, nn)[rng.permutation(nn)]
            L[near] = np.clip(-np.log(tailk[near]) + off, 12.6, 18.0)
        mode = np.where(low, rng.integers(1, 3, size=len(ks)), rng.integers(0, 2, size=len(ks)))
        small = np.where(low, 0, 2)
        third = 3 - mode - small
        w = np.zeros((len(ks), 3), dtype=LD)
        w[np.arange(len(ks)), mode] = 1
        w[np.arange(len(ks)), small] = np.exp(-L.astype(LD))
        w[np.arange(len(ks)), third] = np.exp(-(L.astype(LD) + 5))
        p[ks] = w / w.sum(axis=1, keepdims=True)
        lead[ks] = L
        # their distance, nearer threshold and outcome follow from p and x alone
        (dk, tk, ok_, _o) = f_distance_ld(np.log(p[ks]), xk)
        (d[ks], thr[ks]) = (dk.astype(np.float64), tk)
        sure_out = ok_
    kf = np.flatnonzero(kind == 2)
    if len(kf):
        dm = rng.choice([-1.0, 1.0], size=len(kf)) * _log_uniform(rng, F_DMIN, 1e-6, len(kf))
        qf = x[kf].astype(LD) - dm.astype(LD)
        p[kf, 0] = qf
        p[kf, 1] = (1 - qf) * LD(0.5)
        p[kf, 2] = 1 - p[kf, 0] - p[kf, 1]
        d[kf] = dm
        thr[kf] = 0
        other[kf] = (1 - qf) * LD(0.5) - dm
    ok = (words[tgt, edges] != 0) & (p.min(axis=1) > 0) & (p.max(axis=1) < 1)
    ok &= (kind == 1) | (np.abs(other.astype(np.float64)) > 2.0 * np.abs(d))
    P.dropped["f"] = int((~ok).sum())
    pe = edges[ok]
    _place_f(S_B, lM, lng, r0, pe, tgt[ok], p[ok])
    P.S_B_base = S_B.copy()

    # ---- the oracle's f step on these tables ----------------------------------------------------
    f1 = f0.copy()
    CO.gibbs_f_step(f1, r0, S_B, lM, lng, seed, sweep, chain0)

    # ---- r probes, site by site in the order of the pass ----------------------------------------
    xr = r_uniforms(seed, Nreg, U, chains, sweep)                    # (G, Nreg, U)
    with np.errstate(divide="ignore"):
        lgx = np.abs(np.log(xr / (1.0 - xr)))
    sites_n = Nreg - 1
    rt = ((np.arange(sites_n)[:, None] * 29 + np.arange(U)[None, :] * 11 + 3 + seed) % G).astype(np.int64)
    extreme = np.zeros((sites_n, U), dtype=bool)
    n_ext = (sites_n * U + 9) // 10                                  # a tenth: the sites of the most extreme uniforms of the scan
    flat = np.argsort(-np.where(np.isfinite(lgx[:, :sites_n, :]), lgx[:, :sites_n, :], -1.0), axis=None)
    for i in flat:
        (g, n, u) = np.unravel_index(i, (G, sites_n, U))
        if not extreme[n, u]:
            extreme[n, u] = True
            rt[n, u] = g
            n_ext -= 1
            if n_ext == 0:
                break
    rsign = rng.choice([-1.0, 1.0], size=(sites_n, U))
    rdel = rsign * _log_uniform(rng, r_min, r_range[1], (sites_n, U))
    rp = {k: [] for k in ("n", "u", "chain", "d", "outcome", "extreme", "partner")}
    lM_f = lM.copy()                                                 # the tables of the f probes alone
    r_new = r0.copy()
    for n in range(sites_n):
        if n > 0:
            r_new = r0.copy()
            CO.gibbs_r_step(f1, r_new, lM, lnpi2, seed, sweep, EDGE_SYMMETRIC, chain0)   # rows < n are final by now
        for u in range(U):
            g = rt[n, u]
            xx = xr[g, n, u]
            col = np.concatenate([r_new[g, :n, u], r0[g, n:, u]])
            if not (0.0 < xx < 1.0):
                P.dropped["r"] += 1
                continue
            t = (logit_ld(xx) + LD(rdel[n, u])) - r_v_ld(lM, lnpi2, f1[g], col, n, u)
            placed = False
            for j in range(Nreg - 1 - n):
                ms = n + 1 + (n * 7 + u * 3 + j) % (Nreg - 1 - n)
                c = sym_edge(ms, n)
                l1 = 1 if col[ms] else 2
                new = (lM[c, u, :, l1].astype(LD) + t).astype(np.float64)
                if np.abs(new).max() <= LM_MAX:
                    lM[c, u, :, l1] = new
                    placed = True
                    break
            if not placed:
                P.dropped["r"] += 1
                continue
            for (k, v) in zip(("n", "u", "chain", "d", "outcome", "extreme", "partner"),
                              (n, u, g, rdel[n, u], int(rdel[n, u] > 0), extreme[n, u], ms)):
                rp[k].append(v)
    r1 = r0.copy()
    CO.gibbs_r_step(f1, r1, lM, lnpi2, seed, sweep, EDGE_SYMMETRIC, chain0)
    # the f step once more, on the final tables: it must reproduce the first exactly
    f1b = f0.copy()
    CO.gibbs_f_step(f1b, r0, S_B, lM, lng, seed, sweep, chain0)
    P.f_step_unchanged = bool(np.array_equal(f1, f1b))
    (P.S_B, P.lM, P.lM_before_r, P.f1, P.r1) = (S_B, lM, lM_f, f1, r1)

    # the f probes as they stand in the FINAL tables: distance and outcome in long double
    a = f_logits_ld(S_B, lM, lng, r0[tgt[ok]], pe)
    (dd, near, out, _far) = f_distance_ld(a, x[ok])
    outcome = thr + (d > 0)
    if len(ks):
        outcome[ks] = sure_out
    P.f = dict(edge=pe, chain=tgt[ok], kind=kind[ok], thr=thr[ok], d=d[ok], d_final=dd.astype(np.float64), thr_final=near,
               outcome=outcome[ok], outcome_final=out, x=x[ok], lead=lead[ok], argmax=np.argmax(a, axis=1))
    P.r = {k: np.array(v) for (k, v) in rp.items()}
    # ... and the r probes: v - logit(x) in long double at the state the pass meets, from the final tables
    dfin = np.zeros(len(P.r["n"]))
    for (i, (n, u, g)) in enumerate(zip(P.r["n"], P.r["u"], P.r["chain"])):
        col = np.concatenate([r1[g, :n, u], r0[g, n:, u]])
        dfin[i] = float(r_v_ld(lM, lnpi2, f1[g], col, n, u) - logit_ld(xr[g, n, u]))
    P.r["d_final"] = dfin
    P.r["x"] = xr[P.r["chain"], P.r["n"], P.r["u"]] if len(dfin) else np.zeros(0)
    return P


def build(regime, Nreg, U, G, seed, sweep=0, f_range=(F_DMIN, F_DMAX), r_range=(R_DMIN, R_DMAX), scan=False, chain0=0):
    """_build_once, again with larger smallest distances where the FINAL tables (S_B shifts and r offsets included) turn
    out to resolve less than the estimate made from the base tables."""
    for _ in range(4):
        P = _build_once(regime, Nreg, U, G, seed, sweep, f_range, r_range, scan, chain0)
        (f_need, r_need) = (1e3 * f_resolution(P.S_B, P.lM, P.lng), 1e3 * r_resolution(P.lM, P.lnpi2, Nreg))
        if f_need <= P.f_min and r_need <= P.r_min:
            return P
        (f_range, r_range) = ((max(P.f_min, 1.25 * f_need), f_range[1]), (max(P.r_min, 1.25 * r_need), r_range[1]))
    raise RuntimeError("the smallest distances did not settle")


# ------------------------------------------------------------------------------------------------
# the table sets of the tests: (regime, Nreg, U, G, seed); shapes as small as reach each code path -- three blocks of 16
# regions with one region in the last (33) or one block (16); one patient, one pair, a half-empty last pair, the full
# U <= 64 kernel, the any-U kernel; two chain words and a partial one
# ------------------------------------------------------------------------------------------------
SETS = {
    "weak-33-7": ("weak", 33, 7, 130, 11), "weak-16-2": ("weak", 16, 2, 130, 12), "weak-33-70": ("weak", 33, 70, 130, 13),
    "model-33-7": ("model", 33, 7, 130, 21), "model-16-64": ("model", 16, 64, 130, 22), "model-33-2": ("model", 33, 2, 130, 23),
    "heavy-33-7": ("heavy", 33, 7, 130, 31), "heavy-16-70": ("heavy", 16, 70, 130, 32), "heavy-33-64": ("heavy", 33, 64, 130, 33),
    "shared-33-1": ("shared", 33, 1, 130, 41), "shared-16-1": ("shared", 16, 1, 130, 42),
}
# companions: every probe outside 1e-3 (f) / 1e-2 (r) -- the fast paths must decide nearly everything
FAR_SETS = {"weak-33-7-far": ("weak", 33, 7, 130, 51), "model-33-7-far": ("model", 33, 7, 130, 52)}
# the extreme-uniform scan
SCAN_SETS = {"scan-33-7": ("weak", 33, 7, 2048, 61), "scan-33-7b": ("weak", 33, 7, 2048, 62)}


@functools.lru_cache(maxsize=None)
def build_set(name):
    if name in FAR_SETS:
        return build(*FAR_SETS[name], f_range=(1e-3, F_DMAX), r_range=(1e-2, 1e-1))
    if name in SCAN_SETS:
        return build(*SCAN_SETS[name], scan=True)
    return build(*SETS[name])
