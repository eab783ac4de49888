"""
NumPy restatement of the f pass's rule of decided edges (fcd_common.h: fcd_f_edge_mode, fcd_f_edge_delta; the bounds of
gibbs_f_records_kernel in fcd_gibbs.hip), operation for operation: the wave's butterfly sums, the outward roundings to fp32
and the fp32 error bound delta come out bit for bit, so a prediction of which tiles take the decided-tile path is exact.

Nothing here is fitted to the kernel's output: the constants are the header's, the arithmetic is the rule's.
"""
import numpy as np

T = 16.0                # FCD_F_SURE_T
DELTA_CAP = 0.03125     # FCD_F_SURE_DELTA_CAP
DRIFT = 6.0             # FCD_F_SURE_DRIFT
FT_W = 4                # columns of a pair-aligned tile (two rows)
F32 = np.float32


def edge_table(lM):
    """lM (C, U, 3 types, 3 cases) -> lMf (C, U, 3 cases, 2): log-odds of type 1 and 2 against type 0 (edge_tables_kernel)"""
    return np.stack([lM[:, :, 1, :] - lM[:, :, 0, :], lM[:, :, 2, :] - lM[:, :, 0, :]], axis=-1)


def wave_sum(v):
    """(..., 64) -> (...): the butterfly of fcd_wave_sum / fp_edge_bound (offsets 32, 16, ..., 1), in v's dtype"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def f32_down(x):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(F32)
        return np.where(f.astype(np.float64) > x, np.nextafter(f, F32(-np.inf)), f).astype(F32)


def f32_up(x):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(F32)
        return np.where(f.astype(np.float64) < x, np.nextafter(f, F32(np.inf)), f).astype(F32)


def edge_bounds(lMf):
    """-> a (C,) fp32: fp_edge_bound;  b (C, 6) fp32: lo1, hi1, lo2, hi2, lo12, hi12, NaN where an entry is not finite"""
    (C, U) = lMf.shape[:2]
    assert U <= 64
    with np.errstate(invalid="ignore", over="ignore"):
        big = np.fmax.reduce(np.abs(lMf).astype(F32).reshape(C, U, 6), axis=2, initial=F32(0))        # (fmaxf skips a NaN)
        lane_a = np.zeros((C, 64), dtype=F32)
        lane_a[:, :U] = big * F32(1.0000002)
        a = wave_sum(lane_a)
        v = np.stack([lMf[..., 0], lMf[..., 1], lMf[..., 0] - lMf[..., 1]], axis=-1)          # (C, U, case, 3)
        lanes = np.zeros((C, 64, 6))
        lanes[:, :U, 0::2] = v.min(axis=2)
        lanes[:, :U, 1::2] = v.max(axis=2)
        s = wave_sum(np.moveaxis(lanes, 1, 2))                                                 # (C, 6)
        slack = 8e-15 * a.astype(np.float64)
        b = np.empty((C, 6), dtype=F32)
        b[:, 0::2] = f32_down(s[:, 0::2] - slack[:, None])
        b[:, 1::2] = f32_up(s[:, 1::2] + slack[:, None])
    b[~np.isfinite(lMf).all(axis=(1, 2, 3))] = np.nan
    return a, b


def edge_delta(c1, c2, U, a):
    """fcd_f_edge_delta: the fp32 bound on the error of the term loop's sums, in fp32 as the kernel computes it"""
    npair = (U + 1) // 2
    with np.errstate(invalid="ignore", over="ignore"):
        cm = np.fmax(np.abs(c1).astype(F32), np.abs(c2).astype(F32)) * F32(1.0000002)
        sum_err = F32(npair + 1) * F32(5.97e-8) * F32(1.01) * a
        off_err = F32(2.0) * F32(5.97e-8) * F32(1.01) * (cm + a)
        return sum_err + off_err


def edge_modes(S_B, lng, U, a, b, t=T):
    """fcd_f_edge_mode of every edge at ln gamma = lng: -> (C,) int, the decided mode or -1"""
    lg1, lg2 = lng[1] - lng[0], lng[2] - lng[0]
    with np.errstate(invalid="ignore", over="ignore"):
        c1 = lg1 + (S_B[:, 1] - S_B[:, 0])
        c2 = lg2 + (S_B[:, 2] - S_B[:, 0])
        ok = edge_delta(c1, c2, U, a) <= F32(DELTA_CAP)
        c12 = c1 - c2
        bd = b.astype(np.float64)
        m0 = (-(c1 + bd[:, 1]) > t) & (-(c2 + bd[:, 3]) > t)
        m1 = (c1 + bd[:, 0] > t) & (c12 + bd[:, 4] > t)
        m2 = (c2 + bd[:, 2] > t) & (-(c12 + bd[:, 5]) > t)
    mode = np.where(m0, 0, np.where(m1, 1, np.where(m2, 2, -1)))
    return np.where(ok, mode, -1)


def tiles(N):
    """the pair-aligned tiles of the triangle (fpt_locate): a list of int arrays of edge ids, possibly empty"""
    out = []
    for i in range((N + 1) // 2):
        n0 = 2 * i
        for j in range(i // 2 + 1):
            mb = FT_W * j
            ids = []
            for n in (n0, n0 + 1):
                if n < N:
                    ids += [n * (n - 1) // 2 + m for m in range(mb, min(mb + FT_W, n))]
            out.append(np.array(ids, dtype=np.int64))
    return out


def decided_tiles(N, mode):
    """the tiles (as edge-id arrays) with at least one edge and every edge decided"""
    return [t for t in tiles(N) if len(t) and (mode[t] >= 0).all()]


def hint(N, S_B, lng, U, a, b):
    """the word the record build leaves: some tile is decided at the call's starting hyper with DRIFT nats in hand"""
    return len(decided_tiles(N, edge_modes(S_B, lng, U, a, b, T - DRIFT))) > 0


def in_range(xw):
    """fcd_draw_f_sure's range test of a Philox word, in fp32"""
    xf = np.asarray(xw, dtype=np.uint32).astype(F32) * F32(2.3283064e-10)
    return (xf > F32(1e-6)) & (xf < F32(0.999999))


def philox_words(idx, chain, sweep, kind, seed):
    """Philox4x32-10 of the counters (idx, chain, sweep, kind) (broadcast uint arrays), key = seed: -> (..., 4) uint32"""
    M = np.uint64(0xFFFFFFFF)
    (c0, c1, c2, c3) = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (idx, chain, sweep, kind)])
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        (c0, c1, c2, c3) = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M)
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def predict(N, U, G, chain0, seed, S_B, lMf, lng_start, sweeps):
    """
    What a call's pair-tile f passes count: `sweeps` = [(sweep number, ln gamma of that sweep)] of the passes on the record
    table.  -> (f_sure_passes, f_sure_tiles, f_sure_fallbacks).  A tile here is a workgroup: a pair-aligned tile x a group of
    16 chain words; it goes back where any of its 64-chain words draws a uniform outside fcd_draw_f_sure's range for any edge.
    """
    (a, b) = edge_bounds(lMf)
    if not hint(N, S_B, lng_start, U, a, b):
        return (0, 0, 0)
    GW = (G + 63) // 64
    (n_sure, n_back) = (0, 0)
    for (sweep, lng) in sweeps:
        mode = edge_modes(S_B, lng, U, a, b)
        for t in decided_tiles(N, mode):
            blocks = np.unique(t >> 2)
            for y in range((GW + 15) // 16):
                chains = chain0 + np.arange(64 * 16 * y, 64 * min(GW, 16 * (y + 1)), dtype=np.int64)
                w = philox_words(blocks[:, None], chains[None, :], sweep, 2, seed)           # (blocks, chains, 4)
                ok = in_range(w)
                pos = np.searchsorted(blocks, t >> 2)
                if ok[pos, :, t & 3].all():
                    n_sure += 1
                else:
                    n_back += 1
    return (len(sweeps), n_sure, n_back)


def margins(S_B, lng, b):
    """(C, 3): what each mode's two comparisons of fcd_f_edge_mode leave over 0 (the smaller of the two); decided iff > T"""
    c1 = (lng[1] - lng[0]) + (S_B[:, 1] - S_B[:, 0])
    c2 = (lng[2] - lng[0]) + (S_B[:, 2] - S_B[:, 0])
    c12 = c1 - c2
    bd = b.astype(np.float64)
    return np.stack([np.minimum(-(c1 + bd[:, 1]), -(c2 + bd[:, 3])), np.minimum(c1 + bd[:, 0], c12 + bd[:, 4]),
                     np.minimum(c2 + bd[:, 2], -(c12 + bd[:, 5]))], axis=1)


def place_margin(S_B, c, m, lng, b, target):
    """a copy of S_B with S_B[c][m] shifted so that edge c's margin for mode m becomes `target` (both comparisons move alike)"""
    out = S_B.copy()
    out[c, m] += target - margins(S_B, lng, b)[c, m]
    return out
