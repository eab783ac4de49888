"""
The device forward sampler (fcd_sample.hip: fcd_model_sample, fcd_model_sample_shared) restated in NumPy.

The sampler is counter-based: every output element is a function of (seed, index, kind) alone,
    x = Philox4x32-10(counter = (lo(i), hi(i), 0, kind), key = (lo(seed), hi(seed))),
so it can be compared element for element, not only through population means.

  kind 16  r    index n U + u (shared model: n)        r = u53(x0, x1) < pi
  kind 17  f    index c                                f = 0 if x < g0 else 1 if x < g01 else 2,
                                                       g0 = gamma0 / sum, g01 = (gamma0 + gamma1) / sum, sum = (gamma0 + gamma1) + gamma2
  kind 18  t    index c U + u                          0 if both regions typical, 1 if both anomalous, else x < eta
  kind 19  f~   index c U + u                          keep = epsilon if t else 1 - epsilon;  f~ = f if x < keep else
                                                       (f + 1 + [(x - keep) >= 0.5 (1 - keep)]) % 3
  kind 20  b    index c H + h                          clip(mu[f] + sigma[f] z),  z = sqrt(-2 log(1 - u53(x0, x1))) cos(2 pi u53(x2, x3))
  kind 21  b~   index c U + u                          the same around component f~

Edges are in the fitter's order c = n(n-1)/2 + m, n > m.  Integers and comparisons are exact here as there; log, sqrt
and cos are libm's here and the device library's there, a few ulp apart.
"""
import numpy as np

from oracle import fcdiff_oracle as O

(K_R, K_F, K_T, K_FT, K_B, K_BT) = (16, 17, 18, 19, 20, 21)

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = np.uint64(0x9E3779B9)
_W1 = np.uint64(0xBB67AE85)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays: every word is a uint64 array (or scalar) holding a 32-bit value; four uint64 arrays."""
    (c0, c1, c2, c3) = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _M32 for x in (c0, c1, c2, c3)])
    k0 = np.uint64(int(k0) & 0xFFFFFFFF)
    k1 = np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = _M0 * c0                  # < 2^64: 32 x 32 bits
        p1 = _M1 * c2
        (c0, c1, c2, c3) = ((p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32)
        k0 = (k0 + _W0) & _M32
        k1 = (k1 + _W1) & _M32
    return (c0, c1, c2, c3)


def u53(hi, lo):
    """53 high bits of the 64-bit word (hi, lo) as a double in [0, 1)."""
    w = (hi << _S32) | lo
    return (w >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def block(seed, idx, kind):
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed)
    return philox4x32_10(idx & _M32, idx >> _S32, 0, kind, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def uniform(seed, idx, kind):
    x = block(seed, idx, kind)
    return u53(x[0], x[1])


def normal(seed, idx, kind):
    x = block(seed, idx, kind)
    u1 = 1.0 - u53(x[0], x[1])
    u2 = u53(x[2], x[3])
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


Z_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -53)))          # 8.57: the largest |z| a 53-bit uniform can give


def sample(theta, N, H, U, seed, shared=False):
    """
    theta[12] = pi, eta, epsilon, gamma[3], mu[3], sigma[3].  Returns a dict:
    r (N, U) bool -- shared: (N,) --, t (C, U) bool, f (C,) and ft (C, U) component indices, b (C, H), bt (C, U).
    """
    theta = np.asarray(theta, dtype=np.float64)
    (pi, eta, eps) = (theta[0], theta[1], theta[2])
    gs = theta[3] + theta[4] + theta[5]
    g0 = theta[3] / gs
    g01 = (theta[3] + theta[4]) / gs
    (mu, sigma) = (theta[6:9], theta[9:12])
    ends = O.edge_endpoints(N)
    C = ends.shape[0]
    if shared:
        r = uniform(seed, np.arange(N), K_R) < pi
        (rn, rm) = (r[ends[:, 0]][:, None], r[ends[:, 1]][:, None])
    else:
        r = uniform(seed, np.arange(N * U).reshape(N, U), K_R) < pi
        (rn, rm) = (r[ends[:, 0]], r[ends[:, 1]])
    xf = uniform(seed, np.arange(C), K_F)
    f = np.where(xf < g0, 0, np.where(xf < g01, 1, 2))
    i = np.arange(C * U).reshape(C, U)
    t = np.where(rn ^ rm, uniform(seed, i, K_T) < eta, rn & rm)
    keep = np.where(t, eps, 1.0 - eps)
    x = uniform(seed, i, K_FT)
    other = (f[:, None] + 1 + ((x - keep) >= 0.5 * (1.0 - keep)).astype(np.int64)) % 3
    ft = np.where(x >= keep, other, f[:, None])
    bt = np.clip(mu[ft] + sigma[ft] * normal(seed, i, K_BT), -1.0, 1.0)
    j = np.arange(C * H).reshape(C, H)
    b = np.clip(mu[f][:, None] + sigma[f][:, None] * normal(seed, j, K_B), -1.0, 1.0)
    return dict(r=r, t=t.astype(bool), f=f, ft=ft, b=b, bt=bt)


def theta_of(pi, eta, epsilon, gamma, mu, sigma):
    return np.concatenate([[pi, eta, epsilon], gamma, mu, sigma]).astype(np.float64)


# the parameter sets of the tests: the one of test_model_sample_gpu_statistics, and one that reaches every branch's
# boundary -- epsilon = 0 (keep is 1 or 0: x >= keep never / always), eta = 1 (a discordant pair is always anomalous),
# gamma = (1, 0, 0) (g0 = g01 = 1: f = 0 everywhere) -- with wide components near the ends so that b and b~ reach the clip
THETA_USUAL = theta_of(0.3, 0.4, 0.2, [0.2, 0.5, 0.3], [-0.5, 0.0, 0.5], [0.05, 0.05, 0.05])
THETA_EDGE = theta_of(0.3, 1.0, 0.0, [1.0, 0.0, 0.0], [-0.9, 0.1, 0.9], [0.3, 0.2, 0.3])
THETAS = {"usual": THETA_USUAL, "edge": THETA_EDGE}
SHAPES = [(2, 1, 1), (2, 3, 300), (3, 2, 5), (23, 7, 11), (40, 6, 50)]
SEEDS = [1, (7 << 32) + 12345]            # the second one has a high key word
