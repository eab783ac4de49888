"""
Exact law of the many-chain Gibbs sampler on models small enough to enumerate.  TEST INFRASTRUCTURE ONLY (NumPy).

The sampler (oracle gibbs_init / gibbs_f_step / gibbs_r_step, and the HIP kernels bit-exact with them) is a Markov
chain on the joint states (f, r): f in {0,1,2}^C, r in {0,1}^(Nreg x U).  With Nreg <= 4 and U <= 2 there are at most
3^6 * 2^8 = 186 624 states, so the law of a chain after k sweeps,

    P_k = P_0 K^k,

is computed here in float64 without any sampling, and histograms of many independent chains can be tested against it
exactly at every k (no mixing assumption).

Everything is derived from the log joint alone, written out independently of the sampler's conditionals
(gibbs_logjoint / f_conditional_logits / r_conditional_logits are NOT used): fit.py:149-152 at one-hot q,

    ln p(f, r, b, bt) = sum_c (ln gamma_{f_c} + S_B[c, f_c]) + sum_{n,u} ln pi2[r_nu]
                        + sum_{c,u} lM[c, u, f_c, l(r_nu, r_mu)],      (n, m) = endpoints of c,

with l the mixture case of fit.py:402-405 / 437-443 (0 both typical, 1 both anomalous, 2 discordant).  Shared with the
sampler: the tables S_B and lM (pinned to the reference by G2), the edge index maps (G1) and that three-case definition.

A site update is the conditional of the joint: the log-joints of the states that differ only at the site, normalised
(a softmax along that state axis).  A sweep applies, to a distribution vector (the dense K is never formed):
  * the f block: every edge redrawn given r.  Given r the edges are conditionally independent (the joint is a sum of
    one term per edge), so updating them one edge at a time is the law of the simultaneous f pass;
  * then every r site, n outer, u inner -- the order of gibbs_r_step.  For a fixed u the scan is sequential in n (the
    in-order pass of fcd_gibbs_r.hip realises exactly that: block steps of 16 regions, in order inside a block); sites
    of different u are conditionally independent given f, so any interleaving of patients is the same law.
P_0: f uniform over {0,1,2}, r ~ Bernoulli(pi0), all independent (gibbs_init: min(int(3x), 2), x < pi0).  The sampler
draws those (and every later site) from 53-bit or 32-bit quantised uniforms; that moves any probability by less than
2^-32 per draw, far below what any test with 2^18 chains can see.

Symmetric edge ids only.  With the reference's edge ids (quirk Q1) the r conditionals of the sampler need not be the
conditionals of any joint distribution, so this module has nothing to say about that mode.
"""
import numpy as np

from . import fcdiff_oracle as O


def mix_case(rn, rm):
    """l of lM[c,u,k,l] (fit.py:402-405, 437-443): 0 both typical, 1 both anomalous, 2 discordant."""
    rn = np.asarray(rn)
    rm = np.asarray(rm)
    return np.where((rn == 1) & (rm == 1), 1, np.where(rn != rm, 2, 0))


class ExactChain(object):
    """
    The joint of one (Nreg, U) model and the sweep operator on distributions over its states.

    State axes (C-order): f_0 .. f_{C-1} (size 3 each), then r_{0,0}, r_{0,1}, .., r_{Nreg-1,U-1} (size 2 each), so the
    flat index of a state is numpy.ravel_multi_index of (f, r.reshape(-1)) -- see `state_index`.
    `r_order` (list of (n, u)) replaces the sampler's scan order and `f_first=False` draws the r sites BEFORE the f block;
    both exist only to build wrong laws for the power tests.
    """

    def __init__(self, S_B, lM, gamma, pi2, r_order=None, f_first=True):
        S_B = np.asarray(S_B, dtype=np.float64)
        lM = np.asarray(lM, dtype=np.float64)
        (self.C, self.U) = lM.shape[0:2]
        self.Nreg = int(round(O.C_to_N(self.C)))
        assert O.N_to_C(self.Nreg) == self.C and lM.shape == (self.C, self.U, 3, 3) and S_B.shape == (self.C, 3)
        self.NU = self.Nreg * self.U
        self.shape = (3,) * self.C + (2,) * self.NU
        self.n_states = int(np.prod(self.shape))
        self.lng = np.log(np.asarray(gamma, dtype=np.float64))
        self.lnpi2 = np.log(np.asarray(pi2, dtype=np.float64))
        self.r_order = [(n, u) for n in range(self.Nreg) for u in range(self.U)] if r_order is None else list(r_order)
        self.f_first = bool(f_first)
        self.L = self._logjoint(S_B, lM)
        self._cond = {}

    # ---- axes ----
    def f_axis(self, c):
        return c

    def r_axis(self, n, u):
        return self.C + n * self.U + u

    def _place(self, small, axes):
        """Broadcast `small` (one dimension per entry of `axes`, ascending) into the full state shape."""
        shp = [1] * len(self.shape)
        for (a, s) in zip(axes, small.shape):
            shp[a] = s
        return small.reshape(shp)

    # ---- joint ----
    def _logjoint(self, S_B, lM):
        L = np.zeros(self.shape)
        ends = O.edge_endpoints(self.Nreg)
        for c in range(self.C):
            L += self._place(self.lng + S_B[c], [self.f_axis(c)])
        for n in range(self.Nreg):
            for u in range(self.U):
                L += self._place(self.lnpi2.copy(), [self.r_axis(n, u)])
        rr = np.arange(2)
        for c in range(self.C):
            (n, m) = ends[c]
            for u in range(self.U):
                # t[k, r_m, r_n] = lM[c, u, k, l(r_n, r_m)]; axis of r_m < axis of r_n since m < n
                l = mix_case(rr[None, :], rr[:, None])                   # [r_m, r_n]
                t = lM[c, u][:, l]                                      # (3, 2, 2)
                L += self._place(t, [self.f_axis(c), self.r_axis(m, u), self.r_axis(n, u)])
        return L

    def logjoint_of(self, f, r):
        """Log joint of chains (f (G, C), r (G, Nreg, U)) read from the enumeration."""
        return self.L.reshape(-1)[self.state_index(f, r)]

    def state_index(self, f, r):
        f = np.asarray(f, dtype=np.int64)
        r = np.asarray(r, dtype=np.int64).reshape(f.shape[0], -1)
        cols = [f[:, c] for c in range(self.C)] + [r[:, j] for j in range(self.NU)]
        return np.ravel_multi_index(cols, self.shape)

    def all_states(self):
        """Every state as chains: f (S, C) uint8, r (S, Nreg, U) uint8, in flat-index order."""
        idx = np.unravel_index(np.arange(self.n_states), self.shape)
        f = np.stack(idx[:self.C], axis=1).astype(np.uint8)
        r = np.stack(idx[self.C:], axis=1).astype(np.uint8).reshape(self.n_states, self.Nreg, self.U)
        return f, r

    # ---- conditionals: differences of log-joints between neighbouring states ----
    def conditional(self, axis):
        """p(x_axis = v | rest) at every state, shape = self.shape (normalised along `axis`)."""
        p = self._cond.get(axis)
        if p is None:
            mx = np.max(self.L, axis=axis, keepdims=True)
            e = np.exp(self.L - mx)
            p = e / np.sum(e, axis=axis, keepdims=True)
            self._cond[axis] = p
        return p

    def f_logit_diffs(self, f, r):
        """(G, C, 3): L(state with f_c = k) - L(state with f_c = 0) at each chain's state."""
        out = np.zeros((f.shape[0], self.C, 3))
        for c in range(self.C):
            f2 = np.array(f, dtype=np.int64)
            f2[:, c] = 0
            base = self.logjoint_of(f2, r)
            for k in (1, 2):
                f2[:, c] = k
                out[:, c, k] = self.logjoint_of(f2, r) - base
        return out

    def r_logit_diffs(self, f, r):
        """(G, Nreg, U): L(state with r_nu = 1) - L(state with r_nu = 0) at each chain's state."""
        out = np.zeros((f.shape[0], self.Nreg, self.U))
        for n in range(self.Nreg):
            for u in range(self.U):
                r2 = np.array(r, dtype=np.int64)
                r2[:, n, u] = 1
                v1 = self.logjoint_of(f, r2)
                r2[:, n, u] = 0
                out[:, n, u] = v1 - self.logjoint_of(f, r2)
        return out

    # ---- laws ----
    def initial(self, pi0):
        P = np.ones(self.shape)
        for c in range(self.C):
            P = P * self._place(np.full(3, 1.0 / 3.0), [self.f_axis(c)])
        for j in range(self.NU):
            P = P * self._place(np.array([1.0 - pi0, pi0]), [self.C + j])
        return P

    def site_update(self, P, axis):
        """Law after redrawing the variable of `axis` from its conditional: P'(x) = sum_v P(x | x_axis = v) p(x_axis | rest)."""
        return np.sum(P, axis=axis, keepdims=True) * self.conditional(axis)

    def sweep(self, P):
        f_block = [self.f_axis(c) for c in range(self.C)]
        r_block = [self.r_axis(n, u) for (n, u) in self.r_order]
        for a in (f_block + r_block if self.f_first else r_block + f_block):
            P = self.site_update(P, a)
        return P

    def laws(self, pi0, ks):
        """{k: P_k} for every k of `ks` (flat float64 vectors, summing to 1)."""
        (out, P, done) = ({}, self.initial(pi0), 0)
        for k in sorted(ks):
            while done < k:
                P = self.sweep(P)
                done += 1
            out[k] = P.reshape(-1).copy()
        return out


# ----------------------------------------------------------------------------------------
# statistics of G independent chains against an exact law
# ----------------------------------------------------------------------------------------
def chi2_sf(x, dof):
    """Upper tail of chi^2(dof) by the Wilson-Hilferty cube-root normal approximation (a few % relative in the tails used
    here, dof >= 10)."""
    import math
    k = float(dof)
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def histogram(ec, f, r):
    """Number of chains in every state (flat, ec.n_states)."""
    return np.bincount(ec.state_index(f, r), minlength=ec.n_states).astype(np.float64)


def g_test(hist, P, min_expected=5.0):
    """
    G-test of a histogram of n chains against the law P: cells whose expected count n*P is below `min_expected` are
    merged into one cell (and that cell into the smallest other one if it is still below).  Returns (G, dof, p).
    """
    n = float(hist.sum())
    E = n * P
    small = E < min_expected
    (obs, exp) = (list(hist[~small]), list(E[~small]))
    if small.any():
        (o_s, e_s) = (float(hist[small].sum()), float(E[small].sum()))
        if e_s < min_expected and exp:
            j = int(np.argmin(exp))
            (obs[j], exp[j]) = (obs[j] + o_s, exp[j] + e_s)
        else:
            (obs, exp) = (obs + [o_s], exp + [e_s])
    (obs, exp) = (np.array(obs), np.array(exp))
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(obs > 0, obs * np.log(obs / exp), 0.0)
    G = 2.0 * float(np.sum(terms))
    dof = len(obs) - 1
    return G, dof, chi2_sf(G, dof)


def marginal_groups(ec):
    """(name, state axes) of every low-order marginal the tests check: each f_c, each r_nu, each (r_nu, r_mu) of one
    patient, each (f_c, r_nu) with n an endpoint of c."""
    out = [("f%d" % c, (ec.f_axis(c),)) for c in range(ec.C)]
    out += [("r%d,%d" % (n, u), (ec.r_axis(n, u),)) for n in range(ec.Nreg) for u in range(ec.U)]
    out += [("r%d,%d~r%d,%d" % (m, u, n, u), (ec.r_axis(m, u), ec.r_axis(n, u)))
            for u in range(ec.U) for n in range(ec.Nreg) for m in range(n)]
    for (c, (n, m)) in enumerate(O.edge_endpoints(ec.Nreg)):
        for u in range(ec.U):
            for e in (m, n):
                out.append(("f%d~r%d,%d" % (c, e, u), (ec.f_axis(c), ec.r_axis(e, u))))
    return out


def binom_two_sided(k, n, p):
    """Two-sided tail probability of k successes in Binomial(n, p): twice the exact tail on k's side of the mean (at most 1),
    summed term by term from k outwards."""
    import math
    (k, n, p) = (int(k), int(n), float(p))
    if p <= 0.0 or p >= 1.0:
        return 1.0 if k == (n if p >= 1.0 else 0) else 0.0
    (lp, lq, lgn) = (math.log(p), math.log1p(-p), math.lgamma(n + 1))

    def term(i):
        return math.exp(lgn - math.lgamma(i + 1) - math.lgamma(n - i + 1) + i * lp + (n - i) * lq)
    (tail, step, i) = (0.0, 1 if k >= n * p else -1, k)
    while 0 <= i <= n:
        t = term(i)
        tail += t
        if t == 0.0 or t < 1e-30 * tail:           # (terms only shrink away from the mean)
            break
        i += step
    return min(1.0, 2.0 * tail)


def marginal_tests(ec, hist, P, exact_below=1000.0):
    """
    Every cell of every marginal of `marginal_groups`: z = (observed - n p) / sqrt(n p (1 - p)) and its two-sided p-value --
    erfc(|z| / sqrt 2) where both n p and n (1 - p) are at least `exact_below`, else the exact binomial tail (the normal
    tail is far too thin at 5 sigma for cells expecting a handful of chains).  Returns (names, z, p), one entry per cell.
    """
    import math
    n = float(hist.sum())
    (H, Q) = (hist.reshape(ec.shape), P.reshape(ec.shape))
    (names, zs, ps) = ([], [], [])
    nd = len(ec.shape)
    for (name, axes) in marginal_groups(ec):
        other = tuple(a for a in range(nd) if a not in axes)
        (h, q) = (H.sum(axis=other).reshape(-1), np.clip(Q.sum(axis=other).reshape(-1), 0.0, 1.0))
        for j in range(h.size):
            var = n * q[j] * (1.0 - q[j])
            d = h[j] - n * q[j]
            z = d / math.sqrt(var) if var > 0 else (0.0 if abs(d) < 0.5 else math.copysign(math.inf, d))
            if min(n * q[j], n * (1.0 - q[j])) >= exact_below:
                pv = math.erfc(abs(z) / math.sqrt(2.0))
            else:
                pv = binom_two_sided(h[j], n, q[j])
            names.append("%s=%d" % (name, j))
            zs.append(z)
            ps.append(pv)
    return names, np.array(zs), np.array(ps)
