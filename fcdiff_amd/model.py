"""
The individual anomalous region (IAR) model: parameter container + forward sampler.

Mirrors fcdiff/model.py:9-236: same class name, attributes, defaults, `__str__`, `sample(N, H, U)` and the
six `sample_*` methods with the same return shapes/dtypes.  The sampler is host-side NumPy exactly like
the reference's (it is the synthetic-input generator, not part of the fit path) and consumes the legacy
`RandomState` stream in the same order, so `sample` reproduces the reference draw for draw
(tests/golden/G9).  `sample_fast` is the same distribution from a `numpy.random.Generator`, vectorised,
for benchmark-sized inputs.
"""
import textwrap

import numpy as np

from . import util


def group_labels_csr(labels, U):
    """
    Known group labels of the patients as (names, offsets (G+1,) int64, order (U,) int32): names the sorted unique labels,
    order the patients sorted by group -- the members of a group in ascending patient index -- and offsets each group's span
    in it, what fcd_lik_grouped_tables takes.  Every patient is in exactly one group and no group is empty by construction.
    labels: a (U,) sequence of ints or of strings.  ValueError for another length or rank, a None or NaN label, a label
    that is neither an int nor a str (or a mix of the two), and more than U groups.
    """
    U = int(U)
    if isinstance(labels, (str, bytes)) or np.ndim(labels) != 1 or len(labels) != U:
        raise ValueError("group labels must be a sequence of one label per patient, (U,) = (%d,)" % U)
    vals = []
    for v in (labels.tolist() if isinstance(labels, np.ndarray) else list(labels)):
        if isinstance(v, (bool, np.bool_)) or v is None or (isinstance(v, (float, np.floating)) and v != v):
            raise ValueError("group labels must be ints or strings, one per patient: got %r (None / NaN: every patient is in "
                             "exactly one group)" % (v,))
        if isinstance(v, (int, np.integer)):
            vals.append(int(v))
        elif isinstance(v, str):
            vals.append(str(v))
        else:
            raise ValueError("group labels must be ints or strings, got %r" % (v,))
    if len(set(type(v) for v in vals)) > 1:
        raise ValueError("group labels must be all ints or all strings")
    names = sorted(set(vals))
    if len(names) > U or len(names) < 1:
        raise ValueError("group labels name %d groups for %d patients" % (len(names), U))
    index = {name: g for (g, name) in enumerate(names)}
    group_of = np.array([index[v] for v in vals], dtype=np.int64)
    order = np.argsort(group_of, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(group_of, minlength=len(names)))]).astype(np.int64)
    return names, offsets, order


def group_of_patient(offsets, order):
    """(U,) int64: the group index of every patient, from the CSR arrays of group_labels_csr()."""
    group_of = np.empty(len(order), dtype=np.int64)
    group_of[np.asarray(order, dtype=np.int64)] = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return group_of


class _RegionModelParams(object):
    """The parameters both region models share, their defaults and their packing for the C ABI."""

    def __init__(self):
        self.rng = np.random.RandomState(0)
        self.pi = 0.05
        self.eta = 0.3
        self.gamma = np.array([0.1, 0.8, 0.1])
        self.epsilon = 0.03
        self.mu = np.array([-0.15, 0, 0.3])
        self.sigma = np.array([0.025, 0.035, 0.05])

    # ---- packing used by the C ABI: theta[12] = pi, eta, epsilon, gamma[3], mu[3], sigma[3] ----
    def pi2(self):
        """pi as the 2-vector [1-pi, pi] the fitter indexes (quirk Q4: fit.py:183, :486)."""
        pi = np.asarray(self.pi, dtype=np.float64)
        if pi.ndim == 0:
            return np.array([1.0 - float(pi), float(pi)])
        return pi.astype(np.float64).reshape(2)

    def theta(self):
        return np.concatenate([[self.pi2()[1], self.eta, self.epsilon],
                               np.asarray(self.gamma, dtype=np.float64).reshape(3),
                               np.asarray(self.mu, dtype=np.float64).reshape(3),
                               np.asarray(self.sigma, dtype=np.float64).reshape(3)]).astype(np.float64)


class UnsharedRegionModel(_RegionModelParams):
    """
    Attributes (fcdiff/model.py:13-38)
    ----------
    rng : numpy.random.RandomState     random number generator (seed 0)
    pi : float                         probability of an anomalous region
    eta : float                        probability of an anomalous connection btw a typical and anomalous region
    gamma : ndarray (3,)               probability of each template connection type
    epsilon : float                    probability that a typical connection differs from the template
    mu, sigma : ndarray (3,)           mean / standard deviation of the correlation of each connection type
    """

    def __str__(self):
        return textwrap.dedent('''\
            fcdiff.models.UnsharedRegionModel
                rng = %s
                pi = %g
                eta = %g
                gamma = %s
                epsilon = %g
                mu = %s
                sigma = %s''' % (self.rng, self.pi, self.eta, self.gamma,
                                 self.epsilon, self.mu, self.sigma))

    # ---- forward sampling (model.py:52-236) ----
    def sample(self, N, H, U):
        """
        Returns (r (N,U) bool, t (C,U) bool, f (C,3) bool, f_tilde (C,U,3) bool, b (C,H) float64,
        b_tilde (C,U) float64), C = N(N-1)/2.
        """
        r = self.sample_R(N, U)
        t = self.sample_T(r)
        f = self.sample_F(N)
        f_tilde = self.sample_F_tilde(f, t)
        b = self.sample_B(f, H)
        b_tilde = self.sample_B_tilde(f_tilde)
        return (r, t, f, f_tilde, b, b_tilde)

    def sample_R(self, N, U):
        """Anomalous regions, Bernoulli(pi) (model.py:92-109)."""
        return self.rng.binomial(1, self.pi, (N, U)) > 0

    def sample_T(self, r):
        """
        Anomalous connections given regions (model.py:111-143): both typical -> False, both anomalous ->
        True, discordant -> Bernoulli(eta).  Edges are visited upper-triangular row-major and a variate
        is consumed only for discordant (edge, patient) pairs, in that order.
        """
        (N, U) = r.shape
        C = util.N_to_C(N)
        iu = np.triu_indices(N, 1)            # (n, m > n) row-major: the reference's loop order
        rn = r[iu[0], :]
        rm = r[iu[1], :]
        t = rn & rm
        disc = rn ^ rm
        k = int(disc.sum())
        if k:
            t[disc] = self.rng.binomial(1, self.eta, k) > 0
        assert t.shape == (C, U)
        return t

    def sample_F(self, N):
        """Connection template, one Multinomial(1, gamma) per edge (model.py:145-160)."""
        return self.rng.multinomial(1, self.gamma, util.N_to_C(N)) > 0

    def sample_F_tilde(self, f, t):
        """Patients' connection types given template and anomalous connections (model.py:162-189)."""
        (C, U) = t.shape
        f_tilde = np.zeros((C, U, 3), dtype='bool')
        e = self.epsilon
        draw = self.rng.multinomial
        for c in range(C):
            fc = f[c, :]
            p_typ = (1 - e) * fc + (e * 0.5) * (1 - fc)
            p_ano = e * fc + (1 - e) * 0.5 * (1 - fc)
            tc = t[c]
            out = f_tilde[c]
            for u in range(U):
                out[u, :] = draw(1, p_ano if tc[u] else p_typ) > 0
        return f_tilde

    def sample_B(self, f, H):
        """Healthy correlations, Normal(mu_f, sigma_f) clipped to [-1, 1] (model.py:191-213)."""
        C = f.shape[0]
        k = np.argmax(f, axis=1)
        b = np.zeros((C, H), dtype='float64')
        for c in range(C):
            b[c, :] = self.rng.normal(self.mu[k[c]], self.sigma[k[c]], H)
        return b.clip(-1, 1)

    def sample_B_tilde(self, f_tilde):
        """Patient correlations given their connection types (model.py:215-236)."""
        k = np.argmax(f_tilde, axis=2)
        # one array call draws element by element in C order: the same variates as the scalar loop
        b_tilde = self.rng.normal(np.asarray(self.mu)[k], np.asarray(self.sigma)[k])
        return b_tilde.clip(-1, 1)

    # ---- same distribution, vectorised, own stream: benchmark-sized inputs in milliseconds ----
    def sample_fast(self, N, H, U, seed=0, sessions=None):
        """
        (r, t, f, f_tilde, b, b_tilde) with the shapes of `sample`, drawn with numpy.random.Generator
        (PCG64).  Edge order is the FITTER's (lower-triangular, util.c_to_nm), so the output can be
        fitted as is (no quirk-Q3 re-indexing).
        sessions = K: b_tilde is (C, U, K), K scans of every patient that share the patient's f_tilde (conditionally
        independent Normal draws given it).  sessions = None: one scan, b_tilde (C, U), the same draws as ever.
        """
        if sessions is not None and (int(sessions) != sessions or int(sessions) < 1):
            raise ValueError("sessions must be None or an integer >= 1")
        g = np.random.default_rng(seed)
        C = util.N_to_C(N)
        il = np.tril_indices(N, -1)           # (n, m < n) row-major == util.c_to_nm order
        r = g.random((N, U)) < self.pi
        rn, rm = r[il[0], :], r[il[1], :]
        t = np.where(rn ^ rm, g.random((C, U)) < self.eta, rn & rm)
        gam = np.asarray(self.gamma, dtype=np.float64)
        fk = g.choice(3, size=C, p=gam / gam.sum())
        f = np.zeros((C, 3), dtype=bool)
        f[np.arange(C), fk] = True
        e = self.epsilon
        keep = np.where(t, g.random((C, U)) < e, g.random((C, U)) < (1 - e))
        other = (fk[:, None] + 1 + (g.random((C, U)) < 0.5)) % 3
        ftk = np.where(keep, fk[:, None], other)
        f_tilde = np.zeros((C, U, 3), dtype=bool)
        np.put_along_axis(f_tilde, ftk[:, :, None], True, axis=2)
        mu = np.asarray(self.mu, dtype=np.float64)
        sg = np.asarray(self.sigma, dtype=np.float64)
        b = (mu[fk][:, None] + sg[fk][:, None] * g.standard_normal((C, H))).clip(-1, 1)
        if sessions is None:
            b_tilde = (mu[ftk] + sg[ftk] * g.standard_normal((C, U))).clip(-1, 1)
        else:
            b_tilde = (mu[ftk][:, :, None] + sg[ftk][:, :, None] * g.standard_normal((C, U, int(sessions)))).clip(-1, 1)
        return (r, t, f, f_tilde, b, b_tilde)

    def sample_gpu(self, N, H, U, seed=0, ctx=None):
        """
        `sample` on the GPU (counter RNG, every variable in parallel): same return types and distribution, the
        fitter's edge order like `sample_fast`.  Needs the HIP library and a GPU (no fallback).
        """
        import ctypes as C
        import torch
        from . import _lib
        ctx = ctx if ctx is not None else _lib.Context()
        Ce = util.N_to_C(N)
        dev = ctx.device
        r = torch.empty((N, U), dtype=torch.uint8, device=dev)
        t = torch.empty((Ce, U), dtype=torch.uint8, device=dev)
        fk = torch.empty((Ce,), dtype=torch.uint8, device=dev)
        ftk = torch.empty((Ce, U), dtype=torch.uint8, device=dev)
        b = torch.empty((Ce, H), dtype=torch.float64, device=dev)
        bt = torch.empty((Ce, U), dtype=torch.float64, device=dev)
        (th, _th) = _lib.dbl_array(self.theta())
        ctx.call("fcd_model_sample", th, N, H, U, C.c_uint64(int(seed)), _lib.dptr(r), _lib.dptr(t), _lib.dptr(fk),
                 _lib.dptr(ftk), _lib.dptr(b), _lib.dptr(bt), _lib.stream_ptr())
        fk, ftk = fk.cpu().numpy().astype(np.int64), ftk.cpu().numpy().astype(np.int64)
        f = np.zeros((Ce, 3), dtype=bool)
        f[np.arange(Ce), fk] = True
        f_tilde = np.zeros((Ce, U, 3), dtype=bool)
        np.put_along_axis(f_tilde, ftk[:, :, None], True, axis=2)
        return (r.cpu().numpy() > 0, t.cpu().numpy() > 0, f, f_tilde, b.cpu().numpy(), bt.cpu().numpy())


def _onehot(k, shape):
    out = np.zeros(shape + (3,), dtype=bool)
    np.put_along_axis(out, np.asarray(k, dtype=np.int64)[..., None], True, axis=-1)
    return out


class SharedRegionModel(_RegionModelParams):
    """
    The shared anomalous-region model: the parameters and defaults of UnsharedRegionModel, but one set of anomalous
    regions for the whole patient population.
        r_n ~ Bernoulli(pi) once per region n, the same for every patient;
        T_cu | r_n, r_m drawn independently per patient u: both typical -> 0, both anomalous -> 1, discordant ->
        Bernoulli(eta) (doc/methods.rst:81-105);
        F, F~, B and B~ as in the unshared model.
    Fitted by fcdiff_amd.fit.SharedRegionFit.
    """

    def __str__(self):
        return textwrap.dedent('''\
            fcdiff_amd.SharedRegionModel
                pi = %g
                eta = %g
                gamma = %s
                epsilon = %g
                mu = %s
                sigma = %s''' % (self.pi2()[1], self.eta, self.gamma, self.epsilon, self.mu, self.sigma))

    def sample(self, N, H, U, seed=0):
        """
        (r (N,) bool, t (C,U) bool, f (C,3) bool, f_tilde (C,U,3) bool, b (C,H) float64, b_tilde (C,U) float64), drawn
        with numpy.random.Generator(seed) in the fitter's edge order (as UnsharedRegionModel.sample_fast).
        """
        g = np.random.default_rng(seed)
        C = util.N_to_C(N)
        il = np.tril_indices(N, -1)           # (n, m < n) row-major == util.c_to_nm order
        r = g.random(N) < self.pi2()[1]
        rn, rm = r[il[0]][:, None], r[il[1]][:, None]
        t = np.where(rn ^ rm, g.random((C, U)) < self.eta, np.broadcast_to(rn & rm, (C, U)))
        gam = np.asarray(self.gamma, dtype=np.float64)
        fk = g.choice(3, size=C, p=gam / gam.sum())
        e = self.epsilon
        keep = np.where(t, g.random((C, U)) < e, g.random((C, U)) < (1 - e))
        other = (fk[:, None] + 1 + (g.random((C, U)) < 0.5)) % 3
        ftk = np.where(keep, fk[:, None], other)
        mu = np.asarray(self.mu, dtype=np.float64)
        sg = np.asarray(self.sigma, dtype=np.float64)
        b = (mu[fk][:, None] + sg[fk][:, None] * g.standard_normal((C, H))).clip(-1, 1)
        b_tilde = (mu[ftk] + sg[ftk] * g.standard_normal((C, U))).clip(-1, 1)
        return (r, t, _onehot(fk, (C,)), _onehot(ftk, (C, U)), b, b_tilde)

    def sample_gpu(self, N, H, U, seed=0, ctx=None):
        """`sample` on the GPU (fcd_model_sample_shared, counter RNG): same return types and distribution."""
        import ctypes as C
        import torch
        from . import _lib
        ctx = ctx if ctx is not None else _lib.Context()
        Ce = util.N_to_C(N)
        dev = ctx.device
        r = torch.empty((N,), dtype=torch.uint8, device=dev)
        t = torch.empty((Ce, U), dtype=torch.uint8, device=dev)
        fk = torch.empty((Ce,), dtype=torch.uint8, device=dev)
        ftk = torch.empty((Ce, U), dtype=torch.uint8, device=dev)
        b = torch.empty((Ce, H), dtype=torch.float64, device=dev)
        bt = torch.empty((Ce, U), dtype=torch.float64, device=dev)
        (th, _th) = _lib.dbl_array(self.theta())
        ctx.call("fcd_model_sample_shared", th, N, H, U, C.c_uint64(int(seed)), _lib.dptr(r), _lib.dptr(t), _lib.dptr(fk),
                 _lib.dptr(ftk), _lib.dptr(b), _lib.dptr(bt), _lib.stream_ptr())
        return (r.cpu().numpy() > 0, t.cpu().numpy() > 0, _onehot(fk.cpu().numpy(), (Ce,)),
                _onehot(ftk.cpu().numpy(), (Ce, U)), b.cpu().numpy(), bt.cpu().numpy())


class GroupedRegionModel(_RegionModelParams):
    """
    The grouped anomalous-region model: the parameters and defaults of the other two models, and one set of anomalous
    regions per KNOWN group of patients (diagnosis subtype, medication arm, site, ...).
        r_ng ~ Bernoulli(pi) once per region n and group g; a patient reads the column of its group;
        T_cu | r_n, r_m drawn independently per patient u, F, F~, B and B~ as in SharedRegionModel.
    One group for everyone is SharedRegionModel, a group per patient UnsharedRegionModel.  Fitted by
    fcdiff_amd.fit.GroupedRegionFit.
    """

    def __str__(self):
        return textwrap.dedent('''\
            fcdiff_amd.GroupedRegionModel
                pi = %g
                eta = %g
                gamma = %s
                epsilon = %g
                mu = %s
                sigma = %s''' % (self.pi2()[1], self.eta, self.gamma, self.epsilon, self.mu, self.sigma))

    def sample(self, N, H, labels, seed=0, sessions=None):
        """
        (r (N,G) bool, t (C,U) bool, f (C,3) bool, f_tilde (C,U,3) bool, b (C,H) float64, b_tilde (C,U) float64) for the U
        patients of `labels` (group_labels_csr: G groups, the columns of r in the order of its sorted names), drawn with
        numpy.random.Generator(seed) in the fitter's edge order and in SharedRegionModel.sample's order of draws: with one
        label for everyone it returns that sample, r as a column.
        sessions = K: b_tilde is (C, U, K), K scans of every patient that share the patient's f_tilde (as
        UnsharedRegionModel.sample_fast).
        """
        if sessions is not None and (int(sessions) != sessions or int(sessions) < 1):
            raise ValueError("sessions must be None or an integer >= 1")
        U = len(labels)
        (names, offsets, order) = group_labels_csr(labels, U)
        group_of = group_of_patient(offsets, order)
        g = np.random.default_rng(seed)
        C = util.N_to_C(N)
        il = np.tril_indices(N, -1)           # (n, m < n) row-major == util.c_to_nm order
        r = g.random((N, len(names))) < self.pi2()[1]
        ru = r[:, group_of]                   # (N, U): every patient reads its group's column
        rn, rm = ru[il[0]], ru[il[1]]
        t = np.where(rn ^ rm, g.random((C, U)) < self.eta, rn & rm)
        gam = np.asarray(self.gamma, dtype=np.float64)
        fk = g.choice(3, size=C, p=gam / gam.sum())
        e = self.epsilon
        keep = np.where(t, g.random((C, U)) < e, g.random((C, U)) < (1 - e))
        other = (fk[:, None] + 1 + (g.random((C, U)) < 0.5)) % 3
        ftk = np.where(keep, fk[:, None], other)
        mu = np.asarray(self.mu, dtype=np.float64)
        sg = np.asarray(self.sigma, dtype=np.float64)
        b = (mu[fk][:, None] + sg[fk][:, None] * g.standard_normal((C, H))).clip(-1, 1)
        if sessions is None:
            b_tilde = (mu[ftk] + sg[ftk] * g.standard_normal((C, U))).clip(-1, 1)
        else:
            b_tilde = (mu[ftk][:, :, None] + sg[ftk][:, :, None] * g.standard_normal((C, U, int(sessions)))).clip(-1, 1)
        return (r, t, _onehot(fk, (C,)), _onehot(ftk, (C, U)), b, b_tilde)


class SubtypeRegionModel(_RegionModelParams):
    """
    The subtype-region model: GroupedRegionModel with the group of every patient drawn instead of given.  The parameters
    and defaults of the other models, and
        n_subtypes : int         number of latent subtypes G
        rho : None or (G,)       probabilities of the subtypes; None: 1/G each
        z_u ~ Categorical(rho) per patient; r_ng ~ Bernoulli(pi) per region and subtype; patient u reads column z_u;
        T, F, F~, B and B~ as in GroupedRegionModel.
    Fitted by fcdiff_amd.fit.SubtypeRegionFit, which puts a Dirichlet prior on rho and integrates it out.
    """

    def __init__(self):
        super(SubtypeRegionModel, self).__init__()
        self.n_subtypes = 2
        self.rho = None

    def __str__(self):
        return textwrap.dedent('''\
            fcdiff_amd.SubtypeRegionModel
                n_subtypes = %d
                rho = %s
                pi = %g
                eta = %g
                gamma = %s
                epsilon = %g
                mu = %s
                sigma = %s''' % (self.n_subtypes, self.rho, self.pi2()[1], self.eta, self.gamma, self.epsilon, self.mu, self.sigma))

    def rho_vector(self):
        """(G,) float64 probabilities of the subtypes.  ValueError for n_subtypes < 1, a wrong length, a negative or NaN entry
        or a sum that is not 1."""
        G = int(self.n_subtypes)
        if G != self.n_subtypes or G < 1:
            raise ValueError("n_subtypes must be an integer >= 1, got %r" % (self.n_subtypes,))
        if self.rho is None:
            return np.full(G, 1.0 / G)
        rho = np.asarray(self.rho, dtype=np.float64)
        if rho.shape != (G,) or not np.all(rho >= 0) or abs(rho.sum() - 1.0) > 1e-9:
            raise ValueError("rho must be %d probabilities that sum to 1, got %r" % (G, self.rho))
        return rho / rho.sum()

    def sample(self, N, H, U, seed=0, sessions=None):
        """
        (z (U,) int64, r, t, f, f_tilde, b, b_tilde): the subtype of every patient, drawn with a generator of its own
        (numpy.random.default_rng([seed, n_subtypes])), then GroupedRegionModel.sample(N, H, z, seed, sessions) of this
        model's parameters, element for element -- with one subtype that is SharedRegionModel.sample's draw, r as a column.
        As there, the columns of r (N, .) are the subtypes that OCCUR in z, in ascending order: a subtype no patient
        drew has no column.
        """
        rho = self.rho_vector()
        z = np.random.default_rng([int(seed), len(rho)]).choice(len(rho), size=int(U), p=rho).astype(np.int64)
        grouped = GroupedRegionModel()
        for name in ("pi", "eta", "gamma", "epsilon", "mu", "sigma"):
            setattr(grouped, name, getattr(self, name))
        return (z,) + grouped.sample(N, H, [int(v) for v in z], seed=seed, sessions=sessions)
