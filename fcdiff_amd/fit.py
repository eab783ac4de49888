"""
Fits models to observed correlations -- the MI355X build of fcdiff/fit.py.

`SharedRegionFit` (below) fits the shared-region model through the same machinery at one patient, `GroupedRegionFit` the
grouped-region model (one anomaly map per known group of patients) at one pseudo-patient per group, `SubtypeRegionFit` the
same model with the groups unknown (latent subtypes, VB) at one pseudo-patient per subtype.

`UnsharedRegionFit` keeps the reference's surface (fcdiff/fit.py:12-54): attributes `model, b, bt,
max_iters=10, rel_tol=1e-5, energy`, private state `_lq_R (N,U,2), _lq_F (C,1,3), _lp_B_g_F (C,H,3),
_p_Bt_g_Ft (C,U,3), _lM (C,U,3,3)` readable/assignable as NumPy arrays, `run()` and the private methods
its tests call (`_init_lps, _update_lps, _update_lq_F, _update_lq_R, _update_pi, _update_gamma,
_update_theta, _eval_energy, _is_converged`).  Every one of them runs a hand-written HIP kernel
through the C ABI (include/fcdiff_hip.h) on tensors that stay on the GPU between calls.  There is no
NumPy fallback: without libfcdiff_hip.so or a GPU these methods raise.

New knobs (all optional; defaults reproduce the reference):
    method       'vb' (reference algorithm) | 'gibbs' (many-chain collapsed Gibbs + MCEM for pi, gamma)
    edge_index   'reference' (fit.py:185-186 calls nm_to_c for every ordered pair: quirk Q1) |
                 'symmetric' (doc/methods.rst:646-653).  Default: 'reference' for vb, 'symmetric' for gibbs.
    n_chains, n_sweeps, burn_in, mstep_every, mstep_lag, seed, chain0     sampler controls
    update_theta_sub, theta_sub_every                          (eta, epsilon) step: vb every iteration / gibbs every K sweeps
    connection_marginals, connection_every                     gibbs: count (f_c, mixture case) for connection_posterior()
    anomaly_counts, anomaly_counts_every                       gibbs: histograms of the anomalous-region counts for
                                                               anomaly_count_posterior()
    coanomaly, coanomaly_every                                 gibbs: counts of regions anomalous together and of patients
                                                               sharing anomalous regions for coanomaly_posterior()
    region_sets, region_sets_every                             gibbs: histograms of the anomalous-region counts over sets
                                                               of regions (networks) for region_set_posterior()
    patient_groups, patient_group_contrasts, patient_groups_every
                                                               gibbs: histograms of the number of anomalous patients per
                                                               group of patients, and joint ones per contrast of two groups,
                                                               for patient_group_posterior()
    patient_traits, patient_traits_every                       gibbs: rank-sum (AUC) histograms between the anomalous and the
                                                               other patients of a row, per trait of the patients, for
                                                               patient_trait_posterior()
    missing_data                                               True: NaN entries of b / bt are unobserved and integrated out

Differences from the reference that are deliberate and documented:
  Q4  `model.pi` may be the scalar the model defines or the 2-vector [1-pi, pi] the reference's updates
      index; both are accepted everywhere.
  Q5  tables are float64 (the reference's np.full(shape, 1) buffers turn int64 on modern NumPy).
  Q7  run() is the documented loop (doc/methods.rst:564-600); `energy` is appended to.  The reference's
      run() raises IndexError on its first energy assignment (fit.py:73-74).  The (eta, epsilon)
      optimiser step (fit.py:222-241) cannot run in the reference (it calls undefined names); here it is
      implemented (`_update_theta_sub`, analytic gradient on the device) but stays OFF by default
      (`update_theta_sub = False`) so that the default trajectory is the one the fixtures pin.
"""
import collections

import numpy as np

from . import _lib
from . import util
from . import score as _score
from . import tables
from .model import group_labels_csr, group_of_patient
from .gibbs import (GibbsEngine, run_chains, allreduce_counts, pool_u32, pair_sweeps_in, ACCUMULATORS, PAIR_COUNT_MAX,
                    COUNT_MAX_NREG, COUNT_MAX_U, region_sets_csr, patient_groups_csr, patient_group_contrasts,
                    patient_traits_scores, PATIENT_TRAIT_BINS)

# The knobs of a gibbs fit that attach one of the sampler's accumulators, in the order _run_gibbs() checks, attaches and
# collects them (the region sets before the groups and traits that take them as rows): knob (a flag, or with `give` a
# collection that is on unless None), its period knob, what the messages call it, the row of gibbs.ACCUMULATORS, the attributes
# the pooled buffers and the number of sweeps behind them are left in, and the attributes that describe those buffers (`meta`).
# Three optional hooks, names of methods of the fit: check(a, N, U) refuses before any engine is made (default
# _check_accumulator_row), give(eng) hands the collection to the engine before its accumulator is attached, collect(eng) fills
# `meta` and reshapes after the buffers were pooled.
FitAccumulator = collections.namedtuple("FitAccumulator", "knob every label engine results sweeps meta check give collect")
_ENGINE_ROW = {a.key: a for a in ACCUMULATORS}
GIBBS_ACCUMULATORS = (
    FitAccumulator("connection_marginals", "connection_every", "connection counts", _ENGINE_ROW["pair"],
                   ("connection_counts",), "connection_sweeps", (), None, None, None),
    FitAccumulator("anomaly_counts", "anomaly_counts_every", "anomaly-count histograms", _ENGINE_ROW["count"],
                   ("patient_count_hist", "region_count_hist"), "anomaly_count_sweeps", (), "_check_anomaly_counts", None, None),
    FitAccumulator("coanomaly", "coanomaly_every", "co-anomaly counts", _ENGINE_ROW["coanomaly"],
                   ("region_pair_counts", "patient_pair_counts"), "coanomaly_sweeps", (), None, None, "_collect_coanomaly"),
    FitAccumulator("region_sets", "region_sets_every", "region-set histograms", _ENGINE_ROW["region_set"],
                   ("region_set_hist", "region_set_prevalence_hist"), "region_set_sweeps", ("region_set_names", "region_set_sizes"),
                   "_check_region_sets", "_give_region_sets", "_collect_region_sets"),
    FitAccumulator("patient_groups", "patient_groups_every", "patient-group histograms", _ENGINE_ROW["patient_group"],
                   ("patient_group_hist", "patient_group_joint_hist"), "patient_group_sweeps",
                   ("patient_group_names", "patient_group_sizes", "patient_group_rows", "patient_group_pairs"),
                   "_check_patient_groups", "_give_patient_groups", "_collect_patient_groups"),
    FitAccumulator("patient_traits", "patient_traits_every", "patient-trait histograms", _ENGINE_ROW["patient_trait"],
                   ("patient_trait_hist", "patient_trait_sum"), "patient_trait_sweeps",
                   ("patient_trait_names", "patient_trait_n_known", "patient_trait_rows"),
                   "_check_patient_traits", "_give_patient_traits", "_collect_patient_traits"),
)


class UnsharedRegionFit(object):
    """
    Fits an unshared region model to correlations (fcdiff/fit.py:12-30).

    Attributes
    ----------
    model : fcdiff_amd.UnsharedRegionModel      initial model; updated in place by run()
    b : ndarray (C, H), bt : ndarray (C, U)     correlations of healthy subjects / patients; bt may be (C, U, K): K sessions
                                                of every patient (`n_sessions`), see "Repeated sessions" below
    max_iters : int, rel_tol : float            iteration cap / relative tolerance of _is_converged
    energy : list of float                      variational free energy per iteration (vb) or minus the
                                                chain-mean log-joint per recorded sweep (gibbs)

    Repeated sessions
    -----------------
    bt (C, U, K) holds K scans of every patient.  F~_cu is the patient's latent state of the connection and the sessions
    are conditionally independent measurements of it, so an item's density given F~ = j is prod_k N(bt[c,u,k]; mu_j,
    sigma_j), taken in log form by the table kernel; the state (`_lq_R` (N, U, 2), `_lM` (C, U, 3, 3)), the VB updates,
    the sampler and every query keep their shapes.  Patients with different numbers of sessions pad with NaN and set
    missing_data = True: a NaN session contributes nothing, and missing_counts() counts NaN session entries.  Extra
    sessions of controls are extra columns of b.  Not provided with sessions: the theta_sub step (update_theta_sub,
    theta_sub_every: NotImplementedError from run()) and the per-item table `_p_Bt_g_Ft` (ValueError).

    Measurement noise
    -----------------
    `b_noise_var` (H,) and `bt_noise_var` (U,) or (U, K) give every control and every patient (session) a KNOWN measurement
    variance on top of the population spread: b_ch ~ N(mu_k, sigma_k^2 + b_noise_var[h]), bt_cuk ~ N(mu_j, sigma_j^2 +
    bt_noise_var[u,k]); sigma is then the population spread alone, and a correlation from few frames counts for less instead
    of looking anomalous.  corr.sampling_variance(info) gives the variances of the cleaning front-end's subjects.  A (U,)
    with sessions data applies to every session; None is all zeros, and with both None nothing changes.  The variances
    enter through the table build only (fcd_lik_tables_noise / fcd_lik_shared_tables_noise): both fitters of both models,
    log_evidence(), connection_posterior() and score(bt_new, noise_var=...) take them.  Values must be finite and >= 0
    (ValueError naming "noise" from run() / _update_lps()); to drop a subject use NaN data under missing_data, not an
    infinite variance.  Not provided with noise variances: the theta_sub step and membership() (NotImplementedError), and
    `_p_Bt_g_Ft` (ValueError).
    """

    # SharedRegionFit: the tables are (S_B, L) of ONE patient (tables.build(shared=True)), so the state's patient extent is 1,
    # there are no per-item tables, and _init_lps fills _lM with 0 (here the reference's 1)
    _shared = False

    def _patient_extent(self, U):
        """
        The patient extent of the state (`_lq_R` (N, ., 2), `_lM` (C, ., 3, 3)) and of the sampler for U patients in bt: U
        here, 1 for SharedRegionFit (one population column), the number of groups for GroupedRegionFit.
        """
        return int(U)

    def _groups_kw(self):
        """{} (tables.build is called as before, argument for argument); GroupedRegionFit: its `groups`."""
        return {}

    def _built_table(self, U):
        """
        (key of self._d, patient extent) of the table the data build writes: the state's own `lM`; SubtypeRegionFit: the
        per-patient table it keeps beside the state's L.
        """
        return "lM", self._patient_extent(U)

    def _expand_weights(self, W):
        """Weights or counts (C, extent, 3, 3) of the state as the theta_sub objectives read them; GroupedRegionFit expands."""
        return W

    def __init__(self):
        self.model = None
        self.b = None
        self.bt = None
        self.max_iters = 10
        self.rel_tol = 1e-5
        self.energy = []

        self.method = "vb"
        self.data_check = "sample"   # how _update_lps() notices in-place edits of b / bt: 'sample' | 'full' | 'none' (_data_digest)
        self.edge_index = None
        self.update_theta_sub = False
        self.theta_sub_params = "eta_epsilon"     # 'all': mu and sigma^2 join the optimiser (the reference's commented-out intent)
        self.n_chains = 1024
        self.n_sweeps = 100
        self.burn_in = 20
        self.mstep_every = 1
        self.mstep_lag = 0         # gibbs: 1 = apply an M-step one period late so its all-reduce overlaps the next sweeps
        self.theta_sub_every = 0   # gibbs: re-fit (eta, epsilon) from pooled chain counts every this many sweeps (0: never)
        self.energy_every = 0
        self.trace_every = 0       # gibbs: keep every chain's log-joint every this many sweeps in `trace` (chains, draws)
        self.trace = None          # ... and its number of anomalous sites sum_{n,u} r_nu in `trace_r`
        self.trace_r = None
        self.seed = 0
        self.chain0 = 0
        self.sampler = None       # the GibbsEngine of the last gibbs run
        self.connection_marginals = False   # gibbs: accumulate (f_c, mixture case) counts for connection_posterior()
        self.connection_every = 1           # ... at every this many sweeps from burn_in on
        self.connection_counts = None       # (C, U, 3, 3) int64: those counts, pooled over chains, sweeps and ranks
        self.connection_sweeps = 0          # number of sweeps behind connection_counts (each counts every chain once)
        self.anomaly_counts = False         # gibbs: histograms of sum_n r_nu and sum_u r_nu for anomaly_count_posterior()
        self.anomaly_counts_every = 1       # ... at every this many sweeps from burn_in on
        self.patient_count_hist = None      # (U, Nreg+1) int64: chains x sweeps (x ranks) with sum_n r_nu = k
        self.region_count_hist = None       # (Nreg, U+1) int64: chains x sweeps (x ranks) with sum_u r_nu = k
        self.anomaly_count_sweeps = 0       # number of sweeps behind those histograms
        self.coanomaly = False              # gibbs: pair counts of the r sites for coanomaly_posterior()
        self.coanomaly_every = 1            # ... at every this many sweeps from burn_in on
        self.region_pair_counts = None      # (Nreg, Nreg) int64: (chain, sweep, patient) with r_nu = r_mu = 1, pooled over ranks
        self.patient_pair_counts = None     # (U, U) int64: (chain, sweep, region) with r_nu = r_nv = 1, pooled over ranks
        self.coanomaly_sweeps = 0           # number of sweeps behind those counts
        self.coanomaly_states = 0           # ... and of chain states: sweeps x chains, summed over ranks
        self.region_sets = None             # sets of regions (networks) for region_set_posterior(): a dict name -> indices, a
                                            # sequence of index sequences, or a boolean mask (J, Nreg); gibbs: histograms over them
        self.region_sets_every = 1          # ... at every this many sweeps from burn_in on
        self.region_set_hist = None         # (J, U, S_max+1) int64: chains x sweeps (x ranks) with sum_{n in S_j} r_nu = k
        self.region_set_prevalence_hist = None      # (J, U+1) int64: ... with k patients having an anomalous region in S_j
        self.region_set_sweeps = 0          # number of sweeps behind those histograms
        self.region_set_names = None        # names and sizes of the sets behind them, in order
        self.region_set_sizes = None
        self.patient_groups = None          # groups of patients for patient_group_posterior(): a dict name -> indices, a
                                            # sequence of index sequences, or a boolean mask (J, U); gibbs: histograms over them
        self.patient_group_contrasts = None # pairs (a, b) of names or indices of two disjoint groups: joint histograms of (k_a, k_b)
        self.patient_groups_every = 1       # ... at every this many sweeps from burn_in on
        self.patient_group_hist = None      # (J, R, Umax+1) int64: chains x sweeps (x ranks) with k patients of g_j anomalous at row rho
        self.patient_group_joint_hist = None        # per contrast (R, |a|+1, |b|+1) int64: ... with (k_a, k_b) at row rho
        self.patient_group_sweeps = 0       # number of sweeps behind those histograms
        self.patient_group_names = None     # names and sizes of the groups behind them, the names of the R rows (the regions,
        self.patient_group_sizes = None     # then "set:<name>" for the region sets), and the contrasts as pairs of group indices
        self.patient_group_rows = None
        self.patient_group_pairs = None
        self.patient_traits = None          # traits of the patients for patient_trait_posterior(): a dict name -> (U,) values, a
                                            # sequence of such vectors or an array (Q, U); NaN = not known for this patient
        self.patient_traits_every = 1       # ... at every this many sweeps from burn_in on
        self.patient_trait_hist = None      # (Q, R, Umax+1 + 128 + 3) int64: chains x sweeps (x ranks) by k, by AUC bin, by sign of A
        self.patient_trait_sum = None       # (Q, R, Umax+1) int64: the sum of A over the states with that k
        self.patient_trait_sweeps = 0       # number of sweeps behind them
        self.patient_trait_names = None     # names of the traits behind them, how many patients each is known for, and the
        self.patient_trait_n_known = None   # names of the R rows (the regions, then "set:<name>" for the region sets)
        self.patient_trait_rows = None
        # True: every NaN of b / bt is an unobserved value, integrated out exactly (S_B sums the observed h only, lM = 0 at a
        # missing bt); False: NaN is read as a number, as the reference reads it.  Only NaN is missing, not +-inf.
        self.missing_data = False
        # known measurement variances on top of sigma^2 (see "Measurement noise"): (H,) / (U,) or (U, K), None = zeros
        self.b_noise_var = None
        self.bt_noise_var = None

        self._ctx = None
        self._query_ctx = None    # score(), log_evidence(), membership(): one context apart from the fit's (_query_context)
        self._d = {}              # device tensors: lq_R, lq_F, S_B, lM, lpB, pBt, hyper, b, bt
        self._hyper_key = None

    # ------------------------------------------------------------------ device plumbing
    def _context(self):
        if self._ctx is None:
            self._ctx = _lib.Context()
        return self._ctx

    def _query_context(self):
        """
        The context of score(), log_evidence() and membership(): never the fit's, so that a query touches neither the fit's
        workspace nor its plan.  One serves all three: they run one after another on one stream and use the workspace only
        inside a call.
        """
        if self._query_ctx is None:
            self._query_ctx = _lib.Context()
        return self._query_ctx

    def _torch(self):
        import torch
        return torch

    def _dev(self):
        return self._context().device

    def _up(self, a):
        t = self._torch()
        return t.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self._dev())

    def _data_dev(self, key):
        """The device copy of self.b (key 'b') or self.bt ('bt'): the fit's own where its shape still holds, else a fresh upload
        (not kept: a query leaves the fit as it was)."""
        (d, a) = (self._d.get(key), getattr(self, key))
        if d is None or tuple(d.shape) != np.shape(a):
            d = self._up(a)
        return d

    @property
    def n_sessions(self):
        """K of a bt (C, U, K); 1 for a bt (C, U) (and before bt is set)."""
        shp = np.shape(self.bt) if self.bt is not None else ()
        return int(shp[2]) if len(shp) == 3 else 1

    def _has_sessions(self):
        return self.bt is not None and np.ndim(self.bt) == 3

    def _refuse_theta_sub_sessions(self):
        """The theta_sub objectives read bt item by item, one scan per patient: no sessions form yet."""
        if self._has_sessions() and (self.update_theta_sub or self.theta_sub_every):
            raise NotImplementedError("the theta_sub step (update_theta_sub / theta_sub_every, either theta_sub_params) is not "
                                      "provided for sessions data bt (C, U, K): its objective kernels read one scan per patient")

    def _has_noise(self):
        return self.b_noise_var is not None or self.bt_noise_var is not None

    def _refuse_theta_sub_noise(self):
        """The theta_sub objectives know one sigma per state: an objective that separates sigma from the variances is not made."""
        if self._has_noise() and (self.update_theta_sub or self.theta_sub_every):
            raise NotImplementedError("the theta_sub step (update_theta_sub / theta_sub_every, either theta_sub_params) is not "
                                      "provided with noise variances (b_noise_var / bt_noise_var): its objective kernels take "
                                      "one sigma per state")

    @staticmethod
    def _noise_array(v, shapes, name):
        a = np.ascontiguousarray(v, dtype=np.float64)
        if a.shape not in shapes:
            raise ValueError("noise: %s must have shape %s, got %s" % (name, " or ".join(str(x) for x in shapes), a.shape))
        if not np.all(np.isfinite(a)) or np.any(a < 0):
            raise ValueError("noise: %s must be finite and >= 0 (to drop a subject give NaN data under missing_data, not an "
                             "infinite variance)" % name)
        return a

    _OWN = object()          # _noise_host(bt_var=...): the fit's own bt_noise_var

    def _noise_host(self, bt_shape=None, bt_var=_OWN, name="bt_noise_var"):
        """
        None without noise variances, else (var_b (H,) or None, var_bt (U, K) or None) as checked float64 arrays; a (U,)
        is repeated over the sessions.  Host only: ValueError naming "noise" for a wrong shape, a negative, NaN or inf.
        bt_shape / bt_var: the patients of a query (score()) in place of the fit's own.
        """
        bt_var = self.bt_noise_var if bt_var is UnsharedRegionFit._OWN else bt_var
        if self.b_noise_var is None and bt_var is None:
            return None
        shp = tuple(np.shape(self.bt)) if bt_shape is None else tuple(bt_shape)
        (U, K) = (int(shp[1]), int(shp[2]) if len(shp) == 3 else 1)
        vb = vbt = None
        if self.b_noise_var is not None:
            vb = self._noise_array(self.b_noise_var, ((int(np.shape(self.b)[1]),),), "b_noise_var")
        if bt_var is not None:
            vbt = self._noise_array(bt_var, ((U,), (U, K)), name)
            if vbt.ndim == 1:
                vbt = np.ascontiguousarray(np.repeat(vbt[:, None], K, axis=1))
        return (vb, vbt)

    def _noise_dev(self):
        """The device copies of _noise_host() (None without noise variances), made again whenever the host values change."""
        host = self._noise_host()
        if host is None:
            return None
        key = tuple(None if a is None else (a.shape, a.tobytes()) for a in host)
        cur = self._d.get("noise")
        if cur is None or cur[0] != key:
            cur = (key, tuple(None if a is None else self._up(a) for a in host))
            self._d["noise"] = cur
        return cur[1]

    def _require_fitted(self, what):
        """ValueError unless run() has left a fit of self.method behind: a sampler (gibbs), or q_F and an energy (vb)."""
        fitted = (self.sampler is not None) if self.method == "gibbs" else (self._d.get("lq_F") is not None and bool(self.energy))
        if self.model is None or not fitted:
            raise ValueError("%s needs a fitted model: call run() first" % what)

    def _edge_mode(self):
        name = self.edge_index
        if name is None:
            name = "reference" if self.method == "vb" else "symmetric"
        if name not in _lib.EDGE_MODES:
            raise ValueError("edge_index must be 'reference' or 'symmetric'")
        return name

    def _shape(self):
        lM = self._d.get("lM")
        if lM is None:
            raise ValueError("tables have not been initialized (_init_lps / _update_lps)")
        if lM.dim() != 4 or tuple(lM.shape[2:]) != (3, 3):
            raise ValueError("_lM must have shape (C, U, 3, 3), got %s" % (tuple(lM.shape),))
        C, U = int(lM.shape[0]), int(lM.shape[1])
        N = util.C_to_N(C)
        if (N % 1) != 0:
            raise ValueError("Number of connections (%u) must be a triangular number." % C)
        return int(N), C, U

    def _check_state(self, need=("lq_R", "lq_F", "S_B")):
        """
        (N, C, U) from the tables, after checking that every buffer a kernel is about to index has the shape the
        kernel assumes.  The private state is assignable as NumPy arrays (the reference's tests do it); a mismatch
        there is a NumPy broadcasting error in the reference -- here it would be an out-of-bounds device read, so it
        is refused on the host before anything is launched.
        """
        (N, C, U) = self._shape()
        want = {"lq_R": (N, U, 2), "lq_F": (C, 1, 3), "S_B": (C, 3)}
        for key in need:
            v = self._d.get(key)
            if v is None:
                raise ValueError("_%s has not been initialized (_init_lps)" % key)
            if tuple(v.shape) != want[key]:
                raise ValueError("_%s has shape %s, the tables (_lM %s) need %s"
                                 % (key if key != "S_B" else "lp_B_g_F (summed over H)", tuple(v.shape),
                                    (C, U, 3, 3), want[key]))
        return (N, C, U)

    def _hyper(self):
        """Device hyper block {ln gamma, ln(1-pi), ln pi} refreshed whenever the model's values changed."""
        t = self._torch()
        if "hyper" not in self._d:
            self._d["hyper"] = t.zeros(8, dtype=t.float64, device=self._dev())
        gamma = np.asarray(self.model.gamma, dtype=np.float64).reshape(3)
        pi2 = self._pi2()
        key = (tuple(gamma.tolist()), tuple(pi2.tolist()))
        if key != self._hyper_key:
            tables.write_hyper(self._context(), self._d["hyper"], gamma, pi2)
            self._hyper_key = key
        return self._d["hyper"]

    def _pi2(self):
        pi = np.asarray(self.model.pi, dtype=np.float64)
        if pi.ndim == 0:
            return np.array([1.0 - float(pi), float(pi)])
        return pi.reshape(2)

    # ------------------------------------------------------------------ NumPy views of the device state
    def _get(self, key, shape=None):
        v = self._d.get(key)
        if v is None:
            return None
        a = v.cpu().numpy()
        return a.reshape(shape) if shape is not None else a

    @property
    def _lq_R(self):
        return self._get("lq_R")

    @_lq_R.setter
    def _lq_R(self, a):
        self._d["lq_R"] = None if a is None else self._up(a)

    @property
    def _lq_F(self):
        return self._get("lq_F")

    @_lq_F.setter
    def _lq_F(self, a):
        self._d["lq_F"] = None if a is None else self._up(a)

    @property
    def _lM(self):
        return self._get("lM")

    @_lM.setter
    def _lM(self, a):
        self._d["lM"] = None if a is None else self._up(a)

    @property
    def _lp_B_g_F(self):
        """(C,H,3).  The fit path only ever uses its H-sum; the full table is produced on demand."""
        if self._d.get("lpB") is None and self.b is not None and self.model is not None and "S_B" in self._d:
            self._tables(full=True)
        return self._get("lpB")

    @_lp_B_g_F.setter
    def _lp_B_g_F(self, a):
        if a is None:
            self._d["lpB"] = None
            return
        self._d["lpB"] = self._up(a)
        self._d["S_B"] = self._d["lpB"].sum(dim=1).contiguous()      # fit.py:171 sums over H

    @property
    def _p_Bt_g_Ft(self):
        if self._has_sessions():
            raise ValueError("_p_Bt_g_Ft is not made for sessions data bt (C, U, K): a product of densities underflows")
        if self._has_noise():
            raise ValueError("_p_Bt_g_Ft is not made with noise variances: the noise tables are log-form only")
        if self._d.get("pBt") is None and self.bt is not None and self.model is not None and "lM" in self._d:
            self._tables(full=True)
        return self._get("pBt")

    @_p_Bt_g_Ft.setter
    def _p_Bt_g_Ft(self, a):
        self._d["pBt"] = None if a is None else self._up(a)

    # ------------------------------------------------------------------ reference methods
    def run(self):
        """Runs the fitting procedure (fcdiff/fit.py:56-82; doc/methods.rst:564-600)."""
        self._refuse_theta_sub_sessions()
        self._refuse_theta_sub_noise()
        (C, H) = self.b.shape
        if np.ndim(self.bt) not in (2, 3) or (np.ndim(self.bt) == 3 and np.shape(self.bt)[2] < 1):
            raise ValueError("bt must be (C, U) or (C, U, K) with K >= 1 sessions, got shape %s" % (np.shape(self.bt),))
        U = self.bt.shape[1]
        N = util.C_to_N(C)
        if (N % 1) != 0:
            msg = "Number of connections (%u) must be a triangular number." % C
            raise ValueError(msg)
        if self.model is None:
            msg = "Model has not been initialized."
            raise ValueError(msg)
        self._noise_host()               # (a ValueError for bad noise variances before any context exists)
        N = int(N)
        self._init_lps(N, H, U)
        self._update_lps()
        if self.method == "vb":
            self._run_vb()
        elif self.method == "gibbs":
            self._run_gibbs(N, self._patient_extent(U))
        else:
            raise ValueError("method must be 'vb' or 'gibbs'")

    def _run_vb(self):
        self.energy = [self._eval_energy()]
        for i in range(1, self.max_iters + 1):
            self._update_lq_F()
            self._update_lq_R()
            self._update_theta()
            self._update_lps()
            self.energy.append(self._eval_energy())
            if self._is_converged(i):
                break

    def _init_lps(self, N, H, U):
        """Uniform log-probabilities and float64 tables (fit.py:84-102)."""
        t = self._torch()
        dev = self._dev()
        C = util.N_to_C(N)
        Ut = self._patient_extent(U)
        self._d["lq_R"] = t.full((N, Ut, 2), -np.log(2), dtype=t.float64, device=dev)
        self._d["lq_F"] = t.full((C, 1, 3), -np.log(3), dtype=t.float64, device=dev)
        self._d["S_B"] = t.full((C, 3), float(H), dtype=t.float64, device=dev)
        self._d["lM"] = t.full((C, Ut, 3, 3), 0.0 if self._shared else 1.0, dtype=t.float64, device=dev)
        self._d["lpB"] = None
        self._d["pBt"] = None
        self._d.pop("data_key", None)        # a fit starts from the arrays as they are now (see _tables)

    def _update_lps(self):
        """Likelihood tables from the current parameters (fit.py:104-122): kernel K_lik (K_lik_shared for SharedRegionFit)."""
        self._tables(full=False)

    def _tables(self, full):
        """S_B and lM (full: the per-item tables lpB, pBt too, where the model has them) in ONE launch: tables.build."""
        self._noise_host()               # (a ValueError for bad noise variances before any context exists)
        t = self._torch()
        dev = self._dev()
        b = np.ascontiguousarray(self.b, dtype=np.float64)
        bt = np.ascontiguousarray(self.bt, dtype=np.float64)
        (C, H) = b.shape
        U = bt.shape[1]
        # the device copies of b / bt are made by _init_lps()/run() and kept across the _update_lps() calls of a fit (the
        # reference re-reads self.b / self.bt on every call, fcdiff/fit.py:111-115; here that would be a host digest or
        # a PCIe copy of 16-320 MB per variational iteration).  What is checked on EVERY call is cheap: the arrays'
        # identity, base address, shape, strides -- and, `data_check='sample'`, a strided sample of 4096 elements that
        # visits every column.  `data_check='full'` digests the whole arrays on every call (CRC-32: 8 ms at cfg3,
        # 165 ms at cfg5); invalidate_data() forces the next call to upload.
        key = (self._array_key(self.b), self._array_key(self.bt), self._data_digest(b, self.data_check),
               self._data_digest(bt, self.data_check))
        uploaded = self._d.get("data_key") != key
        if uploaded:
            self._d["b"], self._d["bt"] = self._up(b), self._up(bt)
            self._d["data_key"] = key
        # the buffers are kept when their shape holds: a sampler built on them reads the new tables after refresh_tables()
        (key_lM, extent) = self._built_table(U)
        (S_B, lM) = (self._d.get("S_B"), self._d.get(key_lM))
        if S_B is not None and tuple(S_B.shape) != (C, 3):
            S_B = None
        if lM is not None and tuple(lM.shape) != (C, extent, 3, 3):
            lM = None
        lpB = pBt = None
        if full and not self._shared and not self._groups_kw():
            lpB = t.empty((C, H, 3), dtype=t.float64, device=dev)
            if bt.ndim == 2 and not self._has_noise():       # (sessions, noise: no per-item densities, see _p_Bt_g_Ft)
                pBt = t.empty((C, U, 3), dtype=t.float64, device=dev)
        n_missing = None
        if self.missing_data:
            # the kernel counts the NaN entries on the device; missing_counts() reads them when asked (no sync here).  The
            # counts depend on the data alone, so they are taken when the data is uploaded: the counting build waits for
            # its atomics (5-39 us more at cfg3 with 10 % NaN), the per-iteration builds after it run at the uncounted speed
            if self._d.get("n_missing") is None:
                self._d["n_missing"] = t.zeros(2, dtype=t.int64, device=dev)
            if uploaded or not self._d.get("n_missing_valid"):
                n_missing = self._d["n_missing"]
        (self._d["S_B"], self._d[key_lM]) = tables.build(self._context(), self._d["b"], self._d["bt"], self.model.theta(),
                                                         self._flags(), shared=self._shared, S_B=S_B, lM=lM, lpB=lpB, pBt=pBt,
                                                         n_missing=n_missing, **self._noise_kw(), **self._groups_kw())
        self._d["n_missing_valid"] = bool(self.missing_data)
        self._d["lpB"], self._d["pBt"] = lpB, pBt

    def _flags(self):
        return _lib.FCD_DATA_NAN_MISSING if self.missing_data else 0

    def _noise_kw(self):
        """{} without noise variances (tables.build is then called as before, argument for argument), else its `noise`."""
        noise = self._noise_dev()
        return {} if noise is None else {"noise": noise}

    def _noise_bt_kw(self):
        """conn_posterior()'s `noise_var` of the fit's own patients: {} where bt_noise_var is None."""
        noise = self._noise_dev()
        return {} if noise is None or noise[1] is None else {"noise_var": noise[1]}

    def missing_counts(self):
        """
        (n_missing_b, n_missing_bt): the number of NaN entries of b and of bt the last table build integrated out (of a
        bt (C, U, K): NaN session entries, so a patient padded from 2 to K sessions counts K - 2 per connection).  Needs
        missing_data = True and a table build (run(), _update_lps()); the counts come from the table kernel, so this
        read waits for it.
        """
        if not self.missing_data or not self._d.get("n_missing_valid"):
            raise ValueError("missing_counts() needs missing_data = True and a table build (run() or _update_lps())")
        (nb, nbt) = self._d["n_missing"].cpu().tolist()
        return (int(nb), int(nbt))

    @staticmethod
    def _array_key(a):
        a = np.asarray(a)
        return (id(a), a.__array_interface__["data"][0], a.shape, a.strides, a.dtype.str)

    @staticmethod
    def _data_digest(a, mode="full"):
        """
        Digest of an input array, by `data_check` mode.
        'full'    CRC-32 of the WHOLE array: sees any in-place edit (a single element, one patient's column), at 1-2 GB/s
                  of host time per call (round 3 ran it on every _update_lps: 8.6 ms per variational iteration at cfg3,
                  165 ms at cfg5, beside 0.5 / 2.5 ms of kernels -- VERDICT r3).
        'sample'  (default) CRC-32 of 4096 elements taken with a stride that is coprime to the row length, so that
                  every column (of a bt (C, U, K): every session of every patient; the row is a connection's U*K
                  values) is visited ~4096/U times: sees whole-array edits (scaling, clipping, Fisher z) and
                  whole-column edits; an edit of a few single elements between two _update_lps() calls of the same
                  fit needs invalidate_data() (documented contract; _init_lps() and run() always upload afresh).
        'none'    identity / address / shape only.
        """
        import zlib
        from math import gcd
        flat = np.ascontiguousarray(a).reshape(-1)
        if mode == "none":
            return 0
        if mode == "full" or flat.size <= 8192:
            return zlib.crc32(flat.view(np.uint8))
        if mode != "sample":
            raise ValueError("data_check must be 'sample', 'full' or 'none'")
        row = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1      # (C, U, K): a row is a connection's U*K values
        step = max(1, flat.size // 4096)
        while gcd(step, row) != 1:
            step += 1
        return zlib.crc32(np.ascontiguousarray(flat[::step]).view(np.uint8)) ^ zlib.crc32(flat[-64:].view(np.uint8))

    def invalidate_data(self):
        """Forget the device copies of b / bt: the next _update_lps() uploads them again (after in-place edits)."""
        self._d.pop("data_key", None)

    def _is_converged(self, s):
        """fit.py:124-140 (quirk Q6 kept: a negative energy makes any decrease 'converged')."""
        e = self.energy[s - 1]
        e_star = self.energy[s]
        return ((e - e_star) / e) < self.rel_tol

    def _eval_energy(self):
        """Variational free energy (fit.py:142-155): kernel K_energy."""
        return float(self._energy_terms_signed().sum())

    def _energy_terms(self):
        t = self._torch()
        (N, C, U) = self._check_state()
        out = t.empty(6, dtype=t.float64, device=self._dev())
        self._context().call("fcd_vb_energy", _lib.dptr(self._d["lq_F"]), _lib.dptr(self._d["lq_R"]),
                             _lib.dptr(self._d["S_B"]), _lib.dptr(self._d["lM"]), _lib.dptr(self._hyper()), N, U,
                             _lib.dptr(out), _lib.stream_ptr())
        return out.cpu().numpy()

    def _energy_terms_signed(self):
        return self._energy_terms() * np.array([-1.0, -1.0, -1.0, -1.0, 1.0, 1.0])

    def _update_lq_F(self):
        """Probability of the typical network template (fit.py:157-174): kernel K_qF."""
        t = self._torch()
        (N, C, U) = self._check_state(need=("lq_R", "S_B"))
        out = t.empty((C, 1, 3), dtype=t.float64, device=self._dev())
        self._context().call("fcd_vb_update_qF", _lib.dptr(self._d["lq_R"]), _lib.dptr(self._d["S_B"]),
                             _lib.dptr(self._d["lM"]), _lib.dptr(self._hyper()), N, U, _lib.dptr(out),
                             _lib.stream_ptr())
        self._d["lq_F"] = out

    def _update_lq_R(self):
        """Probability of the anomalous regions (fit.py:176-198): kernel K_qR (Gauss-Seidel over regions)."""
        (N, C, U) = self._check_state(need=("lq_R", "lq_F"))
        lq_R = self._d["lq_R"].clone()
        self._context().call("fcd_vb_update_qR", _lib.dptr(self._d["lq_F"]), _lib.dptr(self._d["lM"]),
                             _lib.dptr(self._hyper()), N, U, _lib.EDGE_MODES[self._edge_mode()], _lib.dptr(lq_R),
                             _lib.stream_ptr())
        self._d["lq_R"] = lq_R

    def _update_theta(self):
        """fit.py:200-206."""
        lq_R, lq_F = self._d.get("lq_R"), self._d.get("lq_F")
        if (lq_R is not None and lq_F is not None and lq_R.dim() == 3 and lq_F.dim() == 3
                and int(lq_F.shape[0]) == util.N_to_C(int(lq_R.shape[0]))):
            # both closed forms come out of ONE launch (and one read-back): the same four numbers _update_pi() and
            # _update_gamma() would each ask the kernel for
            out = self._theta_step(lq_R=lq_R, lq_F=lq_F)
            self.model.pi = float(out[0])
            self.model.gamma = out[1:4].copy()
        else:
            self._update_pi()
            self._update_gamma()
        if self.update_theta_sub:
            self._update_theta_sub()

    def _theta_step(self, lq_R=None, lq_F=None):
        """out4 = {mean q_R[:,:,1], mean_c q_F} from the given (or the current) log-probabilities."""
        t = self._torch()
        lq_R = self._d.get("lq_R") if lq_R is None else lq_R
        lq_F = self._d.get("lq_F") if lq_F is None else lq_F
        if lq_R is None or lq_F is None:
            raise ValueError("_lq_R / _lq_F have not been initialized (_init_lps)")
        if lq_R.dim() != 3 or int(lq_R.shape[2]) != 2 or lq_F.dim() != 3 or tuple(lq_F.shape[1:]) != (1, 3):
            raise ValueError("_lq_R must have shape (N, U, 2) and _lq_F (C, 1, 3), got %s and %s"
                             % (tuple(lq_R.shape), tuple(lq_F.shape)))
        (N, U) = (int(lq_R.shape[0]), int(lq_R.shape[1]))
        if util.N_to_C(N) != int(lq_F.shape[0]):
            raise ValueError("_lq_F and _lq_R disagree on the number of regions")
        out = t.empty(4, dtype=t.float64, device=self._dev())
        self._context().call("fcd_vb_theta_step", _lib.dptr(lq_F), _lib.dptr(lq_R), N, U, _lib.dptr(out),
                             _lib.dptr(None), _lib.stream_ptr())
        return out.cpu().numpy()

    def _update_pi(self):
        """pi* = mean q_R[:, :, 1] (fit.py:208-213); a scalar, as in the reference."""
        t = self._torch()
        lq_R = self._d.get("lq_R")
        if lq_R is None:
            raise ValueError("_lq_R has not been initialized (_init_lps)")
        # pi* needs q_R only (the reference's test sets nothing else, test_fit.py:513-533): q_F is a local stand-in
        # of the matching size, never stored
        lq_F = self._d.get("lq_F")
        if lq_F is None or lq_R.dim() != 3 or int(lq_F.shape[0]) != util.N_to_C(int(lq_R.shape[0])):
            lq_F = t.full((util.N_to_C(int(lq_R.shape[0])), 1, 3), -np.log(3), dtype=t.float64, device=self._dev())
        self.model.pi = float(self._theta_step(lq_R=lq_R, lq_F=lq_F)[0])

    def _update_gamma(self):
        """gamma* = mean_c q_F (fit.py:215-220)."""
        t = self._torch()
        lq_F = self._d.get("lq_F")
        if lq_F is None:
            raise ValueError("_lq_F has not been initialized (_init_lps)")
        # gamma* needs q_F only (test_fit.py:536-557): q_R is a local (N, 1, 2) stand-in, never stored
        N = util.C_to_N(int(lq_F.shape[0]))
        if (N % 1) != 0:
            raise ValueError("Number of connections (%u) must be a triangular number." % int(lq_F.shape[0]))
        lq_R = self._d.get("lq_R")
        if lq_R is None or int(lq_R.shape[0]) != int(N):
            lq_R = t.full((int(N), 1, 2), -np.log(2), dtype=t.float64, device=self._dev())
        self.model.gamma = self._theta_step(lq_R=lq_R, lq_F=lq_F)[1:4].copy()

    def diagnostics(self):
        """
        split-R-hat / effective sample size of the per-chain traces of the last gibbs run (trace_every > 0): the
        log-joint (the summary's own keys, as before) and, under "sum_r", the number of anomalous sites sum_{n,u} r_nu.
        """
        from . import diagnostics as D
        if self.trace is None or self.trace.shape[1] < 4:
            raise ValueError("no trace: set trace_every > 0 and keep at least 4 recorded sweeps after burn_in")
        out = D.summary(self.trace)
        if self.trace_r is not None:
            out["sum_r"] = D.summary(self.trace_r)
        return out

    def _update_theta_sub(self):
        """
        Not provided for sessions data bt (C, U, K) nor with noise variances: NotImplementedError before anything is launched.

        Updates (eta, epsilon) (fit.py:222-241): bounded minimisation of -E_lM with the other terms fixed, bounds
        (1e-5, 1 - 1e-5) on both, L-BFGS-B.  The reference's version cannot run (it calls the undefined `opt_fun`,
        fit.py:239) and would difference the objective numerically (`jac=False`); here objective AND its two analytic
        derivatives (the formulas of `_eval_dE_dh` / `_eval_dE_de`, fit.py:600-697) come from one kernel pass over bt.
        theta_sub_params = 'eta_epsilon' (default): mu and sigma stay fixed, as in the reference as shipped (commented
        out of its optimiser, fit.py:232-237, 250-251); 'all' reads those lines in: (eta, epsilon, mu, sigma^2) jointly,
        objective E[ln p(b|f)] + E[ln p(bt|f,r)] (fit.py:282), fcd_theta_full_objective.
        """
        if self._has_sessions():
            raise NotImplementedError("the theta_sub step is not provided for sessions data bt (C, U, K): its objective "
                                      "kernels read one scan per patient")
        if self._has_noise():
            raise NotImplementedError("the theta_sub step is not provided with noise variances (b_noise_var / bt_noise_var): "
                                      "its objective kernels take one sigma per state")
        W = self._theta_sub_weights()
        if self.theta_sub_params == "all":
            # the reference's commented-out intent (fit.py:232-237, 250-251, 266-267, 282): mu and sigma too
            (eta, epsilon, mu, sigma, info) = minimize_theta_full(self._context(), self._d["b"], self._d["bt"], W, self.model,
                                                                  **self._theta_sub_flags())
            self.model.mu, self.model.sigma = mu, sigma
        elif self.theta_sub_params == "eta_epsilon":
            (eta, epsilon, info) = minimize_theta_sub(self._context(), self._d["bt"], W, self.model,
                                                      **self._theta_sub_flags())
        else:
            raise ValueError("theta_sub_params must be 'eta_epsilon' or 'all'")
        self.model.eta, self.model.epsilon = eta, epsilon
        self._theta_sub_info = info

    def _theta_sub_flags(self):
        """How the theta_sub objectives read W and the data (keyword arguments of minimize_theta_sub / _full)."""
        return {"missing_data": self.missing_data}

    def _theta_sub_weights(self):
        """W[c,u,k,l] = q_F[c,k] * w_l(c,u) on the device (fit.py:382-406, 508-510)."""
        t = self._torch()
        (N, _C, U) = self._check_state(need=("lq_R", "lq_F"))
        lq_R, lq_F = self._d["lq_R"], self._d["lq_F"]
        W = t.empty((util.N_to_C(N), U, 3, 3), dtype=t.float64, device=self._dev())
        self._context().call("fcd_theta_sub_weights_vb", _lib.dptr(lq_F), _lib.dptr(lq_R), N, U, _lib.dptr(W),
                             _lib.stream_ptr())
        return self._expand_weights(W)

    # ------------------------------------------------------------------ gibbs
    def _run_gibbs(self, N, U):
        """
        Many-chain collapsed Gibbs over (f, r) with an MCEM step for (pi, gamma) from statistics pooled
        over all chains of all ranks.  On return `_lq_F` / `_lq_R` hold the logs of the chain-and-sweep
        averaged marginals, `model.pi` / `model.gamma` the last M-step, `energy` minus the mean
        log-joint at the recorded sweeps.
        """
        t = self._torch()
        self.coanomaly_states = 0
        for a in GIBBS_ACCUMULATORS:
            for name in a.results + a.meta:
                setattr(self, name, None)
            setattr(self, a.sweeps, 0)
        live = [a for a in GIBBS_ACCUMULATORS if self._accumulator_on(a)]
        for a in live:
            getattr(self, a.check or "_check_accumulator_row")(a, N, U)
        eng = GibbsEngine(self._d["S_B"], self._d["lM"], N, U, self.n_chains, chain0=self.chain0, seed=self.seed,
                          edge_index=self._edge_mode(), ctx=self._context())
        for a in live:      # (in the table's order: the region sets are set before the accumulators that take them as rows)
            if a.give:
                getattr(self, a.give)(eng)
            getattr(eng, "attach_%s_accumulator" % a.engine.key)(getattr(self, a.every))
        pi2 = self._pi2()
        eng.set_hyper(np.asarray(self.model.gamma, dtype=np.float64), pi2)
        eng.init(float(pi2[1]))
        self.energy = []

        traces = []
        traces_r = []

        def record(i, e):
            want_e = bool(self.energy_every and (i + 1) % self.energy_every == 0)
            want_t = bool(self.trace_every and i >= self.burn_in and (i + 1) % self.trace_every == 0)
            if want_e or want_t:
                lj = e.logjoint()
                if want_e:
                    self.energy.append(-float(lj.mean()))
                if want_t:
                    traces.append(e.host(lj))
                    traces_r.append(e.host(e.r_sums()))
            if self.update_theta_sub and self.theta_sub_every and (i + 1) % self.theta_sub_every == 0 and i + 1 < self.n_sweeps:
                # Monte-Carlo EM for (eta, epsilon): pooled counts of (f_c, mixture case) over all chains of all ranks
                W = self._expand_weights(e.pair_counts())
                if self.theta_sub_params == "all":
                    (eta, epsilon, mu, sigma, _info) = minimize_theta_full(self._context(), self._d["b"], self._d["bt"], W,
                                                                           self.model, reduce=allreduce_counts,
                                                                           **self._theta_sub_flags())
                    self.model.mu, self.model.sigma = mu, sigma
                else:
                    (eta, epsilon, _info) = minimize_theta_sub(self._context(), self._d["bt"], W, self.model,
                                                               reduce=allreduce_counts, **self._theta_sub_flags())
                self.model.eta, self.model.epsilon = eta, epsilon
                self._update_lps()            # tables follow theta_sub ...
                e.refresh_tables()            # ... and so do the sampler's two difference tables
        needs_callback = bool(self.energy_every or self.trace_every or (self.update_theta_sub and self.theta_sub_every))
        run_chains(eng, self.n_sweeps, sweep0=0, mstep_every=self.mstep_every, burn_in=self.burn_in,
                   update_theta=True, on_sweep=record if needs_callback else None, mstep_lag=self.mstep_lag)
        self.sampler = eng
        self.trace = np.stack(traces, axis=1) if traces else None
        self.trace_r = np.stack(traces_r, axis=1).astype(np.float64) if traces_r else None
        # marginals pooled over this rank's chains and, when distributed, over all ranks
        cnt = t.cat([eng.cnt_f.reshape(-1).to(t.int64), eng.cnt_r.reshape(-1).to(t.int64),
                     t.tensor([eng.n_accumulated * eng.G], dtype=t.int64, device=eng.cnt_f.device)])
        cnt = allreduce_counts(cnt).cpu().numpy().astype(np.float64)
        # (that read waited for every sweep: a pipelined r pass that gave up a device-side wait has raised the
        # context's error word by now -- no marginals, pi or gamma from such a state)
        eng.ctx.check_device()
        C = util.N_to_C(N)
        total = max(cnt[-1], 1.0)
        with np.errstate(divide="ignore"):
            self._lq_F = np.log(cnt[:3 * C].reshape(C, 1, 3) / total)
            p1 = cnt[3 * C:3 * C + N * U].reshape(N, U) / total
            self._lq_R = np.log(np.stack([1.0 - p1, p1], axis=2))
        for a in live:
            bufs = getattr(eng, a.engine.attr)
            for (name, buf, dtype) in zip(a.results, bufs if a.engine.paired else (bufs,), a.engine.dtypes):
                # (uint32 counts pool as int64 values; an int64 buffer of signed sums is summed as it is, on a copy)
                setattr(self, name, (pool_u32(buf) if dtype == "int32" else allreduce_counts(buf.clone())).cpu().numpy())
            setattr(self, a.sweeps, getattr(eng, a.engine.key + "_sweeps"))
            if a.collect:
                getattr(self, a.collect)(eng)
        (gamma, pi) = eng.hyper_values()
        self.model.gamma = gamma
        self.model.pi = pi

    # ---- the rows of GIBBS_ACCUMULATORS: which are on, and the hooks they name ----
    def _accumulator_on(self, a):
        knob = getattr(self, a.knob)
        return knob is not None if a.give else bool(knob)

    def _check_accumulator_row(self, a, N, U):
        self._check_accumulator(a.every, a.label, sites=a.engine.sites(N, U) if a.engine.sites else 1)

    def _check_anomaly_counts(self, a, N, U):
        self._check_accumulator_row(a, N, U)
        if N > COUNT_MAX_NREG or U > COUNT_MAX_U:
            raise ValueError("anomaly-count histograms are made for at most %d regions and %d patients (here %d, %d)"
                             % (COUNT_MAX_NREG, COUNT_MAX_U, N, U))

    def _collect_coanomaly(self, eng):
        t = self._torch()
        states = t.tensor([eng.coanomaly_sweeps * eng.G], dtype=t.int64, device=eng.cnt_f.device)
        self.coanomaly_states = int(allreduce_counts(states).cpu()[0])

    def _check_region_sets(self, a, N, U):
        region_sets_csr(self.region_sets, N)
        self._check_accumulator_row(a, N, U)
        if U > COUNT_MAX_U:
            raise ValueError("region-set histograms are made for at most %d patients (here %d)" % (COUNT_MAX_U, U))

    def _give_region_sets(self, eng):
        eng.set_region_sets(self.region_sets)

    def _collect_region_sets(self, eng):
        (self.region_set_names, self.region_set_sizes) = (list(eng.region_names), np.diff(eng.region_offsets).astype(np.int64))

    def _check_patient_groups(self, a, N, U):
        self._refuse_patient_groups_shared()
        patient_group_contrasts(self.patient_group_contrasts, *patient_groups_csr(self.patient_groups, U))
        self._check_accumulator_row(a, N, U)

    def _give_patient_groups(self, eng):
        eng.set_patient_groups(self.patient_groups, self.patient_group_contrasts)

    def _collect_patient_groups(self, eng):
        """The names behind the histograms, and the flat joint histogram as one (R, |a|+1, |b|+1) array per contrast."""
        (hj, R) = (self.patient_group_joint_hist, self.patient_group_hist.shape[1])
        sizes = np.diff(eng.group_offsets).astype(np.int64)
        self.patient_group_joint_hist = [
            hj[R * lo:R * hi].reshape(R, sizes[a] + 1, sizes[b] + 1)
            for ((a, b), lo, hi) in zip(eng.group_contrasts, eng.group_bin_offsets[:-1], eng.group_bin_offsets[1:])]
        (self.patient_group_names, self.patient_group_sizes) = (list(eng.group_names), sizes)
        (self.patient_group_rows, self.patient_group_pairs) = (eng.patient_group_row_names(), eng.group_contrasts.copy())

    def _check_patient_traits(self, a, N, U):
        self._refuse_patient_traits_shared()
        patient_traits_scores(self.patient_traits, U)
        self._check_accumulator_row(a, N, U)

    def _give_patient_traits(self, eng):
        eng.set_patient_traits(self.patient_traits)

    def _collect_patient_traits(self, eng):
        (self.patient_trait_names, self.patient_trait_n_known) = (list(eng.trait_names), eng.trait_n_known.copy())
        self.patient_trait_rows = eng.patient_trait_row_names()

    def _check_accumulator(self, knob, what, sites=1):
        """A uint32 accumulator of the gibbs run: its period self.<knob> is an integer >= 1 and, at that period, chains x
        accumulated sweeps (x `sites`, where one counter takes that many sites of a chain) fit the counter."""
        every = getattr(self, knob)
        if int(every) < 1 or int(every) != every:
            raise ValueError("%s must be an integer >= 1" % knob)
        n_acc = pair_sweeps_in(0, int(self.n_sweeps), int(self.burn_in), int(every))
        if n_acc * int(self.n_chains) * int(sites) > PAIR_COUNT_MAX:
            raise ValueError("%s would overflow uint32: %d chains x %d accumulated sweeps%s; raise %s"
                             % (what, self.n_chains, n_acc, " x %d sites" % sites if sites > 1 else "", knob))

    # ------------------------------------------------------------------ connection-level posteriors
    def _connection_counts_dev(self):
        """
        (counts, N, C): `connection_counts` (C, U, 3, 3) of the last gibbs run as the uint32-in-int32 device tensor
        conn_posterior() takes; ValueError where there are none, nothing was accumulated or a pooled count is over uint32.
        """
        cnt = self.connection_counts
        if cnt is None:
            raise ValueError("no connection counts: set connection_marginals = True before run(method='gibbs')")
        cnt = np.asarray(cnt)
        if int(cnt[0, 0].sum()) == 0:
            raise ValueError("no sweep was accumulated into the connection counts (n_sweeps <= burn_in?)")
        if int(cnt.max()) > PAIR_COUNT_MAX:
            raise ValueError("pooled connection counts exceed uint32; raise connection_every")
        counts = self._torch().as_tensor(np.ascontiguousarray(cnt.astype(np.uint32).view(np.int32)), device=self._dev())
        return counts, int(util.C_to_N(cnt.shape[0])), cnt.shape[0]

    def connection_posterior(self):
        """
        Posterior of the anomalous connections and of each patient's connection state, per connection and patient (edge
        order of `b` / `bt`), from the last run():
            p_T        (C, U)     P(T_cu = 1 | data)
            p_F_tilde  (C, U, 3)  P(F~_cu = j | data), j = negative, none, positive (rows sum to 1)
            p_changed  (C, U)     P(F~_cu != F_c | data)
        as a dict of float64 arrays.  Given f_c = k, the mixture case l of (r_n, r_m) -- n, m the true endpoints of c, in
        either edge-id mode -- and bt_cu, T and F~ have a closed-form law (doc/methods.rst:70-177); it is averaged over
        the fit's posterior of (f_c, l_cu) with theta = the model's CURRENT parameters (the plug-in convention of _lq_F /
        _lq_R):
          method='vb'     the mean-field weights q_F[c,k] w_l(c,u) of _lq_F, _lq_R (computed on demand);
          method='gibbs'  the counts of (f_c = k, l_cu = l) over chains and the sweeps from burn_in on, every
                          `connection_every`-th (Rao-Blackwellised).  Needs `connection_marginals = True` before run();
                          raises ValueError otherwise.  The counts are kept as `connection_counts` (C, U, 3, 3), the
                          number of sweeps behind them as `connection_sweeps`.  With
                          update_theta_sub and theta_sub_every, counts made under earlier (eta, epsilon) are contracted
                          with the final theta all the same.
        With missing_data = True a NaN bt[c,u] takes N_j = 1 in the closed forms: the prior law of T and F~ given (k, l),
        averaged over the same weights.
        """
        if self.model is None or self.bt is None:
            raise ValueError("connection_posterior() needs a model and bt: call run() first")
        if self.method == "gibbs":
            (counts, N, C) = self._connection_counts_dev()
            U = int(counts.shape[1])
            return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), counts=counts,
                                  missing_data=self.missing_data, **self._noise_bt_kw())
        if self.method != "vb":
            raise ValueError("method must be 'vb' or 'gibbs'")
        (N, C, U) = self._check_state(need=("lq_R", "lq_F"))
        return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), lq_F=self._d["lq_F"],
                              lq_R=self._d["lq_R"], missing_data=self.missing_data, **self._noise_bt_kw())

    # ------------------------------------------------------------------ anomalous-region counts
    def anomaly_count_posterior(self):
        """
        Posterior law of how many regions of each patient are anomalous and in how many patients each region is, from the
        last run(), as a dict of NumPy float64 arrays:
            p_patient_count  (U, Nreg+1)  P(sum_n r_nu = k | data)
            p_region_count   (Nreg, U+1)  P(sum_u r_nu = k | data)
            p_patient_any    (U,)         P(patient u has an anomalous region) = 1 - p_patient_count[:, 0]
            p_region_any     (Nreg,)      P(region n is anomalous in some patient) = 1 - p_region_count[:, 0]
        The sites are coupled (inside a patient through the mixture cases of the edges, across patients through f), so
        these are laws of the joint, not products of the marginals of _lq_R:
          method='vb'     the mean-field law: under q_R the sites are independent and each count is Poisson-binomial
                          (computed on demand from _lq_R);
          method='gibbs'  the histograms over chains and the sweeps from burn_in on, every `anomaly_counts_every`-th.
                          Needs `anomaly_counts = True` before run(); raises ValueError otherwise.  The histograms are
                          kept as `patient_count_hist` / `region_count_hist`, the number of sweeps behind them as
                          `anomaly_count_sweeps`.
        """
        if self.model is None or self.bt is None:
            raise ValueError("anomaly_count_posterior() needs a model and bt: call run() first")
        if self.method == "gibbs":
            (hp, hr) = (self.patient_count_hist, self.region_count_hist)
            if hp is None or hr is None:
                raise ValueError("no anomaly-count histograms: set anomaly_counts = True before run(method='gibbs')")
            (hp, hr) = (np.asarray(hp, dtype=np.float64), np.asarray(hr, dtype=np.float64))
            if hp.sum() == 0 or hr.sum() == 0:
                raise ValueError("no sweep was accumulated into the anomaly-count histograms (n_sweeps <= burn_in?)")
            p_patient = hp / hp.sum(axis=1, keepdims=True)
            p_region = hr / hr.sum(axis=1, keepdims=True)
        elif self.method == "vb":
            (N, _C, U) = self._check_state(need=("lq_R",))
            (p_patient, p_region) = count_posterior(self._context(), self._d["lq_R"], N, U)
        else:
            raise ValueError("method must be 'vb' or 'gibbs'")
        return {"p_patient_count": p_patient, "p_region_count": p_region,
                "p_patient_any": 1.0 - p_patient[:, 0], "p_region_any": 1.0 - p_region[:, 0]}

    # ------------------------------------------------------------------ counts over sets of regions (networks)
    def region_set_posterior(self, independent=False):
        """
        Posterior law of the anomalous regions inside each of the sets of `region_sets` (the networks of an atlas, say), from
        the last run(), as a dict of NumPy float64 arrays (J sets, S_max the size of the largest):
            names, sizes                     the sets, in the order given (a list of str, (J,) int64)
            p_count       (J, U, S_max+1)    P(sum_{n in S_j} r_nu = k | data); zero beyond the set's size, rows sum to 1
            p_any         (J, U)             P(patient u has an anomalous region in S_j) = 1 - p_count[..., 0]
            expected      (J, U)             E[sum_{n in S_j} r_nu | data]
            p_prevalence  (J, U+1)           P(exactly k patients have an anomalous region in S_j | data)
            p_none        (J,)               P(no patient has) = p_prevalence[:, 0]
        The sites of a patient are coupled through the mixture cases of their edges, so P(some n in S: r_nu = 1) is NOT
        1 - prod_n (1 - P(r_nu = 1)):
          method='gibbs', independent=False   the histograms over chains and the sweeps from burn_in on, every
                          `region_sets_every`-th.  Needs `region_sets` set before run(); raises ValueError otherwise.  The
                          histograms are kept as `region_set_hist` / `region_set_prevalence_hist`, the number of sweeps
                          behind them as `region_set_sweeps`.
          method='vb', or independent=True on either method   the mean-field law of _lq_R with the CURRENT `region_sets`:
                          the count is Poisson-binomial over the set's rows, the prevalence Poisson-binomial over u with
                          p_u = 1 - prod_{n in S} (1 - q1(n, u)) (both through fcd_vb_count_posterior).
        For a sampler fit, joint minus independent is the excess, the convention of coanomaly_posterior().
        SharedRegionFit: the patient extent is 1; p_count[j, 0] is the law of how many regions of S_j the population's map
        holds.  Not provided: set posteriors of new patients in score() and membership().
        """
        if self.model is None or self.bt is None:
            raise ValueError("region_set_posterior() needs a model and bt: call run() first")
        if self.method not in ("vb", "gibbs"):
            raise ValueError("method must be 'vb' or 'gibbs'")
        if self.method == "gibbs" and not independent:
            (hs, hv) = (self.region_set_hist, self.region_set_prevalence_hist)
            if hs is None or hv is None:
                raise ValueError("no region-set histograms: set region_sets before run(method='gibbs')")
            (hs, hv) = (np.asarray(hs, dtype=np.float64), np.asarray(hv, dtype=np.float64))
            if hs.sum() == 0 or hv.sum() == 0:
                raise ValueError("no sweep was accumulated into the region-set histograms (n_sweeps <= burn_in?)")
            (names, sizes) = (list(self.region_set_names), np.asarray(self.region_set_sizes, dtype=np.int64))
            p_count = hs / hs.sum(axis=2, keepdims=True)
            p_prev = hv / hv.sum(axis=1, keepdims=True)
        else:
            if self.region_sets is None:
                raise ValueError("no region sets: set region_sets first")
            (N, _C, U) = self._check_state(need=("lq_R",))
            (names, offsets, members) = region_sets_csr(self.region_sets, N)
            (p_count, p_prev) = region_set_independent(self._context(), self._d["lq_R"], N, U, offsets, members)
            sizes = np.diff(offsets).astype(np.int64)
        k = np.arange(p_count.shape[2], dtype=np.float64)
        return {"names": names, "sizes": sizes, "p_count": p_count, "p_any": 1.0 - p_count[:, :, 0], "expected": p_count @ k,
                "p_prevalence": p_prev, "p_none": p_prev[:, 0].copy()}

    # ------------------------------------------------------------------ groups of patients and contrasts between them
    def _refuse_patient_groups_shared(self):
        if self._shared:
            raise ValueError("patient_groups compare the patients' own anomaly maps; SharedRegionFit has one population-level r")

    def patient_group_posterior(self, independent=False, level=0.95):
        """
        Is row rho anomalous more often in one group of patients than in another?  For the groups of `patient_groups` and the
        contrasts of `patient_group_contrasts` (pairs of two disjoint groups), from the last run(), as a dict (J groups, Umax
        the size of the largest, P contrasts; R rows: the Nreg regions and, with `region_sets`, the sets after them, whose
        indicator is "patient u has an anomalous region in S"):
            names, sizes, row_names          the groups in the order given (list of str, (J,) int64); "0" .. "Nreg-1", "set:<name>"
            p_count       (J, R, Umax+1)     P(k_j = k | data), k_j = number of patients of g_j anomalous at the row; zero
                                             beyond the group's size, rows sum to 1
            prevalence    (J, R)             E[k_j] / |g_j|
            contrasts                        the contrasts as pairs (name of a, name of b)
            p_joint       list of P arrays (R, |a|+1, |b|+1)     P(k_a = i, k_b = l | data)
            p_greater, p_less, p_equal  (P, R)     P(k_a/|a| > k_b/|b|), <, = (compared as integers, k_a |b| against k_b |a|)
            diff_mean     (P, R)             E[k_a/|a| - k_b/|b|]
            diff_interval (P, R, 2)          the central `level` interval of the law of k_a/|a| - k_b/|b|: the smallest values
                                             of the difference at which its cumulative probability reaches (1 - level)/2 and
                                             (1 + level)/2 (to within 1e-12)
        Patients are coupled through f, so k_j is NOT Poisson-binomial in the per-patient marginals, and the law of a
        difference needs the joint law of both counts:
          method='gibbs', independent=False   the histograms over chains and the sweeps from burn_in on, every
                          `patient_groups_every`-th.  Needs `patient_groups` set before run(); raises ValueError otherwise.
                          The histograms are kept as `patient_group_hist` / `patient_group_joint_hist` (one array per
                          contrast), the number of sweeps behind them as `patient_group_sweeps`.
          method='vb', or independent=True on either method   the mean-field law of _lq_R with the CURRENT groups, contrasts
                          and region sets: k_j is Poisson-binomial over the group's columns, at a set row with
                          p_u = 1 - prod_{n in S} (1 - q1(n, u)) (both through fcd_vb_count_posterior); the joint of a
                          contrast is the outer product of its two marginals (its groups are disjoint).
        For a sampler fit, joint minus independent is the excess, the convention of coanomaly_posterior().
        SharedRegionFit has one population-level r: ValueError.  Not provided: groups in score() and membership().
        """
        self._refuse_patient_groups_shared()
        if self.model is None or self.bt is None:
            raise ValueError("patient_group_posterior() needs a model and bt: call run() first")
        if self.method not in ("vb", "gibbs"):
            raise ValueError("method must be 'vb' or 'gibbs'")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie in (0, 1)")
        if self.method == "gibbs" and not independent:
            (hg, hj) = (self.patient_group_hist, self.patient_group_joint_hist)
            if hg is None or hj is None:
                raise ValueError("no patient-group histograms: set patient_groups before run(method='gibbs')")
            hg = np.asarray(hg, dtype=np.float64)
            if hg.sum() == 0:
                raise ValueError("no sweep was accumulated into the patient-group histograms (n_sweeps <= burn_in?)")
            (names, sizes) = (list(self.patient_group_names), np.asarray(self.patient_group_sizes, dtype=np.int64))
            (row_names, pairs) = (list(self.patient_group_rows), np.asarray(self.patient_group_pairs, dtype=np.int64).reshape(-1, 2))
            p_count = hg / hg.sum(axis=2, keepdims=True)
            p_joint = [np.asarray(h, dtype=np.float64) / np.asarray(h, dtype=np.float64).sum(axis=(1, 2), keepdims=True) for h in hj]
        else:
            if self.patient_groups is None:
                raise ValueError("no patient groups: set patient_groups first")
            (N, _C, U) = self._check_state(need=("lq_R",))
            (names, offsets, members) = patient_groups_csr(self.patient_groups, U)
            (pairs, _bins) = patient_group_contrasts(self.patient_group_contrasts, names, offsets, members)
            sizes = np.diff(offsets).astype(np.int64)
            row_names = [str(n) for n in range(N)]
            sets = None
            if self.region_sets is not None:
                sets = region_sets_csr(self.region_sets, N)
                row_names += ["set:" + name for name in sets[0]]
            p_count = patient_group_independent(self._context(), self._d["lq_R"], N, U, offsets, members,
                                                None if sets is None else sets[1:])
            p_joint = [p_count[a, :, :sizes[a] + 1, None] * p_count[b, :, None, :sizes[b] + 1] for (a, b) in pairs]
        out = {"names": names, "sizes": sizes, "row_names": row_names, "p_count": p_count,
               "contrasts": [(names[a], names[b]) for (a, b) in pairs], "p_joint": p_joint}
        out.update(patient_group_summaries(p_count, p_joint, sizes, pairs, level))
        return out

    # ------------------------------------------------------------------ anomalies against an ordered trait of the patients
    def _refuse_patient_traits_shared(self):
        if self._shared:
            raise ValueError("patient_traits relate the patients' own anomaly maps to a trait; SharedRegionFit has one "
                             "population-level r")

    def patient_trait_posterior(self, level=0.95):
        """
        Do the patients that are anomalous at row rho have the higher (or lower) trait?  For every trait of `patient_traits`
        (values per patient; NaN = not known) and every row -- the Nreg regions and, with `region_sets`, the sets after them,
        whose indicator is "patient u has an anomalous region in S" --, the posterior law of the rank-sum (Mann-Whitney)
        statistic between the known patients that are anomalous at the row and those that are not:
        AUC = P(an anomalous patient has the higher trait) + P(tie) / 2.  No threshold on the trait is needed, and only its
        order counts.  A state with k anomalous among the n_q known patients is DEFINED where 0 < k < n_q.  From the last
        run(method='gibbs'), as a dict (Q traits, Umax the largest n_q, R rows, NB = 128):
            names, n_known, rows             the traits in the order given (list of str, (Q,) int64); "0" .. "Nreg-1", "set:<name>"
            p_count     (Q, R, Umax+1)       P(k = i | data); zero beyond n_q, rows sum to 1
            p_defined   (Q, R)               P(0 < k < n_q | data)
            p_greater, p_less, p_equal  (Q, R)     P(AUC > 1/2), <, = among the defined states (decided on integers); NaN
                                             where no state is defined
            auc_mean    (Q, R)               E[AUC | defined], exact: from the sums of the integer statistic per k; NaN likewise
            auc_hist    (Q, R, NB), auc_edges (NB+1,)     the law of AUC among the defined states in bins of width 1/NB (the
                                             last bin holds AUC = 1); NaN likewise
            auc_interval (Q, R, 2)           the outer edges of the bins in which the cumulative law reaches (1 - level)/2 from
                                             below and from above (to within 1e-12): never narrower than the central `level`
                                             interval of the AUC itself; NaN likewise
            sweeps                           the number of sweeps behind the histograms
        For a binary trait (ones, zeros) the sign of AUC - 1/2 is the sign of the rate difference of the patient-group
        contrast (ones, zeros).  The patients are coupled through f, so the law does not follow from the per-patient marginals:
        the histograms are counted over chains and the sweeps from burn_in on, every `patient_traits_every`-th, and kept as
        `patient_trait_hist` / `patient_trait_sum`.  Needs `patient_traits` set before run(method='gibbs'); ValueError
        otherwise, and for method='vb' (the law needs the sampler's chains) and SharedRegionFit (one population-level r).
        Not provided: a mean-field or independent=True form (it needs a (k, A) convolution per row), and traits in score()
        and membership().
        """
        self._refuse_patient_traits_shared()
        if self.method != "gibbs":
            raise ValueError("patient_trait_posterior() needs method='gibbs': the law of the rank-sum statistic needs the "
                             "sampler's chains (the patients are coupled through f)")
        if not 0.0 < float(level) < 1.0:
            raise ValueError("level must lie in (0, 1)")
        (th, ts) = (self.patient_trait_hist, self.patient_trait_sum)
        if th is None or ts is None:
            if self.patient_traits is None:
                raise ValueError("no patient traits: set patient_traits before run(method='gibbs')")
            raise ValueError("no patient-trait histograms: call run(method='gibbs') first")
        n_known = np.asarray(self.patient_trait_n_known, dtype=np.int64)
        if np.asarray(th)[:, :, :int(n_known.max()) + 1].sum() == 0:
            raise ValueError("no sweep was accumulated into the patient-trait histograms (n_sweeps <= burn_in?)")
        out = {"names": list(self.patient_trait_names), "n_known": n_known, "rows": list(self.patient_trait_rows),
               "sweeps": int(self.patient_trait_sweeps)}
        out.update(patient_trait_summaries(th, ts, n_known, level))
        return out

    # ------------------------------------------------------------------ co-anomaly
    def _coanomaly_counts(self):
        """(region_pair_counts, patient_pair_counts, chain states behind them) of the last gibbs run, or ValueError."""
        (rp, pp) = (self.region_pair_counts, self.patient_pair_counts)
        if rp is None or pp is None:
            raise ValueError("no co-anomaly counts: set coanomaly = True before run(method='gibbs')")
        if int(self.coanomaly_states) < 1:
            raise ValueError("no sweep was accumulated into the co-anomaly counts (n_sweeps <= burn_in?)")
        return np.asarray(rp), np.asarray(pp), int(self.coanomaly_states)

    def coanomaly_posterior(self):
        """
        Which regions are anomalous together and which patients share anomalous regions, from the last run(), as a dict of
        NumPy float64 arrays:
            p_region_pair      (Nreg, Nreg)  (1/U) sum_u P(r_nu = 1, r_mu = 1 | data): for a patient picked at random, the
                                             chance that regions n and m are both anomalous
            expected_patients  (Nreg, Nreg)  U times that: the expected number of patients with both
            p_patient_pair     (U, U)        (1/Nreg) sum_n P(r_nu = 1, r_nv = 1 | data)
            expected_regions   (U, U)        Nreg times that: the expected number of anomalous regions u and v share
            p_region_pair_independent, p_patient_pair_independent
                                             the first and the third if the sites were independent with the fit's marginals
                                             (fcd_vb_coanomaly on _lq_R); joint minus independent is the excess co-anomaly
        All are symmetric; the diagonals are the means of the marginals, (1/U) sum_u P(r_nu = 1) and (1/Nreg) sum_n
        P(r_nu = 1).  The sites are coupled (inside a patient through the mixture cases of the edges, across patients
        through f), so the joint entries are second moments of the joint, not products of the marginals of _lq_R:
          method='vb'     the mean-field law: under q_R the sites are independent, so the joint entries EQUAL the
                          independent ones (computed on demand from _lq_R);
          method='gibbs'  the pair counts over chains and the sweeps from burn_in on, every `coanomaly_every`-th.  Needs
                          `coanomaly = True` before run(); raises ValueError otherwise.  The counts are kept as
                          `region_pair_counts` / `patient_pair_counts`, the number of sweeps behind them as
                          `coanomaly_sweeps`.
        """
        if self.model is None or self.bt is None:
            raise ValueError("coanomaly_posterior() needs a model and bt: call run() first")
        if self.method == "gibbs":
            (rp, pp, states) = self._coanomaly_counts()
        elif self.method != "vb":
            raise ValueError("method must be 'vb' or 'gibbs'")
        (N, _C, U) = self._check_state(need=("lq_R",))
        (ri, pi_) = coanomaly_independent(self._context(), self._d["lq_R"], N, U)
        out = {"p_region_pair_independent": ri / U, "p_patient_pair_independent": pi_ / N}
        if self.method == "gibbs":
            out.update(coanomaly_from_counts(rp, pp, states))
        else:
            out.update({"p_region_pair": ri / U, "expected_patients": ri, "p_patient_pair": pi_ / N, "expected_regions": pi_})
        return out

    # ------------------------------------------------------------------ scoring new patients
    def score(self, bt_new, *, connections=False, max_iters=100, tol=1e-8, n_anneal=200, n_sweeps=50, seed=None,
              noise_var=None):
        """
        Scores patients who were not in the fit: their anomaly maps and a per-patient likelihood measure, with the fitted
        template and theta held fixed.  Scoring is NOT a refit: the new patients never update the template F, q_F, the
        sampler's chains or theta, and score() leaves the fit exactly as it was (model, _lq_R, _lq_F, energy, the device
        tables, `sampler` and its state).  Call it after run().

        bt_new (C, U') correlations of the new patients in the fit's edge order (NaN = unobserved when missing_data), or
        (C, U', K') with K' sessions of every new patient; K' need not be the fit's n_sessions.
        noise_var (U',) or (U', K'): the new patients' measurement variances (see "Measurement noise"; a (U',) applies to
        every session).  A fit with noise variances refuses noise_var=None (ValueError): the caller says what the new
        patients' are, zeros included.  The control side keeps the fit's b_noise_var.
        theta is the model's CURRENT parameters, the plug-in convention of connection_posterior().  Given F and theta the
        patients are independent (doc/methods.rst): with method='vb' a new patient's numbers are exactly those it gets when
        scored alone; with method='gibbs' they have the same law (the random numbers of a site follow its column index).
          method='vb'     q_F and theta held; each new patient's q_R is iterated from uniform (as _init_lps) with the fit's
                          edge ids and taken at the first iteration where its own max_n |delta q_nu| < tol, or at
                          max_iters (`iters` (U',) per patient; `converged` (U',) False where max_iters was reached first);
                          elbo[u] = E_lM[u] + E_lp_R[u] - E_lq_R[u], a lower bound on E_{q_F} log p(bt_u | F).
          method='gibbs'  each chain's template draw f_g (the end state of the fit's sampler, G = its chains) held.
                          Annealed importance sampling over r from the prior (beta = 0) to p(r | f_g, bt) in n_anneal steps
                          (schedule: score.ais_schedule) estimates p(bt_u | f_g) per chain: log_pred[u] = log mean_g of it,
                          unbiased on the exp scale for the mean over the chains' f; log_pred_se (delta method) and ess
                          (sum w)^2 / sum w^2 of the weights.  Then n_sweeps r-only sweeps at beta = 1 (each samples
                          p(r | f_g, bt) exactly, chains equally weighted) give p_R, the count law and, with connections,
                          the connection posteriors.  Needs edge_index 'symmetric'.  A sharded fit scores each rank's own
                          chains and pools the counts and the AIS sums over ranks.  seed: key of the scoring sampler's random
                          numbers (None: derived from the fit's seed; never the fit's own numbers -- see score.SCORE_SWEEP0).
        Returns a dict of NumPy float64 arrays:
            p_R (Nreg, U') P(r_nu = 1);  p_patient_count (U', Nreg+1);  p_patient_any (U',)
            connections=True:  p_T (C, U'), p_F_tilde (C, U', 3), p_changed (C, U') of the new patients
            vb:     elbo (U',), iters (U',) int64, converged (U',) bool
            gibbs:  log_pred, log_pred_se, ess (U',); with connections also connection_counts (C, U', 3, 3) int64, the
                    counts of (f_c, mixture case) over chains and sweeps behind the connection posteriors
        Raises ValueError before run(), for another C, for gibbs with edge_index other than 'symmetric', beyond the
        count-histogram limits and where the tallies could overflow.
        """
        if self.method not in ("vb", "gibbs"):
            raise ValueError("method must be 'vb' or 'gibbs'")
        self._require_fitted("score()")
        bt_new = np.ascontiguousarray(bt_new, dtype=np.float64)
        if bt_new.ndim not in (2, 3) or (bt_new.ndim == 3 and bt_new.shape[2] < 1):
            raise ValueError("bt_new must be (C, U') or (C, U', K') with K' >= 1, got shape %s" % (bt_new.shape,))
        (C, U) = bt_new.shape[:2]
        C_fit = int(self._d["lq_F"].shape[0]) if self.method == "vb" else int(self.sampler.C)
        if C != C_fit:
            raise ValueError("bt_new has %d connections, the fit has %d" % (C, C_fit))
        N = int(util.C_to_N(C))
        if U < 1 or U > COUNT_MAX_U:
            raise ValueError("score() takes 1 to %d patients at a time (count-histogram limit), got %d" % (COUNT_MAX_U, U))
        if N > COUNT_MAX_NREG:
            raise ValueError("score() is made for at most %d regions (count-histogram limit), here %d" % (COUNT_MAX_NREG, N))
        if self.method == "gibbs":
            if self._edge_mode() != "symmetric":
                raise ValueError("score() with method 'gibbs' needs edge_index 'symmetric'")
            if int(n_anneal) < 1 or int(n_sweeps) < 1:
                raise ValueError("n_anneal and n_sweeps must be >= 1")
            if int(n_sweeps) * int(self.sampler.G) > PAIR_COUNT_MAX:
                raise ValueError("score() tallies would overflow uint32: %d chains x %d sweeps" % (self.sampler.G, n_sweeps))
        elif int(max_iters) < 1:
            raise ValueError("max_iters must be >= 1")
        if self._has_noise() and noise_var is None:
            raise ValueError("score(): the fit has noise variances, so the new patients' noise_var must be given (zeros are allowed)")
        noise = self._noise_host(bt_shape=bt_new.shape, bt_var=noise_var, name="noise_var")
        ctx = self._query_context()
        b_dev = self._data_dev("b")
        bt_dev = self._up(bt_new)
        if noise is not None:
            noise = tuple(None if a is None else self._up(a) for a in noise)
        if self.method == "vb":
            return _score.score_vb(ctx, b_dev, bt_dev, N, self._d["lq_F"], self.model, self._pi2(), self._edge_mode(),
                                   self.missing_data, connections, max_iters, float(tol), noise=noise)
        key = _score.score_key(self.seed if seed is None else seed)
        out = _score.score_gibbs(ctx, b_dev, bt_dev, N, self.sampler, self.model, self._pi2(), self.missing_data, connections,
                                 int(n_anneal), int(n_sweeps), key, noise=noise)
        return out

    # ------------------------------------------------------------------ patient or control
    def membership(self, x_new, *, n_anneal=200, seed=None):
        """
        Sets the model's two laws side by side for subjects who were not in the fit: is x_u a patient or a control?

        x_new (C, U') correlations in the fit's edge order (NaN = unobserved when missing_data: it adds 0 to both sides;
        without missing_data NaN propagates, as in score()).  theta is the model's CURRENT parameters (the plug-in convention
        of score()), and like score() the call works on a context of its own and leaves the fit (model, `sampler` and its
        state, energy) exactly as it was.  method='gibbs' only.

        With (f_g, r_g) the end state of the fit's sampler at chain g (the convention of score()):
            control   lc[g, u] = sum_c log N(x_cu; mu_k, sigma_k^2), k = f_gc
            patient   lp[g, u] = the annealed-importance-sampling log-weight over the new patient's own r_u, n_anneal rungs
                      from the prior (score.ais_schedule; seed and the sweep numbers as in score(): score.SCORE_SWEEP0), so
                      that E exp(lp[g, u]) = p(x_u | f_g, patient)
        and each side is pooled over all chains (of all ranks of a sharded fit) exactly as score() pools log_pred.
        Returns a dict of float64 (U',) arrays:
            log_patient, log_patient_se, ess_patient    log mean_g exp(lp[g, u]) = the estimate of log p(x_u | data, patient),
                                                        its delta-method standard error, (sum w)^2 / sum w^2 of the weights
            log_control, log_control_se, ess_control    the same of lc: log p(x_u | data, control)
            log_bf      log_patient - log_control: the log Bayes factor patient against control (add the log prior odds)
            log_bf_se   sqrt(log_patient_se^2 + log_control_se^2).  Both sides are averages over the SAME chains, so they are
                        correlated; the covariance between the two is ignored here.
        and n_chains, the number of chains pooled.  log_patient is score()'s log_pred of the same subjects.
        The cohort is walked in chunks (membership.CHUNK subjects): apart from a chunk's buffers, device memory does not grow
        with U'.  Raises ValueError before run(), for method='vb', for a wrong C, a non-2-D input and for edge_index other than
        'symmetric'; NotImplementedError for a fit with noise variances.
        """
        from . import membership as _membership
        self._refuse_membership_noise()
        (x_new, N) = self._membership_input(x_new)
        if int(n_anneal) < 1:
            raise ValueError("n_anneal must be >= 1")
        key = _score.score_key(self.seed if seed is None else seed)
        return _membership.membership(self._query_context(), self._up, x_new, N, self.sampler, self.model, self.missing_data,
                                      False, b_dev=self._data_dev("b"), pi2=self._pi2(), n_anneal=int(n_anneal), key=key)

    def _refuse_membership_noise(self):
        if self._has_noise():
            raise NotImplementedError("membership() is not provided with noise variances (b_noise_var / bt_noise_var): its "
                                      "kernels take one sigma per state")

    def _membership_input(self, x_new):
        """The checks of membership(), before anything touches the device: (x_new (C, U') float64, Nreg)."""
        if self.method == "vb":
            raise ValueError("membership() needs method='gibbs': the mean-field q of a 'vb' fit gives only bounds on the "
                             "patient side, and a difference of bounds is not a bound")
        if self.method != "gibbs":
            raise ValueError("method must be 'gibbs'")
        self._require_fitted("membership()")
        if self._edge_mode() != "symmetric":
            raise ValueError("membership() needs edge_index 'symmetric'")
        x_new = np.ascontiguousarray(x_new, dtype=np.float64)
        if x_new.ndim != 2:
            raise ValueError("x_new must be (C, U'), got shape %s" % (x_new.shape,))
        (C, U) = x_new.shape
        if C != int(self.sampler.C):
            raise ValueError("x_new has %d connections, the fit has %d" % (C, int(self.sampler.C)))
        if U < 1:
            raise ValueError("x_new holds no subject")
        return x_new, int(util.C_to_N(C))

    # ------------------------------------------------------------------ model evidence
    def log_evidence(self, n_anneal=1000, n_chains=None, seed=None):
        """
        An annealed-importance-sampling estimate of the model evidence at the fitted parameters,

            log Z = log sum_{f,r} p(f; gamma) p(r; pi) exp( sum_c S_B[c,f_c] + sum_{c,u} lM[c,u,f_c,l(r_nu,r_mu)] )
                  = log p(b, bt | theta, model),

        with theta = the model's CURRENT parameters (the plug-in convention of connection_posterior() and score()) and
        missing_data honoured through the tables.  The joint is that of the symmetric edge ids -- the only ids under which it
        is a joint -- also after a VB fit with edge_index='reference'.  SharedRegionFit inherits the method (its tables are
        (S_B, L) at U = 1), and both models have the same 12 parameters, so
            fit_shared.log_evidence()["log_evidence"] - fit_unshared.log_evidence()["log_evidence"]
        is a log Bayes factor at the fitted parameters.

        n_chains chains (None: the fit's `n_chains`) start from a draw of the prior and climb a ladder of n_anneal rungs
        (score.ais_schedule), one sweep of the fit's sampler per rung on tables scaled by the rung's beta; see
        fcdiff_amd/evidence.py.  seed: key of the annealing sampler's random numbers (None: derived from the fit's seed;
        never the fit's own numbers nor score()'s).  Under torch.distributed every rank anneals chains of its own -- the
        fit's global chain ids (`chain0`) for n_chains=None, else ids rank * n_chains onwards -- and the sums are pooled.
        Usable after run() with either method: it needs theta and the data, not the fit's posterior, and like score() it
        works on a context of its own and leaves the fit (model, _lq_R, _lq_F, energy, the device tables, `sampler`) as it
        was.

        Returns a dict:
            log_evidence     log mean_g exp(w_g) over all chains: unbiased for Z on the exp scale
            log_evidence_se  its delta-method standard error;  ess  (sum w)^2 / sum w^2 of the weights exp(w_g)
            lower, lower_se  mean_g w_g and its standard error: E[w] <= log Z (Jensen), a stochastic lower bound that stays
                             valid when the ESS collapses
            n_chains, n_anneal  chains pooled over ranks, rungs
        The variance of w grows with the number of sites over n_anneal.  On models of a few regions 50 rungs give an ESS of
        half the chains; at 200 regions and 100 patients (40 000 sites, 1024 chains) the weights are degenerate at every
        ladder measured -- ESS 1.0 / 2.8 / 3.6 and log_evidence - lower = 112 / 29 / 7 nats at 10^2 / 10^3 / 10^4 rungs
        (profiles/evidence_cost.json).  Where the ESS is near 1, log_evidence is the largest single weight and its
        standard error means nothing: quote `lower`, as a bound that tightens with the ladder.
        Raises ValueError before run() and for n_anneal < 1 or n_chains < 1.
        """
        from . import evidence as _evidence
        if self.method not in ("vb", "gibbs"):
            raise ValueError("method must be 'vb' or 'gibbs'")
        if int(n_anneal) != n_anneal or int(n_anneal) < 1 or int(n_anneal) > _evidence.MAX_ANNEAL:
            raise ValueError("n_anneal must be an integer from 1 to %d" % _evidence.MAX_ANNEAL)
        G = self.n_chains if n_chains is None else n_chains
        if int(G) != G or int(G) < 1:
            raise ValueError("n_chains must be an integer >= 1")
        self._require_fitted("log_evidence()")
        if self.b is None or self.bt is None:
            raise ValueError("log_evidence() needs b and bt: call run() first")
        chain0 = int(self.chain0)
        if n_chains is not None:
            import torch.distributed as dist
            chain0 = dist.get_rank() * int(G) if (dist.is_available() and dist.is_initialized()) else 0
        ctx = self._query_context()
        # fresh tables of the current theta on the query context: the fit's own are not touched
        (S_B, lM) = tables.build(ctx, self._data_dev("b"), self._data_dev("bt"), self.model.theta(), self._flags(),
                                 shared=self._shared, **self._noise_kw(), **self._groups_kw())
        (C, U) = (int(lM.shape[0]), int(lM.shape[1]))
        key = _evidence.evidence_key(self.seed if seed is None else seed)
        return _evidence.log_evidence(ctx, S_B, lM, int(util.C_to_N(C)), U, self.model.gamma, self._pi2(), int(n_anneal), int(G),
                                      chain0, key)

    def _bt_dev(self, C, U):
        bt = self._data_dev("bt")
        if bt.dim() not in (2, 3) or tuple(bt.shape[:2]) != (C, U):
            raise ValueError("bt has shape %s, the fit's state needs %s" % (tuple(bt.shape), (C, U)))
        return bt


class SharedRegionFit(UnsharedRegionFit):
    """
    Fits the shared-region model (fcdiff_amd.SharedRegionModel: one set of anomalous regions r_n for every patient) to
    correlations.  Same attributes and knobs as UnsharedRegionFit; edge ids are always 'symmetric'.

    With T and F~ integrated out per patient, the collapsed joint is
        ln p(b, bt, f, r) = sum_n ln pi_{r_n} + sum_c [ ln gamma_{f_c} + S_B[c, f_c] + L[c, f_c, l(r_n, r_m)] ],
        L[c, k, l] = sum_u lM[c, u, k, l],
    the collapsed joint of the UNSHARED model with one patient whose table is L.  So run() builds S_B and L in one launch
    (fcd_lik_shared_tables, nothing of size C*U) and then runs the unshared fit's own VB loop or sampler at U = 1 on L:
    `_lq_R` is (N, 1, 2) (the population column), `_lq_F` (C, 1, 3), `_lM` holds L as (C, 1, 3, 3).  `energy` is minus
    the ELBO of p(b, bt) under this model, on the unshared fit's scale.  The theta_sub step weights every patient's item
    with its edge's (C, 1, 3, 3) weights (FCD_W_PER_EDGE).
    """

    _shared = True

    def __init__(self):
        super(SharedRegionFit, self).__init__()
        self.edge_index = "symmetric"

    def _edge_mode(self):
        if self.edge_index not in (None, "symmetric"):
            if self.edge_index == "reference":
                raise ValueError("edge_index 'reference' (quirk Q1) exists only for parity with the reference's unshared "
                                 "fit; SharedRegionFit uses 'symmetric'")
            raise ValueError("edge_index must be 'symmetric' for SharedRegionFit")
        return "symmetric"

    def run(self):
        """Builds S_B and L, then the VB loop or the sampler at U = 1 (see the class docstring)."""
        self._edge_mode()
        if self.patient_groups is not None:
            self._refuse_patient_groups_shared()
        if self.patient_traits is not None:
            self._refuse_patient_traits_shared()
        super(SharedRegionFit, self).run()

    def _theta_sub_flags(self):
        return {"missing_data": self.missing_data, "per_edge": True}

    def _patient_extent(self, U):
        return 1

    def _patients(self):
        bt = self._d.get("bt")
        return int(bt.shape[1]) if bt is not None else int(np.asarray(self.bt).shape[1])

    # ------------------------------------------------------------------ posteriors
    def region_posterior(self):
        """(N,) P(r_n = 1 | data) from the last run(): q(r_n = 1) (vb) or the chains' frequency (gibbs)."""
        lq_R = self._lq_R
        if lq_R is None or lq_R.ndim != 3 or lq_R.shape[1] != 1:
            raise ValueError("region_posterior() needs a run(): _lq_R must be (N, 1, 2)")
        return np.exp(lq_R[:, 0, 1])

    def connection_posterior(self):
        """
        Per connection and patient, as UnsharedRegionFit.connection_posterior(): p_T (C, U), p_F_tilde (C, U, 3),
        p_changed (C, U).  Given (f_c, the mixture case of the shared r) each patient's T and F~ have the closed-form law of
        the unshared model, so the fit's weights are broadcast to every patient:
          method='vb'     q_R (N, 1, 2) broadcast to (N, U, 2): exact under the mean field;
          method='gibbs'  the (C, 1, 3, 3) counts of (f_c, mixture case) broadcast to (C, U, 3, 3) (needs
                          connection_marginals = True before run()).
        """
        if self.model is None or self.bt is None:
            raise ValueError("connection_posterior() needs a model and bt: call run() first")
        U = self._patients()
        if self.method == "gibbs":
            (counts, N, C) = self._connection_counts_dev()
            counts = counts.expand(C, U, 3, 3).contiguous()
            return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), counts=counts,
                                  missing_data=self.missing_data, **self._noise_bt_kw())
        if self.method != "vb":
            raise ValueError("method must be 'vb' or 'gibbs'")
        (N, C, _one) = self._check_state(need=("lq_R", "lq_F"))
        lq_R = self._d["lq_R"].expand(N, U, 2).contiguous()
        return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), lq_F=self._d["lq_F"],
                              lq_R=lq_R, missing_data=self.missing_data, **self._noise_bt_kw())

    def anomaly_count_posterior(self):
        """
        The law of the number of anomalous regions sum_n r_n, from the last run():
            p_count (N+1,)  P(sum_n r_n = k | data);   p_any  P(some region is anomalous) = 1 - p_count[0]
          method='vb'     Poisson-binomial law of q(r_n) (fcd_vb_count_posterior at U = 1);
          method='gibbs'  the histogram over chains and sweeps (needs anomaly_counts = True before run()).
        """
        if self.model is None or self.bt is None:
            raise ValueError("anomaly_count_posterior() needs a model and bt: call run() first")
        if self.method == "gibbs":
            hp = self.patient_count_hist
            if hp is None:
                raise ValueError("no anomaly-count histograms: set anomaly_counts = True before run(method='gibbs')")
            hp = np.asarray(hp, dtype=np.float64)[0]
            if hp.sum() == 0:
                raise ValueError("no sweep was accumulated into the anomaly-count histograms (n_sweeps <= burn_in?)")
            p = hp / hp.sum()
        elif self.method == "vb":
            (N, _C, _one) = self._check_state(need=("lq_R",))
            p = count_posterior(self._context(), self._d["lq_R"], N, 1)[0][0]
        else:
            raise ValueError("method must be 'vb' or 'gibbs'")
        return {"p_count": p, "p_any": float(1.0 - p[0])}

    def coanomaly_posterior(self):
        """
        Which regions are anomalous together, from the last run():
            p_region_pair (N, N)              P(r_n = 1, r_m = 1 | data); the diagonal is region_posterior()
            p_region_pair_independent (N, N)  P(r_n = 1 | data) P(r_m = 1 | data) off the diagonal
          method='vb'     the mean-field law: the two are equal (fcd_vb_coanomaly at U = 1);
          method='gibbs'  the pair counts over chains and sweeps (needs coanomaly = True before run()).
        There is no patient matrix: the state has one column.
        """
        out = super(SharedRegionFit, self).coanomaly_posterior()
        return {"p_region_pair": out["p_region_pair"], "p_region_pair_independent": out["p_region_pair_independent"]}

    def score(self, *args, **kwargs):
        """Scoring a new patient under a population-level r is a different question; not provided."""
        raise NotImplementedError("score() is not provided for the shared-region model")

    def membership(self, x_new, *, n_anneal=200, seed=None):
        """
        UnsharedRegionFit.membership() for the shared-region model: same input, same dict, same refusals.  A new patient
        inherits the population's r, so the patient side needs no annealing (n_anneal and seed are ignored):
            patient   lp[g, u] = sum_c log M(x_cu | f_gc, l(r_gn, r_gm)), the log of the mixture lM tabulates, at the
                      population's r of chain g
        pooled over the chains like the control side.  log_patient is the held-out predictive likelihood
        log p(x_u | data, patient) of this model, the number to set against the unshared fit's score()["log_pred"].
        One kernel (fcd_member_loglik) gives both sides straight from x_new: no (C, U', 3, 3) table is made.
        """
        from . import membership as _membership
        self._refuse_membership_noise()
        (x_new, N) = self._membership_input(x_new)
        return _membership.membership(self._query_context(), self._up, x_new, N, self.sampler, self.model,
                                      self.missing_data, True)


GROUP_CONTRAST_MAX = 64          # gibbs.PATIENT_GROUP_MAX_CONTRASTS: the contrasts ride on the patient-group accumulator


class GroupedRegionFit(UnsharedRegionFit):
    """
    Fits the grouped-region model (fcdiff_amd.GroupedRegionModel: one set of anomalous regions r_ng per KNOWN group of
    patients) to correlations.  Same attributes and knobs as UnsharedRegionFit, and
        group_labels     (U,) ints or strings: the group of every patient (diagnosis subtype, arm, site, ...; group_labels_csr)
        group_contrasts  pairs (name_a, name_b) of two labels, for group_contrast_posterior()
    Edge ids are always 'symmetric'.

    With T and F~ integrated out per patient, the collapsed joint is that of the UNSHARED model at G pseudo-patients whose
    tables are the sums over the groups' members,
        L[c, g, k, l] = sum_{u in group g} lM[c, u, k, l].
    So run() builds S_B and L in one launch (fcd_lik_grouped_tables, nothing of size C*U) and then runs the unshared fit's
    own VB loop or sampler at patient extent G: `_lq_R` is (N, G, 2), `_lq_F` (C, 1, 3), `_lM` holds L as (C, G, 3, 3), the
    columns in the order of `group_names` (the sorted labels).  `energy` is minus the ELBO of p(b, bt) under this model, on
    the unshared fit's scale.  missing_data, sessions bt (C, U, K), b_noise_var / bt_noise_var and missing_counts() work as
    in the other fits.  One label for everyone is SharedRegionFit, a label per patient UnsharedRegionFit with 'symmetric'
    ids; the three have the same parameters, so their log_evidence() differ by log Bayes factors: "do these subgroups have
    different anomaly maps?" is a number.

    Inherited with the GROUPS as their "patients": anomaly_count_posterior() (p_patient_count (G, Nreg+1), p_region_count
    (Nreg, G+1): in how many groups a region is anomalous), coanomaly_posterior() (the patient matrix is (G, G): how many
    anomalous regions two groups share), region_set_posterior() (per set and group) and log_evidence().
    connection_posterior() is per connection and PATIENT.  The theta_sub step expands the group weights to the patients
    (W[:, group_of_u]) and calls the unshared objectives unchanged; it stays refused with sessions or noise variances.
    Not provided: score() and membership() (NotImplementedError: which group's map a new patient gets is a separate
    question, answered by SubtypeRegionFit.assign()), user-set patient_groups / patient_traits (ValueError: their "patients"
    would be the groups; use group_contrasts).
    """

    def __init__(self):
        super(GroupedRegionFit, self).__init__()
        self.edge_index = "symmetric"
        self.group_labels = None
        self.group_contrasts = None
        self.group_names = None             # the sorted labels behind the state's columns, set by run()
        self.group_contrast_names = None    # the contrasts of the last run() as pairs of labels

    def _edge_mode(self):
        if self.edge_index not in (None, "symmetric"):
            if self.edge_index == "reference":
                raise ValueError("edge_index 'reference' (quirk Q1) exists only for parity with the reference's unshared "
                                 "fit; GroupedRegionFit uses 'symmetric'")
            raise ValueError("edge_index must be 'symmetric' for GroupedRegionFit")
        return "symmetric"

    # ------------------------------------------------------------------ the groups
    def _patients(self):
        return int(np.shape(self.bt)[1])

    def _groups_host(self, U=None):
        """(names, offsets (G+1,) int64, order (U,) int32, group_of (U,) int64) of group_labels: host only, ValueError as
        group_labels_csr()."""
        if self.group_labels is None:
            raise ValueError("GroupedRegionFit needs group_labels: one label per patient")
        (names, offsets, order) = group_labels_csr(self.group_labels, self._patients() if U is None else U)
        return names, offsets, order, group_of_patient(offsets, order)

    def _patient_extent(self, U):
        return len(self._groups_host(U)[0])

    def _groups_dev(self):
        """The device copies of the CSR arrays and of group_of, made again whenever the labels change."""
        (names, offsets, order, group_of) = self._groups_host()
        key = (offsets.tobytes(), order.tobytes())
        cur = self._d.get("groups")
        if cur is None or cur[0] != key:
            t = self._torch()
            dev = self._dev()
            cur = (key, t.as_tensor(order, device=dev), t.as_tensor(offsets, device=dev), t.as_tensor(group_of, device=dev),
                   len(names))
            self._d["groups"] = cur
        return cur[1:]

    def _groups_kw(self):
        (order, offsets, _group_of, G) = self._groups_dev()
        return {"groups": (order, offsets, G)}

    def _expand_weights(self, W):
        return W.index_select(1, self._groups_dev()[2]).contiguous()

    def _contrast_columns(self, names):
        """group_contrasts as pairs of columns of the state: ValueError for an unknown label, a contrast of a group with
        itself, a contrast given twice, more than 64."""
        rows = [] if self.group_contrasts is None else list(self.group_contrasts)
        if len(rows) > GROUP_CONTRAST_MAX:
            raise ValueError("group_contrasts holds %d contrasts (at most %d)" % (len(rows), GROUP_CONTRAST_MAX))
        pairs = []
        for row in rows:
            row = tuple(row)
            if len(row) != 2:
                raise ValueError("a group contrast is a pair of labels, got %r" % (row,))
            for name in row:
                if name not in names:
                    raise ValueError("a group contrast names the unknown group %r" % (name,))
            pair = (names.index(row[0]), names.index(row[1]))
            if pair[0] == pair[1]:
                raise ValueError("a group contrast names the group %r twice" % (row[0],))
            if pair in pairs:
                raise ValueError("the group contrast %r is given twice" % (row,))
            pairs.append(pair)
        return pairs

    def _refuse_patient_knobs(self):
        if self.patient_groups is not None or self.patient_group_contrasts is not None:
            raise ValueError("GroupedRegionFit takes no patient_groups: the state's columns are the groups of group_labels; "
                             "set group_contrasts and read group_contrast_posterior()")
        if self.patient_traits is not None:
            raise ValueError("GroupedRegionFit takes no patient_traits: the state's columns are groups of patients, not patients")

    def run(self):
        """Builds S_B and L (C, G, 3, 3), then the VB loop or the sampler at patient extent G (see the class docstring)."""
        self._edge_mode()
        self._refuse_patient_knobs()
        if self.bt is None or np.ndim(self.bt) not in (2, 3):
            raise ValueError("bt must be (C, U) or (C, U, K), got shape %s" % (np.shape(self.bt),))
        names = self._groups_host()[0]
        pairs = self._contrast_columns(names)
        super(GroupedRegionFit, self).run()
        self.group_names = list(names)
        self.group_contrast_names = [(names[a], names[b]) for (a, b) in pairs]

    def _run_gibbs(self, N, G):
        """The sampler at G columns; the contrasts ride on the patient-group accumulator as contrasts of singleton groups."""
        names = self._groups_host()[0]
        pairs = self._contrast_columns(names)
        if pairs:
            cols = sorted(set(c for pair in pairs for c in pair))
            self.patient_groups = [[c] for c in cols]
            self.patient_group_contrasts = [(cols.index(a), cols.index(b)) for (a, b) in pairs]
        try:
            super(GroupedRegionFit, self)._run_gibbs(N, G)
        finally:
            (self.patient_groups, self.patient_group_contrasts) = (None, None)

    # ------------------------------------------------------------------ posteriors
    def region_posterior(self):
        """
        {"p_region" (N, G): P(r_ng = 1 | data), "group_names": the G labels of its columns} from the last run(): q(r_ng = 1)
        (vb) or the chains' frequency (gibbs).
        """
        lq_R = self._lq_R
        if lq_R is None or lq_R.ndim != 3 or self.group_names is None or lq_R.shape[1] != len(self.group_names):
            raise ValueError("region_posterior() needs a run(): _lq_R must be (N, G, 2)")
        return {"p_region": np.exp(lq_R[:, :, 1]), "group_names": list(self.group_names)}

    def connection_posterior(self):
        """
        Per connection and PATIENT, as UnsharedRegionFit.connection_posterior(): p_T (C, U), p_F_tilde (C, U, 3), p_changed
        (C, U).  Given (f_c, the mixture case of its group's r) each patient's T and F~ have the closed-form law of the
        unshared model, so the group's weights are gathered to its patients:
          method='vb'     q_R (N, G, 2) gathered to (N, U, 2) with the patients' groups: exact under the mean field;
          method='gibbs'  the (C, G, 3, 3) counts of (f_c, mixture case) gathered to (C, U, 3, 3) (needs
                          connection_marginals = True before run()).
        """
        if self.model is None or self.bt is None:
            raise ValueError("connection_posterior() needs a model and bt: call run() first")
        U = self._patients()
        group_of = self._groups_dev()[2]
        if self.method == "gibbs":
            (counts, N, C) = self._connection_counts_dev()
            counts = counts.index_select(1, group_of).contiguous()
            return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), counts=counts,
                                  missing_data=self.missing_data, **self._noise_bt_kw())
        if self.method != "vb":
            raise ValueError("method must be 'vb' or 'gibbs'")
        (N, C, _G) = self._check_state(need=("lq_R", "lq_F"))
        lq_R = self._d["lq_R"].index_select(1, group_of).contiguous()
        return conn_posterior(self._context(), self._bt_dev(C, U), N, U, self.model.theta(), lq_F=self._d["lq_F"],
                              lq_R=lq_R, missing_data=self.missing_data, **self._noise_bt_kw())

    def group_contrast_posterior(self, independent=False):
        """
        Do two groups differ at a row?  For every contrast (a, b) of `group_contrasts` and every row -- the Nreg regions and,
        with `region_sets`, the sets after them, whose indicator is "the group has an anomalous region in S" --, the joint law
        of the two groups' indicators, from the last run(), as a dict (P contrasts, R rows):
            contrasts, row_names             the contrasts as pairs of labels; "0" .. "Nreg-1", "set:<name>"
            p_both, p_only_a, p_only_b, p_neither  (P, R)     P(a and b anomalous at the row | data), a alone, b alone, neither
            p_a, p_b  (P, R)                 the two marginals, p_both + p_only_a and p_both + p_only_b
        The groups are coupled through f, so the joint is not the product of the marginals:
          method='gibbs', independent=False   read off the (R, 2, 2) joint histograms of the contrasts, counted by the
                          patient-group accumulator over chains and the sweeps from burn_in on, every
                          `patient_groups_every`-th.  Needs `group_contrasts` set before run(); ValueError otherwise.
          method='vb', or independent=True on either method   the mean-field product of the marginals of _lq_R with the
                          CURRENT group_contrasts and region sets (at a set row p = 1 - prod_{n in S} (1 - q1(n, g))).
        """
        if self.model is None or self.bt is None or self.group_names is None:
            raise ValueError("group_contrast_posterior() needs a fitted model: call run() first")
        if self.method not in ("vb", "gibbs"):
            raise ValueError("method must be 'vb' or 'gibbs'")
        names = list(self.group_names)
        if self.method == "gibbs" and not independent:
            hj = self.patient_group_joint_hist
            if not self.group_contrast_names or hj is None:
                raise ValueError("no group-contrast histograms: set group_contrasts before run(method='gibbs')")
            joint = np.stack([np.asarray(h, dtype=np.float64) for h in hj], axis=0)          # (P, R, 2, 2)
            if joint.sum() == 0:
                raise ValueError("no sweep was accumulated into the group-contrast histograms (n_sweeps <= burn_in?)")
            joint = joint / joint.sum(axis=(2, 3), keepdims=True)
            (contrasts, row_names) = (list(self.group_contrast_names), list(self.patient_group_rows))
        else:
            pairs = self._contrast_columns(names)
            if not pairs:
                raise ValueError("no group contrasts: set group_contrasts first")
            lq_R = self._lq_R
            if lq_R is None or lq_R.ndim != 3 or lq_R.shape[1] != len(names):
                raise ValueError("group_contrast_posterior() needs a run(): _lq_R must be (N, G, 2)")
            N = lq_R.shape[0]
            q1 = 1.0 / (1.0 + np.exp(lq_R[:, :, 0] - lq_R[:, :, 1]))                            # (N, G), normalised
            rows = [q1]
            row_names = [str(n) for n in range(N)]
            if self.region_sets is not None:
                (set_names, offsets, members) = region_sets_csr(self.region_sets, N)
                rows.append(np.stack([1.0 - np.prod(1.0 - q1[members[offsets[j]:offsets[j + 1]]], axis=0)
                                      for j in range(len(set_names))], axis=0))
                row_names += ["set:" + name for name in set_names]
            p = np.concatenate(rows, axis=0)                                                    # (R, G)
            joint = np.stack([np.stack([np.stack([(1 - p[:, a]) * (1 - p[:, b]), (1 - p[:, a]) * p[:, b]], axis=1),
                                        np.stack([p[:, a] * (1 - p[:, b]), p[:, a] * p[:, b]], axis=1)], axis=1)
                              for (a, b) in pairs], axis=0)
            contrasts = [(names[a], names[b]) for (a, b) in pairs]
        return {"contrasts": contrasts, "row_names": row_names, "p_both": joint[:, :, 1, 1], "p_only_a": joint[:, :, 1, 0],
                "p_only_b": joint[:, :, 0, 1], "p_neither": joint[:, :, 0, 0], "p_a": joint[:, :, 1, :].sum(axis=2),
                "p_b": joint[:, :, :, 1].sum(axis=2)}

    def patient_group_posterior(self, *args, **kwargs):
        """Not provided: the state's columns are the groups of group_labels; see group_contrast_posterior()."""
        raise ValueError("GroupedRegionFit has no patient_group_posterior(): the state's columns are the groups of "
                         "group_labels; set group_contrasts and read group_contrast_posterior()")

    def patient_trait_posterior(self, *args, **kwargs):
        """Not provided: the state's columns are groups of patients, not patients."""
        raise ValueError("GroupedRegionFit has no patient_trait_posterior(): the state's columns are groups of patients")

    def score(self, *args, **kwargs):
        """Not provided: which group's map a new patient gets is a separate question."""
        raise NotImplementedError("score() is not provided for the grouped-region model: which group's map a new patient "
                                  "gets is a separate question")

    def membership(self, *args, **kwargs):
        """Not provided: which group's map a new patient gets is a separate question."""
        raise NotImplementedError("membership() is not provided for the grouped-region model: which group's map a new "
                                  "patient gets is a separate question")


SUBTYPE_MAX = tables.SUBTYPE_MAX


def _digamma(x):
    import scipy.special
    return scipy.special.digamma(x)


def _gammaln(x):
    import scipy.special
    return scipy.special.gammaln(x)


def subtype_E_ln_rho(n, alpha):
    """E ln rho_g = psi(alpha + n_g) - psi(G alpha + sum n) under q(rho) = Dirichlet(alpha + n), (G,) float64."""
    n = np.asarray(n, dtype=np.float64)
    return _digamma(alpha + n) - _digamma(len(n) * alpha + n.sum())


def subtype_softmax(logits):
    """Row-wise softmax of (U, G) log-weights, by the row maximum."""
    a = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(axis=1, keepdims=True)


def subtype_energy_terms(resp, alpha):
    """
    What the z and rho factors add to the free energy at responsibilities resp (U, G) with q(rho) = Dirichlet(alpha + n),
    n = sum_u resp:  - sum_{u,g} s (E ln rho_g - ln s)  +  KL(Dir(alpha + n) || Dir(alpha)),  taking 0 ln 0 = 0.
    """
    s = np.asarray(resp, dtype=np.float64)
    (U, G) = s.shape
    n = s.sum(axis=0)
    el = subtype_E_ln_rho(n, alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(s > 0, s * np.log(s), 0.0)
    cross = float((s * el[None, :]).sum() - ent.sum())
    kl = float(_gammaln(G * alpha + n.sum()) - _gammaln(alpha + n).sum() - _gammaln(G * alpha) + G * _gammaln(alpha)
               + (n * el).sum())
    return -cross + kl


class SubtypeRegionFit(UnsharedRegionFit):
    """
    Fits the subtype-region model (fcdiff_amd.SubtypeRegionModel: GroupedRegionModel with the group of every patient
    unknown) by mean-field VB: z_u ~ Categorical(rho), rho ~ Dirichlet(alpha, ..., alpha) integrated out, one anomaly map
    r_ng per subtype.  UnsharedRegionFit's attributes, and
        n_subtypes              G, 1 .. min(8, U)
        rho_concentration       alpha of the Dirichlet prior (1.0)
        n_restarts              restarts from seeded initial responsibilities (4); the one with the lowest final energy is kept
        seed                    restart i starts from z0 = default_rng(seed + i).permutation(U) % G, s = 0.1/G + 0.9 onehot(z0)
        init_responsibilities   None, or (U, G) rows of probabilities: ONE run from them, no restarts
    Edge ids are always 'symmetric', method is always 'vb'.

    The family is q(f) q(r) q(z) q(rho) with responsibilities s[u, g] = q(z_u = g) and q(rho) = Dirichlet(alpha + n),
    n_g = sum_u s[u, g].  The expected collapsed log-likelihood is the unshared model's E_lM term at G pseudo-patients with
        L[c, g, k, l] = sum_u s[u, g] lM[c, u, k, l]
    (GroupedRegionFit is the one-hot case), so q_F, q_R, the pi and gamma steps and the energy are the unshared fit's own
    kernels at patient extent G on L.  One outer iteration: q_F, q_R (on L), pi and gamma, then
        E[u, g] = sum_c sum_k q_F[c,k] sum_l w_l^g(c) lM[c, u, k, l]          (fcd_vb_subtype_loglik)
        s[u, :] = softmax_g(E[u, g] + psi(alpha + n_g) - psi(G alpha + U))    (n of the s before the step)
        L = sum_u s lM                                                        (fcd_lik_weighted_tables)
    and `energy` = the inherited energy at L(s) - sum s (E ln rho - ln s) + KL(Dir(alpha + n) || Dir(alpha)): minus a lower
    bound on log p(b, bt | theta).  Every step is an exact coordinate maximiser, so the energy never rises.
    run() keeps the per-patient table (C, U, 3, 3) -- `_lM_patients`, built ONCE: theta_sub is not fitted, so it does not
    change -- beside L (`_lM`, (C, G, 3, 3)); `_lq_R` is (N, G, 2).  missing_data, sessions bt (C, U, K), b_noise_var /
    bt_noise_var and missing_counts() work through that table build as in the other fits.  After the fit the subtypes are
    renumbered by decreasing n_g (ties by index), so the result does not depend on the label permutation of the start.
    run() leaves `energy` (the kept restart's, the start and every outer iteration), `restart_energies` (every restart's
    last) and `responsibilities` (U, G).

    Queries: subtype_posterior(), region_posterior(), connection_posterior() (per connection and PATIENT), assign(bt_new)
    (which subtype's map a new patient gets), and, with the SUBTYPES as their "patients" as in GroupedRegionFit,
    anomaly_count_posterior(), coanomaly_posterior(), region_set_posterior().
    Not provided: method='gibbs' and update_theta_sub (NotImplementedError from run()), score(), membership() and
    log_evidence() (NotImplementedError: the inherited forms would read L as a data table), patient_groups /
    patient_traits (ValueError).
    """

    def __init__(self):
        super(SubtypeRegionFit, self).__init__()
        self.edge_index = "symmetric"
        self.n_subtypes = None
        self.rho_concentration = 1.0
        self.n_restarts = 4
        self.init_responsibilities = None
        self.responsibilities = None        # (U, G) float64 of the last run(), columns by decreasing n_g
        self.restart_energies = None        # the last energy of every restart of the last run()

    def _edge_mode(self):
        if self.edge_index not in (None, "symmetric"):
            if self.edge_index == "reference":
                raise ValueError("edge_index 'reference' (quirk Q1) exists only for parity with the reference's unshared "
                                 "fit; SubtypeRegionFit uses 'symmetric'")
            raise ValueError("edge_index must be 'symmetric' for SubtypeRegionFit")
        return "symmetric"

    # ------------------------------------------------------------------ shapes and refusals
    def _patients(self):
        return int(np.shape(self.bt)[1])

    def _n_subtypes(self, U=None):
        U = self._patients() if U is None else int(U)
        G = self.n_subtypes
        if G is None or isinstance(G, bool) or int(G) != G or not 1 <= int(G) <= min(SUBTYPE_MAX, U):
            raise ValueError("n_subtypes must be an integer in 1 .. min(%d, U = %d), got %r" % (SUBTYPE_MAX, U, G))
        return int(G)

    def _patient_extent(self, U):
        return self._n_subtypes(U)

    def _built_table(self, U):
        return "lM_u", int(U)

    def _alpha(self):
        a = float(self.rho_concentration)
        if not (a > 0 and np.isfinite(a)):
            raise ValueError("rho_concentration must be a finite number > 0, got %r" % (self.rho_concentration,))
        return a

    def _refuse_knobs(self):
        if self.method == "gibbs":
            raise NotImplementedError("SubtypeRegionFit has no sampler (method='gibbs'): the subtypes are fitted by VB only, a "
                                      "sampler for z is not made")
        if self.method != "vb":
            raise ValueError("method must be 'vb' for SubtypeRegionFit")
        if self.update_theta_sub or self.theta_sub_every:
            raise NotImplementedError("the theta_sub step is not provided with subtypes: the fit keeps one per-patient table for "
                                      "all iterations, which a change of (eta, epsilon) would invalidate")
        if self.patient_groups is not None or self.patient_group_contrasts is not None:
            raise ValueError("SubtypeRegionFit takes no patient_groups: the state's columns are the subtypes, not patients")
        if self.patient_traits is not None:
            raise ValueError("SubtypeRegionFit takes no patient_traits: the state's columns are the subtypes, not patients")

    @staticmethod
    def _checked_responsibilities(resp, U, G, name):
        s = np.array(resp, dtype=np.float64)
        if s.shape != (U, G):
            raise ValueError("%s must have shape (U, G) = %s, got %s" % (name, (U, G), s.shape))
        if not np.all(np.isfinite(s)) or np.any(s < 0):
            raise ValueError("%s must be finite and >= 0" % name)
        if np.any(np.abs(s.sum(axis=1) - 1.0) > 1e-9):
            raise ValueError("every row of %s must sum to 1" % name)
        return np.ascontiguousarray(s)

    def _starts(self, U, G):
        """The initial responsibilities of the run(s): the user's alone, or those of the seeded restarts."""
        if self.init_responsibilities is not None:
            return [self._checked_responsibilities(self.init_responsibilities, U, G, "init_responsibilities")]
        R = self.n_restarts
        if isinstance(R, bool) or int(R) != R or int(R) < 1:
            raise ValueError("n_restarts must be an integer >= 1, got %r" % (R,))
        out = []
        for i in range(int(R)):
            z0 = np.random.default_rng(int(self.seed) + i).permutation(U) % G
            s = np.full((U, G), 0.1 / G)
            s[np.arange(U), z0] += 0.9
            out.append(s)
        return out

    # ------------------------------------------------------------------ state
    @property
    def _lM_patients(self):
        """(C, U, 3, 3): the per-patient table the responsibilities weight (`_lM` is L (C, G, 3, 3))."""
        return self._get("lM_u")

    def _resp_dev(self):
        """The device copy of `responsibilities`, made again whenever the host values change."""
        s = self.responsibilities
        if s is None:
            raise ValueError("no responsibilities: call run() first")
        (N, C, G) = self._check_state(need=("lq_R",))
        s = self._checked_responsibilities(s, self._patients(), G, "responsibilities")
        key = s.tobytes()
        cur = self._d.get("resp")
        if cur is None or cur[0] != key:
            cur = (key, self._up(s))
            self._d["resp"] = cur
        return cur[1]

    def _update_lps(self):
        """The per-patient table from the current parameters and, once there are responsibilities, L from it."""
        self._tables(full=False)
        if self.responsibilities is not None:
            self._update_weighted_table()

    def _update_weighted_table(self):
        """L = sum_u s[u, g] lM[c, u] into the state's `_lM`, in place: fcd_lik_weighted_tables through tables.build."""
        resp = self._resp_dev()
        (_S_B, self._d["lM"]) = tables.build(self._context(), self._d["b"], self._d["bt"], self.model.theta(), self._flags(),
                                             S_B=self._d["S_B"], lM=self._d["lM"], weights=(self._d["lM_u"], resp))

    def _expected_loglik(self, ctx, lM_u):
        """E (U', G) of the patients of the table lM_u (C, U', 3, 3) at the fit's q_F and q_R: fcd_vb_subtype_loglik."""
        t = self._torch()
        (N, C, G) = self._check_state(need=("lq_R", "lq_F"))
        if lM_u.dim() != 4 or tuple(lM_u.shape[2:]) != (3, 3) or int(lM_u.shape[0]) != C:
            raise ValueError("the per-patient table must be (C, U, 3, 3) with C = %d, got %s" % (C, tuple(lM_u.shape)))
        U = int(lM_u.shape[1])
        E = t.empty((U, G), dtype=t.float64, device=self._dev())
        ctx.call("fcd_vb_subtype_loglik", _lib.dptr(self._d["lq_F"]), _lib.dptr(self._d["lq_R"]), _lib.dptr(lM_u.contiguous()),
                 N, U, G, _lib.dptr(E), _lib.stream_ptr())
        return E.cpu().numpy()

    def _update_responsibilities(self):
        """s[u, :] = softmax_g(E[u, g] + E ln rho_g) with q(rho) of the responsibilities before the step."""
        E = self._expected_loglik(self._context(), self._d["lM_u"])
        el = subtype_E_ln_rho(self.responsibilities.sum(axis=0), self._alpha())
        self.responsibilities = subtype_softmax(E + el[None, :])

    def _eval_energy(self):
        """The inherited free energy at L(s) plus the terms of z and rho (subtype_energy_terms)."""
        return super(SubtypeRegionFit, self)._eval_energy() + subtype_energy_terms(self.responsibilities, self._alpha())

    # ------------------------------------------------------------------ the fit
    def run(self):
        """The restarts of the VB loop of the class docstring; keeps the one with the lowest final energy."""
        self._edge_mode()
        self._refuse_knobs()
        if self.model is None:
            raise ValueError("Model has not been initialized.")
        if self.bt is None or np.ndim(self.bt) not in (2, 3) or (np.ndim(self.bt) == 3 and np.shape(self.bt)[2] < 1):
            raise ValueError("bt must be (C, U) or (C, U, K) with K >= 1 sessions, got shape %s" % (np.shape(self.bt),))
        (C, H) = np.shape(self.b)
        U = self._patients()
        N = util.C_to_N(C)
        if (N % 1) != 0:
            raise ValueError("Number of connections (%u) must be a triangular number." % C)
        N = int(N)
        G = self._n_subtypes(U)
        self._alpha()
        starts = self._starts(U, G)
        self._noise_host()               # (a ValueError for bad noise variances before any context exists)
        (pi0, gamma0) = (self.model.pi, np.array(self.model.gamma, dtype=np.float64))
        self.responsibilities = None
        # _init_lps is called for what outlives the restarts: it forgets the device copies of b / bt (a run starts from the
        # arrays as they are now) and allocates S_B and the (C, G, 3, 3) buffer L is written into.  Its uniform lq_R / lq_F
        # are replaced at the start of every restart (_run_from).
        self._init_lps(N, H, U)
        self._tables(full=False)         # S_B and the per-patient table, once for every restart and iteration
        best = None
        self.restart_energies = []
        for s0 in starts:
            (self.model.pi, self.model.gamma) = (pi0, gamma0.copy())
            energy = self._run_from(s0, N, C, G)
            self.restart_energies.append(energy[-1])
            if best is None or energy[-1] < best["energy"][-1]:
                best = dict(energy=energy, resp=self.responsibilities, lq_R=self._d["lq_R"], lq_F=self._d["lq_F"],
                            pi=self.model.pi, gamma=self.model.gamma)
        # the kept restart, its subtypes by decreasing n_g (ties by index), and L at those responsibilities
        order = np.argsort(-best["resp"].sum(axis=0), kind="stable")
        self.energy = best["energy"]
        (self.model.pi, self.model.gamma) = (best["pi"], best["gamma"])
        self.responsibilities = np.ascontiguousarray(best["resp"][:, order])
        self._d["lq_F"] = best["lq_F"]
        self._d["lq_R"] = best["lq_R"].index_select(1, self._torch().as_tensor(order, device=self._dev())).contiguous()
        self._update_weighted_table()

    def _run_from(self, s0, N, C, G):
        """One VB run from responsibilities s0 on the tables already built; returns its energies."""
        t = self._torch()
        dev = self._dev()
        self._d["lq_R"] = t.full((N, G, 2), -np.log(2), dtype=t.float64, device=dev)
        self._d["lq_F"] = t.full((C, 1, 3), -np.log(3), dtype=t.float64, device=dev)
        self.responsibilities = s0
        self._update_weighted_table()
        self.energy = [self._eval_energy()]
        for i in range(1, self.max_iters + 1):
            self._update_lq_F()
            self._update_lq_R()
            self._update_theta()
            self._update_responsibilities()
            self._update_weighted_table()
            self.energy.append(self._eval_energy())
            if self._is_converged(i):
                break
        return self.energy

    # ------------------------------------------------------------------ posteriors
    def _require_subtypes(self, what):
        self._require_fitted(what)
        if self.responsibilities is None:
            raise ValueError("%s needs a fitted model: call run() first" % what)

    def subtype_posterior(self):
        """
        The subtypes of the patients, from the last run(), as a dict:
            responsibilities (U, G)  q(z_u = g);   labels (U,) int64  their argmax
            rho_mean (G,)            E rho_g = (alpha + n_g) / (G alpha + U);   n_effective (G,)  n_g = sum_u s[u, g]
            coassignment (U, U)      s s^T: the probability under q that two patients share a subtype (the diagonal is sum_g s^2)
        """
        self._require_subtypes("subtype_posterior()")
        s = np.array(self.responsibilities, dtype=np.float64)
        (U, G) = s.shape
        alpha = self._alpha()
        n = s.sum(axis=0)
        return {"responsibilities": s, "labels": np.argmax(s, axis=1).astype(np.int64), "rho_mean": (alpha + n) / (G * alpha + U),
                "n_effective": n, "coassignment": s @ s.T}

    def region_posterior(self):
        """{"p_region" (N, G): q(r_ng = 1), "subtype_names": the G column indices} from the last run()."""
        self._require_subtypes("region_posterior()")
        lq_R = self._lq_R
        return {"p_region": np.exp(lq_R[:, :, 1]), "subtype_names": list(range(lq_R.shape[1]))}

    def connection_posterior(self):
        """
        Per connection and PATIENT, as UnsharedRegionFit.connection_posterior(): p_T (C, U), p_F_tilde (C, U, 3), p_changed
        (C, U).  Given z_u = g the patient's T and F~ have the closed-form law of the unshared model under subtype g's q_R,
        so the result is the mixture over g, weighted with s[u, g], of G calls of the unshared kernel with q_R[:, g] broadcast
        to every patient, summed on the device.  Sessions and noise variances work as in the unshared fit.
        """
        self._require_subtypes("connection_posterior()")
        (N, C, G) = self._check_state(need=("lq_R", "lq_F"))
        U = self._patients()
        resp = self._resp_dev()
        bt = self._bt_dev(C, U)
        out = None
        for g in range(G):
            lq_R = self._d["lq_R"][:, g:g + 1, :].expand(N, U, 2).contiguous()
            post = conn_posterior(self._context(), bt, N, U, self.model.theta(), lq_F=self._d["lq_F"], lq_R=lq_R,
                                  missing_data=self.missing_data, as_tensors=True, **self._noise_bt_kw())
            w = resp[:, g]
            post = {"p_T": post["p_T"] * w[None, :], "p_F_tilde": post["p_F_tilde"] * w[None, :, None],
                    "p_changed": post["p_changed"] * w[None, :]}
            out = post if out is None else {k: out[k] + post[k] for k in out}
        return {k: v.cpu().numpy() for (k, v) in out.items()}

    def assign(self, bt_new, noise_var=None):
        """
        Which subtype's map does a new patient get?  The fit is held and left exactly as it was (q_F, q_R, q(rho), theta, the
        tables).  bt_new (C, U') or (C, U', K'), any K', in the fit's edge order (NaN = unobserved when missing_data);
        noise_var (U',) or (U', K') as in score(): a fit with noise variances refuses None (ValueError).  Returns a dict:
            expected_loglik (U', G)    E[u, g], the expected log-likelihood of patient u under subtype g's map
            responsibilities (U', G)   softmax_g(E[u, g] + E ln rho_g), E ln rho of the fit's q(rho)
        A patient's row does not depend on the other patients of the call.
        """
        self._require_subtypes("assign()")
        bt_new = np.ascontiguousarray(bt_new, dtype=np.float64)
        if bt_new.ndim not in (2, 3) or (bt_new.ndim == 3 and bt_new.shape[2] < 1):
            raise ValueError("bt_new must be (C, U') or (C, U', K') with K' >= 1, got shape %s" % (bt_new.shape,))
        (C, U) = bt_new.shape[:2]
        C_fit = int(self._d["lq_F"].shape[0])
        if C != C_fit:
            raise ValueError("bt_new has %d connections, the fit has %d" % (C, C_fit))
        if U < 1:
            raise ValueError("assign() needs at least one patient")
        if self._has_noise() and noise_var is None:
            raise ValueError("assign(): the fit has noise variances, so the new patients' noise_var must be given (zeros are allowed)")
        noise = self._noise_host(bt_shape=bt_new.shape, bt_var=noise_var, name="noise_var")
        if noise is not None:
            noise = tuple(None if a is None else self._up(a) for a in noise)
        ctx = self._query_context()
        (_S_B, lM_u) = _score.lik_tables(ctx, self._data_dev("b"), self._up(bt_new), self.model.theta(), self.missing_data, noise)
        E = self._expected_loglik(ctx, lM_u)
        el = subtype_E_ln_rho(np.asarray(self.responsibilities, dtype=np.float64).sum(axis=0), self._alpha())
        return {"responsibilities": subtype_softmax(E + el[None, :]), "expected_loglik": E}

    def patient_group_posterior(self, *args, **kwargs):
        """Not provided: the state's columns are the subtypes, not patients."""
        raise ValueError("SubtypeRegionFit has no patient_group_posterior(): the state's columns are the subtypes")

    def patient_trait_posterior(self, *args, **kwargs):
        """Not provided: the state's columns are the subtypes, not patients."""
        raise ValueError("SubtypeRegionFit has no patient_trait_posterior(): the state's columns are the subtypes")

    def score(self, *args, **kwargs):
        """Not provided: see assign() for the subtype of a new patient."""
        raise NotImplementedError("score() is not provided for the subtype-region model: assign() gives a new patient's subtype")

    def membership(self, *args, **kwargs):
        """Not provided: there is no sampler fit of this model."""
        raise NotImplementedError("membership() is not provided for the subtype-region model: it needs a sampler fit")

    def log_evidence(self, *args, **kwargs):
        """Not provided: the inherited AIS would treat L as a data table, which it is not; -energy[-1] is the comparison number."""
        raise NotImplementedError("log_evidence() is not provided for the subtype-region model: the inherited annealing would "
                                  "read the weighted table L as data; compare models by the ELBO, -energy[-1]")


def count_posterior(ctx, lq_R, Nreg, U):
    """
    (p_patient (U, Nreg+1), p_region (Nreg, U+1)) as NumPy float64 through fcd_vb_count_posterior: the Poisson-binomial
    laws of sum_n r_nu and sum_u r_nu with q_nu = P(r_nu = 1) from lq_R (Nreg, U, 2) float64 (need not be normalised).
    """
    import torch
    if tuple(lq_R.shape) != (Nreg, U, 2) or lq_R.dtype != torch.float64:
        raise ValueError("lq_R must be float64 (Nreg, U, 2) = %s" % ((Nreg, U, 2),))
    dev = lq_R.device
    p_patient = torch.empty((U, Nreg + 1), dtype=torch.float64, device=dev)
    p_region = torch.empty((Nreg, U + 1), dtype=torch.float64, device=dev)
    ctx.call("fcd_vb_count_posterior", _lib.dptr(lq_R.contiguous()), int(Nreg), int(U), _lib.dptr(p_patient),
             _lib.dptr(p_region), _lib.stream_ptr())
    return p_patient.cpu().numpy(), p_region.cpu().numpy()


def region_set_independent(ctx, lq_R, Nreg, U, offsets, members):
    """
    (p_count (J, U, S_max+1), p_prevalence (J, U+1)) as NumPy float64 under independent sites with q_nu = P(r_nu = 1) from
    lq_R (Nreg, U, 2) float64 (need not be normalised), for the sets (offsets, members) of region_sets_csr(): both are
    Poisson-binomial laws, made by fcd_vb_count_posterior -- set j's count from the gathered block (|S_j|, U, 2), the
    prevalences of all sets from one (J, U, 2) block of log(prod_n q0), log(1 - prod_n q0).
    """
    import torch
    if tuple(lq_R.shape) != (Nreg, U, 2) or lq_R.dtype != torch.float64:
        raise ValueError("lq_R must be float64 (Nreg, U, 2) = %s" % ((Nreg, U, 2),))
    J = len(offsets) - 1
    sizes = np.diff(offsets)
    p_count = np.zeros((J, U, int(sizes.max()) + 1))
    # log q0 = -log(1 + e^d), d = lq1 - lq0, to full relative accuracy near q0 = 1 (q1 = 0 and q1 = 1 exact)
    d = lq_R[:, :, 1] - lq_R[:, :, 0]
    lq0 = -(torch.clamp(d, min=0.0) + torch.log1p(torch.exp(-torch.abs(d))))
    idx = torch.as_tensor(np.asarray(members, dtype=np.int64), device=lq_R.device)
    for j in range(J):
        rows = idx[int(offsets[j]):int(offsets[j + 1])]
        p_count[j, :, :sizes[j] + 1] = count_posterior(ctx, lq_R[rows].contiguous(), int(sizes[j]), U)[0]
    p_prev = count_posterior(ctx, _region_set_any_block(lq_R, lq0, offsets, idx), J, U)[1]
    return p_count, p_prev


def _region_set_any_block(lq_R, lq0, offsets, idx):
    """(J, U, 2) of log(prod_{n in S_j} q0(n, u)), log(1 - that): the log-law of "patient u has an anomalous region in S_j"."""
    import torch
    J = len(offsets) - 1
    block = torch.empty((J, lq_R.shape[1], 2), dtype=torch.float64, device=lq_R.device)
    for j in range(J):
        block[j, :, 0] = lq0[idx[int(offsets[j]):int(offsets[j + 1])]].sum(dim=0)
    block[:, :, 1] = torch.log(-torch.expm1(block[:, :, 0]))
    return block


def patient_group_independent(ctx, lq_R, Nreg, U, offsets, members, sets=None):
    """
    p_count (J, R, Umax+1) as NumPy float64 under independent sites with q_nu = P(r_nu = 1) from lq_R (Nreg, U, 2) float64 (need
    not be normalised), for the patient groups (offsets, members) of patient_groups_csr(): the number of patients of g_j
    anomalous at a row is Poisson-binomial over the group's columns, made by fcd_vb_count_posterior from the gathered block
    (Nreg, |g_j|, 2); sets = (offsets, members) of region_sets_csr() adds the J_S set rows from the block of
    region_set_independent(), log(prod_n q0), log(1 - prod_n q0).
    """
    import torch
    if tuple(lq_R.shape) != (Nreg, U, 2) or lq_R.dtype != torch.float64:
        raise ValueError("lq_R must be float64 (Nreg, U, 2) = %s" % ((Nreg, U, 2),))
    rows = lq_R
    if sets is not None:
        d = lq_R[:, :, 1] - lq_R[:, :, 0]
        lq0 = -(torch.clamp(d, min=0.0) + torch.log1p(torch.exp(-torch.abs(d))))
        idx = torch.as_tensor(np.asarray(sets[1], dtype=np.int64), device=lq_R.device)
        rows = torch.cat([lq_R, _region_set_any_block(lq_R, lq0, sets[0], idx)], dim=0)
    R = int(rows.shape[0])
    J = len(offsets) - 1
    sizes = np.diff(offsets)
    p_count = np.zeros((J, R, int(sizes.max()) + 1))
    cols = torch.as_tensor(np.asarray(members, dtype=np.int64), device=lq_R.device)
    for j in range(J):
        block = rows[:, cols[int(offsets[j]):int(offsets[j + 1])]].contiguous()
        p_count[j, :, :sizes[j] + 1] = count_posterior(ctx, block, R, int(sizes[j]))[1]
    return p_count


def patient_group_summaries(p_count, p_joint, sizes, pairs, level=0.95):
    """
    The derived quantities of patient_group_posterior() from the laws alone (host arithmetic): prevalence (J, R) = E[k_j]/|g_j|
    from p_count (J, R, Umax+1); per contrast (a, b) of `pairs` with its joint law p_joint[p] (R, |a|+1, |b|+1): p_greater,
    p_less, p_equal (P, R) of k_a/|a| against k_b/|b| -- decided on the integers k_a |b| - k_b |a|, so equal rates of groups of
    unequal sizes are equal --, diff_mean (P, R) and diff_interval (P, R, 2), the central `level` interval of the difference.
    """
    p_count = np.asarray(p_count, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    (P, R) = (len(pairs), p_count.shape[1])
    out = {"prevalence": (p_count @ np.arange(p_count.shape[2], dtype=np.float64)) / sizes[:, None].astype(np.float64)}
    for key in ("p_greater", "p_less", "p_equal", "diff_mean"):
        out[key] = np.zeros((P, R))
    out["diff_interval"] = np.zeros((P, R, 2))
    (q_lo, q_hi) = ((1.0 - level) / 2.0, (1.0 + level) / 2.0)
    for (p, (a, b)) in enumerate(pairs):
        (na, nb) = (int(sizes[a]), int(sizes[b]))
        pj = np.asarray(p_joint[p], dtype=np.float64).reshape(R, (na + 1) * (nb + 1))
        num = (np.arange(na + 1, dtype=np.int64)[:, None] * nb - np.arange(nb + 1, dtype=np.int64)[None, :] * na).reshape(-1)
        out["p_greater"][p] = pj[:, num > 0].sum(axis=1)
        out["p_less"][p] = pj[:, num < 0].sum(axis=1)
        out["p_equal"][p] = pj[:, num == 0].sum(axis=1)
        diff = num.astype(np.float64) / float(na * nb)
        out["diff_mean"][p] = pj @ diff
        order = np.argsort(num, kind="stable")
        cum = np.cumsum(pj[:, order], axis=1)
        for (i, q) in enumerate((q_lo, q_hi)):
            at = np.minimum((cum < q - 1e-12).sum(axis=1), len(order) - 1)
            out["diff_interval"][p, :, i] = diff[order][at]
    return out


def patient_trait_summaries(trait_hist, trait_sum, n_known, level=0.95):
    """
    The derived quantities of patient_trait_posterior() from the two accumulated buffers alone (host arithmetic): trait_hist
    (Q, R, Umax+1 + NB + 3) and trait_sum (Q, R, Umax+1) as fcd_gibbs_patient_trait_tally fills them, n_known (Q,).  Returns
    p_count, p_defined, p_greater, p_less, p_equal, auc_mean, auc_hist, auc_edges, auc_interval.
    """
    NB = PATIENT_TRAIT_BINS
    h = np.asarray(trait_hist).astype(np.int64)
    s = np.asarray(trait_sum).astype(np.int64)
    n_known = np.asarray(n_known, dtype=np.int64)
    (Q, R, K) = s.shape
    if h.shape != (Q, R, K + NB + 3) or n_known.shape != (Q,) or int(n_known.max()) + 1 != K:
        raise ValueError("trait_hist must be (Q, R, Umax+1+%d+3) and trait_sum (Q, R, Umax+1) with Umax = max(n_known)" % NB)
    (counts, bins, signs) = (h[:, :, :K], h[:, :, K:K + NB], h[:, :, K + NB:])
    total = counts.sum(axis=2).astype(np.float64)
    defined = signs.sum(axis=2).astype(np.float64)
    k = np.arange(K, dtype=np.int64)[None, :]
    d2 = 2 * k * (n_known[:, None] - k)                              # 2 k (n_q - k); <= 0 where the state is not defined
    weight = np.where(d2 > 0, 1.0 / np.maximum(d2, 1), 0.0)          # (Q, K)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"p_count": counts / total[:, :, None], "p_defined": defined / total,
               "p_less": signs[:, :, 0] / defined, "p_equal": signs[:, :, 1] / defined, "p_greater": signs[:, :, 2] / defined,
               "auc_mean": 0.5 + (s * weight[:, None, :]).sum(axis=2) / defined,
               "auc_hist": bins / defined[:, :, None], "auc_edges": np.arange(NB + 1, dtype=np.float64) / NB}
    alpha = (1.0 - float(level)) / 2.0
    up = np.cumsum(out["auc_hist"], axis=2)
    down = np.cumsum(out["auc_hist"][:, :, ::-1], axis=2)
    lo = np.minimum((up < alpha - 1e-12).sum(axis=2), NB - 1)        # first bin at which the mass from below reaches alpha
    hi = NB - 1 - np.minimum((down < alpha - 1e-12).sum(axis=2), NB - 1)
    interval = np.stack([lo / float(NB), (hi + 1) / float(NB)], axis=2)
    interval[defined == 0] = np.nan
    out["auc_interval"] = interval
    return out


def coanomaly_independent(ctx, lq_R, Nreg, U):
    """
    (region (Nreg, Nreg), patient (U, U)) as NumPy float64 through fcd_vb_coanomaly: sum_u q_nu q_mu and sum_n q_nu q_nv off
    the diagonals, sum_u q_nu and sum_n q_nu on them, with q_nu = P(r_nu = 1) from lq_R (Nreg, U, 2) float64 (need not be
    normalised).
    """
    import torch
    if tuple(lq_R.shape) != (Nreg, U, 2) or lq_R.dtype != torch.float64:
        raise ValueError("lq_R must be float64 (Nreg, U, 2) = %s" % ((Nreg, U, 2),))
    dev = lq_R.device
    region = torch.empty((Nreg, Nreg), dtype=torch.float64, device=dev)
    patient = torch.empty((U, U), dtype=torch.float64, device=dev)
    ctx.call("fcd_vb_coanomaly", _lib.dptr(lq_R.contiguous()), int(Nreg), int(U), _lib.dptr(region), _lib.dptr(patient),
             _lib.stream_ptr())
    return region.cpu().numpy(), patient.cpu().numpy()


def coanomaly_from_counts(region_pair_counts, patient_pair_counts, states):
    """
    The joint entries of coanomaly_posterior() from the sampler's pair counts (Nreg, Nreg) and (U, U) over `states` chain
    states (sweeps x chains, all ranks): each count over `states` is an expected number, over U or Nreg more a probability.
    """
    rp = np.asarray(region_pair_counts, dtype=np.float64)
    pp = np.asarray(patient_pair_counts, dtype=np.float64)
    (N, U) = (rp.shape[0], pp.shape[0])
    if rp.shape != (N, N) or pp.shape != (U, U):
        raise ValueError("pair counts must be square: (Nreg, Nreg) and (U, U)")
    states = int(states)
    if states < 1:
        raise ValueError("no chain state behind the pair counts")
    return {"p_region_pair": rp / (float(states) * U), "expected_patients": rp / float(states),
            "p_patient_pair": pp / (float(states) * N), "expected_regions": pp / float(states)}


def conn_posterior(ctx, bt_dev, Nreg, U, theta, counts=None, lq_F=None, lq_R=None, missing_data=False, noise_var=None,
                   as_tensors=False):
    """
    {p_T (C,U), p_F_tilde (C,U,3), p_changed (C,U)} as NumPy float64 through fcd_conn_posterior: weights from `counts`
    (C,U,3,3) uint32 (held in an int32 tensor), or from the log-probabilities lq_F (C,1,3) and lq_R (Nreg,U,2).
    missing_data: a NaN of bt is unobserved (fcd_conn_posterior_ex with FCD_DATA_NAN_MISSING).
    bt_dev (C, U, K): K sessions per patient (fcd_conn_posterior_sessions); an item with no observed session gets the prior law.
    noise_var: float64 device tensor (U, K) ((U,) or (U, 1) for a 2-D bt) of known measurement variances on top of sigma^2
    (fcd_conn_posterior_noise, for a bt of either rank); None: none.
    as_tensors: the three as device tensors, for a caller that combines several calls on the device.
    """
    import torch
    C = util.N_to_C(int(Nreg))
    dev = bt_dev.device
    if bt_dev.dim() not in (2, 3) or tuple(bt_dev.shape[:2]) != (C, U) or bt_dev.dtype != torch.float64:
        raise ValueError("bt must be float64 (C, U) = %s or (C, U, K)" % ((C, U),))
    if bt_dev.dim() == 3 and int(bt_dev.shape[2]) < 1:
        raise ValueError("bt (C, U, K) needs K >= 1 sessions")
    if counts is not None:
        if tuple(counts.shape) != (C, U, 3, 3) or counts.element_size() != 4:
            raise ValueError("counts must be 32-bit (C, U, 3, 3)")
    elif lq_F is None or lq_R is None or tuple(lq_F.shape) != (C, 1, 3) or tuple(lq_R.shape) != (Nreg, U, 2):
        raise ValueError("lq_F must be (C, 1, 3) and lq_R (Nreg, U, 2)")
    p_T = torch.empty((C, U), dtype=torch.float64, device=dev)
    p_Ft = torch.empty((C, U, 3), dtype=torch.float64, device=dev)
    p_ch = torch.empty((C, U), dtype=torch.float64, device=dev)
    (th, _th) = _lib.dbl_array(theta)
    sessions = () if bt_dev.dim() == 2 else (int(bt_dev.shape[2]),)
    name = "fcd_conn_posterior_sessions" if sessions else "fcd_conn_posterior_ex"
    noise = ()
    if noise_var is not None:
        K = sessions[0] if sessions else 1
        if noise_var.dtype != torch.float64 or tuple(noise_var.shape) not in ((U, K),) + (() if sessions else ((U,),)):
            raise ValueError("noise_var must be float64 (U, K) = %s" % ((U, K),))
        (name, sessions, noise) = ("fcd_conn_posterior_noise", (K,), (_lib.dptr(noise_var.contiguous()),))
    ctx.call(name, _lib.dptr(bt_dev.contiguous()), int(Nreg),
             int(U), *sessions, th, *noise, _lib.dptr(None if counts is None else counts.contiguous()),
             _lib.dptr(None if lq_F is None else lq_F.contiguous()), _lib.dptr(None if lq_R is None else lq_R.contiguous()),
             _lib.FCD_DATA_NAN_MISSING if missing_data else 0, _lib.dptr(p_T), _lib.dptr(p_Ft), _lib.dptr(p_ch),
             _lib.stream_ptr())
    if as_tensors:
        return {"p_T": p_T, "p_F_tilde": p_Ft, "p_changed": p_ch}
    return {"p_T": p_T.cpu().numpy(), "p_F_tilde": p_Ft.cpu().numpy(), "p_changed": p_ch.cpu().numpy()}


def _objective_flags(bt_dev, W, missing_data, per_edge):
    """(flags, U) of the theta objectives; per_edge: W is (C, 1, 3, 3) for every patient of bt (C, U)."""
    flags = _lib.FCD_DATA_NAN_MISSING if missing_data else 0
    if not per_edge:
        return flags, int(W.shape[1])
    C, U = int(bt_dev.shape[0]), int(bt_dev.shape[1])
    if tuple(W.shape) != (C, 1, 3, 3):
        raise ValueError("per-edge weights must be (C, 1, 3, 3) = %s, got %s" % ((C, 1, 3, 3), tuple(W.shape)))
    return flags | _lib.FCD_W_PER_EDGE, U


def theta_sub_objective(ctx, bt_dev, W, theta, reduce=None, missing_data=False, per_edge=False):
    """
    (S, dS/d eta, dS/d epsilon), S = sum W ln M(bt; eta, epsilon), through fcd_theta_sub_objective_ex.
    `reduce` (optional) sums the three numbers over ranks (multi-GPU sampler: W holds this rank's chain counts).
    missing_data: an item with NaN bt adds nothing (its M = 1 does not depend on eta or epsilon).
    per_edge: W is (C, 1, 3, 3) and weights every patient's item of its edge, S = sum W[c,k,l] sum_u ln M_kl(bt_cu)
    (FCD_W_PER_EDGE: the shared-region fit).
    """
    import torch
    out = torch.empty(3, dtype=torch.float64, device=W.device)
    (th, _th) = _lib.dbl_array(theta)
    (flags, U) = _objective_flags(bt_dev, W, missing_data, per_edge)
    ctx.call("fcd_theta_sub_objective_ex", _lib.dptr(bt_dev), _lib.dptr(W), int(W.shape[0]), U, th, flags, _lib.dptr(out),
             _lib.stream_ptr())
    if reduce is not None:
        out = reduce(out)
    return out.cpu().numpy()


def theta_full_objective(ctx, b_dev, bt_dev, W, theta, reduce=None, missing_data=False, per_edge=False):
    """
    {S, dS/d eta, dS/d epsilon, dS/d mu[3], dS/d sigma^2[3]} of the full theta_sub objective (fcd_theta_full_objective):
    S = E[ln p(b | f)] + E[ln p(bt | f, r)] for the weights W.  `reduce` sums the nine numbers over ranks.
    With several ranks each rank's W holds its own chain counts, but b is the same on all: pass b_dev on every rank
    (the healthy term scales with the chain counts too, so the sum over ranks is the pooled objective).
    missing_data: a NaN bt item adds nothing to any term, a NaN b adds nothing to the ln N / mu / sigma^2 terms.
    per_edge: W is (C, 1, 3, 3) for every patient of bt (FCD_W_PER_EDGE), as in theta_sub_objective.
    """
    import torch
    out = torch.empty(9, dtype=torch.float64, device=W.device)
    (th, _th) = _lib.dbl_array(theta)
    H = int(b_dev.shape[1]) if b_dev is not None else 0
    (flags, U) = _objective_flags(bt_dev, W, missing_data, per_edge)
    ctx.call("fcd_theta_full_objective_ex", _lib.dptr(b_dev), _lib.dptr(bt_dev), _lib.dptr(W), int(W.shape[0]), H, U, th,
             flags, _lib.dptr(out), _lib.stream_ptr())
    if reduce is not None:
        out = reduce(out)
    return out.cpu().numpy()


def minimize_theta_full(ctx, b_dev, bt_dev, W, model, reduce=None, bound_eps=1e-5, missing_data=False, per_edge=False):
    """
    argmin of -(E[ln p(b | f)] + E[ln p(bt | f, r)]) over theta_sub = (eta, epsilon, mu[3], sigma^2[3]): the step the
    reference intends (fit.py:222-286 with its commented-out lines read in): pack order and sigma ** 2 as in
    fit.py:243-252, bounds of fit.py:228-237 -- eta, epsilon in (e, 1-e), mu_0 in (-1+e, -e), mu_1 in (-e, e), mu_2 in
    (e, 1-e), sigma^2 > e --, analytic gradient, L-BFGS-B.  Returns (eta, epsilon, mu, sigma, scipy result).
    missing_data: NaN in b / bt is unobserved (theta_full_objective).  per_edge: W is (C, 1, 3, 3) (theta_sub_objective).
    """
    import scipy.optimize as spopt
    base = np.array(model.theta(), dtype=np.float64)
    e = bound_eps

    def unpack(x):
        th = base.copy()
        th[1], th[2] = float(x[0]), float(x[1])
        th[6:9] = x[2:5]
        th[9:12] = np.sqrt(x[5:8])
        return th

    def fun(x):
        o = theta_full_objective(ctx, b_dev, bt_dev, W, unpack(x), reduce, missing_data=missing_data, per_edge=per_edge)
        return (-o[0], -o[1:9])
    bnds = ((e, 1 - e), (e, 1 - e), (-1 + e, 0 - e), (0 - e, 0 + e), (0 + e, 1 - e), (0 + e, None), (0 + e, None), (0 + e, None))
    x0 = np.concatenate([[model.eta, model.epsilon], np.asarray(model.mu, dtype=np.float64),
                         np.asarray(model.sigma, dtype=np.float64) ** 2])
    lo = np.array([bd[0] for bd in bnds])
    hi = np.array([np.inf if bd[1] is None else bd[1] for bd in bnds])
    x0 = np.minimum(np.maximum(x0, lo), hi)
    res = spopt.minimize(fun, x0, jac=True, bounds=bnds, method="L-BFGS-B")
    th = unpack(res.x)
    return float(th[1]), float(th[2]), th[6:9].copy(), th[9:12].copy(), res


def minimize_theta_sub(ctx, bt_dev, W, model, reduce=None, bound_eps=1e-5, missing_data=False, per_edge=False):
    """
    argmin over (eta, epsilon) in [1e-5, 1-1e-5]^2 of -sum W ln M (fit.py:222-241), analytic gradient, L-BFGS-B.
    Returns (eta, epsilon, scipy result).  The model is not modified.  missing_data: NaN in bt is unobserved.
    per_edge: W is (C, 1, 3, 3) for every patient (theta_sub_objective).
    """
    import scipy.optimize as spopt
    base = np.array(model.theta(), dtype=np.float64)

    def fun(x):
        th = base.copy()
        th[1], th[2] = float(x[0]), float(x[1])
        (S, dh, de) = theta_sub_objective(ctx, bt_dev, W, th, reduce, missing_data=missing_data, per_edge=per_edge)
        return (-S, np.array([-dh, -de]))
    bnds = ((bound_eps, 1 - bound_eps), (bound_eps, 1 - bound_eps))          # fit.py:228-231
    x0 = np.clip(np.array([model.eta, model.epsilon], dtype=np.float64), bound_eps, 1 - bound_eps)
    res = spopt.minimize(fun, x0, jac=True, bounds=bnds, method="L-BFGS-B")
    return float(res.x[0]), float(res.x[1]), res


# ---------------------------------------------------------------------------------------------------------
# Module-level helpers of the reference (fcdiff/fit.py:382-733).  They are small closed forms on whole arrays
# that the reference's tests call directly; the fit path itself evaluates them inside the kernels above.
# Kept as NumPy one-liners with the reference's names, argument order and return shapes.
# ---------------------------------------------------------------------------------------------------------
def _eval_q_R_w(q_R, n, m):
    """(U,3) weights of a region pair: both typical, both anomalous, discordant (fit.py:382-406)."""
    w = np.zeros((q_R.shape[1], 3))
    w[:, 0] = q_R[n, :, 0] * q_R[m, :, 0]
    w[:, 1] = q_R[n, :, 1] * q_R[m, :, 1]
    w[:, 2] = q_R[n, :, 0] * q_R[m, :, 1]
    w[:, 2] += q_R[n, :, 1] * q_R[m, :, 0]
    return w


def _eval_M_eps(eta, epsilon, l):
    """Probability of keeping the template type under mixture case l (fit.py:433-444)."""
    if l == 0:
        return 1 - epsilon
    if l == 1:
        return epsilon
    eps = eta * epsilon
    eps += (1 - eta) * (1 - epsilon)
    return eps


def _eval_M(N, eta, epsilon, k, l):
    """M_kl from the Normal densities N (C,U,3) (fit.py:409-430)."""
    eps = _eval_M_eps(eta, epsilon, l)
    others = [j for j in range(3) if j != k]
    return eps * N[:, :, k] + (1 - eps) * 0.5 * (N[:, :, others[0]] + N[:, :, others[1]])


def _eval_E_lp_F(q_F, gamma):
    return np.sum(q_F * np.log(gamma))


def _eval_E_lp_B_g_F(q_F, lp_B_g_F):
    return np.sum(q_F * lp_B_g_F)


def _eval_E_lp_R(q_R, pi):
    return np.sum(q_R * np.log(pi))


def _eval_E_lM(q_F, q_R, lM):
    """E[log p(bt | f, r)] (fit.py:489-511), vectorised over edges."""
    C = q_F.shape[0]
    N = q_R.shape[0]
    (n, m) = np.tril_indices(N, -1)       # lower-triangular row-major == util.c_to_nm order
    assert n.shape[0] == C
    w = np.stack([q_R[n, :, 0] * q_R[m, :, 0], q_R[n, :, 1] * q_R[m, :, 1],
                  q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]], axis=2)      # (C,U,3)
    return np.sum(q_F[:, 0, :] * np.einsum("cul,cukl->ck", w, lM))


def _eval_E_lq_F(q_F, lq_F):
    return np.sum(q_F * lq_F)


def _eval_E_lq_R(q_R, lq_R):
    return np.sum(q_R * lq_R)


def _eval_dlN_dm(b, mu, sigma):
    return (b - mu) / (sigma * sigma)


def _eval_dlN_ds(b, mu, sigma):
    diff = b - mu
    sigma2 = sigma * sigma
    return ((diff * diff) - sigma2) / (2 * sigma2)


def _eval_dN_dm(N, b, mu, sigma):
    return N * _eval_dlN_dm(b, mu, sigma)


def _eval_dN_ds(N, b, mu, sigma):
    return N * _eval_dlN_ds(b, mu, sigma)


def _eval_dlM_dm(norm, mix, mu, sigma, eta, epsilon, k, l):
    """fit.py:572-597, quirk Q8 included (tests k != l; passes the density array where b is expected)."""
    eps = _eval_M_eps(eta, epsilon, l)
    if k != l:
        eps = 0.5 * (1 - eps)
    return eps * _eval_dlN_dm(norm, mu, sigma) / mix


def _eval_dlM_dh(norm, mix, epsilon, k):
    """fit.py:618-641."""
    eps = (2 * epsilon) - 1
    others = [j for j in range(3) if j != k]
    s = norm[:, :, others[0]] + norm[:, :, others[1]]
    return (eps * norm[:, :, k] - 0.5 * eps * s) / mix


def _eval_dlM_de(norm, mix, eta, k, l):
    """fit.py:667-697."""
    eps = -1 if l == 0 else (1 if l == 1 else 2 * eta - 1)
    others = [j for j in range(3) if j != k]
    s = norm[:, :, others[0]] + norm[:, :, others[1]]
    return (eps * norm[:, :, k] - 0.5 * eps * s) / mix


def _pair_weights(q_R):
    N = q_R.shape[0]
    (n, m) = np.tril_indices(N, -1)
    w0 = q_R[n, :, 0] * q_R[m, :, 0]
    w1 = q_R[n, :, 1] * q_R[m, :, 1]
    w2 = q_R[n, :, 0] * q_R[m, :, 1] + q_R[n, :, 1] * q_R[m, :, 0]
    return w0, w1, w2


def _eval_dE_dm(q_F, q_R, dlN_dmj, dlM_dmj, j):
    """dE/dmu_j (fit.py:542-569), vectorised over edges."""
    (w0, w1, w2) = _pair_weights(q_R)
    w = np.stack([w0, w1, w2], axis=2)
    d = -np.sum(q_F[:, 0, j] * np.sum(dlN_dmj, axis=1))
    d -= np.sum(q_F[:, 0, :] * np.einsum("cul,cukl->ck", w, dlM_dmj))
    return d


def _eval_dE_dh(q_R, q_F, norm, mix, epsilon):
    """dE/deta (fit.py:600-615)."""
    (_w0, _w1, w2) = _pair_weights(q_R)
    d = 0.0
    for k in range(3):
        d -= np.sum(q_F[:, 0, k] * np.sum(w2 * _eval_dlM_dh(norm, mix[:, :, k, 2], epsilon, k), axis=1))
    return d


def _eval_dE_de(q_R, q_F, norm, mix, eta):
    """dE/depsilon (fit.py:644-664)."""
    (w0, w1, w2) = _pair_weights(q_R)
    d = 0.0
    for k in range(3):
        s = w0 * _eval_dlM_de(norm, mix[:, :, k, 0], eta, k, 0)
        s += w1 * _eval_dlM_de(norm, mix[:, :, k, 1], eta, k, 1)
        s += w2 * _eval_dlM_de(norm, mix[:, :, k, 2], eta, k, 2)
        d -= np.sum(q_F[:, 0, k] * np.sum(s, axis=1))
    return d
