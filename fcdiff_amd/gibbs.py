"""
Many-chain collapsed Gibbs sampler for the IAR model on one MI355X, plus the multi-GPU driver.

The reference ships only the variational fitter (doc/methods.rst:236-239); this sampler is the build's
extension named by BASELINE.json.  Its conditionals are the reference's updates at one-hot q
(fcdiff/fit.py:170-173 for f, :187-194 for r), its M-step for (pi, gamma) the sample version of
fit.py:208-220 -- see include/fcdiff_hip.h for the kernel-level contract.

Multi-GPU (one process per GPU, torch.distributed, backend "nccl" = RCCL): chains are independent given
the tables, so rank k simply owns global chain ids [chain0, chain0 + G).  The only exchange is the
all-reduce of the 8-word pooled-count vector before an M-step; there is no data-path collective.
"""
import collections
import ctypes as C
import weakref

import numpy as np

from . import _lib
from . import tables
from . import util


PAIR_COUNT_MAX = (1 << 32) - 1
COUNT_MAX_NREG, COUNT_MAX_U = 1023, 512      # largest shape of the anomalous-region histograms (fcd_gibbs_count_tally)

REGION_SET_MAX_SIZE, REGION_SET_MAX_SETS = 1023, 1024     # fcd_region_sets_set
PATIENT_GROUP_MAX_U, PATIENT_GROUP_MAX_GROUPS, PATIENT_GROUP_MAX_CONTRASTS = 512, 64, 64     # fcd_patient_groups_set
PATIENT_GROUP_MAX_BINS = 16384          # (|a|+1)(|b|+1) of a contrast: the LDS of the workgroup that owns a joint row
PATIENT_TRAIT_MAX_U, PATIENT_TRAIT_MAX_TRAITS, PATIENT_TRAIT_BINS = 512, 16, 128     # fcd_patient_traits_set

# The accumulators GibbsEngine.run() can add to after a counted sweep, in the order it checks and attaches them (the order of
# FCD_ACC_* in fcd_common.h).  Engine attributes of one: `attr` holds the buffers (None: detached; one tensor, or a pair where
# `paired`), <key>_every the period and <key>_sweeps the sweeps added so far.  shapes: engine -> shape of each buffer; dtypes:
# of each buffer ("int32" holds uint32 counts, like cnt_f; "int64" sums of signed scores); setter: the library's entry point
# (buffers, Nreg, U, every); sites: None, or (Nreg, U) -> how many sites of a chain one counter can take per sweep; label: the
# accumulator's name in the error messages; send: None, or the engine's method that puts on the shared context what the
# setter's kernels read there (sets, groups, traits), called before the setter.
Accumulator = collections.namedtuple("Accumulator", "key attr paired shapes dtypes setter sites label send")
ACCUMULATORS = (
    Accumulator("pair", "pair_acc", False, lambda e: ((e.C, e.U, 3, 3),), ("int32",),
                "fcd_gibbs_set_pair_accumulator", None, "pair", None),
    Accumulator("count", "count_hist", True, lambda e: ((e.U, e.Nreg + 1), (e.Nreg, e.U + 1)), ("int32", "int32"),
                "fcd_gibbs_set_count_accumulator", None, "count", None),
    # (a diagonal entry counts up to G x U or G x Nreg sites per sweep)
    Accumulator("coanomaly", "coanomaly_acc", True, lambda e: ((e.Nreg, e.Nreg), (e.U, e.U)), ("int32", "int32"),
                "fcd_gibbs_set_coanomaly_accumulator", lambda Nreg, U: max(Nreg, U), "co-anomaly", None),
    # (shapes from the sets of set_region_sets())
    Accumulator("region_set", "region_set_acc", True,
                lambda e: ((e.region_J, e.U, e.region_smax + 1), (e.region_J, e.U + 1)), ("int32", "int32"),
                "fcd_gibbs_set_region_set_accumulator", None, "region-set", "_send_region_sets"),
    # (shapes from set_patient_groups(): (J, R, Umax+1) and the flat joint histograms of the contrasts)
    Accumulator("patient_group", "patient_group_acc", True,
                lambda e: ((e.group_J, e.patient_group_rows(), e.group_umax + 1),
                           (max(1, e.patient_group_rows() * int(e.group_bin_offsets[-1])),)), ("int32", "int32"),
                "fcd_gibbs_set_patient_group_accumulator", None, "patient-group", "_send_patient_groups"),
    # (rank sums of the patient traits: (Q, R, Umax+1 + NB + 3) counts and (Q, R, Umax+1) sums)
    Accumulator("patient_trait", "patient_trait_acc", True,
                lambda e: ((e.trait_Q, e.patient_trait_rows(), e.trait_umax + 1 + PATIENT_TRAIT_BINS + 3),
                           (e.trait_Q, e.patient_trait_rows(), e.trait_umax + 1)), ("int32", "int64"),
                "fcd_gibbs_set_patient_trait_accumulator", None, "patient-trait", "_send_patient_traits"),
)
(_PAIR, _COUNT, _COANOMALY, _REGION_SET, _PATIENT_GROUP, _PATIENT_TRAIT) = ACCUMULATORS


# the wording of _index_sets_csr()'s refusals for the two axes: knob, one set, many, a member, the mask's name and extent
_REGION_WORDS = ("region_sets", "region set", "sets", "region", "region-set", "Nreg")
_PATIENT_WORDS = ("patient_groups", "patient group", "groups", "patient", "patient-group", "U")


def _index_sets_csr(sets, extent, words, max_sets, max_size=None):
    """What region_sets_csr() and patient_groups_csr() share: the three input forms, the refusals, the CSR arrays."""
    (knob, one, many, member, mask_name, extent_name) = words
    if isinstance(sets, dict):
        names = [str(k) for k in sets.keys()]
        rows = list(sets.values())
    else:
        mask = sets if isinstance(sets, np.ndarray) else None
        if mask is not None and mask.dtype == np.bool_:
            if mask.ndim != 2 or mask.shape[1] != extent:
                raise ValueError("a %s mask must be boolean (J, %s=%d)" % (mask_name, extent_name, extent))
            rows = [np.flatnonzero(m) for m in mask]
        else:
            rows = list(sets)
        names = [str(j) for j in range(len(rows))]
    if len(rows) < 1:
        raise ValueError("%s holds no %s" % (knob, many[:-1]))
    if len(rows) > max_sets:
        raise ValueError("%s holds %d %s (at most %d)" % (knob, len(rows), many, max_sets))
    (offsets, members) = ([0], [])
    for (name, row) in zip(names, rows):
        a = np.asarray(row)
        if a.ndim != 1 or a.size == 0:
            raise ValueError("%s %r is empty (or not a sequence of indices)" % (one, name))
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("%s %r must hold integer %s indices" % (one, name, member))
        a = np.sort(a.astype(np.int64))
        if a[0] < 0 or a[-1] >= extent:
            raise ValueError("%s %r has an index outside [0, %d)" % (one, name, extent))
        if np.any(a[1:] == a[:-1]):
            raise ValueError("%s %r names a %s twice" % (one, name, member))
        if max_size is not None and a.size > max_size:
            raise ValueError("%s %r has %d members (at most %d)" % (one, name, a.size, max_size))
        members.append(a)
        offsets.append(offsets[-1] + a.size)
    return names, np.asarray(offsets, dtype=np.int32), np.concatenate(members).astype(np.int32)


def region_sets_csr(sets, Nreg):
    """
    Region sets in any of their three forms -- a dict name -> sequence of region indices, a sequence of index sequences
    (named "0", "1", ...), a boolean mask (J, Nreg) -- as (names, offsets (J+1,) int32, members int32): CSR with the members
    of a set ascending, what fcd_region_sets_set takes.  ValueError for no set, an empty set, a duplicate, an index outside
    [0, Nreg), more than 1023 members or more than 1024 sets.
    """
    return _index_sets_csr(sets, int(Nreg), _REGION_WORDS, REGION_SET_MAX_SETS, REGION_SET_MAX_SIZE)


def patient_groups_csr(groups, U):
    """
    Groups of patients in any of their three forms -- a dict name -> sequence of patient indices, a sequence of index
    sequences (named "0", "1", ...), a boolean mask (J, U) -- as (names, offsets (J+1,) int32, members int32): CSR with the
    members of a group ascending, what fcd_patient_groups_set takes.  The ValueErrors of region_sets_csr() on the patient
    axis: no group, an empty group, a duplicate, an index outside [0, U), more than 64 groups or more than 512 patients.
    """
    U = int(U)
    if U > PATIENT_GROUP_MAX_U:
        raise ValueError("patient groups are made for at most %d patients (here %d)" % (PATIENT_GROUP_MAX_U, U))
    return _index_sets_csr(groups, U, _PATIENT_WORDS, PATIENT_GROUP_MAX_GROUPS)


def patient_group_contrasts(contrasts, names, offsets, members):
    """
    Contrasts between the groups of patient_groups_csr() -- pairs (a, b) of group names or indices, or None -- as
    (pairs (P, 2) int32, bin_offsets (P+1,) int64): bin_offsets[p] = sum_{q < p} (|a_q|+1)(|b_q|+1), the start of contrast p's
    joint histogram of one row.  ValueError for an unknown name or index, a contrast that names a group twice, overlapping
    groups, more than 64 contrasts or a contrast of more than 16384 joint bins.
    """
    J = len(names)
    rows = [] if contrasts is None else list(contrasts)
    if len(rows) > PATIENT_GROUP_MAX_CONTRASTS:
        raise ValueError("patient_group_contrasts holds %d contrasts (at most %d)" % (len(rows), PATIENT_GROUP_MAX_CONTRASTS))

    def index(key):
        if isinstance(key, str):
            if key not in names:
                raise ValueError("a contrast names the unknown patient group %r" % key)
            return names.index(key)
        if isinstance(key, (bool, np.bool_)) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < J:
            raise ValueError("a contrast names the patient group %r: not a name or an index in [0, %d)" % (key, J))
        return int(key)
    sizes = np.diff(offsets).astype(np.int64)
    pairs = np.zeros((len(rows), 2), dtype=np.int32)
    bin_offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    for (p, row) in enumerate(rows):
        row = tuple(row)
        if len(row) != 2:
            raise ValueError("a contrast is a pair of patient groups, got %r" % (row,))
        (a, b) = (index(row[0]), index(row[1]))
        if a == b:
            raise ValueError("contrast %d names patient group %r twice" % (p, names[a]))
        if np.intersect1d(members[offsets[a]:offsets[a + 1]], members[offsets[b]:offsets[b + 1]]).size:
            raise ValueError("the patient groups %r and %r of contrast %d overlap" % (names[a], names[b], p))
        bins = int((sizes[a] + 1) * (sizes[b] + 1))
        if bins > PATIENT_GROUP_MAX_BINS:
            raise ValueError("contrast %d of patient groups %r and %r has %d joint bins (at most %d)"
                             % (p, names[a], names[b], bins, PATIENT_GROUP_MAX_BINS))
        pairs[p] = (a, b)
        bin_offsets[p + 1] = bin_offsets[p] + bins
    return pairs, bin_offsets


def patient_traits_scores(traits, U):
    """
    Traits of the patients -- a dict name -> (U,) values, a sequence of such vectors (named "0", "1", ...) or an array (Q, U);
    NaN: not known for this patient -- as (names, scores (Q, U) int32, known (Q, U) bool, n_known (Q,) int64), what
    fcd_patient_traits_set takes: scores[q, u] = 2 midrank_u - (n_q + 1) over the n_q known patients of trait q (tied values
    share a midrank; integers in [-(n_q - 1), n_q - 1] that sum to 0), 0 where the trait is not known.  A binary trait with n1
    ones and n0 zeros gives -n1 on the zeros and n0 on the ones.  ValueError for no trait, more than 16 traits, more than 512
    patients, a vector that is not (U,) numbers, an infinite value, fewer than two known patients, or known values all equal.
    """
    U = int(U)
    if U > PATIENT_TRAIT_MAX_U:
        raise ValueError("patient traits are made for at most %d patients (here %d)" % (PATIENT_TRAIT_MAX_U, U))
    if isinstance(traits, dict):
        names = [str(k) for k in traits.keys()]
        rows = list(traits.values())
    else:
        if isinstance(traits, np.ndarray) and traits.ndim != 2:
            raise ValueError("a patient-trait array must be (Q, U=%d)" % U)
        rows = list(traits)
        names = [str(q) for q in range(len(rows))]
    if len(rows) < 1:
        raise ValueError("patient_traits holds no trait")
    if len(rows) > PATIENT_TRAIT_MAX_TRAITS:
        raise ValueError("patient_traits holds %d traits (at most %d)" % (len(rows), PATIENT_TRAIT_MAX_TRAITS))
    scores = np.zeros((len(rows), U), dtype=np.int32)
    known = np.zeros((len(rows), U), dtype=np.bool_)
    for (q, (name, row)) in enumerate(zip(names, rows)):
        try:
            y = np.asarray(row, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("patient trait %r must hold numbers" % name)
        if y.shape != (U,):
            raise ValueError("patient trait %r must be a vector of U=%d values" % (name, U))
        if np.isinf(y).any():
            raise ValueError("patient trait %r has an infinite value (NaN marks a patient it is not known for)" % name)
        known[q] = ~np.isnan(y)
        n = int(known[q].sum())
        if n < 2:
            raise ValueError("patient trait %r is known for %d patients (at least 2)" % (name, n))
        (_values, inverse, counts) = np.unique(y[known[q]], return_inverse=True, return_counts=True)
        if counts.size < 2:
            raise ValueError("the known values of patient trait %r are all equal" % name)
        below = np.cumsum(counts)                       # 2 midrank = 2 below - count + 1 (ranks from 1)
        scores[q, known[q]] = (2 * below - counts)[inverse.reshape(-1)] - n
    return names, scores, known, known.sum(axis=1).astype(np.int64)


def pair_sweeps_in(sweep0, n_sweeps, accumulate_from, every):
    """Number of sweeps s in [sweep0, sweep0 + n_sweeps) with s >= accumulate_from and (s - accumulate_from) % every == 0."""
    end = sweep0 + n_sweeps
    first = max(sweep0, accumulate_from)
    first = accumulate_from + -(-(first - accumulate_from) // every) * every
    return 0 if first >= end else (end - first + every - 1) // every


def shard_chains(total_chains, world_size, rank):
    """Contiguous split of global chain ids: returns (chain0, n_local).  Earlier ranks take the remainder."""
    base, rem = divmod(int(total_chains), int(world_size))
    n_local = base + (1 if rank < rem else 0)
    chain0 = rank * base + min(rank, rem)
    return chain0, n_local


def allreduce_counts(counts, group=None):
    """Sum the pooled sufficient statistics over ranks (RCCL on GPUs, gloo on CPU); no-op for one process."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    return counts


def pool_u32(t):
    """
    The sampler's tallies are uint32 held in int32 tensors (torch has no uint32 arithmetic): their values as int64, summed
    over ranks.  Every host read of such a tally that pools goes through here.
    """
    import torch
    return allreduce_counts(t.to(torch.int64) & 0xFFFFFFFF)


def mstep_from_counts(counts, Nreg, U):
    """Host restatement of fcd_gibbs_mstep (used to report pi/gamma; the device keeps its own copy)."""
    counts = [int(x) for x in counts]
    G = counts[4]
    n_r = float(G * Nreg * U)
    pi = min(max(counts[0] / n_r, 0.5 / n_r), 1.0 - 0.5 / n_r)
    n_f = float(G * util.N_to_C(Nreg))
    gamma = np.array([max(counts[1 + k] / n_f, 0.5 / n_f) for k in range(3)])
    return pi, gamma


class GibbsEngine(object):
    """
    Device-resident state of G chains and the kernels that move it.

    S_B (C,3) and lM (C,U,3,3) are float64 CUDA tensors produced by `tables.build` (fcd_lik_tables_ex, or
    fcd_lik_shared_tables at U = 1); they are shared by all chains.  State layout (include/fcdiff_hip.h):
    f_state (GW, C, 64) uint8, r_bits (GW, Nreg, U) uint64 bit planes (held in an int64 tensor), GW = ceil(G / 64).
    """

    def __init__(self, S_B, lM, Nreg, U, n_chains, chain0=0, seed=0, edge_index="symmetric", ctx=None,
                 region_major=True):
        """region_major=False keeps only lM: the generic f / r kernels run (any shape, several times slower)."""
        import torch
        self.torch = torch
        self.ctx = ctx if ctx is not None else _lib.Context()
        self.Nreg, self.U, self.G = int(Nreg), int(U), int(n_chains)
        self.C = util.N_to_C(self.Nreg)
        self.GW = (self.G + 63) // 64
        self.chain0, self.seed = int(chain0), int(seed)
        self.edge_mode = _lib.EDGE_MODES[edge_index]
        if tuple(lM.shape) != (self.C, self.U, 3, 3) or tuple(S_B.shape) != (self.C, 3):
            raise ValueError("tables do not match Nreg=%d, U=%d" % (self.Nreg, self.U))
        self.S_B, self.lM = S_B.contiguous(), lM.contiguous()
        dev = self.S_B.device
        self.hyper = torch.zeros(8, dtype=torch.float64, device=dev)
        self.f_state = torch.zeros((self.GW, self.C, 64), dtype=torch.uint8, device=dev)
        self.r_bits = torch.zeros((self.GW, self.Nreg, self.U), dtype=torch.int64, device=dev)
        self.counts = torch.zeros(8, dtype=torch.int64, device=dev)
        self.cnt_f = torch.zeros((self.C, 3), dtype=torch.int32, device=dev)
        self.cnt_r = torch.zeros((self.Nreg, self.U), dtype=torch.int32, device=dev)
        self.n_accumulated = 0
        for a in ACCUMULATORS:      # a.attr: the buffers run() adds to (None until attach_<key>_accumulator()), period, sweeps so far
            self._detach(a)
            setattr(self, a.key + "_every", 1)
        self.region_names = None    # the sets of set_region_sets(): names, CSR offsets and members, their number, the largest
        self.region_offsets = self.region_members = None
        self.region_J = self.region_smax = 0
        self.group_names = None     # the groups of set_patient_groups(): names, CSR offsets and members, contrasts (P, 2) and
        self.group_offsets = self.group_members = self.group_contrasts = None      # the bin offsets of their joint histograms
        self.group_bin_offsets = None
        self.group_J = self.group_umax = 0
        self.group_with_sets = False        # the rows of patient_group_acc include the region sets it was attached with
        self.trait_names = None     # the traits of set_patient_traits(): names, scores (Q, U) int32, known (Q, U) bool, n_known (Q,)
        self.trait_scores = self.trait_known = self.trait_n_known = None
        self.trait_Q = self.trait_umax = 0
        self.trait_with_sets = False        # the rows of patient_trait_acc include the region sets it was attached with
        self.ctx.call("fcd_ctx_reserve", self.Nreg, self.U, self.G)
        self.lMd = self.lMf = None
        if region_major:
            self.lMd = torch.empty((self.U, self.Nreg, self.Nreg, 3, 2), dtype=torch.float64, device=dev)
            self.lMf = torch.empty((self.C, self.U, 3, 2), dtype=torch.float64, device=dev)
            self.refresh_tables()

    def refresh_tables(self):
        """Re-derive the two difference tables after lM changed (a table build = a theta_sub change)."""
        if self.lMd is not None:
            self.ctx.call("fcd_gibbs_region_tables", _lib.dptr(self.lM), self.Nreg, self.U, self.edge_mode,
                          _lib.dptr(self.lMd), _lib.stream_ptr())
            self.ctx.call("fcd_gibbs_edge_tables", _lib.dptr(self.lM), self.Nreg, self.U, _lib.dptr(self.lMf),
                          _lib.stream_ptr())

    # ---- hyper-parameters ----
    def set_hyper(self, gamma, pi2):
        tables.write_hyper(self.ctx, self.hyper, gamma, pi2)

    def hyper_values(self):
        h = self.hyper.cpu().numpy()
        self.ctx.check_device()
        return np.exp(h[0:3]), float(np.exp(h[4]))

    def host(self, t):
        """Device tensor -> NumPy array; raises if a sweep before it abandoned a device-side wait (fcd_ctx_check)."""
        a = t.cpu().numpy()
        self.ctx.check_device()
        return a

    # ---- state ----
    def init(self, pi):
        self.ctx.call("fcd_gibbs_init", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      self.chain0, C.c_uint64(self.seed), float(pi), _lib.stream_ptr())

    def export_state(self):
        t = self.torch
        f = t.empty((self.G, self.C), dtype=t.uint8, device=self.f_state.device)
        r = t.empty((self.G, self.Nreg, self.U), dtype=t.uint8, device=self.f_state.device)
        self.ctx.call("fcd_gibbs_export_state", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U,
                      self.G, _lib.dptr(f), _lib.dptr(r), _lib.stream_ptr())
        (fh, rh) = (f.cpu().numpy(), r.cpu().numpy())
        self.ctx.check_device()          # (the copies above waited for every sweep before them)
        return fh, rh

    def import_state(self, f, r):
        t = self.torch
        f = np.ascontiguousarray(f, dtype=np.uint8)
        r = np.ascontiguousarray(r, dtype=np.uint8)
        if f.shape != (self.G, self.C) or r.shape != (self.G, self.Nreg, self.U):
            raise ValueError("state shapes must be (G, C) and (G, Nreg, U)")
        if (f > 2).any():
            raise ValueError("f values must be 0, 1 or 2")
        f = t.as_tensor(f, device=self.f_state.device)
        r = t.as_tensor(r, device=self.f_state.device)
        self.ctx.call("fcd_gibbs_import_state", _lib.dptr(f), _lib.dptr(r), self.Nreg, self.U, self.G,
                      _lib.dptr(self.f_state), _lib.dptr(self.r_bits), _lib.stream_ptr())

    # ---- moves ----
    def f_step(self, sweep):
        self.ctx.call("fcd_gibbs_f_step", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.lMf), _lib.dptr(self.hyper),
                      _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, self.chain0,
                      C.c_uint64(self.seed), int(sweep), _lib.stream_ptr())

    def r_step(self, sweep):
        self.ctx.call("fcd_gibbs_r_step", _lib.dptr(self.lM), _lib.dptr(self.lMd), _lib.dptr(self.hyper),
                      _lib.dptr(self.f_state),
                      _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, self.chain0, C.c_uint64(self.seed),
                      int(sweep), self.edge_mode, _lib.stream_ptr())

    def sweeps(self, sweep0, n_sweeps, with_counts=False):
        self.ctx.call("fcd_gibbs_sweeps", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.lMf), _lib.dptr(self.lMd),
                      _lib.dptr(self.hyper),
                      _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, self.chain0,
                      C.c_uint64(self.seed), int(sweep0), int(n_sweeps), self.edge_mode,
                      _lib.dptr(self.counts if with_counts else None), _lib.stream_ptr())
        return self.counts if with_counts else None

    def run(self, sweep0, n_sweeps, mstep_every=0, accumulate_from=None, want_counts=False):
        """
        n_sweeps x (f pass, r pass, tally) in one call (fcd_gibbs_run): the tally of each sweep feeds the marginal
        counters from sweep `accumulate_from` on (None: never), runs the (pi, gamma) M-step on this rank's pooled counts
        every `mstep_every` sweeps (0: never -- several ranks all-reduce the returned counts and call mstep()), and
        packs the r words of the next f pass.  Returns the counts tensor of the last sweep (or None).
        The same call also adds to every attached accumulator of ACCUMULATORS (attach_<key>_accumulator) at every
        <key>_every-th sweep from `accumulate_from` on; a call that could overflow a counter of one raises ValueError.
        """
        acc = accumulate_from is not None
        live = []                   # (accumulator, sweeps this call adds to it), attached ones only
        # (in the table's order, and nothing more of an accumulator is read unless it is attached)
        for a in ACCUMULATORS:
            if not acc or getattr(self, a.attr) is None:
                continue
            n = pair_sweeps_in(int(sweep0), int(n_sweeps), int(accumulate_from), getattr(self, a.key + "_every"))
            total = getattr(self, a.key + "_sweeps") + n
            sites = a.sites(self.Nreg, self.U) if a.sites else 1
            if total * self.G * sites > PAIR_COUNT_MAX:
                raise ValueError("the %s accumulator would overflow uint32: %d chains x %s%d accumulated sweeps > %d"
                                 % (a.label, self.G, "%d sites x " % sites if a.sites else "", total, PAIR_COUNT_MAX))
            live.append((a, n))
        # (attached for this call only: the context is shared, no other engine's sweeps may add to these buffers)
        try:
            for (a, _n) in live:
                if a.send:
                    getattr(self, a.send)()
                self.ctx.call(a.setter, *([_lib.dptr(b) for b in self._acc_buffers(a)]
                                          + [self.Nreg, self.U, getattr(self, a.key + "_every")]))
            self._run(sweep0, n_sweeps, mstep_every, accumulate_from, want_counts)
        finally:
            for (a, _n) in live:
                self.ctx.call(a.setter, *([None] * (2 if a.paired else 1) + [0, 0, 1]))
        for (a, n) in live:
            setattr(self, a.key + "_sweeps", getattr(self, a.key + "_sweeps") + n)
        if acc:
            self.n_accumulated += max(0, int(sweep0) + int(n_sweeps) - max(int(accumulate_from), int(sweep0)))
        return self.counts if want_counts else None

    def _run(self, sweep0, n_sweeps, mstep_every, accumulate_from, want_counts):
        acc = accumulate_from is not None
        self.ctx.call("fcd_gibbs_run", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.lMf), _lib.dptr(self.lMd),
                      _lib.dptr(self.hyper), _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      self.chain0, C.c_uint64(self.seed), int(sweep0), int(n_sweeps), self.edge_mode, int(mstep_every),
                      int(accumulate_from) if acc else 0, _lib.dptr(self.counts if want_counts else None),
                      _lib.dptr(self.cnt_f if acc else None), _lib.dptr(self.cnt_r if acc else None), _lib.stream_ptr())

    # ---- the accumulators of run(): one implementation for the rows of ACCUMULATORS ----
    def _acc_buffers(self, a):
        bufs = getattr(self, a.attr)
        return bufs if a.paired else (bufs,)

    def _attach(self, a, every):
        every = int(every)
        if every < 1:
            raise ValueError("every must be >= 1")
        t = self.torch
        # (uint32 on the device is held in int32 tensors like cnt_f; _acc_host() reads those back as uint32)
        bufs = tuple(t.zeros(shape, dtype=getattr(t, dtype), device=self.f_state.device)
                     for (shape, dtype) in zip(a.shapes(self), a.dtypes))
        setattr(self, a.attr, bufs if a.paired else bufs[0])
        setattr(self, a.key + "_every", every)
        setattr(self, a.key + "_sweeps", 0)
        return getattr(self, a.attr)

    def _detach(self, a):
        setattr(self, a.attr, None)
        setattr(self, a.key + "_sweeps", 0)

    def _acc_host(self, a):
        if getattr(self, a.attr) is None:
            raise ValueError("no %s accumulator is attached" % a.label)
        out = tuple(self.host(b).view(np.uint32) if dtype == "int32" else self.host(b)
                    for (b, dtype) in zip(self._acc_buffers(a), a.dtypes))
        return out if a.paired else out[0]

    # ---- what the patient-group and patient-trait accumulators (`what`: "group", "trait") share: rows, and the context ----
    def _rows(self, a, what):
        """R: the regions and, while an attached accumulator has them or else if region sets are set, the region sets after them."""
        with_sets = getattr(self, what + "_with_sets") if getattr(self, a.attr) is not None else bool(self.region_J)
        return self.Nreg + (self.region_J if with_sets else 0)

    def _row_names(self, R):
        """The names of R rows: the region indices as str, then "set:<name>" for the region sets."""
        return [str(n) for n in range(self.Nreg)] + ["set:" + s for s in (self.region_names or [])[:R - self.Nreg]]

    def _send_rows(self, what, R, setter, *args):
        """
        As _send_region_sets(), for the groups or traits (`what`) of this engine: the shared context holds them (and, where
        the R rows include them, this engine's region sets) before a launch.
        """
        with_sets = R > self.Nreg
        if with_sets:
            self._send_region_sets()
        owner = getattr(self.ctx, "patient_%ss_owner" % what, None)
        if owner is not None and owner[0]() is self and owner[1] == with_sets:
            return
        self.ctx.call(setter, *(args + (1 if with_sets else 0,)))
        setattr(self.ctx, "patient_%ss_owner" % what, (weakref.ref(self), with_sets))

    # ---- (f_c, mixture case) counts for the connection posteriors ----
    def attach_pair_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep counts of (f_c = k, mixture case l at (c,u)) to `pair_acc` (C, U, 3, 3),
        at every `every`-th sweep from its `accumulate_from` on (none when accumulate_from is None).  Zeroes the counts.
        """
        return self._attach(_PAIR, every)

    def detach_pair_accumulator(self):
        self._detach(_PAIR)

    def pair_counts_host(self):
        """The attached accumulator as a NumPy uint32 array (C, U, 3, 3)."""
        return self._acc_host(_PAIR)

    def pair_tally(self, acc):
        """acc (C, U, 3, 3) uint32-in-int32 tensor += the (f_c, mixture case) counts of the current state."""
        self.ctx.call("fcd_gibbs_pair_tally", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      _lib.dptr(acc), _lib.stream_ptr())
        return acc

    # ---- histograms of the anomalous-region counts ----
    def attach_count_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep histograms of sum_n r_nu (hist_patient (U, Nreg+1)) and sum_u r_nu
        (hist_region (Nreg, U+1)) over chains to `count_hist`, at every `every`-th sweep from its `accumulate_from` on
        (none when accumulate_from is None).  Zeroes the histograms.
        """
        return self._attach(_COUNT, every)

    def detach_count_accumulator(self):
        self._detach(_COUNT)

    def count_hist_host(self):
        """The attached histograms as NumPy uint32 arrays (hist_patient (U, Nreg+1), hist_region (Nreg, U+1))."""
        return self._acc_host(_COUNT)

    def count_tally(self, hist_patient, hist_region):
        """hist_patient (U, Nreg+1), hist_region (Nreg, U+1) uint32-in-int32 tensors += the histograms of the current state."""
        if (tuple(hist_patient.shape) != (self.U, self.Nreg + 1) or tuple(hist_region.shape) != (self.Nreg, self.U + 1)
                or hist_patient.element_size() != 4 or hist_region.element_size() != 4
                or not hist_patient.is_contiguous() or not hist_region.is_contiguous()):
            raise ValueError("histograms must be contiguous 32-bit (U, Nreg+1) and (Nreg, U+1)")
        self.ctx.call("fcd_gibbs_count_tally", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(hist_patient),
                      _lib.dptr(hist_region), _lib.stream_ptr())
        return hist_patient, hist_region

    # ---- counts over sets of regions (networks): how many regions of a set, in how many patients a set is hit ----
    def set_region_sets(self, sets):
        """
        The region sets of this engine's histograms, in any form region_sets_csr() takes; None clears.  They are copied to
        the context (fcd_region_sets_set).  ValueError while the accumulator is attached: its buffers have the old shapes.
        """
        if self.region_set_acc is not None:
            raise ValueError("detach the region-set accumulator before changing the sets")
        if self.patient_group_acc is not None:
            raise ValueError("detach the patient-group accumulator before changing the sets: they may be rows of it")
        if self.patient_trait_acc is not None:
            raise ValueError("detach the patient-trait accumulator before changing the sets: they may be rows of it")
        if sets is None:
            (self.region_names, self.region_offsets, self.region_members) = (None, None, None)
            (self.region_J, self.region_smax) = (0, 0)
            self.ctx.call("fcd_region_sets_set", None, None, 0)
            self.ctx.region_sets_owner = None
            return
        (self.region_names, self.region_offsets, self.region_members) = region_sets_csr(sets, self.Nreg)
        self.region_J = len(self.region_names)
        self.region_smax = int(np.diff(self.region_offsets).max())
        self.ctx.region_sets_owner = None
        self._send_region_sets()

    def _send_region_sets(self):
        """The context is shared: make sure ITS sets are this engine's before a launch that writes this engine's buffers."""
        owner = getattr(self.ctx, "region_sets_owner", None)        # (a weak reference: the context does not keep an engine alive)
        if owner is not None and owner() is self:
            return
        if not self.region_J:
            raise ValueError("no region sets: call set_region_sets() first")
        self.ctx.call("fcd_region_sets_set", self.region_offsets.ctypes.data_as(C.c_void_p),
                      self.region_members.ctypes.data_as(C.c_void_p), self.region_J)
        self.ctx.region_sets_owner = weakref.ref(self)

    def attach_region_set_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep histograms over the sets of set_region_sets() to `region_set_acc`: hist_set
        (J, U, S_max+1), over chains, of sum_{n in S_j} r_nu (bins beyond a set's size stay 0) and hist_prev (J, U+1) of the
        number of patients with an anomalous region in S_j, at every `every`-th sweep from its `accumulate_from` on (none
        when accumulate_from is None).  Zeroes the histograms.
        """
        if not self.region_J:
            raise ValueError("no region sets: call set_region_sets() first")
        if self.U > COUNT_MAX_U:
            raise ValueError("region-set histograms are made for at most %d patients (here %d)" % (COUNT_MAX_U, self.U))
        return self._attach(_REGION_SET, every)

    def detach_region_set_accumulator(self):
        self._detach(_REGION_SET)

    def region_set_host(self):
        """The attached histograms as NumPy uint32 arrays (hist_set (J, U, S_max+1), hist_prev (J, U+1))."""
        return self._acc_host(_REGION_SET)

    def region_set_tally(self, hist_set, hist_prev):
        """hist_set (J, U, S_max+1), hist_prev (J, U+1) uint32-in-int32 tensors += the histograms of the current state."""
        if not self.region_J:
            raise ValueError("no region sets: call set_region_sets() first")
        if (tuple(hist_set.shape) != (self.region_J, self.U, self.region_smax + 1)
                or tuple(hist_prev.shape) != (self.region_J, self.U + 1)
                or hist_set.element_size() != 4 or hist_prev.element_size() != 4
                or not hist_set.is_contiguous() or not hist_prev.is_contiguous()):
            raise ValueError("histograms must be contiguous 32-bit (J, U, S_max+1) and (J, U+1)")
        self._send_region_sets()
        self.ctx.call("fcd_gibbs_region_set_tally", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(hist_set),
                      _lib.dptr(hist_prev), _lib.stream_ptr())
        return hist_set, hist_prev

    # ---- counts over groups of patients and contrasts between two groups ----
    def set_patient_groups(self, groups, contrasts=None):
        """
        The patient groups of this engine's histograms, in any form patient_groups_csr() takes, and the contrasts between
        them (pairs of names or indices of disjoint groups; patient_group_contrasts()); groups=None clears.  They are copied
        to the context (fcd_patient_groups_set).  ValueError while the accumulator is attached: its buffers have the old shapes.
        """
        if self.patient_group_acc is not None:
            raise ValueError("detach the patient-group accumulator before changing the groups")
        self.ctx.patient_groups_owner = None
        if groups is None:
            if contrasts is not None:
                raise ValueError("contrasts without patient groups")
            (self.group_names, self.group_offsets, self.group_members) = (None, None, None)
            (self.group_contrasts, self.group_bin_offsets) = (None, None)
            (self.group_J, self.group_umax) = (0, 0)
            self.ctx.call("fcd_patient_groups_set", None, None, 0, None, 0, 0)
            return
        (names, offsets, members) = patient_groups_csr(groups, self.U)
        (pairs, bin_offsets) = patient_group_contrasts(contrasts, names, offsets, members)
        (self.group_names, self.group_offsets, self.group_members) = (names, offsets, members)
        (self.group_contrasts, self.group_bin_offsets) = (pairs, bin_offsets)
        self.group_J = len(names)
        self.group_umax = int(np.diff(offsets).max())
        self._send_patient_groups()

    def patient_group_rows(self):
        """R: the regions and, while an attached accumulator has them or else if region sets are set, the region sets after them."""
        return self._rows(_PATIENT_GROUP, "group")

    def patient_group_row_names(self):
        """The names of the R rows: the region indices as str, then "set:<name>" for the region sets."""
        return self._row_names(self.patient_group_rows())

    def _send_patient_groups(self):
        if not self.group_J:
            raise ValueError("no patient groups: call set_patient_groups() first")
        self._send_rows("group", self.patient_group_rows(), "fcd_patient_groups_set",
                        self.group_offsets.ctypes.data_as(C.c_void_p), self.group_members.ctypes.data_as(C.c_void_p), self.group_J,
                        self.group_contrasts.ctypes.data_as(C.c_void_p) if len(self.group_contrasts) else None,
                        len(self.group_contrasts))

    def attach_patient_group_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep histograms over the groups of set_patient_groups() to `patient_group_acc`:
        hist_group (J, R, Umax+1), over chains, of the number of patients of g_j anomalous at row rho (bins beyond a group's
        size stay 0) and hist_joint, flat: block p of contrast (a, b) is (R, |a|+1, |b|+1), the joint histogram of (k_a, k_b),
        and starts at R * group_bin_offsets[p] (one placeholder word without contrasts).  The rows are the regions and, if
        region sets are set NOW, the sets after them; at every `every`-th sweep from its `accumulate_from` on (none when
        accumulate_from is None).  Zeroes the histograms.
        """
        if not self.group_J:
            raise ValueError("no patient groups: call set_patient_groups() first")
        self.patient_group_acc = None
        self.group_with_sets = bool(self.region_J)
        return self._attach(_PATIENT_GROUP, every)

    def detach_patient_group_accumulator(self):
        self._detach(_PATIENT_GROUP)

    def patient_group_host(self):
        """The attached histograms as NumPy uint32 arrays (hist_group (J, R, Umax+1), hist_joint flat)."""
        return self._acc_host(_PATIENT_GROUP)

    def patient_group_tally(self, hist_group, hist_joint):
        """hist_group (J, R, Umax+1), hist_joint (max(1, R * bins of all contrasts),) uint32-in-int32 tensors += the histograms of the current state."""
        if not self.group_J:
            raise ValueError("no patient groups: call set_patient_groups() first")
        R = self.patient_group_rows()
        if (tuple(hist_group.shape) != (self.group_J, R, self.group_umax + 1)
                or hist_joint.numel() != max(1, R * int(self.group_bin_offsets[-1]))
                or hist_group.element_size() != 4 or hist_joint.element_size() != 4
                or not hist_group.is_contiguous() or not hist_joint.is_contiguous()):
            raise ValueError("histograms must be contiguous 32-bit (J, R, Umax+1) and R x the joint bins of all contrasts")
        self._send_patient_groups()
        self.ctx.call("fcd_gibbs_patient_group_tally", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(hist_group),
                      _lib.dptr(hist_joint), _lib.stream_ptr())
        return hist_group, hist_joint

    # ---- rank-sum (AUC) statistics between the anomalous and the other patients of a row, per patient trait ----
    def set_patient_traits(self, traits):
        """
        The patient traits of this engine's rank-sum histograms, in any form patient_traits_scores() takes; None clears.  They
        are copied to the context (fcd_patient_traits_set).  ValueError while the accumulator is attached: its buffers have the
        old shapes.
        """
        if self.patient_trait_acc is not None:
            raise ValueError("detach the patient-trait accumulator before changing the traits")
        self.ctx.patient_traits_owner = None
        if traits is None:
            (self.trait_names, self.trait_scores, self.trait_known, self.trait_n_known) = (None, None, None, None)
            (self.trait_Q, self.trait_umax) = (0, 0)
            self.ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)
            return
        (names, scores, known, n_known) = patient_traits_scores(traits, self.U)
        (self.trait_names, self.trait_n_known) = (names, n_known)
        (self.trait_scores, self.trait_known) = (np.ascontiguousarray(scores), np.ascontiguousarray(known.astype(np.uint8)))
        self.trait_Q = len(names)
        self.trait_umax = int(n_known.max())
        self._send_patient_traits()

    def patient_trait_rows(self):
        """R: the regions and, while an attached accumulator has them or else if region sets are set, the region sets after them."""
        return self._rows(_PATIENT_TRAIT, "trait")

    def patient_trait_row_names(self):
        """The names of the R rows: the region indices as str, then "set:<name>" for the region sets."""
        return self._row_names(self.patient_trait_rows())

    def _send_patient_traits(self):
        if not self.trait_Q:
            raise ValueError("no patient traits: call set_patient_traits() first")
        self._send_rows("trait", self.patient_trait_rows(), "fcd_patient_traits_set",
                        self.trait_scores.ctypes.data_as(C.c_void_p), self.trait_known.ctypes.data_as(C.c_void_p), self.trait_Q, self.U)

    def attach_patient_trait_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep rank-sum statistics of the traits of set_patient_traits() to `patient_trait_acc`,
        with k the number of known patients of trait q anomalous at row rho and A the sum of their scores (Umax = the largest
        n_q, NB = 128): trait_hist (Q, R, Umax+1 + NB + 3) uint32 -- [0 .. n_q] the histogram of k over chains,
        [Umax+1 .. Umax+NB] the AUC bins min(NB-1, floor(NB (A + d) / (2 d))), d = k (n_q - k), of the states with 0 < k < n_q,
        the last three words those states with A < 0, = 0, > 0 -- and trait_sum (Q, R, Umax+1) int64, [k] the sum of A over the
        states with that k.  The rows are the regions and, if region sets are set NOW, the sets after them; at every `every`-th
        sweep from its `accumulate_from` on (none when accumulate_from is None).  Zeroes both.
        """
        if not self.trait_Q:
            raise ValueError("no patient traits: call set_patient_traits() first")
        self.patient_trait_acc = None
        self.trait_with_sets = bool(self.region_J)
        return self._attach(_PATIENT_TRAIT, every)

    def detach_patient_trait_accumulator(self):
        self._detach(_PATIENT_TRAIT)

    def patient_trait_host(self):
        """The attached buffers as NumPy arrays (trait_hist (Q, R, Umax+1+NB+3) uint32, trait_sum (Q, R, Umax+1) int64)."""
        return self._acc_host(_PATIENT_TRAIT)

    def patient_trait_tally(self, trait_hist, trait_sum):
        """trait_hist (Q, R, Umax+1+NB+3) uint32-in-int32, trait_sum (Q, R, Umax+1) int64 tensors += the statistics of the current state."""
        if not self.trait_Q:
            raise ValueError("no patient traits: call set_patient_traits() first")
        R = self.patient_trait_rows()
        if (tuple(trait_hist.shape) != (self.trait_Q, R, self.trait_umax + 1 + PATIENT_TRAIT_BINS + 3)
                or tuple(trait_sum.shape) != (self.trait_Q, R, self.trait_umax + 1)
                or trait_hist.element_size() != 4 or trait_sum.dtype != self.torch.int64
                or not trait_hist.is_contiguous() or not trait_sum.is_contiguous()):
            raise ValueError("buffers must be contiguous 32-bit (Q, R, Umax+1+%d+3) and int64 (Q, R, Umax+1)" % PATIENT_TRAIT_BINS)
        self._send_patient_traits()
        self.ctx.call("fcd_gibbs_patient_trait_tally", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(trait_hist),
                      _lib.dptr(trait_sum), _lib.stream_ptr())
        return trait_hist, trait_sum

    # ---- co-anomaly: pairs of regions anomalous together, pairs of patients sharing anomalous regions ----
    def attach_coanomaly_accumulator(self, every=1):
        """
        From now on run() adds the end-of-sweep counts region_pairs[n, m] = #{(chain, u): r_nu = r_mu = 1} (Nreg, Nreg) and
        patient_pairs[u, v] = #{(chain, n): r_nu = r_nv = 1} (U, U) to `coanomaly_acc`, at every `every`-th sweep from its
        `accumulate_from` on (none when accumulate_from is None).  Zeroes the matrices.
        """
        return self._attach(_COANOMALY, every)

    def detach_coanomaly_accumulator(self):
        self._detach(_COANOMALY)

    def coanomaly_host(self):
        """The attached matrices as NumPy uint32 arrays (region_pairs (Nreg, Nreg), patient_pairs (U, U))."""
        return self._acc_host(_COANOMALY)

    def coanomaly_tally(self, region, patient):
        """region (Nreg, Nreg), patient (U, U) uint32-in-int32 tensors += the pair counts of the current state."""
        if (tuple(region.shape) != (self.Nreg, self.Nreg) or tuple(patient.shape) != (self.U, self.U)
                or region.element_size() != 4 or patient.element_size() != 4
                or not region.is_contiguous() or not patient.is_contiguous()):
            raise ValueError("pair matrices must be contiguous 32-bit (Nreg, Nreg) and (U, U)")
        self.ctx.call("fcd_gibbs_coanomaly_tally", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(region),
                      _lib.dptr(patient), _lib.stream_ptr())
        return region, patient

    # ---- pooled statistics / M-step ----
    def stats(self):
        self.ctx.call("fcd_gibbs_stats", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      _lib.dptr(self.counts), _lib.stream_ptr())
        return self.counts

    def mstep(self, counts):
        self.ctx.call("fcd_gibbs_mstep", _lib.dptr(counts), self.Nreg, self.U, _lib.dptr(self.hyper), _lib.stream_ptr())

    def accumulate(self):
        self.ctx.call("fcd_gibbs_accumulate", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U,
                      self.G, _lib.dptr(self.cnt_f), _lib.dptr(self.cnt_r), _lib.stream_ptr())
        self.n_accumulated += 1

    def tally(self, want_counts=True, accumulate=True):
        """stats() and accumulate() in one pass over the state; returns the counts tensor (or None)."""
        self.ctx.call("fcd_gibbs_tally", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      _lib.dptr(self.counts if want_counts else None), _lib.dptr(self.cnt_f if accumulate else None),
                      _lib.dptr(self.cnt_r if accumulate else None), _lib.stream_ptr())
        if accumulate:
            self.n_accumulated += 1
        return self.counts if want_counts else None

    def pair_counts(self, out=None, accumulate=False):
        """(C, U, 3, 3) float64: number of this rank's chains with f_c = k and mixture case l at (c, u)."""
        t = self.torch
        if out is None:
            out = t.empty((self.C, self.U, 3, 3), dtype=t.float64, device=self.f_state.device)
            accumulate = False
        self.ctx.call("fcd_gibbs_pair_counts", _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G,
                      1 if accumulate else 0, _lib.dptr(out), _lib.stream_ptr())
        return out

    # ---- diagnostics ----
    def logjoint(self):
        out = self.torch.empty(self.G, dtype=self.torch.float64, device=self.f_state.device)
        self.ctx.call("fcd_gibbs_logjoint", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.hyper),
                      _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(out),
                      _lib.stream_ptr())
        return out

    def r_sums(self):
        """(G,) int32: number of anomalous (region, patient) sites of each chain (fcd_gibbs_chain_rsum)."""
        out = self.torch.empty(self.G, dtype=self.torch.int32, device=self.f_state.device)
        self.ctx.call("fcd_gibbs_chain_rsum", _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, _lib.dptr(out),
                      _lib.stream_ptr())
        return out

    def conditionals(self, want_f=True, want_r=True):
        t = self.torch
        dev = self.f_state.device
        cf = t.empty((self.G, self.C, 3), dtype=t.float64, device=dev) if want_f else None
        cr = t.empty((self.G, self.Nreg, self.U, 2), dtype=t.float64, device=dev) if want_r else None
        self.ctx.call("fcd_gibbs_conditionals", _lib.dptr(self.S_B), _lib.dptr(self.lM), _lib.dptr(self.hyper),
                      _lib.dptr(self.f_state), _lib.dptr(self.r_bits), self.Nreg, self.U, self.G, self.edge_mode,
                      _lib.dptr(cf), _lib.dptr(cr), _lib.stream_ptr())
        return cf, cr


def _world_size(group=None):
    import torch.distributed as dist
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def run_chains(engine, n_sweeps, sweep0=0, mstep_every=1, burn_in=0, update_theta=True, group=None,
               on_sweep=None, mstep_lag=0, force_collective=False, direct=True):
    """
    The sampler loop shared by UnsharedRegionFit(method='gibbs') and bench.py.

    Every sweep: f pass, r pass, one tally launch (marginal counters after `burn_in` sweeps, the packed r words of the
    next f pass).  Every `mstep_every` sweeps the pooled counts give the (pi, gamma) M-step:
      * one rank, mstep_lag=0: inside the tally launch (fcd_gibbs_run), the whole loop is ONE call;
      * several ranks, mstep_lag=0: counts -> blocking all-reduce (RCCL) -> fcd_gibbs_mstep, between two calls;
      * mstep_lag=1: the M-step from the counts of period j (mstep_every sweeps) is applied after period j+1 (it
        shapes period j+2), so the all-reduce of period j runs on the collective's stream WHILE period j+1 computes.
        The schedule -- and with it every chain's path -- is the same for any number of ranks, one rank included.
    `engine` is anything with run/mstep (the HIP engine here; the CPU tests pass an oracle-backed stand-in to
    exercise the multi-process logic under gloo).
    direct=True (default; HIP engine, mstep_lag=0): several ranks pool their counts through the context's own RCCL
    communicator INSIDE fcd_gibbs_run (Context.attach_comm); direct=False keeps round 3's loop through torch.distributed.
    force_collective=True takes the several-rank path -- counts, all-reduce, fcd_gibbs_mstep between calls -- also in a
    process group of ONE rank (bench.py --force-pg, tests/test_dist_nccl.py: RCCL initialised and used on a one-GPU box;
    the chains are those of the plain loop, bit for bit).
    """
    import torch.distributed as dist
    world = _world_size(group)
    collective = world > 1 or (bool(force_collective) and dist.is_available() and dist.is_initialized())
    k = int(mstep_every) if (update_theta and mstep_every and mstep_every > 0) else 0
    acc_from = sweep0 + burn_in
    if collective and direct and not mstep_lag and hasattr(engine, "ctx") and hasattr(engine.ctx, "attach_comm"):
        # Round 4: the all-reduce of the pooled counts is RCCL called by the library itself on the stream of the sweep
        # kernels (fcd_comm_*): the several-rank loop is then the one-rank loop -- ONE fcd_gibbs_run call per chunk, the
        # tally, the all-reduce, the M-step kernel and the next f pass queued behind one another.
        # (the path has only ever run on ONE rank -- the build box has one GPU -- so it is taken only if EVERY rank could make
        # its communicator: one all-reduce of a flag through the torch group decides, all ranks alike; else round 3's loop)
        import torch
        decided = getattr(engine, "_direct_comm", None)            # (the agreement is made once per engine, not once per call)
        if decided is not None:
            collective = not decided
        ok = 1
        try:
            if decided is None:
                engine.ctx.attach_comm(group)
        except Exception as exc:      # noqa: BLE001
            import warnings
            warnings.warn("fcdiff_amd: the library's own RCCL communicator could not be made (%s); pooling the counts through "
                          "torch.distributed instead" % (exc,))
            ok = 0
        if decided is None:
            flag = torch.tensor([ok], dtype=torch.int32, device=engine.ctx.device if dist.get_backend(group) == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            engine._direct_comm = int(flag.item()) == 1
            if engine._direct_comm:
                collective = False
            else:
                engine.ctx.detach_comm()
    if not collective and on_sweep is None and not mstep_lag:
        engine.run(sweep0, n_sweeps, mstep_every=k, accumulate_from=acc_from)
        return
    pending = None       # (counts clone, work handle or None): the M-step that waits for its turn (mstep_lag)

    def apply(p):
        (cl, work) = p
        if work is not None:
            work.wait()          # the compute stream waits for the collective; the host does not (RCCL)
        engine.mstep(cl)
    i = 0
    while i < n_sweeps:
        c = n_sweeps - i
        if on_sweep is not None:
            c = 1
        if k:
            c = min(c, k - (i % k))
        end = i + c
        do_m = bool(k and end % k == 0)
        local = do_m and not collective and not mstep_lag
        counts = engine.run(sweep0 + i, c, mstep_every=(c if local else 0), accumulate_from=acc_from,
                            want_counts=do_m and not local)
        if mstep_lag and pending is not None and do_m:      # one M-step PERIOD later, whatever the chunking
            apply(pending)
            pending = None
        if do_m and not local:
            if mstep_lag:
                cl = counts.clone()
                work = dist.all_reduce(cl, op=dist.ReduceOp.SUM, group=group, async_op=True) if collective else None
                pending = (cl, work)
            else:
                if collective:
                    dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
                engine.mstep(counts)
        if on_sweep is not None:
            on_sweep(i, engine)
        i = end
    if pending is not None:
        apply(pending)
