"""
Stand-ins for GibbsEngine.run() without a library or a GPU: an engine made with __new__ that holds only the state run() and
the _send_* methods read, on a context that records its calls.  Shared by the accumulator tests of tests/test_fit_helpers.py,
test_region_sets.py, test_patient_groups.py and test_patient_traits.py.
"""
import numpy as np

from fcdiff_amd import gibbs


class Recorder(object):
    """A context that keeps (entry point, its last three arguments) of every call."""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args[-3:]))


def one_word_buffers(a):
    """Buffers of row `a` as run() wants to find them attached: one word each, of the row's dtypes."""
    import torch
    bufs = tuple(torch.zeros(1, dtype=getattr(torch, dtype)) for dtype in a.dtypes)
    return bufs if a.paired else bufs[0]


def stand_in_engine(G, N, U, attached=(), sets=None, groups=None, contrasts=None, traits=None):
    """
    G chains of N regions and U patients with the rows of `attached` (keys of gibbs.ACCUMULATORS) attached at period 1 with
    no sweeps behind them, every other row detached, and the region sets, patient groups (with contrasts) and patient traits
    given, as set_region_sets(), set_patient_groups() and set_patient_traits() would leave them; _run does nothing.
    """
    eng = gibbs.GibbsEngine.__new__(gibbs.GibbsEngine)
    (eng.G, eng.Nreg, eng.U) = (G, N, U)
    (eng.region_names, eng.region_offsets, eng.region_members, eng.region_J, eng.region_smax) = (None, None, None, 0, 0)
    if sets is not None:
        (eng.region_names, eng.region_offsets, eng.region_members) = gibbs.region_sets_csr(sets, N)
        (eng.region_J, eng.region_smax) = (len(eng.region_names), int(np.diff(eng.region_offsets).max()))
    (eng.group_J, eng.group_umax, eng.group_with_sets) = (0, 0, sets is not None)
    if groups is not None:
        (eng.group_names, eng.group_offsets, eng.group_members) = gibbs.patient_groups_csr(groups, U)
        (eng.group_contrasts, eng.group_bin_offsets) = gibbs.patient_group_contrasts(contrasts, eng.group_names, eng.group_offsets,
                                                                                     eng.group_members)
        (eng.group_J, eng.group_umax) = (len(eng.group_names), int(np.diff(eng.group_offsets).max()))
    (eng.trait_Q, eng.trait_umax, eng.trait_with_sets) = (0, 0, sets is not None)
    if traits is not None:
        (eng.trait_names, scores, known, eng.trait_n_known) = gibbs.patient_traits_scores(traits, U)
        (eng.trait_scores, eng.trait_known) = (np.ascontiguousarray(scores), np.ascontiguousarray(known.astype(np.uint8)))
        (eng.trait_Q, eng.trait_umax) = (len(eng.trait_names), int(eng.trait_n_known.max()))
    for a in gibbs.ACCUMULATORS:
        setattr(eng, a.attr, None)
        if a.key in attached:
            setattr(eng, a.attr, one_word_buffers(a))
            setattr(eng, a.key + "_every", 1)
            setattr(eng, a.key + "_sweeps", 0)
    (eng.ctx, eng.n_accumulated, eng._run, eng.counts) = (Recorder(), 0, lambda *args: None, None)
    return eng
