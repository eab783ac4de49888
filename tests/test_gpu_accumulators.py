"""
The six accumulators of fcd_gibbs_run attached at once on the MI355X: GibbsEngine.run() walks gibbs.ACCUMULATORS in one loop,
sends the region sets, patient groups and patient traits to the shared context and attaches every row's buffers, and each
buffer equals that of a run with its accumulator attached alone.
"""
import numpy as np
import numpy.testing as nptest
import pytest

pytestmark = pytest.mark.gpu

HOST = {"pair": "pair_counts_host", "count": "count_hist_host", "coanomaly": "coanomaly_host", "region_set": "region_set_host",
        "patient_group": "patient_group_host", "patient_trait": "patient_trait_host"}


def test_all_six_together_equal_each_alone():
    """
    Periods 1, 2, 3, 1, 2, 3 in the table's order, so that the rows count different sweeps: every buffer of a run with all six
    attached equals, bit for bit and dtype for dtype, that of a run from the same seed with this one attached alone (the
    region sets stay set where the patient groups and traits take them as rows), and the sweep counters are pair_sweeps_in's.
    Nreg = 6, U = 3, G = 130: three chain words, two live lanes in the last.  Two region sets, one a singleton; two disjoint
    patient groups and their contrast; one trait that is not known for one patient.
    """
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import ACCUMULATORS, GibbsEngine, PATIENT_TRAIT_BINS, pair_sweeps_in
    from oracle import c_oracle as CO
    _lib.load()
    ctx = _lib.Context()
    (N, U, G, n_sweeps, burn) = (6, 3, 130, 7, 2)
    keys = [a.key for a in ACCUMULATORS]
    assert keys == list(HOST)
    every = dict(zip(keys, (1, 2, 3, 1, 2, 3)))
    (sets, groups, contrasts) = ({"net": [0, 2, 5], "one": [3]}, {"a": [0], "b": [1, 2]}, [("a", "b")])
    traits = {"dose": [1.0, float("nan"), 3.0]}
    m = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, 4, U, seed=11)
    (S_B, lM) = (torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in CO.lik_tables(b, bt, m.theta()))

    def run(attach):
        e = GibbsEngine(S_B, lM, N, U, G, chain0=0, seed=77, edge_index="symmetric", ctx=ctx)
        e.set_hyper(m.gamma, m.pi2())
        e.init(0.3)
        if set(attach) & {"region_set", "patient_group", "patient_trait"}:
            e.set_region_sets(sets)
        if "patient_group" in attach:
            e.set_patient_groups(groups, contrasts)
        if "patient_trait" in attach:
            e.set_patient_traits(traits)
        for k in attach:
            getattr(e, "attach_%s_accumulator" % k)(every[k])
        e.run(0, n_sweeps, mstep_every=1, accumulate_from=burn)
        return e

    def buffers(e, a):
        got = getattr(e, HOST[a.key])()
        return got if a.paired else (got,)
    together = run(keys)
    want_sweeps = [pair_sweeps_in(0, n_sweeps, burn, every[k]) for k in keys]
    assert want_sweeps == [5, 3, 2, 5, 3, 2]
    assert [getattr(together, k + "_sweeps") for k in keys] == want_sweeps
    assert together.patient_group_rows() == together.patient_trait_rows() == N + 2
    for (a, want) in zip(ACCUMULATORS, want_sweeps):
        alone = run([a.key])
        assert [getattr(alone, b.attr) is not None for b in ACCUMULATORS] == [b is a for b in ACCUMULATORS]
        assert getattr(alone, a.key + "_sweeps") == want
        (one, all6) = (buffers(alone, a), buffers(together, a))
        assert [tuple(x.shape) for x in one] == [tuple(x.shape) for x in all6] == [tuple(s) for s in a.shapes(alone)]
        assert [x.dtype for x in one] == [x.dtype for x in all6] == [np.uint32 if d == "int32" else np.int64 for d in a.dtypes]
        for (x, y) in zip(one, all6):
            nptest.assert_array_equal(x, y)
    # (nothing compared above was empty: every histogram holds G states per counted sweep)
    assert int(together.pair_counts_host()[0, 0].sum()) == G * 5
    assert np.all(together.count_hist_host()[0].astype(np.int64).sum(axis=1) == G * 3)
    (rp, pp) = (x.astype(np.int64) for x in together.coanomaly_host())
    assert np.trace(rp) == np.trace(pp) and np.array_equal(rp, rp.T)
    assert np.all(together.region_set_host()[0].astype(np.int64).sum(axis=2) == G * 5)
    (hist_group, hist_joint) = together.patient_group_host()
    assert np.all(hist_group.astype(np.int64).sum(axis=2) == G * 3) and int(hist_joint.astype(np.int64).sum()) == (N + 2) * G * 3
    (trait_hist, trait_sum) = together.patient_trait_host()
    assert together.trait_umax == 2 and trait_hist.shape[2] == 3 + PATIENT_TRAIT_BINS + 3
    trait_hist = trait_hist.astype(np.int64)
    assert np.all(trait_hist[:, :, :3].sum(axis=2) == G * 2)
    # (two known patients with scores -1 and 1: at k = 1 the rank sum A is -1 or 1, and trait_sum[k = 1] the balance of the two)
    assert np.array_equal(trait_hist[:, :, -3] + trait_hist[:, :, -1], trait_hist[:, :, 1]) and not trait_hist[:, :, -2].any()
    assert np.array_equal(trait_sum[:, :, 1], trait_hist[:, :, -1] - trait_hist[:, :, -3]) and not trait_sum[:, :, [0, 2]].any()
