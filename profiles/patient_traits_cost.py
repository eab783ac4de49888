"""
Cost of the patient-trait rank-sum tally (fcd_patient_traits.hip) on one MI355X, at cfg3's shape (Nreg 200, U 100, 1024 chains).

Q = 1, 4 and 16 traits of the 100 patients (continuous values; every fourth trait has 10 patients it is not known for),
measured
  * without region sets (R = 200 rows) and with 7 disjoint region sets as rows after the regions (R = 207): one
    fcd_gibbs_patient_trait_tally call (two launches: per-chain (k, A) of every (trait, row), then one workgroup per (trait,
    row) that bins them);
beside two other times from the same run: one fcd_gibbs_patient_group_tally call for the two halves of the patients and their
contrast (the case of profiles/patient_groups_cost.py), and one sweep of fcd_gibbs_run with nothing attached.

    python profiles/patient_traits_cost.py [--sweeps 200] [--reps 7] [--calls 20]

Prints one JSON document.  Timings: HIP events around --calls calls (or --sweeps sweeps), after one warm-up of each, the
median of --reps repeats; all repeats are listed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    """ms of fn() per repeat (HIP events), after one warm-up call."""
    fn()
    out = []
    for _ in range(reps):
        (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def partition(Nreg, J):
    """J disjoint runs of regions that cover 0 .. Nreg-1, sizes as equal as they come."""
    edges = [round(j * Nreg / J) for j in range(J + 1)]
    return [list(range(edges[j], edges[j + 1])) for j in range(J)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import fcdiff_amd
    from fcdiff_amd.gibbs import GibbsEngine, PATIENT_TRAIT_BINS
    torch.cuda.set_device(0)
    (Nreg, H, U, G) = (200, 50, 100, 1024)
    model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(Nreg, H, U, seed=0)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model, fit.b, fit.bt = model, b, bt
    fit._init_lps(Nreg, H, U)
    fit._update_lps()
    eng = GibbsEngine(fit._d["S_B"], fit._d["lM"], Nreg, U, G, seed=1, edge_index="symmetric", ctx=fit._context())
    eng.set_hyper(model.gamma, model.pi2())
    eng.init(float(model.pi))
    eng.run(0, 20, mstep_every=1, accumulate_from=0)             # a state off the initial draw
    rng = np.random.default_rng(0)
    values = rng.normal(size=(16, U))
    values[::4, :10] = np.nan
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "U": U, "G": G},
           "calls_per_timing": args.calls, "repeats": args.reps, "tally_us": {}}

    def per_call(ms):
        return [1e3 * x / args.calls for x in ms]

    for (name, sets) in (("without_region_sets", None), ("with_7_region_sets", partition(Nreg, 7))):
        eng.set_region_sets(sets)
        res["tally_us"][name] = {}
        for Q in (1, 4, 16):
            eng.set_patient_traits(values[:Q])
            R = eng.patient_trait_rows()
            hist = torch.zeros((Q, R, eng.trait_umax + 1 + PATIENT_TRAIT_BINS + 3), dtype=torch.int32, device="cuda")
            total = torch.zeros((Q, R, eng.trait_umax + 1), dtype=torch.int64, device="cuda")
            us = per_call(timed(torch, lambda: [eng.patient_trait_tally(hist, total) for _ in range(args.calls)], args.reps))
            res["tally_us"][name]["Q=%d" % Q] = {"rows": R, "us": statistics.median(us), "all_us": us,
                                                 "scratch_MB": Q * R * eng.GW * 64 * 6 / 1e6, "histogram_rows": Q * R}
    # the patient-group tally of the two halves and their contrast (7 region sets as rows), and one sweep with nothing attached
    eng.set_patient_groups({"first_half": list(range(U // 2)), "second_half": list(range(U // 2, U))},
                           [("first_half", "second_half")])
    R = eng.patient_group_rows()
    hg = torch.zeros((eng.group_J, R, eng.group_umax + 1), dtype=torch.int32, device="cuda")
    hj = torch.zeros(R * int(eng.group_bin_offsets[-1]), dtype=torch.int32, device="cuda")
    us = per_call(timed(torch, lambda: [eng.patient_group_tally(hg, hj) for _ in range(args.calls)], args.reps))
    res["patient_group_tally_us"] = {"rows": R, "groups": 2, "contrasts": 1, "us": statistics.median(us), "all_us": us}
    state = {"s": 20}

    def sweeps():
        eng.run(state["s"], args.sweeps, mstep_every=1, accumulate_from=state["s"])
        state["s"] += args.sweeps
    us = [1e3 * x / args.sweeps for x in timed(torch, sweeps, args.reps)]
    res["sweep_us"] = {"sweeps_per_timing": args.sweeps, "us": statistics.median(us), "all_us": us}
    for cases in res["tally_us"].values():
        for case in cases.values():
            case["times_patient_group_tally"] = case["us"] / res["patient_group_tally_us"]["us"]
            case["fraction_of_sweep"] = case["us"] / res["sweep_us"]["us"]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
