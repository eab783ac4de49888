"""
Cost of the region-set counts (fcd_region_sets.hip) on one MI355X, at cfg3's shape (Nreg 200, U 100, 1024 chains).

  * one fcd_gibbs_region_set_tally call alone (two launches: per-chain sums of every (set, patient) and the "any" counts of
    every set, then one workgroup per histogram row) for 7 disjoint sets, 17 disjoint sets (both partitions of the regions)
    and the 200 singletons, with fcd_gibbs_count_tally from the same run beside them;
  * accumulation: fcd_gibbs_run with and without the region-set accumulator attached (7 sets, every sweep counted).

A partition reads the r state once, as the count tally does; what grows with the sets is the scratch, (J U + J) rows of
1024 uint16 written by the first launch and read by the second, listed per case.

    python profiles/region_sets_cost.py [--sweeps 500] [--reps 3]

Prints one JSON document.  Timings: HIP events around the calls, best of --reps, after one warm-up call each.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, reps):
    best = None
    for _ in range(reps):
        (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def partition(Nreg, J):
    """J disjoint runs of regions that cover 0 .. Nreg-1, sizes as equal as they come."""
    edges = [round(j * Nreg / J) for j in range(J + 1)]
    return [list(range(edges[j], edges[j + 1])) for j in range(J)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd.gibbs import GibbsEngine
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
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "U": U, "G": G},
           "r_state_MB": eng.GW * Nreg * U * 8 / 1e6, "calls_per_timing": args.calls, "tally_us": {}}
    hp = torch.zeros((U, Nreg + 1), dtype=torch.int32, device="cuda")
    hr = torch.zeros((Nreg, U + 1), dtype=torch.int32, device="cuda")
    eng.count_tally(hp, hr)
    res["count_tally_us"] = 1e3 * timed(torch, lambda: [eng.count_tally(hp, hr) for _ in range(args.calls)], args.reps) / args.calls
    res["count_tally_scratch_MB"] = (U + Nreg) * eng.GW * 64 * 2 / 1e6
    cases = {"7_disjoint": partition(Nreg, 7), "17_disjoint": partition(Nreg, 17), "200_singletons": [[n] for n in range(Nreg)]}
    for (name, sets) in cases.items():
        eng.set_region_sets(sets)
        (J, s_max) = (eng.region_J, eng.region_smax)
        hs = torch.zeros((J, U, s_max + 1), dtype=torch.int32, device="cuda")
        hv = torch.zeros((J, U + 1), dtype=torch.int32, device="cuda")
        eng.region_set_tally(hs, hv)
        us = 1e3 * timed(torch, lambda: [eng.region_set_tally(hs, hv) for _ in range(args.calls)], args.reps) / args.calls
        res["tally_us"][name] = {"J": J, "S_max": s_max, "us": us, "times_count_tally": us / res["count_tally_us"],
                                 "scratch_MB": (J * U + J) * eng.GW * 64 * 2 / 1e6, "histogram_rows": J * U + J}
    # one sweep with and without the accumulator (7 sets)
    eng.set_region_sets(cases["7_disjoint"])
    state = {"s": 20}

    def run(attached):
        if attached:
            eng.attach_region_set_accumulator(1)
        else:
            eng.detach_region_set_accumulator()
        s0 = state["s"]
        eng.run(s0, args.sweeps, mstep_every=1, accumulate_from=s0)
        state["s"] += args.sweeps
    run(False)
    run(True)
    (t_plain, t_acc) = ([], [])
    for _ in range(args.reps):          # alternated: drift of the clock hits both alike
        t_plain.append(timed(torch, lambda: run(False), 1))
        t_acc.append(timed(torch, lambda: run(True), 1))
    eng.detach_region_set_accumulator()
    (tp, ta) = (min(t_plain) / args.sweeps, min(t_acc) / args.sweeps)
    res["sweep"] = {"sets": "7_disjoint", "sweeps": args.sweeps, "sweep_ms_without": tp, "sweep_ms_with": ta,
                    "accumulate_ms_per_sweep": ta - tp, "accumulate_fraction_of_sweep": (ta - tp) / tp,
                    "all_sweep_ms_without": [x / args.sweeps for x in t_plain],
                    "all_sweep_ms_with": [x / args.sweeps for x in t_acc]}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
