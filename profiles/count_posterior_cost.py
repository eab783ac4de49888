"""
Cost of the anomalous-region counts (fcd_count.hip) on one MI355X.

  * accumulation: fcd_gibbs_run, 500 sweeps, with and without the count accumulator attached (every sweep counted), at
    cfg3 (Nreg 200, U 50, 1024 chains) and at cfg5's per-GPU share (Nreg 400, U 250, 1024 chains); the difference per
    sweep against the sweep itself and against the byte floor of one tally (the r state read once; the two histograms,
    which a tally touches only where chains land, are listed apart);
  * one fcd_gibbs_count_tally call alone (two launches: per-chain sums, then one workgroup per histogram row);
  * fcd_vb_count_posterior (the Poisson-binomial kernel of the variational fit) at both shapes.

    python profiles/count_posterior_cost.py [--sweeps 500] [--reps 3]

Prints one JSON document.  Timings: HIP events around the calls, best of --reps, after one warm-up call each.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal


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


def shape_run(torch, np, fcdiff_amd, name, Nreg, H, U, G, sweeps, reps):
    from fcdiff_amd import _lib
    from fcdiff_amd.gibbs import GibbsEngine
    model = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(Nreg, H, U, seed=0)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model, fit.b, fit.bt = model, b, bt
    fit._init_lps(Nreg, H, U)
    fit._update_lps()
    ctx = fit._context()
    eng = GibbsEngine(fit._d["S_B"], fit._d["lM"], Nreg, U, G, seed=1, edge_index="symmetric", ctx=ctx)
    eng.set_hyper(model.gamma, model.pi2())
    eng.init(float(model.pi))
    state = {"s": 0}

    def run(attached):
        if attached:
            eng.attach_count_accumulator(1)
        else:
            eng.detach_count_accumulator()
        s0 = state["s"]
        eng.run(s0, sweeps, mstep_every=1, accumulate_from=s0)
        state["s"] += sweeps
    run(False)
    run(True)
    t_plain, t_acc = [], []
    for _ in range(reps):          # alternated: drift of the clock hits both alike
        t_plain.append(timed(torch, lambda: run(False), 1))
        t_acc.append(timed(torch, lambda: run(True), 1))
    eng.detach_count_accumulator()
    (tp, ta) = (min(t_plain) / sweeps, min(t_acc) / sweeps)
    r_bytes = eng.GW * Nreg * U * 8
    hist_bytes = (U * (Nreg + 1) + Nreg * (U + 1)) * 4
    out = {"shape": {"Nreg": Nreg, "U": U, "G": G}, "sweeps": sweeps,
           "sweep_ms_without": tp, "sweep_ms_with": ta, "accumulate_ms_per_sweep": ta - tp,
           "accumulate_fraction_of_sweep": (ta - tp) / tp,
           "r_state_MB": r_bytes / 1e6, "r_state_us_at_peak": r_bytes / (HBM_PEAK_GBS * 1e3),
           "histograms_MB": hist_bytes / 1e6,
           "all_sweep_ms_without": [x / sweeps for x in t_plain], "all_sweep_ms_with": [x / sweeps for x in t_acc]}
    # one tally alone
    hp = torch.zeros((U, Nreg + 1), dtype=torch.int32, device="cuda")
    hr = torch.zeros((Nreg, U + 1), dtype=torch.int32, device="cuda")
    eng.count_tally(hp, hr)
    us = 1e3 * timed(torch, lambda: [eng.count_tally(hp, hr) for _ in range(20)], reps) / 20
    out["count_tally_us"] = us
    out["count_tally_r_state_GB_per_s"] = r_bytes / (us * 1e3)
    # the variational fit's kernel, on the fit's own lq_R
    lq_R = fit._d["lq_R"]
    p_p = torch.empty((U, Nreg + 1), dtype=torch.float64, device="cuda")
    p_r = torch.empty((Nreg, U + 1), dtype=torch.float64, device="cuda")

    def kern(n=10):
        for _ in range(n):
            ctx.call("fcd_vb_count_posterior", _lib.dptr(lq_R), Nreg, U, _lib.dptr(p_p), _lib.dptr(p_r), _lib.stream_ptr())
    kern(1)
    out["vb_count_posterior_us"] = 1e3 * timed(torch, kern, reps) / 10
    print("%s done" % name, file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="cfg3,cfg5")
    args = ap.parse_args()
    import numpy as np
    import torch
    import fcdiff_amd
    torch.cuda.set_device(0)
    shapes = {"cfg3": (200, 50, 50, 1024), "cfg5": (400, 250, 250, 1024)}
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS}
    for name in args.only.split(","):
        res[name] = shape_run(torch, np, fcdiff_amd, name, *shapes[name], sweeps=args.sweeps, reps=args.reps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
