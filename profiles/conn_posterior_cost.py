"""
Cost of the connection-level posteriors (fcd_post.hip) on one MI355X.

  * accumulation: fcd_gibbs_run, 500 sweeps, with and without the (f_c, mixture case) accumulator attached (every sweep
    counted), at cfg3 (Nreg 200, U 50, 1024 chains) and at cfg5's per-GPU share (Nreg 400, U 250, 1024 chains);
    the difference per sweep against the sweep itself and against the byte floor of the accumulator (f state read once,
    counts read and written once);
  * contraction: fcd_conn_posterior at both shapes and both weight sources, time and GB/s of its byte floor
    (counts: 36 B counts + 8 B bt + 40 B out per item; mean-field: 8 B bt + 40 B out, the q tables are small).

    python profiles/conn_posterior_cost.py [--sweeps 500] [--reps 3]

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
    from fcdiff_amd.gibbs import GibbsEngine
    from fcdiff_amd.fit import conn_posterior
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
    C = eng.C
    state = {"s": 0}

    def run(attached):
        if attached:
            eng.attach_pair_accumulator(1)
        else:
            eng.detach_pair_accumulator()
        s0 = state["s"]
        eng.run(s0, sweeps, mstep_every=1, accumulate_from=s0)
        state["s"] += sweeps
    run(False)
    run(True)
    t_plain, t_acc = [], []
    for _ in range(reps):          # alternated: drift of the clock hits both alike
        t_plain.append(timed(torch, lambda: run(False), 1))
        t_acc.append(timed(torch, lambda: run(True), 1))
    eng.detach_pair_accumulator()
    (tp, ta) = (min(t_plain) / sweeps, min(t_acc) / sweeps)
    floor_bytes = eng.GW * C * 64 + 2 * C * U * 36
    out = {"shape": {"Nreg": Nreg, "C": C, "U": U, "G": G}, "sweeps": sweeps,
           "sweep_ms_without": tp, "sweep_ms_with": ta, "accumulate_ms_per_sweep": ta - tp,
           "accumulate_fraction_of_sweep": (ta - tp) / tp,
           "accumulate_floor_MB": floor_bytes / 1e6,
           "accumulate_floor_us_at_peak": floor_bytes / (HBM_PEAK_GBS * 1e3),
           "all_sweep_ms_without": [x / sweeps for x in t_plain], "all_sweep_ms_with": [x / sweeps for x in t_acc]}
    # one launch of the accumulator alone
    acc = torch.zeros((C, U, 3, 3), dtype=torch.int32, device="cuda")
    eng.pair_tally(acc)
    out["pair_tally_us"] = 1e3 * timed(torch, lambda: [eng.pair_tally(acc) for _ in range(20)], reps) / 20
    # contraction, both weight sources
    counts = torch.randint(0, 1000, (C, U, 3, 3), dtype=torch.int32, device="cuda")
    bt_d = fit._d["bt"]
    theta = model.theta()
    items = C * U
    pc = lambda: conn_posterior(ctx, bt_d, Nreg, U, theta, counts=counts)         # noqa: E731
    pc()
    lq_F, lq_R = fit._d["lq_F"], fit._d["lq_R"]
    pv = lambda: conn_posterior(ctx, bt_d, Nreg, U, theta, lq_F=lq_F, lq_R=lq_R)  # noqa: E731
    pv()
    # the kernel alone: outputs allocated once, launches back to back
    p_T = torch.empty((C, U), dtype=torch.float64, device="cuda")
    p_Ft = torch.empty((C, U, 3), dtype=torch.float64, device="cuda")
    p_ch = torch.empty((C, U), dtype=torch.float64, device="cuda")
    from fcdiff_amd import _lib
    (th, _th) = _lib.dbl_array(theta)

    def kern(use_counts, n=10):
        for _ in range(n):
            ctx.call("fcd_conn_posterior", _lib.dptr(bt_d), Nreg, U, th, _lib.dptr(counts if use_counts else None),
                     _lib.dptr(None if use_counts else lq_F), _lib.dptr(None if use_counts else lq_R), _lib.dptr(p_T),
                     _lib.dptr(p_Ft), _lib.dptr(p_ch), _lib.stream_ptr())
    kern(True, 1)
    kern(False, 1)
    for (key, use, nbytes) in (("contraction_counts", True, 84), ("contraction_vb", False, 48)):
        ms = timed(torch, lambda: kern(use), reps) / 10
        gbs = items * nbytes / (ms * 1e6)
        out[key] = {"us": ms * 1e3, "bytes_per_item": nbytes, "GB": items * nbytes / 1e9, "GB_per_s": gbs,
                    "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS}
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
