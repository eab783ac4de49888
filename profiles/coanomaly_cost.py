"""
Cost of the co-anomaly counts (fcd_coanomaly.hip) on one MI355X.

  * one fcd_gibbs_coanomaly_tally call alone (one launch for both matrices), at cfg3 (Nreg 200, U 50, 1024 chains) and
    at cfg5's per-GPU share (Nreg 400, U 500, 1024 chains), with fcd_gibbs_count_tally (the anomalous-region
    histograms, two launches) in the same session for comparison;
  * accumulation: fcd_gibbs_run with and without the accumulator attached (every sweep counted), alternated; the sweep
    time of that run and the difference per sweep;
  * fcd_vb_coanomaly (the independence form of the variational fit) at both shapes.

    python profiles/coanomaly_cost.py [--sweeps 200] [--reps 3] [--label TEXT] [--embed KEY=FILE ...]

Prints one JSON document.  Timings: HIP events around the calls, best of --reps, after one warm-up call each.
--label names the library variant measured (FCDIFF_HIP_LIB: builds with another -DFCD_CO_WG_PER_CU, see the Makefile);
--embed KEY=FILE puts a JSON file under KEY of the document: `bench`, the bench.py samples of this branch and its parent
commit, alternated in one session; `split_targets`, this script's figures for other FCD_CO_WG_PER_CU builds.
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


def shape_run(torch, fcdiff_amd, name, Nreg, H, U, G, sweeps, reps):
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
            eng.attach_coanomaly_accumulator(1)
        else:
            eng.detach_coanomaly_accumulator()
        s0 = state["s"]
        eng.run(s0, sweeps, mstep_every=1, accumulate_from=s0)
        state["s"] += sweeps
    run(False)
    run(True)
    t_plain, t_acc = [], []
    for _ in range(reps):          # alternated: drift of the clock hits both alike
        t_plain.append(timed(torch, lambda: run(False), 1))
        t_acc.append(timed(torch, lambda: run(True), 1))
    eng.detach_coanomaly_accumulator()
    (tp, ta) = (min(t_plain) / sweeps, min(t_acc) / sweeps)
    gw = eng.GW
    terms = gw * (Nreg * (Nreg + 1) // 2 * U + U * (U + 1) // 2 * Nreg)        # AND + popcount + add, lower triangles
    out = {"shape": {"Nreg": Nreg, "U": U, "G": G}, "sweeps": sweeps,
           "sweep_ms_without": tp, "sweep_ms_with": ta, "accumulate_ms_per_sweep": ta - tp,
           "accumulate_fraction_of_sweep": (ta - tp) / tp,
           "r_state_MB": gw * Nreg * U * 8 / 1e6, "popcount_terms_lower_triangles": terms,
           "all_sweep_ms_without": [x / sweeps for x in t_plain], "all_sweep_ms_with": [x / sweeps for x in t_acc]}
    # one tally alone, and the count tally beside it
    rp = torch.zeros((Nreg, Nreg), dtype=torch.int32, device="cuda")
    pp = torch.zeros((U, U), dtype=torch.int32, device="cuda")
    eng.coanomaly_tally(rp, pp)
    us = 1e3 * timed(torch, lambda: [eng.coanomaly_tally(rp, pp) for _ in range(50)], reps) / 50
    out["coanomaly_tally_us"] = us
    out["coanomaly_tally_Gterms_per_s"] = terms / (us * 1e3)
    if Nreg <= 1023 and U <= 512:
        hp = torch.zeros((U, Nreg + 1), dtype=torch.int32, device="cuda")
        hr = torch.zeros((Nreg, U + 1), dtype=torch.int32, device="cuda")
        eng.count_tally(hp, hr)
        out["count_tally_us"] = 1e3 * timed(torch, lambda: [eng.count_tally(hp, hr) for _ in range(50)], reps) / 50
    # the variational fit's kernel, on the fit's own lq_R
    lq_R = fit._d["lq_R"]
    reg = torch.empty((Nreg, Nreg), dtype=torch.float64, device="cuda")
    pat = torch.empty((U, U), dtype=torch.float64, device="cuda")

    def kern(n=10):
        for _ in range(n):
            ctx.call("fcd_vb_coanomaly", _lib.dptr(lq_R), Nreg, U, _lib.dptr(reg), _lib.dptr(pat), _lib.stream_ptr())
    kern(1)
    out["vb_coanomaly_us"] = 1e3 * timed(torch, kern, reps) / 10
    print("%s done" % name, file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="cfg3,cfg5")
    ap.add_argument("--label", default="product build")
    ap.add_argument("--embed", action="append", default=[], metavar="KEY=FILE")
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    torch.cuda.set_device(0)
    shapes = {"cfg3": (200, 50, 50, 1024), "cfg5": (400, 250, 500, 1024)}
    res = {"device": torch.cuda.get_device_name(0), "library": args.label}
    for name in args.only.split(","):
        res[name] = shape_run(torch, fcdiff_amd, name, *shapes[name], sweeps=args.sweeps, reps=args.reps)
    for item in args.embed:
        (key, path) = item.split("=", 1)
        res[key] = json.load(open(path))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
