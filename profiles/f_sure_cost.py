#!/usr/bin/env python3
"""What the decided-tile path of the pair-tile f pass costs where no tile is decided, and what it takes where all are.

Sweep time at Nreg 200, U 50, 1024 chains in one fcd_gibbs_run call, on
  weak    H 2, broad components (sigma 0.2 / 0.25 / 0.3, mu -0.05 / 0 / 0.05): no edge decided -- the record build leaves no
          hint and the call runs the kernel without the path;
  cfg3    H 50, the model's components: every tile decided -- the decided path runs in its run form (stat f_run_passes);
  mixed   H 20: most tiles decided, not all -- the per-tile kernel with the decided-tile path.
Prints one JSON line with ms per sweep of `--runs` calls of `--sweeps` sweeps each and the f_sure counters.  Run it once per
build to compare two builds (FCDIFF_HIP_LIB names another library of the same ABI), alternating; knob f_sure = 1
(--off) switches the path off inside one build.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", choices=("weak", "cfg3", "mixed"), default="weak")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--off", action="store_true", help="knob f_sure = 1: never the decided-tile path")
    args = ap.parse_args()
    import fcdiff_amd
    from fcdiff_amd.gibbs import GibbsEngine
    (Nreg, U, G) = (200, 50, 1024)
    H = {"weak": 2, "cfg3": 50, "mixed": 20}[args.data]
    model = fcdiff_amd.UnsharedRegionModel()
    if args.data == "weak":
        model.sigma = np.array([0.2, 0.25, 0.3])
        model.mu = np.array([-0.05, 0.0, 0.05])
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(Nreg, H, U, seed=0)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model, fit.b, fit.bt = model, b, bt
    fit._init_lps(Nreg, H, U)
    fit._update_lps()
    ctx = fit._context()
    if args.off:
        ctx.set_knob("f_sure", 1)
    eng = GibbsEngine(fit._d["S_B"], fit._d["lM"], Nreg, U, G, seed=1, ctx=ctx)
    eng.set_hyper(model.gamma, model.pi2())
    eng.init(float(model.pi))
    eng.run(0, 64, mstep_every=1)
    torch.cuda.synchronize()

    def stat(name):
        try:
            return ctx.stat(name)
        except Exception:      # noqa: BLE001  (a build from before the counters)
            return None
    names = ("f_rec_passes", "f_sure_passes", "f_run_passes", "f_sure_tiles", "f_sure_fallbacks", "f_repeats", "tally_f_in_f")
    s0 = [stat(k) for k in names]
    ms = []
    sweep = 64
    for _ in range(args.runs):
        t0 = time.perf_counter()
        eng.run(sweep, args.sweeps, mstep_every=1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.sweeps * 1e3)
        sweep += args.sweeps
    rise = {k: (None if a is None else stat(k) - a) for (k, a) in zip(names, s0)}
    i = (Nreg + 1) // 2                                    # pair-aligned tiles: fpt_tiles((Nreg + 1) / 2)
    tiles = (i // 2) * (i // 2 + 1) if i % 2 == 0 else (i // 2 + 1) ** 2
    out = {"data": args.data, "f_sure_off": bool(args.off), "lib": os.environ.get("FCDIFF_HIP_LIB", "default"),
           "ms_per_sweep": [round(x, 5) for x in ms], "min": round(min(ms), 5), "range": round(max(ms) - min(ms), 5), "rise": rise,
           "tiles_per_pass": tiles,
           "share_on_path": None if not rise["f_sure_tiles"] else rise["f_sure_tiles"] / float(tiles * rise["f_rec_passes"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
