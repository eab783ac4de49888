"""
Cost of the options of the permutation baselines (fcd_baseline_group_perm_opt, fcd_baseline_network_bits_opt;
fcd_baseline.hip) on one MI355X, at C = 19 900 connections (200 regions), H = U = 100, P = 1000 and 10 000 labellings already
on the device.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around a window of
back-to-back calls, --rounds rounds; best and median round per variant).  Per P, for the group test (one call) and for the
network-based statistic at threshold 3 (the bits call and the components call of one chunk of P labellings):
  default              the call without options (fcd_baseline_group_perm, fcd_baseline_network_bits): the yardstick
  missing_complete     FCD_BASELINE_MISSING on the same complete data: A and n1, two accumulators
  missing_nan          FCD_BASELINE_MISSING with 5 % of the entries NaN
  welch_complete       FCD_BASELINE_WELCH on complete data: A and B, two accumulators
  welch_nan            both flags with 5 % NaN: A, n1 and B, three accumulators
Under "ratios": every variant over the default of the same run and P.  The MFMA count predicts about 2 for one more accumulator
and 3 for two; the loads do not grow.  Under "agreement": missing_complete against default, compared bit for bit.
--default-only times the two default variants alone and binds no call with options: for a library of the parent commit
(FCDIFF_HIP_LIB), alternated with this one in one session.  A record, not a gate.

    python profiles/baseline_missing_cost.py [--rounds 7] [--default-only] [--out profiles/baseline_missing_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS = (1000, 10000)
THRESHOLD = 3.0
(MISSING, WELCH) = (1, 2)
OPTIONS = {"missing_complete": (MISSING, False), "missing_nan": (MISSING, True), "welch_complete": (WELCH, False),
           "welch_nan": (MISSING | WELCH, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baseline_missing_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline
    if args.default_only:
        for name in ("fcd_baseline_group_perm_opt", "fcd_baseline_network_bits_opt"):
            _lib.SIGNATURES.pop(name, None)
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    C = fcdiff_amd.N_to_C(Nreg)
    W = (C + 31) // 32
    rng = np.random.default_rng(0)
    b = rng.normal(0.3, 0.1, (C, H))
    bt = rng.normal(0.3, 0.1, (C, U))
    bt[:Nreg - 1] += 0.05
    (bn, btn) = (b.copy(), bt.copy())
    bn[rng.random(b.shape) < 0.05] = np.nan
    btn[rng.random(bt.shape) < 0.05] = np.nan
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    data = {False: (dev(b), dev(bt)), True: (dev(bn), dev(btn))}
    ctx = _lib.Context()
    (Pt, stream) = (_lib.dptr, _lib.stream_ptr())
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device="cuda")
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")
    i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device="cuda")
    labels = dict((P, dev(baseline.draw_labels(P, H, U, seed=P))) for P in PS)
    out = {}

    def group(P, name):
        o = out.setdefault(("group", P, name), dict(t=f64(C), region=f64(Nreg), mt=f64(P), mr=f64(P), ct=i64(C), cr=i64(Nreg),
                                                    nc=i64(C), np=i64(C)))
        if name == "default":
            (x, y) = data[False]
            ctx.call("fcd_baseline_group_perm", Pt(x), Pt(y), C, H, U, Pt(labels[P]), P, Pt(o["t"]), Pt(o["region"]), Pt(o["mt"]),
                     Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), stream)
        else:
            (flags, nan) = OPTIONS[name]
            (x, y) = data[nan]
            ctx.call("fcd_baseline_group_perm_opt", Pt(x), Pt(y), C, H, U, Pt(labels[P]), P, flags, Pt(o["t"]), Pt(o["region"]),
                     Pt(o["mt"]), Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), Pt(o["nc"]), Pt(o["np"]), stream)

    def network(P, name):
        o = out.setdefault(("network", P, name), dict(bits=i32(P, W), ne=i32(P), me=i32(P), mg=i32(P)))
        if name == "default":
            (x, y) = data[False]
            ctx.call("fcd_baseline_network_bits", Pt(x), Pt(y), C, H, U, Pt(labels[P]), P, THRESHOLD, 0, Pt(o["bits"]), Pt(None),
                     stream)
        else:
            (flags, nan) = OPTIONS[name]
            (x, y) = data[nan]
            ctx.call("fcd_baseline_network_bits_opt", Pt(x), Pt(y), C, H, U, Pt(labels[P]), P, THRESHOLD, 0, flags, Pt(o["bits"]),
                     Pt(None), stream)
        ctx.call("fcd_graph_components", Pt(o["bits"]), P, C, Pt(None), Pt(o["ne"]), Pt(o["me"]), Pt(o["mg"]), stream)

    names = ["default"] + ([] if args.default_only else list(OPTIONS))
    variants = {}
    for P in PS:
        for name in names:
            variants["group_P%d_%s" % (P, name)] = (lambda P=P, name=name: group(P, name), 20 if P <= 1000 else 4)
            variants["network_P%d_%s" % (P, name)] = (lambda P=P, name=name: network(P, name), 20 if P <= 1000 else 4)
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's workspace, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):                 # alternated: drift of the clock hits all alike
        for (name, (fn, n)) in variants.items():
            (a, z) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a.record()
            for _i in range(n):
                fn()
            z.record()
            z.synchronize()
            times[name].append(1e3 * a.elapsed_time(z) / n)
    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("FCDIFF_HIP_LIB", "this tree's"),
           "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U, "nan_fraction": 0.05, "threshold": THRESHOLD},
           "rounds": args.rounds, "calls_per_window": dict((k, v[1]) for (k, v) in variants.items()),
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round",
           "variants": {}, "ratios": {}, "agreement": {}}
    for name in variants:
        res["variants"][name] = {"us": min(times[name]), "median_us": float(np.median(times[name])), "all_us": times[name]}
    v = res["variants"]
    for P in PS:
        for kind in ("group", "network"):
            base = v["%s_P%d_default" % (kind, P)]["median_us"]
            for name in names[1:]:
                res["ratios"]["%s_P%d_%s_over_default" % (kind, P, name)] = v["%s_P%d_%s" % (kind, P, name)]["median_us"] / base
        if not args.default_only:
            (d, m) = (out[("group", P, "default")], out[("group", P, "missing_complete")])
            same = all(bool(torch.equal(d[k].view(torch.int64), m[k].view(torch.int64))) for k in ("t", "region", "mt", "mr", "ct", "cr"))
            bits = bool(torch.equal(out[("network", P, "default")]["bits"], out[("network", P, "missing_complete")]["bits"]))
            res["agreement"]["P%d" % P] = {"group_missing_complete_equals_default": same, "bits_missing_complete_equal_default": bits,
                                           "n_controls_all_H": bool((m["nc"] == H).all().item())}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
