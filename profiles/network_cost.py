"""
Cost of the network-based statistic (fcd_baseline_network_bits + fcd_graph_components; fcd_baseline.hip) on one MI355X, at
C = 19 900 connections (200 regions), H = U = 100, threshold 3.0.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around a window of
back-to-back calls, --rounds rounds; best and median round per variant):
  network_P{1000,10000}  the device half of baseline.network_test on P drawn labellings already on the device: the observed
                         labelling (bits at P = 1, components with labels) and the P labellings (bits, components without
                         labels) -- four calls of the C ABI, eight launches, no copy to the host
  group_P{1000,10000}    fcd_baseline_group_perm on the same labellings: the edge-wise and region-wise permutation test
  copy_bits_P{...}       a device-to-device copy of the (P, W) bit array: the floor of one pass over what the two halves
                         hand each other
Under "ratios": the network call over the group test at both P (the bits pass does half the group test's MFMA work, so the
expectation was <= 1 at P = 10 000) and over the copy.  A record, not a gate.

The two kernels separately come from a run of their own,
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/network_cost.py --trace-run
(--trace-run: warm-up, then --trace-calls network calls and as many group calls at P = 10 000, nothing else), whose
*_kernel_stats.csv is then merged into the record, per whole call, with
    python profiles/network_cost.py --merge-stats <dir>/.../..._kernel_stats.csv

    python profiles/network_cost.py [--rounds 7] [--out profiles/network_cost.json]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS = (1000, 10000)
THRESHOLD = 3.0
# matched as substrings of the traced names: the shells are templates over the statistic (network_bits_kernel<stat_plain>, ...).
# baseline_group_kernel is what group_perm_kernel was called before the three statistics shared their shells: a library of
# that time is traced with the same script.
KERNELS = ("network_bits_kernel", "graph_components_kernel", "group_centre_kernel", "group_pack_kernel", "group_perm_kernel",
           "baseline_group_kernel", "group_observed_kernel", "group_observed_region_kernel", "group_fold_kernel")


def merge_stats(path, out, calls):
    """Per whole call (the trace run makes `calls` network calls and `calls` group calls) from a rocprofv3 kernel_stats.csv."""
    rows = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if k in row["Name"]:
                    rows[k] = {"launches": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) * 1e-3,
                               "min_us": float(row["MinNs"]) * 1e-3, "max_us": float(row["MaxNs"]) * 1e-3}
    with open(out) as fh:
        res = json.load(fh)
    res["kernel_trace"] = {"note": "rocprofv3 --kernel-trace --stats of --trace-run (its own run): warm-up launches included in "
                                   "launches and total_us; max_us = the launch at P = 10 000, min_us = the observed labelling's",
                           "trace_calls": calls, "kernels": rows}
    with open(out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernel_trace"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_cost.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-calls", type=int, default=10)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out, args.trace_calls)
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    (C, S) = (fcdiff_amd.N_to_C(Nreg), H + U)
    W = (C + 31) // 32
    rng = np.random.default_rng(0)
    b = rng.normal(0.3, 0.1, (C, H))
    bt = rng.normal(0.3, 0.1, (C, U))
    bt[:Nreg - 1] += 0.05
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    (b_d, bt_d) = (dev(b), dev(bt))
    ctx = _lib.Context()
    (Pt, stream) = (_lib.dptr, _lib.stream_ptr())
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device="cuda")
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")
    i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device="cuda")
    labels = {}
    net = {}
    grp = {}
    for P in PS:
        labels[P] = dev(baseline.draw_labels(P, H, U, seed=P))
        net[P] = dict(t=f64(C), bits1=i32(1, W), comp=i32(1, Nreg), o=[i32(1) for _ in range(3)], bits=i32(P, W),
                      copy=i32(P, W), n=[i32(P) for _ in range(3)])
        grp[P] = dict(t=f64(C), region=f64(Nreg), mt=f64(P), mr=f64(P), ct=i64(C), cr=i64(Nreg))

    def network(P):
        o = net[P]
        ctx.call("fcd_baseline_network_bits", Pt(b_d), Pt(bt_d), C, H, U, Pt(None), 1, THRESHOLD, 0, Pt(o["bits1"]), Pt(o["t"]), stream)
        ctx.call("fcd_graph_components", Pt(o["bits1"]), 1, C, Pt(o["comp"]), Pt(o["o"][0]), Pt(o["o"][1]), Pt(o["o"][2]), stream)
        ctx.call("fcd_baseline_network_bits", Pt(b_d), Pt(bt_d), C, H, U, Pt(labels[P]), P, THRESHOLD, 0, Pt(o["bits"]), Pt(None),
                 stream)
        ctx.call("fcd_graph_components", Pt(o["bits"]), P, C, Pt(None), Pt(o["n"][0]), Pt(o["n"][1]), Pt(o["n"][2]), stream)

    def group(P):
        o = grp[P]
        ctx.call("fcd_baseline_group_perm", Pt(b_d), Pt(bt_d), C, H, U, Pt(labels[P]), P, Pt(o["t"]), Pt(o["region"]),
                 Pt(o["mt"]), Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), stream)

    if args.trace_run:
        for fn in (network, group):
            for _ in range(3):
                fn(PS[-1])
        torch.cuda.synchronize()
        for fn in (network, group):
            for _ in range(args.trace_calls):
                fn(PS[-1])
        torch.cuda.synchronize()
        return
    variants = {}
    for P in PS:
        variants["network_P%d" % P] = (lambda P=P: network(P), 20 if P <= 1000 else 5)
        variants["group_P%d" % P] = (lambda P=P: group(P), 20 if P <= 1000 else 5)
        variants["copy_bits_P%d" % P] = (lambda P=P: net[P]["copy"].copy_(net[P]["bits"]), 200)
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's workspace
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
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U, "W": W},
           "threshold": THRESHOLD, "rounds": args.rounds, "calls_per_window": dict((k, v[1]) for (k, v) in variants.items()),
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round",
           "variants": {}, "ratios": {}, "results": {}}
    for name in variants:
        res["variants"][name] = {"us": min(times[name]), "median_us": float(np.median(times[name])), "all_us": times[name]}
    v = res["variants"]
    for P in PS:
        v["copy_bits_P%d" % P]["bytes"] = 4 * P * W
        res["ratios"]["network_over_group_P%d" % P] = v["network_P%d" % P]["median_us"] / v["group_P%d" % P]["median_us"]
        res["ratios"]["network_over_copy_bits_P%d" % P] = v["network_P%d" % P]["median_us"] / v["copy_bits_P%d" % P]["median_us"]
        o = net[P]
        res["results"]["P%d" % P] = {"observed_n_edges": int(o["o"][0].item()), "observed_max_extent": int(o["o"][1].item()),
                                     "null_n_edges_mean": float(o["n"][0].double().mean().item()),
                                     "null_max_extent_max": int(o["n"][1].max().item()),
                                     "null_max_regions_max": int(o["n"][2].max().item())}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
