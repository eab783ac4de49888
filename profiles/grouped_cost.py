"""
Cost of the grouped tables (lik_grouped_kernel, fcd_lik_sessions.hip) on one MI355X, at cfg3's edges with 100 subjects a side
(Nreg 200: C = 19 900, H = U = 100).

In one process, after a warm-up of every variant, the variants are timed in alternation (HIP events around --launches
back-to-back launches, --rounds rounds).  At K = 1 and K = 4 sessions:
  * fcd_lik_grouped_tables for G = 1, 2, 4, 10 equal groups (patients dealt round-robin) and G = 100 (singletons);
  * fcd_lik_shared_tables_sessions and fcd_lik_tables_sessions of the same data, the two builds the grouped one lies between.
Beside each time: the median over the rounds with the smallest and the largest round (the run-to-run spread), the algorithmic
bytes 8 C (H + U K) + 24 C + 72 C G (+ 4 U + 8 (G + 1) of indices) and the achieved fraction of the HBM peak.  Two
expectations are evaluated from these numbers and written under "expectations":
  G = 1 reads the bytes of the shared build plus the indices: its median lies inside the two builds' own spread;
  G = U writes what the unshared build writes: the ratio of the medians is reported.

    python profiles/grouped_cost.py [--launches 200] [--rounds 7] [--out profiles/grouped_cost.json]

Where the time of G = 1 beyond the shared build goes: profiles/experiments/grouped_ablation.patch gives the kernel switches
that remove, one at a time, what it does beyond the shared kernel (right for ONE group in patient order only, so such a
build is timed with --groups 1, in a process of its own, against the shared build of that same process):
    make -C fcdiff_amd/csrc SUF=.ga2.o LIB=../libfcdiff_hip_ga2.so EXTRA=-DFCD_GROUPED_ABLATE=2
    FCDIFF_HIP_LIB=fcdiff_amd/libfcdiff_hip_ga2.so python profiles/grouped_cost.py --groups 1 --out ...
(profiles/grouped_ablation.txt holds those runs.)

Prints one JSON document (and writes it to --out where given).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal
KS = (1, 4)
GS = (1, 2, 4, 10, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", default=",".join(str(g) for g in GS), help="the numbers of groups to time, e.g. 1")
    args = ap.parse_args()
    import numpy as np
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib
    from fcdiff_amd.fit import group_labels_csr
    torch.cuda.set_device(0)
    groups = tuple(int(g) for g in args.groups.split(","))
    (Nreg, H, U) = (200, 100, 100)
    C = fcdiff_amd.N_to_C(Nreg)
    model = fcdiff_amd.UnsharedRegionModel()
    ctx = _lib.Context()
    (_r, _t, _f, _ft, b, bt4) = model.sample_fast(Nreg, H, U, seed=0, sessions=max(KS))
    b_d = torch.as_tensor(b, device="cuda")
    S_B = torch.empty((C, 3), dtype=torch.float64, device="cuda")
    lM = torch.empty((C, U, 3, 3), dtype=torch.float64, device="cuda")       # the largest output: every variant writes into it
    (th, _th) = _lib.dbl_array(model.theta())
    (P, stream) = (_lib.dptr, _lib.stream_ptr())
    variants = {}
    keep = []

    def add(name, entry, a, nbytes):
        # the library call tables.build makes for this input, its arguments made once: the window times launches, not Python
        variants[name] = (lambda: ctx.call(entry, *a), nbytes)
    for K in KS:
        bt_d = torch.as_tensor(bt4[:, :, :K].copy(), device="cuda")
        keep.append(bt_d)
        read = 8 * C * (H + U * K) + 24 * C
        add("shared_sessions_K%d" % K, "fcd_lik_shared_tables_sessions",
            (P(b_d), P(bt_d), C, H, U, K, th, P(S_B), P(lM), 0, P(None), stream), read + 72 * C)
        add("unshared_sessions_K%d" % K, "fcd_lik_tables_sessions",
            (P(b_d), P(bt_d), C, H, U, K, th, P(S_B), P(lM), P(None), 0, P(None), stream), read + 72 * C * U)
        for G in groups:
            (_names, offsets, order) = group_labels_csr((np.arange(U) % G).tolist(), U)
            (order_d, offsets_d) = (torch.as_tensor(order, device="cuda"), torch.as_tensor(offsets, device="cuda"))
            keep.extend([order_d, offsets_d])
            add("grouped_G%d_K%d" % (G, K), "fcd_lik_grouped_tables",
                (P(b_d), P(bt_d), C, H, U, K, th, P(None), P(None), P(order_d), P(offsets_d), G, P(S_B), P(lM), 0, P(None), stream),
                read + 72 * C * G + 4 * U + 8 * (G + 1))
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's tables
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):                 # alternated: drift of the clock hits all alike
        for (name, (fn, _n)) in variants.items():
            (a, z) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a.record()
            for _i in range(args.launches):
                fn()
            z.record()
            z.synchronize()
            times[name].append(1e3 * a.elapsed_time(z) / args.launches)
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U},
           "library": os.path.basename(_lib.LIB_PATH), "launches_per_round": args.launches, "rounds": args.rounds,
           "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS,
           "note": "us per library call, launches back to back on one stream; us = the median round, min_us / max_us = the "
                   "run-to-run spread, all_us = every round",
           "variants": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = statistics.median(times[name])
        gbs = nbytes / (us * 1e3)
        res["variants"][name] = {"us": us, "min_us": min(times[name]), "max_us": max(times[name]), "all_us": times[name],
                                 "algorithmic_MB": nbytes / 1e6, "GB_per_s": gbs, "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS}
    v = res["variants"]
    res["expectations"] = {}
    for K in KS:
        (sh, un) = (v["shared_sessions_K%d" % K], v["unshared_sessions_K%d" % K])
        e = {"over_shared": {"G%d" % G: v["grouped_G%d_K%d" % (G, K)]["us"] / sh["us"] for G in groups}}
        if 1 in groups:
            g1 = v["grouped_G1_K%d" % K]
            e["G1_over_shared"] = g1["us"] / sh["us"]
            e["G1_inside_the_two_builds_spread"] = bool(sh["min_us"] <= g1["us"] <= sh["max_us"]
                                                        or g1["min_us"] <= sh["us"] <= g1["max_us"])
            e["spread_of_the_two_us"] = [min(g1["min_us"], sh["min_us"]), max(g1["max_us"], sh["max_us"])]
        if U in groups:
            e["GU_over_unshared"] = v["grouped_G%d_K%d" % (U, K)]["us"] / un["us"]
        res["expectations"]["K%d" % K] = e
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
