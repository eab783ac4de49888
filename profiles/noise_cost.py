"""
Cost of the measurement-noise tables (fcd_lik_sessions.hip) on one MI355X, at cfg3's shape (Nreg 200, H = U = 50).

In one process, after a warm-up of every variant, the variants are timed in alternation (HIP events around --launches
back-to-back calls, --rounds rounds, best round per variant), at K = 1, 2, 4, 8:
  * fcd_lik_tables_noise with var_b and var_bt (two launches per call: the records, then the tables) beside the existing
    build of the same input -- fcd_lik_tables_ex on the 2-D bt at K = 1, fcd_lik_tables_sessions at K >= 2;
  * fcd_lik_shared_tables_noise beside fcd_lik_shared_tables / fcd_lik_shared_tables_sessions;
  * fcd_conn_posterior_noise beside fcd_conn_posterior_sessions (mean-field weights).
Beside each time: the algorithmic bytes 8 C (H + U K) + 24 C + 72 C U (shared: 72 C) of a build and the achieved fraction
of the HBM peak.  Under "ratios": noise over existing per K, and whether the unshared ratio is within the 1.15 the change
expected (a larger ratio is a finding to report, not a failure).

    python profiles/noise_cost.py [--launches 200] [--rounds 7] [--out profiles/noise_cost.json]

Prints one JSON document (and writes it to --out where given).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal
KS = (1, 2, 4, 8)
MARGIN = 1.15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 50, 50)
    C = fcdiff_amd.N_to_C(Nreg)
    model = fcdiff_amd.UnsharedRegionModel()
    (th, _th) = _lib.dbl_array(model.theta())
    ctx = _lib.Context()
    (_r, _t, _f, _ft, b, bt8) = model.sample_fast(Nreg, H, U, seed=0, sessions=max(KS))
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    b_d = dev(b)
    vb_d = dev(rng.uniform(0, 0.02, H))
    S_B = torch.empty((C, 3), dtype=torch.float64, device="cuda")
    lM = torch.empty((C, U, 3, 3), dtype=torch.float64, device="cuda")
    L = torch.empty((C, 1, 3, 3), dtype=torch.float64, device="cuda")
    lq_F = torch.full((C, 1, 3), -np.log(3), dtype=torch.float64, device="cuda")
    lq_R = torch.full((Nreg, U, 2), -np.log(2), dtype=torch.float64, device="cuda")
    post = [torch.empty((C, U), dtype=torch.float64, device="cuda"), torch.empty((C, U, 3), dtype=torch.float64, device="cuda"),
            torch.empty((C, U), dtype=torch.float64, device="cuda")]
    (P, stream) = (_lib.dptr, _lib.stream_ptr())
    variants = {}
    keep = []

    def add(name, entry, a, nbytes):
        variants[name] = (lambda: ctx.call(entry, *a), nbytes)

    for K in KS:
        btk = dev(bt8[:, :, :K])
        bt2 = dev(bt8[:, :, 0])
        vbt = dev(rng.uniform(0, 0.02, (U, K)))
        keep.extend([btk, bt2, vbt])
        nb = 8 * C * (H + U * K) + 24 * C + 72 * C * U
        nb_s = 8 * C * (H + U * K) + 24 * C + 72 * C
        nb_p = 8 * C * U * K + 40 * C * U
        add("noise_K%d" % K, "fcd_lik_tables_noise",
            (P(b_d), P(btk), C, H, U, K, th, P(vb_d), P(vbt), P(S_B), P(lM), P(None), 0, P(None), stream), nb)
        add("shared_noise_K%d" % K, "fcd_lik_shared_tables_noise",
            (P(b_d), P(btk), C, H, U, K, th, P(vb_d), P(vbt), P(S_B), P(L), 0, P(None), stream), nb_s)
        add("posterior_noise_K%d" % K, "fcd_conn_posterior_noise",
            (P(btk), Nreg, U, K, th, P(vbt), P(None), P(lq_F), P(lq_R), 0, P(post[0]), P(post[1]), P(post[2]), stream), nb_p)
        if K == 1:
            add("existing_K1", "fcd_lik_tables_ex",
                (P(b_d), P(bt2), C, H, U, th, P(S_B), P(lM), P(None), P(None), 0, P(None), stream), nb)
            add("shared_existing_K1", "fcd_lik_shared_tables", (P(b_d), P(bt2), C, H, U, th, P(S_B), P(L), 0, P(None), stream), nb_s)
        else:
            add("existing_K%d" % K, "fcd_lik_tables_sessions",
                (P(b_d), P(btk), C, H, U, K, th, P(S_B), P(lM), P(None), 0, P(None), stream), nb)
            add("shared_existing_K%d" % K, "fcd_lik_shared_tables_sessions",
                (P(b_d), P(btk), C, H, U, K, th, P(S_B), P(L), 0, P(None), stream), nb_s)
        add("posterior_existing_K%d" % K, "fcd_conn_posterior_sessions",
            (P(btk), Nreg, U, K, th, P(None), P(lq_F), P(lq_R), 0, P(post[0]), P(post[1]), P(post[2]), stream), nb_p)
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's tables and record block
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
           "launches_per_round": args.launches, "rounds": args.rounds, "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS,
           "records": "max(H, U K) = %s per K, all <= NOISE_LDS_RECORDS = %d: read from LDS" % (
               [max(H, U * K) for K in KS], tables.NOISE_LDS_RECORDS),
           "note": "us per library call, calls back to back on one stream, best round; all_us = every round.  A noise call "
                   "is two launches (records, tables); an existing call is one.",
           "variants": {}, "ratios": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = min(times[name])
        gbs = nbytes / (us * 1e3)
        res["variants"][name] = {"us": us, "all_us": times[name], "algorithmic_MB": nbytes / 1e6, "GB_per_s": gbs,
                                 "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS}
    v = res["variants"]
    for K in KS:
        r = v["noise_K%d" % K]["us"] / v["existing_K%d" % K]["us"]
        res["ratios"]["K%d" % K] = {"noise_over_existing": r, "within_%.2f" % MARGIN: bool(r <= MARGIN),
                                    "shared_noise_over_existing": v["shared_noise_K%d" % K]["us"] / v["shared_existing_K%d" % K]["us"],
                                    "posterior_noise_over_sessions":
                                        v["posterior_noise_K%d" % K]["us"] / v["posterior_existing_K%d" % K]["us"]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
