"""
Cost of the covariate adjustment (fcd_edge_cov_fit, fcd_edge_cov_apply; fcd_covariates.hip) on one MI355X, at
C = 19 900 connections (200 regions), H = U = 100, Q = 1 / 4 / 16 covariate columns, with 0 % and 5 % of b set to NaN.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around --launches
back-to-back calls, --rounds rounds; best and median round per variant):
  fit_Q{Q}_nan{0,5}    fcd_edge_cov_fit on b (C, H) with FCD_DATA_NAN_MISSING (two launches: the all-controls design, the rows)
  apply_Q{Q}           fcd_edge_cov_apply on bt (C, U)
  lik_tables_nan{0,5}  fcd_lik_tables_ex on the same b and bt (FCD_DATA_NAN_MISSING), the build a fit makes from them
  copy_b, copy_b_bt    a device-to-device copy of the bytes of b, and of b and bt: the floor of a pass over the data
Beside each time the algorithmic bytes (fit: b once, beta, resid_var and info written; apply: bt read and written, beta read)
and the rate they give.  Under "ratios": fit and apply over lik_tables of the same NaN share and over the copies.
A record, not a gate: no target was set for these kernels.

    python profiles/covariates_cost.py [--launches 200] [--rounds 7] [--out profiles/covariates_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QS = (1, 4, 16)
NANS = (0, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariates_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    C = fcdiff_amd.N_to_C(Nreg)
    model = fcdiff_amd.UnsharedRegionModel()
    (th, _th) = _lib.dbl_array(model.theta())
    ctx = _lib.Context()
    (_r, _t, _f, _ft, b, bt) = model.sample_fast(Nreg, H, U, seed=0)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    b = np.array(b, dtype=np.float64)
    b5 = b.copy()
    b5[rng.random(b.shape) < 0.05] = np.nan
    b_d = {0: dev(b), 5: dev(b5)}
    bt_d = dev(np.array(bt, dtype=np.float64))
    rows_with_nan = int(np.isnan(b5).any(axis=1).sum())
    S_B = torch.empty((C, 3), dtype=torch.float64, device="cuda")
    lM = torch.empty((C, U, 3, 3), dtype=torch.float64, device="cuda")
    out = torch.empty((C, U), dtype=torch.float64, device="cuda")
    rv = torch.empty((C,), dtype=torch.float64, device="cuda")
    info = torch.empty((C, 4), dtype=torch.int32, device="cuda")
    dst = torch.empty((C, H + U), dtype=torch.float64, device="cuda")
    (P, stream, FLAG) = (_lib.dptr, _lib.stream_ptr(), _lib.FCD_DATA_NAN_MISSING)
    variants = {}
    keep = []
    for Q in QS:
        z_b = dev(rng.standard_normal((H, Q)))
        z_bt = dev(rng.standard_normal((U, Q)) + 0.5)
        z_ref = dev(np.zeros(Q))
        beta = torch.empty((C, Q), dtype=torch.float64, device="cuda")
        keep.extend([z_b, z_bt, z_ref, beta])
        for nan in NANS:
            variants["fit_Q%d_nan%d" % (Q, nan)] = (
                lambda a=(P(b_d[nan]), C, H, P(z_b), Q, FLAG, P(beta), P(rv), P(info), stream): ctx.call("fcd_edge_cov_fit", *a),
                8 * C * H + 8 * C * Q + 8 * C + 16 * C)
        variants["apply_Q%d" % Q] = (
            lambda a=(P(bt_d), C, U, P(z_bt), Q, P(z_ref), P(beta), P(out), stream): ctx.call("fcd_edge_cov_apply", *a),
            16 * C * U + 8 * C * Q)
    for nan in NANS:
        variants["lik_tables_nan%d" % nan] = (
            lambda a=(P(b_d[nan]), P(bt_d), C, H, U, th, P(S_B), P(lM), P(None), P(None), FLAG, P(None), stream):
            ctx.call("fcd_lik_tables_ex", *a), 8 * C * (H + U) + 24 * C + 72 * C * U)
    variants["copy_b"] = (lambda: dst.view(-1)[:C * H].copy_(b_d[0].view(-1)), 16 * C * H)
    variants["copy_b_bt"] = (lambda: (dst.view(-1)[:C * H].copy_(b_d[0].view(-1)), dst.view(-1)[C * H:].copy_(bt_d.view(-1))),
                             16 * C * (H + U))
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's workspace
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
           "launches_per_round": args.launches, "rounds": args.rounds, "rows_with_nan_at_5_percent": rows_with_nan,
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round.  A fit "
                   "call is two launches, copy_b_bt two copies; the others one.",
           "variants": {}, "ratios": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = min(times[name])
        res["variants"][name] = {"us": us, "median_us": float(np.median(times[name])), "all_us": times[name],
                                 "algorithmic_MB": nbytes / 1e6, "GB_per_s": nbytes / (us * 1e3)}
    v = res["variants"]
    for Q in QS:
        r = {}
        for nan in NANS:
            fit = v["fit_Q%d_nan%d" % (Q, nan)]["median_us"]
            r["fit_nan%d_over_lik_tables" % nan] = fit / v["lik_tables_nan%d" % nan]["median_us"]
            r["fit_nan%d_over_copy_b" % nan] = fit / v["copy_b"]["median_us"]
        r["apply_over_lik_tables"] = v["apply_Q%d" % Q]["median_us"] / v["lik_tables_nan0"]["median_us"]
        r["apply_over_copy_b"] = v["apply_Q%d" % Q]["median_us"] / v["copy_b"]["median_us"]
        r["fit_nan5_plus_two_applies_over_lik_tables"] = (
            (v["fit_Q%d_nan5" % Q]["median_us"] + 2 * v["apply_Q%d" % Q]["median_us"]) / v["lik_tables_nan5"]["median_us"])
        res["ratios"]["Q%d" % Q] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
