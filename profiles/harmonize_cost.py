"""
Cost of the site harmonisation (fcd_site_harmonize_fit, fcd_site_harmonize_apply; fcd_harmonize.hip) on one MI355X, at
C = 19 900 connections (200 regions), H = U = 100, B = 2 / 4 / 16 sites, Q = 0 / 4 covariate columns, and at Q = 0 with 0 % and
5 % of b set to NaN.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around --launches
back-to-back calls, --rounds rounds; best and median round per variant):
  fit_B{B}_Q{Q}_nan{0,5}   fcd_site_harmonize_fit on b (C, H) (nan5: with FCD_DATA_NAN_MISSING; Q = 0 only)
  apply_B{B}_Q{Q}          fcd_site_harmonize_apply on bt (C, U)
  dummies_B{B}_Q{Q}_nan{n} fcd_edge_cov_fit on the same b with B - 1 site dummies plus the Q columns: the nearest existing way
                           to take site means out (not for B = 16 with Q = 4: 19 columns, it takes 16)
  lik_tables_nan{0,5}      fcd_lik_tables_ex on the same b and bt, the build a fit makes from them
  copy_b                   a device-to-device copy of the bytes of b: the floor of a pass over the data
Under "ratios": every fit over copy_b, over lik_tables and over the dummy-coded fcd_edge_cov_fit of the same run, and apply
over copy_b.  A record, not a gate: no time was set for these kernels.

    python profiles/harmonize_cost.py [--launches 200] [--rounds 7] [--out profiles/harmonize_cost.json]
    python profiles/harmonize_cost.py --one-call 4 0      one warm and one traced fit + apply, for a kernel trace
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS = (2, 4, 16)
QS = (0, 4)
NANS = (0, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmonize_cost.json"))
    ap.add_argument("--one-call", type=int, nargs=2, metavar=("B", "Q"), default=None)
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, covariates
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
    S_B = torch.empty((C, 3), dtype=torch.float64, device="cuda")
    lM = torch.empty((C, U, 3, 3), dtype=torch.float64, device="cuda")
    out = torch.empty((C, U), dtype=torch.float64, device="cuda")
    rv = torch.empty((C,), dtype=torch.float64, device="cuda")
    info = torch.empty((C, 4), dtype=torch.int32, device="cuda")
    dst = torch.empty((C, H), dtype=torch.float64, device="cuda")
    (P, stream, FLAG) = (_lib.dptr, _lib.stream_ptr(), _lib.FCD_DATA_NAN_MISSING)
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    variants = {}
    keep = []

    def harmonize_variants(B, Q):
        idx = (np.arange(H) % B).astype(np.uint8)
        idx_t = (np.arange(U) % B).astype(np.uint8)
        z = rng.standard_normal((H, Q))
        (W, T, z_bar, _i) = covariates.site_design(z, idx, B)
        z_ref = np.ascontiguousarray(z.mean(axis=0))
        o = dict(grand_mean=torch.empty((C,), **f64), pooled_sd=torch.empty((C,), **f64), beta=torch.empty((C, max(Q, 1)), **f64),
                 n_obs=torch.empty((B, C), **i32), n_iter=torch.empty((B, C), **i32), info=torch.empty((C, 4), **i32),
                 prior=torch.empty((6, B), **f64), prior_info=torch.empty((B, 3), **i32))
        for k in ("gamma_hat", "delta2_hat", "gamma_star", "delta2_star", "shift", "scale"):
            o[k] = torch.empty((B, C), **f64)
        dv = dict(site=dev(idx), site_t=dev(idx_t), W=dev(W) if Q else None, z_t=dev(rng.standard_normal((U, Q))) if Q else None)
        host = dict(T=T.ctypes.data if Q else None, z_bar=z_bar.ctypes.data if Q else None, z_ref=z_ref.ctypes.data if Q else None)
        keep.extend([o, dv, W, T, z_bar, z_ref])
        made = {}
        for nan in NANS if Q == 0 else (0,):
            d = _lib.HarmonizeDesc.make(flags=FLAG if nan else 0, C=C, H=H, B=B, Q=Q, Qp=W.shape[1], stream=stream, b=P(b_d[nan]),
                                        site=P(dv["site"]), W=P(dv["W"]), **dict(host, **dict((k, P(v)) for (k, v) in o.items())))
            keep.append(d)
            made["fit_B%d_Q%d_nan%d" % (B, Q, nan)] = (
                lambda d=d: ctx.call("fcd_site_harmonize_fit", ctypes.byref(d)),
                8 * C * H + 8 * C * (2 + Q) + 16 * C + (6 * 8 + 2 * 4) * B * C)
        d = _lib.HarmonizeDesc.make(C=C, S=U, B=B, Q=Q, stream=stream, x=P(bt_d), site=P(dv["site_t"]), z=P(dv["z_t"]), z_ref=host["z_ref"],
                                    grand_mean=P(o["grand_mean"]), beta=P(o["beta"]), shift=P(o["shift"]), scale=P(o["scale"]), out=P(out))
        keep.append(d)
        made["apply_B%d_Q%d" % (B, Q)] = (lambda d=d: ctx.call("fcd_site_harmonize_apply", ctypes.byref(d)),
                                          16 * C * U + 8 * C * (1 + Q) + 16 * B * C)
        # the dummy-coded covariate fit of the same sites and columns
        Qd = B - 1 + Q
        if Qd <= covariates.MAX_COLUMNS:
            zd = dev(np.concatenate([(idx[:, None] == np.arange(1, B)[None, :]).astype(np.float64), z], axis=1))
            beta = torch.empty((C, Qd), **f64)
            keep.extend([zd, beta])
            for nan in NANS if Q == 0 else (0,):
                made["dummies_B%d_Q%d_nan%d" % (B, Q, nan)] = (
                    lambda a=(P(b_d[nan]), C, H, P(zd), Qd, FLAG if nan else 0, P(beta), P(rv), P(info), stream): ctx.call("fcd_edge_cov_fit", *a),
                    8 * C * H + 8 * C * Qd + 8 * C + 16 * C)
        return made

    if args.one_call:
        made = harmonize_variants(*args.one_call)
        for _ in range(2):
            for (fn, _n) in made.values():
                fn()
            torch.cuda.synchronize()
        return
    for B in BS:
        for Q in QS:
            variants.update(harmonize_variants(B, Q))
    for nan in NANS:
        variants["lik_tables_nan%d" % nan] = (
            lambda a=(P(b_d[nan]), P(bt_d), C, H, U, th, P(S_B), P(lM), P(None), P(None), FLAG, P(None), stream):
            ctx.call("fcd_lik_tables_ex", *a), 8 * C * (H + U) + 24 * C + 72 * C * U)
    variants["copy_b"] = (lambda: dst.view(-1).copy_(b_d[0].view(-1)), 16 * C * H)
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's workspace
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ctx.check_device()
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
           "launches_per_round": args.launches, "rounds": args.rounds,
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round.  A "
                   "harmonisation fit is three launches (rows, priors, empirical Bayes) plus one per 128 doubles of the design's "
                   "small arrays at Q > 0; a dummy-coded fit two; the others one.",
           "variants": {}, "ratios": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = min(times[name])
        res["variants"][name] = {"us": us, "median_us": float(np.median(times[name])), "all_us": times[name],
                                 "algorithmic_MB": nbytes / 1e6, "GB_per_s": nbytes / (us * 1e3)}
    v = res["variants"]
    med = lambda name: v[name]["median_us"]
    for name in variants:
        if name.startswith("fit_"):
            tail = name[len("fit_"):]
            nan = tail[-1]
            r = {"over_copy_b": med(name) / med("copy_b"), "over_lik_tables": med(name) / med("lik_tables_nan" + nan)}
            r["over_dummy_coded_edge_cov_fit"] = med(name) / med("dummies_" + tail) if "dummies_" + tail in v else None
            res["ratios"][name] = r
        elif name.startswith("apply_"):
            res["ratios"][name] = {"over_copy_b": med(name) / med("copy_b"), "over_lik_tables": med(name) / med("lik_tables_nan0")}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
