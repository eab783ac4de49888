"""
Cost of the two passes of the subtype-region model over the per-patient table (fcd_lik_weighted_tables,
fcd_vb_subtype_loglik; fcd_subtype.hip) on one MI355X, at C = 19 900 connections (200 regions), U = 100 patients,
G = 2 / 4 / 8 subtypes.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around --launches
back-to-back calls, --rounds rounds; best and median round per variant):
  weighted_G{G}        fcd_lik_weighted_tables: lM (C, U, 3, 3) read once, L (C, G, 3, 3) written
  loglik_G{G}          fcd_vb_subtype_loglik (three launches: the exponentials, the edge slices, the fold): lM read once
  patient_elbo_xG{G}   G calls of fcd_vb_patient_elbo with a (Nreg, U, 2) q_R each: what E[u, g] costs on the existing kernel,
                       lM read G times
  copy_lM              a device-to-device copy of lM's bytes: the floor of one pass over the table
  iteration_G{G}       one outer iteration of SubtypeRegionFit (q_F, q_R, pi and gamma, responsibilities, L, energy), host
                       steps and read-backs included; --launches / 10 per round
Beside each time the algorithmic bytes and the rate they give.  Under "ratios" per G: both kernels over the copy, and
loglik over the G patient_elbo calls.

ONE condition, derived from traffic and not from a measurement: at G = 4 fcd_vb_subtype_loglik takes less than half the
time of the four fcd_vb_patient_elbo calls of the same run (it reads lM once where they read it four times; the factor 2
is slack for its extra arithmetic).  "condition_holds" records it and the script exits 1 where it does not.  Everything else
is a record, not a gate.

    python profiles/subtype_cost.py [--launches 200] [--rounds 7] [--out profiles/subtype_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GS = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subtype_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, tables
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    C = fcdiff_amd.N_to_C(Nreg)
    model = fcdiff_amd.SubtypeRegionModel()
    ctx = _lib.Context()
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    (P, stream) = (_lib.dptr, _lib.stream_ptr())
    variants = {}
    keep = []
    fits = {}
    lM = None
    for G in GS:
        model.n_subtypes = G
        (_z, _r, _t, _f, _ft, b, bt) = model.sample(Nreg, H, U, seed=0)
        fit = fcdiff_amd.fit.SubtypeRegionFit()
        (fit._ctx, fit.model, fit.b, fit.bt, fit.n_subtypes) = (ctx, fcdiff_amd.SubtypeRegionModel(), b, bt, G)
        (fit.max_iters, fit.n_restarts, fit.rel_tol) = (2, 1, -np.inf)
        fit.run()                                    # the state one iteration works on: tables, q_F, q_R, responsibilities
        fits[G] = fit
        lM = fit._d["lM_u"]
        resp = dev(rng.dirichlet(np.ones(G), size=U))
        L = torch.empty((C, G, 3, 3), dtype=torch.float64, device="cuda")
        E = torch.empty((U, G), dtype=torch.float64, device="cuda")
        (lq_F, lq_R) = (fit._d["lq_F"], fit._d["lq_R"])
        cols = [lq_R[:, g:g + 1, :].expand(Nreg, U, 2).contiguous() for g in range(G)]
        out4 = torch.empty((U, 4), dtype=torch.float64, device="cuda")
        hyper = fit._hyper()
        keep.extend([resp, L, E, cols, out4, lM])
        variants["weighted_G%d" % G] = (
            lambda a=(P(lM), P(resp), C, U, G, P(L), stream): ctx.call("fcd_lik_weighted_tables", *a), 72 * C * U + 72 * C * G)
        variants["loglik_G%d" % G] = (
            lambda a=(P(lq_F), P(lq_R), P(lM), Nreg, U, G, P(E), stream): ctx.call("fcd_vb_subtype_loglik", *a), 72 * C * U)
        variants["patient_elbo_xG%d" % G] = (
            lambda a=[(P(lq_F), P(c), P(lM), P(hyper), Nreg, U, P(out4), stream) for c in cols]:
            [ctx.call("fcd_vb_patient_elbo", *x) for x in a], 72 * C * U * G)

        def iteration(fit=fit):
            fit._update_lq_F()
            fit._update_lq_R()
            fit._update_theta()
            fit._update_responsibilities()
            fit._update_weighted_table()
            fit._eval_energy()
        variants["iteration_G%d" % G] = (iteration, 0)
    dst = torch.empty_like(lM)
    variants["copy_lM"] = (lambda: dst.copy_(lM), 2 * 72 * C * U)
    for (fn, _n) in variants.values():               # warm-up: code objects, the context's workspace
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):                     # alternated: drift of the clock hits all alike
        for (name, (fn, _n)) in variants.items():
            n = max(1, args.launches // 10) if name.startswith("iteration") else args.launches
            (a, z) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a.record()
            for _i in range(n):
                fn()
            z.record()
            z.synchronize()
            times[name].append(1e3 * a.elapsed_time(z) / n)
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U, "G": list(GS)},
           "launches_per_round": args.launches, "rounds": args.rounds,
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round.  A loglik "
                   "call is three launches, a patient_elbo_xG entry G calls of two launches; an iteration includes its host "
                   "steps and read-backs.  lM is 143 MB, less than the 256 MB Infinity Cache, and every call reads it again: part of it may come from that "
                   "cache (no counters were read), so the rates are rates of algorithmic bytes, not measured HBM rates.",
           "variants": {}, "ratios": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = min(times[name])
        res["variants"][name] = {"us": us, "median_us": float(np.median(times[name])), "all_us": times[name]}
        if nbytes:
            res["variants"][name].update({"algorithmic_MB": nbytes / 1e6, "GB_per_s": nbytes / (us * 1e3)})
    v = res["variants"]
    for G in GS:
        res["ratios"]["G%d" % G] = {
            "weighted_over_copy_lM": v["weighted_G%d" % G]["median_us"] / v["copy_lM"]["median_us"],
            "loglik_over_copy_lM": v["loglik_G%d" % G]["median_us"] / v["copy_lM"]["median_us"],
            "loglik_over_patient_elbo_calls": v["loglik_G%d" % G]["median_us"] / v["patient_elbo_xG%d" % G]["median_us"],
            "kernels_share_of_iteration": (v["weighted_G%d" % G]["median_us"] + v["loglik_G%d" % G]["median_us"])
            / v["iteration_G%d" % G]["median_us"]}
    res["condition"] = "loglik_G4 median_us < 0.5 * patient_elbo_xG4 median_us"
    res["condition_holds"] = bool(v["loglik_G4"]["median_us"] < 0.5 * v["patient_elbo_xG4"]["median_us"])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if res["condition_holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
