"""
Cost of nuisance covariates in the permutation baselines (fcd_baseline_group_glm, fcd_baseline_network_bits_glm;
fcd_baseline.hip) on one MI355X, at C = 19 900 connections (200 regions), H = U = 100, P = 1000 and 10 000 permutations
already on the device, Q' = 1, 4 and 8 covariate columns kept (R = Q' + 1 = 2, 5, 9 design columns: the widths 2, 5 and 9).

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around a window of
back-to-back calls, --rounds rounds; best and median round per variant).  Per P, for the group test (one call) and for the
network-based statistic at threshold 3 (the bits call and the components call of one chunk of P permutations):
  default              the call without covariates (fcd_baseline_group_perm, fcd_baseline_network_bits): the yardstick
  glm_q1, glm_q4, glm_q8   the call with a design of R = 2, 5, 9 columns
Under "ratios": every variant over the default of the same run and P.  The MFMA count predicts about R: R accumulators per
group of 16 permutations where the default call has one; the B operand's loads do not grow, the A operand is an 8-byte LDS read
per MFMA in place of a bit.  A record, not a gate.
--default-only times the two default variants alone and binds no call with a design: for a library of the parent commit
(FCDIFF_HIP_LIB), alternated with this one in one session; --guard-dir DIR merges the records guard_<library>_<run>.json such
runs wrote there into "default_path_guard".

    python profiles/baseline_covariates_cost.py [--rounds 7] [--default-only] [--guard-dir DIR] [--out profiles/baseline_covariates_cost.json]
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS = (1000, 10000)
QS = (1, 4, 8)
THRESHOLD = 3.0
GLM_CALLS = ("fcd_baseline_group_glm", "fcd_baseline_network_bits_glm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--guard-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baseline_covariates_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline
    if args.default_only:
        for name in GLM_CALLS:
            _lib.SIGNATURES.pop(name, None)
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    S = H + U
    C = fcdiff_amd.N_to_C(Nreg)
    W = (C + 31) // 32
    rng = np.random.default_rng(0)
    Z = rng.normal(0.0, 1.0, (S, max(QS)))
    Z[H:, 0] += 0.5
    X = rng.normal(0.3, 0.1, (C, S)) + 0.03 * rng.normal(0.0, 1.0, (C, max(QS))).dot(Z.T)
    X[:Nreg - 1, H:] += 0.05
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    (bd, btd) = (dev(X[:, :H]), dev(X[:, H:]))
    ctx = _lib.Context()
    (Pt, stream) = (_lib.dptr, _lib.stream_ptr())
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device="cuda")
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")
    i64 = lambda *sh: torch.empty(sh, dtype=torch.int64, device="cuda")
    perms = dict((P, baseline.draw_permutations(P, S, seed=P)) for P in PS)
    labels = dict((P, dev((perms[P] >= H).astype(np.uint8))) for P in PS)
    permd = dict((P, dev(perms[P].astype(np.uint16).view(np.int16))) for P in PS)
    designs = {}
    if not args.default_only:
        for Q in QS:
            (Wd, info) = baseline.glm_design(Z[:H, :Q], Z[H:, :Q])
            assert info["rank"] == Q
            designs[Q] = dev(Wd)
    out = {}

    def group(P, Q):
        o = out.setdefault(("group", P, Q), dict(t=f64(C), region=f64(Nreg), mt=f64(P), mr=f64(P), ct=i64(C), cr=i64(Nreg)))
        if Q == 0:
            ctx.call("fcd_baseline_group_perm", Pt(bd), Pt(btd), C, H, U, Pt(labels[P]), P, Pt(o["t"]), Pt(o["region"]), Pt(o["mt"]),
                     Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), stream)
        else:
            ctx.call("fcd_baseline_group_glm", Pt(bd), Pt(btd), C, H, U, Pt(designs[Q]), Q + 1, Pt(permd[P]), P, Pt(o["t"]),
                     Pt(o["region"]), Pt(o["mt"]), Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), stream)

    def network(P, Q):
        o = out.setdefault(("network", P, Q), dict(bits=i32(P, W), ne=i32(P), me=i32(P), mg=i32(P)))
        if Q == 0:
            ctx.call("fcd_baseline_network_bits", Pt(bd), Pt(btd), C, H, U, Pt(labels[P]), P, THRESHOLD, 0, Pt(o["bits"]), Pt(None),
                     stream)
        else:
            ctx.call("fcd_baseline_network_bits_glm", Pt(bd), Pt(btd), C, H, U, Pt(designs[Q]), Q + 1, Pt(permd[P]), P, THRESHOLD, 0,
                     Pt(o["bits"]), Pt(None), stream)
        ctx.call("fcd_graph_components", Pt(o["bits"]), P, C, Pt(None), Pt(o["ne"]), Pt(o["me"]), Pt(o["mg"]), stream)

    names = {0: "default"}
    if not args.default_only:
        names.update((Q, "glm_q%d" % Q) for Q in QS)
    variants = {}
    for P in PS:
        for (Q, name) in names.items():
            n = (20 if P <= 1000 else 4) if Q == 0 else (6 if P <= 1000 else 2)
            variants["group_P%d_%s" % (P, name)] = (lambda P=P, Q=Q: group(P, Q), n)
            variants["network_P%d_%s" % (P, name)] = (lambda P=P, Q=Q: network(P, Q), n)
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
           "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U, "columns_kept": list(QS), "threshold": THRESHOLD},
           "rounds": args.rounds, "calls_per_window": dict((k, v[1]) for (k, v) in variants.items()),
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round",
           "variants": {}, "ratios": {}, "predicted_ratio_R": dict(("glm_q%d" % Q, Q + 1) for Q in QS)}
    for name in variants:
        res["variants"][name] = {"us": min(times[name]), "median_us": float(np.median(times[name])), "all_us": times[name]}
    v = res["variants"]
    for P in PS:
        for kind in ("group", "network"):
            base = v["%s_P%d_default" % (kind, P)]["median_us"]
            for (Q, name) in names.items():
                if Q:
                    res["ratios"]["%s_P%d_%s_over_default" % (kind, P, name)] = v["%s_P%d_%s" % (kind, P, name)]["median_us"] / base
    if args.guard_dir:
        runs = []
        for path in sorted(glob.glob(os.path.join(args.guard_dir, "guard_*_*.json"))):
            g = json.load(open(path))
            (lib, run) = os.path.basename(path)[len("guard_"):-len(".json")].rsplit("_", 1)
            runs.append({"library": lib, "run": int(run), "median_us": dict((k, round(x["median_us"], 2)) for (k, x) in g["variants"].items()),
                         "best_us": dict((k, round(x["us"], 2)) for (k, x) in g["variants"].items())})
        res["default_path_guard"] = {"what": "--default-only (%d rounds each) in the same session, the library of the parent commit and "
                                             "this tree's alternated.  The default calls are not supposed to have changed." % args.rounds,
                                     "runs": sorted(runs, key=lambda r: (r["run"], r["library"]))}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
