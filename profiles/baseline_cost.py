"""
Cost of the classical baselines (fcd_baseline_normative, fcd_baseline_group_perm; fcd_baseline.hip) on one MI355X, at
C = 19 900 connections (200 regions), H = U = 100.

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around a window of
back-to-back calls, --rounds rounds; best and median round per variant):
  normative            fcd_baseline_normative without z / z0 (one launch)
  normative_z          ... with z (C, U) and z0 (C, H) written
  group_P{1000,10000}  fcd_baseline_group_perm on P drawn labellings already on the device (six launches, two memsets)
  torch_P{1000,10000}  the same permutation statistics written with torch ops on the device, what one would write without the
                       kernel: rows centred, fp64 matmul labels (P, S) x X^T (S, C), elementwise t^2, index_add_ into the
                       regions, amax, exceedance counts -- a (P, C) array in memory several times over
  copy_b_bt            a device-to-device copy of the bytes of b and bt: the floor of one pass over the data
Under "ratios": the fused call over the torch formulation at both P (the aim was <= 1 at P = 10 000), the normative call over
the copy (it reads every row twice), and the share of the fp64 MFMA peak the fused call's 2 x 2 P C S flop amount to (every
connection is multiplied once per endpoint).  Under "agreement": the torch and the fused statistics of the timed inputs
compared.  A record, not a gate.

    python profiles/baseline_cost.py [--rounds 7] [--out profiles/baseline_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS = (1000, 10000)
MFMA_F64_PEAK = 77.9e12          # v_mfma_f64_16x16x4_f64 back to back on this chip, flop/s (r02_ubench_mfma64.txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baseline_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline, util
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    (C, S) = (fcdiff_amd.N_to_C(Nreg), H + U)
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

    # normative
    nv = dict(msq0=f64(Nreg, H), ne0=i32(Nreg, H), no0=i32(Nreg, H), msq=f64(Nreg, U), ne=i32(Nreg, U), no=i32(Nreg, U),
              nc=i32(C), z0=f64(C, H), z=f64(C, U))

    def normative(with_z):
        ctx.call("fcd_baseline_normative", Pt(b_d), Pt(bt_d), C, H, U, 3.0, Pt(nv["msq0"]), Pt(nv["ne0"]), Pt(nv["no0"]),
                 Pt(nv["msq"]), Pt(nv["ne"]), Pt(nv["no"]), Pt(nv["nc"]), Pt(nv["z0"] if with_z else None),
                 Pt(nv["z"] if with_z else None), stream)

    # group test: fused and torch
    nm = np.array([util.c_to_nm(c) for c in range(C)], dtype=np.int64)
    (idx_n, idx_m) = (dev(nm[:, 0]), dev(nm[:, 1]))
    observed = torch.zeros((1, S), dtype=torch.float64, device="cuda")
    observed[0, H:] = 1.0
    (kf, dof) = (S / (U * H), S - 2.0)
    fused_out = {}
    torch_out = {}
    labels = {}
    for P in PS:
        lab = dev(baseline.draw_labels(P, H, U, seed=P))
        labels[P] = (lab, lab.to(torch.float64))
        fused_out[P] = dict(t=f64(C), region=f64(Nreg), mt=f64(P), mr=f64(P), ct=i64(C), cr=i64(Nreg))

    def fused(P):
        o = fused_out[P]
        ctx.call("fcd_baseline_group_perm", Pt(b_d), Pt(bt_d), C, H, U, Pt(labels[P][0]), P, Pt(o["t"]), Pt(o["region"]),
                 Pt(o["mt"]), Pt(o["mr"]), Pt(o["ct"]), Pt(o["cr"]), stream)

    def t2_of(lab64, xc, q):
        g = torch.matmul(lab64, xc.t())
        g = g * g * kf
        return g * dof / (q[None, :] - g)

    def regions_of(t2):
        R = torch.zeros((t2.shape[0], Nreg), dtype=torch.float64, device="cuda")
        R.index_add_(1, idx_n, t2)
        R.index_add_(1, idx_m, t2)
        return R

    def by_torch(P):
        x = torch.cat([b_d, bt_d], dim=1)
        xc = x - x.mean(dim=1, keepdim=True)
        q = (xc * xc).sum(dim=1)
        t2o = t2_of(observed, xc, q)
        Ro = regions_of(t2o)
        t2 = t2_of(labels[P][1], xc, q)
        R = regions_of(t2)
        torch_out[P] = dict(t2=t2o[0], region=Ro[0], mt=t2.amax(dim=1).sqrt(), mr=R.amax(dim=1), ct=(t2 >= t2o).sum(dim=0),
                            cr=(R >= Ro).sum(dim=0))

    dst = f64(C, S)

    def copy():
        dst.view(-1)[:C * H].copy_(b_d.view(-1))
        dst.view(-1)[C * H:].copy_(bt_d.view(-1))

    # name -> (call, calls per timed window)
    variants = {"normative": (lambda: normative(False), 50), "normative_z": (lambda: normative(True), 50),
                "copy_b_bt": (copy, 200)}
    for P in PS:
        variants["group_P%d" % P] = (lambda P=P: fused(P), 20 if P <= 1000 else 5)
        variants["torch_P%d" % P] = (lambda P=P: by_torch(P), 10 if P <= 1000 else 3)
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
    res = {"device": torch.cuda.get_device_name(0), "shape": {"Nreg": Nreg, "C": C, "H": H, "U": U},
           "rounds": args.rounds, "calls_per_window": dict((k, v[1]) for (k, v) in variants.items()),
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round",
           "variants": {}, "ratios": {}, "agreement": {}}
    for name in variants:
        res["variants"][name] = {"us": min(times[name]), "median_us": float(np.median(times[name])), "all_us": times[name]}
    v = res["variants"]
    copy_bytes = 16 * C * S
    v["copy_b_bt"]["GB_per_s"] = copy_bytes / (v["copy_b_bt"]["median_us"] * 1e3)
    res["ratios"]["normative_over_copy_b_bt"] = v["normative"]["median_us"] / v["copy_b_bt"]["median_us"]
    res["ratios"]["normative_z_over_copy_b_bt"] = v["normative_z"]["median_us"] / v["copy_b_bt"]["median_us"]
    for P in PS:
        res["ratios"]["group_over_torch_P%d" % P] = v["group_P%d" % P]["median_us"] / v["torch_P%d" % P]["median_us"]
        flop = 2.0 * 2.0 * P * C * S
        v["group_P%d" % P]["mfma_flop"] = flop
        v["group_P%d" % P]["share_of_fp64_mfma_peak"] = flop / (v["group_P%d" % P]["median_us"] * 1e-6) / MFMA_F64_PEAK
        (f, t) = (fused_out[P], torch_out[P])
        rel = lambda x, y: float(((x - y).abs() / y.abs()).max().item())
        res["agreement"]["P%d" % P] = {
            "t2_max_rel": rel(f["t"] * f["t"], t["t2"]), "region_max_rel": rel(f["region"], t["region"]),
            "null_max_t_max_rel": rel(f["mt"], t["mt"]), "null_max_region_max_rel": rel(f["mr"], t["mr"]),
            "count_t_differ": int((f["ct"] != t["ct"]).sum().item()), "count_region_differ": int((f["cr"] != t["cr"]).sum().item())}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
