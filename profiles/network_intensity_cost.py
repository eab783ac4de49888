"""
Cost of the intensity form of the network-based statistic (fcd_baseline_network_excess + fcd_graph_components_weighted) against
the extent form (fcd_baseline_network_bits + fcd_graph_components) on one MI355X, by the method of profiles/network_cost.py:
C = 19 900 connections (200 regions), H = U = 100, P = 1000 and 10 000 drawn labellings already on the device, thresholds 3.0
(about 0.3 % of the bits set under the null) and 1.5 (about 13 %).

In one process, after a warm-up of every variant, the variants are timed in alternation (device events around a window of
back-to-back calls, --rounds rounds; best and median round per variant):
  extent_P{..}_thr{..}     the device half of baseline.network_test(statistic="extent"): four calls of the C ABI
  intensity_P{..}_thr{..}  the device half of statistic="intensity": the observed labelling, then the labellings in chunks whose
                           (n, 32 W) excess values stay within baseline._X_BYTES (256 MB: six chunks at P = 10 000), the buffer
                           allocated once outside the window
  parent_P{..}_thr3.0      the extent calls through another build of the library (--parent-lib: the parent commit's), loaded
                           beside this one in the same process: the default path must sit within the spread of the rounds
Under "ratios": intensity over extent per (P, threshold), and this build's extent call over the parent's.  A record, not a gate.

The kernels separately come from a run of their own,
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/network_intensity_cost.py --trace-run

    python profiles/network_intensity_cost.py [--rounds 7] [--parent-lib PATH] [--out profiles/network_intensity_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PS = (1000, 10000)
THRESHOLDS = (3.0, 1.5)


class ParentContext(object):
    """a context of another build of the library: the two flat entry points of the extent call, bound by hand"""

    def __init__(self, path, signatures):
        self.lib = ctypes.CDLL(path)
        for name in ("fcd_baseline_network_bits", "fcd_graph_components"):
            fn = getattr(self.lib, name)
            (fn.restype, fn.argtypes) = signatures[name]
        self.lib.fcd_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.handle = ctypes.c_void_p()
        assert self.lib.fcd_ctx_create(ctypes.byref(self.handle)) == 0

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.handle, *args)
        assert rc == 0, (name, rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "network_intensity_cost.json"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib, baseline
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 100, 100)
    C = fcdiff_amd.N_to_C(Nreg)
    W = (C + 31) // 32
    rng = np.random.default_rng(0)
    b = rng.normal(0.3, 0.1, (C, H))
    bt = rng.normal(0.3, 0.1, (C, U))
    bt[:Nreg - 1] += 0.05
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    (b_d, bt_d) = (dev(b), dev(bt))
    ctx = _lib.Context()
    parent = ParentContext(args.parent_lib, _lib.SIGNATURES) if args.parent_lib else None
    (Pt, stream) = (_lib.dptr, _lib.stream_ptr())
    f64 = lambda *sh: torch.empty(sh, dtype=torch.float64, device="cuda")
    i32 = lambda *sh: torch.empty(sh, dtype=torch.int32, device="cuda")
    chunk = baseline._excess_chunk(W)
    labels = {}
    buf = {}
    for P in PS:
        labels[P] = dev(baseline.draw_labels(P, H, U, seed=P))
        buf[P] = dict(t=f64(C), bits1=i32(1, W), comp=i32(1, Nreg), o=[i32(1) for _ in range(3)], bits=i32(P, W),
                      n=[i32(P) for _ in range(3)], x1=f64(1, 32 * W), s1=f64(1, Nreg), m1=f64(1), x=f64(min(P, chunk), 32 * W),
                      m=f64(P))

    def extent(P, thr, c=ctx):
        o = buf[P]
        c.call("fcd_baseline_network_bits", Pt(b_d), Pt(bt_d), C, H, U, Pt(None), 1, thr, 0, Pt(o["bits1"]), Pt(o["t"]), stream)
        c.call("fcd_graph_components", Pt(o["bits1"]), 1, C, Pt(o["comp"]), Pt(o["o"][0]), Pt(o["o"][1]), Pt(o["o"][2]), stream)
        c.call("fcd_baseline_network_bits", Pt(b_d), Pt(bt_d), C, H, U, Pt(labels[P]), P, thr, 0, Pt(o["bits"]), Pt(None), stream)
        c.call("fcd_graph_components", Pt(o["bits"]), P, C, Pt(None), Pt(o["n"][0]), Pt(o["n"][1]), Pt(o["n"][2]), stream)

    def excess(lab, n, thr, bits, x, t):
        d = _lib.NetworkExcessDesc.make(C=C, H=H, U=U, P=n, threshold=thr, tail=0, stream=stream, b=Pt(b_d), bt=Pt(bt_d), labels=Pt(lab),
                                        bits=Pt(bits), excess=Pt(x), t=Pt(t))
        ctx.call("fcd_baseline_network_excess", ctypes.byref(d))

    def weighted(bits, x, n, comp, e, sums, top):
        d = _lib.ComponentsDesc.make(B=n, C=C, stream=stream, bits=Pt(bits), weights=Pt(x), component=Pt(comp), n_edges=Pt(e[0]),
                                     max_extent=Pt(e[1]), max_regions=Pt(e[2]), intensity=Pt(sums), max_intensity=Pt(top))
        ctx.call("fcd_graph_components_weighted", ctypes.byref(d))

    def intensity(P, thr):
        o = buf[P]
        excess(None, 1, thr, o["bits1"], o["x1"], o["t"])
        weighted(o["bits1"], o["x1"], 1, o["comp"], o["o"], o["s1"], o["m1"])
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            excess(labels[P][p0:p0 + n], n, thr, o["bits"][p0:p0 + n], o["x"], None)
            weighted(o["bits"][p0:p0 + n], o["x"], n, None, [v[p0:p0 + n] for v in o["n"]], None, o["m"][p0:p0 + n])

    if args.trace_run:
        for thr in THRESHOLDS:
            for fn in (extent, intensity):
                for _ in range(3):
                    fn(PS[-1], thr)
        torch.cuda.synchronize()
        for fn in (extent, intensity):
            for _ in range(args.trace_calls):
                fn(PS[-1], THRESHOLDS[0])
        torch.cuda.synchronize()
        return
    variants = {}
    for P in PS:
        n = 20 if P <= 1000 else 5
        for thr in THRESHOLDS:
            variants["extent_P%d_thr%.1f" % (P, thr)] = (lambda P=P, thr=thr: extent(P, thr), n)
            variants["intensity_P%d_thr%.1f" % (P, thr)] = (lambda P=P, thr=thr: intensity(P, thr), n)
        if parent is not None:
            variants["parent_P%d_thr3.0" % P] = (lambda P=P: extent(P, 3.0, parent), n)
    for (fn, _n) in variants.values():           # warm-up: code objects, the contexts' workspaces
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
           "thresholds": list(THRESHOLDS), "rounds": args.rounds, "excess_chunk": chunk,
           "calls_per_window": dict((k, v[1]) for (k, v) in variants.items()),
           "note": "us per call, calls back to back on one stream; us = best round, median_us, all_us = every round",
           "variants": {}, "ratios": {}, "results": {}}
    for name in variants:
        res["variants"][name] = {"us": min(times[name]), "median_us": float(np.median(times[name])), "all_us": times[name]}
    v = res["variants"]
    for P in PS:
        for thr in THRESHOLDS:
            key = "P%d_thr%.1f" % (P, thr)
            res["ratios"]["intensity_over_extent_" + key] = v["intensity_" + key]["median_us"] / v["extent_" + key]["median_us"]
            intensity(P, thr)
            o = buf[P]
            res["results"][key] = {"observed_n_edges": int(o["o"][0].item()), "observed_max_intensity": float(o["m1"].item()),
                                   "null_bits_set_share": float(o["n"][0].double().mean().item()) / C,
                                   "null_max_intensity_max": float(o["m"].max().item()),
                                   "null_max_extent_max": int(o["n"][1].max().item())}
        if parent is not None:
            res["ratios"]["extent_over_parent_P%d_thr3.0" % P] = v["extent_P%d_thr3.0" % P]["median_us"] / v["parent_P%d_thr3.0" % P]["median_us"]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
