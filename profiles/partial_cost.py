"""
Cost of the partial correlations (fcd_corr_partial, fcd_corr_partial.hip) on one MI355X at the front-end shapes of cfg3
(S = 100 subjects, Nreg = 200, T = 1200) and cfg5 (Nreg = 400).

    python profiles/partial_cost.py [--out profiles/partial_cost.json] [--calls 50] [--windows 5]

Per shape, in this order:
  1. the kernels' own times: a child process per shape under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing
     slows the host) that makes --calls calls of fcd_corr_partial (Ledoit-Wolf) after a warm-up; average ns per kernel name
     from its kernel_stats.csv.  The children run BEFORE this process touches the device.
  2. call times with the profiler off: device events around windows of --calls back-to-back calls (queue kept full), after
     a warm-up of every kind; the kinds alternated --windows times so that clock drift hits them alike:
       partial_lw     fcd_corr_partial, Ledoit-Wolf (all its launches)
       partial_fixed  fcd_corr_partial, alpha = 0.1 (no moments, no frame norms)
       plain          fcd_corr_edges on the same series: what correlations(ts) runs
       torch_inverse  torch.linalg.cholesky + torch.cholesky_inverse, fp64, on the same (S, p, p) matrices R_alpha (made on
                      the host from the device's alpha) -- the generic library's route to the same inverse
     best and median per call of each, and all windows.
The record's one condition: the inversion kernel (its average under 1.) is faster than torch_inverse's median in the same
run.  If torch's batched factorisation does not run on the box the record says so and the condition becomes "the inversion
at cfg3's shape takes less than 200 unblocked steps of 2.5 us" (clean_chol_kernel's measured step).
fp64 MFMA rate: p^3 flops per subject of the blocked Gauss-Jordan on the lower tiles over the inversion kernel's time, as a fraction of
78.6 TFLOP/s.  Writes one JSON document; a record, not a gate.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": dict(S=100, Nreg=200, T=1200), "cfg5": dict(S=100, Nreg=400, T=1200)}
KERNELS = ("corr_moments", "corr_gram_subject", "corr_gram_kernel", "corr_transpose", "pc_dense", "pc_rows", "pc_total", "pc_moments", "pc_frame",
           "pc_shrink", "pc_invert", "pc_emit")
FP64_MFMA_TFLOPS = 78.6
UNBLOCKED_STEP_US = 2.5


def make_series(np, sh):
    rs = np.random.RandomState(2000 + sh["Nreg"])
    (S, N, T) = (sh["S"], sh["Nreg"], sh["T"])
    return rs.standard_normal((S, N, T)) + 0.7 * rs.standard_normal((S, 1, T)) + 100.0


class Work(object):
    """Device buffers of one shape and the calls."""

    def __init__(self, name):
        import numpy as np
        import torch
        from fcdiff_amd import _lib, util
        (self.np, self.torch, self.lib, self.sh) = (np, torch, _lib, SHAPES[name])
        self.ctx = _lib.Context()
        dev = self.ctx.device
        (S, N) = (self.sh["S"], self.sh["Nreg"])
        self.host = make_series(np, self.sh)
        self.ts = torch.as_tensor(self.host, device=dev)
        self.out = torch.empty((util.N_to_C(N), S), dtype=torch.float64, device=dev)
        self.alpha = torch.empty((S,), dtype=torch.float64, device=dev)
        self.info = torch.empty((S, 2), dtype=torch.int32, device=dev)
        self.mats = None

    def partial(self, mode, value=0.0):
        (p, sh) = (self.lib.dptr, self.sh)
        self.ctx.call("fcd_corr_partial", p(self.ts), sh["S"], sh["Nreg"], sh["T"], p(None), mode, value, 0, p(self.out), p(self.alpha),
                      p(self.info), self.lib.stream_ptr())

    def plain(self):
        (p, sh) = (self.lib.dptr, self.sh)
        self.ctx.call("fcd_corr_edges", p(self.ts), sh["S"], sh["Nreg"], sh["T"], 0, p(self.out), self.lib.stream_ptr())

    def make_mats(self):
        """R_alpha (S, p, p) on the device, from the host's correlations and the device's Ledoit-Wolf alpha."""
        np = self.np
        self.partial(1)
        a = self.alpha.cpu().numpy()
        N = self.sh["Nreg"]
        R = np.stack([(1.0 - a[s]) * np.corrcoef(self.host[s]) + a[s] * np.eye(N) for s in range(self.sh["S"])])
        self.mats = self.torch.as_tensor(R, device=self.ctx.device)
        return a

    def torch_inverse(self):
        return self.torch.cholesky_inverse(self.torch.linalg.cholesky(self.mats))


def workload(name, calls):
    """What the traced child runs: warm-up, then `calls` Ledoit-Wolf calls."""
    w = Work(name)
    for n in (3, calls):
        for _ in range(n):
            w.partial(1)
        w.torch.cuda.synchronize()


def kernel_stats(name, calls, scratch):
    d = os.path.join(scratch, "kstats_%s" % name)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--",
           sys.executable, os.path.abspath(__file__), "--workload", name, "--calls", str(calls)]
    subprocess.run(cmd, check=True, timeout=400, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 left no kernel_stats.csv under %s" % d)
    out = {}
    for row in csv.DictReader(open(files[0])):
        for key in KERNELS:
            if key in row["Name"]:
                # the warm-up calls are in the average too: 3 of calls + 3
                out[key + "_kernel"] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                        "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    out["kernels_sum_us"] = sum(v["avg_us"] for v in out.values())
    return out


def timed_windows(name, calls, windows):
    import numpy as np
    w = Work(name)
    torch = w.torch
    alpha = w.make_mats()
    kinds = {"partial_lw": lambda: w.partial(1), "partial_fixed": lambda: w.partial(0, 0.1), "plain": w.plain}
    res = {"alpha_min": float(alpha.min()), "alpha_max": float(alpha.max())}
    try:
        inv = w.torch_inverse()
        torch.cuda.synchronize()
        # the same inverse: the device's rho against the one from torch's Theta
        w.partial(1)
        d = torch.rsqrt(torch.diagonal(inv, dim1=1, dim2=2))
        rho = -inv * d[:, :, None] * d[:, None, :]
        (n, m) = np.tril_indices(w.sh["Nreg"], -1)
        res["max_abs_diff_to_torch"] = float((w.out.cpu().numpy() - rho.cpu().numpy()[:, n, m].T).__abs__().max())
        kinds["torch_inverse"] = w.torch_inverse
        res["torch_inverse_ran"] = True
    except Exception as e:           # the record says so; the condition falls back (module docstring)
        res["torch_inverse_ran"] = False
        res["torch_inverse_error"] = repr(e)[:300]
    for fn in kinds.values():          # warm-up of every kind
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in kinds}
    for _ in range(windows):
        for (k, fn) in kinds.items():
            (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            a.record()
            for _c in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    info = w.info.cpu().numpy()
    res["status_ok"] = bool((info[:, 1] == 0).all())
    for (k, v) in ms.items():
        res[k] = {"best_us": 1e3 * min(v), "median_us": 1e3 * float(np.median(v)), "all_us": [1e3 * x for x in v]}
    res["partial_lw_over_plain"] = res["partial_lw"]["median_us"] / res["plain"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partial_cost.json"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scratch", default=None, help="where the traced children write (default: a temporary directory)")
    ap.add_argument("--workload", default=None, help="(the traced child) run the calls of this shape and exit")
    args = ap.parse_args()
    if args.workload is not None:
        workload(args.workload, args.calls)
        return
    if args.scratch is None:
        import tempfile
        args.scratch = tempfile.mkdtemp(prefix="partial_cost_")
    res = {"shapes": SHAPES, "calls_per_window": args.calls, "windows": args.windows,
           "method": "kernels: rocprofv3 --kernel-trace --stats, one child per shape, average over calls + 3 launches; calls: device "
                     "events around windows of back-to-back calls, profiler off, the kinds alternated",
           "shape": {}}
    stats = {name: kernel_stats(name, args.calls, args.scratch) for name in SHAPES}      # before this process opens the device
    import torch
    torch.cuda.set_device(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in SHAPES:
        r = timed_windows(name, args.calls, args.windows)
        r["kernels"] = stats[name]
        inv_us = stats[name]["pc_invert_kernel"]["avg_us"]
        sh = SHAPES[name]
        r["invert_fraction_of_fp64_mfma_rate"] = 1.0 * sh["S"] * sh["Nreg"] ** 3 / (inv_us * 1e-6) / (FP64_MFMA_TFLOPS * 1e12)
        if r["torch_inverse_ran"]:
            r["condition"] = "pc_invert_kernel avg < torch_inverse median"
            r["condition_met"] = bool(inv_us < r["torch_inverse"]["median_us"])
        else:
            r["condition"] = "pc_invert_kernel avg < 200 unblocked steps x %.1f us" % UNBLOCKED_STEP_US
            r["condition_met"] = bool(inv_us < 200 * UNBLOCKED_STEP_US)
        res["shape"][name] = r
        print("%s done" % name, file=sys.stderr)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
