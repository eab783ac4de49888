"""
Cost of the cleaning front-end (fcd_corr_clean, fcd_corr_clean.hip) on one MI355X, at cfg3's front-end shape
(S = 100 subjects, Nreg = 200, T = 1200), Q in {0, 6, 24, 36} confounds, 10 % of the frames dropped per subject.

    python profiles/corr_clean_cost.py [--out profiles/corr_clean_cost.json] [--calls 200] [--windows 5]

Per Q, in this order:
  1. the kernels' own times: a child process per Q under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing
     slows the host) that makes --calls calls of fcd_corr_clean + fcd_corr_edges after a warm-up; average ns per kernel
     name from its kernel_stats.csv.  The children run BEFORE this process touches the device.
  2. call times with the profiler off: device events around windows of --calls back-to-back calls (queue kept full), after
     a warm-up of every shape; three kinds of window alternated --windows times so that clock drift hits them alike:
       clean          fcd_corr_clean (all its launches)
       edges_after    fcd_corr_edges on the residuals it left
       plain          fcd_corr_edges on the raw series: what correlations(ts) runs
     best and median per call of each, and all windows.
Bytes: `ts_MB` is one pass over ts; by bytes cleaning is at most three reads and one write of it (plus Q / Nreg of that for
the confounds).  Writes one JSON document; a record, not a gate.
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

SHAPE = dict(S=100, Nreg=200, T=1200)
QS = (0, 6, 24, 36)
DROP = 0.10


def make_inputs(np, Q):
    rs = np.random.RandomState(1000 + Q)
    (S, N, T) = (SHAPE["S"], SHAPE["Nreg"], SHAPE["T"])
    z = rs.standard_normal((S, max(Q, 1), T))[:, :Q]
    ts = rs.standard_normal((S, N, T)) + 0.7 * rs.standard_normal((S, 1, T)) + 100.0
    if Q:
        ts += np.einsum("snq,sqt->snt", rs.standard_normal((S, N, Q)) / np.sqrt(Q), z)
    mask = rs.uniform(size=(S, T)) >= DROP
    return (ts, z + 0.5, mask)


class Work(object):
    """Device buffers of one Q and the three calls."""

    def __init__(self, Q):
        import numpy as np
        import torch
        from fcdiff_amd import _lib, util
        (self.torch, self.lib, self.Q) = (torch, _lib, Q)
        self.ctx = _lib.Context()
        (ts, cf, mask) = make_inputs(np, Q)
        dev = self.ctx.device
        self.ts = torch.as_tensor(ts, device=dev)
        self.cf = torch.as_tensor(np.ascontiguousarray(cf), device=dev) if Q else None
        self.mask = torch.as_tensor(mask.astype(np.uint8), device=dev)
        (S, N, T) = (SHAPE["S"], SHAPE["Nreg"], SHAPE["T"])
        self.resid = torch.empty((S, N, T), dtype=torch.float64, device=dev)
        self.info = torch.empty((S, 3), dtype=torch.int32, device=dev)
        self.out = torch.empty((util.N_to_C(N), S), dtype=torch.float64, device=dev)
        self.kept = int(mask.sum())

    def clean(self):
        p = self.lib.dptr
        self.ctx.call("fcd_corr_clean", p(self.ts), p(self.cf), p(self.mask), SHAPE["S"], SHAPE["Nreg"], self.Q, SHAPE["T"],
                      p(self.resid), p(self.info), self.lib.stream_ptr())

    def edges(self, src):
        p = self.lib.dptr
        self.ctx.call("fcd_corr_edges", p(src), SHAPE["S"], SHAPE["Nreg"], SHAPE["T"], 0, p(self.out), self.lib.stream_ptr())


def workload(Q, calls):
    """What the traced child runs: warm-up, then `calls` x (clean, edges on the residuals)."""
    w = Work(Q)
    for n in (3, calls):
        for _ in range(n):
            w.clean()
            w.edges(w.resid)
        w.torch.cuda.synchronize()


def kernel_stats(Q, calls, scratch):
    d = os.path.join(scratch, "kstats_q%d" % Q)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--",
           sys.executable, os.path.abspath(__file__), "--workload", str(Q), "--calls", str(calls)]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 left no kernel_stats.csv under %s" % d)
    out = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Name"]
        for key in ("clean_index", "clean_moments", "clean_gram", "clean_chol", "clean_beta", "clean_resid", "clean_finish",
                    "corr_gram_subject", "corr_transpose"):
            if key in name:
                # the warm-up calls are in the average too: 3 of calls + 3
                out[key + "_kernel"] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                        "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    out["clean_kernels_sum_us"] = sum(v["avg_us"] for (k, v) in out.items() if k.startswith("clean_"))
    return out


def timed_windows(Q, calls, windows):
    import numpy as np
    w = Work(Q)
    torch = w.torch
    kinds = {"clean": w.clean, "edges_after": lambda: w.edges(w.resid), "plain": lambda: w.edges(w.ts)}
    for fn in kinds.values():          # warm-up of every shape
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
    res = {"kept_frames": w.kept, "rank_min": int(info[:, 1].min()), "rank_max": int(info[:, 1].max())}
    for (k, v) in ms.items():
        res[k] = {"best_us": 1e3 * min(v), "median_us": 1e3 * float(np.median(v)), "all_us": [1e3 * x for x in v]}
    res["clean_over_plain"] = res["clean"]["median_us"] / res["plain"]["median_us"]
    res["clean_over_edges_after"] = res["clean"]["median_us"] / res["edges_after"]["median_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_clean_cost.json"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scratch", default=None, help="where the traced children write (default: a temporary directory)")
    ap.add_argument("--workload", type=int, default=None, help="(the traced child) run the calls of this Q and exit")
    args = ap.parse_args()
    if args.workload is not None:
        workload(args.workload, args.calls)
        return
    if args.scratch is None:
        import tempfile
        args.scratch = tempfile.mkdtemp(prefix="corr_clean_cost_")
    ts_bytes = SHAPE["S"] * SHAPE["Nreg"] * SHAPE["T"] * 8
    res = {"shape": SHAPE, "drop": DROP, "calls_per_window": args.calls, "windows": args.windows, "ts_MB": ts_bytes / 1e6,
           "method": "kernels: rocprofv3 --kernel-trace --stats, one child per Q, average over calls + 3 launches; calls: device "
                     "events around windows of back-to-back calls, profiler off, three kinds alternated",
           "Q": {}}
    stats = {Q: kernel_stats(Q, args.calls, args.scratch) for Q in QS}      # before this process opens the device
    import torch
    torch.cuda.set_device(0)
    res["device"] = torch.cuda.get_device_name(0)
    for Q in QS:
        r = timed_windows(Q, args.calls, args.windows)
        r["kernels"] = stats[Q]
        res["Q"][str(Q)] = r
        print("Q %d done" % Q, file=sys.stderr)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
