"""
Cost of the tangent-space front-end (fcd_tangent_fit, fcd_tangent_apply, fcd_sym_eigh; fcd_corr_tangent.hip) on one MI355X at
the front-end shapes of cfg3 (S = 100 subjects, Nreg = 200, T = 1200) and cfg5 (Nreg = 400).

    python profiles/tangent_cost.py [--out profiles/tangent_cost.json] [--calls 2] [--windows 3]

(profiles/tangent_cost.json was made by this command with its defaults.)

Per shape, in this order (the method of profiles/partial_cost.py):
  1. the kernels' own times: a child process per shape under `rocprofv3 --kernel-trace --stats` (a run of its own) that makes
     --calls calls of fcd_tangent_apply after one warm-up call, with W = the inverse root of the mean correlation matrix made on
     the host -- no fit runs in the child, so every launch in its averages is one of apply on the whole batch; average ns
     per kernel name from its kernel_stats.csv.  The children run BEFORE this process touches the device.
  2. call times with the profiler off: device events around windows of --calls back-to-back calls, after a warm-up of every
     kind; the kinds alternated --windows times:
       fit            fcd_tangent_fit, geometric, Ledoit-Wolf, on the S subjects as controls (with its iteration count; the
                      fit waits for its stream once per iteration, so its window is host time too)
       apply          fcd_tangent_apply on the same subjects with the fit's W
       eigh           fcd_sym_eigh on the (S, p, p) matrices M_s = W R_a W (made on the host)
       eigh_one       fcd_sym_eigh on the first of them alone: one workgroup on an otherwise idle device
       torch_eigh     torch.linalg.eigh on the same matrices
       torch_logm     torch.linalg.eigh + (V * log w) @ V^T: the generic library's route from M_s to T_s
       partial_lw     fcd_corr_partial, Ledoit-Wolf, beside them
The aim: fcd_sym_eigh's median below torch_eigh's median in the same run.  The ratio is written down whatever it is; a record,
not a gate.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": dict(S=100, Nreg=200, T=1200), "cfg5": dict(S=100, Nreg=400, T=1200)}
KERNELS = ("corr_moments", "corr_gram_subject", "corr_gram_kernel", "corr_transpose", "pc_dense", "pc_rows", "pc_total", "pc_moments", "pc_frame",
           "pc_shrink", "tg_pad", "tg_dead", "tg_gemm_nt", "eig_jacobi", "tg_fvals", "tg_emit", "tg_diag")


def make_series(np, sh):
    """four shared factors through fixed loadings plus region noise: correlated regions, every subject near the reference"""
    rs = np.random.RandomState(2000 + sh["Nreg"])
    (S, N, T) = (sh["S"], sh["Nreg"], sh["T"])
    L = rs.standard_normal((N, 4))
    return np.einsum("nf,sft->snt", L, rs.standard_normal((S, 4, T))) + rs.standard_normal((S, N, T)) * (0.5 + rs.random_sample((S, N, 1)))


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
        f64 = dict(dtype=torch.float64, device=dev)
        (self.out, self.diag) = (torch.empty((util.N_to_C(N), S), **f64), torch.empty((N, S), **f64))
        (self.alpha, self.info) = (torch.empty((S,), **f64), torch.empty((S, 2), dtype=torch.int32, device=dev))
        (self.G, self.Gh, self.W) = (torch.empty((N, N), **f64), torch.empty((N, N), **f64), torch.eye(N, **f64))
        self.used = torch.empty((S,), dtype=torch.uint8, device=dev)
        (self.n_iter, self.grad) = (ctypes.c_int32(0), ctypes.c_double(0.0))
        (self.w, self.V, self.st) = (torch.empty((S, N), **f64), torch.empty((S, N, N), **f64), torch.empty((S,), dtype=torch.int32, device=dev))
        self.mats = None

    def desc(self, **kw):
        (p, sh) = (self.lib.dptr, self.sh)
        return self.lib.TangentDesc.make(S=sh["S"], Nreg=sh["Nreg"], T=sh["T"], shrink_mode=1, max_iter=50, tol=1e-10,
                                         stream=self.lib.stream_ptr(), ts=p(self.ts), alpha=p(self.alpha), info=p(self.info), W=p(self.W), **kw)

    def fit(self):
        p = self.lib.dptr
        d = self.desc(G=p(self.G), G_half=p(self.Gh), used=p(self.used), n_iter=ctypes.cast(ctypes.pointer(self.n_iter), ctypes.c_void_p),
                      grad_norm=ctypes.cast(ctypes.pointer(self.grad), ctypes.c_void_p))
        self.ctx.call("fcd_tangent_fit", ctypes.byref(d))

    def apply(self):
        p = self.lib.dptr
        d = self.desc(out=p(self.out), diag=p(self.diag))
        self.ctx.call("fcd_tangent_apply", ctypes.byref(d))

    def partial(self):
        (p, sh) = (self.lib.dptr, self.sh)
        self.ctx.call("fcd_corr_partial", p(self.ts), sh["S"], sh["Nreg"], sh["T"], p(None), 1, 0.0, 0, p(self.out), p(self.alpha),
                      p(self.info), self.lib.stream_ptr())

    def make_mats(self):
        """M_s = W R_a W (S, p, p) on the device, from the host's correlations, the device's alpha and the fit's W"""
        np = self.np
        a = self.alpha.cpu().numpy()
        W = self.W.cpu().numpy()
        N = self.sh["Nreg"]
        M = np.stack([W.dot((1.0 - a[s]) * np.corrcoef(self.host[s]) + a[s] * np.eye(N)).dot(W) for s in range(self.sh["S"])])
        self.mats = self.torch.as_tensor((M + M.transpose(0, 2, 1)) / 2, device=self.ctx.device)

    def host_whitening(self):
        """W of the traced child: the inverse root of the mean correlation matrix, on the host"""
        np = self.np
        (w, V) = np.linalg.eigh(np.mean([np.corrcoef(x) for x in self.host], axis=0))
        self.W.copy_(self.torch.as_tensor((V / np.sqrt(w)).dot(V.T)))

    def eigh(self, B=None):
        (p, sh) = (self.lib.dptr, self.sh)
        d = self.lib.EighDesc.make(B=sh["S"] if B is None else B, n=sh["Nreg"], stream=self.lib.stream_ptr(), A=p(self.mats), w=p(self.w), V=p(self.V), status=p(self.st))
        self.ctx.call("fcd_sym_eigh", ctypes.byref(d))

    def torch_eigh(self):
        return self.torch.linalg.eigh(self.mats)

    def torch_logm(self):
        (w, V) = self.torch.linalg.eigh(self.mats)
        return (V * self.torch.log(w)[:, None, :]) @ V.transpose(1, 2)


def workload(name, calls):
    """What the traced child runs: a warm-up call of apply, then `calls` more."""
    w = Work(name)
    w.host_whitening()
    for n in (1, calls):
        for _ in range(n):
            w.apply()
        w.torch.cuda.synchronize()


def kernel_stats(name, calls, scratch):
    d = os.path.join(scratch, "kstats_%s" % name)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "k", "--",
           sys.executable, os.path.abspath(__file__), "--workload", name, "--calls", str(calls)]
    subprocess.run(cmd, check=True, timeout=500, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 left no kernel_stats.csv under %s" % d)
    out = {}
    for row in csv.DictReader(open(files[0])):
        for key in KERNELS:
            if key in row["Name"]:
                # (the warm-up call is in the averages too)
                out[key + "_kernel"] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                        "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def timed_windows(name, calls, windows):
    import numpy as np
    w = Work(name)
    torch = w.torch
    w.fit()
    torch.cuda.synchronize()
    res = {"fit_n_iter": int(w.n_iter.value), "fit_grad_norm": float(w.grad.value), "controls_used": int(w.used.sum().item())}
    w.apply()
    w.make_mats()
    res["status_ok"] = bool((w.info.cpu().numpy()[:, 1] == 0).all())
    res["alpha_min"] = float(w.alpha.min().item())
    res["alpha_max"] = float(w.alpha.max().item())
    kinds = {"fit": w.fit, "apply": w.apply, "eigh": w.eigh, "eigh_one": lambda: w.eigh(1), "partial_lw": w.partial}
    try:
        T = w.torch_logm()
        torch.cuda.synchronize()
        (n, m) = np.tril_indices(w.sh["Nreg"], -1)
        res["max_abs_diff_to_torch"] = float(np.abs(w.out.cpu().numpy() - T.cpu().numpy()[:, n, m].T).max())
        ev = torch.linalg.eigvalsh(w.mats)
        res["kappa_max"] = float((ev[:, -1] / ev[:, 0]).max().item())
        kinds["torch_eigh"] = w.torch_eigh
        kinds["torch_logm"] = w.torch_logm
        res["torch_eigh_ran"] = True
    except Exception as e:
        res["torch_eigh_ran"] = False
        res["torch_eigh_error"] = repr(e)[:300]
    for fn in kinds.values():
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
    res["eigh_status_ok"] = bool((w.st.cpu().numpy() == 0).all())
    for (k, v) in ms.items():
        res[k] = {"best_us": 1e3 * min(v), "median_us": 1e3 * float(np.median(v)), "all_us": [1e3 * x for x in v]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent_cost.json"))
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--scratch", default=None, help="where the traced children write (default: a temporary directory)")
    ap.add_argument("--workload", default=None, help="(the traced child) run the calls of this shape and exit")
    ap.add_argument("--no-trace", action="store_true", help="skip the traced children (no per-kernel times)")
    args = ap.parse_args()
    if args.workload is not None:
        workload(args.workload, args.calls)
        return
    if args.scratch is None:
        import tempfile
        args.scratch = tempfile.mkdtemp(prefix="tangent_cost_")
    res = {"shapes": SHAPES, "calls_per_window": args.calls, "windows": args.windows,
           "method": "kernels: rocprofv3 --kernel-trace --stats, one child per shape, average over a warm-up call and the calls of "
                     "apply (no fit in the child); calls: device events around windows of back-to-back calls, profiler off, the kinds alternated",
           "shape": {}}
    stats = {} if args.no_trace else {name: kernel_stats(name, args.calls, args.scratch) for name in SHAPES}
    import torch
    torch.cuda.set_device(0)
    res["device"] = torch.cuda.get_device_name(0)
    for name in SHAPES:
        r = timed_windows(name, args.calls, args.windows)
        r["kernels"] = stats.get(name)
        if r["torch_eigh_ran"]:
            r["eigh_one_over_eigh"] = r["eigh_one"]["median_us"] / r["eigh"]["median_us"]
            r["eigh_over_torch_eigh"] = r["eigh"]["median_us"] / r["torch_eigh"]["median_us"]
            r["apply_over_torch_logm"] = r["apply"]["median_us"] / r["torch_logm"]["median_us"]
            r["aim"] = "fcd_sym_eigh median < torch_eigh median"
            r["aim_met"] = bool(r["eigh_over_torch_eigh"] < 1.0)
        res["shape"][name] = r
        print("%s done" % name, file=sys.stderr)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
