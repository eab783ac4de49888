"""
Cost of the missing-data form of the table kernel: fcd_lik_tables (flag off) and fcd_lik_tables_ex with
FCD_DATA_NAN_MISSING on data with ~10 % NaN, at cfg3 (Nreg=200, H=U=50), `--reps` launches each.  Run it under
`rocprofv3 --kernel-trace --stats -- python3 profiles/missing_data_cost.py`: lik_kernel<false> and lik_kernel<true> come
out as separate rows.  --lib loads another build of the library through ctypes alone (a build without the _ex entry
points times the flag-off launch only), so the same script times the library before the flag existed.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "fcdiff_amd", "libfcdiff_hip.so"))
    ap.add_argument("--nreg", type=int, default=200)
    ap.add_argument("--subjects", type=int, default=100)
    ap.add_argument("--nan", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    torch.cuda.init()
    lib = C.CDLL(a.lib)
    from fcdiff_amd.model import UnsharedRegionModel
    m = UnsharedRegionModel()
    (N, H) = (a.nreg, a.subjects // 2)
    U = a.subjects - H
    (_r, _t, _f, _ft, b, bt) = m.sample_fast(N, H, U, seed=3)
    Cn = b.shape[0]
    rng = np.random.default_rng(1)
    (bn, btn) = (b.copy(), bt.copy())
    bn[rng.random(b.shape) < a.nan] = np.nan
    btn[rng.random(bt.shape) < a.nan] = np.nan
    dev = torch.device("cuda", 0)
    t = {k: torch.as_tensor(v, device=dev) for (k, v) in dict(b=b, bt=bt, bn=bn, btn=btn).items()}
    S_B = torch.empty((Cn, 3), dtype=torch.float64, device=dev)
    lM = torch.empty((Cn, U, 3, 3), dtype=torch.float64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    th = np.ascontiguousarray(m.theta(), dtype=np.float64)
    thp = th.ctypes.data_as(C.POINTER(C.c_double))
    ctx = C.c_void_p()
    assert lib.fcd_ctx_create(C.byref(ctx)) == 0
    p = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.fcd_lik_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                   C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    runs = [("flag off", lambda: lib.fcd_lik_tables(ctx, p(t["b"]), p(t["bt"]), Cn, H, U, thp, p(S_B), p(lM), None, None, s))]
    if hasattr(lib, "fcd_lik_tables_ex"):
        lib.fcd_lik_tables_ex.argtypes = lib.fcd_lik_tables.argtypes[:11] + [C.c_int, C.c_void_p, C.c_void_p]

        def ex(bk, btk, counted):
            return lambda: lib.fcd_lik_tables_ex(ctx, p(t[bk]), p(t[btk]), Cn, H, U, thp, p(S_B), p(lM), None, None, 1,
                                                 p(cnt) if counted else None, s)
        pct = "%.0f %% NaN" % (100 * a.nan)
        runs += [("flag on, no NaN", ex("b", "bt", True)), ("flag on, %s, uncounted" % pct, ex("bn", "btn", False)),
                 ("flag on, %s" % pct, ex("bn", "btn", True))]
    for (name, fn) in runs:
        for _ in range(5):
            assert fn() == 0
        torch.cuda.synchronize()
        (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e0.record()
        for _ in range(a.reps):
            assert fn() == 0
        e1.record()
        torch.cuda.synchronize()
        print("%-32s %8.2f us per table build (events, %d launches; %s)" % (name, 1e3 * e0.elapsed_time(e1) / a.reps, a.reps,
                                                                            os.path.basename(a.lib)))
    if len(runs) > 1:
        print("missing counts:", cnt.cpu().tolist(), "expected:", [int(np.isnan(bn).sum()), int(np.isnan(btn).sum())])
    lib.fcd_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
