"""
Cost of the sessions tables (fcd_lik_sessions.hip) on one MI355X, at cfg3's shape (Nreg 200, H = U = 50).

In one process, after a warm-up of every variant, the variants are timed in alternation (HIP events around --launches
back-to-back launches, --rounds rounds, best round per variant):
  * fcd_lik_tables, the 2-D build every other number is set against;
  * fcd_lik_tables_sessions at K = 1, 2, 4, 8;
  * fcd_lik_shared_tables_sessions at the same K (and the 2-D fcd_lik_shared_tables beside it).
Beside each time: the algorithmic bytes 8 C (H + U K) + 24 C + 72 C U (shared: 72 C), and the achieved fraction of the HBM
peak.  The two conditions of the feature are evaluated from these numbers and written under "conditions":
  K = 1 sessions <= 1.5 x the 2-D build, K = 8 sessions < 8 x the 2-D build.

    python profiles/sessions_cost.py [--launches 200] [--rounds 7] [--out profiles/sessions_cost.json]

The other read form of the unshared kernel (every thread reads its own item's K doubles from global memory) is a build of
its own, loaded in a process of its own and set against the 2-D kernel of that same process:
    make -C fcdiff_amd/csrc SUF=.strided.o LIB=../libfcdiff_hip_strided.so EXTRA=-DFCD_SESS_STRIDED
    FCDIFF_HIP_LIB=fcdiff_amd/libfcdiff_hip_strided.so python profiles/sessions_cost.py --read-form strided \
        --out profiles/sessions_cost_strided.json

Prints one JSON document (and writes it to --out where given).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal
KS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--read-form", default="staged: a tile's 256 K doubles loaded coalesced through the stage buffer, 9 sessions "
                    "per pass", help="label of the build under FCDIFF_HIP_LIB (a -DFCD_SESS_STRIDED build: 'strided')")
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    from fcdiff_amd import _lib
    torch.cuda.set_device(0)
    (Nreg, H, U) = (200, 50, 50)
    C = fcdiff_amd.N_to_C(Nreg)
    model = fcdiff_amd.UnsharedRegionModel()
    theta = model.theta()
    ctx = _lib.Context()
    (_r, _t, _f, _ft, b, bt8) = model.sample_fast(Nreg, H, U, seed=0, sessions=max(KS))
    b_d = torch.as_tensor(b, device="cuda")
    S_B = torch.empty((C, 3), dtype=torch.float64, device="cuda")
    lM = torch.empty((C, U, 3, 3), dtype=torch.float64, device="cuda")
    L = torch.empty((C, 1, 3, 3), dtype=torch.float64, device="cuda")
    variants = {}

    (th, _th) = _lib.dbl_array(theta)
    (P, stream) = (_lib.dptr, _lib.stream_ptr())

    def add(name, bt_d, shared, K):
        # the library call tables.build makes for this input, its arguments made once: the window times launches, not Python
        nbytes = 8 * C * (H + U * K) + 24 * C + 72 * C * (1 if shared else U)
        k = () if bt_d.dim() == 2 else (K,)
        if shared:
            entry = "fcd_lik_shared_tables_sessions" if k else "fcd_lik_shared_tables"
            a = (P(b_d), P(bt_d), C, H, U) + k + (th, P(S_B), P(L), 0, P(None), stream)
        elif k:
            (entry, a) = ("fcd_lik_tables_sessions", (P(b_d), P(bt_d), C, H, U, K, th, P(S_B), P(lM), P(None), 0, P(None), stream))
        else:
            (entry, a) = ("fcd_lik_tables", (P(b_d), P(bt_d), C, H, U, th, P(S_B), P(lM), P(None), P(None), stream))
        keep.append(bt_d)
        variants[name] = (lambda: ctx.call(entry, *a), nbytes)
    keep = []
    bt2 = torch.as_tensor(bt8[:, :, 0].copy(), device="cuda")
    add("lik_tables_2d", bt2, False, 1)
    add("lik_shared_tables_2d", bt2, True, 1)
    for K in KS:
        btk = torch.as_tensor(bt8[:, :, :K].copy(), device="cuda")
        add("sessions_K%d" % K, btk, False, K)
        add("shared_sessions_K%d" % K, btk, True, K)
    for (fn, _n) in variants.values():           # warm-up: code objects, the context's tables
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
           "launches_per_round": args.launches, "rounds": args.rounds, "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS,
           "read_form": args.read_form,
           "note": "us per library call, launches back to back on one stream, best round; all_us = every round",
           "variants": {}}
    for (name, (_fn, nbytes)) in variants.items():
        us = min(times[name])
        gbs = nbytes / (us * 1e3)
        res["variants"][name] = {"us": us, "all_us": times[name], "algorithmic_MB": nbytes / 1e6, "GB_per_s": gbs,
                                 "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS}
    base = res["variants"]["lik_tables_2d"]["us"]
    (k1, k8) = (res["variants"]["sessions_K1"]["us"], res["variants"]["sessions_K8"]["us"])
    res["conditions"] = {"K1_over_2d": k1 / base, "K1_at_most_1.5x_2d": bool(k1 <= 1.5 * base),
                         "K8_over_2d": k8 / base, "K8_below_8x_2d": bool(k8 < 8.0 * base)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
