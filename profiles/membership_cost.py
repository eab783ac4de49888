"""
Cost of the patient-or-control kernel (UnsharedRegionFit.membership, fcd_member.hip) on one MI355X, at cfg3's model size
(Nreg 200, 1024 chains):
  * fcd_member_loglik (both launches: the walk and the fold of its slices) at U' in {100, 1000, 10000} subjects, with r one
    column for all subjects (r_cols = 1, the shared-region model) and one column per subject (r_cols = U'), both sides
    computed; and the control side alone (out_patient NULL), which is what the unshared model's membership() asks of it;
  * beside it, from the same session, the existing way to the patient side through the table at U' = 100: fcd_lik_tables
    (the (C, U', 3, 3) table) + one fcd_score_ais_step from beta 0 to 1.  Context, not a gate.
Random data and random chain states: the kernel's work does not depend on the values.

    python profiles/membership_cost.py [--reps 3] [--only 100,1000,10000] [--out profiles/membership_cost.json]

Writes one JSON document (kept as profiles/membership_cost.json).  Timings: HIP events around the calls, best of --reps,
after one warm-up call each.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NREG, G = 200, 1024
GPU_TESTS = 68               # tests/test_gpu_membership.py, all passing on the MI355X in the session that measured this


def timed(torch, fn, reps):
    best = None
    for _ in range(reps):
        (a, b) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return best


def shape_run(torch, fcdiff_amd, U, reps):
    from fcdiff_amd import _lib, score
    gen = fcdiff_amd.UnsharedRegionModel()
    theta = gen.theta()
    ctx = _lib.Context()
    C = NREG * (NREG - 1) // 2
    GW = (G + 63) // 64
    g = torch.Generator(device="cuda").manual_seed(U)
    x = (0.35 * torch.randn((C, U), dtype=torch.float64, device="cuda", generator=g)).clamp_(-1, 1)
    f_state = torch.randint(0, 3, (GW, C, 64), dtype=torch.uint8, device="cuda", generator=g)
    # (random 64-bit words: every chain's r_nu an independent fair coin)
    r_all = torch.randint(-(1 << 62), 1 << 62, (GW, NREG, U), dtype=torch.int64, device="cuda", generator=g)
    r_one = r_all[:, :, :1].contiguous()
    lc = torch.empty((G, U), dtype=torch.float64, device="cuda")
    lp = torch.empty((G, U), dtype=torch.float64, device="cuda")
    (th, _th) = _lib.dbl_array(theta)
    n = 5 if U <= 1000 else 2
    out = {"shape": {"Nreg": NREG, "U": U, "G": G}}

    def member(r_bits, r_cols, patient):
        def run():
            for _ in range(n):
                ctx.call("fcd_member_loglik", _lib.dptr(x), th, _lib.dptr(f_state), _lib.dptr(r_bits), NREG, U, G, r_cols, 0,
                         _lib.dptr(lc), _lib.dptr(lp if patient else None), _lib.stream_ptr())
        run()
        return 1e3 * timed(torch, run, reps) / n
    out["member_loglik_r_cols_1_us"] = member(r_one, 1, True)
    out["member_loglik_r_cols_U_us"] = member(r_all, U, True)
    out["member_loglik_control_only_us"] = member(None, 1, False)
    out["items_C_times_U"] = C * U
    out["lookups_per_side_C_U_G"] = C * U * G
    if U == 100:
        b = torch.zeros((C, 1), dtype=torch.float64, device="cuda")
        w = torch.zeros((G, U), dtype=torch.float64, device="cuda")

        def tables():
            for _ in range(n):
                score.lik_tables(ctx, b, x, theta, False)
        tables()
        out["lik_tables_us"] = 1e3 * timed(torch, tables, reps) / n
        (_S_B, lM) = score.lik_tables(ctx, b, x, theta, False)

        def ais():
            for _ in range(n):
                ctx.call("fcd_score_ais_step", _lib.dptr(lM), _lib.dptr(f_state), _lib.dptr(r_all), NREG, U, G, 0.0, 1.0,
                         _lib.dptr(w), _lib.dptr(None), _lib.stream_ptr())
        ais()
        out["score_ais_step_0_to_1_us"] = 1e3 * timed(torch, ais, reps) / n
        out["table_path_us"] = out["lik_tables_us"] + out["score_ais_step_0_to_1_us"]
    ctx.check_device()
    print("U' = %d done" % U, file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="100,1000,10000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "membership_cost.json"))
    args = ap.parse_args()
    import torch
    import fcdiff_amd
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "gpu_tests_passed": GPU_TESTS}
    for U in [x for x in args.only.split(",") if x]:
        res["U%s" % U] = shape_run(torch, fcdiff_amd, int(U), args.reps)
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
