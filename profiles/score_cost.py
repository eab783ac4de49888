"""
Cost of scoring new patients (UnsharedRegionFit.score, fcd_score.hip) on one MI355X, at cfg3's shape (Nreg 200, H 50,
1024 chains) with U' in {1, 16, 100} new patients:
  * score() end to end, vb (q_R fixed point, tol 1e-8) and gibbs (n_anneal 200, n_sweeps 50: the defaults);
  * fcd_vb_patient_elbo alone, and one fcd_vb_update_qR of the scoring loop (without its read-back);
  * one AIS step alone (fcd_score_ais_step: the l_gu pass, the fold into w and the beta * lM table), against the byte floor
    of the step -- lM read once, beta * lM written once, the f state and the r words read once, w read and written once --
    and the rest of an AIS step as score() runs it (fcd_gibbs_region_tables + fcd_gibbs_r_step on the tempered table);
  * fcd_score_ais_finish alone.

    python profiles/score_cost.py [--reps 3] [--only 1,16,100]

Prints one JSON document.  Timings: HIP events around the calls, best of --reps, after one warm-up call each.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal
NREG, H, U_FIT, G = 200, 50, 50, 1024


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


def fits(fcdiff_amd):
    gen = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(NREG, H, U_FIT, seed=0)
    vb = fcdiff_amd.fit.UnsharedRegionFit()
    vb.model, vb.b, vb.bt, vb.max_iters = fcdiff_amd.UnsharedRegionModel(), b, bt, 5
    vb.run()
    gb = fcdiff_amd.fit.UnsharedRegionFit()
    gb.model, gb.b, gb.bt = fcdiff_amd.UnsharedRegionModel(), b, bt
    gb.method, gb.n_chains, gb.n_sweeps, gb.burn_in = "gibbs", G, 100, 20
    gb.run()
    return gen, vb, gb


def shape_run(torch, np, gen, vb, gb, U, reps):
    from fcdiff_amd import _lib, score
    from fcdiff_amd.gibbs import GibbsEngine
    (_r, _t, _f, _ft, _b, bt_new) = gen.sample_fast(NREG, H, U, seed=100 + U)
    out = {"shape": {"Nreg": NREG, "U_new": U, "G": G}}
    vb.score(bt_new)
    out["score_vb_ms"] = timed(torch, lambda: vb.score(bt_new), reps)
    res = vb.score(bt_new)
    out["score_vb_iters_max"] = int(res["iters"].max())
    out["score_vb_converged"] = int(res["converged"].sum())
    gb.score(bt_new, n_anneal=5, n_sweeps=2)
    out["score_gibbs_ms"] = timed(torch, lambda: gb.score(bt_new), reps)
    # the kernels alone, on a context of their own
    ctx = _lib.Context()
    C = NREG * (NREG - 1) // 2
    (S_B, lM) = score.lik_tables(ctx, vb._d["b"], torch.as_tensor(bt_new, device="cuda"), vb.model.theta(), False)
    hyper = score.hyper_block(ctx, vb.model.gamma, vb._pi2(), "cuda")
    lq_R = torch.full((NREG, U, 2), -np.log(2), dtype=torch.float64, device="cuda")
    o4 = torch.empty((U, 4), dtype=torch.float64, device="cuda")

    def elbo(n=10):
        for _ in range(n):
            ctx.call("fcd_vb_patient_elbo", _lib.dptr(vb._d["lq_F"]), _lib.dptr(lq_R), _lib.dptr(lM), _lib.dptr(hyper), NREG, U,
                     _lib.dptr(o4), _lib.stream_ptr())
    elbo(1)
    out["vb_patient_elbo_us"] = 1e3 * timed(torch, elbo, reps) / 10
    out["vb_patient_elbo_lM_GB_per_s"] = 72.0 * C * U / (out["vb_patient_elbo_us"] * 1e3)
    lq_R2 = lq_R.clone()

    def qr(n=10):
        for _ in range(n):
            ctx.call("fcd_vb_update_qR", _lib.dptr(vb._d["lq_F"]), _lib.dptr(lM), _lib.dptr(hyper), NREG, U,
                     _lib.EDGE_MODES["reference"], _lib.dptr(lq_R2), _lib.stream_ptr())
    qr(1)
    out["vb_update_qR_us"] = 1e3 * timed(torch, qr, reps) / 10          # one q_R update of the scoring loop, without its read-back
    lMw = lM.clone()
    eng = GibbsEngine(S_B, lMw, NREG, U, G, seed=3, edge_index="symmetric", ctx=ctx)
    eng.set_hyper(vb.model.gamma, vb._pi2())
    eng.init(0.05)
    w = torch.zeros((G, U), dtype=torch.float64, device="cuda")

    def step(n=10):
        for _ in range(n):
            ctx.call("fcd_score_ais_step", _lib.dptr(lM), _lib.dptr(eng.f_state), _lib.dptr(eng.r_bits), NREG, U, G, 0.5, 0.6,
                     _lib.dptr(w), _lib.dptr(lMw), _lib.stream_ptr())
    step(1)
    us = 1e3 * timed(torch, step, reps) / 10
    floor = 2 * 72.0 * C * U + eng.GW * C * 64.0 + eng.GW * NREG * U * 8.0 + 2 * 8.0 * G * U
    out["ais_step_us"] = us
    out["ais_step_floor_MB"] = floor / 1e6
    out["ais_step_floor_us"] = floor / (HBM_PEAK_GBS * 1e3)
    out["ais_step_fraction_of_floor"] = out["ais_step_floor_us"] / us

    def rest(n=10):
        for i in range(n):
            ctx.call("fcd_gibbs_region_tables", _lib.dptr(lMw), NREG, U, _lib.EDGE_MODES["symmetric"], _lib.dptr(eng.lMd),
                     _lib.stream_ptr())
            eng.r_step(score.SCORE_SWEEP0 + i)
    rest(1)
    out["region_tables_plus_r_step_us"] = 1e3 * timed(torch, rest, reps) / 10

    def fin(n=10):
        for _ in range(n):
            ctx.call("fcd_score_ais_finish", _lib.dptr(w), U, G, _lib.dptr(o4), _lib.stream_ptr())
    fin(1)
    out["ais_finish_us"] = 1e3 * timed(torch, fin, reps) / 10
    print("U' = %d done" % U, file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="1,16,100")
    args = ap.parse_args()
    import numpy as np
    import torch
    import fcdiff_amd
    torch.cuda.set_device(0)
    (gen, vb, gb) = fits(fcdiff_amd)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS}
    for U in args.only.split(","):
        res["U%s" % U] = shape_run(torch, np, gen, vb, gb, int(U), args.reps)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
