"""
Cost of the model evidence (UnsharedRegionFit.log_evidence, fcd_evidence.hip) on one MI355X, at cfg3's shape (Nreg 200,
H 50, 1024 chains):
  * fcd_evidence_energy at U in {1, 16, 100} against its byte floor -- lM, the f state and the r words read once, w read and
    written once -- and against fcd_score_ais_step (the same gathers, lM read once per chain word; with and without its
    beta * lM output, the speed-up quoted against the latter) on the same shapes in the same session;
  * fcd_evidence_temper (the four working tables in one launch) against its byte floor, every table read and written once;
  * one rung (energy + temper + sweep) against the plain sweep (fcd_gibbs_sweeps, one sweep per call) at U = 100, and
    whether the sweep dominates the rung;
  * log_evidence() end to end at U = 100 for n_anneal in {100, 1000, 10000}: time, ESS and log_evidence - lower.

    python profiles/evidence_cost.py [--reps 3] [--only 1,16,100] [--anneal 100,1000,10000]

Prints one JSON document (kept as profiles/evidence_cost.json).  Timings: HIP events around the calls, best of --reps,
after one warm-up call each.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E, nominal
NREG, H, G = 200, 50, 1024


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


def shape_run(torch, np, fcdiff_amd, U, reps):
    from fcdiff_amd import _lib, score, evidence
    gen = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(NREG, H, U, seed=100 + U)
    ctx = _lib.Context()
    C = NREG * (NREG - 1) // 2
    (S_B, lM) = score.lik_tables(ctx, torch.as_tensor(b, device="cuda"), torch.as_tensor(bt, device="cuda"), gen.theta(), False)
    ev = evidence.EvidenceEngine(ctx, S_B, lM, NREG, U, G, 0, 3, gen.gamma, gen.pi2())
    ev.temper(0.0)
    ev.sweep(0)
    ev.temper(0.5)
    ev.sweep(1)
    eng = ev.eng
    out = {"shape": {"Nreg": NREG, "U": U, "G": G}}
    n = 10

    def energy():
        for _ in range(n):
            ev.energy_step(0.5, 0.6)
    energy()
    us = 1e3 * timed(torch, energy, reps) / n
    floor = 72.0 * C * U + 24.0 * C + eng.GW * C * 64.0 + eng.GW * NREG * U * 8.0 + 2 * 8.0 * G
    out["energy_us"] = us
    out["energy_floor_MB"] = floor / 1e6
    out["energy_floor_us"] = floor / (HBM_PEAK_GBS * 1e3)
    out["energy_fraction_of_floor"] = out["energy_floor_us"] / us
    w = torch.zeros((G, U), dtype=torch.float64, device="cuda")

    def ais():
        for _ in range(n):
            ctx.call("fcd_score_ais_step", _lib.dptr(lM), _lib.dptr(eng.f_state), _lib.dptr(eng.r_bits), NREG, U, G, 0.5, 0.6,
                     _lib.dptr(w), _lib.dptr(None), _lib.stream_ptr())
    ais()
    out["score_ais_step_no_table_us"] = 1e3 * timed(torch, ais, reps) / n

    def ais_table():
        for _ in range(n):
            ctx.call("fcd_score_ais_step", _lib.dptr(lM), _lib.dptr(eng.f_state), _lib.dptr(eng.r_bits), NREG, U, G, 0.5, 0.6,
                     _lib.dptr(w), _lib.dptr(ev.work[1]), _lib.stream_ptr())
    ais_table()
    out["score_ais_step_us"] = 1e3 * timed(torch, ais_table, reps) / n          # (as score() calls it: with its beta * lM table)
    out["energy_speedup_over_score_ais_step"] = out["score_ais_step_no_table_us"] / us

    def temper():
        for _ in range(n):
            ev.temper(0.6)
    temper()
    tus = 1e3 * timed(torch, temper, reps) / n
    tbytes = 2 * 8.0 * sum(t.numel() for t in ev.base)
    out["temper_us"] = tus
    out["temper_floor_MB"] = tbytes / 1e6
    out["temper_floor_us"] = tbytes / (HBM_PEAK_GBS * 1e3)
    out["temper_fraction_of_floor"] = out["temper_floor_us"] / tus
    count = [2]

    def sweeps():
        for _ in range(n):
            ev.sweep(count[0])
            count[0] += 1
    sweeps()
    out["sweep_us"] = 1e3 * timed(torch, sweeps, reps) / n

    def rungs():
        for _ in range(n):
            ev.energy_step(0.5, 0.6)
            ev.temper(0.6)
            ev.sweep(count[0])
            count[0] += 1
    rungs()
    out["rung_us"] = 1e3 * timed(torch, rungs, reps) / n
    out["rung_over_sweep"] = out["rung_us"] / out["sweep_us"]
    out["sweep_dominates_rung"] = bool(out["sweep_us"] > 0.5 * out["rung_us"])
    ctx.check_device()
    print("U = %d done" % U, file=sys.stderr)
    return out


def ladder_run(torch, np, fcdiff_amd, anneal):
    """log_evidence() at cfg3's shape (U = 100) after a short sampler fit: what the estimate is worth at each ladder length."""
    gen = fcdiff_amd.UnsharedRegionModel()
    (_r, _t, _f, _ft, b, bt) = gen.sample_fast(NREG, H, 100, seed=0)
    fit = fcdiff_amd.fit.UnsharedRegionFit()
    fit.model, fit.b, fit.bt = fcdiff_amd.UnsharedRegionModel(), b, bt
    fit.method, fit.n_chains, fit.n_sweeps, fit.burn_in = "gibbs", G, 100, 20
    fit.run()
    fit.log_evidence(n_anneal=2)
    rows = []
    for T in anneal:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fit.log_evidence(n_anneal=T)
        res["seconds"] = time.perf_counter() - t0
        res["log_evidence_minus_lower"] = res["log_evidence"] - res["lower"]
        rows.append(res)
        print("n_anneal = %d done" % T, file=sys.stderr)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="1,16,100")
    ap.add_argument("--anneal", default="100,1000,10000")
    args = ap.parse_args()
    import numpy as np
    import torch
    import fcdiff_amd
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_GB_per_s_assumed": HBM_PEAK_GBS}
    for U in [x for x in args.only.split(",") if x]:
        res["U%s" % U] = shape_run(torch, np, fcdiff_amd, int(U), args.reps)
    anneal = [int(x) for x in args.anneal.split(",") if x]
    if anneal:
        res["ladder_cfg3"] = ladder_run(torch, np, fcdiff_amd, anneal)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
