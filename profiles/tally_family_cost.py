"""
The tallies over r_bits on two builds of the library, side by side: count, region-set, patient-group and patient-trait
tally (and fcd_vb_count_posterior) as timed by count_posterior_cost.py, region_sets_cost.py, patient_groups_cost.py and
patient_traits_cost.py, each script in a fresh process per repeat, alternately with FCDIFF_HIP_LIB = another build (the
parent commit's, made with the Makefile's SUF= / LIB= route) and this tree's library.

    python profiles/tally_family_cost.py ../libfcdiff_hip_parent.so [--rounds 5] [--out FILE]

Prints per figure the medians and spreads (largest - smallest repeat) of both builds, and writes one JSON document with
all repeats.  "within_parent_spread": this build's median is not above the other build's by more than that build's own spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = {
    "count_posterior_cost": ["--sweeps", "20", "--reps", "5", "--only", "cfg3"],
    "region_sets_cost": ["--sweeps", "20", "--reps", "5", "--calls", "200"],
    "patient_groups_cost": ["--sweeps", "20", "--reps", "7", "--calls", "200"],
    "patient_traits_cost": ["--sweeps", "20", "--reps", "7", "--calls", "200"],
}


def figures(name, doc):
    out = {}
    if name == "count_posterior_cost":
        out["count_tally_us"] = doc["cfg3"]["count_tally_us"]
        out["vb_count_posterior_us"] = doc["cfg3"]["vb_count_posterior_us"]
    elif name == "region_sets_cost":
        out["count_tally_us"] = doc["count_tally_us"]
        for (k, v) in doc["tally_us"].items():
            out["region_set_tally_us/" + k] = v["us"]
    elif name == "patient_groups_cost":
        for (k, v) in doc["tally_us"].items():
            out["patient_group_tally_us/" + k] = v["us"]
        out["region_set_tally_us/7_disjoint"] = doc["region_set_tally_us"]["us"]
    else:
        for (k, cases) in doc["tally_us"].items():
            for (q, v) in cases.items():
                out["patient_trait_tally_us/%s/%s" % (k, q)] = v["us"]
        out["patient_group_tally_us/with_7_region_sets"] = doc["patient_group_tally_us"]["us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--deadline", type=float, default=840.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tally_family_cost.json"))
    args = ap.parse_args()
    libs = {"parent": os.path.abspath(args.parent_lib), "new": os.path.join(ROOT, "fcdiff_amd", "libfcdiff_hip.so")}
    for p in libs.values():
        assert os.path.exists(p), p
    data = {}       # script -> figure -> build -> [repeats]
    t0 = time.time()
    rounds_done = 0
    device = None
    failed = None
    for r in range(args.rounds):
        if r > 0 and time.time() - t0 > args.deadline * r / (r + 1.0):       # (no room for another round like the ones so far)
            break
        for name in SCRIPTS:
            order = ("parent", "new") if r % 2 == 0 else ("new", "parent")
            for build in order:
                env = dict(os.environ, FCDIFF_HIP_LIB=libs[build])
                t1 = time.time()
                try:
                    run = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", name + ".py")] + SCRIPTS[name], env=env,
                                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
                except subprocess.TimeoutExpired:
                    failed = "%s on %s: no end after 240 s" % (name, build)
                    break
                if run.returncode != 0:
                    failed = "%s on %s: exit %d\n%s" % (name, build, run.returncode, run.stderr.decode()[-3000:])
                    break
                text = run.stdout.decode()
                doc = json.loads(text[text.index("{"):])
                device = doc.get("device", device)
                for (k, v) in figures(name, doc).items():
                    data.setdefault(name, {}).setdefault(k, {"parent": [], "new": []})[build].append(v)
                print("round %d %s %s: %.1f s" % (r, name, build, time.time() - t1), flush=True)
            if failed:
                break
        if failed:
            break
        rounds_done += 1
    res = {"device": device, "rounds": rounds_done, "scripts": {k: " ".join(v) for (k, v) in SCRIPTS.items()}, "figures": {}}
    worst = []
    for (name, figs) in data.items():
        for (k, v) in figs.items():
            row = {}
            for build in ("parent", "new"):
                xs = v[build]
                if xs:
                    row[build] = {"median_us": statistics.median(xs), "spread_us": max(xs) - min(xs), "all_us": xs}
            if "parent" in row and "new" in row:
                row["new_minus_parent_us"] = row["new"]["median_us"] - row["parent"]["median_us"]
                row["within_parent_spread"] = row["new_minus_parent_us"] <= row["parent"]["spread_us"]
                if not row["within_parent_spread"]:
                    worst.append("%s:%s" % (name, k))
            res["figures"]["%s:%s" % (name, k)] = row
    res["above_parent_spread"] = worst
    if failed:
        res["failed"] = failed
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for (k, row) in res["figures"].items():
        if "new_minus_parent_us" in row:
            print("%-70s parent %9.2f (+-%7.2f)  new %9.2f (+-%7.2f)  %s" % (k, row["parent"]["median_us"], row["parent"]["spread_us"],
                                                                       row["new"]["median_us"], row["new"]["spread_us"],
                                                                       "ok" if row["within_parent_spread"] else "ABOVE"))
    if failed:
        print("FAILED: " + failed)
        sys.exit(1)


if __name__ == "__main__":
    main()
