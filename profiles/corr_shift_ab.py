"""
A/B of the bench's K_corr leg between two builds of the library, interleaved: every run is a fresh `bench.py` process
(cfg3: 100 subjects, 200 regions, 1200 samples; Gibbs leg cut to two steps, no VB, no CPU baseline), run A with
FCDIFF_HIP_LIB pointing at the other build (the parent's), run B with the tree's own library.

    python profiles/corr_shift_ab.py --parent-lib PATH/libfcdiff_hip_parent.so [--runs 4] [--out profiles/corr_shift_ab.json]

Criterion (the project's usual one): every time of the new build lies inside the parent's range widened by its own width.
A child that does not end normally ends the series: nothing more is started on the device after it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(lib):
    env = dict(os.environ)
    env.pop("FCDIFF_HIP_LIB", None)
    if lib:
        env["FCDIFF_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--no-vb", "--no-cpu-baseline"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=240, universal_newlines=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit("bench.py ended with %d: series stopped" % p.returncode)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["corr"]["ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    (parent, new) = ([], [])
    for i in range(a.runs):
        parent.append(one(os.path.abspath(a.parent_lib)))
        new.append(one(None))
        print("run %d: parent %.4f ms, this build %.4f ms" % (i, parent[-1], new[-1]), flush=True)
    (lo, hi) = (min(parent), max(parent))
    width = hi - lo
    inside = all(lo - width <= x <= hi + width for x in new)
    res = {"leg": "bench.py K_corr, cfg3 (S=100, Nreg=200, T=1200), ms per call over 20 queued calls",
           "parent_ms": parent, "new_ms": new, "parent_range": [lo, hi], "allowed": [lo - width, hi + width],
           "new_inside": inside, "new_worst_over_ms": max(0.0, max(new) - (hi + width))}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
