"""
Byte parity of two builds of the permutation baselines (fcd_baseline.hip): all six entry points of the C ABI on seeded
inputs, every output array saved; then two such files compared byte for byte.  One library per process:

    FCDIFF_HIP_LIB=<the other build's libfcdiff_hip.so> python profiles/baseline_family_parity.py --save a.npz
    python profiles/baseline_family_parity.py --save b.npz
    python profiles/baseline_family_parity.py --compare a.npz b.npz

Inputs: the shapes of tests/baseline_ref.py, test_gpu_baseline.GROUP_EXTRA and tests/baseline_glm_ref.py; flags 0, 1, 2, 3 on
complete data and with 7 % NaN; thresholds 1.5 and 3.0 with tails 0, 1, 2; t asked for and NULL; the observed call (rows
NULL, P = 1); row 0 of every set of rows is the observed labelling (the identity).  profiles/baseline_family_merge.txt is
the record of the run that went with the merge of the kernel family.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUP_EXTRA = [(4, 100, 45, 20, 5), (3, 1000, 24, 3, 6), (4, 10, 9, 150, 7)]
THRESHOLDS = (1.5, 3.0)
NAN_FRACTION = 0.07


def compare(path_a, path_b):
    (a, b) = (np.load(path_a), np.load(path_b))
    if sorted(a.files) != sorted(b.files):
        print("the two files hold different arrays")
        return 1
    (n_bytes, differ) = (0, [])
    for k in a.files:
        (x, y) = (a[k], b[k])
        n_bytes += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            differ.append(k)
    print("%d arrays, %d bytes, %d arrays differ" % (len(a.files), n_bytes, len(differ)))
    for k in differ[:20]:
        print("  differs:", k)
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import torch
    import baseline_glm_ref as GR
    import baseline_ref as BR
    from fcdiff_amd import _lib, baseline, util
    torch.cuda.set_device(0)
    ctx = _lib.Context()
    (Pt, stream) = (_lib.dptr, _lib.stream_ptr())
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    out = {}

    def keep(name, **tensors):
        torch.cuda.synchronize()
        for (k, v) in tensors.items():
            out["%s/%s" % (name, k)] = v.cpu().numpy()

    def new(dtype, *sh):                # (filled: a value a call leaves alone is the same in both runs)
        return torch.full(sh, -1, dtype=dtype, device="cuda")

    def group(name, entry, head, tail_args, C, N, P, counts):
        o = dict(t=new(torch.float64, C), region=new(torch.float64, N), null_max_t=new(torch.float64, P),
                 null_max_region=new(torch.float64, P), count_t=new(torch.int64, C), count_region=new(torch.int64, N))
        extra = [new(torch.int64, C), new(torch.int64, C)] if counts else []
        ctx.call(entry, *head, *tail_args, Pt(o["t"]), Pt(o["region"]), Pt(o["null_max_t"]), Pt(o["null_max_region"]),
                 Pt(o["count_t"]), Pt(o["count_region"]), *[Pt(e) for e in extra], stream)
        keep(name, **o, **dict(zip(("n_controls", "n_patients"), extra)))

    def bits(name, entry, head, rows, P, C, flags):
        W = (C + 31) // 32
        for thr in THRESHOLDS:
            for tail in (0, 1, 2):
                for (rows_c, n) in ((rows, P), (None, 1)):
                    for want_t in (True, False):
                        (bt_, t) = (new(torch.int32, n, W), new(torch.float64, C) if want_t else None)
                        ctx.call(entry, *head, Pt(rows_c), n, thr, tail, *flags, Pt(bt_), Pt(t), stream)
                        tag = "%s/thr%g_tail%d_%s_t%d" % (name, thr, tail, "rows" if rows_c is not None else "observed", want_t)
                        keep(tag, bits=bt_, **({"t": t} if want_t else {}))

    for (i, shape) in enumerate(BR.SHAPES + GROUP_EXTRA):
        (N, H, U, P, _seed) = shape
        C = util.N_to_C(N)
        for f in (None, NAN_FRACTION):
            (b, bt, labels) = BR.make_data(*shape, f=f)
            labels[0] = np.arange(H + U) >= H
            (b_d, bt_d, lab_d) = (dev(b), dev(bt), dev(labels))
            head = (Pt(b_d), Pt(bt_d), C, H, U)
            name = "plain%d_%s" % (i, "nan" if f else "complete")
            group(name + "/group", "fcd_baseline_group_perm", head, (Pt(lab_d), P), C, N, P, False)
            bits(name + "/bits", "fcd_baseline_network_bits", head, lab_d, P, C, ())
            for flags in (0, 1, 2, 3):
                if (flags & 2) and (H < 2 or U < 2):
                    continue
                group("%s/group_opt%d" % (name, flags), "fcd_baseline_group_perm_opt", head, (Pt(lab_d), P, flags), C, N, P, True)
                bits("%s/bits_opt%d" % (name, flags), "fcd_baseline_network_bits_opt", head, lab_d, P, C, (flags,))
    for (i, shape) in enumerate(GR.SHAPES):
        (N, H, U, _Q, P, _seed) = shape
        C = util.N_to_C(N)
        (b, bt, z_b, z_bt, perms) = GR.make_data(*shape)
        (Wd, _info) = baseline.glm_design(z_b, z_bt)
        perms[0] = np.arange(H + U)
        (b_d, bt_d, W_d) = (dev(b), dev(bt), dev(Wd))
        perm_d = dev(perms.astype(np.uint16).view(np.int16))
        head = (Pt(b_d), Pt(bt_d), C, H, U, Pt(W_d), int(Wd.shape[1]))
        group("glm%d/group" % i, "fcd_baseline_group_glm", head, (Pt(perm_d), P), C, N, P, False)
        bits("glm%d/bits" % i, "fcd_baseline_network_bits_glm", head, perm_d, P, C, ())
    np.savez(args.save, **out)
    print("%d arrays, %d bytes -> %s (%s)" % (len(out), sum(v.nbytes for v in out.values()), args.save,
                                             os.environ.get("FCDIFF_HIP_LIB", "this tree's library")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
