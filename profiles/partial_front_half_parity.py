"""
Byte parity of two builds of fcd_corr_partial: the move of its front half (correlations -> dense -> live flags -> alpha ->
R_alpha) behind fcd_corr_shrunk_at must change no bit.  Every shape of tests/test_gpu_partial_corr.py (CASES, the long and
wide shapes, BATCHES), Ledoit-Wolf and alpha = 0.1 and 0, with Fisher z and without, a chunk knob of 7, shortened scans
through n_frames, and dead regions; out, alpha and info saved, then two such files compared byte for byte.  One library per
process:

    FCDIFF_HIP_LIB=<the parent commit's libfcdiff_hip.so> python profiles/partial_front_half_parity.py --save a.npz
    python profiles/partial_front_half_parity.py --save b.npz
    python profiles/partial_front_half_parity.py --compare a.npz b.npz

profiles/partial_front_half_parity.txt is the record of the run that went with the change.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NB = 16
CASES = [(2, 1, 9), (2, 3, 40), (3, 9, 41), (NB - 1, 3, 61), (NB - 1, 1, 8), (NB, 9, 64), (NB, 3, 9), (NB + 1, 1, 69), (NB + 1, 9, 10),
         (2 * NB + 1, 3, 133), (2 * NB + 1, 1, 20), (64, 1, 256), (64, 3, 33), (65, 9, 261), (65, 1, 40), (130, 3, 521), (130, 1, 66),
         (209, 3, 40), (520, 1, 64)]                                                                     # (N, S, T)
BATCHES = [(31, 5, 40), (32, 5, 41), (33, 17, 69), (65, 5, 40), (70, 17, 69), (40, 33, 300), (9, 33, 64), (9, 20, 700)]   # (S, N, T)


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
    import partial_corr_ref as PR
    from fcdiff_amd import _lib, corr
    torch.cuda.set_device(0)
    # the parent's library knows nothing of the entry points that came with the change: bind what it has
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.SIGNATURES if not hasattr(raw, k)]:
        print("not in %s: %s" % (_lib.LIB_PATH, name))
        del _lib.SIGNATURES[name]
    ctx = _lib.Context()
    saved = {}
    shapes = [(S, N, T, 1000 + 7 * N + T) for (N, S, T) in CASES] + [(S, N, T, 3000 + S + N) for (S, N, T) in BATCHES]
    for (S, N, T, seed) in shapes:
        ts = PR.make_series(seed, S, N, T)
        if N > 4:
            ts[S // 2, 1, :] = 0.25                     # a dead region
        rng = np.random.default_rng(seed)
        nfr = rng.integers(max(2, T // 2), T + 1, S).astype(np.int32)
        short = ts - ts.mean(axis=2, keepdims=True)
        for s in range(S):
            short[s] -= short[s][:, :nfr[s]].mean(axis=1, keepdims=True)
            short[s][:, nfr[s]:] = 0.0
        for (sh, fz, chunk, frames) in (("ledoit_wolf", False, None, False), (0.1, True, None, False), (0.0, False, None, False),
                                        ("ledoit_wolf", False, 7, False), ("ledoit_wolf", False, None, True)):
            if frames:
                (mode, value) = corr._check_shrinkage(sh)
                t = torch.as_tensor(short, device=ctx.device)
                out = torch.empty((N * (N - 1) // 2, S), dtype=torch.float64, device=ctx.device)
                alpha = torch.empty((S,), dtype=torch.float64, device=ctx.device)
                pinfo = torch.empty((S, 2), dtype=torch.int32, device=ctx.device)
                ctx.call("fcd_corr_partial", _lib.dptr(t), S, N, T, _lib.dptr(torch.as_tensor(nfr, device=ctx.device)), mode, value, 0,
                         _lib.dptr(out), _lib.dptr(alpha), _lib.dptr(pinfo), _lib.stream_ptr())
                (out, info) = (out.cpu().numpy(), dict(alpha=alpha.cpu().numpy(), n_live=pinfo[:, 0].cpu().numpy(), status=pinfo[:, 1].cpu().numpy()))
            else:
                (out, info) = corr.partial_correlations(ts, shrinkage=sh, fisher_z=fz, ctx=ctx, return_info=True, _max_chunk=chunk)
            key = "S%d_N%d_T%d_%s_z%d_c%s_f%d" % (S, N, T, sh, fz, chunk, frames)
            saved[key + "_out"] = out
            for k in ("alpha", "n_live", "status"):
                saved[key + "_" + k] = info[k]
    np.savez(args.save, **saved)
    print("%d arrays saved to %s" % (len(saved), args.save))
    return 0


if __name__ == "__main__":
    sys.exit(main())
