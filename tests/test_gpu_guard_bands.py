"""
Every device entry point on buffers carved between guard bands (tests/guard_arena.py), the third sweep over the registry of
tests/caller_stream_cases.py after the caller's stream and the reused context: memory extent and alignment.

Every other suite takes its buffers from torch.empty -- 512-byte aligned blocks, sizes rounded up, small blocks packed into
shared segments -- so a kernel that touches a few elements outside a caller's buffer, or that works only at that alignment,
passes there.  Here each buffer of a case is a view into an allocation of its own, 16 bytes after a 256-byte boundary,
between two 4 KiB guards:

  sixteen-byte starts   per case and size, with the guards 0xFF (every fp64 guard element a NaN, every integer its largest)
                        and 0x00: the bits are those of the default allocation under BOTH fills -- no value from outside a
                        buffer has entered a result -- no guard byte has changed, and the context reports no device error;
  element starts        the three entry points that choose their path by the address (fcd_edge_cov_apply,
                        fcd_site_harmonize_apply, fcd_evidence_temper), one small shape on each side of each switch (even
                        and odd length; source, destination, both and neither 8 bytes off), against a NumPy loop of the
                        stated operation order and against the default allocation;
  refusals              every (entry point, argument) of the header's alignment table: that one argument 8 bytes (f_state:
                        1 byte) off, every other buffer at a sixteen-byte start.  FCD_ERR_ARG with the argument's name, every
                        output still the sentinel, every guard intact, and the context serves the case directly afterwards.
                        The refusal is made on the host: no kernel is ever handed an address it is not aligned for, here
                        or anywhere in this file.

What this does not cover: a read outside a buffer whose value is discarded is not seen, only its influence on a result, and
only within 4 KiB either way; the context's internal workspace is not guarded.  Nothing is timed and nothing has a tolerance:
every comparison is on bytes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402
import guard_arena as GA  # noqa: E402
import harmonize_ref as HR  # noqa: E402
from test_gpu_harmonize import HARM_CASES, random_parameters, raw_apply  # noqa: E402
from test_gpu_tangent import TG_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_CASES = R.CASES + HARM_CASES + TG_CASES
(ALIGN16, BY_ADDRESS) = GA.alignment_contract()

# the case's buffer that an entry point takes as the named argument, where the two names differ
BUFFER_OF = {("corr_clean", "fcd_corr_edges", "ts"): "resid", ("tangent_fit_apply", "fcd_tangent_fit", "ts"): "tc"}
# (case, entry point) pairs that get no refusal parameter, with the reason; another case reaches the entry point
NOT_REFUSED_HERE = {
    ("tangent_fit_apply", "fcd_tangent_apply"): "the case asserts on what its fit returned before it calls apply, and the "
                                                "refusal test lets no other call through; tangent_apply_sym_eigh has it",
}


def refusal_params():
    """(case, entry point, argument, buffer) for every listed argument that the case passes non-null"""
    out = []
    for case in ALL_CASES:
        spec = case.spec("small")
        for ep in case.entry_points:
            if (case.name, ep) in NOT_REFUSED_HERE:
                continue
            for arg in ALIGN16.get(ep, ()):
                buf = BUFFER_OF.get((case.name, ep, arg), arg)
                if buf in spec["inputs"] or buf in spec["outputs"]:
                    if arg == "ts":
                        assert spec["host"]["T"] % 2 == 0, (case.name, "the contract asks for 16 bytes when T is even")
                    out.append((case, ep, arg, buf))
    return out


REFUSALS = refusal_params()


@pytest.fixture(scope="module")
def gpu():
    import torch
    from fcdiff_amd import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return dict(torch=torch, lib=_lib, device=torch.device("cuda", 0))


def run_carved(gpu, ctx, case, size, start, fill):
    """the case on carved buffers -> (bits, arena); synchronises"""
    t = gpu["torch"]
    (din, dout, arena) = GA.carve(case, size, gpu["device"], start, fill)
    case.setup(ctx, din, dout)
    try:
        R.fill_outputs(dout)
        R.feed(case, din, R.pinned_inputs(case, size))
        t.cuda.synchronize()
        case.run(ctx, din, dout)
        t.cuda.synchronize()
        bits = R.snapshot(case, din, dout)
    finally:
        case.teardown(ctx)
    return bits, arena


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_sixteen_byte_starts_between_guards(gpu, case, size):
    (want, _stats) = R.fresh(case, size, gpu["device"])
    ctx = gpu["lib"].Context()
    try:
        for fill in GA.FILLS:
            (bits, arena) = run_carved(gpu, ctx, case, size, "sixteen", fill)
            assert arena.names_start_at(16) == sorted(arena.bands)
            bad = R.differing(bits, want)
            assert not bad, "%s/%s, guards 0x%02X: %s differ from the default allocation" % (case.name, size, fill, bad)
            changed = arena.check()
            assert not changed, "%s/%s, guards 0x%02X: stored outside a buffer: %s" % (case.name, size, fill, changed)
            assert ctx.stat("dev_err") == 0
            ctx.check_device()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, rc, message):
        Exception.__init__(self, message)
        (self.rc, self.message) = (rc, message)


class OnlyThis(object):
    """a context that lets ONE entry point through, stops at its return code, and answers every other call with success
    without making it: nothing but the call under test can write a buffer or launch a kernel"""

    def __init__(self, ctx, entry_point):
        (self.ctx, self.entry_point, self.lib, self.handle, self.skipped) = (ctx, entry_point, ctx.lib, ctx.handle, [])

    def call(self, name, *args):
        if name != self.entry_point:
            self.skipped.append(name)
            return
        rc = getattr(self.lib, name)(self.handle, *args)
        raise Refused(rc, self.lib.fcd_last_message(self.handle).decode())


@pytest.mark.parametrize("param", REFUSALS, ids=lambda p: "%s-%s-%s" % (p[0].name, p[1], p[2]))
def test_a_misaligned_argument_is_refused_on_the_host(gpu, param):
    (case, ep, arg, buf) = param
    (t, L, size) = (gpu["torch"], gpu["lib"], "small")
    (want, _stats) = R.fresh(case, size, gpu["device"])
    ctx = L.Context()
    try:
        (din, dout, arena) = GA.carve(case, size, gpu["device"], {"*": "sixteen", buf: "element"}, 0xFF)
        moved = arena.bands[buf].view
        assert moved.data_ptr() % 16 == moved.element_size() % 16 and arena.names_start_at(16) == sorted(set(arena.bands) - set([buf]))
        case.setup(ctx, din, dout)
        try:
            R.fill_outputs(dout)
            R.feed(case, din, R.pinned_inputs(case, size))
            t.cuda.synchronize()
            n_alloc = ctx.stat("n_alloc")
            with pytest.raises(Refused) as e:
                case.run(OnlyThis(ctx, ep), din, dout)
            t.cuda.synchronize()
            assert e.value.rc == L.FCD_ERR_ARG, (e.value.rc, e.value.message)
            assert "argument %s must be 16-byte aligned" % arg in e.value.message and e.value.message.startswith("fcd_"), e.value.message
            with pytest.raises(ValueError, match="argument %s must be 16-byte aligned" % arg):      # ... as the binding raises it
                L.check(e.value.rc, ctx.handle)
            for (k, v) in dout.items():
                assert bool((R.as_bytes(v) == R.SENTINEL).all()), "%s was written by a refused call" % k
            fed = case.make(size)
            for (k, v) in case.tensors(din).items():
                assert R.as_bytes(v).cpu().numpy().tobytes() == fed[k].tobytes(), "%s was written by a refused call" % k
            assert arena.check() == [] and ctx.stat("n_alloc") == n_alloc and ctx.stat("dev_err") == 0
        finally:
            case.teardown(ctx)
        (bits, arena) = run_carved(gpu, ctx, case, size, "sixteen", 0xFF)
        bad = R.differing(bits, want)
        assert not bad, "%s after a refusal: %s differ" % (case.name, bad)
        assert arena.check() == [] and ctx.stat("dev_err") == 0
        ctx.check_device()
    finally:
        ctx.close()


def test_the_correlation_wrappers_copy_a_view_that_the_library_would_refuse(gpu):
    """fcdiff_amd.corr takes device tensors as they come.  A (S, Nreg, T) view that starts one double into a flat buffer is
    contiguous and 8 bytes off a 16-byte boundary; with T even the library refuses it, so the wrappers pass an aligned copy,
    and the results are those of the same data in an allocation of its own."""
    from fcdiff_amd import corr
    t = gpu["torch"]
    (S, N, T) = (2, 5, 6)
    rng = np.random.default_rng(64)
    ts = rng.standard_normal((S, N, T))
    flat = t.zeros(1 + S * N * T, dtype=t.float64, device=gpu["device"])
    view = flat[1:].view(S, N, T)
    view.copy_(t.as_tensor(ts))
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    ctx = gpu["lib"].Context()
    try:
        with pytest.raises(ValueError, match="fcd_corr_edges: argument ts must be 16-byte aligned"):
            out = t.empty((R.tri(N), S), dtype=t.float64, device=gpu["device"])
            ctx.call("fcd_corr_edges", R.P(view), S, N, T, 0, R.P(out), R.ST())
        got = corr.correlations(view, ctx=ctx)
        assert got.tobytes() == corr.correlations(ts, ctx=ctx).tobytes()
        got = corr.partial_correlations(view, ctx=ctx)
        assert got.tobytes() == corr.partial_correlations(ts, ctx=ctx).tobytes()
        assert view.cpu().numpy().tobytes() == ts.tobytes()
        ctx.check_device()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# element-aligned starts: the entry points that choose their path by the address
# ---------------------------------------------------------------------------------------------------------------------
STARTS2 = [(a, b) for a in GA.STARTS for b in GA.STARTS]            # (source, destination)


def put(arena, name, a, start):
    """the NumPy array on the device, carved at this start"""
    import torch
    a = np.ascontiguousarray(a)
    v = arena.add(name, a.shape, torch.from_numpy(a).dtype, start)
    v.copy_(torch.from_numpy(a))
    return v


def sentinel(arena, name, shape, start):
    import torch
    v = arena.add(name, shape, torch.float64, start)
    R.as_bytes(v).fill_(R.SENTINEL)
    return v


def cov_apply_loop(x, z, z_ref, beta):
    """include/fcdiff_hip.h: d added up over q ascending from 0.0, one rounded product and one rounded sum per term"""
    d = np.zeros(x.shape)
    for q in range(z.shape[1]):
        d = d + beta[:, q][:, None] * (z[:, q] - z_ref[q])[None, :]
    return x - d


@pytest.mark.parametrize("fill", GA.FILLS, ids=lambda f: "guards%02X" % f)
@pytest.mark.parametrize("starts", STARTS2, ids=lambda s: "x_%s-out_%s" % s)
@pytest.mark.parametrize("S", [6, 7, 258])
def test_edge_cov_apply_at_every_start(gpu, S, starts, fill):
    """S even with both pointers at sixteen: 16 bytes per lane; anything else: 8.  37 rows: two blocks of rows; 258 columns:
    two blocks of columns, the second one two wide."""
    (t, dev) = (gpu["torch"], gpu["device"])
    (C, Q) = (37, 3)
    rng = np.random.default_rng([61, S])
    x = rng.standard_normal((C, S))
    x[rng.random((C, S)) < 0.1] = np.nan
    (z, z_ref, beta) = (rng.standard_normal((S, Q)) * 3.0 + 1.0, rng.standard_normal(Q), 0.1 * rng.standard_normal((C, Q)))
    want = cov_apply_loop(x, z, z_ref, beta)
    ctx = gpu["lib"].Context()
    try:
        arena = GA.Arena(dev, fill)
        other = "element" if "element" in starts else "sixteen"       # (every other pointer is read one element at a time)
        (xd, od) = (put(arena, "x", x, starts[0]), sentinel(arena, "out", (C, S), starts[1]))
        (zd, rd, bd) = (put(arena, "z", z, other), put(arena, "z_ref", z_ref, other), put(arena, "beta", beta, other))
        assert [v.data_ptr() % 16 for v in (xd, od)] == [16 % 16 if s == "sixteen" else 8 for s in starts]
        ctx.call("fcd_edge_cov_apply", R.P(xd), C, S, R.P(zd), Q, R.P(rd), R.P(bd), R.P(od), R.ST())
        t.cuda.synchronize()
        got = od.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (S, starts, fill)
        assert np.array_equal(np.isnan(got), np.isnan(x)) and xd.cpu().numpy().tobytes() == x.tobytes()
        assert arena.check() == [] and ctx.stat("dev_err") == 0
        # ... and the default allocation gives the same bits
        (x0, o0) = (t.as_tensor(x, device=dev), t.empty((C, S), dtype=t.float64, device=dev))
        (z0, r0, b0) = (t.as_tensor(z, device=dev), t.as_tensor(z_ref, device=dev), t.as_tensor(beta, device=dev))
        ctx.call("fcd_edge_cov_apply", R.P(x0), C, S, R.P(z0), Q, R.P(r0), R.P(b0), R.P(o0), R.ST())
        assert o0.cpu().numpy().tobytes() == got.tobytes()
        ctx.check_device()
    finally:
        ctx.close()


class _Env(object):
    pass


@pytest.mark.parametrize("fill", GA.FILLS, ids=lambda f: "guards%02X" % f)
@pytest.mark.parametrize("starts", STARTS2, ids=lambda s: "x_%s-out_%s" % s)
@pytest.mark.parametrize("S", [6, 7, 258])
def test_site_harmonize_apply_at_every_start(gpu, S, starts, fill):
    """the pattern of test_gpu_harmonize.py's apply test (views 8 bytes off a 16-byte boundary), with real guards and with
    every other pointer of the descriptor one element off as well"""
    (t, dev) = (gpu["torch"], gpu["device"])
    (C, B, Q) = (37, 3, 3)
    rng = np.random.default_rng([62, S])
    x = rng.standard_normal((C, S))
    x[rng.random((C, S)) < 0.1] = np.nan
    site = rng.integers(0, B, S).astype(np.uint8)
    site[0] = B - 1
    (z, z_ref) = (rng.standard_normal((S, Q)) * 3.0 + 1.0, rng.standard_normal(Q))
    par = random_parameters(rng, C, B, Q)
    want = HR.apply_loop(x, site, z, par["grand_mean"], par["beta"], par["shift"], par["scale"], z_ref)
    env = _Env()
    (env.lib, env.ctx) = (gpu["lib"], gpu["lib"].Context())
    try:
        arena = GA.Arena(dev, fill)
        other = "element" if "element" in starts else "sixteen"
        (xd, od) = (put(arena, "x", x, starts[0]), sentinel(arena, "out", (C, S), starts[1]))
        (sd, zd) = (put(arena, "site", site, other), put(arena, "z", z, other))
        dpar = dict((k, put(arena, k, v, other)) for (k, v) in par.items())
        raw_apply(env, xd, sd, zd, dpar, z_ref, od, B)
        t.cuda.synchronize()
        got = od.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (S, starts, fill)
        assert xd.cpu().numpy().tobytes() == x.tobytes()
        assert arena.check() == [] and env.ctx.stat("dev_err") == 0
        env.ctx.check_device()
    finally:
        env.ctx.close()


@pytest.mark.parametrize("fill", GA.FILLS, ids=lambda f: "guards%02X" % f)
@pytest.mark.parametrize("starts", STARTS2, ids=lambda s: "src_%s-dst_%s" % s)
@pytest.mark.parametrize("n", [6, 7, 1026, 1027])
def test_evidence_temper_at_every_start(gpu, n, starts, fill):
    """two tables in one launch, the second always at sixteen-byte starts: the kernel chooses per table.  n odd: a last element
    behind the pairs; 1026: more pairs than one workgroup has threads."""
    (t, dev) = (gpu["torch"], gpu["device"])
    rng = np.random.default_rng([63, n])
    (a, b) = (rng.standard_normal(n), rng.standard_normal(n + 1))
    a[0] = -np.inf
    ctx = gpu["lib"].Context()
    try:
        arena = GA.Arena(dev, fill)
        (sa, da) = (put(arena, "src0", a, starts[0]), sentinel(arena, "dst0", (n,), starts[1]))
        (sb, db) = (put(arena, "src1", b, "sixteen"), sentinel(arena, "dst1", (n + 1,), "sixteen"))
        src = (ctypes.c_void_p * 2)(sa.data_ptr(), sb.data_ptr())
        dst = (ctypes.c_void_p * 2)(da.data_ptr(), db.data_ptr())
        cnt = (ctypes.c_int64 * 2)(n, n + 1)
        ctx.call("fcd_evidence_temper", 0.375, 2, src, dst, cnt, R.ST())
        t.cuda.synchronize()
        assert da.cpu().numpy().tobytes() == (0.375 * a).tobytes() and db.cpu().numpy().tobytes() == (0.375 * b).tobytes()
        assert sa.cpu().numpy().tobytes() == a.tobytes() and arena.check() == [] and ctx.stat("dev_err") == 0
        # in place (dst[j] may be src[j]), at the source's start
        src2 = (ctypes.c_void_p * 2)(sa.data_ptr(), sb.data_ptr())
        ctx.call("fcd_evidence_temper", 1.0, 2, src2, src2, cnt, R.ST())
        t.cuda.synchronize()
        assert sa.cpu().numpy().tobytes() == a.tobytes() and arena.check() == []
        ctx.check_device()
    finally:
        ctx.close()
