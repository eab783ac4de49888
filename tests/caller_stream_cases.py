"""
One small case per device entry point of include/fcdiff_hip.h (or per inseparable group of them), for the two suites that
run every entry point on a caller's stream (tests/test_gpu_caller_stream.py) and on a context that has just served another
family (tests/test_gpu_context_reuse.py).  tests/test_caller_stream_cases.py checks on the CPU that every prototype that
takes an fcd_stream is named by a case or exempt with a reason.  TEST INFRASTRUCTURE ONLY; nothing here touches the GPU at
import, and torch is imported inside alloc() only.

A case goes through the C ABI (ctx.call) with _lib.stream_ptr() read at call time and with device buffers that exist
before the call: no upload, no host read, so nothing in the case itself orders the call against its producers.

    case.make(size)              dict of NumPy arrays, the device inputs ("small" / "large"); deterministic
    case.host(size)              dict of host-side arguments (sizes, theta, seeds)
    case.alloc(size, device)     (dev_inputs, dev_outputs): torch tensors of the inputs' and outputs' shapes, uninitialised;
                                 dev_inputs["_host"] = case.host(size)
    case.setup(ctx, din, dout)   host-side state of the context the call needs (knobs, region sets, attached accumulators);
                                 may synchronise; once per context before the first run, undone by case.teardown(ctx)
    case.run(ctx, din, dout)     the call(s); no host read
    case.compared(din, dout)     the tensors a run leaves: every output, and the inputs the call updates in place
    case.refuse(ctx)             a call of the same family that the library must refuse -> its return code
    case.syncs_stream            the entry point waits for its own stream before it returns (the line that does is cited)
    case.extents(size)           the shape numbers, for "large differs from small"
    case.conditions(size)        asserts what the family's own reference asks of its inputs

Unsigned arrays travel as the signed type of the same width (torch has no arithmetic on them and none is needed).
Shapes: small = Nreg 17, H 3, U 3, G 64, T 40, Q 2; large = Nreg 33, H 5, U 7, G 128, T 100 (136 where the correlation
kernels should cut the time axis into slices), Q 9.  Families whose reference needs more subjects than that (the covariate
fit needs H > Q + 1) say so at their builder.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baseline_glm_ref as BG  # noqa: E402
import baseline_ref as BR  # noqa: E402
import corr_clean_ref as CC  # noqa: E402
import covariates_ref as CV  # noqa: E402
import f_pass_table_cases as FC  # noqa: E402
import partial_corr_ref as PC  # noqa: E402

SIZES = ("small", "large")
DIMS = {"small": dict(N=17, H=3, U=3, G=64, T=40, Q=2, P=32, K=2, J=2),
        "large": dict(N=33, H=5, U=7, G=128, T=100, Q=9, P=40, K=3, J=3)}
SYM = 1                                    # FCD_EDGE_SYMMETRIC
MISSING = 1                                # FCD_DATA_NAN_MISSING
W_PER_EDGE = 2                             # FCD_W_PER_EDGE
SENTINEL = 0xA5                            # the byte every output holds before a run
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


def tri(N):
    return N * (N - 1) // 2


def _dev(a):
    a = np.ascontiguousarray(a)
    return a.view(_SIGNED[a.dtype]) if a.dtype in _SIGNED else a


def _hp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _lib():
    from fcdiff_amd import _lib as L
    return L


def P(t):
    return _lib().dptr(t)


def ST():
    return _lib().stream_ptr()


class Case(object):
    def __init__(self, name, entry_points, build, call, syncs_stream=False, knobs=None, setup=None, teardown=None,
                 conditions=None):
        (self.name, self.entry_points, self._build, self._call) = (name, tuple(entry_points), build, call)
        (self.syncs_stream, self.knobs) = (bool(syncs_stream), dict(knobs or {}))
        (self._setup, self._teardown, self._conditions) = (setup, teardown, conditions)
        self._built = {}

    def spec(self, size):
        """the case at one size, built once: inputs, outputs (name -> (shape, dtype)), inout, host, extents"""
        if size not in self._built:
            s = self._build(dict(DIMS[size]))
            s["inputs"] = dict((k, _dev(v)) for (k, v) in s["inputs"].items())
            s.setdefault("inout", ())
            s.setdefault("host", {})
            self._built[size] = s
        return self._built[size]

    def make(self, size):
        return dict((k, v.copy()) for (k, v) in self.spec(size)["inputs"].items())

    def host(self, size):
        return self.spec(size)["host"]

    def extents(self, size):
        """every shape number of the case: the shapes of its inputs and outputs and the integers among its host arguments"""
        s = self.spec(size)
        ext = dict(("in." + k, v.shape) for (k, v) in s["inputs"].items())
        ext.update(("out." + k, tuple(v[0])) for (k, v) in s["outputs"].items())
        ext.update(("host." + k, v) for (k, v) in s["host"].items() if isinstance(v, int))
        return ext

    def conditions(self, size):
        if self._conditions is not None:
            self._conditions(self.spec(size))

    def alloc(self, size, device):
        import torch
        s = self.spec(size)
        din = dict((k, torch.empty(v.shape, dtype=_tdtype(v.dtype), device=device)) for (k, v) in s["inputs"].items())
        (din["_host"], din["_inout"]) = (s["host"], tuple(s["inout"]))
        dout = dict((k, torch.empty(tuple(shape), dtype=_tdtype(dtype), device=device)) for (k, (shape, dtype)) in s["outputs"].items())
        return din, dout

    def setup(self, ctx, din, dout):
        for (k, v) in self.knobs.items():
            ctx.set_knob(k, v)
        if self._setup is not None:
            self._setup(ctx, din, dout, din["_host"])

    def teardown(self, ctx):
        if self._teardown is not None:
            self._teardown(ctx)
        for k in self.knobs:
            ctx.set_knob(k, 0)

    def run(self, ctx, din, dout):
        self._call(ctx, din, dout, din["_host"])

    @staticmethod
    def tensors(din):
        """the device tensors among dev_inputs"""
        return dict((k, v) for (k, v) in din.items() if not k.startswith("_"))

    @staticmethod
    def compared(din, dout):
        return [("out." + k, dout[k]) for k in sorted(dout)] + [("inout." + k, din[k]) for k in din["_inout"]]

    def refuse(self, ctx):
        """
        The return code of a call of this family that the library must refuse: the case's first entry point with every pointer
        null and every size zero (each entry point checks its pointers and sizes on the host before any device work -- the
        refusal every family's own suite tests).
        """
        name = self.entry_points[0]
        args = []
        for t in _lib().SIGNATURES[name][1][1:]:
            args.append(0 if t in (C.c_int, C.c_int64, C.c_uint64) else 0.0 if t is C.c_double else None)
        return getattr(ctx.lib, name)(ctx.handle, *args)


def _tdtype(dtype):
    import torch
    dt = np.dtype(dtype)
    return torch.from_numpy(np.empty(0, dtype=_SIGNED.get(dt, dt))).dtype


# ---------------------------------------------------------------------------------------------------------------------
# shared data
# ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def model_data(d, K=None):
    """(theta, gamma, pi2, b, bt) of the default model at the case's shape; K: sessions"""
    def go():
        (m, b, bt) = FC.data(d["N"], d["H"], d["U"], 11 + d["N"], sessions=K)
        return (np.ascontiguousarray(m.theta()), np.array(m.gamma, dtype=np.float64), np.array(m.pi2(), dtype=np.float64), b, bt)
    return _memo(("data", d["N"], d["H"], d["U"], K), go)


def hyper_of(gamma, pi2):
    return np.concatenate([np.log(gamma), np.log(pi2), np.zeros(3)])


def tables(d):
    """S_B (C, 3), lM (C, U, 3, 3) of the one-scan data, from the oracle"""
    def go():
        (_th, _g, _p, b, bt) = model_data(d)
        return FC.one_scan_tables(FC.model(), b, bt)
    (S_B, lM) = _memo(("tables", d["N"], d["H"], d["U"]), go)
    return np.ascontiguousarray(S_B), np.ascontiguousarray(lM)


def q_logs(d, U=None, seed=3):
    """normalised lq_F (C, 1, 3) and lq_R (Nreg, U, 2)"""
    U = d["U"] if U is None else U
    rng = np.random.default_rng([seed, d["N"], U])
    qF = rng.uniform(0.05, 1.0, (tri(d["N"]), 1, 3))
    qR = rng.uniform(0.05, 1.0, (d["N"], U, 2))
    return np.log(qF / qF.sum(axis=2, keepdims=True)), np.log(qR / qR.sum(axis=2, keepdims=True))


def chain_state(d, U=None, seed=5):
    """a packed chain state: f_state (GW, C, 64) uint8 in {0, 1, 2}, r_bits (GW, Nreg, U) uint64, about a third of the bits set"""
    U = d["U"] if U is None else U
    rng = np.random.default_rng([seed, d["N"], U, d["G"]])
    GW = (d["G"] + 63) // 64
    f = rng.integers(0, 3, (GW, tri(d["N"]), 64), dtype=np.uint8)
    r = rng.integers(0, 2 ** 63, (GW, d["N"], U), dtype=np.uint64) & rng.integers(0, 2 ** 63, (GW, d["N"], U), dtype=np.uint64)
    return f, r


def model_hyper(d):
    (_th, gamma, pi2, _b, _bt) = model_data(d)
    return hyper_of(gamma, pi2)


def nan_some(a, seed, share=0.1):
    a = a.copy()
    a[np.random.default_rng(seed).random(a.shape) < share] = np.nan
    return a


CASES = []


def case(name, entry_points, **kw):
    def deco(build):
        call = kw.pop("call")
        CASES.append(Case(name, entry_points, build, call, **kw))
        return build
    return deco


# ---------------------------------------------------------------------------------------------------------------------
# hyper-parameters and likelihood tables
# ---------------------------------------------------------------------------------------------------------------------
def _call_hyper_set(ctx, i, o, h):
    ctx.call("fcd_hyper_set", P(o["hyper"]), _hp(h["gamma"]), _hp(h["pi2"]), ST())


@case("hyper_set", ["fcd_hyper_set"], call=_call_hyper_set)
def _b_hyper_set(d):
    (_th, gamma, pi2, _b, _bt) = model_data(d)
    # no device input and one shape only (ONE_SHAPE): the sizes differ in the values
    if d["N"] != 17:
        (gamma, pi2) = (np.ascontiguousarray(gamma[::-1]), np.array([0.75, 0.25]))
    return dict(inputs={}, outputs={"hyper": ((8,), np.float64)}, host=dict(gamma=gamma, pi2=pi2))


def _lik_io(d, K=None, missing=False, lp=True, shared=False, G=None):
    (th, _g, _p, b, bt) = model_data(d, K)
    if missing:
        (b, bt) = (nan_some(b, 21), nan_some(bt, 22))
    (C_, H, U) = (tri(d["N"]), d["H"], d["U"])
    outs = {"S_B": ((C_, 3), np.float64)}
    if shared:
        outs["L"] = ((C_, 3, 3) if G is None else (C_, G, 3, 3), np.float64)
    else:
        outs["lM"] = ((C_, U, 3, 3), np.float64)
        if lp:
            outs["lp_B_g_F"] = ((C_, H, 3), np.float64)
    if missing:
        outs["n_missing2"] = ((2,), np.int64)
    return dict(inputs={"b": b, "bt": bt}, outputs=outs, host=dict(theta=th, C=C_, H=H, U=U, K=K or 1))


def _call_lik_tables(ctx, i, o, h):
    ctx.call("fcd_lik_tables", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], _hp(h["theta"]), P(o["S_B"]), P(o["lM"]),
             P(o["lp_B_g_F"]), P(o["p_Bt_g_Ft"]), ST())


@case("lik_tables", ["fcd_lik_tables"], call=_call_lik_tables)
def _b_lik_tables(d):
    s = _lik_io(d)
    s["outputs"]["p_Bt_g_Ft"] = ((s["host"]["C"], d["U"], 3), np.float64)
    return s


def _call_lik_tables_ex(ctx, i, o, h):
    ctx.call("fcd_lik_tables_ex", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], _hp(h["theta"]), P(o["S_B"]), P(o["lM"]),
             P(o["lp_B_g_F"]), P(o["p_Bt_g_Ft"]), MISSING, P(o["n_missing2"]), ST())


@case("lik_tables_ex", ["fcd_lik_tables_ex"], call=_call_lik_tables_ex)
def _b_lik_tables_ex(d):
    s = _lik_io(d, missing=True)
    s["outputs"]["p_Bt_g_Ft"] = ((s["host"]["C"], d["U"], 3), np.float64)
    return s


def _call_lik_shared(ctx, i, o, h):
    ctx.call("fcd_lik_shared_tables", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], _hp(h["theta"]), P(o["S_B"]), P(o["L"]),
             MISSING, P(o["n_missing2"]), ST())


@case("lik_shared_tables", ["fcd_lik_shared_tables"], call=_call_lik_shared)
def _b_lik_shared(d):
    return _lik_io(d, missing=True, shared=True)


def _call_lik_sessions(ctx, i, o, h):
    ctx.call("fcd_lik_tables_sessions", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], h["K"], _hp(h["theta"]), P(o["S_B"]),
             P(o["lM"]), P(o["lp_B_g_F"]), MISSING, P(o["n_missing2"]), ST())


@case("lik_tables_sessions", ["fcd_lik_tables_sessions"], call=_call_lik_sessions)
def _b_lik_sessions(d):
    return _lik_io(d, K=d["K"], missing=True)


def _call_lik_shared_sessions(ctx, i, o, h):
    ctx.call("fcd_lik_shared_tables_sessions", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], h["K"], _hp(h["theta"]),
             P(o["S_B"]), P(o["L"]), MISSING, P(o["n_missing2"]), ST())


@case("lik_shared_tables_sessions", ["fcd_lik_shared_tables_sessions"], call=_call_lik_shared_sessions)
def _b_lik_shared_sessions(d):
    return _lik_io(d, K=d["K"], missing=True, shared=True)


def _noise_io(d, **kw):
    s = _lik_io(d, K=d["K"], missing=True, **kw)
    rng = np.random.default_rng([77, d["N"]])
    s["inputs"]["var_b"] = rng.uniform(0.0, 4e-4, size=d["H"])
    s["inputs"]["var_bt"] = rng.uniform(0.0, 9e-4, size=(d["U"], d["K"]))
    return s


def _call_lik_noise(ctx, i, o, h):
    ctx.call("fcd_lik_tables_noise", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], h["K"], _hp(h["theta"]), P(i["var_b"]),
             P(i["var_bt"]), P(o["S_B"]), P(o["lM"]), P(o["lp_B_g_F"]), MISSING, P(o["n_missing2"]), ST())


@case("lik_tables_noise", ["fcd_lik_tables_noise"], call=_call_lik_noise)
def _b_lik_noise(d):
    return _noise_io(d)


def _call_lik_shared_noise(ctx, i, o, h):
    ctx.call("fcd_lik_shared_tables_noise", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], h["K"], _hp(h["theta"]),
             P(i["var_b"]), P(i["var_bt"]), P(o["S_B"]), P(o["L"]), MISSING, P(o["n_missing2"]), ST())


@case("lik_shared_tables_noise", ["fcd_lik_shared_tables_noise"], call=_call_lik_shared_noise)
def _b_lik_shared_noise(d):
    return _noise_io(d, shared=True)


def _group_csr(U, J):
    """patients dealt to J groups in turn -> order (U,) int32 sorted by group, offsets (J + 1,) int64"""
    labels = np.arange(U) % J
    order = np.argsort(labels, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=J))]).astype(np.int64)
    return order, offsets


def _call_lik_grouped(ctx, i, o, h):
    ctx.call("fcd_lik_grouped_tables", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], h["K"], _hp(h["theta"]),
             P(i.get("var_b")), P(i.get("var_bt")), P(i["order"]), P(i["offsets"]), h["J"], P(o["S_B"]), P(o["L"]), MISSING,
             P(o["n_missing2"]), ST())


def _grouped_io(d, noise):
    s = _noise_io(d, shared=True, G=d["J"]) if noise else _lik_io(d, K=d["K"], missing=True, shared=True, G=d["J"])
    (s["inputs"]["order"], s["inputs"]["offsets"]) = _group_csr(d["U"], d["J"])
    s["host"] = dict(s["host"], J=d["J"])
    return s


@case("lik_grouped_tables_sigma", ["fcd_lik_grouped_tables"], call=_call_lik_grouped)
def _b_lik_grouped_sigma(d):
    return _grouped_io(d, False)


@case("lik_grouped_tables_records", ["fcd_lik_grouped_tables"], call=_call_lik_grouped)
def _b_lik_grouped_records(d):
    return _grouped_io(d, True)


def _call_lik_weighted(ctx, i, o, h):
    ctx.call("fcd_lik_weighted_tables", P(i["lM"]), P(i["resp"]), h["C"], h["U"], h["J"], P(o["L"]), ST())


@case("lik_weighted_tables", ["fcd_lik_weighted_tables"], call=_call_lik_weighted)
def _b_lik_weighted(d):
    (_S_B, lM) = tables(d)
    resp = np.random.default_rng([8, d["N"]]).uniform(0.1, 1.0, (d["U"], d["J"]))
    resp /= resp.sum(axis=1, keepdims=True)
    resp[0] = 0.0
    resp[0, 0] = 1.0                                   # an exact zero weight
    return dict(inputs={"lM": lM, "resp": resp}, outputs={"L": ((tri(d["N"]), d["J"], 3, 3), np.float64)},
                host=dict(C=tri(d["N"]), U=d["U"], J=d["J"]))


def _call_subtype_loglik(ctx, i, o, h):
    ctx.call("fcd_vb_subtype_loglik", P(i["lq_F"]), P(i["lq_R"]), P(i["lM"]), h["N"], h["U"], h["J"], P(o["E"]), ST())


@case("vb_subtype_loglik", ["fcd_vb_subtype_loglik"], call=_call_subtype_loglik)
def _b_subtype_loglik(d):
    (_S_B, lM) = tables(d)
    (lq_F, lq_R) = q_logs(d, U=d["J"])
    return dict(inputs={"lq_F": lq_F, "lq_R": lq_R, "lM": lM}, outputs={"E": ((d["U"], d["J"]), np.float64)},
                host=dict(N=d["N"], U=d["U"], J=d["J"]))


# ---------------------------------------------------------------------------------------------------------------------
# connection posteriors
# ---------------------------------------------------------------------------------------------------------------------
def _conn_io(d, K=None, counts=False, noise=False):
    (th, _g, _p, _b, bt) = model_data(d, K)
    bt = nan_some(bt, 23)
    (C_, U) = (tri(d["N"]), d["U"])
    ins = {"bt": bt}
    if counts:
        ins["counts"] = np.random.default_rng([9, d["N"]]).integers(0, 50, (C_, U, 3, 3)).astype(np.uint32)
    else:
        (ins["lq_F"], ins["lq_R"]) = q_logs(d)
    if noise:
        ins["var_bt"] = np.random.default_rng([78, d["N"]]).uniform(0.0, 9e-4, size=(U, K))
    outs = {"p_T": ((C_, U), np.float64), "p_F_tilde": ((C_, U, 3), np.float64), "p_changed": ((C_, U), np.float64)}
    return dict(inputs=ins, outputs=outs, host=dict(theta=th, N=d["N"], U=U, K=K or 1))


def _call_conn(ctx, i, o, h):
    ctx.call("fcd_conn_posterior", P(i["bt"]), h["N"], h["U"], _hp(h["theta"]), P(i.get("counts")), P(i.get("lq_F")),
             P(i.get("lq_R")), P(o["p_T"]), P(o["p_F_tilde"]), P(o["p_changed"]), ST())


@case("conn_posterior_vb", ["fcd_conn_posterior"], call=_call_conn)
def _b_conn_vb(d):
    s = _conn_io(d)
    s["inputs"]["bt"] = model_data(d)[4]               # (without the flag a NaN spreads: complete data)
    return s


def _call_conn_ex(ctx, i, o, h):
    ctx.call("fcd_conn_posterior_ex", P(i["bt"]), h["N"], h["U"], _hp(h["theta"]), P(i.get("counts")), P(i.get("lq_F")),
             P(i.get("lq_R")), MISSING, P(o["p_T"]), P(o["p_F_tilde"]), P(o["p_changed"]), ST())


@case("conn_posterior_ex_counts", ["fcd_conn_posterior_ex"], call=_call_conn_ex)
def _b_conn_ex(d):
    return _conn_io(d, counts=True)


def _call_conn_sessions(ctx, i, o, h):
    ctx.call("fcd_conn_posterior_sessions", P(i["bt"]), h["N"], h["U"], h["K"], _hp(h["theta"]), P(i.get("counts")),
             P(i.get("lq_F")), P(i.get("lq_R")), MISSING, P(o["p_T"]), P(o["p_F_tilde"]), P(o["p_changed"]), ST())


@case("conn_posterior_sessions", ["fcd_conn_posterior_sessions"], call=_call_conn_sessions)
def _b_conn_sessions(d):
    return _conn_io(d, K=d["K"])


def _call_conn_noise(ctx, i, o, h):
    ctx.call("fcd_conn_posterior_noise", P(i["bt"]), h["N"], h["U"], h["K"], _hp(h["theta"]), P(i["var_bt"]), P(i.get("counts")),
             P(i.get("lq_F")), P(i.get("lq_R")), MISSING, P(o["p_T"]), P(o["p_F_tilde"]), P(o["p_changed"]), ST())


@case("conn_posterior_noise", ["fcd_conn_posterior_noise"], call=_call_conn_noise)
def _b_conn_noise(d):
    return _conn_io(d, K=d["K"], counts=True, noise=True)


# ---------------------------------------------------------------------------------------------------------------------
# variational updates, theta objectives, post-fit reductions
# ---------------------------------------------------------------------------------------------------------------------
def _vb_io(d, names, outs, inout=()):
    (S_B, lM) = tables(d)
    (lq_F, lq_R) = q_logs(d)
    pool = dict(S_B=S_B, lM=lM, lq_F=lq_F, lq_R=lq_R, hyper=model_hyper(d))
    return dict(inputs=dict((k, pool[k]) for k in names), outputs=outs, inout=inout, host=dict(N=d["N"], U=d["U"]))


def _call_qF(ctx, i, o, h):
    ctx.call("fcd_vb_update_qF", P(i["lq_R"]), P(i["S_B"]), P(i["lM"]), P(i["hyper"]), h["N"], h["U"], P(o["lq_F"]), ST())


@case("vb_update_qF", ["fcd_vb_update_qF"], call=_call_qF)
def _b_qF(d):
    return _vb_io(d, ("lq_R", "S_B", "lM", "hyper"), {"lq_F": ((tri(d["N"]), 1, 3), np.float64)})


def _call_qR(ctx, i, o, h):
    ctx.call("fcd_vb_update_qR", P(i["lq_F"]), P(i["lM"]), P(i["hyper"]), h["N"], h["U"], SYM, P(i["lq_R"]), ST())


for (_name, _form) in (("vb_update_qR_gather", 1), ("vb_update_qR_region_major", 2)):
    case(_name, ["fcd_vb_update_qR"], call=_call_qR, knobs={"qr_form": _form})(
        lambda d: _vb_io(d, ("lq_F", "lM", "hyper", "lq_R"), {}, inout=("lq_R",)))


def _call_energy(ctx, i, o, h):
    ctx.call("fcd_vb_energy", P(i["lq_F"]), P(i["lq_R"]), P(i["S_B"]), P(i["lM"]), P(i["hyper"]), h["N"], h["U"], P(o["terms6"]),
             ST())


@case("vb_energy", ["fcd_vb_energy"], call=_call_energy)
def _b_energy(d):
    return _vb_io(d, ("lq_F", "lq_R", "S_B", "lM", "hyper"), {"terms6": ((6,), np.float64)})


def _call_theta_step(ctx, i, o, h):
    ctx.call("fcd_vb_theta_step", P(i["lq_F"]), P(i["lq_R"]), h["N"], h["U"], P(o["out4"]), P(i["hyper"]), ST())


@case("vb_theta_step", ["fcd_vb_theta_step"], call=_call_theta_step)
def _b_theta_step(d):
    return _vb_io(d, ("lq_F", "lq_R", "hyper"), {"out4": ((4,), np.float64)}, inout=("hyper",))


def _call_sub_weights(ctx, i, o, h):
    ctx.call("fcd_theta_sub_weights_vb", P(i["lq_F"]), P(i["lq_R"]), h["N"], h["U"], P(o["W"]), ST())


@case("theta_sub_weights_vb", ["fcd_theta_sub_weights_vb"], call=_call_sub_weights)
def _b_sub_weights(d):
    return _vb_io(d, ("lq_F", "lq_R"), {"W": ((tri(d["N"]), d["U"], 3, 3), np.float64)})


def _objective_io(d, n_out, missing=False, with_b=False):
    (th, _g, _p, b, bt) = model_data(d)
    if missing:
        (b, bt) = (nan_some(b, 24), nan_some(bt, 25))
    W = np.random.default_rng([10, d["N"]]).uniform(0.0, 1.0, (tri(d["N"]), d["U"], 3, 3))
    ins = {"bt": bt, "W": W}
    if with_b:
        ins["b"] = b
    return dict(inputs=ins, outputs={"out": ((n_out,), np.float64)}, host=dict(theta=th, C=tri(d["N"]), H=d["H"], U=d["U"]))


def _call_sub_objective(ctx, i, o, h):
    ctx.call("fcd_theta_sub_objective", P(i["bt"]), P(i["W"]), h["C"], h["U"], _hp(h["theta"]), P(o["out"]), ST())


case("theta_sub_objective", ["fcd_theta_sub_objective"], call=_call_sub_objective)(lambda d: _objective_io(d, 3))


def _call_sub_objective_ex(ctx, i, o, h):
    ctx.call("fcd_theta_sub_objective_ex", P(i["bt"]), P(i["W"]), h["C"], h["U"], _hp(h["theta"]), MISSING, P(o["out"]), ST())


case("theta_sub_objective_ex", ["fcd_theta_sub_objective_ex"], call=_call_sub_objective_ex)(
    lambda d: _objective_io(d, 3, missing=True))


def _call_full_objective(ctx, i, o, h):
    ctx.call("fcd_theta_full_objective", P(i["b"]), P(i["bt"]), P(i["W"]), h["C"], h["H"], h["U"], _hp(h["theta"]), P(o["out"]),
             ST())


case("theta_full_objective", ["fcd_theta_full_objective"], call=_call_full_objective)(
    lambda d: _objective_io(d, 9, with_b=True))


def _call_full_objective_ex(ctx, i, o, h):
    ctx.call("fcd_theta_full_objective_ex", P(i["b"]), P(i["bt"]), P(i["W"]), h["C"], h["H"], h["U"], _hp(h["theta"]), MISSING,
             P(o["out"]), ST())


case("theta_full_objective_ex", ["fcd_theta_full_objective_ex"], call=_call_full_objective_ex)(
    lambda d: _objective_io(d, 9, missing=True, with_b=True))


def _per_edge(build):
    """the objective with FCD_W_PER_EDGE: one weight table per edge for every patient, W (C, 1, 3, 3)"""
    def go(d):
        s = build(d)
        s["inputs"]["W"] = np.ascontiguousarray(s["inputs"]["W"][:, :1])
        return s
    return go


def _call_sub_objective_edge(ctx, i, o, h):
    ctx.call("fcd_theta_sub_objective_ex", P(i["bt"]), P(i["W"]), h["C"], h["U"], _hp(h["theta"]), MISSING | W_PER_EDGE, P(o["out"]),
             ST())


def _call_full_objective_edge(ctx, i, o, h):
    ctx.call("fcd_theta_full_objective_ex", P(i["b"]), P(i["bt"]), P(i["W"]), h["C"], h["H"], h["U"], _hp(h["theta"]),
             MISSING | W_PER_EDGE, P(o["out"]), ST())


case("theta_sub_objective_per_edge", ["fcd_theta_sub_objective_ex"], call=_call_sub_objective_edge)(
    _per_edge(lambda d: _objective_io(d, 3, missing=True)))
case("theta_full_objective_per_edge", ["fcd_theta_full_objective_ex"], call=_call_full_objective_edge)(
    _per_edge(lambda d: _objective_io(d, 9, missing=True, with_b=True)))


def _call_count_posterior(ctx, i, o, h):
    ctx.call("fcd_vb_count_posterior", P(i["lq_R"]), h["N"], h["U"], P(o["p_patient"]), P(o["p_region"]), ST())


@case("vb_count_posterior", ["fcd_vb_count_posterior"], call=_call_count_posterior)
def _b_count_posterior(d):
    return _vb_io(d, ("lq_R",), {"p_patient": ((d["U"], d["N"] + 1), np.float64), "p_region": ((d["N"], d["U"] + 1), np.float64)})


def _call_vb_coanomaly(ctx, i, o, h):
    ctx.call("fcd_vb_coanomaly", P(i["lq_R"]), h["N"], h["U"], P(o["region"]), P(o["patient"]), ST())


@case("vb_coanomaly", ["fcd_vb_coanomaly"], call=_call_vb_coanomaly)
def _b_vb_coanomaly(d):
    return _vb_io(d, ("lq_R",), {"region": ((d["N"], d["N"]), np.float64), "patient": ((d["U"], d["U"]), np.float64)})


def _call_patient_elbo(ctx, i, o, h):
    ctx.call("fcd_vb_patient_elbo", P(i["lq_F"]), P(i["lq_R"]), P(i["lM"]), P(i["hyper"]), h["N"], h["U"], P(o["out4"]), ST())


@case("vb_patient_elbo", ["fcd_vb_patient_elbo"], call=_call_patient_elbo)
def _b_patient_elbo(d):
    return _vb_io(d, ("lq_F", "lq_R", "lM", "hyper"), {"out4": ((d["U"], 4), np.float64)})


# ---------------------------------------------------------------------------------------------------------------------
# forward sampler and the counter RNG
# ---------------------------------------------------------------------------------------------------------------------
def _sample_io(d, shared):
    (th, _g, _p, _b, _bt) = model_data(d)
    (N, H, U, C_) = (d["N"], d["H"], d["U"], tri(d["N"]))
    outs = {"r": ((N,) if shared else (N, U), np.uint8), "t": ((C_, U), np.uint8), "f": ((C_,), np.uint8),
            "f_tilde": ((C_, U), np.uint8), "b": ((C_, H), np.float64), "b_tilde": ((C_, U), np.float64)}
    return dict(inputs={}, outputs=outs, host=dict(theta=th, N=N, H=H, U=U, seed=1234 + N))


def _call_sample(name):
    def go(ctx, i, o, h):
        ctx.call(name, _hp(h["theta"]), h["N"], h["H"], h["U"], C.c_uint64(h["seed"]), P(o["r"]), P(o["t"]), P(o["f"]),
                 P(o["f_tilde"]), P(o["b"]), P(o["b_tilde"]), ST())
    return go


case("model_sample", ["fcd_model_sample"], call=_call_sample("fcd_model_sample"))(lambda d: _sample_io(d, False))
case("model_sample_shared", ["fcd_model_sample_shared"], call=_call_sample("fcd_model_sample_shared"))(lambda d: _sample_io(d, True))


def _call_philox(ctx, i, o, h):
    ctx.call("fcd_philox_uniforms", P(i["ctr4"]), h["n"], C.c_uint64(h["seed"]), P(o["out"]), ST())


@case("philox_uniforms", ["fcd_philox_uniforms"], call=_call_philox)
def _b_philox(d):
    n = 3 * d["G"] + 1
    ctr = np.random.default_rng([12, n]).integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    return dict(inputs={"ctr4": ctr}, outputs={"out": ((2 * n,), np.float64)}, host=dict(n=n, seed=99))


# ---------------------------------------------------------------------------------------------------------------------
# front-end: correlations, cleaning, partial correlations
# ---------------------------------------------------------------------------------------------------------------------
def _call_corr_edges(ctx, i, o, h):
    ctx.call("fcd_corr_edges", P(i["ts"]), h["S"], h["N"], h["T"], h["fisher_z"], P(o["out"]), ST())


def _corr_io(S, N, T, seed, fisher_z=0):
    ts = PC.make_series(seed, S, N, T, mix=0.3 / np.sqrt(N)) + 5.0
    return dict(inputs={"ts": ts}, outputs={"out": ((tri(N), S), np.float64)}, host=dict(S=S, N=N, T=T, fisher_z=fisher_z))


@case("corr_edges_subject", ["fcd_corr_edges"], call=_call_corr_edges)
def _b_corr_subject(d):
    # large: T = 136 gives the subject kernel two time slices per subject (KS > 1): the tickets are drawn more than once
    return _corr_io(d["U"], d["N"], 136 if d["N"] == 33 else d["T"], 31)


@case("corr_edges_block", ["fcd_corr_edges"], call=_call_corr_edges)
def _b_corr_block(d):
    # the 64 x 64 block form with its moments pass: both sizes sit above the 208 regions of the subject kernel
    return _corr_io(2 if d["N"] == 17 else 3, 209 if d["N"] == 17 else 215, d["T"], 32, fisher_z=1)


@case("corr_edges_block_by_knob", ["fcd_corr_edges"], call=_call_corr_edges, knobs={"corr_form": 1})
def _b_corr_block_knob(d):
    # the block form at the subject kernel's shapes (17 / 33 regions: one partial 64 x 64 block)
    return _corr_io(d["U"], d["N"], d["T"], 34)


def _call_corr_clean(ctx, i, o, h):
    ctx.call("fcd_corr_clean", P(i["ts"]), P(i["confounds"]), P(i["frame_mask"]), h["S"], h["N"], h["Q"], h["T"], P(o["resid"]),
             P(o["info"]), ST())
    ctx.call("fcd_corr_edges", P(o["resid"]), h["S"], h["N"], h["T"], 0, P(o["out"]), ST())


def _clean_conditions(s):
    i = s["inputs"]
    CC.assert_conditions(CC.clean_ld(i["ts"], i["confounds"], i["frame_mask"] != 0))


@case("corr_clean", ["fcd_corr_clean", "fcd_corr_edges"], call=_call_corr_clean, conditions=_clean_conditions)
def _b_corr_clean(d):
    (S, N, T, Q) = (d["U"], d["N"], d["T"], d["Q"])
    (ts, cf, mask) = CC.make_input(600 + N, S, N, T, Q, drop=0.15, level=1.0)
    return dict(inputs={"ts": ts, "confounds": cf, "frame_mask": mask.astype(np.uint8)},
                outputs={"resid": ((S, N, T), np.float64), "info": ((S, 3), np.int32), "out": ((tri(N), S), np.float64)},
                host=dict(S=S, N=N, T=T, Q=Q))


def _call_corr_partial(ctx, i, o, h):
    ctx.call("fcd_corr_partial", P(i["ts"]), h["S"], h["N"], h["T"], P(i.get("n_frames")), h["mode"], h["value"], h["fisher_z"],
             P(o["out"]), P(o["alpha"]), P(o["info"]), ST())


def _partial_io(d, mode, value, T=None, frames=False):
    (S, N) = (d["U"], d["N"])
    T = d["T"] if T is None else T
    s = _corr_io(S, N, T, 33)
    s["inputs"]["ts"] = s["inputs"]["ts"] - 5.0
    if frames:
        # what fcd_corr_clean leaves: zero mean over the first n frames, exact zeros behind them
        n = np.array([T - 3 * (k % 3) for k in range(S)], dtype=np.int32)
        ts = s["inputs"]["ts"]
        for k in range(S):
            ts[k, :, n[k]:] = 0.0
            ts[k, :, :n[k]] -= ts[k, :, :n[k]].mean(axis=1, keepdims=True)
        s["inputs"]["n_frames"] = n
    s["outputs"].update({"alpha": ((S,), np.float64), "info": ((S, 2), np.int32)})
    s["host"].update(mode=mode, value=value)
    return s


@case("corr_partial_lw", ["fcd_corr_partial"], call=_call_corr_partial)
def _b_partial_lw(d):
    return _partial_io(d, 1, 0.0, T=136 if d["N"] == 33 else None)


@case("corr_partial_fixed", ["fcd_corr_partial"], call=_call_corr_partial)
def _b_partial_fixed(d):
    return _partial_io(d, 0, 0.25, frames=True)


@case("corr_partial_block_form", ["fcd_corr_partial"], call=_call_corr_partial)
def _b_partial_block(d):
    # above 208 regions the correlations come from the 64 x 64 block kernels (as corr_edges_block)
    return _partial_io(dict(d, U=2 if d["N"] == 17 else 3, N=209 if d["N"] == 17 else 215), 1, 0.0)


@case("corr_partial_chunked", ["fcd_corr_partial"], call=_call_corr_partial, knobs={"partial_chunk": 2})
def _b_partial_chunked(d):
    return _partial_io(d, 1, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# covariate adjustment (its reference needs H > Q + 1 observed controls: H = 8 / 16 here, Q = 2 / 9)
# ---------------------------------------------------------------------------------------------------------------------
def _cov_data(d):
    def go():
        (H, Q, C_) = (8 if d["N"] == 17 else 16, d["Q"], tri(d["N"]))
        rng = np.random.default_rng([40, d["N"]])
        z = CV.make_design(rng, H, Q)
        return (z, CV.make_rows(rng, C_, z, nan=0.05))
    return _memo(("cov", d["N"]), go)


def _call_cov_fit(ctx, i, o, h):
    ctx.call("fcd_edge_cov_fit", P(i["b"]), h["C"], h["H"], P(i["z"]), h["Q"], MISSING, P(o["beta"]), P(o["resid_var"]),
             P(o["info"]), ST())
    ctx.call("fcd_edge_cov_apply", P(i["b"]), h["C"], h["H"], P(i["z"]), h["Q"], P(i["z_ref"]), P(o["beta"]), P(o["adjusted"]),
             ST())


def _cov_conditions(s):
    CV.assert_conditions(CV.fit_ld(s["inputs"]["b"], s["inputs"]["z"], missing=True))


@case("edge_cov_fit_apply", ["fcd_edge_cov_fit", "fcd_edge_cov_apply"], call=_call_cov_fit, conditions=_cov_conditions)
def _b_cov_fit(d):
    (z, b) = _cov_data(d)
    (H, Q) = z.shape
    C_ = b.shape[0]
    return dict(inputs={"b": b, "z": z, "z_ref": np.ascontiguousarray(z.mean(axis=0))},
                outputs={"beta": ((C_, Q), np.float64), "resid_var": ((C_,), np.float64), "info": ((C_, 4), np.int32),
                         "adjusted": ((C_, H), np.float64)},
                host=dict(C=C_, H=H, Q=Q))


# ---------------------------------------------------------------------------------------------------------------------
# classical baselines
# ---------------------------------------------------------------------------------------------------------------------
def _base_data(d, f=None):
    return _memo(("base", d["N"], f), lambda: BR.make_data(d["N"], d["H"], d["U"], d["P"], 50 + d["N"], f=f))


def _base_host(d):
    return dict(C=tri(d["N"]), H=d["H"], U=d["U"], P=d["P"], N=d["N"])


def _call_normative(ctx, i, o, h):
    ctx.call("fcd_baseline_normative", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], 1.5, P(o["msq0"]), P(o["n_edges0"]),
             P(o["n_over0"]), P(o["msq"]), P(o["n_edges"]), P(o["n_over"]), P(o["n_controls"]), P(o["z0"]), P(o["z"]), ST())


@case("baseline_normative", ["fcd_baseline_normative"], call=_call_normative)
def _b_normative(d):
    # (leave-one-out scores need at least three OTHER controls to be defined: H + 2 controls)
    (N, H, U, C_) = (d["N"], d["H"] + 2, d["U"], tri(d["N"]))
    (b, bt, _lab) = BR.make_data(N, H, U, 1, 51 + N, f=0.05)
    outs = {"msq0": ((N, H), np.float64), "n_edges0": ((N, H), np.int32), "n_over0": ((N, H), np.int32),
            "msq": ((N, U), np.float64), "n_edges": ((N, U), np.int32), "n_over": ((N, U), np.int32),
            "n_controls": ((C_,), np.int32), "z0": ((C_, H), np.float64), "z": ((C_, U), np.float64)}
    return dict(inputs={"b": b, "bt": bt}, outputs=outs, host=dict(C=C_, H=H, U=U))


def _perm_outs(d, opt=False):
    (N, C_, P_) = (d["N"], tri(d["N"]), d["P"])
    outs = {"t": ((C_,), np.float64), "region": ((N,), np.float64), "null_max_t": ((P_,), np.float64),
            "null_max_region": ((P_,), np.float64), "count_t": ((C_,), np.int64), "count_region": ((N,), np.int64)}
    if opt:
        outs.update({"n_controls": ((C_,), np.int64), "n_patients": ((C_,), np.int64)})
    return outs


def _call_group_perm(ctx, i, o, h):
    ctx.call("fcd_baseline_group_perm", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["labels"]), h["P"], P(o["t"]),
             P(o["region"]), P(o["null_max_t"]), P(o["null_max_region"]), P(o["count_t"]), P(o["count_region"]), ST())


@case("baseline_group_perm", ["fcd_baseline_group_perm"], call=_call_group_perm)
def _b_group_perm(d):
    (b, bt, labels) = _base_data(d)
    return dict(inputs={"b": b, "bt": bt, "labels": labels}, outputs=_perm_outs(d), host=_base_host(d))


def _call_group_perm_opt(ctx, i, o, h):
    ctx.call("fcd_baseline_group_perm_opt", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["labels"]), h["P"], h["flags"],
             P(o["t"]), P(o["region"]), P(o["null_max_t"]), P(o["null_max_region"]), P(o["count_t"]), P(o["count_region"]),
             P(o["n_controls"]), P(o["n_patients"]), ST())


def _b_group_perm_opt(flags):
    def build(d):
        (b, bt, labels) = _base_data(d, f=0.1)
        return dict(inputs={"b": b, "bt": bt, "labels": labels}, outputs=_perm_outs(d, opt=True), host=dict(_base_host(d), flags=flags))
    return build


case("baseline_group_perm_missing", ["fcd_baseline_group_perm_opt"], call=_call_group_perm_opt)(_b_group_perm_opt(1))
case("baseline_group_perm_missing_welch", ["fcd_baseline_group_perm_opt"], call=_call_group_perm_opt)(_b_group_perm_opt(3))


def _bits_outs(d):
    return {"bits": ((d["P"], (tri(d["N"]) + 31) // 32), np.uint32), "t": ((tri(d["N"]),), np.float64)}


def _components_outs(d, B):
    return {"component": ((B, d["N"]), np.int32), "n_edges": ((B,), np.int32), "max_extent": ((B,), np.int32),
            "max_regions": ((B,), np.int32)}


def _call_components(ctx, o, h, B):
    ctx.call("fcd_graph_components", P(o["bits"]), B, h["C"], P(o["component"]), P(o["n_edges"]), P(o["max_extent"]),
             P(o["max_regions"]), ST())


def _call_network_bits(ctx, i, o, h):
    ctx.call("fcd_baseline_network_bits", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["labels"]), h["P"], 1.0, 0,
             P(o["bits"]), P(o["t"]), ST())
    _call_components(ctx, o, h, h["P"])


@case("baseline_network_bits", ["fcd_baseline_network_bits", "fcd_graph_components"], call=_call_network_bits)
def _b_network_bits(d):
    (b, bt, labels) = _base_data(d)
    return dict(inputs={"b": b, "bt": bt, "labels": labels}, outputs=dict(_bits_outs(d), **_components_outs(d, d["P"])),
                host=_base_host(d))


def _call_network_bits_opt(ctx, i, o, h):
    ctx.call("fcd_baseline_network_bits_opt", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["labels"]), h["P"], 1.0, 1, 3,
             P(o["bits"]), P(o["t"]), ST())


@case("baseline_network_bits_opt", ["fcd_baseline_network_bits_opt"], call=_call_network_bits_opt)
def _b_network_bits_opt(d):
    (b, bt, labels) = _base_data(d, f=0.1)
    return dict(inputs={"b": b, "bt": bt, "labels": labels}, outputs=_bits_outs(d), host=_base_host(d))


def _call_network_bits_observed(ctx, i, o, h):
    # labels == NULL with P = 1: the observed labelling, through the same kernel
    ctx.call("fcd_baseline_network_bits", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], None, 1, 1.0, 2, P(o["bits"]), P(o["t"]), ST())
    _call_components(ctx, o, h, 1)


@case("baseline_network_bits_observed", ["fcd_baseline_network_bits", "fcd_graph_components"], call=_call_network_bits_observed)
def _b_network_bits_observed(d):
    (b, bt, _labels) = _base_data(d)
    return dict(inputs={"b": b, "bt": bt}, outputs=dict(_bits_outs(dict(d, P=1)), **_components_outs(d, 1)), host=_base_host(d))


def _glm_data(d):
    def go():
        from fcdiff_amd import baseline
        Q = 1 if d["N"] == 17 else 3
        (b, bt, z_b, z_bt, perms) = BG.make_data(d["N"], d["H"] + 2, d["U"], Q, d["P"], d["N"])
        (W, info) = baseline.glm_design(z_b, z_bt)
        return (np.ascontiguousarray(b), np.ascontiguousarray(bt), np.ascontiguousarray(W, dtype=np.float64),
                np.ascontiguousarray(perms, dtype=np.uint16))
    return _memo(("glm", d["N"]), go)


def _glm_io(d, outs):
    (b, bt, W, perms) = _glm_data(d)
    assert perms.shape == (d["P"], b.shape[1] + bt.shape[1]) and W.shape[0] == perms.shape[1]
    return dict(inputs={"b": b, "bt": bt, "design": W, "perms": perms}, outputs=outs,
                host=dict(C=tri(d["N"]), H=b.shape[1], U=bt.shape[1], R=W.shape[1], P=d["P"]))


def _call_group_glm(ctx, i, o, h):
    ctx.call("fcd_baseline_group_glm", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["design"]), h["R"], P(i["perms"]), h["P"],
             P(o["t"]), P(o["region"]), P(o["null_max_t"]), P(o["null_max_region"]), P(o["count_t"]), P(o["count_region"]), ST())


case("baseline_group_glm", ["fcd_baseline_group_glm"], call=_call_group_glm)(lambda d: _glm_io(d, _perm_outs(d)))


def _call_network_bits_glm(ctx, i, o, h):
    ctx.call("fcd_baseline_network_bits_glm", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["design"]), h["R"], P(i["perms"]),
             h["P"], 1.0, 2, P(o["bits"]), P(o["t"]), ST())


case("baseline_network_bits_glm", ["fcd_baseline_network_bits_glm"], call=_call_network_bits_glm)(lambda d: _glm_io(d, _bits_outs(d)))


def _call_network_bits_glm_identity(ctx, i, o, h):
    # perms == NULL with P = 1: the identity
    ctx.call("fcd_baseline_network_bits_glm", P(i["b"]), P(i["bt"]), h["C"], h["H"], h["U"], P(i["design"]), h["R"], None, 1, 1.0, 0,
             P(o["bits"]), P(o["t"]), ST())


@case("baseline_network_bits_glm_identity", ["fcd_baseline_network_bits_glm"], call=_call_network_bits_glm_identity)
def _b_network_bits_glm_identity(d):
    s = _glm_io(d, _bits_outs(dict(d, P=1)))
    del s["inputs"]["perms"]
    return s


# ---------------------------------------------------------------------------------------------------------------------
# Gibbs sampler: single moves, counts and views of one state
# ---------------------------------------------------------------------------------------------------------------------
def _gibbs_host(d, U=None):
    return dict(N=d["N"], U=d["U"] if U is None else U, G=d["G"], chain0=3, seed=77 + d["N"], C=tri(d["N"]))


def _state_shapes(d, U=None):
    U = d["U"] if U is None else U
    GW = (d["G"] + 63) // 64
    return {"f_state": ((GW, tri(d["N"]), 64), np.uint8), "r_bits": ((GW, d["N"], U), np.uint64)}


def _call_init(ctx, i, o, h):
    ctx.call("fcd_gibbs_init", P(o["f_state"]), P(o["r_bits"]), h["N"], h["U"], h["G"], h["chain0"], C.c_uint64(h["seed"]), 0.3, ST())


case("gibbs_init", ["fcd_gibbs_init"], call=_call_init)(lambda d: dict(inputs={}, outputs=_state_shapes(d), host=_gibbs_host(d)))


def _state_io(d, outs, extra=None, inout=()):
    (f, r) = chain_state(d)
    ins = {"f_state": f, "r_bits": r}
    ins.update(extra or {})
    return dict(inputs=ins, outputs=outs, inout=inout, host=_gibbs_host(d))


def _call_tables(ctx, i, o, h):
    ctx.call("fcd_gibbs_edge_tables", P(i["lM"]), h["N"], h["U"], P(o["lMf"]), ST())
    ctx.call("fcd_gibbs_region_tables", P(i["lM"]), h["N"], h["U"], h["edge_mode"], P(o["lMd"]), ST())


def _table_outs(d, U=None):
    U = d["U"] if U is None else U
    return {"lMf": ((tri(d["N"]), U, 3, 2), np.float64), "lMd": ((U, d["N"], d["N"], 3, 2), np.float64)}


for (_name, _mode) in (("gibbs_tables_symmetric", 1), ("gibbs_tables_reference", 0)):
    case(_name, ["fcd_gibbs_edge_tables", "fcd_gibbs_region_tables"], call=_call_tables)(
        lambda d, _mode=_mode: dict(inputs={"lM": tables(d)[1]}, outputs=_table_outs(d), host=dict(_gibbs_host(d), edge_mode=_mode)))


def _move_io(d, blocked):
    (S_B, lM) = tables(d)
    outs = _table_outs(d) if blocked else {}
    return _state_io(d, outs, extra={"S_B": S_B, "lM": lM, "hyper": model_hyper(d)}, inout=("f_state", "r_bits"))


def _call_moves(ctx, i, o, h):
    if o:
        _call_tables(ctx, i, o, dict(h, edge_mode=SYM))
    ctx.call("fcd_gibbs_f_step", P(i["S_B"]), P(i["lM"]), P(o.get("lMf")), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]), h["N"],
             h["U"], h["G"], h["chain0"], C.c_uint64(h["seed"]), 2, ST())
    ctx.call("fcd_gibbs_r_step", P(i["lM"]), P(o.get("lMd")), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"],
             h["chain0"], C.c_uint64(h["seed"]), 2, SYM, ST())


_MOVE_EPS = ["fcd_gibbs_f_step", "fcd_gibbs_r_step", "fcd_gibbs_edge_tables", "fcd_gibbs_region_tables"]
case("gibbs_steps_generic", _MOVE_EPS[:2], call=_call_moves)(lambda d: _move_io(d, False))
case("gibbs_steps_blocked_pipelined", _MOVE_EPS, call=_call_moves)(lambda d: _move_io(d, True))
case("gibbs_steps_blocked_step_form", _MOVE_EPS, call=_call_moves, knobs={"r_path": 3})(lambda d: _move_io(d, True))
case("gibbs_steps_f_any_u", _MOVE_EPS, call=_call_moves, knobs={"f_form": 2})(lambda d: _move_io(d, True))
case("gibbs_steps_f_scalar_mask", _MOVE_EPS, call=_call_moves, knobs={"f_form": 3})(lambda d: _move_io(d, True))
case("gibbs_steps_blocked_cooperative", _MOVE_EPS, call=_call_moves, knobs={"r_coop": 1})(lambda d: _move_io(d, True))


def _call_tally(ctx, i, o, h):
    a = (P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"])
    ctx.call("fcd_gibbs_stats", *(a + (P(o["counts"]), ST())))
    ctx.call("fcd_gibbs_accumulate", *(a + (P(i["cnt_f"]), P(i["cnt_r"]), ST())))
    ctx.call("fcd_gibbs_tally", *(a + (P(o["counts2"]), P(i["cnt_f"]), P(i["cnt_r"]), ST())))
    ctx.call("fcd_gibbs_mstep", P(o["counts2"]), h["N"], h["U"], P(o["hyper"]), ST())


@case("gibbs_tally", ["fcd_gibbs_stats", "fcd_gibbs_accumulate", "fcd_gibbs_tally", "fcd_gibbs_mstep"], call=_call_tally)
def _b_tally(d):
    extra = {"cnt_f": np.zeros((tri(d["N"]), 3), dtype=np.uint32) + 7, "cnt_r": np.zeros((d["N"], d["U"]), dtype=np.uint32) + 9}
    return _state_io(d, {"counts": ((8,), np.int64), "counts2": ((8,), np.int64), "hyper": ((8,), np.float64)}, extra=extra,
                     inout=("cnt_f", "cnt_r"))


def _call_diagnostics(ctx, i, o, h):
    ctx.call("fcd_gibbs_logjoint", P(i["S_B"]), P(i["lM"]), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"],
             P(o["logjoint"]), ST())
    ctx.call("fcd_gibbs_chain_rsum", P(i["r_bits"]), h["N"], h["U"], h["G"], P(o["rsum"]), ST())
    ctx.call("fcd_gibbs_conditionals", P(i["S_B"]), P(i["lM"]), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"],
             h["G"], SYM, P(o["cond_f"]), P(o["cond_r"]), ST())


@case("gibbs_diagnostics", ["fcd_gibbs_logjoint", "fcd_gibbs_chain_rsum", "fcd_gibbs_conditionals"], call=_call_diagnostics)
def _b_diagnostics(d):
    (S_B, lM) = tables(d)
    (N, U, G) = (d["N"], d["U"], d["G"])
    outs = {"logjoint": ((G,), np.float64), "rsum": ((G,), np.uint32), "cond_f": ((G, tri(N), 3), np.float64),
            "cond_r": ((G, N, U, 2), np.float64)}
    return _state_io(d, outs, extra={"S_B": S_B, "lM": lM, "hyper": model_hyper(d)})


def _call_export_import(ctx, i, o, h):
    ctx.call("fcd_gibbs_export_state", P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"], P(o["f"]), P(o["r"]), ST())
    ctx.call("fcd_gibbs_import_state", P(o["f"]), P(o["r"]), h["N"], h["U"], h["G"], P(o["f_state2"]), P(o["r_bits2"]), ST())


@case("gibbs_export_import", ["fcd_gibbs_export_state", "fcd_gibbs_import_state"], call=_call_export_import)
def _b_export_import(d):
    sh = _state_shapes(d)
    outs = {"f": ((d["G"], tri(d["N"])), np.uint8), "r": ((d["G"], d["N"], d["U"]), np.uint8), "f_state2": sh["f_state"],
            "r_bits2": sh["r_bits"]}
    return _state_io(d, outs)


def _call_pair_counts(ctx, i, o, h):
    a = (P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"])
    ctx.call("fcd_gibbs_pair_counts", *(a + (0, P(o["W"]), ST())))
    ctx.call("fcd_gibbs_pair_counts", *(a + (1, P(o["W"]), ST())))
    ctx.call("fcd_gibbs_pair_tally", *(a + (P(i["acc"]), ST())))


@case("gibbs_pair_counts", ["fcd_gibbs_pair_counts", "fcd_gibbs_pair_tally"], call=_call_pair_counts)
def _b_pair_counts(d):
    shape = (tri(d["N"]), d["U"], 3, 3)
    return _state_io(d, {"W": (shape, np.float64)}, extra={"acc": np.zeros(shape, dtype=np.uint32) + 5}, inout=("acc",))


# ---- histograms over chains: their sets, groups and traits live in the context (setup) --------------------------------
def region_sets(N, J):
    """J overlapping sets of regions, CSR int32"""
    sets = [list(range(j, N, j + 2)) for j in range(J)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    return off, np.concatenate(sets).astype(np.int32), max(len(s) for s in sets)


def patient_groups(U):
    """three groups, the first two disjoint (one contrast), the third everyone"""
    groups = [list(range(0, U, 2)), list(range(1, U, 2)), list(range(U))]
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return off, np.concatenate(groups).astype(np.int32), np.array([[0, 1]], dtype=np.int32), [len(g) for g in groups]


def patient_traits(U):
    """two traits as doubled centred midranks: one known for everyone and without ties, one unknown for patient 0"""
    s0 = 2 * (np.arange(U) + 1) - (U + 1)
    n1 = U - 1
    s1 = np.concatenate([[0], 2 * (np.arange(n1)[::-1] + 1) - (n1 + 1)])
    known = np.ones((2, U), dtype=np.uint8)
    known[1, 0] = 0
    return np.ascontiguousarray(np.stack([s0, s1]).astype(np.int32)), known, U


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _set_side_tables(ctx, h):
    (off, mem, _smax) = region_sets(h["N"], h["J"])
    ctx.call("fcd_region_sets_set", _vp(off), _vp(mem), h["J"])
    (goff, gmem, con, _sizes) = patient_groups(h["U"])
    ctx.call("fcd_patient_groups_set", _vp(goff), _vp(gmem), 3, _vp(con), 1, 1)
    (scores, known, _umax) = patient_traits(h["U"])
    ctx.call("fcd_patient_traits_set", _vp(scores), _vp(known), 2, h["U"], 0)


def _clear_side_tables(ctx):
    ctx.call("fcd_patient_traits_set", None, None, 0, 0, 0)
    ctx.call("fcd_patient_groups_set", None, None, 0, None, 0, 0)
    ctx.call("fcd_region_sets_set", None, None, 0)


def _hist_shapes(d):
    """name -> (shape, dtype) of every histogram of the chain-count tallies at this shape"""
    (N, U, J) = (d["N"], d["U"], d["J"])
    (_off, _mem, smax) = region_sets(N, J)
    (_g, _m, _c, sizes) = patient_groups(U)
    R = N + J                                                      # the groups' rows: the regions, then the region sets
    joint = R * (sizes[0] + 1) * (sizes[1] + 1)
    umax_t = U                                                     # max_q n_q of patient_traits
    return {"hist_patient": ((U, N + 1), np.uint32), "hist_region": ((N, U + 1), np.uint32),
            "hist_set": ((J, U, smax + 1), np.uint32), "hist_prev": ((J, U + 1), np.uint32),
            "hist_group": ((3, R, max(sizes) + 1), np.uint32), "hist_joint": ((joint,), np.uint32),
            "trait_hist": ((2, N, umax_t + 1 + 128 + 3), np.uint32), "trait_sum": ((2, N, umax_t + 1), np.int64),
            "region_pairs": ((N, N), np.uint32), "patient_pairs": ((U, U), np.uint32)}


def _hist_inputs(d):
    return dict((k, np.zeros(shape, dtype=dt) + 1) for (k, (shape, dt)) in _hist_shapes(d).items())


def _call_chain_counts(ctx, i, o, h):
    a = (P(i["r_bits"]), h["N"], h["U"], h["G"])
    ctx.call("fcd_gibbs_count_tally", *(a + (P(i["hist_patient"]), P(i["hist_region"]), ST())))
    ctx.call("fcd_gibbs_region_set_tally", *(a + (P(i["hist_set"]), P(i["hist_prev"]), ST())))
    ctx.call("fcd_gibbs_patient_group_tally", *(a + (P(i["hist_group"]), P(i["hist_joint"]), ST())))
    ctx.call("fcd_gibbs_patient_trait_tally", *(a + (P(i["trait_hist"]), P(i["trait_sum"]), ST())))
    ctx.call("fcd_gibbs_coanomaly_tally", *(a + (P(i["region_pairs"]), P(i["patient_pairs"]), ST())))


_COUNT_EPS = ["fcd_gibbs_count_tally", "fcd_gibbs_region_set_tally", "fcd_gibbs_patient_group_tally",
              "fcd_gibbs_patient_trait_tally", "fcd_gibbs_coanomaly_tally"]


@case("gibbs_chain_counts", _COUNT_EPS, call=_call_chain_counts, setup=lambda ctx, i, o, h: _set_side_tables(ctx, h),
      teardown=_clear_side_tables)
def _b_chain_counts(d):
    hists = _hist_inputs(d)
    s = _state_io(d, {}, extra=hists, inout=tuple(sorted(hists)))
    del s["inputs"]["f_state"]
    s["host"]["J"] = d["J"]
    return s


# ---------------------------------------------------------------------------------------------------------------------
# Gibbs sampler: the sweep loops.  Four sweeps, an M-step every two, every accumulator attached; the difference tables are
# made by the same call sequence (fcd_gibbs_edge_tables / _region_tables), on the same stream.
# fcd_gibbs_run and fcd_gibbs_sweeps wait for the device where a call builds the f pass's records: fcd_hint_wait
# (fcd_gibbs.hip) polls the pinned hint word the record build leaves, and synchronises the stream after two seconds.  Every
# case below has such a build (knob f_records = 2, or four sweeps on the pair-tile pass), so syncs_stream is True.
# ---------------------------------------------------------------------------------------------------------------------
N_SWEEPS = 4
_ACCS = (("fcd_gibbs_set_pair_accumulator", ("acc",)), ("fcd_gibbs_set_count_accumulator", ("hist_patient", "hist_region")),
         ("fcd_gibbs_set_coanomaly_accumulator", ("region_pairs", "patient_pairs")),
         ("fcd_gibbs_set_region_set_accumulator", ("hist_set", "hist_prev")),
         ("fcd_gibbs_set_patient_group_accumulator", ("hist_group", "hist_joint")),
         ("fcd_gibbs_set_patient_trait_accumulator", ("trait_hist", "trait_sum")))


def _attach(ctx, i, o, h):
    _set_side_tables(ctx, h)
    for (name, bufs) in _ACCS:
        ctx.call(name, *([P(i[b]) for b in bufs] + [h["N"], h["U"], 1]))


def _detach(ctx):
    for (name, bufs) in reversed(_ACCS):
        ctx.call(name, *([None] * len(bufs) + [0, 0, 1]))
    _clear_side_tables(ctx)


def _run_tables(d, U_groups):
    """a grouped table of f_pass_table_cases at this Nreg: one pseudo-patient per group, U' = len(U_groups)"""
    return _memo(("run", d["N"], U_groups), lambda: FC.grouped(d["N"], 16, sum(U_groups), 5, sizes=U_groups))


def _run_groups(d):
    return (1, 2, 8) if d["U"] == 3 else (1, 2, 1, 2, 1, 2, 2)


def _run_io(d):
    (S_B, lM, N, U, _p) = _run_tables(d, _run_groups(d))
    assert (N, U) == (d["N"], d["U"])
    (f, r) = chain_state(d)
    ins = {"S_B": S_B, "lM": lM, "hyper": model_hyper(d), "f_state": f, "r_bits": r,
           "cnt_f": np.zeros((tri(N), 3), dtype=np.uint32), "cnt_r": np.zeros((N, U), dtype=np.uint32),
           "acc": np.zeros((tri(N), U, 3, 3), dtype=np.uint32)}
    ins.update(_hist_inputs(d))
    outs = dict(_table_outs(d), counts=((8,), np.int64))
    inout = tuple(k for k in sorted(ins) if k not in ("S_B", "lM"))
    return dict(inputs=ins, outputs=outs, inout=inout, host=dict(_gibbs_host(d), J=d["J"], edge_mode=SYM))


def _run_conditions(s):
    h = s["host"]
    p = FC.premise(h["N"], s["inputs"]["S_B"], s["inputs"]["lM"], h["U"])
    assert p["any"], "no decided tile: the decided-tile and run forms of the f pass would not be reached"


def _call_run(ctx, i, o, h):
    _call_tables(ctx, i, o, h)
    ctx.call("fcd_gibbs_run", P(i["S_B"]), P(i["lM"]), P(o["lMf"]), P(o["lMd"]), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]),
             h["N"], h["U"], h["G"], h["chain0"], C.c_uint64(h["seed"]), 0, N_SWEEPS, SYM, 2, 1, P(o["counts"]), P(i["cnt_f"]),
             P(i["cnt_r"]), ST())


_RUN_EPS = ["fcd_gibbs_run", "fcd_gibbs_edge_tables", "fcd_gibbs_region_tables"]
for (_name, _knobs) in (("gibbs_run_record_form", {"f_records": 2, "f_sure": 1}),
                        ("gibbs_run_decided_tile_form", {"f_records": 2, "f_runs": 1}),
                        ("gibbs_run_run_form", {"f_records": 2, "f_runs": 2}),
                        ("gibbs_run_step_per_launch", {"f_records": 2, "r_path": 3}),
                        ("gibbs_run_tile_records", {"f_records": 1})):
    # "tile_records": no record build, so no hint to wait for -- the one sweep loop that does not wait for its stream
    case(_name, _RUN_EPS, call=_call_run, knobs=_knobs, syncs_stream=_knobs["f_records"] == 2, setup=_attach, teardown=_detach,
         conditions=_run_conditions)(_run_io)


def _call_sweeps(ctx, i, o, h):
    _call_tables(ctx, i, o, h)
    ctx.call("fcd_gibbs_sweeps", P(i["S_B"]), P(i["lM"]), P(o["lMf"]), P(o["lMd"]), P(i["hyper"]), P(i["f_state"]), P(i["r_bits"]),
             h["N"], h["U"], h["G"], h["chain0"], C.c_uint64(h["seed"]), 1, N_SWEEPS, SYM, P(o["counts"]), ST())


@case("gibbs_sweeps", ["fcd_gibbs_sweeps", "fcd_gibbs_edge_tables", "fcd_gibbs_region_tables"], call=_call_sweeps,
      knobs={"f_records": 2}, syncs_stream=True, conditions=_run_conditions)
def _b_sweeps(d):
    s = _run_io(d)
    keep = ("S_B", "lM", "hyper", "f_state", "r_bits")
    s["inputs"] = dict((k, s["inputs"][k]) for k in keep)
    s["inout"] = ("f_state", "r_bits")
    return s


# ---------------------------------------------------------------------------------------------------------------------
# scoring, evidence, membership
# ---------------------------------------------------------------------------------------------------------------------
def _call_ais(ctx, i, o, h):
    ctx.call("fcd_score_ais_step", P(i["lM"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"], 0.25, 0.5, P(i["w"]),
             P(o["lM_beta"]), ST())
    ctx.call("fcd_score_ais_finish", P(i["w"]), h["U"], h["G"], P(o["out4"]), ST())


@case("score_ais", ["fcd_score_ais_step", "fcd_score_ais_finish"], call=_call_ais)
def _b_ais(d):
    (_S_B, lM) = tables(d)
    w = np.random.default_rng([14, d["N"]]).normal(0.0, 1.0, (d["G"], d["U"]))
    return _state_io(d, {"lM_beta": (lM.shape, np.float64), "out4": ((d["U"], 4), np.float64)}, extra={"lM": lM, "w": w},
                     inout=("w",))


def _call_evidence(ctx, i, o, h):
    ctx.call("fcd_evidence_energy", P(i["S_B"]), P(i["lM"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"], 0.25, 0.5,
             P(i["w"]), ST())
    n = 2
    src = (C.c_void_p * n)(i["S_B"].data_ptr(), i["lM"].data_ptr())
    dst = (C.c_void_p * n)(o["S_B_beta"].data_ptr(), o["lM_beta"].data_ptr())
    cnt = (C.c_int64 * n)(i["S_B"].numel(), i["lM"].numel())
    ctx.call("fcd_evidence_temper", 0.5, n, src, dst, cnt, ST())


@case("evidence", ["fcd_evidence_energy", "fcd_evidence_temper"], call=_call_evidence)
def _b_evidence(d):
    (S_B, lM) = tables(d)
    w = np.random.default_rng([15, d["N"]]).normal(0.0, 1.0, (d["G"],))
    return _state_io(d, {"S_B_beta": (S_B.shape, np.float64), "lM_beta": (lM.shape, np.float64)},
                     extra={"S_B": S_B, "lM": lM, "w": w}, inout=("w",))


def _call_member(ctx, i, o, h):
    ctx.call("fcd_member_loglik", P(i["x"]), _hp(h["theta"]), P(i["f_state"]), P(i["r_bits"]), h["N"], h["U"], h["G"], h["r_cols"],
             MISSING, P(o["out_control"]), P(o["out_patient"]), ST())


def _member_io(d, r_cols):
    (th, _g, _p, _b, bt) = model_data(d)
    (f, r) = chain_state(d, U=r_cols)
    outs = {"out_control": ((d["G"], d["U"]), np.float64), "out_patient": ((d["G"], d["U"]), np.float64)}
    return dict(inputs={"x": nan_some(bt, 26), "f_state": f, "r_bits": r}, outputs=outs,
                host=dict(_gibbs_host(d), theta=th, r_cols=r_cols))


case("member_loglik", ["fcd_member_loglik"], call=_call_member)(lambda d: _member_io(d, d["U"]))
case("member_loglik_shared_r", ["fcd_member_loglik"], call=_call_member)(lambda d: _member_io(d, 1))


ONE_SHAPE = ("hyper_set",)                 # cases whose entry point has no extent: "large" differs in its values
BY_NAME = dict((c.name, c) for c in CASES)
assert len(BY_NAME) == len(CASES)

# Prototypes with an fcd_stream that no case calls, each with its reason (tests/test_caller_stream_cases.py).
EXEMPT = {
    "fcd_allreduce_stats": "needs an RCCL communicator on the context; tests/test_dist_gloo.py and the multi-rank runs cover it",
}


# ---------------------------------------------------------------------------------------------------------------------
# running a case (GPU; torch is imported here, never at import of this module)
# ---------------------------------------------------------------------------------------------------------------------
# what a call adds to the context's counters: the forms it took are part of what it computes (a form chosen from a word the
# call before left behind changes no bit, by design)
HOST_STATS = ("f_rec_passes", "f_rec_builds", "f_sure_passes", "f_run_passes", "pack_launches", "tally_f_in_pack", "tally_f_in_r")
DEVICE_STATS = ("f_repeats", "r_exact_rows", "f_sure_tiles", "f_sure_fallbacks")          # (reading them synchronises)


def as_bytes(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


def fill_outputs(dout):
    for t in dout.values():
        as_bytes(t).fill_(SENTINEL)


def poison_inputs(case, din):
    """NaN in every floating-point input, 0xFF bytes in every other"""
    for t in case.tensors(din).values():
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            as_bytes(t).fill_(0xFF)


def pinned_inputs(case, size):
    import torch
    return dict((k, torch.from_numpy(v).pin_memory()) for (k, v) in case.make(size).items())


STRUCTURAL = ("offsets", "order", "perms", "n_frames", "labels")      # inputs a kernel indexes with: never scrambled


def scrambled_inputs(case, size):
    """
    The inputs with the values of every array in reverse order (pinned): other data of the same shape, type and range, so
    that a run on them leaves the context's scratch holding what the true inputs do NOT give.  Index arrays stay.
    """
    import torch
    return dict((k, torch.from_numpy(v if k in STRUCTURAL else np.ascontiguousarray(v.reshape(-1)[::-1]).reshape(v.shape)).pin_memory())
                for (k, v) in case.make(size).items())


def feed(case, din, host, non_blocking=False):
    for (k, t) in case.tensors(din).items():
        t.copy_(host[k], non_blocking=non_blocking)


def snapshot(case, din, dout):
    """name -> bytes (a CPU tensor) of everything the call leaves; synchronises"""
    return dict((k, as_bytes(t).cpu()) for (k, t) in case.compared(din, dout))


def differing(got, want):
    """the names whose bytes differ"""
    import torch
    assert sorted(got) == sorted(want)
    return [k for k in sorted(got) if not torch.equal(got[k], want[k])]


def read_stats(ctx, names):
    return dict((k, ctx.stat(k)) for k in names)


def run_once(ctx, case, size, device, stats=False):
    """the case on ctx and on the current stream, from freshly fed buffers -> (bits, rise of the counters or None); synchronises"""
    import torch
    (din, dout) = case.alloc(size, device)
    case.setup(ctx, din, dout)
    try:
        fill_outputs(dout)
        feed(case, din, pinned_inputs(case, size))
        torch.cuda.synchronize()
        names = HOST_STATS + DEVICE_STATS
        before = read_stats(ctx, names) if stats else None
        case.run(ctx, din, dout)
        torch.cuda.synchronize()
        bits = snapshot(case, din, dout)
        rise = None
        if stats:
            after = read_stats(ctx, names)
            rise = dict((k, after[k] - before[k]) for k in names)
            loops = set(("fcd_gibbs_run", "fcd_gibbs_sweeps")) & set(case.entry_points)       # (the calls that always set it)
            rise["r_form_last"] = ctx.stat("r_form_last") if loops else 0
    finally:
        case.teardown(ctx)
    return bits, rise


_fresh = {}


def fresh(case, size, device):
    """(bits, counters) of the case on a context made for that one call, on the default stream; computed once and shared"""
    key = (case.name, size)
    if key not in _fresh:
        ctx = _lib().Context()
        try:
            _fresh[key] = run_once(ctx, case, size, device, stats=True)
        finally:
            ctx.close()
        # a case that leaves a buffer as it found it would prove nothing: every output is written somewhere, every input
        # that the call updates in place is changed somewhere
        fed = case.make(size)
        for (k, got) in _fresh[key][0].items():
            (kind, name) = k.split(".", 1)
            before = np.full(got.numel(), SENTINEL, dtype=np.uint8) if kind == "out" else fed[name].reshape(-1).view(np.uint8)
            assert not np.array_equal(got.numpy(), before), "%s/%s: %s is untouched by the call" % (case.name, size, k)
    return _fresh[key]
