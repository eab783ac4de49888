"""
Every device entry point on a caller's stream (tests/caller_stream_cases.py has one case per entry point).

The rest of the suite runs on torch's default stream, where every launch, memset and copy is ordered whatever stream the
library puts it on.  A PyTorch user calls inside `with torch.cuda.stream(s):`, and there a launch that falls onto the null
stream, or a helper that is not handed the stream, is a data race: torch's side streams do not wait for the null stream.

Per case, on a context of its own:
  1  the case at "small" on the default stream on a context made for that call: the reference bits (what they should BE is
     pinned by the family's own suite; every kernel's header promises that two calls agree bit for bit);
  2  once more inside `with torch.cuda.stream(side)`: grows the workspace, sets the LDS attributes, allocates the tickets;
     then once on the same inputs in reverse order, so that the scratch the context keeps holds other numbers;
  3  the delayed producer: every input poisoned, then on `side` a chain of matrix products (the delay), the copies of the
     true inputs from pinned memory, an event `fed`, the call.  The host must be through the whole call while the inputs are
     still poison (`fed` not reached -- unless the entry point waits for its stream by design), the outputs must be the
     reference bits, and the context must not have grown (a growth drains the device and would hide a fault).
The delay is sized per case: ten times the host-side duration of the warm call, at least 20 ms.  The side stream is one
that is SEEN to run beside the null stream (runs_beside): the runtime maps streams onto a few hardware queues, and on a
side stream that shares its queue with the null stream a stray launch is ordered by accident.

Then three pairs of cases on two contexts and two streams, enqueued alternately without any synchronisation: process-wide
device state would show as a difference from the solo bits.
"""
import math
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

DELAY_FACTOR = 10.0            # the delay against the host-side duration of the call
DELAY_FLOOR_MS = 20.0          # ... and its floor, for launch jitter
MM = 4096                      # side of the delay's matrix products


class Delay(object):
    """a chain of (MM x MM) matrix products on the current stream; no allocation after the first use"""

    def __init__(self, torch, device):
        self.torch = torch
        # b = 1 / MM everywhere: a product is the row means of a, so the values stay where they are however long the chain
        (self.a, self.c) = (torch.randn((MM, MM), device=device), torch.empty((MM, MM), device=device))
        self.b = torch.full((MM, MM), 1.0 / MM, device=device)
        self.enqueue(4)
        torch.cuda.synchronize()
        (e0, e1) = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e0.record()
        self.enqueue(16)
        e1.record()
        e1.synchronize()
        self.ms_per_product = e0.elapsed_time(e1) / 16.0

    def enqueue(self, n):
        for _ in range(n):
            self.torch.mm(self.a, self.b, out=self.c)
            (self.a, self.c) = (self.c, self.a)

    def products_for(self, ms):
        return int(math.ceil(ms / self.ms_per_product))


def runs_beside(torch, delay, busy, other):
    """
    True if work queued on `other` finishes while `busy` is still held up by a delay.  The runtime maps its streams onto a
    few hardware queues, and two streams that share one run in the order of submission: work that strays from `busy` to
    `other` is then ordered by accident, and a test on that pair of streams would prove nothing.
    """
    torch.cuda.synchronize()
    (end_busy, end_other) = (torch.cuda.Event(), torch.cuda.Event())
    tiny = torch.zeros(64, device=delay.a.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        delay.enqueue(delay.products_for(DELAY_FLOOR_MS))
        end_busy.record()
    with torch.cuda.stream(other):
        tiny.add_(1.0)
        end_other.record()
    while not end_other.query() and not end_busy.query():      # (at most the delay)
        pass
    beside = end_other.query() and not end_busy.query()
    torch.cuda.synchronize()
    return beside


def independent_streams(torch, delay, n):
    """n side streams that run beside the null stream and beside one another (found by trying, out of at most 16)"""
    found = []
    null = torch.cuda.default_stream()
    for _ in range(16):
        s = torch.cuda.Stream()
        if all(runs_beside(torch, delay, s, o) and runs_beside(torch, delay, o, s) for o in [null] + found):
            found.append(s)
            if len(found) == n:
                return found
    raise AssertionError("no %d streams that run beside the null stream and one another among 16: every stray launch would be "
                         "ordered by a shared hardware queue, and these tests would prove nothing" % n)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from fcdiff_amd import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    delay = Delay(torch, dev)
    print("\ncaller-stream delay: one %d x %d product takes %.3f ms" % (MM, MM, delay.ms_per_product))
    return dict(torch=torch, lib=_lib, device=dev, delay=delay, streams=independent_streams(torch, delay, 2))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_on_a_side_stream_behind_a_delayed_producer(gpu, case):
    (t, dev, delay) = (gpu["torch"], gpu["device"], gpu["delay"])
    (want, _stats) = R.fresh(case, "small", dev)                                     # 1
    ctx = gpu["lib"].Context()
    side = gpu["streams"][0]
    (din, dout) = case.alloc("small", dev)
    host = R.pinned_inputs(case, "small")
    case.setup(ctx, din, dout)
    try:
        R.fill_outputs(dout)                                                         # 2
        R.feed(case, din, host)
        t.cuda.synchronize()
        with t.cuda.stream(side):
            t0 = time.perf_counter()
            case.run(ctx, din, dout)
            host_ms = (time.perf_counter() - t0) * 1e3
        t.cuda.synchronize()
        warm = R.differing(R.snapshot(case, din, dout), want)
        assert not warm, "%s on a side stream differs from the default stream in %s" % (case.name, warm)
        # ... and once on other data, so that what the call leaves in the context's scratch is not by chance what the delayed
        # call would have put there (a kernel that runs too early then reads something WRONG)
        R.feed(case, din, R.scrambled_inputs(case, "small"))
        with t.cuda.stream(side):
            case.run(ctx, din, dout)
        t.cuda.synchronize()
        n_alloc = ctx.stat("n_alloc")

        R.poison_inputs(case, din)                                                   # 3
        R.fill_outputs(dout)
        t.cuda.synchronize()
        n_products = delay.products_for(max(DELAY_FACTOR * host_ms, DELAY_FLOOR_MS))
        fed = t.cuda.Event()
        with t.cuda.stream(side):
            delay.enqueue(n_products)
            R.feed(case, din, host, non_blocking=True)
            fed.record()
            case.run(ctx, din, dout)
            reached = fed.query()
        print("\ncaller-stream %s: host %.3f ms, delay %.1f ms (%d products)%s"
              % (case.name, host_ms, n_products * delay.ms_per_product, n_products, ", waits for its stream" if case.syncs_stream else ""))
        if not case.syncs_stream:
            assert not reached, ("%s: the inputs had arrived before the call returned -- the delay of %d products was too short "
                                 "to prove anything (host %.3f ms)" % (case.name, n_products, host_ms))
        else:
            assert reached, "%s is declared to wait for its stream, but it returned before its inputs had arrived" % case.name
        side.synchronize()
        t.cuda.synchronize()
        bad = R.differing(R.snapshot(case, din, dout), want)
        assert not bad, "%s read its inputs, or wrote its outputs, out of the caller's stream order: %s differ" % (case.name, bad)
        assert ctx.stat("n_alloc") == n_alloc, "%s: the context grew in the delayed call" % case.name
        assert ctx.stat("dev_err") == 0
        ctx.check_device()
    finally:
        case.teardown(ctx)
        ctx.close()


PAIRS = ((("corr_partial_lw", "small"), ("corr_edges_subject", "large")),
         (("gibbs_run_run_form", "small"), ("gibbs_run_record_form", "large")),
         (("baseline_group_perm", "small"), ("lik_tables_noise", "large")))
ROUNDS = 6


class Lane(object):
    """one case on a context and a stream of its own; every round restores the inputs and keeps the outputs, on the stream"""

    def __init__(self, gpu, name, size, stream):
        t = gpu["torch"]
        (self.case, self.size, self.t) = (R.BY_NAME[name], size, t)
        (self.want, _stats) = R.fresh(self.case, size, gpu["device"])
        self.ctx = gpu["lib"].Context()
        self.stream = stream
        (self.din, self.dout) = self.case.alloc(size, gpu["device"])
        self.case.setup(self.ctx, self.din, self.dout)
        self.pristine = dict((k, v.to(gpu["device"])) for (k, v) in R.pinned_inputs(self.case, size).items())
        self.kept = [dict((k, t.empty_like(R.as_bytes(v))) for (k, v) in self.case.compared(self.din, self.dout)) for _ in range(ROUNDS + 1)]
        self.round(0)                       # warm: the context grows here, not between the rounds
        t.cuda.synchronize()

    def round(self, i):
        with self.t.cuda.stream(self.stream):
            R.fill_outputs(self.dout)
            R.feed(self.case, self.din, self.pristine, non_blocking=True)
            self.case.run(self.ctx, self.din, self.dout)
            for (k, v) in self.case.compared(self.din, self.dout):
                self.kept[i][k].copy_(R.as_bytes(v), non_blocking=True)

    def close(self):
        self.case.teardown(self.ctx)
        self.ctx.close()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s+%s" % (p[0][0], p[1][0]))
def test_two_contexts_side_by_side(gpu, pair):
    t = gpu["torch"]
    lanes = [Lane(gpu, name, size, stream) for ((name, size), stream) in zip(pair, gpu["streams"])]
    try:
        grown = [lane.ctx.stat("n_alloc") for lane in lanes]
        for i in range(1, ROUNDS + 1):
            for lane in lanes:
                lane.round(i)
        t.cuda.synchronize()
        for (lane, n_alloc) in zip(lanes, grown):
            for i in range(ROUNDS + 1):
                bad = R.differing(dict((k, v.cpu()) for (k, v) in lane.kept[i].items()), lane.want)
                assert not bad, "%s beside %s, round %d: %s differ from the solo run" % (lane.case.name, pair, i, bad)
            assert lane.ctx.stat("n_alloc") == n_alloc and lane.ctx.stat("dev_err") == 0
            lane.ctx.check_device()
    finally:
        for lane in lanes:
            lane.close()
