"""
One long-lived context serves every case of tests/caller_stream_cases.py, at both sizes, in three orders; after every
call its outputs must be what a context made for that one call gives, bit for bit, and so must the forms it took (the
counters of fcd_ctx_stat: a form chosen from what the call before left behind changes no bit, by design, so the bits alone
would not show it).

What a context carries from call to call: one workspace that every family carves up differently, words that are "zero
between launches" because the last kernel puts them back (the pooled counts, the NaN slots, the correlation tickets, the
hint counters of the record build), the pinned hint word, cached launch attributes and occupancy answers, and tables that
are valid inside one call.  The rest of the suite feeds one context the same few shapes of one family.

Orders: the registry's with the sizes alternating small, large; its reverse with the alternation flipped, so that every
case sees large -> small as well as small -> large and follows the family behind it as well as the one before it; and a
shuffle with a fixed seed in which every call follows a refused call of its own family.
"""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = [(c.name, size) for c in R.CASES for size in R.SIZES]


def orders():
    n = len(R.CASES)
    forward = [(c.name, size) for c in R.CASES for size in R.SIZES]                       # small, large, small, large, ...
    backward = [(c.name, size) for c in reversed(R.CASES) for size in reversed(R.SIZES)]  # ... and large, small from the end
    shuffled = list(KEYS)
    random.Random(20240607).shuffle(shuffled)
    assert sorted(forward) == sorted(backward) == sorted(shuffled) == sorted(KEYS) and len(forward) == 2 * n
    return dict(forward=forward, backward=backward, shuffled=shuffled)


def test_the_orders_cover_every_pair_both_ways():
    o = orders()
    seen = set()
    for seq in (o["forward"], o["backward"]):
        last = {}
        for (name, size) in seq:
            if name in last:
                seen.add((name, last[name], size))
            last[name] = size
    for c in R.CASES:
        assert (c.name, "small", "large") in seen and (c.name, "large", "small") in seen, c.name


@pytest.fixture(scope="module")
def gpu():
    import torch
    from fcdiff_amd import _lib
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return dict(torch=torch, lib=_lib, device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def shared_ctx(gpu):
    ctx = gpu["lib"].Context()
    yield ctx
    ctx.close()


def check_call(gpu, ctx, name, size, where):
    case = R.BY_NAME[name]
    (want, want_stats) = R.fresh(case, size, gpu["device"])
    (got, stats) = R.run_once(ctx, case, size, gpu["device"], stats=True)
    bad = R.differing(got, want)
    assert not bad, "%s: %s/%s differs from a fresh context in %s" % (where, name, size, bad)
    assert stats == want_stats, "%s: %s/%s took other forms than on a fresh context: %s, fresh %s" % (where, name, size, stats, want_stats)
    assert ctx.stat("dev_err") == 0, (where, name, size)


ORDERS = orders()
STEPS = [(order, i) for order in ("forward", "backward", "shuffled") for i in range(len(KEYS))]


@pytest.mark.parametrize("order,i", STEPS, ids=lambda v: str(v))
def test_every_call_after_any_other(gpu, shared_ctx, order, i):
    """step i of an order, on the ONE context that has served every step before it (and the orders before this one)"""
    ctx = shared_ctx
    (name, size) = ORDERS[order][i]
    where = "%s[%d]" % (order, i)
    if order == "shuffled":
        n_alloc = ctx.stat("n_alloc")
        rc = R.BY_NAME[name].refuse(ctx)
        assert rc < 0, "%s: %s took a call with null pointers and zero sizes (returned %d)" % (where, name, rc)
        assert ctx.stat("n_alloc") == n_alloc, (where, name)
    check_call(gpu, ctx, name, size, where)


def test_a_context_closed_and_made_again(gpu, shared_ctx):
    """at the end of the three orders the context is sound, and a new one gives the fresh bits again"""
    shared_ctx.check_device()
    assert shared_ctx.stat("dev_err") == 0
    shared_ctx.close()
    ctx = gpu["lib"].Context()
    try:
        for (name, size) in (("gibbs_sweeps", "small"), ("corr_edges_subject", "large"), ("lik_tables_ex", "small")):
            check_call(gpu, ctx, name, size, "new context")
        ctx.check_device()
    finally:
        ctx.close()
