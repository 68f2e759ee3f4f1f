"""What the op-level entry points keep from call to call belongs to the context, and a context gives back what it allocated.

The trunk ops' inbox and launch counter and the kept weight-gradient batch with its key are members of dbm_ctx (dbm_ctx::op), made on
first use and released by ~dbm_ctx with every other allocation of the context (sync_buf included).  Both tests run the same two cases
through the builders of the op-level suites, on the default context or on one of their own:

  trunk forward: nrdb = 3, N = 1, 27-position tiles, keep, 8 images per launch (run_forward of test_gpu_trunk_ops.py, which asserts the
                 launch report -- form and workgroups -- of every call against the same expectation, whatever the context);
  wgrad batch:   one descriptor, C = O = 32 on 8 x 8, 3 x 3 / stride 1 / pad 1, N = 2 (WgradRun of test_gpu_conv_launches.py).

Every op call synchronises before it returns: nothing here runs concurrently.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_conv_launches as cl  # noqa: E402
import test_gpu_trunk_ops as tk  # noqa: E402

pytestmark = pytest.mark.gpu

RS = 0.3
RID = "ctx-state"
cl.EXTRA_WGRAD_ROWS[RID] = [cl.wd((2, 32, 8, 8, 32, 3, 1, 1, 0))]

# What one context's op-level state takes from the device: the trunk inbox (trunk_fused_inbox_bytes(64)) plus the kept batch's plan
# tables, measured as the drop of free device memory around the first trunk op (23068672 bytes, what a process's first persistent launch
# loads included) plus the first wgrad batch op (2097152 bytes) of a fresh process on the library before the state moved into the
# context (profiles/r8/api_ops_refactor.txt).  The test allows ONE such unit, since the allocator's granularity can hide one.  (That
# library kept the state process-wide, made once and never freed, so its rounds lost nothing either: measured 0 bytes.  What this test
# pins is that state made per context goes back with the context; this tree measured 0 bytes lost over the five rounds as well.)
OP_STATE_BYTES = 25165824


@pytest.fixture(scope="module")
def dbm():
    import deepbedmap_amd as d
    from deepbedmap_amd import _lib

    return d, _lib, _lib.default_context()


def shutdown(_lib, ctx):
    handle, ctx.handle = ctx.handle, None
    _lib.check(_lib.lib().dbm_shutdown(handle))


def trunk(dbm, ctx=None, epoch0=-1):
    cat, _ = tk.run_forward(dbm, tk.problem(3, 1), RS, "tp27", True, ipl=8, epoch0=epoch0, ctx=ctx)
    return cat


def wgrad(run, ctx, cleared=0):
    run.ctx = ctx
    _, raw, cat, S = run.call(cleared)
    return raw, cat, S


def same_trunk(a, b):
    return len(a) == len(b) and all(tk.same_bits(x, y) for x, y in zip(a, b))


def same_wgrad(a, b):
    return a[1:] == b[1:] and len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


def test_op_state_belongs_to_the_context(dbm):
    d, _lib, ctx0 = dbm
    run = cl.WgradRun(dbm, RID)
    second = third = None
    try:
        _lib.check(_lib.lib().dbm_set_deterministic(ctx0.handle, 1), ctx0.handle)
        t0, w0 = trunk(dbm), wgrad(run, ctx0)
        second = _lib.Context()
        assert same_trunk(trunk(dbm, second), t0), "the trunk op on a second context gave other bits"
        assert same_wgrad(wgrad(run, second), w0), "the wgrad batch op on a second context gave other bits"
        _, cat, S = wgrad(run, second, cleared=1)      # the kept batch's re-plan (WgradBatch::launch), on the second context's batch
        assert (cat, S) == w0[1:]
        shutdown(_lib, second)
        second = None
        assert same_trunk(trunk(dbm), t0), "the default context's trunk state changed with another context's life"
        assert same_wgrad(wgrad(run, ctx0), w0), "the default context's kept batch changed with another context's life"
        third = _lib.Context()                         # a zeroed inbox and the initial counter: the first call of a context, again
        assert same_trunk(trunk(dbm, third, epoch0=-1), t0)
    finally:
        for c in (second, third):
            if c is not None:
                shutdown(_lib, c)
        cl.restore_deterministic(ctx0)


def test_a_context_gives_back_what_it_took(dbm):
    import torch

    d, _lib, ctx0 = dbm
    run = cl.WgradRun(dbm, RID)                        # (operands on the device once: the rounds allocate through their context only)
    tk.problem(3, 1)

    def one_round():
        ctx = _lib.Context()
        try:
            _lib.check(_lib.lib().dbm_set_sync_batch_stats(ctx.handle, 1, None, None), ctx.handle)   # (world = 1, no hook: accepted)
            wgrad(run, ctx)
            trunk(dbm, ctx)
        finally:
            shutdown(_lib, ctx)
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    shutdown(_lib, _lib.Context())                     # warm-up pair
    free = [one_round() for _ in range(5)]
    run.ctx = ctx0
    print(f"free device memory after each round: {free}; lost between the first and the fifth: {free[0] - free[4]} bytes "
          f"(allowed: {OP_STATE_BYTES})")
    assert free[0] - free[4] <= OP_STATE_BYTES, (free, OP_STATE_BYTES)
