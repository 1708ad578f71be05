"""Staging for the stream-order tests (tests/test_gpu_stream_order.py).

A context runs on a non-blocking stream of its own.  A device-form entry point
is correct only if it orders that stream after the work the caller has queued
on the legacy default stream -- where torch runs -- before it touches the
caller's device memory.  On an idle device nothing can tell whether it does, so
every case is staged the same way:

  1. the input buffer holds a stale but valid input A, the device is idle;
  2. `queued_work` keeps the default stream busy for many times the call's own
     duration (fill_ over 256 MiB, again and again, between two timing events);
  3. behind it, still without any synchronisation, the fresh input B is copied
     into the input buffer, every caller output buffer is filled with CANARY,
     and a snapshot of it is taken -- all on the default stream;
  4. the entry point is called at once, with B's arguments.

A call that does not wait reads A (a well-defined wrong answer), and what it
writes is overwritten by the fill that lands afterwards.  The staging itself is
held to two conditions, which are failures and not skips: the queued work is
still running immediately before the call, and it lasted at least FACTOR times
the wall time of the same call on an idle, warm device (the call's whole
duration bounds the time until it first touches its input).  `control` runs the
same staging with a raw copy on a fresh stream in place of the library: without
`wait_stream` it must see A, with it B; if the unordered copy sees B the staging
cannot tell a missing wait and the tests mean nothing.

Every tensor the staged part uses is allocated before it: an allocation inside
could synchronise the device and hide what the test is looking for.  That is
why the snapshot and the control's copies are `copy_` into tensors made
beforehand, not `clone()`.
"""
import math
import time

CANARY = 0xEE
FILL_BYTES = 256 << 20
FACTOR = 4        # the queued work lasts at least this many idle calls (asserted)
ASK = 2 * FACTOR  # and this many are asked for, so that jitter does not fail the staging
MIN_MS = 20.0     # never less queued work than this
MAX_FILLS = 100000

_calibration = {}  # {"buf": the filler's tensor, "ms": milliseconds per fill_}: once per process
REPORT = []        # (name, queued ms, idle call ms, staged call ms) of every staged call


def require_default_stream(torch):
    """torch's current stream must be the legacy default stream: the one the entry points order after."""
    assert torch.cuda.current_stream().cuda_stream == 0, \
        "torch's current stream is not the legacy default stream: the stream-order tests would test nothing"


class QueuedWork:
    def __init__(self, start, end, fills):
        self._start, self._end, self.fills = start, end, fills

    def still_running(self):
        return not self._end.query()

    def duration_ms(self):
        """Valid after a synchronize."""
        return self._start.elapsed_time(self._end)


def _calibrate(torch):
    if not _calibration:
        buf = torch.empty(FILL_BYTES, dtype=torch.uint8, device="cuda")
        buf.fill_(1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rounds = 64
        e0.record()
        for k in range(rounds):
            buf.fill_(k & 0xFF)
        e1.record()
        torch.cuda.synchronize()
        _calibration.update(buf=buf, ms=e0.elapsed_time(e1) / rounds)
        assert _calibration["ms"] > 0
        print(f"stream-order filler: {_calibration['ms'] * 1e3:.1f} us per fill_ of {FILL_BYTES >> 20} MiB", flush=True)
    return _calibration["buf"], _calibration["ms"]


def queued_work(torch, at_least_ms):
    """Queue fill_ calls on the default stream that last at_least_ms (by the
    calibration, with half as much again on top); returns at once."""
    require_default_stream(torch)
    buf, per_fill = _calibrate(torch)
    fills = max(8, math.ceil(1.5 * at_least_ms / per_fill))
    assert fills <= MAX_FILLS, f"{at_least_ms:.1f} ms of queued work would take {fills} fills"
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(fills):
        buf.fill_(k & 0xFF)
    end.record()
    return QueuedWork(start, end, fills)


def staged_call(torch, name, call, inputs=(), outputs=()):
    """inputs: [(d_in, d_stale, d_fresh)], device uint8 tensors of one size each;
    outputs: the caller device buffers the call writes; call(): the entry
    point with the fresh input's arguments, complete on return.

    Returns (the staged call's result, the idle call's result).  The outputs
    hold what the staged call left; the caller compares them, canaries
    included, with its reference."""
    require_default_stream(torch)
    # the same call on an idle, warm device, the fresh input already in place
    for d_in, _, d_fresh in inputs:
        d_in.copy_(d_fresh)
    for d_out in outputs:
        d_out.fill_(CANARY)
    torch.cuda.synchronize()
    call()  # the scratch buffers of this shape are made here
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idle_result = call()
    idle_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    # the stale input, outputs that are neither canary nor a result
    snaps = [torch.empty_like(d_out) for d_out in outputs]
    for d_in, d_stale, _ in inputs:
        d_in.copy_(d_stale)
    for d_out in outputs:
        d_out.fill_(0x11)
    torch.cuda.synchronize()
    # the hazard
    work = queued_work(torch, max(MIN_MS, ASK * idle_ms))
    for d_in, _, d_fresh in inputs:
        d_in.copy_(d_fresh)
    for d_out, snap in zip(outputs, snaps):
        d_out.fill_(CANARY)
        snap.copy_(d_out)
    running = work.still_running()
    t0 = time.perf_counter()
    result = call()
    staged_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    queued_ms = work.duration_ms()
    REPORT.append((name, queued_ms, idle_ms, staged_ms))
    print(f"stream-order {name}: queued work {queued_ms:.2f} ms ({work.fills} fills), idle call {idle_ms:.3f} ms, "
          f"staged call {staged_ms:.2f} ms", flush=True)
    assert running, f"{name}: the queued work had ended before the call: nothing was staged"
    assert queued_ms >= FACTOR * idle_ms, \
        f"{name}: {queued_ms:.2f} ms of queued work is less than {FACTOR} idle calls of {idle_ms:.3f} ms"
    for k, snap in enumerate(snaps):
        assert bool((snap == CANARY).all()), \
            f"{name}: output {k} was written under a reader queued on the default stream before the call"
    return result, idle_result


def control(torch, n=1 << 20):
    """The staging with a raw copy of the input on a fresh stream in place of
    the library call: first with no wait_stream, then after one."""
    require_default_stream(torch)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    a = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    b = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    d_in, unordered, ordered = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
    side = torch.cuda.Stream()
    d_in.copy_(a)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):  # the side stream's first copy, out of the way
        unordered.copy_(d_in)
    side.synchronize()
    unordered.zero_()
    torch.cuda.synchronize()
    work = queued_work(torch, MIN_MS)
    d_in.copy_(b)
    before = work.still_running()
    with torch.cuda.stream(side):
        unordered.copy_(d_in)
    side.synchronize()
    after = work.still_running()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ordered.copy_(d_in)
    side.synchronize()
    torch.cuda.synchronize()
    out = dict(running_before=before, running_after_unordered=after, queued_ms=work.duration_ms(),
               unordered_sees_stale=bool(torch.equal(unordered, a)), unordered_sees_fresh=bool(torch.equal(unordered, b)),
               ordered_sees_fresh=bool(torch.equal(ordered, b)), inputs_differ=not bool(torch.equal(a, b)))
    print(f"stream-order control: {out}", flush=True)
    return out
