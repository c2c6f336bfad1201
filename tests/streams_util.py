"""Helpers of tests/test_gpu_streams.py: a delayed producer, and the pattern "build on stream A behind a hold, consume on B"."""
import math
import time

import torch

HOLD_MS = 50.0           # how long a producer is held back; the "producer was not delayed" assertion decides whether it sufficed
_RATE = []


def cycles_per_ms():
    """Counter ticks of torch.cuda._sleep per millisecond on this device: one short spin timed with a pair of events, once
    per process.  Fails (never skips) when that does not give a finite positive rate."""
    if not _RATE:
        torch.cuda._sleep(1000)                      # loads the spin kernel
        torch.cuda.synchronize()
        ticks = 2_000_000
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda._sleep(ticks)
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        rate = ticks / ms if ms > 0 else float("nan")
        assert math.isfinite(rate) and rate > 0, f"torch.cuda._sleep({ticks}) took {ms} ms: no usable calibration"
        _RATE.append(rate)
    return _RATE[0]


def hold(stream, ms):
    """Enqueue a spin of about `ms` milliseconds on `stream`: what is enqueued there afterwards starts that much later."""
    ticks = int(ms * cycles_per_ms())
    if ticks > 0:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(ticks)


def poison(sizes):
    """Under the current stream: blocks of these byte sizes filled with 0xFF and freed again.  The next allocations of these
    sizes under this stream get them back: all-ones bytes (NaN as fp32, bf16 or fp16), not the stale but correct values a
    freed block could hold -- and the fill runs in stream order, behind whatever holds this stream back."""
    junk = [torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda").fill_(0xFF) for n in sizes]
    del junk


def first_done(probe, busy, limit=1.0):
    """Spin until one of two events is done -> True when `probe` was, with `busy` still pending.  `probe` stands on a stream
    that has nothing to wait for, so it is done at once unless the device runs that stream behind the held one."""
    t0 = time.perf_counter()
    while True:
        p, h = probe.query(), busy.query()
        if p or h or time.perf_counter() - t0 > limit:
            return p and not h


def runs_concurrently(held_stream, other, ms=2.0):
    """Whether work on `other` completes while `held_stream` is held: two streams may share a hardware queue, and then the
    second runs behind the first whatever the program says -- an unordered consumer would look ordered."""
    torch.cuda.synchronize()
    hold(held_stream, ms)
    busy, probe = torch.cuda.Event(), torch.cuda.Event()
    busy.record(held_stream)
    probe.record(other)
    ok = first_done(probe, busy)
    held_stream.synchronize()
    return ok


def independent_streams(tries=12):
    """Two side streams that the device runs concurrently with each other and with the current stream; fails when it finds
    none, since no test here can tell ordered from unordered work on streams that run one behind the other."""
    cycles_per_ms()
    cur = torch.cuda.current_stream()
    for _ in range(tries):
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        if runs_concurrently(a, b) and runs_concurrently(a, cur) and runs_concurrently(b, cur):
            return a, b
    raise AssertionError(f"no two of {2 * tries} side streams ran concurrently with each other and with the current stream")


def held(a, b, producer, consumer, sizes, what, ms=None):
    """Streams a and b wait for the current stream and not for each other.  On a: poison(sizes), a hold, producer() (a cache
    build; its results are dropped), an event.  On b: consumer().  -> consumer's result, after both streams have drained.
    Fails with "producer was not delayed" when the event behind the producer is done once the consumer has been enqueued, and
    when a marker in front of the consumer on b did not complete while a was held (the device ran b behind a: nothing shown)."""
    ms = HOLD_MS if ms is None else ms
    cycles_per_ms()                                  # calibrated before anything is held
    cur = torch.cuda.current_stream()
    a.wait_stream(cur)
    b.wait_stream(cur)
    with torch.cuda.stream(a):
        poison(sizes)
        hold(a, ms)
        producer()
        built = torch.cuda.Event()
        built.record(a)
    with torch.cuda.stream(b):
        marker = torch.cuda.Event()
        marker.record(b)
        t0 = time.perf_counter()
        out = consumer()
        enqueue = time.perf_counter() - t0
    delayed = built.query() is False
    concurrent = first_done(marker, built)
    b.synchronize()
    a.synchronize()
    print(f"\n{what}: consumer enqueued in {enqueue * 1e3:.2f} ms, producer still pending then: {delayed}, "
          f"consumer's stream running meanwhile: {concurrent}")
    assert delayed, "producer was not delayed"
    assert concurrent, "producer was not delayed relative to the consumer: the device ran the consumer's stream behind the held one"
    return out
