"""Forced timings for the stream hand-overs of a training step (tests/test_gpu_streams.py).

At test sizes every kernel has finished before the host issues the next one, so a missing wait between two HIP streams cannot
change a bit.  The two tools here take that luck away:

stall(stream)      queues known-long work on `stream` -- repeated in-place multiplies of one 2^27-float tensor, the technique of
                   tests/test_gpu_call.py -- and returns an event recorded behind it.  Whatever the host issues next on that stream
                   starts a quarter of a second late; whatever it issues on another stream and does not order behind this one runs
                   first, on stale or unwritten data.  The caller proves the stall did its job with still_running(ev) once the host
                   has issued the whole section under test and before anything synchronises: a stall that was over by then fails
                   the test ("stall too short"), it never lets it pass vacuously.
scribble(sizes, s) allocates, on stream `s`, four tensors of every byte size in `sizes` and fills them with 0xFF bytes (NaN as fp32).
                   A block that went back to that stream's pool while another stream still reads it is what the caching allocator
                   hands out next for its size: the scribble turns such an early free into NaNs in the result.  The caller holds
                   the returned tensors until its final synchronise.

The repeat count is calibrated once per session from HIP-event timing of the multiply itself.  The targets are test parameters, not
pass bars: 0.25 s for a single render call (STALL_S), 0.04 s per step of a 36-step loop (LOOP_STALL_S; the loop keeps the host at
most two steps ahead of the device, so the stall of the step being issued has not even begun when the host is done with it).
Calibrated on an MI355X: one multiply of the 2^27-float tensor takes 0.177 ms (1 GiB of traffic); 0.25 s = 1415 multiplies,
0.04 s = 227.

concurrent_streams(device) hands out the side and data streams the tests use: streams proven to run beside the default stream.
"""
import math

import torch

STALL_S = 0.25
LOOP_STALL_S = 0.04

_BUSY = {}      # device index -> (the 2^27-float tensor, kept for the session; milliseconds per multiply)


def _busy(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _BUSY:
        with torch.cuda.device(idx):
            t = torch.ones(1 << 27, device=device)
            for _ in range(4):                       # warm-up: the first launch loads the kernel
                t.mul_(-1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(32):
                t.mul_(-1.0)                         # (a sign flip: the values stay +-1 however often a session stalls)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / 32.0
        assert ms > 0.0, "stall calibration: the timed multiplies took no time"
        _BUSY[idx] = (t, ms)
        print(f"\nstream_stall: calibrated on cuda:{idx}: one multiply {ms:.3f} ms; {STALL_S} s = {math.ceil(STALL_S * 1e3 / ms)} multiplies, "
              f"{LOOP_STALL_S} s = {math.ceil(LOOP_STALL_S * 1e3 / ms)}")
    return _BUSY[idx]


def repeats(device, seconds=STALL_S):
    """how many multiplies make a stall of `seconds` on `device` (calibrates on first use)"""
    return max(1, math.ceil(seconds * 1e3 / _busy(device)[1]))


def stall(stream, seconds=STALL_S):
    """~`seconds` of device work queued on `stream`; -> the event recorded behind it.  Issues launches only: nothing here waits."""
    t, _ = _busy(stream.device)
    n = repeats(stream.device, seconds)
    with torch.cuda.stream(stream):
        for _ in range(n):
            t.mul_(-1.0)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


_PROBE_S = 0.02
_STREAMS = {}      # device index -> the streams concurrent_streams() has proven


def _runs_beside(a, b):
    """work issued on stream `a` completes while stream `b` is still stalled"""
    torch.cuda.synchronize(a.device)
    stalled = stall(b, _PROBE_S)
    done = torch.cuda.Event()
    done.record(a)
    done.synchronize()
    beside = not stalled.query()
    torch.cuda.synchronize(a.device)
    return beside


def concurrent_streams(device, n=2):
    """`n` streams of `device` that demonstrably run beside the default stream and beside each other; the same ones for the whole
    session.  The HIP runtime maps a process's streams onto a few hardware queues (four by default) in turn, and two streams that
    share a queue run in issue order: a stall on one holds the other back, and no missing wait between them can ever show.  One
    fresh torch stream in four shares the default stream's queue -- so the tests take their side and data streams from here, not
    from torch.cuda.Stream() as it comes."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    have = _STREAMS.setdefault(idx, [])
    tried = 0
    while len(have) < n:
        tried += 1
        assert tried <= 16, f"no {n} streams that run beside the default stream and each other among 16 fresh ones (fewer than {n + 1} hardware queues?)"
        cand = torch.cuda.Stream(device)
        others = [torch.cuda.default_stream(device)] + have
        if all(_runs_beside(cand, s) and _runs_beside(s, cand) for s in others):
            have.append(cand)
        if len(have) == n:
            print(f"\nstream_stall: {n} concurrent streams on cuda:{idx} after {tried} candidate(s)")
    return have[:n]


def still_running(ev, what=""):
    """the guard of every stalled case: the stall behind `ev` is not over yet"""
    assert not ev.query(), f"stall too short: it was over before the host had issued {what or 'the section under test'}"


def scribble(sizes, stream):
    """four 0xFF-filled tensors of every byte size in `sizes`, allocated and written on `stream`; hold the result"""
    held = []
    with torch.cuda.stream(stream):
        for nbytes in sizes:
            for _ in range(4):
                t = torch.empty(int(nbytes), dtype=torch.uint8, device=stream.device)
                t.fill_(0xFF)
                held.append(t)
    return held
