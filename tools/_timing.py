"""What the timing tools share."""
import statistics
import time

import torch


def window_ms(fn, inner):
    """milliseconds per call of fn over one event-bracketed window of `inner` back-to-back calls on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def warm_window_ms(fn, reps):
    """window_ms after one warm-up call outside the window"""
    fn()
    return window_ms(fn, reps)


def wall_ms(fn, reps):
    """median wall-clock milliseconds of fn over `reps` synchronised calls, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)
