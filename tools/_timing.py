"""What the timing tools share."""
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
