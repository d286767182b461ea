#!/usr/bin/env python3
"""The warp kernels (snerf_amd eval/utils/warp.py, csrc/warp.hip) on synthetic rasters built here: --sides^2 source cells under a
destination of the same extent at the steps 0.5, 1 (half a cell off), 2, 34/13, 8 and 64.  Nothing outside the repository is read.

Prints one JSON line.  Per side and step: the device time of snerf_warp_planes for every float method on one plane and of
snerf_warp_labels for both label methods -- the median, minimum and maximum over --windows event-bracketed windows of --reps
back-to-back calls each, after a warm-up call of that shape -- and the effective rate of the median, (source + destination bytes) /
time, which counts every byte once however often a kernel reads it; and beside them the host's time for the same job: one call of
scipy.ndimage.zoom (order 1, the bilinear job) when scipy is installed, else of the numpy restatement's average."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import window_ms  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.eval.utils import warp as W  # noqa: E402

STEPS = (("0.5", 0.5, 0.0), ("1_off_0.5", 1.0, 0.5), ("2", 2.0, 0.0), ("34_13", 34.0 / 13.0, 0.0), ("8", 8.0, 0.0), ("64", 64.0, 0.0))


def windows_ms(fn, reps, windows):
    """(median, min, max) milliseconds per call over `windows` windows of `reps` calls, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = [window_ms(fn, reps) for _ in range(windows)]
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true", help="skip the host's time for the same job (a profiler run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    out = {}
    for side in a.sides:
        host = rng.uniform(0.0, 100.0, (side, side)).astype(np.float32)
        host[rng.random((side, side)) < 0.02] = np.nan
        src = torch.from_numpy(host).to(dev).unsqueeze(0).contiguous()
        lab = torch.from_numpy(rng.integers(0, 6, (side, side)).astype(np.uint8)).to(dev)
        for tag, step, off in STEPS:
            n = int(side / step)
            m = _lib.SnerfWarpMap(off, step, off, step, side, side, n, n)
            key = f"s{side}_step{tag}"
            out[f"{key}_dst_side"] = n
            dst = torch.empty((1, n, n), dtype=torch.float32, device=dev)
            ldst = torch.empty((n, n), dtype=torch.uint8, device=dev)
            stats = torch.zeros(3, dtype=torch.int64, device=dev)
            for name in W.FLOAT_METHODS:
                med, lo, hi = windows_ms(lambda: _lib.call("snerf_warp_planes", src, 1, m, W.METHODS[name], 0.5, dst, stats), a.reps, a.windows)
                out[f"{key}_{name}_ms"] = [round(med, 5), round(lo, 5), round(hi, 5)]
                out[f"{key}_{name}_GBps"] = round(4.0 * (side * side + n * n) / (med * 1e-3) / 1e9, 1)
            for name in W.LABEL_METHODS:
                med, lo, hi = windows_ms(lambda: _lib.call("snerf_warp_labels", lab, m, W.METHODS[name], ldst, stats), a.reps, a.windows)
                out[f"{key}_label_{name}_ms"] = [round(med, 5), round(lo, 5), round(hi, 5)]
                out[f"{key}_label_{name}_GBps"] = round((side * side + n * n) / (med * 1e-3) / 1e9, 1)
            if a.no_host_route:
                continue
            try:
                from scipy import ndimage
                t0 = time.perf_counter()
                ndimage.zoom(host, 1.0 / step, order=1)
                out[f"{key}_scipy_zoom_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            except ImportError:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import warp_numpy as N
                t0 = time.perf_counter()
                N.warp_planes(host, N.Map(off, step, off, step, side, side, n, n), N.AVERAGE)
                out[f"{key}_numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
