#!/usr/bin/env python3
"""Wall time of the device SSIM (snerf_amd.eval.utils.metrics) beside the fp64 torch restatement of tests/ssim_ref.py on the
CPU: the kornia form (window 3, reflect) on a (1, 3, H, W) frame and ssim_inria (window 11, zeros), each the median of --reps
synchronised calls after one warm-up call.  The restatement column times one call.  Also prints the bytes the kernel must read
(8 B per pixel) and the fp64 FMAs of its window sums (5 ws^2 per pixel), from which a reader can place the times against the
HBM and fp64 peaks.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from snerf_amd.eval.utils import metrics as M  # noqa: E402
from tests import ssim_ref as R  # noqa: E402


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def cpu_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.rand((1, 3, a.size, a.size), generator=g)
    y = (0.9 * x + 0.1 * torch.rand((1, 3, a.size, a.size), generator=g)).clamp(0, 1)
    xd, yd = x.to(dev), y.to(dev)
    px = x.numel()
    out = {"shape": list(x.shape), "bytes_read": 8 * px}
    out["kornia_ws3_ms"] = gpu_ms(lambda: M.ssim(xd, yd), a.reps)
    out["kornia_ws3_fp64_fma"] = 5 * 9 * px
    out["inria_ws11_ms"] = gpu_ms(lambda: M.ssim_inria(xd, yd, 11), a.reps)
    out["inria_ws11_fp64_fma"] = 5 * 121 * px
    out["kornia_ws3_torch_cpu_fp64_ms"] = cpu_ms(lambda: R.kornia_map(x, y).mean())
    out["inria_ws11_torch_cpu_fp64_ms"] = cpu_ms(lambda: R.inria(x, y, 11))
    out["torch_threads"] = torch.get_num_threads()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
