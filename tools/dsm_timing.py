#!/usr/bin/env python3
"""Wall time of the device DSM evaluation (snerf_amd.eval.utils.dsm) beside the numpy restatement of tests/dsm_numpy.py:
rasterising a 1M-point cloud onto a 1024^2 grid, registering a 1024^2 DSM pair (the whole pyramid: 1024 -> 64, five levels of
121 shifts), and the whole compute_mae.  GPU numbers are the median of --reps calls after one warm-up call, each call
synchronised (every level of the search reads its 121 correlations back to the host, as the API does).  The numpy column
times one call (the registration: the finest level's 121-shift search only, the rest being smaller).  Prints one JSON line."""
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

from snerf_amd.eval.utils import dsm as D  # noqa: E402
from tests import dsm_numpy as N  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--points", type=int, default=1 << 20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, res = a.size, 0.5
    rng = np.random.default_rng(0)
    cloud = np.stack([rng.uniform(0, n * res, a.points) + 3.0e5, rng.uniform(0, n * res, a.points) + 4.0e6,
                      300.0 + 10.0 * rng.standard_normal(a.points)], 1)
    c = torch.from_numpy(cloud).to(dev)
    grid = D.dsm_grid_from_cloud(c)
    out = {"points": a.points, "grid": [grid.ysize, grid.xsize]}
    out["rasterize_ms"] = gpu_ms(lambda: D.rasterize(c, grid), a.reps)
    out["rasterize_numpy_ms"] = cpu_ms(lambda: N.rasterize(cloud, *grid))
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    f = 300.0 + 4.0 * np.sin(x / 37.0) + 3.0 * np.cos(y / 23.0)
    for _ in range(400):
        j, i = rng.integers(0, n - 30, 2)
        f[j:j + rng.integers(5, 30), i:i + rng.integers(5, 30)] += rng.uniform(3.0, 20.0)
    gt = f.astype(np.float32)
    pred = (np.roll(f, (3, -2), (0, 1)) + 0.5 + rng.normal(0, 0.1, f.shape)).astype(np.float32)
    pred[rng.random(pred.shape) < 0.05] = np.nan
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    trace = []
    D.compute_shift(g, p, trace=trace)
    out["levels"] = len(trace)
    out["shift"] = list(trace[-1][4:])
    out["register_ms"] = gpu_ms(lambda: D.compute_shift(g, p), a.reps)
    out["compute_mae_ms"] = gpu_ms(lambda: D.compute_mae(p, g), a.reps)
    out["register_level0_numpy_ms"] = cpu_ms(lambda: N.compute_ncc(gt, pred, 5, trace[-1][2], trace[-1][3]))
    out["torch_threads"] = torch.get_num_threads()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
