#!/usr/bin/env python3
"""The ortho kernels (snerf_amd eval/utils/ortho.py, csrc/ortho.hip) on the cloud of the fixture's largest frame
(tests/golden/geo_cloud_small.npz, 41 x 37 rays through GeoFrame.cloud) tiled to --side^2 points (a DFC2019 frame is about
1024^2), at radius 0 and 1, on the bounds grid of the cloud.  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/ortho_timing.py --no-host-route`, whose kernel statistics give the device
times of ortho_top_kernel, ortho_votes_kernel and ortho_gather_kernel; on its own it prints, as one JSON line, the wall time
per call as the host sees it (launch + synchronise; the median of --reps calls after a warm-up call) and, beside it, the only
route to the same arrays without these kernels: the device-to-host copy of cloud, colours and labels plus the numpy restatement
(tests/ortho_numpy.py).  The tiled cloud repeats 1,517 points, so a cell receives hundreds of equal offers: the contended case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import wall_ms  # noqa: E402
from snerf_amd.baseline.components.normalization import StandardNormalization  # noqa: E402
from snerf_amd.eval.utils import dsm as D  # noqa: E402
from snerf_amd.eval.utils import ortho as OR  # noqa: E402
from snerf_amd.framework.components.coordinate_systems import GeoFrame  # noqa: E402

KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")
N_CLASSES = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true", help="skip the copy + numpy route (a profiler run)")
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "geo_cloud_small.npz"))
    geo = GeoFrame(StandardNormalization().set_params(dict(zip(KEYS, z["norm_params"].tolist()))), str(z["zone_string"]))
    n0 = int(z["frame_w"][0] * z["frame_h"][0])
    dev = torch.device("cuda:0")
    rays, depth = torch.from_numpy(z["rays"][:n0]).to(dev), torch.from_numpy(z["depth"][:n0]).to(dev)
    frame, bounds = geo.cloud(rays, depth)
    grid = D.dsm_grid_from_cloud(None, D.RESOLUTION, bounds=bounds)
    n = a.side * a.side
    cloud = frame.repeat(-(-n // n0), 1)[:n].contiguous()
    g = torch.Generator().manual_seed(0)
    rgb = torch.rand((n, 3), generator=g).to(dev)
    labels = torch.randint(0, N_CLASSES, (n,), generator=g).to(dev)
    out = {"points": n, "grid": [grid.ysize, grid.xsize], "cells": grid.ysize * grid.xsize}
    for radius in (0, 1):
        top, _ = OR.top_surface(cloud, grid, radius)
        out[f"r{radius}_top_wall_ms"] = wall_ms(lambda: OR.top_surface(cloud, grid, radius), a.reps)
        out[f"r{radius}_votes_wall_ms"] = wall_ms(lambda: OR.label_votes(cloud, labels, grid, N_CLASSES, radius), a.reps)
        out[f"r{radius}_gather_wall_ms"] = wall_ms(lambda: OR.gather(top, 0, n, rgb=rgb, labels=labels), a.reps)
        if a.no_host_route:
            continue
        from tests import ortho_numpy as R
        gd = R.grid(grid.xoff, grid.yoff, grid.resolution, grid.xsize, grid.ysize)
        t0 = time.perf_counter()
        h_cloud, h_rgb, h_labels = cloud.cpu().numpy(), rgb.cpu().numpy(), labels.cpu().numpy()
        t1 = time.perf_counter()
        h_top, _ = R.top_at(h_cloud, gd, radius)
        R.votes_at(h_cloud, h_labels, gd, N_CLASSES, radius)
        R.gather(h_top, 0, n, rgb=h_rgb, labels=h_labels)
        t2 = time.perf_counter()
        out[f"r{radius}_copy_to_host_ms"] = (t1 - t0) * 1e3
        out[f"r{radius}_numpy_ms"] = (t2 - t1) * 1e3
        out[f"r{radius}_same_words"] = bool(np.array_equal(top.cpu().numpy().reshape(-1).view(np.uint64), h_top))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
