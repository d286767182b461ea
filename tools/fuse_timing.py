#!/usr/bin/env python3
"""The fuse kernels (snerf_amd eval/utils/fuse.py, csrc/fuse.hip) on the clouds of tools/ortho_timing.py: the cloud of the fixture's
largest frame (tests/golden/geo_cloud_small.npz, 41 x 37 rays through GeoFrame.cloud) tiled to --side^2 points (a DFC2019 frame is
about 1024^2) on the bounds grid of the cloud (172 x 150 cells), at radius 0 and 1 -- hundreds to thousands of offers in every
occupied cell, nearly all of them EQUAL in altitude, so the selection is decided in the index bytes -- and a cloud of --side^2
DISTINCT points spread evenly over the same grid, which stands for a rendered frame.

Prints one JSON line.  Per cloud and radius: the device time of each entry over an event-bracketed window of --reps back-to-back
calls (count, scatter, select with the quartiles), the whole fuse_clouds call as the host sees it (two walks, the prefix sums and
their .item(), the select, the gathers; launch + synchronise, the median of --reps calls after a warm-up call), and beside them the
only route to the same rasters without these kernels: the device-to-host copy of the cloud plus the numpy restatement
(tests/fuse_numpy.py), whose words are compared with the device's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _timing import wall_ms, window_ms  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.baseline.components.normalization import StandardNormalization  # noqa: E402
from snerf_amd.eval.utils import dsm as D  # noqa: E402
from snerf_amd.eval.utils import fuse as F  # noqa: E402
from snerf_amd.framework.components.coordinate_systems import GeoFrame  # noqa: E402

KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


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
    g = D.grid_struct(grid)
    n = a.side * a.side
    tiled = frame.repeat(-(-n // n0), 1)[:n].contiguous()
    gen = torch.Generator().manual_seed(0)
    u = torch.rand((n, 3), generator=gen, dtype=torch.float64)
    distinct = torch.stack([grid.xoff + u[:, 0] * grid.xsize * grid.resolution, grid.yoff - u[:, 1] * grid.ysize * grid.resolution,
                            frame[:, 2].min().cpu() + u[:, 2] * 30.0], 1).to(dev)
    out = {"points": n, "grid": [grid.ysize, grid.xsize], "cells": grid.ysize * grid.xsize}
    for name, cloud in (("tiled", tiled), ("distinct", distinct)):
        for radius in (0, 1):
            tag = f"{name}_r{radius}"
            count, stats = F.count_offers(cloud, g, radius)
            offsets, total = F.offsets_of(count)
            keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            cursor = torch.zeros(count.numel(), dtype=torch.int32, device=dev)
            F.scatter_keys(cloud, g, offsets, cursor, keys, radius, 0, stats)
            words = F.select(keys, offsets, cursor, F.QUARTILES, g.out_h, g.out_w, stats)
            occupied = count[count > 0]
            out[f"{tag}_offers"] = total
            out[f"{tag}_offers_per_occupied_cell"] = [int(occupied.min()), float(occupied.float().mean()), int(occupied.max())]
            scratch = torch.zeros_like(count)
            out[f"{tag}_count_ms"] = window_ms(lambda: F.count_offers(cloud, g, radius, scratch, stats), a.reps)

            def scatter():                                     # the cursor starts from zero, as in a walk (its memset is in the window)
                cursor.zero_()
                F.scatter_keys(cloud, g, offsets, cursor, keys, radius, 0, stats)
            out[f"{tag}_scatter_ms"] = window_ms(scatter, a.reps)
            table, K = F.quantile_table(F.QUARTILES)
            out[f"{tag}_select_ms"] = window_ms(lambda: _lib.call("snerf_fuse_select", keys, offsets, keys.numel(), cursor, count.numel(),
                                                                  table, K, words, stats), a.reps)
            out[f"{tag}_fuse_clouds_wall_ms"] = wall_ms(lambda: F.fuse_clouds([cloud], g, radius), a.reps)
            if a.no_host_route:
                continue
            from tests import fuse_numpy as N
            from tests import ortho_numpy as R
            gd = R.grid(grid.xoff, grid.yoff, grid.resolution, grid.xsize, grid.ysize)
            t0 = time.perf_counter()
            h_cloud = cloud.cpu().numpy()
            t1 = time.perf_counter()
            want = N.fuse([h_cloud], gd, radius, F.QUARTILES)
            t2 = time.perf_counter()
            out[f"{tag}_copy_to_host_ms"] = (t1 - t0) * 1e3
            out[f"{tag}_numpy_ms"] = (t2 - t1) * 1e3
            out[f"{tag}_same_words"] = bool(np.array_equal(words.cpu().numpy().reshape(3, -1).view(np.uint64), want["words"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
