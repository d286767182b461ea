#!/usr/bin/env python3
"""The terrain kernels (snerf_amd eval/utils/terrain.py, csrc/terrain.hip) on synthetic towns built here: --sides^2 cells at 0.5 m,
a gently sloped ground with boxes of 12 to 60 cells a side on a jittered street grid (roofs 6 to 40 m above the ground).  Nothing
outside the repository is read.

Prints one JSON line.  Per side: the device time of snerf_terrain_keys, of snerf_terrain_open (its four launches, with the flag
update) at radius 1, 16, 128 and 512 and of snerf_terrain_fill (its three launches) on the town's ground mask and on a raster whose
only ground cell is one corner, each over an event-bracketed window of --reps back-to-back calls; the two ratios the design is held
to -- open at radius 512 over radius 1 (van Herk: a constant number of operations per cell, so what is left is how well each radius
fills the machine) and fill on the one-corner raster over the town (the scans do the same work on both; the combining pass does its
fp64 arithmetic on the cells that are not ground only); the whole terrain() call as the host sees it (launches + synchronise + the
counts, the median of --reps calls after a warm-up call) at the default schedule; and beside them the only route to the same
opening without these kernels: the device-to-host copy of the key plane plus scipy.ndimage.grey_opening per level, when scipy is
installed."""
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

from _timing import wall_ms, warm_window_ms as window_ms  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.eval.utils import dsm as D  # noqa: E402
from snerf_amd.eval.utils import ortho as OR  # noqa: E402
from snerf_amd.eval.utils import terrain as TR  # noqa: E402

RADII = (1, 16, 128, 512)


def town(side, seed=0):
    rng = np.random.default_rng(seed)
    jj, ii = np.mgrid[0:side, 0:side]
    alt = (3.0 + (ii + 2 * jj) / 1024.0).astype(np.float32)
    pitch = 80
    for j0 in range(8, side - pitch, pitch):
        for i0 in range(8, side - pitch, pitch):
            nj, ni = rng.integers(12, 61, 2)
            dj, di = rng.integers(0, pitch - 64, 2)
            alt[j0 + dj:j0 + dj + nj, i0 + di:i0 + di + ni] = 3.0 + float(rng.integers(6, 41))
    return alt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true", help="skip the copy + scipy route (a profiler run)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for side in a.sides:
        tag = f"s{side}"
        alt = torch.from_numpy(town(side)).to(dev)
        grid = D.DsmGrid(500000.0, 4100000.0, 0.5, side, side)
        ws = TR.workspace(side, side, dev)
        key = torch.empty((side, side), dtype=torch.int32, device=dev)
        flags = torch.empty((side, side), dtype=torch.uint8, device=dev)
        kstats = torch.zeros(3, dtype=torch.int64, device=dev)
        out[f"{tag}_keys_ms"] = window_ms(
            lambda: _lib.call("snerf_terrain_keys", alt, None, side, side, None, OR.Z0, OR.Q, key, flags, kstats), a.reps)
        opened = torch.empty_like(key)
        ostats = torch.zeros(1, dtype=torch.int64, device=dev)
        for r in RADII:
            scratch = flags.clone()
            out[f"{tag}_open_r{r}_ms"] = window_ms(
                lambda: _lib.call("snerf_terrain_open", key, side, side, r, 65536, opened, scratch, ws, ostats), a.reps)
        out[f"{tag}_open_r512_over_r1"] = out[f"{tag}_open_r512_ms"] / out[f"{tag}_open_r1_ms"]
        res = TR.terrain(alt, grid)
        out[f"{tag}_levels"] = len(res["schedule"]["radii"])
        out[f"{tag}_not_ground_cells"] = side * side - res["stats"]["ground"]
        dtm, ndsm = torch.empty_like(alt), torch.empty_like(alt)
        reach = torch.empty_like(key)
        fstats = torch.zeros(3, dtype=torch.int64, device=dev)
        corner = torch.full_like(flags, TR.FLAGGED)
        corner[-1, 0] = 0
        for name, f in (("town", res["flags"]), ("one_corner", corner)):
            out[f"{tag}_fill_{name}_ms"] = window_ms(
                lambda: _lib.call("snerf_terrain_fill", key, f, alt, side, side, OR.Z0, OR.Q, dtm, ndsm, reach, ws, fstats), a.reps)
        out[f"{tag}_fill_one_corner_over_town"] = out[f"{tag}_fill_one_corner_ms"] / out[f"{tag}_fill_town_ms"]
        out[f"{tag}_terrain_wall_ms"] = wall_ms(lambda: TR.terrain(alt, grid), a.reps)
        if a.no_host_route:
            continue
        try:
            from scipy import ndimage
        except ImportError:
            continue
        t0 = time.perf_counter()
        hk = key.cpu().numpy()
        t1 = time.perf_counter()
        out[f"{tag}_copy_to_host_ms"] = (t1 - t0) * 1e3
        for r in RADII:
            t1 = time.perf_counter()
            host = ndimage.grey_opening(hk, size=(2 * r + 1, 2 * r + 1), mode="constant", cval=0)
            out[f"{tag}_scipy_open_r{r}_ms"] = (time.perf_counter() - t1) * 1e3
            del host
    print(json.dumps(out))


if __name__ == "__main__":
    main()
