#!/usr/bin/env python3
"""What orthorectifying costs: ONE snerf_orthorectify launch for --size^2 cells and --images images, next to the
composition of the existing entries whose work it does in one pass:

    fused      snerf_orthorectify with labels and a visibility plane, accumulators only (no per-image output)
    composed   snerf_geo_points (world -> scene, lla_out) once, then snerf_rpc_project per image: the projection ALONE, holding
               (cells, 3) + (cells, 3) fp64 points and per image (cells) fp64 columns and rows -- the sampling, the votes and the sums
               would still have to follow

The scene is synthetic and seeded: the five RPCs of tests/golden/scene_small with their image grids refined --refine times (41 x 37
pixels become 1025 x 925 at 25), random pixels and labels, a plane with boxes as the DSM, on the lattice over the images' corners.
Kernel times come from a profiler run of this program -- rocprofv3 --kernel-trace --stats -- python tools/orthorect_timing.py --
(kernels orthorectify_kernel, geo_scene_kernel, rpc_project_kernel); the JSON line printed here holds the wall time per call between
two device events (median over --reps windows of --inner calls after --warmup windows), for both legs alternating."""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from snerf_amd import _lib  # noqa: E402
from snerf_amd.baseline.components.camera_models import RPCModel, rpc_struct, struct_to_device  # noqa: E402
from snerf_amd.framework.util.conversions import zone_central_meridian  # noqa: E402
from tests import orthorect_numpy as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--refine", type=int, default=25)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("orthorect_timing: needs a GPU (a time from anywhere else says nothing)")
    if not 1 <= a.images <= _lib.RECT_MAX_IMAGES:
        raise SystemExit(f"orthorect_timing: --images in [1, {_lib.RECT_MAX_IMAGES}] (one launch)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = a.size
    xoff, yoff, _, _, _, w2, h2 = N.fixture_lattice(2.0)
    res = 2.0 * max(w2, h2) / n
    grid = _lib.SnerfDsmGrid(xoff, yoff, res, n, n, 0, 0, n, n)
    cells = n * n
    host = np.zeros((n, n), np.float32)
    for _ in range(cells // 4096):
        i, j = rng.integers(0, n, 2)
        bw, bh = rng.integers(8, 41, 2)
        host[j:j + bh, i:i + bw] = np.float32(rng.uniform(3.0, 30.0))
    dsm = torch.from_numpy(host).to(dev)
    metas = N.fixture_scene()["metas"]
    table = (_lib.SnerfRectImage * a.images)()
    cams, at = [], 0
    for k in range(a.images):
        m = metas[k % len(metas)]
        rpc = copy.deepcopy(m["rpc"])
        for key in ("col_offset", "col_scale", "row_offset", "row_scale"):
            rpc[key] *= a.refine
        table[k].rpc, table[k].row0 = rpc_struct(rpc), at
        table[k].w, table[k].h = (m["width"] - 1) * a.refine + 1, (m["height"] - 1) * a.refine + 1
        at += table[k].w * table[k].h
        cams.append(RPCModel(rpc, device=dev))
    table_dev = struct_to_device(table, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rgbs = torch.rand((at, 3), device=dev, generator=gen)
    labels = torch.randint(0, 5, (at,), device=dev, generator=gen, dtype=torch.uint8)
    visible = (torch.rand((a.images, cells), device=dev, generator=gen) > 0.05).to(torch.uint8)
    total = torch.zeros((3, cells), dtype=torch.int64, device=dev)
    count = torch.zeros(cells, dtype=torch.int32, device=dev)
    votes = torch.zeros((5, cells), dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    lon0 = zone_central_meridian(N.ZONE)

    def fused():
        _lib.call("snerf_orthorectify", dsm, grid, lon0, 0, table, table_dev, a.images, rgbs, labels, at, 5, visible, total, count, votes,
                  None, None, None, None, stats)

    east, north = N.cell_centres((xoff, yoff, res, 0, 0, n, n))
    enu = torch.from_numpy(np.stack([east, north, host.reshape(-1).astype(np.float64)], 1)).to(dev)
    params = _lib.SnerfGeoParams((C.c_double * 3)(0.0, 0.0, 0.0), 1.0, lon0, 0, _lib.GEO_TO_SCENE)
    xyz, lla = torch.empty_like(enu), torch.empty_like(enu)
    gstats = torch.zeros(8, dtype=torch.int64, device=dev)
    lon, lat, alt = (torch.empty(cells, dtype=torch.float64, device=dev) for _ in range(3))
    cols, rows = torch.empty((a.images, cells), dtype=torch.float64, device=dev), torch.empty((a.images, cells), dtype=torch.float64, device=dev)

    def composed():
        _lib.call("snerf_geo_points", enu, cells, params, xyz, lla, gstats)
        lat.copy_(lla[:, 0]), lon.copy_(lla[:, 1]), alt.copy_(lla[:, 2])
        for k, cam in enumerate(cams):
            _lib.call("snerf_rpc_project", cam.struct, cam.dev, lon, lat, alt, cells, cols[k], rows[k])

    for _ in range(a.warmup):
        window_ms(fused, a.inner), window_ms(composed, a.inner)
    ms = {"fused": [], "composed": []}
    for _ in range(a.reps):
        ms["fused"].append(window_ms(fused, a.inner))
        ms["composed"].append(window_ms(composed, a.inner))
    calls = (a.warmup + a.reps) * a.inner
    seen = int(stats[0]) // calls
    print(json.dumps({"cells": cells, "images": a.images, "pixels": at, "res_m": round(res, 4), "seen_pairs_per_call": seen,
                      "share_seen": round(seen / (cells * a.images), 4),
                      "fused_ms": round(statistics.median(ms["fused"]), 4), "fused_ms_min_max": [round(min(ms["fused"]), 4), round(max(ms["fused"]), 4)],
                      "composed_ms": round(statistics.median(ms["composed"]), 4),
                      "composed_ms_min_max": [round(min(ms["composed"]), 4), round(max(ms["composed"]), 4)],
                      "composed_fp64_bytes_held": int(8 * cells * (6 + 3 + 2 * a.images))}), flush=True)


if __name__ == "__main__":
    main()
