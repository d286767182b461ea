#!/usr/bin/env python3
"""The world-cloud launch (snerf_amd GeoFrame.cloud, csrc/geo.hip) on frames of the fixture's rays: the largest frame of
tests/golden/geo_cloud_small.npz (41 x 37 rays) and the same rays tiled to --side^2 rays (a DFC2019 frame is about 1024^2).
Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/geo_timing.py`, whose kernel statistics give the device
time of geo_cloud_kernel; on its own it prints the wall time per call (launch + the host's read of the 8 stats words), the
median of --reps calls after a warm-up call, as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import wall_ms  # noqa: E402
from snerf_amd.baseline.components.normalization import StandardNormalization  # noqa: E402
from snerf_amd.framework.components.coordinate_systems import GeoFrame  # noqa: E402

KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "geo_cloud_small.npz"))
    geo = GeoFrame(StandardNormalization().set_params(dict(zip(KEYS, z["norm_params"].tolist()))), str(z["zone_string"]))
    n0 = int(z["frame_w"][0] * z["frame_h"][0])
    dev = torch.device("cuda:0")
    rays, depth = torch.from_numpy(z["rays"]).to(dev), torch.from_numpy(z["depth"]).to(dev)
    out = {"frame_rays": n0, "frame_wall_ms": wall_ms(lambda: geo.cloud(rays[:n0], depth[:n0]), a.reps)}
    n = a.side * a.side
    k = -(-n // rays.shape[0])
    big_r, big_d = rays.repeat(k, 1)[:n].contiguous(), depth.repeat(k)[:n].contiguous()
    out.update(tiled_rays=n, tiled_wall_ms=wall_ms(lambda: geo.cloud(big_r, big_d), a.reps),
               tiled_wall_ms_with_lla=wall_ms(lambda: geo.cloud(big_r, big_d, want_lla=True), a.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
