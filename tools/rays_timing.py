#!/usr/bin/env python3
"""Wall time of building a scene's rays: --images synthetic RPC images of --size^2 pixels (tests/rpc_numpy.synthetic_rpc, JAX-like
offsets, cubic and denominator terms).  Device: snerf_rpc_rays for every image in one call (a counting launch and a ray launch), then the normalisation
parameters (snerf_ray_bounds) and the in-place normalisation (snerf_normalize_rows) -- medians of --reps synchronised runs
after one warm-up.  Host: the fp64 numpy restatement of the same work (rpcm localisation at both altitudes, geodetic -> ECEF,
directions and bounds, as the reference's satnerf_construct; tests/rpc_numpy.py) on --workers processes, one image per task,
over the first --numpy-images images (the per-image time is reported, and the total scaled to all images).  The numpy part
runs first, before the process touches the GPU (the workers are forked).  Prints one JSON line."""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import rpc_numpy  # noqa: E402

ARGS = None


def _meta(k, size):
    return {"rpc": rpc_numpy.synthetic_rpc(1000 + k, w=size, h=size), "min_alt": -30.0, "max_alt": 50.0, "w": size, "h": size}


def numpy_image(k):
    m = _meta(k, ARGS.size)
    cam = rpc_numpy.RPCModel(m["rpc"])
    cols, rows = np.meshgrid(np.arange(m["w"]), np.arange(m["h"]))
    cols, rows = cols.ravel().astype(np.float64), rows.ravel().astype(np.float64)
    pts = []
    for alt in (m["max_alt"], m["min_alt"]):
        lon, lat = cam.localization(cols, rows, alt * np.ones(cols.shape))
        pts.append(np.vstack(rpc_numpy.geodetic_to_ecef(lat, lon, alt * np.ones(cols.shape))).T)
    d = pts[1] - pts[0]
    n = np.linalg.norm(d, axis=1)
    rays = np.hstack([pts[0], d / n[:, None], np.zeros((len(n), 1)), n[:, None]]).astype(np.float32)
    far = rays[:, :3] + rays[:, 7:8] * rays[:, 3:6]
    allp = np.concatenate([rays[:, :3], far])
    return allp.min(0), allp.max(0)


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--numpy-images", type=int, default=20)
    ARGS = ap.parse_args()
    res = {"images": ARGS.images, "size": ARGS.size, "rays": ARGS.images * ARGS.size ** 2}
    nimg = min(ARGS.numpy_images, ARGS.images)
    if nimg > 0:
        t0 = time.perf_counter()
        with mp.get_context("fork").Pool(ARGS.workers) as pool:
            for _ in pool.imap_unordered(numpy_image, range(nimg)):
                print(f"numpy image done at {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        s = time.perf_counter() - t0
        res.update(numpy_workers=ARGS.workers, numpy_images=nimg, numpy_s=round(s, 2),
                   numpy_s_scaled_to_all_images=round(s * ARGS.images / nimg, 2))

    import torch
    from snerf_amd.baseline.components.camera_models import RPCModel
    from snerf_amd.baseline.components.normalization import StandardNormalization
    from snerf_amd.baseline.components.rays import raise_on_failures, satnerf_construct
    dev = torch.device("cuda:0")
    metas = [_meta(k, ARGS.size) for k in range(ARGS.images)]
    cams = [RPCModel(m["rpc"], device=dev) for m in metas]

    def run():
        rays, fails = satnerf_construct(cams, [m["min_alt"] for m in metas], [m["max_alt"] for m in metas],
                                        sizes=[(m["w"], m["h"]) for m in metas], device=dev, check=False)
        norm = StandardNormalization()
        from snerf_amd.baseline.components.normalization import ray_bounds
        b = ray_bounds([rays])
        norm.center_range = b[9:13]
        norm.normalize_rays_(rays)
        return rays, fails

    rays, fails = run()
    torch.cuda.synchronize()
    raise_on_failures(fails)
    ts = []
    for _ in range(ARGS.reps):
        del rays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rays, fails = run()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    # the ray kernel alone, with HIP events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kt = []
    for _ in range(ARGS.reps):
        ev[0].record()
        r2, _ = satnerf_construct(cams, [m["min_alt"] for m in metas], [m["max_alt"] for m in metas],
                                  sizes=[(m["w"], m["h"]) for m in metas], device=dev, check=False)
        ev[1].record()
        torch.cuda.synchronize()
        kt.append(ev[0].elapsed_time(ev[1]))
        del r2
    res.update(gpu_build_normalise_ms=round(statistics.median(ts), 2), gpu_rays_ms=round(statistics.median(kt), 2),
               gpu_reps=ARGS.reps, finite=bool(torch.isfinite(rays).all()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
