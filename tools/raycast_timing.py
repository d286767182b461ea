#!/usr/bin/env python3
"""What the DSM ray cast costs and what guided sampling saves, on a synthetic map: a 1024 x 1024 DSM of
0.5 m cells (rolling ground with blocks on it) under slanted rays 70 m long, built through GeoFrame.to_scene as nadir rays are.

    (a) the cast launch alone (snerf_dsm_segment_hit on ready UTM end points) at 4,096 rays and at 2^20 rays;
    (b) at the bench model (W = 512, L = 8, C = 5) and --frame rays: lean_inference at n_samples = 64 against
        guided_lean_inference at 16 and at 32 samples on the same rays, the cast (two GeoFrame.cloud launches, the march, the
        depth), guide_rays and sample_z INSIDE the guided time.  Wall time of whole calls between device synchronisations: the
        host work of a call is part of what a user waits for.

Each figure is the median (and min - max) over --reps windows after --warmup windows; the legs alternate window by window, so that
a drift of the machine falls on all of them.  Prints one JSON line.  No ratio is promised: the tool reports.
Run it under one time limit, e.g. `timeout -k 10 300 python tools/raycast_timing.py`."""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from bench import make_cfgs  # noqa: E402
from snerf_amd.eval.utils import raycast as R  # noqa: E402
from snerf_amd.eval.utils.dsm import DsmGrid  # noqa: E402
from snerf_amd.eval.utils.util import guided_lean_inference, lean_inference  # noqa: E402
from snerf_amd.framework.components.coordinate_systems import GeoFrame  # noqa: E402
from snerf_amd.framework.pipelines import load_pipeline  # noqa: E402

CELLS, RES = 1024, 0.5
ALT_LO, ALT_HI = -30.0, 40.0       # the rays' altitude slab round the ground's mean, metres
BAND = (4.0, 6.0)                  # the band of leg (b): 4 m in front of the hit, 6 m behind


def ecef(lat_deg, lon_deg, alt):
    a, e2 = 6378137.0, 6.69437999014e-3
    lat, lon = math.radians(lat_deg), math.radians(lon_deg)
    n = a / math.sqrt(1.0 - e2 * math.sin(lat) ** 2)
    return ((n + alt) * math.cos(lat) * math.cos(lon), (n + alt) * math.cos(lat) * math.sin(lon), (n * (1.0 - e2) + alt) * math.sin(lat))


def scene(dev, seed=0):
    """(GeoFrame, DsmGrid, dsm (1024, 1024) f32): a frame centred near Jacksonville (zone 17R) with a range of 300 m, the lattice
    centred under it, rolling ground (+-4 m) with 200 flat-roofed blocks of 5 to 25 m"""
    norm = types.SimpleNamespace(calculate_center_range=lambda: (ecef(30.3, -81.66, 0.0), 300.0))
    geo = GeoFrame(norm, "17R")
    origin = geo.points(torch.zeros((1, 3), dtype=torch.float64, device=dev))[0][0].cpu().tolist()
    half = CELLS * RES / 2
    grid = DsmGrid(math.floor(origin[0]) - half, math.floor(origin[1]) + half, RES, CELLS, CELLS)
    g = torch.Generator().manual_seed(seed)
    j, i = torch.meshgrid(torch.arange(CELLS, dtype=torch.float32), torch.arange(CELLS, dtype=torch.float32), indexing="ij")
    dsm = origin[2] + 4.0 * torch.sin(i / 90.0) * torch.cos(j / 70.0)
    for _ in range(200):
        w, h = (int(v) for v in torch.randint(8, 60, (2,), generator=g))
        x, y = int(torch.randint(0, CELLS - w, (1,), generator=g)), int(torch.randint(0, CELLS - h, (1,), generator=g))
        dsm[y:y + h, x:x + w] = origin[2] + float(torch.empty(1).uniform_(5.0, 25.0, generator=g))
    return geo, grid, dsm.contiguous().to(dev), origin


def slanted_rays(geo, origin, n, dev, seed=1):
    """n rays (n, 8) fp32 [o, d, near = 0, far]: from (E + 20 m, N + 10 m, alt + 40 m) down to (E, N, alt - 30 m), (E, N) uniform over the
    central 400 m square of the lattice -- built as nadir_construct builds its vertical ones"""
    g = torch.Generator().manual_seed(seed)
    en = (torch.rand((n, 2), generator=g, dtype=torch.float64) - 0.5) * 400.0
    pts = torch.empty((2, n, 3), dtype=torch.float64)
    pts[0, :, 0], pts[0, :, 1], pts[0, :, 2] = origin[0] + en[:, 0] + 20.0, origin[1] + en[:, 1] + 10.0, origin[2] + ALT_HI
    pts[1, :, 0], pts[1, :, 1], pts[1, :, 2] = origin[0] + en[:, 0], origin[1] + en[:, 1], origin[2] + ALT_LO
    xyz, _ = geo.to_scene(pts.reshape(-1, 3).to(dev))
    top, d = xyz[:n], xyz[n:] - xyz[:n]
    norm = torch.linalg.vector_norm(d, dim=1, keepdim=True)
    return torch.cat([top, d / norm, torch.zeros_like(norm), norm], 1).float().contiguous()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(result, name, values):
    result[f"{name}_ms"] = round(statistics.median(values), 4)
    result[f"{name}_ms_min_max"] = [round(min(values), 4), round(max(values), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=40960 * 2, help="rays of leg (b)")
    ap.add_argument("--chunk", type=int, default=40960)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    geo, grid, dsm, origin = scene(dev)
    result = {"dsm": [CELLS, CELLS], "res_m": RES, "ray_m": round(math.hypot(math.hypot(20.0, 10.0), ALT_HI - ALT_LO), 2)}

    # (a) the launch alone
    legs = {}
    for n in (4096, 1 << 20):
        rays = slanted_rays(geo, origin, n, dev)
        p0, p1 = geo.cloud(rays, rays[:, 6].contiguous())[0], geo.cloud(rays, rays[:, 7].contiguous())[0]
        s, state, cell = R.segment_hits(p0, p1, grid, dsm, want_cells=True)
        result[f"cast_{n}_states"] = torch.bincount(state.long(), minlength=6).cpu().tolist()
        legs[f"cast_{n}"] = (lambda p0=p0, p1=p1: R.segment_hits(p0, p1, grid, dsm, want_cells=True))
    ms = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for k in legs:
            v = window_ms(legs[k], a.inner)
            if rep >= a.warmup:
                ms[k].append(v)
    for k, v in ms.items():
        summary(result, k, v)
    result["cast_ns_per_ray_at_2^20"] = round(result[f"cast_{1 << 20}_ms"] * 1e6 / (1 << 20), 3)

    # (b) a frame at the bench model
    cfgs = make_cfgs(4096, 64, 1)
    cfgs.pipeline.render_chunk_size = a.chunk
    pipe = load_pipeline(cfgs).to(dev)
    rays = slanted_rays(geo, origin, a.frame, dev, seed=2)
    extras = torch.zeros((a.frame, 4), dtype=torch.float32, device=dev)
    extras[:, 2] = 1.0
    keys = ("rgb_coarse", "depth_coarse", "semantic_label_coarse")
    guides = {S: R.DsmGuide(geo, grid, dsm, BAND[0], BAND[1], S) for S in (16, 32)}
    legs = {"lean_64": lambda: lean_inference(cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options={"perturb": 0})}
    for S, guide in guides.items():
        legs[f"guided_{S}"] = (lambda guide=guide: guided_lean_inference(cfgs, pipe.renderer, pipe.models, rays, extras, guide, keys=keys))
    legs["cast_and_guide_only"] = lambda: R.guide_rays(rays, R.cast_rays(rays, geo, grid, dsm), BAND[0], BAND[1], geo.params.range)
    ms = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for k in legs:
            v = wall_ms(legs[k])
            if rep >= a.warmup:
                ms[k].append(v)
    for k, v in ms.items():
        summary(result, k, v)
    state = guided_lean_inference(cfgs, pipe.renderer, pipe.models, rays, extras, guides[16], keys=("depth_coarse",))["guide_state"]
    result.update(frame_rays=a.frame, chunk=a.chunk, band_m=list(BAND), guided_rows=int(R.is_hit(state).sum()), reps=a.reps)
    for S in (16, 32):
        result[f"guided_{S}_over_lean_64"] = round(result[f"guided_{S}_ms"] / result["lean_64_ms"], 4)
        result[f"samples_ratio_{S}"] = S / 64
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
