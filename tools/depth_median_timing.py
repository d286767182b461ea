#!/usr/bin/env python3
"""What the median-depth launch costs: at the bench model (W = 512, H = 256, L = 8, C = 5) and 4096 rays x 64
samples, the device time of four legs, in the default arithmetic and then again with SNERF_FLAG_F16X1:

    a  the inference pass asked for rgb, depth, weights and z_vals            (depth_mode = "mean")
    b  the same pass with SNERF_FLAG_DEPTH_MEDIAN                              (depth_mode = "median")
    c  the geometry pass asked for depth, weights and z_vals
    d  the same pass with SNERF_FLAG_DEPTH_MEDIAN

b - a and d - c are the one launch the flag adds.  Each figure is the median (and min - max) over --reps windows of --inner
back-to-back calls between two device events in one process, after --warmup windows of the same shape; the legs alternate window by
window, so that a drift of the machine (the power cap) falls on all of them.  Before timing, every result but
the depth is checked to carry the same bits with and without the flag.  Prints one JSON line per arithmetic.
Run it under one time limit, e.g. `timeout -k 10 300 python tools/depth_median_timing.py`."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from oracle import snerf_oracle as O  # noqa: E402
from snerf_amd import _lib, ops  # noqa: E402


def run_mode(mode, a, dev):
    ops.BASE_FLAGS = _lib.MFMA_FLAGS[mode]
    N, S = a.rays, a.samples
    cfg = O.OracleCfg(n_samples=S)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    spec = ops.ModelSpec()
    packed = ops.pack_params(spec, params)
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    sun = extras[:, :3].contiguous()
    t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()]
    zs = torch.linspace(0, 1, S).to(dev)
    shapes = {"rgb": (N, 3), "depth": (N,), "weights": (N, S), "z_vals": (N, S)}

    def outs(keys):
        return {k: torch.empty(shapes[k], device=dev) for k in keys}

    pin_f = ops.PassInputs(sun_d=sun, rays=rays, z_steps=zs, u=u)
    pin_g = ops.PassInputs(rays=rays, z_steps=zs, u=u)
    legs = {}
    for full, (lo, hi) in ((True, ("a", "b")), (False, ("c", "d"))):
        keys = ("rgb", "depth", "weights", "z_vals") if full else ("depth", "weights", "z_vals")
        res = {}
        for leg, dm in ((lo, "mean"), (hi, "median")):
            o = outs(keys)
            if full:
                ws = ops.render_pass_into(spec, params, pin_f, t, None, o, packed=packed, depth_mode=dm)
                legs[leg] = (lambda o=o, w=ws, dm=dm: ops.render_pass_into(spec, params, pin_f, t, None, o, packed=packed, workspace=w, depth_mode=dm))
            else:
                ws = ops.geometry_pass_into(spec, params, pin_g, o, packed=packed, depth_mode=dm)
                legs[leg] = (lambda o=o, w=ws, dm=dm: ops.geometry_pass_into(spec, params, pin_g, o, packed=packed, workspace=w, depth_mode=dm))
            res[leg] = o
        torch.cuda.synchronize()
        for k in keys:      # the flag moves the depth and nothing else
            same = torch.equal(res[lo][k].view(torch.int32), res[hi][k].view(torch.int32))
            assert same == (k != "depth"), (mode, lo, hi, k)
    ms = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for k in sorted(legs):
            v = window_ms(legs[k], a.inner)
            if rep >= a.warmup:
                ms[k].append(v)
    result = {"mode": mode, "rays": N, "samples": S, "reps": a.reps, "inner": a.inner}
    for k in sorted(ms):
        result[f"{k}_ms"] = round(statistics.median(ms[k]), 4)
        result[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    for lo, hi in (("a", "b"), ("c", "d")):
        result[f"{hi}_minus_{lo}_ms"] = round(statistics.median(ms[hi]) - statistics.median(ms[lo]), 4)
        result[f"{hi}_over_{lo}"] = round(statistics.median(ms[hi]) / statistics.median(ms[lo]), 4)
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="f16x2,f16x1")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for mode in a.modes.split(","):
        run_mode(mode, a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
