#!/usr/bin/env python3
"""What the geometry pass saves: at the bench model (W = 512, H = 256, L = 8, C = 5) and 4096 rays, the device
time of four legs, in the default arithmetic and then again with SNERF_FLAG_F16X1:

    a  4096 x 64   the full inference pass asked for weights and z_vals   (the proposal of n_importance > 0 as it was)
    b  4096 x 64   the geometry pass asked for the same two results       (the proposal as it is)
    c  4096 x 128  the full inference pass asked for depth                (a depth-only product as it was)
    d  4096 x 128  the geometry pass asked for depth

Each figure is the median (and min - max) over --reps windows of --inner back-to-back calls between two device events in one
process, after --warmup windows of the same shape; the legs alternate window by window, so that a drift of the machine (the power
cap) falls on all of them.  Prints one JSON line per arithmetic.  Exits 1 when a geometry leg is slower than
its full leg beyond the windows' own spread, i.e. when even its fastest window is slower than the full leg's slowest.
Run it under one time limit, e.g. `timeout -k 10 300 python tools/geometry_timing.py`."""
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
    N = a.rays
    cfg = O.OracleCfg(n_samples=a.samples)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    spec = ops.ModelSpec()
    packed = ops.pack_params(spec, params)
    legs, sizes = {}, {}
    for S, keys, full_leg, geo_leg in ((a.samples, ("weights", "z_vals"), "a", "b"), (2 * a.samples, ("depth",), "c", "d")):
        b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
        rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
        sun = extras[:, :3].contiguous()
        t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()]
        zs = torch.linspace(0, 1, S).to(dev)

        def outs():
            return {k: torch.empty((N,) if k == "depth" else (N, S), device=dev) for k in keys}

        pin_f = ops.PassInputs(sun_d=sun, rays=rays, z_steps=zs, u=u)
        pin_g = ops.PassInputs(rays=rays, z_steps=zs, u=u)
        of, og = outs(), outs()
        ws_f = ops.render_pass_into(spec, params, pin_f, t, None, of, packed=packed)
        ws_g = ops.geometry_pass_into(spec, params, pin_g, og, packed=packed)
        torch.cuda.synchronize()
        for k in keys:      # the two legs compute the same thing
            assert torch.equal(of[k].view(torch.int32), og[k].view(torch.int32)), (mode, S, k)
        sizes[full_leg], sizes[geo_leg] = ws_f.numel(), ws_g.numel()
        legs[full_leg] = (lambda pin=pin_f, t=t, o=of, w=ws_f: ops.render_pass_into(spec, params, pin, t, None, o, packed=packed, workspace=w))
        legs[geo_leg] = (lambda pin=pin_g, o=og, w=ws_g: ops.geometry_pass_into(spec, params, pin, o, packed=packed, workspace=w))
    ms = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for k in sorted(legs):
            v = window_ms(legs[k], a.inner)
            if rep >= a.warmup:
                ms[k].append(v)
    result = {"mode": mode, "rays": N, "samples": [a.samples, 2 * a.samples], "reps": a.reps, "inner": a.inner}
    for k in sorted(ms):
        result[f"{k}_ms"] = round(statistics.median(ms[k]), 4)
        result[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        result[f"{k}_workspace_mib"] = round(sizes[k] / 2 ** 20, 1)
    slower = []
    for full_leg, geo_leg in (("a", "b"), ("c", "d")):
        result[f"{geo_leg}_over_{full_leg}"] = round(statistics.median(ms[geo_leg]) / statistics.median(ms[full_leg]), 4)
        if min(ms[geo_leg]) > max(ms[full_leg]):
            slower.append(geo_leg)
    result["geometry_slower_beyond_spread"] = slower
    print(json.dumps(result), flush=True)
    return not slower


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
    ok = True
    for mode in a.modes.split(","):
        ok = run_mode(mode, a, dev) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
