#!/usr/bin/env python3
"""What importance resampling costs: at the bench model (W = 512, H = 256, L = 8, C = 5) and 4096 rays with
n_samples = n_importance = 64, in the default arithmetic, the device time of

    proposal  the inference main pass on the 64 stratified depths asked for weights and z_vals (ops.render_pass_into)
    resample  the snerf_resample_z launch on its results (ops.resample_z, random uniforms)
    render    the inference main pass on the 128 merged depths asked for rgb, depth and weights: the pass the launch feeds

Each figure is the median over --reps windows of --inner back-to-back calls between two device events in one process, after
warm-up windows of the same shape; the legs alternate window by window, so that a drift of the machine falls on all of them.
Prints one JSON line and exits 1 when the resample launch takes 2 % of the rendering pass or more."""
import argparse
import json
import statistics
import sys
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from oracle import snerf_oracle as O  # noqa: E402
from snerf_amd import ops  # noqa: E402

BOUND = 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, S, Ni = a.rays, a.samples, a.importance
    cfg = O.OracleCfg(n_samples=S)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    sun = extras[:, :3].contiguous()
    t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()]
    zs = torch.linspace(0, 1, S).to(dev)
    ui = torch.rand(N, Ni, device=dev)
    spec = ops.ModelSpec()
    packed = ops.pack_params(spec, params)
    prop = {"weights": torch.empty(N, S, device=dev), "z_vals": torch.empty(N, S, device=dev)}
    pin = ops.PassInputs(sun_d=sun, rays=rays, z_steps=zs, u=u)
    ws_p = ops.render_pass_into(spec, params, pin, t, None, prop, packed=packed)
    zm = ops.resample_z(prop["z_vals"], prop["weights"], Ni, ui)
    out = {"rgb": torch.empty(N, 3, device=dev), "depth": torch.empty(N, device=dev), "weights": torch.empty(N, S + Ni, device=dev)}
    pin_m = ops.PassInputs(sun_d=sun, rays=rays, z_vals=zm)
    ws_m = ops.render_pass_into(spec, params, pin_m, t, None, out, packed=packed)
    legs = {"proposal": lambda: ops.render_pass_into(spec, params, pin, t, None, prop, packed=packed, workspace=ws_p),
            "resample": lambda: ops.resample_z(prop["z_vals"], prop["weights"], Ni, ui),
            "render": lambda: ops.render_pass_into(spec, params, pin_m, t, None, out, packed=packed, workspace=ws_m)}
    ms = {k: [] for k in legs}
    for rep in range(a.warmup + a.reps):
        for k, fn in legs.items():
            v = window_ms(fn, a.inner)
            if rep >= a.warmup:
                ms[k].append(v)
    result = {"rays": N, "samples": S, "importance": Ni, "reps": a.reps, "inner": a.inner}
    for k, v in ms.items():
        result[f"{k}_ms"] = round(statistics.median(v), 4)
        result[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    share = statistics.median(ms["resample"]) / statistics.median(ms["render"])
    result["resample_over_render"] = round(share, 5)
    result["bound"] = BOUND
    print(json.dumps(result))
    return 0 if share < BOUND else 1


if __name__ == "__main__":
    sys.exit(main())
