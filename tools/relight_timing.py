#!/usr/bin/env python3
"""What an extra sun costs: at the bench model (W = 512, H = 256, L = 8, C = 5) and 4096 rays x 64 samples,
in the default and the one-plane arithmetic, the device time of

    full     one inference main pass asked for rgb and sun (ops.render_pass_into), the unit a loop over suns pays per sun
    relight  one relight of that chunk asked for rgb and sun (ops.relight_pass_into)

Each figure is the median over --reps windows of --inner back-to-back passes between two device events, after warm-up windows of
the same shape; the two legs alternate window by window, so that a drift of the machine falls on both.  Prints one JSON line.
--full-only times the full pass alone: the leg that also runs on a build without the relight pass (a parent commit's library through
SNERF_LIB_PATH), to confirm that the full pass itself costs what it did."""
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
from snerf_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, S = a.rays, a.samples
    cfg = O.OracleCfg(n_samples=S)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    sun_a = extras[:, :3].contiguous()
    sun_b = torch.nn.functional.normalize(sun_a + torch.tensor([0.3, -0.2, 0.1], device=dev), dim=1)
    t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()]
    zs = torch.linspace(0, 1, S).to(dev)
    result = {"rays": N, "samples": S, "reps": a.reps, "inner": a.inner, "lib": os.environ.get("SNERF_LIB_PATH", "tree")}
    for mode in ("f16x2", "f16x1"):
        spec = ops.ModelSpec(mfma=mode)
        packed = ops.pack_params(spec, params)
        out = {"rgb": torch.empty(N, 3, device=dev), "sun": torch.empty(N, S, 1, device=dev)}
        pin = ops.PassInputs(sun_d=sun_a, rays=rays, z_steps=zs, u=u)
        ws = ops.render_pass_into(spec, params, pin, t, None, out, packed=packed)
        legs = {"full": lambda: ops.render_pass_into(spec, params, pin, t, None, out, packed=packed, workspace=ws)}
        if not a.full_only:
            legs["relight"] = lambda: ops.relight_pass_into(spec, params, sun_b, t, None, out, ws, packed=packed, n_samples=S)
        ms = {k: [] for k in legs}
        for rep in range(a.warmup + a.reps):
            for k, fn in legs.items():      # (a relight follows a full pass on the workspace in every window order)
                v = window_ms(fn, a.inner)
                if rep >= a.warmup:
                    ms[k].append(v)
        for k, v in ms.items():
            result[f"{mode}_{k}_ms"] = round(statistics.median(v), 4)
            result[f"{mode}_{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        if "relight" in ms:
            result[f"{mode}_relight_over_full"] = round(statistics.median(ms["relight"]) / statistics.median(ms["full"]), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
