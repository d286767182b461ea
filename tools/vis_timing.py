#!/usr/bin/env python3
"""Wall time of the streaming visualisation maps (snerf_amd.eval.utils.vismaps, csrc/vismaps.hip) on one --size^2 frame at
--samples samples per ray: snerf_vis_fold alone on one chunk with every head (it must read m * S * 36 B: weights, albedo, sun,
sky, beta), lean_frame_maps (render + fold chunk by chunk), and the route it replaces: lean_inference of the per-sample results
followed by torch.sum(weights[..., None] * factor, -2) per factor.  Medians of --reps synchronised runs after one warm-up run;
the peak allocation growth of both frame paths.  Random-init model of the flagship width.  Prints one JSON line.  Under
`rocprofv3 --kernel-trace --stats -- python tools/vis_timing.py` the kernel's own time is vis_fold_kernel's row."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import snerf_oracle as O  # noqa: E402
from snerf_amd.eval.utils import vismaps as V  # noqa: E402
from snerf_amd.eval.utils.util import lean_inference  # noqa: E402
from tests.test_gpu_pipeline import _pipeline_for  # noqa: E402


def gpu_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=1 << 16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = O.OracleCfg(n_samples=a.samples, render_chunk_size=a.chunk)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    n, S, m = a.size * a.size, a.samples, a.chunk
    bank = O.batch_to_torch(O.synthetic_batch(4096, S, seed=1))
    reps = -(-n // 4096)
    rays = bank["rays"].to(dev).repeat(reps, 1)[:n].contiguous()
    extras = bank["extras"].to(dev).repeat(reps, 1)[:n].contiguous()
    opts = {"perturb": 0}
    heads = ("albedo", "sun", "sky", "beta")
    keys = [k + "_coarse" for k in ("weights",) + heads]
    out = {"rays": n, "samples": S, "chunk": m, "fc_units": cfg.fc_units, "fold_bytes_read": m * S * 36}

    r = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays[:m], extras[:m], keys=keys, render_options=opts)
    planes = {"albedo_map": torch.empty(3, m, device=dev), "sun_map": torch.empty(m, device=dev),
              "sky_map": torch.empty(3, m, device=dev), "beta_map": torch.empty(m, device=dev)}
    stats = V.new_stats(dev)

    def fold():
        V.fold_chunk(planes, stats, 0, m, m, S, weights=r["weights_coarse"], albedo=r["albedo_coarse"], sun=r["sun_coarse"],
                     sky=r["sky_coarse"], beta=r["beta_coarse"])
    out["fold_ms_per_chunk"] = gpu_ms(fold, 20)
    out["fold_gb_per_s"] = out["fold_bytes_read"] / out["fold_ms_per_chunk"] / 1e6
    del r

    def streamed():
        return V.lean_frame_maps(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, products=heads, render_options=opts)

    def full_frame():
        res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=opts)
        w = res["weights_coarse"].unsqueeze(-1)
        return [torch.sum(w * res[h + "_coarse"], -2) for h in heads]
    out["lean_frame_maps_ms"] = gpu_ms(streamed, a.reps)
    out["lean_inference_plus_torch_ms"] = gpu_ms(full_frame, a.reps)
    out["lean_frame_maps_peak_growth_mb"] = peak_mb(streamed)
    out["lean_inference_plus_torch_peak_growth_mb"] = peak_mb(full_frame)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
