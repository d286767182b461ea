#!/usr/bin/env python3
"""What a normals pass costs.

At the bench model (W = 512, H = 256, L = 8, skip at 4, F = 10, C = 5) and --rays x --samples (default 4096 x 64), default arithmetic,
the device time of

    inference      snerf_forward of an inference main pass asked for rgb, depth and weights (what a frame render pays per chunk)
    geometry       snerf_forward under SNERF_FLAG_GEOMETRY asked for depth and weights: trunk, sigma and the composite, no head launch
    train_forward  snerf_forward under SNERF_FLAG_TRAIN asked for depth and weights (the forward a normals pass runs: it keeps the
                   activations -- and runs the head launches the pass does not need, which is measured here, not removed)
    normals        train_forward + snerf_density_grad with coef = the pass's weights (the normals pass)
    train_step     train_forward + snerf_backward with a gradient buffer (the backward a training step runs)

A window is --inner calls between device events; the legs alternate window by window, the figure is the median over --reps windows
after --warmup windows.  The share of snerf_density_grad spent in the kernels of csrc/normals.hip comes from torch.profiler's kernel
table over --inner calls (null when the profiler reports no kernel).  Prints one JSON line."""
import argparse
import ctypes as C
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

NEW_KERNELS = ("encgrad_kernel", "encgrad_weights_kernel", "ray_fold3_kernel")


def kernel_share(fn, inner):
    """{kernel name fragment: device microseconds per call} of NEW_KERNELS and "all" over `inner` calls of fn, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
        rows = [(e.key, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))) for e in prof.key_averages()]
    except Exception as exc:      # a profiler that cannot trace here: the figure is reported as missing, the timings stand
        return {"error": f"{type(exc).__name__}: {exc}"}
    total = sum(us for _, us in rows)
    if total <= 0:
        return None
    out = {k: round(sum(us for name, us in rows if k in name) / inner, 2) for k in NEW_KERNELS}
    out["all"] = round(total / inner, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normals_timing.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    N, S = a.rays, a.samples
    cfg = O.OracleCfg(n_samples=S)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()].contiguous()
    spec = ops.ModelSpec()
    packed = ops.pack_params(spec, params)
    pin = ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_steps=torch.linspace(0, 1, S).to(dev), u=u)
    si = pin.struct(t, None)
    d_inf, d_tr, d_geo = spec.desc(N, S, 0), spec.desc(N, S, _lib.FLAG_TRAIN), spec.desc(N, S, _lib.FLAG_GEOMETRY)
    ws_inf = torch.empty(_lib.call_size("snerf_workspace_bytes", d_inf), dtype=torch.uint8, device=dev)
    ws = torch.empty(_lib.call_size("snerf_workspace_bytes", d_tr), dtype=torch.uint8, device=dev)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().snerf_normals_scratch_bytes(C.byref(d_tr), C.byref(n)), "snerf_normals_scratch_bytes")
    scratch = torch.empty(n.value, dtype=torch.uint8, device=dev)
    rgb, depth, weights = torch.empty(N, 3, device=dev), torch.empty(N, device=dev), torch.empty(N, S, device=dev)
    so_inf, so_tr = _lib.SnerfOutputs(), _lib.SnerfOutputs()
    so_inf.rgb, so_inf.depth, so_inf.weights = rgb.data_ptr(), depth.data_ptr(), weights.data_ptr()
    so_tr.depth, so_tr.weights = depth.data_ptr(), weights.data_ptr()
    grad = torch.empty(N, 3, dtype=torch.float64, device=dev)
    go = _lib.SnerfOutGrads()
    g_w = (torch.rand(N, S, device=dev) * 2 - 1) / N
    go.weights = g_w.data_ptr()
    pg = torch.zeros(_lib.call_size("snerf_grad_floats", d_tr), device=dev)
    d_t = torch.empty_like(t)

    def inference():
        _lib.call("snerf_forward", d_inf, packed, si, so_inf, ws_inf, ws_inf.numel())

    def geometry():
        _lib.call("snerf_forward", d_geo, packed, si, so_tr, ws_inf, ws_inf.numel())

    def train_forward():
        _lib.call("snerf_forward", d_tr, packed, si, so_tr, ws, ws.numel())

    def density_grad():
        _lib.call("snerf_density_grad", d_tr, packed, si, weights, grad, None, ws, scratch)

    def normals():
        train_forward()
        density_grad()

    def train_step():
        train_forward()
        _lib.call("snerf_backward", d_tr, packed, si, go, pg, d_t, None, ws, ws.numel())

    legs = {"inference": inference, "geometry": geometry, "train_forward": train_forward, "normals": normals, "train_step": train_step}
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            ms = window_ms(fn, a.inner)
            if r >= a.warmup:
                times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    train_forward()
    share = kernel_share(density_grad, a.inner)
    out = {"rays": N, "samples": S, "reps": a.reps, "inner": a.inner, "scratch_bytes": n.value,
           "inference_ms": round(med["inference"], 4), "geometry_ms": round(med["geometry"], 4), "train_forward_ms": round(med["train_forward"], 4),
           "normals_pass_ms": round(med["normals"], 4), "density_grad_ms": round(med["normals"] - med["train_forward"], 4),
           "train_backward_ms": round(med["train_step"] - med["train_forward"], 4),
           "normals_over_inference": round(med["normals"] / med["inference"], 3),
           "spread_ms": {k: round(max(v) - min(v), 4) for k, v in times.items()},
           "density_grad_kernels_us": share, "grad_finite": bool(torch.isfinite(grad).all())}
    if isinstance(share, dict) and share.get("all"):
        out["new_kernels_share_of_density_grad"] = round(sum(share[k] for k in NEW_KERNELS) / share["all"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
