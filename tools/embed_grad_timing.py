#!/usr/bin/env python3
"""What the embedding-only backward saves.

backward (default): at the bench model (W = 512, H = 256, L = 8, C = 5, use_tj_instead_of_beta so that the colour reads t) and
    4096 rays x 64 samples, in the default and the one-plane arithmetic, the device time and the profiled launch counts of

        full     snerf_backward of a main training pass with a gradient buffer (the backward a training step runs)
        flagged  snerf_backward under SNERF_FLAG_EMBED_GRAD with a NULL gradient buffer

    each after the same training forward, whose time is reported too (a fit step pays forward + flagged).  A window is --inner
    forward + backward pairs between device events with the forward's own windows subtracted; the legs alternate window by window,
    the figure is the median over --reps windows after warm-up windows.  --full-only: the leg that also runs on a library without
    the flag (a parent commit's build through SNERF_LIB_PATH).

fit: on tests/golden/scene_small with a model trained for --train-steps steps, per test view the wall time of one
    fit_image_embedding at --steps / --lr / --rays-per-fit, its loss curve, and the PSNR of the whole frame and of the held-out
    half under row 0, under the row the loader gives the view, and under the fitted vector.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from oracle import snerf_oracle as O  # noqa: E402
from snerf_amd import _lib, ops  # noqa: E402


def launches(fn):
    L = _lib.lib()
    _lib.check(L.snerf_profile_begin(), "snerf_profile_begin")
    fn()
    prof = _lib.SnerfProfile()
    _lib.check(L.snerf_profile_end(C.byref(prof)), "snerf_profile_end")
    return [int(prof.launches[i]) for i in range(4)]


def backward_timing(a):
    dev = torch.device("cuda:0")
    N, S = a.rays, a.samples
    cfg = O.OracleCfg(n_samples=S, use_tj_instead_of_beta=True)
    params = {k: torch.from_numpy(v).to(dev) for k, v in O.init_params_numpy(cfg, 1).items()}
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=5))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    t = torch.from_numpy(O.init_embedding_numpy(cfg, 1)).to(dev)[extras[:, 3].long()].contiguous()
    zs = torch.linspace(0, 1, S).to(dev)
    g_rgb = (torch.rand(N, 3, device=dev) * 2 - 1) / N
    have_flag = hasattr(_lib, "FLAG_EMBED_GRAD") and not a.full_only
    result = {"rays": N, "samples": S, "reps": a.reps, "inner": a.inner, "lib": os.environ.get("SNERF_LIB_PATH", "tree")}
    for mode in ("f16x2", "f16x1"):
        spec = ops.ModelSpec(mfma=mode, use_tj_instead_of_beta=True)
        packed = ops.pack_params(spec, params)
        pin = ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_steps=zs, u=u)
        d = spec.desc(N, S, _lib.FLAG_TRAIN)
        de = spec.desc(N, S, _lib.FLAG_TRAIN | _lib.FLAG_EMBED_GRAD) if have_flag else None
        ws = torch.empty(_lib.call_size("snerf_workspace_bytes", d), dtype=torch.uint8, device=dev)
        rgb = torch.empty(N, 3, device=dev)
        so = _lib.SnerfOutputs()
        so.rgb = rgb.data_ptr()
        si = pin.struct(t, None)
        go = _lib.SnerfOutGrads()
        go.rgb = g_rgb.data_ptr()
        pg = torch.zeros(_lib.call_size("snerf_grad_floats", d), device=dev)
        d_t = torch.empty_like(t)

        def fwd():
            _lib.call("snerf_forward", d, packed, si, so, ws, ws.numel())

        def full():
            fwd()
            _lib.call("snerf_backward", d, packed, si, go, pg, d_t, None, ws, ws.numel())

        def flagged():
            fwd()
            _lib.call("snerf_backward", de, packed, si, go, None, d_t, None, ws, ws.numel())

        legs = {"forward": fwd, "full": full}
        if have_flag:
            legs["flagged"] = flagged
        times = {k: [] for k in legs}
        for r in range(a.warmup + a.reps):
            for k, fn in legs.items():
                ms = window_ms(fn, a.inner)
                if r >= a.warmup:
                    times[k].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        entry = {"forward_ms": round(med["forward"], 4), "full_backward_ms": round(med["full"] - med["forward"], 4),
                 "full_spread_ms": round(max(times["full"]) - min(times["full"]), 4)}
        fwd()
        entry["full_launches"] = launches(lambda: _lib.call("snerf_backward", d, packed, si, go, pg, d_t, None, ws, ws.numel()))
        if have_flag:
            want = d_t.clone()
            entry["flagged_backward_ms"] = round(med["flagged"] - med["forward"], 4)
            entry["flagged_spread_ms"] = round(max(times["flagged"]) - min(times["flagged"]), 4)
            fwd()
            entry["flagged_launches"] = launches(lambda: _lib.call("snerf_backward", de, packed, si, go, None, d_t, None, ws, ws.numel()))
            entry["d_t_equal"] = bool(torch.equal(want, d_t))
            entry["fit_step_over_train_step"] = round(med["flagged"] / med["full"], 4)
        result[mode] = entry
    print(json.dumps(result))


def fit_timing(a):
    from snerf_amd.eval.utils import metrics
    from snerf_amd.eval.utils.embedding import fit_image_embedding, region_mask
    from snerf_amd.eval.utils.util import lean_inference
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import TrainLoop, load_pipeline
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    scene = os.path.join(ROOT, "tests", "golden", "scene_small")
    c = MainConfig(run={"max_train_steps": a.train_steps, "dataset_dp": scene, "cache_dp": a.cache, "dataset_name": "scene_small"},
                   pipeline={"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": a.width, "n_samples": 32,
                             "batch_size": 256, "depth_enabled": False, "first_beta_epoch": 0, "sparsity_n_images": 2,
                             "use_tj_instead_of_beta": True, "render_chunk_size": 1 << 20})
    pipe = load_pipeline(c)
    loop = TrainLoop(pipe, c, dev)
    for step in range(a.train_steps):
        loop.step(step)
    torch.cuda.synchronize()
    n_train = len(pipe.datasets["rgb"].metas) if hasattr(pipe.datasets["rgb"], "metas") else None
    out = {"train_steps": a.train_steps, "steps": a.steps, "lr": a.lr, "rays_per_fit": a.rays_per_fit, "views": {}}
    opts = {"perturb": 0}
    for im in pipe.datasets["rgb_test"].scene_images()[1:]:
        rays, extras = (im[k].reshape(-1, im[k].shape[-1]) for k in ("rays", "extras"))
        rgbs = im["rgbs"].reshape(-1, 3)
        mask = region_mask(im["w"], im["h"], "left")
        held = ~mask.to(dev)
        kw = dict(fit_mask=mask, steps=a.steps, lr=a.lr, rays_per_fit=a.rays_per_fit, n_train=n_train)
        fit_image_embedding(c, pipe.renderer, pipe.models, rays, extras, rgbs, **dict(kw, steps=2))      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = fit_image_embedding(c, pipe.renderer, pipe.models, rays, extras, rgbs, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0

        def psnrs(ro, ex=extras):
            rgb = lean_inference(c, pipe.renderer, pipe.models, rays, ex, keys=("rgb_coarse",), render_options=dict(opts, **ro))["rgb_coarse"]
            return [round(float(metrics.psnr(rgb, rgbs)), 3), round(float(metrics.psnr(rgb, rgbs, valid_mask=held)), 3)]

        row0 = extras.clone()
        row0[:, 3] = 0
        out["views"][im["name"]] = {
            "rays": int(rays.shape[0]), "fit_rays": fit["rays"], "fit_wall_s": round(wall, 4), "best_step": fit["best_step"],
            "loss": [round(v, 6) for v in fit["loss"][::max(1, a.steps // 20)]] + [round(fit["loss"][-1], 6)],
            "loader_row": int(extras[0, 3]), "psnr_frame_heldout_row0": psnrs({}, row0), "psnr_frame_heldout_loader_row": psnrs({}),
            "psnr_frame_heldout_fitted": psnrs({"t_vector": fit["t"]})}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="backward", choices=("backward", "fit"))
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full-only", action="store_true")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--rays-per-fit", type=int, default=4096)
    ap.add_argument("--cache", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_grad_timing.py measures on the GPU: none found")
    (backward_timing if a.what == "backward" else fit_timing)(a)


if __name__ == "__main__":
    main()
