#!/usr/bin/env python3
"""Wall time of the streaming semantic evaluation (snerf_amd.eval.utils.semantic, csrc/semeval.hip) on one --size^2 frame at
--samples samples per ray: snerf_semeval_accumulate alone on the frame's labels, weights and beta (one call over the whole
frame), lean_semantic_eval (render + accumulate chunk by chunk + the one host read of image_entry), and the full-frame path it
replaces: lean_inference of the labels, weights and beta, then the torch statistics (bincount confusion matrix, error count,
composited beta at the car rays) and their host reads.  Medians of --reps synchronised runs after one warm-up run.  Also
prints the bytes the accumulate call reads (labels, targets, and the weights and beta of the car rays) and the peak
allocation growth of both frame paths.  Random-init model of the flagship width.  Prints one JSON line."""
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
from snerf_amd.eval.utils.semantic import SemanticEvalAccumulator, lean_semantic_eval  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=1 << 16)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C, car = 5, 4
    cfg = O.OracleCfg(n_samples=a.samples, render_chunk_size=a.chunk)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    n = a.size * a.size
    bank = O.batch_to_torch(O.synthetic_batch(4096, a.samples, seed=1))
    reps = -(-n // 4096)
    rays = bank["rays"].to(dev).repeat(reps, 1)[:n].contiguous()
    extras = bank["extras"].to(dev).repeat(reps, 1)[:n].contiguous()
    sem = bank["semantic"].to(torch.uint8).reshape(-1, 1).to(dev).repeat(reps, 1)[:n].contiguous()
    keys = ("semantic_label_coarse", "weights_coarse", "beta_coarse")
    opts = {"perturb": 0}

    res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=opts)
    lab, w, b = res["semantic_label_coarse"], res["weights_coarse"], res["beta_coarse"]
    cars = int((sem == car).sum())
    out = {"rays": n, "samples": a.samples, "chunk": a.chunk, "fc_units": cfg.fc_units, "car_rays": cars,
           "accumulate_bytes_read": n * (8 + 1) + cars * 2 * a.samples * 4}

    def accumulate():
        SemanticEvalAccumulator(C, car, dev).add(lab, sem, weights=w, beta=b)
    out["accumulate_ms"] = gpu_ms(accumulate, 20)

    def streamed():
        lean_semantic_eval(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, sem, car_cls_idx=car,
                           render_options=opts).image_entry()

    def full_frame():
        r = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=opts)
        p, g = r["semantic_label_coarse"], sem.reshape(-1).long()
        conf = torch.bincount(g * C + p, minlength=C * C).reshape(C, C)
        err = (g != p).sum()
        mask = g == car
        beta = torch.sum(r["weights_coarse"].unsqueeze(-1) * r["beta_coarse"], -2)[mask].sum() / mask.sum()
        conf.cpu(), err.item(), beta.item()
    del res, lab, w, b
    out["lean_semantic_eval_ms"] = gpu_ms(streamed, a.reps)
    out["lean_inference_plus_torch_ms"] = gpu_ms(full_frame, a.reps)
    out["lean_semantic_eval_peak_growth_mb"] = peak_mb(streamed)
    out["lean_inference_plus_torch_peak_growth_mb"] = peak_mb(full_frame)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
