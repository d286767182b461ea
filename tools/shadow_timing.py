#!/usr/bin/env python3
"""What casting shadows costs: the wall time per call of eval/utils/shadow.py cast_shadows on a synthetic city
of boxes on a plane (res 0.5 m), at 512^2 and 1024^2 cells, K in {1, 8, 64} suns, all at elevation 10 or all at 45 degrees with the
azimuths spread over the circle, against

    torch    a torch restatement of the same march on the same GPU: fp64 tensors of K x H x W, one Python iteration per march step,
             ending when no ray is active (looked at every 16 steps) -- what the map product would run without the kernel

Kernel: the median over --reps windows of --inner back-to-back calls between two device events, after --warmup windows.  The torch leg
is slow by construction: --torch-reps single-call windows after one warm-up call, and only up to --torch-max-pairs (cell, sun) pairs;
beyond that its figure is null: not measured.  Each configuration also reports that the two legs gave equal masks.  z_top is the
city's largest altitude for both (cast_shadows' default, passed explicitly so that no host read falls into the window).
Prints one JSON line per configuration."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools._timing import window_ms  # noqa: E402
from snerf_amd.eval.utils import shadow as S  # noqa: E402

RES = 0.5


def city(n, seed=0):
    """(n, n) fp32: a plane at 2 m with n^2 / 4096 boxes of 8 .. 40 cells a side and 5 .. 60 m"""
    rng = np.random.default_rng(seed)
    d = np.full((n, n), 2.0, np.float32)
    for _ in range(n * n // 4096):
        i, j = rng.integers(0, n, 2)
        a, b = rng.integers(8, 41, 2)
        d[j:j + b, i:i + a] = np.float32(rng.uniform(5.0, 60.0))
    return d


def torch_cast(dsm, rows, bias, z_top):
    """the march of include/snerf_hip.h on K x H x W fp64 tensors: lit (K, H, W) u8"""
    dev = dsm.device
    h, w = dsm.shape
    K = len(rows)
    r = torch.from_numpy(np.asarray(rows, np.float64)).to(dev)
    ux, uy, rise = (r[:, c].reshape(K, 1, 1) for c in range(3))
    inf = torch.full_like(ux, math.inf)
    stepx, stepy = torch.where(ux > 0, 1, -1), torch.where(uy > 0, 1, -1)
    tdx, tdy = torch.where(ux == 0, inf, 1.0 / ux.abs()), torch.where(uy == 0, inf, 1.0 / uy.abs())
    d64 = dsm.double()
    flat = d64.reshape(-1)
    jj, ii = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    i, j = ii.expand(K, h, w).clone(), jj.expand(K, h, w).clone()
    tmx, tmy = (0.5 * tdx).expand(K, h, w).clone(), (0.5 * tdy).expand(K, h, w).clone()
    h0 = (d64 + bias).unsqueeze(0)
    hole = torch.isnan(d64).expand(K, h, w)
    lit = torch.where(hole, 255, 1).to(torch.uint8)
    active = ~hole
    for s in range(h + w + 2):
        if s % 16 == 0 and not bool(active.any()):
            break
        takex = tmx <= tmy
        t = torch.where(takex, tmx, tmy)
        i = torch.where(takex, i + stepx, i)
        j = torch.where(takex, j, j + stepy)
        tmx = torch.where(takex, tmx + tdx, tmx)
        tmy = torch.where(takex, tmy, tmy + tdy)
        inside = (i >= 0) & (i < w) & (j >= 0) & (j < h)
        hr = h0 + rise * t
        go = active & inside & ~(hr > z_top)
        cell = flat[j.clamp(0, h - 1) * w + i.clamp(0, w - 1)]
        blocked = go & (cell > hr)
        lit = torch.where(blocked, torch.zeros_like(lit), lit)
        active = go & ~blocked
    return lit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--suns", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--elevations", type=float, nargs="+", default=[10.0, 45.0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-max-pairs", type=int, default=1 << 24)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shadow_timing: needs a GPU (a time from anywhere else says nothing)")
    dev = torch.device("cuda:0")
    for n in a.sizes:
        host = city(n)
        dsm = torch.from_numpy(host).to(dev)
        z_top = float(host.max())
        for K in a.suns:
            for el in a.elevations:
                suns = [(el, 360.0 * k / K + 33.3) for k in range(K)]
                rows = S.sun_rows(suns, RES)
                call = lambda: S.cast_rows(dsm, rows, 0.0, z_top)      # noqa: E731
                for _ in range(a.warmup):
                    window_ms(call, a.inner)
                ms = [window_ms(call, a.inner) for _ in range(a.reps)]
                lit = call()
                out = {"cells": n * n, "suns": K, "elevation_deg": el, "shadowed_share": round(float((lit == 0).double().mean()), 4),
                       "kernel_ms": round(statistics.median(ms), 4), "kernel_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                       "torch_ms": None, "torch_over_kernel": None, "torch_equal": None}
                if n * n * K <= a.torch_max_pairs:
                    ref = torch_cast(dsm, rows, 0.0, z_top)             # the warm-up call
                    out["torch_equal"] = bool(torch.equal(ref, lit))
                    del ref
                    tms = [window_ms(lambda: torch_cast(dsm, rows, 0.0, z_top), 1) for _ in range(a.torch_reps)]
                    out["torch_ms"] = round(statistics.median(tms), 2)
                    out["torch_over_kernel"] = round(statistics.median(tms) / statistics.median(ms), 1)
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
