#!/usr/bin/env python3
"""Generate the golden vectors of the DSM registration and altitude MAE by running the REFERENCE's own registration code.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_dsm.py

It loads eval/utils/dsmr.py of the reference (read-only) with two stub modules: `numba` (jit = the identity decorator, so the
loops run as plain Python) and `rasterio` (only its file helpers use it; they are not called).  The arrays are fed as float64,
which is the arithmetic numba applies to the float32 DSMs (every accumulator starts as an int and is promoted to float64);
`mean_std` is wrapped to return Python floats, so that `ncc` meets the ZeroDivisionError of a zero variance exactly as the
numba-compiled function makes it.  The lines of eval/utils/dsm.py:compute_mae that need gdal / rasterio are restated below
with their line numbers.  Writes tests/golden/dsmr_*.npz (inputs, every pyramid level, the shift found at every level,
muu / muv / b, the registered DSM, the difference, mean and median).
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True


def load_dsmr():
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (lambda f: f)
    sys.modules["numba"] = numba
    sys.modules["rasterio"] = types.ModuleType("rasterio")
    spec = importlib.util.spec_from_file_location("ref_dsmr", os.path.join(REF, "eval", "utils", "dsmr.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    raw_mean_std = m.mean_std
    m.mean_std = lambda u, v, dx=0, dy=0: tuple(float(x) for x in raw_mean_std(u, v, dx, dy))
    return m


D = load_dsmr()


def run_reference(gt, pred, mask=None, init=(0, 0)):
    """compute_mae (eval/utils/dsm.py:160-266) on arrays; registration on the raw cropped gt as the reference reads it"""
    levels, shifts = [], []
    raw_ds, raw_cn = D.downsample2x, D.compute_ncc

    def ds(u):
        out = raw_ds(u)
        levels.append(out[0].copy())
        return out

    def cn(u, v, irange, initdx, initdy):
        dx, dy = raw_cn(u, v, irange, initdx, initdy)
        shifts.append((u.shape[-2], u.shape[-1], initdx, initdy, dx, dy))
        return dx, dy

    D.downsample2x, D.compute_ncc = ds, cn
    try:
        pred_m = pred.copy()
        if mask is not None:
            pred_m[mask.astype(bool)] = np.nan                       # dsm.py:218-224
        u = gt.astype(np.float64)[None]                               # compute_shift reads tmp_gt_path: the raw crop (:236)
        v = pred_m.astype(np.float64)[None]
        dx, dy = D.recursive_ncc(u, v, 5, init[0], init[1])           # dsmr.py:269 (recursive_ncc(u, v) with an init)
        muu, muv, sigu, sigv, xcorr = D.mean_std(u, v, dx, dy)        # dsmr.py:271
        a, b = 1, muu - muv                                           # dsmr.py:273-274, scaling=False
        out = np.zeros(v.shape, dtype=np.float32)
        rdsm = D.apply_shift_(v, out, dx, dy, a, b, 0, 0)[0]          # dsmr.py:298 (apply_shift, c = d = 0)
        gt_dsm = gt.copy()
        gt_dsm[gt_dsm < -500.0] = 0.0                                 # dsm.py:229-231
        diff = rdsm - gt_dsm                                          # dsm.py:241
        mean = np.nanmean(abs(diff.ravel()))                          # dsm.py:263-266 (the reference formats these)
        median = np.nanmedian(abs(diff.ravel()))
    finally:
        D.downsample2x, D.compute_ncc = raw_ds, raw_cn
    # recursion: the downsample2x calls go u, v per level from fine to coarse; compute_ncc returns coarse to fine
    res = {"gt": gt, "pred": pred, "v": pred_m, "init": np.array(init, np.int64), "dx": np.int64(dx), "dy": np.int64(dy),
           "shifts": np.array(shifts, np.int64), "muu": np.float64(muu), "muv": np.float64(muv), "b": np.float64(b),
           "rdsm": rdsm, "diff": diff, "mean": np.float64(mean), "median": np.float64(median),
           "n_levels": np.int64(len(levels) // 2)}
    for k in range(len(levels) // 2):
        res[f"ds_u_{k + 1}"] = levels[2 * k]
        res[f"ds_v_{k + 1}"] = levels[2 * k + 1]
    if mask is not None:
        res["mask"] = mask
    return res


def terrain(rng, h, w, pad=24):
    """smooth ground + a few rectangular buildings, float64, (h + 2 pad, w + 2 pad)"""
    H, W = h + 2 * pad, w + 2 * pad
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = 300.0 + 4.0 * np.sin(x / 17.0) + 3.0 * np.cos(y / 13.0) + 0.02 * x
    for _ in range(max(4, h * w // 900)):
        j, i = rng.integers(0, H - 8), rng.integers(0, W - 8)
        f[j:j + rng.integers(3, 9), i:i + rng.integers(3, 9)] += rng.uniform(4.0, 20.0)
    return f, pad


def pair(rng, h, w, dx, dy, bias, noise=0.1):
    """gt (h, w) and a prediction with pred[j + dy, i + dx] = gt[j, i] + bias + noise (both float32)"""
    f, p = terrain(rng, h, w)
    gt = f[p:p + h, p:p + w]
    pred = f[p - dy:p - dy + h, p - dx:p - dx + w] + bias + rng.normal(0.0, noise, (h, w))
    return gt.astype(np.float32), pred.astype(np.float32)


def cases():
    rng = np.random.default_rng(20261015)
    out = {}
    gt, pred = pair(rng, 64, 64, 2, -3, 1.5)
    out["dsmr_64"] = run_reference(gt, pred)
    gt, pred = pair(rng, 130, 150, 3, 4, -0.75)
    out["dsmr_130x150"] = run_reference(gt, pred)
    gt, pred = pair(rng, 203, 101, -2, 1, 0.3)
    out["dsmr_odd"] = run_reference(gt, pred)
    # true shift (-7, +9): beyond the +-5 window of the finest level, found through the coarse one; the search starts at (-3, 5),
    # halved to (-2, 2) by floor division on the way down
    gt, pred = pair(rng, 130, 150, -7, 9, 2.0)
    out["dsmr_shift"] = run_reference(gt, pred, init=(-3, 5))
    # NaN holes in the prediction and a water mask (class 9) applied before registration
    gt, pred = pair(rng, 96, 112, 1, 2, 0.5)
    pred[rng.random(pred.shape) < 0.08] = np.nan
    pred[40:52, 10:30] = np.nan
    water = np.zeros(gt.shape, np.uint8)
    water[60:80, 70:100] = 9
    water[5:9, 5:9] = 6
    out["dsmr_holes_water"] = run_reference(gt, pred, mask=(water == 9).astype(np.uint8))
    out["dsmr_holes_water"]["water"] = water
    # ground truth with no-data values below -500 (zeroed for the difference, raw in the registration)
    gt, pred = pair(rng, 72, 80, -1, 1, 0.0)
    gt[10:14, 20:25] = -9999.0
    out["dsmr_gt_low"] = run_reference(gt, pred)
    # flat gt except its last three columns: every shift with dx >= 3 sees a constant gt (zero variance, NCC 0)
    gt = np.full((64, 64), 10.0, np.float32)
    gt[:, 61:] = rng.uniform(0.0, 5.0, (64, 3)).astype(np.float32) + 10.0
    pred = (rng.uniform(0.0, 5.0, (64, 64)) + 12.0).astype(np.float32)
    pred[:, 61:] = gt[:, 61:] + 2.0
    out["dsmr_flat"] = run_reference(gt, pred)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, res in cases().items():
        np.savez(os.path.join(OUT, name + ".npz"), **res)
        print(f"{name}: {res['gt'].shape} levels {int(res['n_levels'])} shifts {res['shifts'].tolist()} "
              f"b {float(res['b']):.6f} mean {float(res['mean']):.6f} median {float(res['median']):.6f}")


if __name__ == "__main__":
    main()
