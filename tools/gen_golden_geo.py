#!/usr/bin/env python3
"""Write the fixtures of the world-cloud path: the REFERENCE's own stage outputs for a frame's rays and depth, and a small
synthetic DSM ground truth in the reference's on-disk layout.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_geo.py

1. tests/golden/geo_cloud_small.npz: the normalised rays of tests/golden/scene_small_ref.npz (the three test frames, then the
   second and third train frame: 5,107 rays; the first train frame IS the first test frame), a synthetic fp32 depth per ray (a
   smooth function of the pixel position between near and far), the normalisation parameters, and what the reference computes
   from them: get_xyz_from_nerf_prediction -> xyz_n, StandardNormalization.denormalize -> ecef, ecef_to_latlon_custom ->
   lat / lon / alt.  east / north are NOT the reference's (`utm` is an inert stub here): they are the numpy RESTATEMENT of the
   utm package's series in tests/utm_numpy.py, and labelled so ("east_restated", "north_restated").
   Condition: every point of that cloud lies at least EDGE_MARGIN = 1e-4 m from every edge of the 0.5 m DSM lattice in east and
   in north, so that a disagreement of 1e-6 m cannot move a point into another cell.  The depth of an offending ray is scaled
   by (1 + k 1e-5), k = 1, 2, ..., until it holds; the count of nudged rays is stored.
2. tests/golden/scene_small_dsm/: dsm/JAX_068_DSM.txt (xoff, yoff, size, resolution), dsm/JAX_068_DSM.tif (float32, georeferenced
   through the ModelPixelScale / ModelTiepoint tags, a few cells larger than the ROI on every side), dsm/JAX_068_CLS.tif (8-bit
   classes on the same raster, a few cells of class 9 = water), root.json (scene_small's plus "dsm_cls_fp") and expected.json.
   The ground truth is the numpy pipeline's own DSM of the cloud above (tests/dsm_numpy.py), moved by (dx, dy) = (2, -1) cells,
   plus a constant, plus smooth noise; cells the moved DSM leaves empty take a smooth surface.  expected.json holds the shift,
   b, mean and median the numpy pipeline finds on the ROI.  A test assembles the scene by copying tests/golden/scene_small and
   adding these files (scene_small itself must stay without a DSM).

Every file regenerates byte for byte."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
from PIL import Image, TiffImagePlugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
SCENE = os.path.join(OUT, "scene_small")
DSM_DIR = os.path.join(OUT, "scene_small_dsm")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsm_numpy  # noqa: E402
import utm_numpy  # noqa: E402

FRAMES = [("JAX_068_013_RGB", 41, 37), ("JAX_068_002_RGB", 31, 23), ("JAX_068_005_RGB", 25, 39), ("JAX_068_007_RGB", 33, 29),
          ("JAX_068_009_RGB", 27, 35)]
ZONE = 17
RES = 0.5
EDGE_MARGIN = 1e-4
ROI_SIDE = 104          # above 100 cells: recursive_ncc runs one pyramid level
SHIFT = (2, -1)
GT_CONST = 0.7
PAD = (3, 5, 4, 2)      # cells of the ground-truth raster beyond the ROI: west, north, east, south


def _scene_tool():
    spec = importlib.util.spec_from_file_location("gen_golden_scene", os.path.join(ROOT, "tools", "gen_golden_scene.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _depth(rays):
    """fp32 depth per ray: near + (far - near) * s, s a smooth function of the pixel position within [0.2, 0.8]"""
    out, lo = [], 0
    for k, (_, w, h) in enumerate(FRAMES):
        n = w * h
        i = np.arange(n)
        row, col = i // w, i % w
        s = 0.5 + 0.2 * np.sin(col / 6.0 + k) * np.cos(row / 5.0 - 0.5 * k) + 0.1 * (col / w - 0.5)
        near, far = rays[lo:lo + n, 6].astype(np.float64), rays[lo:lo + n, 7].astype(np.float64)
        out.append((near + (far - near) * s).astype(np.float32))
        lo += n
    assert lo == rays.shape[0]
    return np.concatenate(out)


def _reference_stages(rays, depth, norm_params):
    """the reference's own functions on CPU tensors, as its eval path chains them"""
    from baseline.components.normalization import StandardNormalization
    from baseline.dataset.satnerf_dataset import SatNeRFDataset
    from framework.util.conversions import ecef_to_latlon_custom
    xyz_n = SatNeRFDataset.get_xyz_from_nerf_prediction(None, torch.from_numpy(rays), torch.from_numpy(depth))
    norm = object.__new__(StandardNormalization)
    norm.norm_params = dict(zip(("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset"), norm_params.tolist()))
    ecef = norm.denormalize({"xyz": xyz_n}).data.numpy()
    lat, lon, alt = ecef_to_latlon_custom(ecef[:, 0], ecef[:, 1], ecef[:, 2])
    return xyz_n.numpy(), ecef, lat, lon, alt


def _edge_distance(v):
    f = np.mod(v / RES, 1.0)
    return np.minimum(f, 1.0 - f) * RES


def cloud_fixture():
    ref = np.load(os.path.join(OUT, "scene_small_ref.npz"))
    n_first = FRAMES[0][1] * FRAMES[0][2]
    rays = np.concatenate([ref["test_rays"], ref["train_rays"][n_first:]]).astype(np.float32)
    assert rays.shape == (sum(w * h for _, w, h in FRAMES), 8)
    depth = _depth(rays)
    base = depth.copy()
    nudged = np.zeros(depth.size, bool)
    for k in range(1, 200):
        xyz_n, ecef, lat, lon, alt = _reference_stages(rays, depth, ref["norm_params"])
        east, north = utm_numpy.from_latlon(lat, lon, ZONE)
        bad = (_edge_distance(east) < EDGE_MARGIN) | (_edge_distance(north) < EDGE_MARGIN)
        if not bad.any():
            break
        nudged |= bad
        depth[bad] = (base[bad].astype(np.float64) * (1.0 + 1e-5 * k)).astype(np.float32)
    else:
        raise RuntimeError("the edge-distance condition could not be met")
    out = {"rays": rays, "depth": depth, "norm_params": ref["norm_params"], "frame_names": np.array([f[0] for f in FRAMES]),
           "frame_w": np.array([f[1] for f in FRAMES], np.int64), "frame_h": np.array([f[2] for f in FRAMES], np.int64),
           "xyz_n": xyz_n, "ecef": ecef, "lat": lat, "lon": lon, "alt": alt, "east_restated": east, "north_restated": north,
           "zone": np.int64(ZONE), "zone_string": np.array("17R"), "edge_margin": np.float64(EDGE_MARGIN),
           "n_nudged": np.int64(nudged.sum())}
    np.savez_compressed(os.path.join(OUT, "geo_cloud_small.npz"), **out)
    return out


def _save_tagged(fp, a, mode, x0, y0):
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[33550] = (RES, RES, 0.0)
    ifd.tagtype[33550] = 12          # DOUBLE
    ifd[33922] = (0.0, 0.0, 0.0, float(x0), float(y0), 0.0)
    ifd.tagtype[33922] = 12
    Image.fromarray(a, mode).save(fp, compression=None, tiffinfo=ifd)


def dsm_fixture(c):
    cloud = np.stack([c["east_restated"], c["north_restated"], c["alt"]], 1)
    xoff, yoff, res, xsize, ysize = dsm_numpy.bounds_grid(cloud, RES)
    full = dsm_numpy.rasterize(cloud, xoff, yoff, res, xsize, ysize)[0].astype(np.float32)
    n = ROI_SIDE
    note = None
    if min(xsize, ysize) < n + 2 * 8:
        n = min(xsize, ysize) - 16
        note = f"the footprint ({xsize} x {ysize} cells) does not hold a {ROI_SIDE}-cell ROI: no pyramid level runs"
    i0, j0 = (xsize - n) // 2, (ysize - n) // 2              # the ROI window on the bounds lattice
    pw, pn, pe, ps = PAD
    h, w = n + pn + ps, n + pw + pe                          # the ground-truth raster
    dx, dy = SHIFT
    jj, ii = np.mgrid[0:h, 0:w]
    src = full[j0 - pn + dy: j0 - pn + dy + h, i0 - pw + dx: i0 - pw + dx + w]
    assert src.shape == (h, w)
    noise = 0.05 * np.sin(ii / 11.0) * np.cos(jj / 13.0)
    fill = 10.0 + 4.0 * np.sin(ii / 17.0 + 1.0) + 3.0 * np.cos(jj / 19.0)
    gt = np.where(np.isnan(src), fill, src.astype(np.float64) + GT_CONST + noise).astype(np.float32)
    cls = np.full((h, w), 2, np.uint8)
    cls[pn + 20: pn + 24, pw + 30: pw + 37] = 9              # water: 4 x 7 cells inside the ROI
    cls[pn + 70: pn + 72, pw + 5: pw + 8] = 9
    roi = np.array([xoff + i0 * res, yoff - (j0 + n) * res, n, res], np.float64)
    x0, y0 = xoff + (i0 - pw) * res, yoff - (j0 - pn) * res  # the outer corner of the raster's north-west pixel
    os.makedirs(os.path.join(DSM_DIR, "dsm"), exist_ok=True)
    np.savetxt(os.path.join(DSM_DIR, "dsm", "JAX_068_DSM.txt"), roi, fmt="%.17g")
    _save_tagged(os.path.join(DSM_DIR, "dsm", "JAX_068_DSM.tif"), gt, "F", x0, y0)
    _save_tagged(os.path.join(DSM_DIR, "dsm", "JAX_068_CLS.tif"), cls, "L", x0, y0)
    with open(os.path.join(SCENE, "root.json")) as f:
        root = json.load(f)
    root["dsm_cls_fp"] = "dsm/JAX_068_CLS.tif"
    with open(os.path.join(DSM_DIR, "root.json"), "w") as f:
        json.dump(root, f, indent=2)
    pred = full[j0:j0 + n, i0:i0 + n]
    gt_roi = gt[pn:pn + n, pw:pw + n]
    water = cls[pn:pn + n, pw:pw + n] == 9
    m = dsm_numpy.compute_mae(pred, gt_roi, mask=water)
    assert (m["dx"], m["dy"]) == SHIFT, (m["dx"], m["dy"])
    meta = {"roi_side": n, "roi": roi.tolist(), "raster_shape": [h, w], "raster_origin": [x0, y0], "pad_w_n_e_s": list(PAD),
            "bounds_grid": [xoff, yoff, res, xsize, ysize], "finite_fraction_of_pred": float(np.isfinite(pred).mean()),
            "water_cells": int(water.sum()), "dx": m["dx"], "dy": m["dy"], "b": m["b"], "mean": m["mean"], "median": m["median"],
            "trace": [list(t) for t in m["trace"]], "gt_const": GT_CONST, "note": note,
            "source": "tools/gen_golden_geo.py: the cloud of geo_cloud_small.npz (east / north from tests/utm_numpy.py) through "
                      "tests/dsm_numpy.py"}
    with open(os.path.join(DSM_DIR, "expected.json"), "w") as f:
        json.dump(meta, f, indent=2)
    return meta, pred, gt_roi, water, cloud, (xoff, yoff, res, xsize, ysize), (i0, j0, n)


def _quantised_check(cloud, grid, win, gt_roi, water, meta):
    """how far the device rasteriser's integer accumulation (round((z - Z0)/Q), Q = 2^-24, fp32 store) can move b, mean, median"""
    xoff, yoff, res, xsize, ysize = grid
    q = 2.0 ** -24
    zq = np.rint(cloud[:, 2] / q) * q
    full = dsm_numpy.rasterize(np.stack([cloud[:, 0], cloud[:, 1], zq], 1), xoff, yoff, res, xsize, ysize)[0].astype(np.float32)
    i0, j0, n = win
    m = dsm_numpy.compute_mae(full[j0:j0 + n, i0:i0 + n], gt_roi, mask=water)
    print("quantised rasteriser: shift", (m["dx"], m["dy"]), "rel b", abs(m["b"] - meta["b"]) / abs(meta["b"]),
          "rel mean", abs(m["mean"] - meta["mean"]) / meta["mean"], "rel median", abs(m["median"] - meta["median"]) / meta["median"])


def main():
    _scene_tool()._install_shims()
    c = cloud_fixture()
    print("points", c["rays"].shape[0], "nudged", int(c["n_nudged"]),
          "min edge distance", float(min(_edge_distance(c["east_restated"]).min(), _edge_distance(c["north_restated"]).min())))
    ke, kn = utm_numpy.kruger(c["lat"], c["lon"], ZONE)
    print("restatement vs Krueger on the fixture", float(max(np.abs(ke - c["east_restated"]).max(), np.abs(kn - c["north_restated"]).max())))
    meta, pred, gt_roi, water, cloud, grid, win = dsm_fixture(c)
    print({k: meta[k] for k in ("roi_side", "bounds_grid", "finite_fraction_of_pred", "dx", "dy", "b", "mean", "median", "trace", "note")})
    _quantised_check(cloud, grid, win, gt_roi, water, meta)
    for dp, _, files in sorted(os.walk(DSM_DIR)):
        for f in sorted(files):
            print(os.path.relpath(os.path.join(dp, f), ROOT), os.path.getsize(os.path.join(dp, f)))
    print("tests/golden/geo_cloud_small.npz", os.path.getsize(os.path.join(OUT, "geo_cloud_small.npz")))


if __name__ == "__main__":
    main()
