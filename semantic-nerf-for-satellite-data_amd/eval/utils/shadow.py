"""Cast shadows on the map: the shadow a DSM casts under a sun, and how far a model's learned shadow maps agree with it -- the
question the S-NeRF / Sat-NeRF irradiance model raises (do the learned shadows follow from the learned geometry?) as a number.
The reference has no counterpart; the spec is include/snerf_hip.h, the stages are the kernels of
csrc/shadow.hip, torch is plumbing.  All functions take and return device tensors; there is no CPU fallback.

cast_shadows marches, per cell and sun, from the cell towards the sun over the height field (an Amanatides-Woo walk in cell
units, fp64): 0 = shadowed, 1 = lit, 255 = the cell itself is a hole.  The sun's direction follows rays.construct_sun_dir
(azimuth clockwise from north, elevation above the horizon); every transcendental is evaluated here on the host, in numpy fp64.

shadow_agreement counts, per sun, the cells of a learned shadow map (`sun` of nadir_sun_sweep: 1 = lit) against a cast mask:
a 2 x 2 table, the cells left out and the quantised sums of the learned value over the lit and the shadowed cells -- integer words
(order-, chunking- and rank-independent); accuracy, the IoU of the shadow class and the two means are derived from them here.

shadow_check runs both on the products of nadir_sun_sweep: against the model's own DSM (self-consistency) and, with `gt`, against
the lidar DSM.  eval/ortho.py export_shadow_check writes the masks and the figures.

`bias` (metres) lifts the start of every march: 0.0 is the exact-spec value, and on a noisy learned DSM a cell's own neighbours
rise above it by the noise and shadow it at low suns.  What bias a learned DSM needs is UNMEASURED; it stays a parameter.

The suns of a date and place come from eval/utils/solar.py sun_position, whose (elevation, azimuth) pairs are a `suns` list; a year
of suns is cheaper through that module's horizon planes than through one march per sun.
Out of scope: soft shadows and penumbrae, sub-cell interpolation of the height field, a max-mip acceleration.  The occlusion of a satellite's view direction is cast_rows under a view row (eval/utils/orthorect.py visibility)."""
import ctypes as C
import math

import numpy as np
import torch

from ... import _lib

MAX_SUNS = _lib.SHADOW_MAX_SUNS
UNKNOWN = _lib.SHADOW_UNKNOWN
GT_HOLE_BELOW = -500.0     # a lidar DSM's no-data altitudes (the reference's dsm.py:229-231 tests the same bound)
METRICS = ("n", "left_out", "accuracy", "iou_shadow", "mean_sun_lit", "mean_sun_shadow")


def sun_rows(suns, res):
    """(elevation_deg, azimuth_deg) pairs -> the (K, 3) fp64 rows (ux, uy, rise) of snerf_shadow_cast: ux = sin(az) (east = +column),
    uy = -cos(az) (north = -row), rise = tan(el) * res metres per cell of horizontal travel; numpy fp64, the convention of
    rays.construct_sun_dir.  Elevation must lie in (0, 90].  Any K: cast_shadows cuts lists longer than 64 into calls."""
    pairs = np.asarray([(float(el), float(az)) for el, az in suns], np.float64).reshape(-1, 2)
    if not len(pairs):
        raise ValueError("sun_rows: no sun")
    if not (np.isfinite(pairs).all() and (pairs[:, 0] > 0.0).all() and (pairs[:, 0] <= 90.0).all()):
        raise ValueError("sun_rows: every sun needs a finite azimuth and an elevation in (0, 90] degrees")
    res = float(res)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"sun_rows: res = {res} must be positive and finite")
    el, az = np.deg2rad(pairs).T
    return np.stack([np.sin(az), -np.cos(az), np.tan(el) * res], 1)


def _dsm(dsm, who):
    if not (torch.is_tensor(dsm) and dsm.is_cuda):
        raise ValueError(f"{who}: the DSM must be a GPU tensor (the HIP path has no CPU fallback)")
    if dsm.dim() != 2 or dsm.dtype != torch.float32 or not dsm.numel():
        raise ValueError(f"{who}: the DSM must be a non-empty (H, W) float32 tensor, not {tuple(dsm.shape)} of {dsm.dtype}")
    return dsm.contiguous()


def cast_rows(dsm, rows, bias=0.0, z_top=None, want_dist=False):
    """cast_shadows on ready-made (K, 3) fp64 rows (ux, uy, rise), K >= 1: one snerf_shadow_cast per 64 rows"""
    dsm = _dsm(dsm, "cast_shadows")
    rows = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(-1, 3))
    K = len(rows)
    if not K:
        raise ValueError("cast_shadows: no sun")
    h, w = dsm.shape
    if z_top is None:      # the largest finite altitude (-inf for a DSM without one: every march then ends at its first step)
        z_top = float(torch.where(torch.isfinite(dsm), dsm, torch.full_like(dsm, -math.inf)).max())
    lit = torch.empty((K, h, w), dtype=torch.uint8, device=dsm.device)
    dist = torch.empty((K, h, w), dtype=torch.float32, device=dsm.device) if want_dist else None
    for k in range(0, K, MAX_SUNS):
        part = np.ascontiguousarray(rows[k:k + MAX_SUNS])
        _lib.call("snerf_shadow_cast", dsm, h, w, part.ctypes.data_as(C.c_void_p), len(part), bias, z_top, lit[k:k + len(part)],
                  dist[k:k + len(part)] if want_dist else None, exc=ValueError)
    return (lit, dist) if want_dist else lit


def cast_shadows(dsm, suns, res, bias=0.0, z_top=None, want_dist=False):
    """The shadows `dsm` ((H, W) f32 on the GPU, row 0 = the north edge, NaN = a hole) casts under `suns` ((elevation_deg,
    azimuth_deg) pairs) at `res` metres per cell: lit (K, H, W) u8 -- 0 shadowed, 1 lit, 255 where the cell itself is NaN -- and,
    with `want_dist`, (lit, dist): dist (K, H, W) f32, the horizontal distance to the blocking cell in cells (NaN where lit or
    unknown).  `bias` (metres) is added to the start altitude of every march.  `z_top` ends a march once the ray is above it;
    None takes the largest finite altitude of the DSM (one host read), and any value at or above that gives the same bits."""
    return cast_rows(dsm, sun_rows(suns, res), bias, z_top, want_dist)


def agreement_words(sun_maps, lit, valid=None, threshold=0.5, acc=None):
    """snerf_shadow_agreement on (K, ...) maps: the (K, 8) int64 tensor holding the u64 words, added to `acc` when given (the
    parts of a map, or the maps of several ranks, accumulate into one)"""
    if not (torch.is_tensor(sun_maps) and sun_maps.is_cuda and torch.is_tensor(lit) and lit.is_cuda):
        raise ValueError("shadow_agreement: the maps must be GPU tensors (the HIP path has no CPU fallback)")
    if sun_maps.dtype != torch.float32 or lit.dtype != torch.uint8 or sun_maps.dim() < 2 or sun_maps.shape != lit.shape or not lit.numel():
        raise ValueError(f"shadow_agreement: a (K, ...) float32 shadow map and a uint8 mask of the same shape expected, got "
                         f"{tuple(sun_maps.shape)} of {sun_maps.dtype} and {tuple(lit.shape)} of {lit.dtype}")
    K = sun_maps.shape[0]
    cells = sun_maps[0].numel()
    if valid is not None:
        if not (torch.is_tensor(valid) and valid.is_cuda) or valid.numel() != cells:
            raise ValueError(f"shadow_agreement: valid must be a GPU tensor of {cells} cells")
        valid = valid.reshape(-1).ne(0).to(torch.uint8)
    if acc is None:
        acc = torch.zeros((K, 8), dtype=torch.int64, device=sun_maps.device)
    if acc.dtype != torch.int64 or tuple(acc.shape) != (K, 8) or not acc.is_contiguous():
        raise ValueError(f"shadow_agreement: acc must be a contiguous ({K}, 8) int64 tensor")
    s, m = sun_maps.contiguous().reshape(K, cells), lit.contiguous().reshape(K, cells)
    for k in range(0, K, MAX_SUNS):
        n = min(MAX_SUNS, K - k)
        _lib.call("snerf_shadow_agreement", s[k:k + n], m[k:k + n], valid, cells, n, threshold, acc[k:k + n], exc=ValueError)
    return acc


def _div(a, b):
    return a / b if b else math.nan


def agreement_metrics(words):
    """one sun's 8 words (Python ints, the u64 values or their int64 views) -> {"n", "left_out", "accuracy", "iou_shadow",
    "mean_sun_lit", "mean_sun_shadow", "words"}; an empty denominator gives NaN"""
    w = [int(v) % 2 ** 64 for v in words]
    s_lit, s_shadow = ((v - 2 ** 64 if v >= 2 ** 63 else v) for v in w[5:7])
    n = sum(w[:4])
    return {"n": n, "left_out": w[4], "accuracy": _div(w[0] + w[3], n), "iou_shadow": _div(w[3], w[1] + w[2] + w[3]),
            "mean_sun_lit": _div(s_lit / 2.0 ** 24, w[0] + w[1]), "mean_sun_shadow": _div(s_shadow / 2.0 ** 24, w[2] + w[3]),
            "words": w}


def shadow_agreement(sun_maps, lit, valid=None, threshold=0.5):
    """K learned shadow maps `sun_maps` ((K, H, W) f32, 1 = lit) against K cast masks `lit` ((K, H, W) u8 of cast_shadows): a cell
    is predicted lit when its value >= `threshold`; cells with lit == 255, with `valid` ((H, W), 0 = leave out) zero or with a value
    that is not finite are left out.  Returns one dict per sun: "n" (cells counted), "left_out", "accuracy", "iou_shadow" (of the
    shadow class: both shadow / either shadow), "mean_sun_lit" / "mean_sun_shadow" (the mean learned value over the cast-lit /
    cast-shadowed cells, from sums quantised to 2^-24) and "words", the 8 raw u64 words of include/snerf_hip.h.  Derived on the
    host from the integer words; an empty denominator gives NaN."""
    return [agreement_metrics(row) for row in agreement_words(sun_maps, lit, valid, threshold).cpu().tolist()]


@torch.no_grad()
def shadow_check(products, gt=None, water_mask=None, ignore_mask=None, bias=0.0, threshold=0.5):
    """The shadow-consistency check of a sun sweep.  `products`: what ortho.nadir_sun_sweep returns ("dsm" (H, W), "sun" (K, H, W),
    "suns", "grid").  The model's own DSM is cast under products["suns"] and compared with the learned shadow maps; with `gt`
    ((H, W), the lidar DSM on the same lattice; altitudes below -500 count as holes) the lidar DSM is cast too.  `water_mask` /
    `ignore_mask` leave out the cells dsm.compute_mae leaves out (water_mask == 9, ignore_mask != 0), in both comparisons.

    Returns {"suns", "cast_model": (K, H, W) u8, "agreement_model": [per sun, see shadow_agreement][, "cast_gt", "agreement_gt"],
    "disagree": (K, H, W) u8 -- 1 where the thresholded learned map and cast_model differ, 0 where they agree, 255 where the cell
    is left out}."""
    dsm, sun, suns = products["dsm"], products["sun"], products["suns"]
    res = float(products["grid"].resolution)
    if sun.dim() != 3 or tuple(sun.shape[1:]) != tuple(dsm.shape) or sun.shape[0] != len(suns):
        raise ValueError(f"shadow_check: {len(suns)} suns, shadow maps {tuple(sun.shape)} and a DSM {tuple(dsm.shape)} do not belong together")
    dev = dsm.device
    valid = None
    if water_mask is not None or ignore_mask is not None:
        valid = torch.ones(dsm.shape, dtype=torch.bool, device=dev)
        if water_mask is not None:
            valid &= water_mask.to(dev).reshape(dsm.shape) != 9
        if ignore_mask is not None:
            valid &= ignore_mask.to(dev).reshape(dsm.shape) == 0
    out = {"suns": list(suns), "cast_model": cast_shadows(dsm, suns, res, bias)}
    out["agreement_model"] = shadow_agreement(sun, out["cast_model"], valid, threshold)
    if gt is not None:
        g = gt.to(dev).float()
        if g.shape != dsm.shape:
            raise ValueError(f"shadow_check: the ground truth {tuple(g.shape)} is not on the DSM's lattice {tuple(dsm.shape)}")
        g = torch.where(g < GT_HOLE_BELOW, torch.full_like(g, math.nan), g)
        out["cast_gt"] = cast_shadows(g, suns, res, bias)
        out["agreement_gt"] = shadow_agreement(sun, out["cast_gt"], valid, threshold)
    cast = out["cast_model"]
    left = (cast > 1) | ~torch.isfinite(sun)
    if valid is not None:
        left |= ~valid
    differ = (sun.double() >= float(threshold)) != (cast == 1)      # the kernel compares in fp64
    out["disagree"] = torch.where(left, torch.full_like(cast, UNKNOWN), differ.to(torch.uint8))
    return out
