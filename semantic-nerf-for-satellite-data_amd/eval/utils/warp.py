"""Rasters from one map lattice onto another -- any resolution, any offset -- on the device: what holds a lidar DSM at 1 m (or at
0.5 m with its corner half a cell off) against a 0.5 m map, a model exported at 0.25 m against the rectified ground truth at 0.5 m, or
two exports at different resolutions against each other.  The reference does this implicitly through GDAL (gdal.Translate / gdalwarp);
neither GDAL nor rasterio is part of this build, so parity with their resampling is UNPINNED.  The spec is include/snerf_warp.h
(DESIGN.md section 5zd), the kernels are csrc/warp.hip, torch is plumbing.  Both lattices are north-up and axis-parallel.

  Lattice         (x0, y0, sx, sy, w, h): the outer corner of the north-west cell, the cell size east / south, the cell counts;
  lattice_of      a DsmGrid, a window _lib.SnerfDsmGrid or a geotransform (x0, y0, sx, sy) with a shape -> Lattice;
  warp_map        the destination lattice in the source's cell coordinates (a _lib.SnerfWarpMap), snapped as crop_to_roi snaps;
  same_lattice    two lattices with the same corner, cell size and shape (to the same tolerances);
  warp            float planes (nearest, bilinear, average, min, max) and label planes (nearest, mode); a raster that only shifts by
                  whole cells is sliced and padded, no launch, and keeps its bits;
  warp_products   every plane of a products dict onto another lattice;
  mae_between     a prediction on one lattice against a ground truth on another: dsm.compute_mae on the ground truth's lattice.

Everything is fixed operation by operation in fp64 and the only atomics are integer: the planes are bit-reproducible, bit for bit
the numpy restatement of tests/warp_numpy.py.  Out of scope: cubic and Lanczos kernels, rotated or sheared geotransforms and
reprojection between UTM zones, area-weighted label votes, rank-sharded rasters."""
import math
from collections import namedtuple

import torch

from ... import _lib
from . import dsm as D

NEAREST, BILINEAR, AVERAGE, MIN, MAX, MODE = (_lib.WARP_NEAREST, _lib.WARP_BILINEAR, _lib.WARP_AVERAGE, _lib.WARP_MIN, _lib.WARP_MAX,
                                              _lib.WARP_MODE)
MAX_STEP = _lib.WARP_MAX_STEP
MAX_PLANES = _lib.WARP_MAX_PLANES
NO_LABEL = _lib.ORTHO_NO_LABEL
METHODS = {"nearest": NEAREST, "bilinear": BILINEAR, "average": AVERAGE, "min": MIN, "max": MAX, "mode": MODE}
FLOAT_METHODS = ("nearest", "bilinear", "average", "min", "max")
LABEL_METHODS = ("nearest", "mode")
STEP_TOLERANCE = 1e-9       # relative: a step this close to 1 is 1 (crop_to_roi's resolution test)
OFFSET_TOLERANCE = 1e-6     # cells: at step 1, an offset this close to an integer is that integer (crop_to_roi's corner test)

Lattice = namedtuple("Lattice", "x0 y0 sx sy w h")


def lattice_of(grid, shape=None):
    """a Lattice from a DsmGrid, a window _lib.SnerfDsmGrid (through ortho.window_grid), a Lattice, or a geotransform
    (x0, y0, sx, sy) as img_utils.load_dsm_geotiff returns it; `shape` = (h, w) is required with a geotransform and checked against
    a grid"""
    if isinstance(grid, Lattice):
        lat = grid
    elif isinstance(grid, (D.DsmGrid, _lib.SnerfDsmGrid)):
        from .ortho import window_grid
        g = window_grid(grid)
        lat = Lattice(float(g.xoff), float(g.yoff), float(g.resolution), float(g.resolution), int(g.xsize), int(g.ysize))
    else:
        if shape is None:
            raise ValueError("lattice_of: a geotransform (x0, y0, sx, sy) needs the raster's shape")
        x0, y0, sx, sy = (float(v) for v in grid)
        lat = Lattice(x0, y0, sx, sy, int(shape[-1]), int(shape[-2]))
    if shape is not None and (int(shape[-2]), int(shape[-1])) != (lat.h, lat.w):
        raise ValueError(f"lattice_of: the lattice has {lat.h} x {lat.w} cells, the raster {int(shape[-2])} x {int(shape[-1])}")
    if not (lat.sx > 0.0 and lat.sy > 0.0 and all(math.isfinite(v) for v in lat[:4]) and lat.w >= 1 and lat.h >= 1):
        raise ValueError(f"lattice_of: finite corners, positive cell sizes and at least one cell are required, got {lat}")
    return lat


def _snap(off, step):
    if abs(step - 1.0) <= STEP_TOLERANCE:
        step = 1.0
        if abs(off - round(off)) <= OFFSET_TOLERANCE:
            off = float(round(off))
    return off, step


def warp_map(src, dst):
    """the _lib.SnerfWarpMap that places lattice `dst` in the cell coordinates of lattice `src`"""
    src, dst = lattice_of(src), lattice_of(dst)
    off_x, step_x = _snap((dst.x0 - src.x0) / src.sx, dst.sx / src.sx)
    off_y, step_y = _snap((src.y0 - dst.y0) / src.sy, dst.sy / src.sy)
    return _lib.SnerfWarpMap(off_x, step_x, off_y, step_y, src.w, src.h, dst.w, dst.h)


def _integer_shift(m):
    return m.step_x == 1.0 and m.step_y == 1.0 and m.off_x == round(m.off_x) and m.off_y == round(m.off_y)


def same_lattice(a, b):
    """True when the two lattices have the same corner, cell size and shape, to warp_map's tolerances"""
    m = warp_map(a, b)
    return _integer_shift(m) and m.off_x == 0.0 and m.off_y == 0.0 and (m.src_w, m.src_h) == (m.dst_w, m.dst_h)


def default_method(m, labels=False):
    """bilinear / nearest when both steps are <= 1 (the destination is as fine or finer), average / mode otherwise"""
    fine = m.step_x <= 1.0 and m.step_y <= 1.0
    return ("nearest" if fine else "mode") if labels else ("bilinear" if fine else "average")


def _shift(raster, m, fill):
    """the integer-shift warp: a slice of the source, padded with `fill` where the destination leaves it; (dst, stats)"""
    ox, oy = int(m.off_x), int(m.off_y)
    out = raster.new_full(tuple(raster.shape[:-2]) + (m.dst_h, m.dst_w), fill)
    i0, i1 = max(0, -ox), min(m.dst_w, m.src_w - ox)
    j0, j1 = max(0, -oy), min(m.dst_h, m.src_h - oy)
    inside = max(0, i1 - i0) * max(0, j1 - j0)
    if inside:
        out[..., j0:j1, i0:i1] = raster[..., j0 + oy:j1 + oy, i0 + ox:i1 + ox]
    return out, inside


def warp(raster, src, dst, method=None, min_valid=0.5, return_stats=False):
    """`raster` on lattice `src` -> the same quantity on lattice `dst` (anything lattice_of takes).
      float (h, w) or (C, h, w), C <= 16   snerf_warp_planes; method "nearest", "bilinear", "average", "min" or "max"; other float
                                           dtypes go through .float(); a destination cell is NaN unless at least `min_valid` of its
                                           weight fell on finite source cells;
      uint8 (h, w)                         snerf_warp_labels; method "nearest" or "mode"; 255 = no label.
    The default method is bilinear / nearest when both steps are <= 1, average / mode otherwise.  When the lattices differ by a whole
    number of cells the result is a slice of `raster` padded with NaN / 255: no launch, the bits kept (a value that is not finite
    included).  `return_stats`: also the three counts of the header as a list of ints (a device-to-host copy) -- words written
    finite / labelled, holes written, destination cells with a tap outside the source."""
    if not torch.is_tensor(raster):
        raise ValueError("warp: raster must be a tensor")
    labels = raster.dtype == torch.uint8
    if not (labels or raster.is_floating_point()):
        raise ValueError(f"warp: a float or uint8 raster is taken, got {raster.dtype}")
    if raster.dim() not in ((2,) if labels else (2, 3)):
        raise ValueError(f"warp: {'a label raster is (h, w)' if labels else 'a float raster is (h, w) or (C, h, w)'}, got {tuple(raster.shape)}")
    m = warp_map(lattice_of(src, raster.shape), dst)
    name = default_method(m, labels) if method is None else method
    if name not in (LABEL_METHODS if labels else FLOAT_METHODS):
        raise ValueError(f"warp: method {name!r} is none of {LABEL_METHODS if labels else FLOAT_METHODS} for a {raster.dtype} raster")
    if not (0.0 < float(min_valid) <= 1.0):
        raise ValueError(f"warp: min_valid = {min_valid!r} outside (0, 1]")
    x = raster if labels else raster.float()
    if _integer_shift(m):
        out, inside = _shift(x, m, NO_LABEL if labels else math.nan)
        if not return_stats:
            return out
        holes = int((out == NO_LABEL).sum() if labels else (~torch.isfinite(out)).sum())
        return out, [out.numel() - holes, holes, m.dst_h * m.dst_w - inside]
    if not x.is_cuda:
        raise ValueError("warp: raster must be a GPU tensor (the HIP path has no CPU fallback)")
    x = x.contiguous()
    stats = torch.zeros(3, dtype=torch.int64, device=x.device)
    out = torch.empty(tuple(x.shape[:-2]) + (m.dst_h, m.dst_w), dtype=x.dtype, device=x.device)
    if labels:
        _lib.call("snerf_warp_labels", x, m, METHODS[name], out, stats, exc=ValueError)
    else:
        planes = x.shape[0] if x.dim() == 3 else 1
        if not 1 <= planes <= MAX_PLANES:
            raise ValueError(f"warp: {planes} planes: between 1 and {MAX_PLANES} (SNERF_WARP_MAX_PLANES) are taken in one call")
        _lib.call("snerf_warp_planes", x, planes, m, METHODS[name], float(min_valid), out, stats, exc=ValueError)
    return (out, [int(v) for v in stats.cpu()]) if return_stats else out


def warp_products(products, dst_grid, methods=None):
    """a products dict (ortho_products, nadir_products, rectify, ...: "grid" and planes on it) on lattice `dst_grid` (a DsmGrid):
    every (h, w) float plane, every (h, w) uint8 label plane and every (3, h, w) colour plane -- float in [0, 1] as the products hold
    it, or uint8, which goes through float and back (torch.round, clamp to [0, 255], holes -> 0) -- is warped; "grid" becomes
    `dst_grid`; everything else is passed on.  `methods`: {key: method name} for the planes that should not take the default."""
    src = lattice_of(products["grid"])
    dst = lattice_of(dst_grid)
    methods = methods or {}
    out = {}
    for key, v in products.items():
        if key == "grid":
            out[key] = dst_grid
        elif torch.is_tensor(v) and tuple(v.shape[-2:]) == (src.h, src.w) and (
                (v.dim() == 2 and (v.dtype == torch.uint8 or v.is_floating_point())) or
                (v.dim() == 3 and v.shape[0] == 3 and (v.dtype == torch.uint8 or v.is_floating_point()))):
            if v.dim() == 3 and v.dtype == torch.uint8:
                w = warp(v.float(), src, dst, methods.get(key))
                out[key] = torch.where(torch.isfinite(w), torch.round(w).clamp(0.0, 255.0), torch.zeros_like(w)).to(torch.uint8)
            else:
                out[key] = warp(v, src, dst, methods.get(key))
        else:
            out[key] = v
    return out


def mae_between(pred, pred_grid, gt, gt_grid, water_mask=None, ignore_mask=None, method=None, **kw):
    """the altitude MAE of a prediction on one lattice against a ground truth on another: `pred` is warped onto the ground truth's
    lattice (the masks lie on it already) and dsm.compute_mae runs there.  **kw (min_valid) go to warp."""
    warped = warp(pred, lattice_of(pred_grid, pred.shape), lattice_of(gt_grid, gt.shape), method, **kw)
    return D.compute_mae(warped, gt.to(warped.device), water_mask=water_mask, ignore_mask=ignore_mask)
