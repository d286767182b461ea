"""Roof planes on the map: per-cell normals, roof facets, pitch, aspect and a roof type per building, and how far the surface departs
from its facets' planes -- the LoD2 attributes a user of a satellite surface model asks for after the buildings themselves, and a
per-building quality measure that needs no lidar.  The reference has no counterpart; the spec is include/snerf_roofs.h (DESIGN.md
section 5z), the stages are the kernels of csrc/roofs.hip, torch is plumbing.  The raster functions take and return device tensors.

  normals        snerf_roofs_normals: a least-squares plane over each building cell's neighbours of the same building (integer sums,
                 an fp64 tail): the gradient east / north, an orientation code (flat, eight downslope octants, steep) and the tag
                 object id * 16 + code;
  link           snerf_roofs_link: facets = the connected components of equal tags (the union-find of objects.link);
                 objects.ids_from_parent numbers them 1..F in raster order;
  facet_rows     snerf_roofs_moments: every facet's cells folded into 16 integer words relative to the facet's root cell;
  facet_table    the plane of every facet from those words, exactly in Python ints up to one fp64 division per slope, and the columns
                 a user reads (pitch, azimuth, areas, centroid, bbox; with residual rows rms / mean / max and eave / ridge);
  residuals      snerf_roofs_residuals: the distance of every facet cell from its facet's plane and 8 integer words per facet;
  filter_facets  drops the small facets and the ones without a plane and compacts the ids;
  roof_table     per building: facets, flat and pitched shares, the dominant facet's pitch and azimuth, rms, eave and ridge height and
                 a roof type by a rule whose thresholds are keyword parameters;
  roofs          all of the above in one call;
  roof_agreement two maps' roofs over the buildings match_objects pairs (torch, any device).

Everything a kernel writes is integer or fp64 arithmetic fixed operation by operation: the planes are bit-reproducible.  The defaults
(radius, flat_deg, wall_deg, min_facet_m2 and the roof-type thresholds) are parameters, not claims: what a trained scene's noisy DSM
needs is unmeasured."""
import math

import numpy as np
import torch

from ... import _lib
from . import ortho as OR
from . import objects as OB
from . import terrain as TR

MAX_RADIUS = _lib.ROOFS_MAX_RADIUS
MAX_SIDE = _lib.ROOFS_MAX_SIDE
MAX_OBJECTS = _lib.ROOFS_MAX_OBJECTS
MOMENT_WORDS, RESIDUAL_WORDS = _lib.ROOFS_MOMENT_WORDS, _lib.ROOFS_RESIDUAL_WORDS
FLAT, STEEP, HOLE, DEGENERATE, NONE = _lib.ROOFS_FLAT, _lib.ROOFS_STEEP, _lib.ROOFS_HOLE, _lib.ROOFS_DEGENERATE, _lib.ROOFS_NONE
OCTANTS = ("N", "NE", "E", "SE", "S", "SW", "W", "NW")       # codes 1..8: where the surface falls to
UNIT = 64.0                                                     # key units per residual step: 2^-10 m at q = 2^-16 m
_MOMENT_INIT = (0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 0, -1, 0, 0, 0, 0)     # int64 words: -1 holds 2^64 - 1
_RESIDUAL_INIT = (0, 0, 0, 0, -1, 0, 0, 0)
_BIAS = 2 ** 31


def _raster(t, dtype, name, shape=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"roofs: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"roofs: {name} must be a 2-D {dtype} raster{'' if shape is None else f' of shape {tuple(shape)}'}, got "
                         f"{t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _sizes(h, w):
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"roofs: a raster of {h} x {w} cells: between 1 and {MAX_SIDE} cells a side are taken")


def _count(n, name):
    n = int(n)
    if not 0 <= n < MAX_OBJECTS:
        raise ValueError(f"roofs: {name} = {n} outside [0, 2^27)")
    return n


def _band(band, h):
    return (0, h) if band is None else (int(band[0]), int(band[1]))


def _rows(rows, n, words, init, device):
    if rows is None:
        return torch.tensor(init, dtype=torch.int64, device=device).repeat(n, 1)
    if rows.dtype != torch.int64 or tuple(rows.shape) != (n, words) or not rows.is_contiguous() or not rows.is_cuda:
        raise ValueError(f"roofs: rows must be a contiguous int64 GPU tensor of shape {(n, words)}")
    return rows


def normals(key, ids, K, res, radius=1, flat_deg=5.0, wall_deg=60.0, aspect0_deg=0.0, q=OR.Q):
    """snerf_roofs_normals on the key plane of terrain.keys and the id plane of objects() -> (slope_e, slope_n (H, W) f32: the rise
    per metre east / north, NaN without a normal; code (H, W) uint8; tag (H, W) int32; stats (4) int64: object cells, cells with a
    normal, degenerate cells, hole cells).  `res`: metres per cell; a cell is flat up to a slope of flat_deg, steep beyond wall_deg;
    the octant bins are turned by aspect0_deg (clockwise, one angle for the whole map).  K == 0 launches nothing."""
    key = _raster(key, torch.int32, "key")
    ids = _raster(ids, torch.int32, "ids", key.shape)
    h, w = key.shape
    _sizes(h, w)
    K = _count(K, "K")
    if int(radius) != radius or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"roofs: radius = {radius!r} outside [1, {MAX_RADIUS}]")
    if not (0.0 <= flat_deg <= wall_deg < 90.0):
        raise ValueError(f"roofs: 0 <= flat_deg <= wall_deg < 90 required, got {flat_deg!r} and {wall_deg!r}")
    if not (res > 0.0 and math.isfinite(res) and q > 0.0 and math.isfinite(q) and math.isfinite(aspect0_deg)):
        raise ValueError(f"roofs: res and q must be positive and finite, aspect0_deg finite, got {res!r}, {q!r}, {aspect0_deg!r}")
    dev = key.device
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    if K == 0:
        nan = torch.full((h, w), math.nan, dtype=torch.float32, device=dev)
        return nan, nan.clone(), torch.full((h, w), NONE, dtype=torch.uint8, device=dev), \
            torch.full((h, w), -1, dtype=torch.int32, device=dev), stats
    slope_e, slope_n = torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.float32, device=dev)
    code, tag = torch.empty((h, w), dtype=torch.uint8, device=dev), torch.empty((h, w), dtype=torch.int32, device=dev)
    a0 = math.radians(aspect0_deg)
    tf, tw = math.tan(math.radians(flat_deg)), math.tan(math.radians(wall_deg))
    _lib.call("snerf_roofs_normals", key, ids, h, w, K, int(radius), q, res, math.cos(a0), math.sin(a0), tf * tf, tw * tw, slope_e,
              slope_n, code, tag, stats, exc=ValueError)
    return slope_e, slope_n, code, tag, stats


def link(tag, connectivity=4):
    """snerf_roofs_link -> (parent (H * W) int32, stats (2) int64): per cell -1 where tag < 0, else the smallest linear index of the
    cell's facet.  Raises RuntimeError if the walk's guard tripped (stats[0]); reading it is the one host synchronisation."""
    tag = _raster(tag, torch.int32, "tag")
    if connectivity not in (4, 8):
        raise ValueError(f"roofs: connectivity must be 4 or 8, got {connectivity!r}")
    h, w = tag.shape
    _sizes(h, w)
    parent = torch.empty(h * w, dtype=torch.int32, device=tag.device)
    stats = torch.zeros(2, dtype=torch.int64, device=tag.device)
    _lib.call("snerf_roofs_link", tag, h, w, connectivity, parent, stats, exc=ValueError)
    trips = int(stats[0].item())
    if trips:
        raise RuntimeError(f"roofs.link: the union-find guard tripped {trips} time(s): `parent` was written during the call")
    return parent, stats


def facet_rows(fids, F, root, key, tag, rows=None, stats=None, band=None):
    """snerf_roofs_moments -> (rows (F, 16) int64 holding the u64 words, stats (3) int64: cells folded, left out, ignored).  `root`: the
    parent plane of link(); `rows` / `stats`: accumulators of earlier calls; `band` = (row0, row1): fold the cells of those rows only
    -- bands that partition the raster, accumulated into one `rows`, give the words of one call.  F == 0 launches nothing."""
    fids = _raster(fids, torch.int32, "fids")
    h, w = fids.shape
    _sizes(h, w)
    root = _raster(root.reshape(h, w), torch.int32, "root", fids.shape)
    key = _raster(key, torch.int32, "key", fids.shape)
    tag = _raster(tag, torch.int32, "tag", fids.shape)
    F = _count(F, "F")
    rows = _rows(rows, F, MOMENT_WORDS, _MOMENT_INIT, fids.device)
    stats = torch.zeros(3, dtype=torch.int64, device=fids.device) if stats is None else stats
    row0, row1 = _band(band, h)
    if F:
        _lib.call("snerf_roofs_moments", fids, root, key, tag, h, w, F, row0, row1, rows, stats, exc=ValueError)
    return rows, stats


def residuals(fids, F, root, key, planes, q=OR.Q, unit=UNIT, rows=None, stats=None, band=None, out=None):
    """snerf_roofs_residuals -> (residual (H, W) f32 in metres, NaN off facets and on facets without a plane; rows (F, 8) int64 holding
    the u64 words; stats (3) int64: cells with a residual, facet cells without one, ignored cells).  `planes` (F, 3) f64 on the GPU:
    (gamma, alpha, beta) per facet in key units, NaN = no plane (facet_table's "plane").  `band`, `rows`, `stats`, `out`: as
    facet_rows; a band writes its own rows of `out`.  F == 0 launches nothing."""
    fids = _raster(fids, torch.int32, "fids")
    h, w = fids.shape
    _sizes(h, w)
    root = _raster(root.reshape(h, w), torch.int32, "root", fids.shape)
    key = _raster(key, torch.int32, "key", fids.shape)
    F = _count(F, "F")
    if not (torch.is_tensor(planes) and planes.is_cuda and planes.dtype == torch.float64 and tuple(planes.shape) == (F, 3)):
        raise ValueError(f"roofs: planes must be a float64 GPU tensor of shape {(F, 3)}")
    if not (q > 0.0 and math.isfinite(q) and unit > 0.0 and math.isfinite(unit)):
        raise ValueError(f"roofs: q and unit must be positive and finite, got {q!r} and {unit!r}")
    rows = _rows(rows, F, RESIDUAL_WORDS, _RESIDUAL_INIT, fids.device)
    stats = torch.zeros(3, dtype=torch.int64, device=fids.device) if stats is None else stats
    if out is None:
        out = torch.full((h, w), math.nan, dtype=torch.float32, device=fids.device)
    else:
        out = _raster(out, torch.float32, "out", fids.shape)
    row0, row1 = _band(band, h)
    if F:
        _lib.call("snerf_roofs_residuals", fids, root, key, h, w, F, planes.contiguous(), q, unit, row0, row1, out, rows, stats,
                  exc=ValueError)
    else:
        out[row0:row1] = math.nan
    return out, rows, stats


def _signed(rows, words):
    r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
    return r.view(np.int64).reshape(-1, words) if r.dtype == np.uint64 else r.astype(np.int64).reshape(-1, words)


def solve(row):
    """the plane of one facet from its moment words -> (gamma, alpha, beta) predicting dk from (di, dj) in key units; NaNs for an empty
    facet or collinear cells (D == 0).  The central moments n Sxx - Sx^2, ... are exact Python ints (each below 2^116); the slopes are
    one fp64 division each, gamma comes from the means."""
    n, sx, sy, sk, sxx, sxy, syy, sxk, syk = (int(v) for v in row[:9])
    if n <= 0:
        return math.nan, math.nan, math.nan
    cxx, cxy, cyy = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    cxk, cyk = n * sxk - sx * sk, n * syk - sy * sk
    D = cxx * cyy - cxy * cxy
    if D == 0:
        return math.nan, math.nan, math.nan
    alpha, beta = (cxk * cyy - cyk * cxy) / D, (cyk * cxx - cxk * cxy) / D
    return ((float(sk) - alpha * float(sx)) - beta * float(sy)) / float(n), alpha, beta


def facet_table(rows, grid, z0=OR.Z0, q=OR.Q, root_key=None, residual_rows=None, unit=UNIT):
    """per-facet columns from the moment words, on the host -> a dict of numpy arrays of length F (facet n is entry n - 1).  `grid`: the
    lattice of the raster (a DsmGrid, or a _lib.SnerfDsmGrid window).
      object, code                          the building's id and the orientation code, from the tag                      int64
      area_cells, left_out, area_m2         the cells folded, the ones left out (|dk| >= 2^24), area_cells res^2
      plane (F, 3)                          (gamma, alpha, beta) of solve(): NaN for a facet without a plane (D == 0, a strip)
      slope_e, slope_n                      alpha q / res, -beta q / res: the rise per metre east / north
      pitch_deg, azimuth_deg                atan of the slope; where the facet falls to, clockwise from north (NaN on a level facet)
      surface_m2                            area_m2 sqrt(1 + slope^2)
      east, north, bbox (F, 4)              the centroid of the cell centres; east_min, north_min, east_max, north_max of the cell edges
      root                                  the linear index of the facet's root cell                                      int64
      alt                                   the plane's altitude at the centroid; needs `root_key` ((F) the keys at the roots), else NaN
    With `residual_rows` (the words of residuals()) also
      rms_m, mean_abs_m, max_abs_m          of the cells' distances from the plane, in steps of q unit
      clamped                               cells whose distance was clamped at 2^18 steps                                 int64
      eave_alt, ridge_alt                   the lowest and the highest altitude among the facet's cells"""
    r = _signed(rows, MOMENT_WORDS)
    g = OR.window_grid(grid)
    xoff, yoff, res = float(g.xoff), float(g.yoff), float(g.resolution)
    F = len(r)
    plane = np.array([solve(row) for row in r.tolist()], np.float64).reshape(F, 3)
    f = r.astype(np.float64)
    n = f[:, 0]
    k0 = np.full(F, np.nan) if root_key is None else np.asarray(root_key.cpu() if torch.is_tensor(root_key) else root_key, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope_e, slope_n = plane[:, 1] * q / res, -plane[:, 2] * q / res
        s2 = slope_e * slope_e + slope_n * slope_n
        azimuth = np.where(s2 > 0.0, np.degrees(np.arctan2(-slope_e, -slope_n)) % 360.0, np.nan)
        mi, mj = f[:, 1] / n, f[:, 2] / n
        i0, j0 = r[:, 14] % int(g.xsize), r[:, 14] // int(g.xsize)
        alt = z0 + q * (k0 + plane[:, 0] + plane[:, 1] * mi + plane[:, 2] * mj)
        east, north = xoff + (i0 + mi + 0.5) * res, yoff - (j0 + mj + 0.5) * res
    has = r[:, 0] > 0
    bbox = np.where(has[:, None], np.stack([xoff + f[:, 9] * res, yoff - (f[:, 12] + 1.0) * res, xoff + (f[:, 10] + 1.0) * res,
                                            yoff - f[:, 11] * res], 1), np.nan)
    area_m2 = n * res * res
    table = {"object": r[:, 13] >> 4, "code": r[:, 13] & 15, "area_cells": r[:, 0].copy(), "left_out": r[:, 15].copy(), "area_m2": area_m2,
             "plane": plane, "slope_e": slope_e, "slope_n": slope_n, "pitch_deg": np.degrees(np.arctan(np.sqrt(s2))), "azimuth_deg": azimuth,
             "surface_m2": area_m2 * np.sqrt(1.0 + s2), "east": east, "north": north, "bbox": bbox, "root": r[:, 14].copy(), "alt": alt}
    if residual_rows is not None:
        e = _signed(residual_rows, RESIDUAL_WORDS)
        if len(e) != F:
            raise ValueError(f"roofs: {F} rows but {len(e)} residual rows")
        ef = e.astype(np.float64)
        step = q * unit
        with np.errstate(divide="ignore", invalid="ignore"):
            got = e[:, 0] > 0
            nan = np.full(F, np.nan)
            table.update(rms_m=np.where(got, step * np.sqrt(ef[:, 2] / ef[:, 0]), nan), mean_abs_m=np.where(got, step * ef[:, 1] / ef[:, 0], nan),
                         max_abs_m=np.where(got, step * ef[:, 3], nan), clamped=e[:, 6].copy(), residual_cells=e[:, 0].copy(),
                         eave_alt=np.where(got, z0 + q * (ef[:, 4] - _BIAS), nan), ridge_alt=np.where(got, z0 + q * (ef[:, 5] - _BIAS), nan))
    return table


def filter_facets(fids, table, min_facet_m2=0.0):
    """drop the facets below `min_facet_m2` and the ones without a plane -> (fids with the dropped facets' cells 0 and the others
    renumbered 1..F' in the same order, table with their entries removed): one lookup table, one gather, as filter_objects"""
    keep = (np.asarray(table["area_m2"]) >= float(min_facet_m2)) & np.isfinite(np.asarray(table["plane"])).all(axis=1)
    lut = np.zeros(len(keep) + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    out = torch.from_numpy(lut).to(fids.device)[fids.long()]
    return out, {k: np.asarray(v)[keep] for k, v in table.items()}


def _opposed(a, b):
    return (int(a) - int(b)) % 8 == 4


def roof_table(facets, objects_table, flat_share=0.2, major_share=0.1):
    """per building (entry n - 1 = object n of `objects_table`, objects()'s table) from the kept facets (filter_facets' table) -> a dict
    of numpy arrays of length K:
      facets, flat_facets, pitched_facets       counts                                                               int64
      facet_area_m2, flat_share, pitched_share  the kept facets' area and the shares of it on flat (code 0) / pitched (1..8) facets
      pitch_deg, azimuth_deg                    of the dominant (largest; at a tie the first) facet
      pitch_mean_deg                            the area-weighted mean pitch
      rms_m                                     over all kept facet cells (NaN without residual columns)
      eave_height, ridge_height                 the lowest eave / highest ridge over the object's ground_alt
      roof_type, levels                         "none" without a kept facet; "flat" when pitched_share < flat_share, with levels = the
          number of flat facets (0 otherwise); else by the pitched facets that hold at least major_share of the kept area each: one
          "shed", two whose octants are 4 apart "gabled", four in two opposing pairs "hipped", anything else "complex".
    flat_share and major_share are parameters, not claims."""
    K = len(objects_table["area_cells"])
    obj, code = np.asarray(facets["object"], np.int64), np.asarray(facets["code"], np.int64)
    area, pitch, azim = (np.asarray(facets[k], np.float64) for k in ("area_m2", "pitch_deg", "azimuth_deg"))
    has_res = "rms_m" in facets
    ground = np.asarray(objects_table["ground_alt"], np.float64)
    out = {k: np.zeros(K, np.int64) for k in ("facets", "flat_facets", "pitched_facets", "levels")}
    out.update({k: np.full(K, np.nan) for k in ("facet_area_m2", "flat_share", "pitched_share", "pitch_deg", "azimuth_deg", "pitch_mean_deg",
                                                "rms_m", "eave_height", "ridge_height")})
    types = []
    for n in range(1, K + 1):
        at = np.flatnonzero(obj == n)
        if not len(at):
            types.append("none")
            continue
        a, total = area[at], float(area[at].sum())
        flat, pitched = code[at] == FLAT, code[at] != FLAT
        top = at[int(np.argmax(a))]
        k = n - 1
        out["facets"][k], out["flat_facets"][k], out["pitched_facets"][k] = len(at), int(flat.sum()), int(pitched.sum())
        out["facet_area_m2"][k] = total
        out["flat_share"][k], out["pitched_share"][k] = float(a[flat].sum()) / total, float(a[pitched].sum()) / total
        out["pitch_deg"][k], out["azimuth_deg"][k] = pitch[top], azim[top]
        out["pitch_mean_deg"][k] = float((a * pitch[at]).sum()) / total
        if has_res:
            cells = np.asarray(facets["residual_cells"], np.float64)[at]
            rms = np.asarray(facets["rms_m"], np.float64)[at]
            got = cells > 0
            if got.any():
                out["rms_m"][k] = math.sqrt(float((cells[got] * rms[got] ** 2).sum()) / float(cells[got].sum()))
                out["eave_height"][k] = float(np.nanmin(np.asarray(facets["eave_alt"], np.float64)[at])) - ground[k]
                out["ridge_height"][k] = float(np.nanmax(np.asarray(facets["ridge_alt"], np.float64)[at])) - ground[k]
        if out["pitched_share"][k] < flat_share:
            types.append("flat")
            out["levels"][k] = int(flat.sum())
            continue
        major = sorted(int(c) for c in code[at][pitched & (a >= major_share * total)])
        if len(major) == 1:
            types.append("shed")
        elif len(major) == 2 and _opposed(major[0], major[1]):
            types.append("gabled")
        elif len(major) == 4 and _opposed(major[0], major[2]) and _opposed(major[1], major[3]) and len(set(major)) == 4:
            types.append("hipped")
        else:
            types.append("complex")
    out["roof_type"] = np.array(types, dtype=object)
    return out


def roofs(alt, ids, K, grid, objects_table, radius=1, flat_deg=5.0, wall_deg=60.0, aspect0_deg=0.0, connectivity=4, min_facet_m2=4.0,
          z0=OR.Z0, q=OR.Q):
    """The roofs of the altitude plane `alt` ((H, W) f32 on the GPU) under the object ids `ids`, K and table of objects(), on the
    lattice `grid`: terrain.keys, normals, link, objects.ids_from_parent, facet_rows, facet_table, residuals, filter_facets and
    roof_table in one call -> {"slope_e", "slope_n", "pitch_deg", "residual" (H, W) f32, "code" (H, W) uint8, "facet_ids" (H, W) int32:
    the kept facets 1..n_facets, "n_facets", "facets": their table, "buildings": roof_table's, "stats": {"object_cells", "normals",
    "degenerate", "holes", "facet_cells", "facets_found", "folded", "left_out", "residual_cells", "without_residual"} as Python ints,
    "parameters"}.  Reading the counts is the host synchronisation."""
    alt = _raster(alt, torch.float32, "alt")
    ids = _raster(ids, torch.int32, "ids", alt.shape)
    res = float(OR.window_grid(grid).resolution)
    key, _, _ = TR.keys(alt, z0=z0, q=q)
    slope_e, slope_n, code, tag, nstats = normals(key, ids, K, res, radius, flat_deg, wall_deg, aspect0_deg, q)
    parent, lstats = link(tag, connectivity)
    fids, F = OB.ids_from_parent(parent, *alt.shape)
    rows, mstats = facet_rows(fids, F, parent, key, tag)
    root_key = key.reshape(-1)[rows[:, 14]] if F else torch.zeros(0, dtype=torch.int32, device=alt.device)
    planes = facet_table(rows, grid, z0, q)["plane"]
    residual, rrows, rstats = residuals(fids, F, parent, key, torch.from_numpy(planes).to(alt.device), q)
    table = facet_table(rows, grid, z0, q, root_key=root_key, residual_rows=rrows)
    fids, table = filter_facets(fids, table, min_facet_m2)
    residual = torch.where(fids > 0, residual, torch.full_like(residual, math.nan))
    n, l, m, r = ([int(v) for v in s.cpu()] for s in (nstats, lstats, mstats, rstats))
    return {"slope_e": slope_e, "slope_n": slope_n, "pitch_deg": torch.rad2deg(torch.atan(torch.sqrt(slope_e * slope_e + slope_n * slope_n))),
            "code": code, "facet_ids": fids, "residual": residual, "n_facets": len(table["object"]), "facets": table,
            "buildings": roof_table(table, objects_table),
            "stats": {"object_cells": n[0], "normals": n[1], "degenerate": n[2], "holes": n[3], "facet_cells": l[1], "facets_found": F,
                      "folded": m[0], "left_out": m[1], "residual_cells": r[0], "without_residual": r[1]},
            "parameters": {"radius": int(radius), "flat_deg": flat_deg, "wall_deg": wall_deg, "aspect0_deg": aspect0_deg,
                           "connectivity": connectivity, "min_facet_m2": min_facet_m2}}


def roof_agreement(res, ref, pairs):
    """a map's roofs (`res`, as roofs() returns them) against a reference's (`ref`) over the buildings that match_objects pairs
    (`pairs` (M, 2) of (id in res, id in ref)) -> {"pairs", "types": the roof types in order of appearance, "type_table": the
    confusion table [type of res][type of ref] as counts, "type_agreement": the share of pairs with one type, "per_pair": [{"a", "b",
    "type_a", "type_b", "pitch_error_deg" (dominant pitch, a - b), "azimuth_agrees" (within 45 degrees; None where either is level)}],
    "pitch_mae_deg", "normal_cells", "normal_angle_mean_deg", "normal_angle_median_deg": the angle between the two maps' normals over the
    cells where both have one (None without a cell)}.  A lattice mismatch is a ValueError.  Plain torch: any device."""
    if tuple(res["slope_e"].shape) != tuple(ref["slope_e"].shape):
        raise ValueError(f"roof_agreement: the maps differ in shape: {tuple(res['slope_e'].shape)} and {tuple(ref['slope_e'].shape)}")
    pairs = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, np.int64).reshape(-1, 2)
    ta, tb = res["buildings"], ref["buildings"]
    per_pair, types = [], []
    for a, b in pairs.tolist():
        ka, kb = str(ta["roof_type"][a - 1]), str(tb["roof_type"][b - 1])
        for t in (ka, kb):
            if t not in types:
                types.append(t)
        za, zb = float(ta["azimuth_deg"][a - 1]), float(tb["azimuth_deg"][b - 1])
        agrees = None if math.isnan(za) or math.isnan(zb) else bool(abs((za - zb + 180.0) % 360.0 - 180.0) <= 45.0)
        d = float(ta["pitch_deg"][a - 1]) - float(tb["pitch_deg"][b - 1])
        per_pair.append({"a": a, "b": b, "type_a": ka, "type_b": kb, "pitch_error_deg": None if math.isnan(d) else d,
                         "azimuth_agrees": agrees})
    table = [[sum(1 for p in per_pair if p["type_a"] == x and p["type_b"] == y) for y in types] for x in types]
    errs = [abs(p["pitch_error_deg"]) for p in per_pair if p["pitch_error_deg"] is not None]
    ea, na, eb, nb = (t.double() for t in (res["slope_e"], res["slope_n"], ref["slope_e"], ref["slope_n"]))
    both = torch.isfinite(ea) & torch.isfinite(na) & torch.isfinite(eb) & torch.isfinite(nb)
    ea, na, eb, nb = ea[both], na[both], eb[both], nb[both]
    # the normals (-e, -n, 1): atan2 of their cross product's length over their dot product -- exactly 0 for equal gradients
    cx, cy, cz = nb - na, ea - eb, ea * nb - na * eb
    angle = torch.rad2deg(torch.atan2(torch.sqrt(cx * cx + cy * cy + cz * cz), ea * eb + na * nb + 1.0))
    cells = int(angle.numel())
    return {"pairs": len(per_pair), "types": types, "type_table": table,
            "type_agreement": sum(1 for p in per_pair if p["type_a"] == p["type_b"]) / len(per_pair) if per_pair else None,
            "per_pair": per_pair, "pitch_mae_deg": float(np.mean(errs)) if errs else None, "normal_cells": cells,
            "normal_angle_mean_deg": float(angle.mean()) if cells else None,
            "normal_angle_median_deg": float(angle.median()) if cells else None}


def table_records(table):
    """a facet or building table as a list of JSON-ready records (entry k is record k, with "id": k + 1); a non-finite value is None"""
    def plain(v):
        if isinstance(v, np.ndarray):
            return [plain(x) for x in v]
        if isinstance(v, (np.integer, int)):
            return int(v)
        if isinstance(v, str):
            return v
        v = float(v)
        return v if np.isfinite(v) else None
    n = len(next(iter(table.values()))) if table else 0
    return [dict({"id": k + 1}, **{name: plain(col[k]) for name, col in table.items()}) for k in range(n)]
