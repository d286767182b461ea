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
  grow           snerf_roofs_grow: the kept facets grown over the dropped cells of their buildings, so that neighbours touch;
  lines          the arcs of the grown facets (eval/utils/arcs.py) as ridge, hip, valley, step, eave, top and rake lines with heights;
  line_table     per building the summed line lengths per kind;
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


# ---- roof lines ---------------------------------------------------------------------------------------------------------------------------
GROW_BATCH = 8                                                  # rounds queued between two reads of the counters
LINE_KINDS = ("ridge", "hip", "valley", "crease", "step", "enclosed", "eave", "top", "rake", "flat_edge")


def grow(fids, ids, key, table, grow_m=0.25, q=OR.Q, unit=UNIT, max_rounds=None):
    """snerf_roofs_grow: the kept facets (`fids`, `table`: what filter_facets returns) grown over the cells of their buildings that
    carry no facet -- the hip lines and steps the facet filter dropped -- so that neighbouring facets touch -> (grown (H, W) int32,
    grown_cells (F) int64 numpy: the cells every facet gained, rounds: how many rounds assigned a cell).  In a round a building cell
    without a facet takes, among the facets of its N, E, S, W neighbours in the same building, the one whose plane it misses by the least,
    if that is at most `grow_m` metres (in steps of q unit); the rounds are Jacobi steps, GROW_BATCH of them are queued between two reads
    of the counters, and the growth stops after a batch whose last round assigned nothing, or at `max_rounds` (default H + W) rounds.  A
    facet only gains cells next to itself: it stays one component.  grow_m is a parameter, not a claim."""
    fids = _raster(fids, torch.int32, "fids")
    h, w = fids.shape
    _sizes(h, w)
    ids = _raster(ids, torch.int32, "ids", fids.shape)
    key = _raster(key, torch.int32, "key", fids.shape)
    F = _count(len(table["object"]), "F")
    if not (grow_m >= 0.0 and math.isfinite(grow_m) and q > 0.0 and math.isfinite(q) and unit > 0.0 and math.isfinite(unit)):
        raise ValueError(f"roofs: grow_m >= 0, q > 0 and unit > 0, all finite, required, got {grow_m!r}, {q!r}, {unit!r}")
    limit = h + w if max_rounds is None else int(max_rounds)
    if limit < 1:
        raise ValueError(f"roofs: max_rounds = {max_rounds!r} is below 1")
    dev = fids.device
    planes = torch.from_numpy(np.ascontiguousarray(np.asarray(table["plane"], np.float64).reshape(F, 3))).to(dev)
    root = torch.from_numpy(np.asarray(table["root"]).astype(np.int32).reshape(F)).to(dev)
    max_rq = int(math.floor(grow_m / (q * unit)))
    cur, a, b = fids, torch.empty_like(fids), torch.empty_like(fids)
    counts = []
    while len(counts) < limit:
        n = min(GROW_BATCH, limit - len(counts))
        stats = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        _lib.call("snerf_roofs_grow", cur, ids, key, root, planes, h, w, F, unit, max_rq, n, a, b, stats, exc=ValueError)
        # the batch's result lies in the buffer its last round wrote; the next batch reads it and writes the other one first
        cur, a, b = (a, b, a) if n & 1 else (b, a, b)
        s = [int(v) for v in stats.cpu()]
        if s[n]:
            raise RuntimeError(f"roofs.grow: {s[n]} guard trip(s): a facet id outside [0, {F}] or a facet root outside the raster")
        counts += s[:n]
        if s[n - 1] == 0:
            break
    grown = cur.clone()
    gained = (torch.bincount(grown.reshape(-1).long(), minlength=F + 1) - torch.bincount(fids.reshape(-1).long(), minlength=F + 1))[1:F + 1]
    return grown, gained.cpu().numpy().astype(np.int64), max([r + 1 for r, c in enumerate(counts) if c], default=0)


def _line(kind, obj, right, left, xyz, step=None, height=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    seg = np.diff(xyz, axis=0)
    length = float(np.hypot(seg[:, 0], seg[:, 1]).sum())
    pitch = math.degrees(math.atan2(abs(float(xyz[-1, 2] - xyz[0, 2])), length)) if length > 0.0 else 0.0
    return {"kind": kind, "object": int(obj), "facet_right": int(right), "facet_left": int(left),
            "coordinates": [[float(e), float(n), float(z)] for e, n, z in xyz], "length_m": length, "pitch_deg": pitch,
            "step_m": None if step is None else float(step), "height_m": None if height is None else float(height)}


def lines(arcs, facets, grid, step_m=1.0, level_deg=5.0, simplify_cells=0, z0=OR.Z0, q=OR.Q):
    """The roof lines of a facet raster, on the host: `arcs` is what arcs.arcs() returns for the (grown) facet ids, `facets` the kept
    facets' table (with "alt": facet_table needs `root_key`), `grid` the raster's lattice -> a list of records {"kind", "object",
    "facet_right", "facet_left", "coordinates": [[east, north, z], ...], "length_m" (in plan), "pitch_deg" (of the line itself, end to
    end), "step_m", "height_m"}.  Every arc is taken once, from its owner.  The raster is north-up and an arc runs with its own facet R
    on its right: in (east, north), with the unit tangent t, the left normal is nl = (-t_n, t_e); s = (slope_e, slope_n) of a facet.
    INTERIOR arc (R and the facet on the left, L, belong to one building): t is the chord from the first to the last vertex; a zero
    chord, or a closed arc, is "enclosed".  d = the mean over the vertices of z_R - z_L; |d| > step_m is a "step" (step_m = |d|, z from
    the higher plane).  Else, with a = s_R . nl and b = -s_L . nl, the rise per metre of either facet towards the line, and tol =
    tan(level_deg): a, b > tol is a "ridge" when |(s_R + s_L) / 2 . t| <= tol and a "hip" otherwise; a, b < -tol a "valley"; anything
    else a "crease"; z = (z_R + z_L) / 2.
    OUTER arc (nothing on the left, or another building): simplified by `simplify_cells` (outline's distance; nodes stay), then segment
    by segment with o = s_R . nl, the rise going outward: o < -tol "eave", o > tol "top", else "flat_edge" on a flat facet (code 0) and
    "rake" on a pitched one; consecutive segments of one kind are one line; z from R's plane; height_m = the line's mean z minus the
    mean altitude of the cells across, where the arcs carry key sums.
    step_m, level_deg and simplify_cells are parameters, not claims."""
    from fractions import Fraction
    from . import outline as OL
    g = OR.window_grid(grid)
    xoff, yoff, res = float(g.xoff), float(g.yoff), float(g.resolution)
    tol = math.tan(math.radians(level_deg))
    obj, code = np.asarray(facets["object"], np.int64), np.asarray(facets["code"], np.int64)
    se, sn, alt = (np.asarray(facets[k], np.float64) for k in ("slope_e", "slope_n", "alt"))
    ce, cn = np.asarray(facets["east"], np.float64) - xoff, yoff - np.asarray(facets["north"], np.float64)
    if not np.isfinite(alt).all():
        raise ValueError("roofs.lines: the facet table carries no altitudes (facet_table needs root_key)")
    t2 = Fraction(simplify_cells) ** 2

    def plane(f, xy):
        """the altitude of facet f's plane at lattice vertices"""
        k = f - 1
        return alt[k] + se[k] * (xy[:, 0] * res - ce[k]) - sn[k] * (xy[:, 1] * res - cn[k])

    def to_xyz(xy, z):
        return np.stack([xoff + xy[:, 0] * res, yoff - xy[:, 1] * res, z], 1)

    out = []
    for a in np.flatnonzero(np.asarray(arcs["owner"])).tolist():
        R, L = int(arcs["right"][a]), int(arcs["left"][a])
        pts = OL.arc_points(arcs, a)
        closed = bool(arcs["closed"][a])
        if L > 0 and obj[L - 1] == obj[R - 1]:
            xy = np.array(pts, np.float64).reshape(-1, 2)
            if closed:
                xy = np.concatenate([xy, xy[:1]])
            zr, zl = plane(R, xy), plane(L, xy)
            chord = np.array([(xy[-1, 0] - xy[0, 0]) * res, -(xy[-1, 1] - xy[0, 1]) * res])
            norm = float(np.hypot(*chord))
            d = float(np.mean(zr - zl))
            if closed or norm == 0.0:
                out.append(_line("enclosed", obj[R - 1], R, L, to_xyz(xy, 0.5 * (zr + zl))))
            elif abs(d) > step_m:
                out.append(_line("step", obj[R - 1], R, L, to_xyz(xy, zr if d > 0.0 else zl), step=abs(d)))
            else:
                t = chord / norm
                nl = np.array([-t[1], t[0]])
                sa, sb = se[R - 1] * nl[0] + sn[R - 1] * nl[1], -(se[L - 1] * nl[0] + sn[L - 1] * nl[1])
                along = 0.5 * ((se[R - 1] + se[L - 1]) * t[0] + (sn[R - 1] + sn[L - 1]) * t[1])
                if sa > tol and sb > tol:
                    kind = "ridge" if abs(along) <= tol else "hip"
                elif sa < -tol and sb < -tol:
                    kind = "valley"
                else:
                    kind = "crease"
                out.append(_line(kind, obj[R - 1], R, L, to_xyz(xy, 0.5 * (zr + zl))))
            continue
        if t2 > 0 and len(pts) >= 3:
            pts = [pts[k] for k in (OL._ring_keep(pts, t2) if closed else OL._open_keep(pts, t2))]
        xy = np.array(pts, np.float64).reshape(-1, 2)
        if closed:
            xy = np.concatenate([xy, xy[:1]])
        xyz = to_xyz(xy, plane(R, xy))
        kinds = []
        for k in range(len(xy) - 1):
            te, tn = (xy[k + 1, 0] - xy[k, 0]) * res, -(xy[k + 1, 1] - xy[k, 1]) * res
            norm = math.hypot(te, tn)
            o = (se[R - 1] * -tn + sn[R - 1] * te) / norm if norm > 0.0 else 0.0
            kinds.append("eave" if o < -tol else "top" if o > tol else "flat_edge" if code[R - 1] == FLAT else "rake")
        runs = []                                               # [kind, first segment, one past the last]
        for k, kind in enumerate(kinds):
            if runs and runs[-1][0] == kind:
                runs[-1][2] = k + 1
            else:
                runs.append([kind, k, k + 1])
        ground = None
        if int(arcs["key_edges"][a]) > 0:
            ground = z0 + q * (float(arcs["key_sum_left"][a]) / float(arcs["key_edges"][a]))
        if closed and len(runs) > 1 and runs[0][0] == runs[-1][0]:          # a closed arc's first and last run meet at its start
            kind, lo, hi = runs.pop()
            first_run = runs.pop(0)
            joined = np.concatenate([xyz[lo:hi + 1], xyz[1:first_run[2] + 1]])
            out.append(_line(kind, obj[R - 1], R, L, joined, height=None if ground is None else float(joined[:, 2].mean()) - ground))
        for kind, lo, hi in runs:
            part = xyz[lo:hi + 1]
            out.append(_line(kind, obj[R - 1], R, L, part, height=None if ground is None else float(part[:, 2].mean()) - ground))
    return out


def line_table(lines, K):
    """per building (entry n - 1 = object n) the summed plan lengths of its lines per kind -> {"lines": (K) int64, kind: (K) f64 for every
    kind of LINE_KINDS}"""
    out = {"lines": np.zeros(K, np.int64)}
    out.update({kind: np.zeros(K, np.float64) for kind in LINE_KINDS})
    for rec in lines:
        n = int(rec["object"])
        if 1 <= n <= K:
            out["lines"][n - 1] += 1
            out[rec["kind"]][n - 1] += rec["length_m"]
    return out


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
