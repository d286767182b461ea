"""Objects on the map: the connected components of a class raster, per-object footprints, heights and volumes, and the object-level
comparison of two maps -- which buildings there are, where they stand, how big and how tall, without the rasters leaving the device
for scipy.ndimage.  The reference has no counterpart; the spec is include/snerf_objects.h, the stages are the
kernels of csrc/objects.hip, torch is plumbing.  The raster functions take and return device tensors.

  components     snerf_objects_link (a lock-free union-find: init, merge, flatten) gives every member cell the smallest index of its
                 component; a cumsum over the roots turns them into ids 1..K in raster order (0 = background);
  object_rows    snerf_objects_stats folds every object's cells into 16 integer words (area, index sums and extremes, altitude sums
                 and extremes, the ground cells in a ring round the object, the perimeter, the class);
  object_table   derives the columns a user reads (m2, centroid, bbox, height, volume) from the words in fp64 on the host;
  filter_objects drops the small ones and compacts the ids;
  objects        the three above in one call, plus the raster of every cell's object height;
  match_objects  pairs the objects of two id rasters by IoU > 1/2 in integers (an object then has at most one partner);
  object_scores  detection precision / recall / F1, footprint IoU and the height error of the matched objects.

Everything a kernel writes is integer: the words are bit-reproducible and do not depend on launch order or on row banding."""
import ctypes as C

import numpy as np
import torch

from ... import _lib
from . import ortho as OR

ROW_WORDS = _lib.OBJECTS_ROW_WORDS
NO_LABEL = _lib.ORTHO_NO_LABEL
MAX_RING = _lib.ORTHO_MAX_RADIUS
_ROW_INIT = (0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0)      # int64 words: -1 holds 2^64 - 1
_BIAS = 2 ** 31


def class_table(classes, what="classes"):
    """a set of class ids -> the 256-byte HOST table the entries take (a ctypes array)"""
    t = (C.c_ubyte * 256)()
    for c in classes:
        if int(c) != c or not 0 <= int(c) < NO_LABEL:
            raise ValueError(f"objects: {what} must be class ids in [0, {NO_LABEL}) ({NO_LABEL} means no label), got {c!r}")
        t[int(c)] = 1
    return t


def _raster(t, dtype, name, shape=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"objects: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"objects: {name} must be a 2-D {dtype} raster{'' if shape is None else f' of shape {tuple(shape)}'}, got "
                         f"{t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def link(label, classes, connectivity=4, parent=None):
    """snerf_objects_link -> (parent (H * W) int32, stats (2) int64): per cell -1 off `classes`, else the smallest linear index of
    the cell's component.  Raises RuntimeError if the walk's guard tripped (stats[0]); reading it is the one host synchronisation."""
    label = _raster(label, torch.uint8, "label")
    if connectivity not in (4, 8):
        raise ValueError(f"objects: connectivity must be 4 or 8, got {connectivity!r}")
    h, w = label.shape
    if h * w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"objects: a raster of {h} x {w} cells: between 1 and 2^31 - 1 cells are taken")
    table = class_table(classes)
    if parent is None:
        parent = torch.empty(h * w, dtype=torch.int32, device=label.device)
    if parent.dtype != torch.int32 or parent.numel() != h * w or not parent.is_cuda:
        raise ValueError(f"objects: parent must hold {h * w} int32 words on the GPU")
    stats = torch.zeros(2, dtype=torch.int64, device=label.device)
    _lib.call("snerf_objects_link", label, h, w, table, connectivity, parent, stats, exc=ValueError)
    trips = int(stats[0].item())
    if trips:
        raise RuntimeError(f"objects.link: the union-find guard tripped {trips} time(s): `parent` was written during the call")
    return parent, stats


def ids_from_parent(parent, h, w):
    """roots -> (ids (h, w) int32, K): 0 = background, 1..K in the raster order of the roots (plain torch, any device)"""
    parent = parent.reshape(-1)
    is_root = parent == torch.arange(parent.numel(), dtype=parent.dtype, device=parent.device)
    rank = torch.cumsum(is_root, 0, dtype=torch.int32)
    ids = torch.where(parent < 0, torch.zeros_like(rank), rank[parent.clamp_min(0).long()])
    return ids.reshape(h, w), int(rank[-1].item())


def components(label, classes, connectivity=4):
    """the connected components of the cells of `label` ((H, W) uint8 on the GPU) whose class is in `classes`; two cells are linked
    when they are 4- / 8-neighbours and of the SAME class -> (ids (H, W) int32, K)"""
    parent, _ = link(label, classes, connectivity)
    return ids_from_parent(parent, *label.shape)


def new_rows(K, device):
    """(K, 16) int64 holding the initial u64 words of snerf_objects_stats"""
    return torch.tensor(_ROW_INIT, dtype=torch.int64, device=device).repeat(K, 1)


def object_rows(ids, K, label, alt, ground, ring=2, z0=OR.Z0, q=OR.Q, rows=None, stats=None, band=None):
    """snerf_objects_stats -> (rows (K, 16) int64 holding the u64 words, stats (4) int64).  `ground`: the classes that count as
    ground round an object; `rows` / `stats`: accumulators of earlier calls (fresh ones are made otherwise); `band` = (row0, row1):
    fold the cells of those rows only (default all) -- bands that partition the raster, accumulated into one `rows`, give the words of
    one call.  K == 0 launches nothing."""
    ids = _raster(ids, torch.int32, "ids")
    label = _raster(label, torch.uint8, "label", ids.shape)
    alt = _raster(alt, torch.float32, "alt", ids.shape)
    h, w = ids.shape
    K = int(K)
    if not 0 <= K < 2 ** 31:
        raise ValueError(f"objects: K = {K} outside [0, 2^31)")
    if int(ring) != ring or not 0 <= ring <= MAX_RING:
        raise ValueError(f"objects: ring = {ring!r} outside [0, {MAX_RING}]")
    row0, row1 = (0, h) if band is None else (int(band[0]), int(band[1]))
    table = class_table(ground, "ground")
    rows = new_rows(K, ids.device) if rows is None else rows
    if rows.dtype != torch.int64 or tuple(rows.shape) != (K, ROW_WORDS) or not rows.is_contiguous() or not rows.is_cuda:
        raise ValueError(f"objects: rows must be a contiguous int64 GPU tensor of shape {(K, ROW_WORDS)}")
    stats = torch.zeros(4, dtype=torch.int64, device=ids.device) if stats is None else stats
    _lib.call("snerf_objects_stats", ids, label, alt, h, w, K, table, int(ring), z0, q, row0, row1, rows if K else None, stats,
              exc=ValueError)
    return rows, stats


def _window_origin(grid):
    g = OR.window_grid(grid)
    return float(g.xoff), float(g.yoff), float(g.resolution)


def object_table(rows, grid, z0=OR.Z0, q=OR.Q, terrain_rows=None):
    """per-object columns from the integer words, in fp64 on the host -> a dict of numpy arrays of length K (object n is entry
    n - 1).  `grid`: the lattice of the raster (a DsmGrid, or a _lib.SnerfDsmGrid window: its window offsets are applied).
      class, area_cells, holes (cells without a valid altitude)       int64
      area_m2, perimeter_m                                            area res^2; boundary edges x res
      east, north                                                     the centroid of the cell centres
      bbox (K, 4)                                                     east_min, north_min, east_max, north_max of the cell edges
      alt_mean, alt_min, alt_max                                      over the cells with a valid altitude (NaN without one)
      ground_alt, ground_min                                          mean / min over the ring pairs (NaN without one)
      height = alt_mean - ground_alt, height_max = alt_max - ground_alt
      volume_m3 = (q sum_k + n_valid (z0 - ground_alt)) res^2         the prism over the ground level
    With `terrain_rows` (the words of a second object_rows call over a DTM plane, ring = 0) also
      terrain_alt                                                     the DTM's mean over the footprint (NaN without a valid cell)
      height_over_terrain = alt_mean - terrain_alt
      volume_over_terrain_m3 = n_valid (alt_mean - terrain_alt) res^2 the prism over the terrain under the footprint"""
    r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
    r = r.view(np.int64).reshape(-1, ROW_WORDS)                # sums are signed; every other word is far below 2^63 where it is used
    xoff, yoff, res = _window_origin(grid)
    f = r.astype(np.float64)
    area, nk, ng = f[:, 0], f[:, 7], f[:, 11]
    nan = np.full(len(r), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        has_k, has_g = r[:, 7] > 0, r[:, 11] > 0
        alt_mean = np.where(has_k, z0 + q * (f[:, 8] / nk), nan)
        alt_min = np.where(has_k, z0 + q * (f[:, 9] - _BIAS), nan)
        alt_max = np.where(has_k, z0 + q * (f[:, 10] - _BIAS), nan)
        ground = np.where(has_g, z0 + q * (f[:, 12] / ng), nan)
        ground_min = np.where(has_g, z0 + q * (f[:, 13] - _BIAS), nan)
        east = xoff + (f[:, 1] / area + 0.5) * res
        north = yoff - (f[:, 2] / area + 0.5) * res
    bbox = np.stack([xoff + f[:, 3] * res, yoff - (f[:, 6] + 1.0) * res, xoff + (f[:, 4] + 1.0) * res, yoff - f[:, 5] * res], 1)
    table = {"class": r[:, 15].copy(), "area_cells": r[:, 0].copy(), "area_m2": area * res * res, "east": east, "north": north, "bbox": bbox,
             "perimeter_m": f[:, 14] * res, "alt_mean": alt_mean, "alt_min": alt_min, "alt_max": alt_max, "ground_alt": ground,
             "ground_min": ground_min, "height": alt_mean - ground, "height_max": alt_max - ground,
             "volume_m3": (q * f[:, 8] + nk * (z0 - ground)) * res * res, "holes": r[:, 0] - r[:, 7]}
    if terrain_rows is not None:
        t = terrain_rows.detach().cpu().numpy() if torch.is_tensor(terrain_rows) else np.asarray(terrain_rows)
        t = t.view(np.int64).reshape(-1, ROW_WORDS)
        if len(t) != len(r):
            raise ValueError(f"objects: {len(r)} rows but {len(t)} terrain rows")
        tf = t.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            terrain_alt = np.where(t[:, 7] > 0, z0 + q * (tf[:, 8] / tf[:, 7]), nan)
        table.update(terrain_alt=terrain_alt, height_over_terrain=alt_mean - terrain_alt,
                     volume_over_terrain_m3=nk * (alt_mean - terrain_alt) * res * res)
    return table


def filter_objects(ids, table, min_area_m2=0.0):
    """drop the objects below `min_area_m2` -> (ids with the dropped objects' cells 0 and the others renumbered 1..K' in the same
    order, table with their entries removed): one lookup table, one gather"""
    keep = np.asarray(table["area_m2"]) >= float(min_area_m2)
    lut = np.zeros(len(keep) + 1, np.int32)
    lut[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    out = torch.from_numpy(lut).to(ids.device)[ids.long()]
    return out, {k: np.asarray(v)[keep] for k, v in table.items()}


def objects(label, alt, grid, classes, ground, connectivity=4, ring=2, min_area_m2=0.0, dtm=None):
    """components, object_rows, object_table and filter_objects in one call -> {"ids" (H, W) int32, "n", "table", "object_height"
    (H, W) f32: the height of the cell's object, NaN off objects, "stats": the 4 words of snerf_objects_stats as Python ints}.
    `dtm`: a terrain plane ((H, W) f32, eval/utils/terrain.py) -- one further object_rows call at ring = 0 folds it over the
    footprints and the table gains terrain_alt, height_over_terrain and volume_over_terrain_m3; without it nothing else is launched."""
    ids, K = components(label, classes, connectivity)
    rows, stats = object_rows(ids, K, label, alt, ground, ring)
    terrain_rows = None if dtm is None else object_rows(ids, K, label, dtm, ground, ring=0)[0]
    table = object_table(rows, grid, terrain_rows=terrain_rows)
    ids, table = filter_objects(ids, table, min_area_m2)
    height = torch.from_numpy(np.concatenate([[np.nan], table["height"]]).astype(np.float32)).to(ids.device)
    return {"ids": ids, "n": len(table["class"]), "table": table, "object_height": height[ids.long()],
            "stats": [int(v) for v in stats.cpu()]}


def match_objects(ids_a, n_a, ids_b, n_b):
    """pair the objects of two id rasters on one lattice: a and b match when 2 inter > area_a + area_b - inter, i.e. IoU > 1/2, in
    integers; an object then has at most one partner -> (pairs (M, 2) int64 of (id_a, id_b) in ascending id_a, inter (M,), union
    (M,)).  Plain torch: any device."""
    if tuple(ids_a.shape) != tuple(ids_b.shape):
        raise ValueError(f"match_objects: the id rasters differ in shape: {tuple(ids_a.shape)} and {tuple(ids_b.shape)}")
    a, b = ids_a.reshape(-1).long(), ids_b.reshape(-1).long()
    area_a, area_b = torch.bincount(a, minlength=n_a + 1), torch.bincount(b, minlength=n_b + 1)
    both = (a > 0) & (b > 0)
    key, inter = torch.unique(a[both] * (n_b + 1) + b[both], return_counts=True)
    pa, pb = torch.div(key, n_b + 1, rounding_mode="floor"), key % (n_b + 1)
    union = area_a[pa] + area_b[pb] - inter
    hit = 2 * inter > union
    return torch.stack([pa[hit], pb[hit]], 1), inter[hit], union[hit]


def _f1(matched, n_a, n_b):
    p, r = (matched / n_a if n_a else 0.0), (matched / n_b if n_b else 0.0)
    return {"n_a": int(n_a), "n_b": int(n_b), "matched": int(matched), "precision": p, "recall": r,
            "f1": 2 * p * r / (p + r) if p + r > 0 else 0.0}


def object_scores(table_a, table_b, pairs, inter, union):
    """object-level agreement of map a (the model's) with map b (the ground truth's) from their tables and match_objects' result:
    n_a, n_b, matched, precision (matched / n_a), recall (matched / n_b), f1; iou_mean and area_ratio_mean (area_a / area_b) over the
    matches; height_mae, height_median_abs, height_bias (a - b) over the matches whose two heights are finite (None without one);
    per_class: the counts by class (matches by the class of b); class_confusions: the pairs that overlap by IoU > 1/2 but differ in
    class -- reported, not counted as matched."""
    pairs = np.asarray(pairs.cpu() if torch.is_tensor(pairs) else pairs, np.int64).reshape(-1, 2)
    inter = np.asarray(inter.cpu() if torch.is_tensor(inter) else inter, np.float64)
    union = np.asarray(union.cpu() if torch.is_tensor(union) else union, np.float64)
    cls_a, cls_b = np.asarray(table_a["class"]), np.asarray(table_b["class"])
    ia, ib = pairs[:, 0] - 1, pairs[:, 1] - 1
    same = cls_a[ia] == cls_b[ib]
    out = _f1(int(same.sum()), len(cls_a), len(cls_b))
    out["class_confusions"] = [{"a": int(a + 1), "b": int(b + 1), "class_a": int(cls_a[a]), "class_b": int(cls_b[b])}
                               for a, b in zip(ia[~same], ib[~same])]
    ia, ib, iou = ia[same], ib[same], inter[same] / union[same]

    def mean(v):
        return float(np.mean(v)) if len(v) else None

    out["iou_mean"] = mean(iou)
    out["area_ratio_mean"] = mean(np.asarray(table_a["area_cells"], np.float64)[ia] / np.asarray(table_b["area_cells"], np.float64)[ib])
    d = np.asarray(table_a["height"], np.float64)[ia] - np.asarray(table_b["height"], np.float64)[ib]
    d = d[np.isfinite(d)]
    out["height_pairs"] = int(len(d))
    out["height_mae"], out["height_bias"] = mean(np.abs(d)), mean(d)
    out["height_median_abs"] = float(np.median(np.abs(d))) if len(d) else None
    out["per_class"] = {int(c): _f1(int((cls_b[ib] == c).sum()), int((cls_a == c).sum()), int((cls_b == c).sum()))
                        for c in sorted(set(cls_a.tolist()) | set(cls_b.tolist()))}
    return out


def table_records(table):
    """the table as a list of JSON-ready records (object n is record n - 1, with "id": n); a non-finite value is None"""
    def plain(v):
        if isinstance(v, np.ndarray):
            return [plain(x) for x in v]
        if isinstance(v, (np.integer, int)):
            return int(v)
        v = float(v)
        return v if np.isfinite(v) else None
    n = len(table["class"])
    return [dict({"id": k + 1}, **{name: plain(col[k]) for name, col in table.items()}) for k in range(n)]
