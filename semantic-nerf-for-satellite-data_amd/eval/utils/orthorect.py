"""Orthorectification: the scene's OWN images and labels on the map -- a true ortho-image per date, the multi-date mosaic, and the
voted ground-truth class raster in the scene's label set, against which a model's land-cover map is scored in map space.  The
reference has no counterpart; the spec is include/snerf_orthorect.h, the stage is
the kernel of csrc/orthorect.hip, torch is plumbing.  All functions take and return device tensors; there is no CPU fallback.

rectify walks the lattice of a DSM -- the model's (ortho_products(...)["dsm"], nadir_products' "dsm") or the lidar ground truth
(dataset.dsm["gt"]): any (H, W) fp32 plane with its grid.  Every cell is projected into every image (UTM -> lat / lon -> RPC), the
colour is sampled bilinearly, the label at the nearest pixel, and both are fused into integer accumulators (sums quantised to
2^-24, counts, votes): the result does not depend on the order of the images or on how they are cut into calls of 64.

Occlusion: a cell is HIDDEN from an image when the DSM blocks the line of sight towards the satellite -- snerf_shadow_cast's march
with a view row in place of a sun row (view_rows, visibility).  One direction per image is an approximation: the line of sight
turns by about scene width / orbit height across the scene (measured on the fixture: DESIGN.md section 5t).

map_agreement scores a model's map products (ortho_products / nadir_products on the same grid) against the mosaic: PSNR of the
colour, and the confusion matrix, accuracy and mIoU of a label plane against the voted labels.

The int64 colour sums cannot wrap while |pixel| * (images seeing a cell) < 2^38; image values lie in [0, 1].

Out of scope: a per-cell median over the dates, a best-view mosaic, a per-cell view direction, sub-pixel footprint integration,
radiometric normalisation between dates, rectified images as training targets, sharding the images over ranks (the accumulators
are integer words and would combine by a SUM all-reduce)."""
import math

import numpy as np
import torch

from ... import _lib
from ...baseline.components.camera_models import RPCModel, struct_to_device
from ...framework.util.conversions import utm_from_latlon
from . import dsm as D
from . import metrics, shadow
from .ortho import finish_votes, window_grid
from .semantic import normalized_confusion, semantic_miou

MAX_IMAGES = _lib.RECT_MAX_IMAGES
SEEN, HOLE, OUTSIDE, HIDDEN = _lib.RECT_SEEN, _lib.RECT_HOLE, _lib.RECT_OUTSIDE, _lib.RECT_HIDDEN
STATES = ("seen", "hole", "outside", "hidden")
NO_LABEL = _lib.ORTHO_NO_LABEL
Q = 2.0 ** -24       # quantisation step of the colour sums (the DSM rasteriser's)
NADIR_REL = 1e-9     # an image whose line of sight travels less than this times the altitude range horizontally is nadir


def _per_image(v, n, what):
    v = [float(v)] * n if np.isscalar(v) else [float(x) for x in v]
    if len(v) != n:
        raise ValueError(f"view_rows: {len(v)} {what} values for {n} images")
    return v


def view_rows(cams, alt_min, alt_max, sizes, geo, res):
    """The (n_images, 3) fp64 rows (ux, uy, rise) of the images' lines of sight, in exactly the form of snerf_shadow_cast's sun rows
    and pointing TOWARDS THE SATELLITE: the centre pixel ((w - 1) / 2, (h - 1) / 2) of image k is localised at alt_min and at
    alt_max (cams[k].localization, on the device), both points are taken to UTM in `geo`'s zone, and with (de, dn) their
    difference and dh its length: ux = de / dh (east = +column), uy = -dn / dh (north = -row), rise = (alt_max - alt_min) / dh *
    res metres per cell of horizontal travel.  An image with dh < 1e-9 (alt_max - alt_min) is nadir: its row is NaN (visibility
    casts nothing for it).  `cams`: RPCModels; `alt_min` / `alt_max`: a value or one per image; `sizes`: (w, h) per image."""
    n = len(cams)
    if not n or len(sizes) != n:
        raise ValueError(f"view_rows: {n} cameras and {len(sizes)} sizes")
    lo, hi = _per_image(alt_min, n, "alt_min"), _per_image(alt_max, n, "alt_max")
    res = float(res)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"view_rows: res = {res} must be positive and finite")
    rows = np.full((n, 3), np.nan)
    for k, (cam, (w, h)) in enumerate(zip(cams, sizes)):
        if not (math.isfinite(lo[k]) and math.isfinite(hi[k]) and lo[k] < hi[k]):
            raise ValueError(f"view_rows: image {k} needs finite alt_min < alt_max, got {lo[k]} and {hi[k]}")
        col, row = (int(w) - 1) / 2.0, (int(h) - 1) / 2.0
        lon, lat = cam.localization([col, col], [row, row], [lo[k], hi[k]])
        east, north, _ = utm_from_latlon(lat, lon, geo.zone_string)
        (e0, e1), (n0, n1) = east.cpu().tolist(), north.cpu().tolist()
        de, dn = e1 - e0, n1 - n0
        dh = math.hypot(de, dn)
        if dh >= NADIR_REL * (hi[k] - lo[k]):
            rows[k] = (de / dh, -dn / dh, (hi[k] - lo[k]) / dh * res)
    return rows


def visibility(dsm, rows, bias=0.0):
    """(n_images, H, W) u8: snerf_shadow_cast's lit_out of `dsm` under the view rows (1 = the satellite sees the cell, 0 = the DSM
    blocks the line of sight, 255 = the cell is a hole); the plane of a nadir image (a NaN row) is all 1.  `bias` (metres) lifts
    the start of every march, as for cast shadows."""
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    if not len(rows):
        raise ValueError("visibility: no image")
    slant = ~np.isnan(rows).any(1)
    out = torch.ones((len(rows),) + tuple(dsm.shape), dtype=torch.uint8, device=dsm.device)
    if slant.all():
        return shadow.cast_rows(dsm, rows, bias)
    if slant.any():
        out[torch.from_numpy(np.nonzero(slant)[0]).to(dsm.device)] = shadow.cast_rows(dsm, rows[slant], bias)
    return out


def _camera(img, device):
    cam = img.get("cam")
    if cam is None:
        raise ValueError(f"rectify: image {img.get('name')!r} carries no 'cam' (an RPCModel or an rpcm dict)")
    return cam if isinstance(cam, RPCModel) else RPCModel(cam["rpc"] if "rpc" in cam else cam, device=device)


def _column(t, n, dtype, width, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"rectify: {what} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or t.numel() != n * width:
        raise ValueError(f"rectify: {what} must hold {n} x {width} values of {dtype}, not {t.numel()} of {t.dtype}")
    return t.contiguous()


def _rows_in_place(cols, row_bytes):
    """per-image columns that are slices of ONE tensor (what the loaders hand out): (base address, first row of every image), else
    None"""
    store = cols[0].untyped_storage().data_ptr()
    if any(c.untyped_storage().data_ptr() != store for c in cols):
        return None
    base = min(c.data_ptr() for c in cols)
    offs = [c.data_ptr() - base for c in cols]
    return (base, [o // row_bytes for o in offs]) if all(o % row_bytes == 0 for o in offs) else None


def _pack(rgbs, labels):
    """the pixels of a call's images as ONE (n_rows, 3) fp32 array and ONE (n_rows) u8 array that the kernel indexes by row:
    (rgbs base, labels base or None, row0 per image, n_rows, what must stay alive).  Slices of the bank's tensors are addressed in
    place when both columns are laid out alike; anything else is concatenated."""
    n = [t.numel() // 3 for t in rgbs]
    a = _rows_in_place(rgbs, 12)
    b = _rows_in_place(labels, 1) if labels is not None else None
    if a is not None and (labels is None or (b is not None and b[1] == a[1])):
        return a[0], b[0] if b else None, a[1], max(r + m for r, m in zip(a[1], n)), (rgbs, labels)
    whole = torch.cat([t.reshape(-1, 3) for t in rgbs])
    lwhole = torch.cat([t.reshape(-1) for t in labels]) if labels is not None else None
    row0 = np.cumsum([0] + n[:-1]).tolist()
    return whole.data_ptr(), lwhole.data_ptr() if labels is not None else None, row0, sum(n), (whole, lwhole)


def dataset_images(dataset):
    """the per-image dicts rectify takes, from a loaded SatNeRFDataset / SemanticDataset: name, w, h, alt_min, alt_max, rgbs,
    semantic (a semantic scene) and cam"""
    out, lo = [], 0
    for it, meta in zip(dataset.items, dataset.metas):
        hi = lo + it["n"]
        d = {"name": it["name"], "w": it["w"], "h": it["h"], "alt_min": it["alt_min"], "alt_max": it["alt_max"],
             "rgbs": dataset.t["rgbs"][lo:hi], "cam": RPCModel(meta["rpc"], device=dataset.device)}
        if "semantic" in dataset.t:
            d["semantic"] = dataset.t["semantic"][lo:hi]
        out.append(d)
        lo = hi
    return out


@torch.no_grad()
def rectify(dsm, grid, geo, images, n_classes=None, occlusion=True, keep_images=False, bias=0.0):
    """Orthorectify `images` on `dsm` ((H, W) fp32 on the GPU, NaN = a hole) whose lattice is `grid` (a DsmGrid of H x W cells, or a
    window of one from dsm.grid_struct) in `geo`'s UTM zone (a GeoFrame).

    `images`: the per-image dicts the test bank hands out -- "rgbs" (w h, 3) fp32, "w", "h"[, "semantic" (w h[, 1]) uint8] -- plus
    "cam" (the image's RPCModel, or its rpcm dict) and, for the occlusion, "alt_min" / "alt_max" (dataset_images builds them from
    a loaded dataset).  `n_classes`: the label set's size; None leaves the labels out.  `occlusion`: cast the DSM against every
    image's view row (view_rows, visibility; `bias` metres lift the marches' starts) and leave HIDDEN cells out; False takes every
    cell inside an image as seen.  The split is cut into calls of at most 64 images.

    Returns {"grid": DsmGrid of the window, "rgb": (3, H, W) f32 -- the mean colour of the images that see a cell, NaN where none
    does --, "count": (H, W) int32 -- how many do --, "states": {"seen", "hole", "outside", "hidden"}: the (image, cell) totals[,
    "label_vote": (H, W) u8 (255 = no vote), "vote_share": (H, W) f32, "max_votes"][, "view_rows": (n, 3)][, with `keep_images`:
    "images": {"rgb": (n, 3, H, W) f32 (NaN where not seen), "state": (n, H, W) u8[, "label": (n, H, W) u8]}]}."""
    dsm = shadow._dsm(dsm, "rectify")
    g = D.grid_struct(grid)
    h, w = dsm.shape
    if (g.out_h, g.out_w) != (h, w):
        raise ValueError(f"rectify: a DSM of {h} x {w} cells on a window of {g.out_h} x {g.out_w}")
    images = list(images)
    n = len(images)
    if not n:
        raise ValueError("rectify: no image")
    dev = dsm.device
    cells = D.cell_count(g, "a map")
    with_labels = n_classes is not None
    if with_labels and not 1 <= n_classes <= _lib.ORTHO_MAX_CLASSES:
        raise ValueError(f"rectify: n_classes must lie in [1, {_lib.ORTHO_MAX_CLASSES}]")
    cams = [_camera(img, dev) for img in images]
    sizes = [(int(img["w"]), int(img["h"])) for img in images]
    rgbs = [_column(img.get("rgbs"), wi * hi, torch.float32, 3, f"'rgbs' of image {k}") for k, (img, (wi, hi)) in enumerate(zip(images, sizes))]
    labels = None
    if with_labels:
        if any(img.get("semantic") is None for img in images):
            raise ValueError("rectify: n_classes given, but an image carries no 'semantic' labels")
        labels = [_column(img["semantic"], wi * hi, torch.uint8, 1, f"'semantic' of image {k}") for k, (img, (wi, hi)) in enumerate(zip(images, sizes))]
    rows = None
    if occlusion:
        if any("alt_min" not in img or "alt_max" not in img for img in images):
            raise ValueError("rectify: the occlusion needs every image's 'alt_min' and 'alt_max' (or pass occlusion=False)")
        rows = view_rows(cams, [img["alt_min"] for img in images], [img["alt_max"] for img in images], sizes, geo, g.res)

    total = torch.zeros((3, cells), dtype=torch.int64, device=dev)
    count = torch.zeros(cells, dtype=torch.int32, device=dev)
    votes = torch.zeros((n_classes, cells), dtype=torch.int32, device=dev) if with_labels else None
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    kept = None
    if keep_images:
        kept = {"rgb": torch.empty((n, 3, h, w), dtype=torch.float32, device=dev), "state": torch.empty((n, h, w), dtype=torch.uint8, device=dev)}
        if with_labels:
            kept["label"] = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    for k in range(0, n, MAX_IMAGES):
        m = min(MAX_IMAGES, n - k)
        base, lbase, row0, n_rows, alive = _pack(rgbs[k:k + m], labels[k:k + m] if with_labels else None)
        table = (_lib.SnerfRectImage * m)()
        for s in range(m):
            table[s].rpc, table[s].row0 = cams[k + s].struct, row0[s]
            table[s].w, table[s].h = sizes[k + s]
        table_dev = struct_to_device(table, dev)
        vis = visibility(dsm, rows[k:k + m], bias) if occlusion else None
        _lib.call("snerf_orthorectify", dsm, g, geo.params.lon0, geo.params.south, table, table_dev, m, base, lbase, n_rows,
                  n_classes if with_labels else 0, vis, total, count, votes, None, kept["rgb"][k:k + m] if kept else None,
                  kept["label"][k:k + m] if kept and with_labels else None, kept["state"][k:k + m] if kept else None, stats,
                  exc=ValueError)
        del alive, table_dev, vis
    rgb = torch.empty((3, h, w), dtype=torch.float32, device=dev)
    fstats = D.new_stats(dev)
    for ch in range(3):
        _lib.call("snerf_dsm_finish", count, total[ch], cells, 0.0, Q, rgb[ch], fstats)
    out = {"grid": window_grid(grid), "rgb": rgb, "count": count.reshape(h, w),
           "states": dict(zip(STATES, (int(v) for v in stats.cpu())))}
    if with_labels:
        out["label_vote"], out["vote_share"], vstats = finish_votes(votes, h, w)
        out["max_votes"] = int(vstats[1])
    if rows is not None:
        out["view_rows"] = rows
    if kept:
        out["images"] = kept
    return out


def map_agreement(pred_rgb, pred_label, mosaic, n_classes, ignore=NO_LABEL):
    """A model's map against the rectified mosaic (`mosaic`: what rectify returns, on the same lattice).
    pred_rgb (3, H, W) f32 or None: "psnr" -- metrics.psnr over the cells where both colours are finite in every channel -- and
    "psnr_cells".  pred_label (H, W) u8 or None: "confusion" -- the n_classes x n_classes counts [voted label][predicted label]
    over the cells where both labels lie below n_classes and differ from `ignore`, from torch.bincount on the device --,
    "accuracy" (the trace over the total), "mIoU" (semantic.semantic_miou of the row-normalised matrix, as the per-image
    evaluation) and "label_cells".  An empty comparison gives NaN."""
    out = {}
    if pred_rgb is not None:
        ref = mosaic["rgb"]
        if tuple(pred_rgb.shape) != tuple(ref.shape):
            raise ValueError(f"map_agreement: a colour map {tuple(pred_rgb.shape)} against a mosaic {tuple(ref.shape)}")
        both = torch.isfinite(pred_rgb).all(0) & torch.isfinite(ref).all(0)
        cells = int(both.sum())
        out["psnr_cells"] = cells
        out["psnr"] = float(metrics.psnr(pred_rgb.permute(1, 2, 0), ref.permute(1, 2, 0), both)) if cells else math.nan
    if pred_label is not None:
        if "label_vote" not in mosaic:
            raise ValueError("map_agreement: the mosaic carries no voted labels (rectify without n_classes)")
        ref = mosaic["label_vote"]
        if tuple(pred_label.shape) != tuple(ref.shape):
            raise ValueError(f"map_agreement: a label map {tuple(pred_label.shape)} against a mosaic {tuple(ref.shape)}")
        p, r = pred_label.reshape(-1).long(), ref.reshape(-1).long()
        both = (p < n_classes) & (r < n_classes) & (p != ignore) & (r != ignore)
        conf = torch.bincount(r[both] * n_classes + p[both], minlength=n_classes * n_classes).reshape(n_classes, n_classes).cpu().numpy()
        cells = int(conf.sum())
        out["confusion"] = conf.tolist()
        out["label_cells"] = cells
        out["accuracy"] = float(np.trace(conf)) / cells if cells else math.nan
        out["mIoU"] = semantic_miou(normalized_confusion(conf)) if cells else math.nan
    return out
