"""Geo-referenced ortho products: the colour, the class and the votes of a semantic satellite NeRF ON THE MAP -- a true
ortho-image, a land-cover map and the fusion of a scene's views into one raster, on the lattice of the DSM rasteriser
(eval/utils/dsm.py).  The reference has no counterpart; the spec is the ortho section of include/snerf_hip.h (DESIGN.md section
5j), the stages are the kernels of csrc/ortho.hip, torch is plumbing.  All functions take and return device tensors.

Top surface -- every point of a UTM (east, north, alt) cloud offers a 64-bit key to the cells of its (2 radius + 1)^2 window:
(round((z - Z0)/Q) + 2^31) << 32 | (2^32 - 1 - global point index), folded with an integer atomic max.  The highest quantised
altitude wins a cell, the lowest index on a tie; 0 means no point.  Keys commute, so a map does not depend on launch order, on
how a cloud is cut into calls, on the order of the images, or on ranks (a MAX all-reduce of `top` would combine them).  Z0 and Q
are constants (all ranks agree): Q = 2^-16 m keeps 2^32 steps over +-32,768 m, and 15 um is below the fp32 spacing of any
altitude above 128 m -- the key holds the altitude in 32 bits where the DSM's int64 sums afford 2^-24.

Gather -- per cell the winner's altitude and global index; colour, label or any per-point scalar are copied only where the
winner belongs to the image of the call ([index0, index0 + n)), so a fused map gathers once per image into shared buffers.

Votes -- every point adds 1 to votes[label][cell] over the same window (integer atomic add); finish_votes gives the argmax
(the lowest class on a tie, 255 for a cell without a vote) and the winner's share of the cell's votes.

ortho_products walks a set of images and returns the fused map; eval/ortho.py writes it (PNG and GeoTIFF).  A splatted map has
cells no view's point reaches, and its occlusion is "the highest point wins".  With robust=True it adds the per-cell quartiles of
the views' altitudes (eval/utils/fuse.py): the median surface, its colour and label, and the spread.

nadir_products asks the model instead: one vertical ray per cell of the lattice
(baseline/components/rays.py nadir_construct, through GeoFrame.to_scene), rendered under a chosen sun -- a DSM without holes, a
true nadir ortho-image, the shadow map and the top-surface label, with occlusion resolved by the renderer.

Out of scope: finite-sigma splats, slanted or perspective map cameras, RPC tags.  Map-space accuracy is eval/utils/orthorect.py: the
ground-truth class raster is the scene's own labels, orthorectified and voted (the US3D classes of dsm_cls_fp are not the scene's
label set).

nadir_sun_sweep renders that map under a list of suns in one walk: per chunk one full pass and one relight
per further sun -- the shadow maps of a day, or the scene lit as each of its acquisitions saw it."""
import torch

from ... import _lib
from ...framework.components.rendering import n_render_samples
from . import dsm as D
from .dsm import grid_struct, new_stats      # the lattice plumbing is the DSM's

Z0 = 0.0             # quantisation origin of the key's altitude (metres)
Q = 2.0 ** -16       # quantisation step (metres): 2^32 steps span +-32,768 m
NO_LABEL = _lib.ORTHO_NO_LABEL
MAX_INDEX = 2 ** 32 - 1


def _cloud(cloud):
    if not (torch.is_tensor(cloud) and cloud.is_cuda):
        raise ValueError("ortho: the cloud must be a GPU tensor (the HIP path has no CPU fallback)")
    return D.cloud_f64(cloud)


def _cells(g):
    return D.cell_count(g, "a map")


def top_surface(cloud, grid, radius=0, index0=0, top=None, stats=None):
    """fold `cloud` (N, 3) (east, north, alt) into the top-surface keys of `grid` -> (top (out_h, out_w) int64 holding the
    u64 words, stats).  `index0`: the global index of the cloud's first point (the running ray offset of a fused map);
    `top` / `stats`: accumulators of earlier calls (zeroed ones are made otherwise)."""
    g = grid_struct(grid)
    xyz = _cloud(cloud)
    if top is None:
        top = torch.zeros((g.out_h, g.out_w), dtype=torch.int64, device=xyz.device)
    if top.dtype != torch.int64 or top.numel() != _cells(g):
        raise ValueError(f"top must hold {g.out_h} x {g.out_w} int64 words")
    stats = new_stats(xyz.device) if stats is None else stats
    _lib.call("snerf_ortho_top", xyz, xyz.shape[0], index0, g, radius, Z0, Q, top, stats, exc=ValueError)
    return top, stats


def gather(top, index0, n, rgb=None, labels=None, scalar=None, out=None):
    """the winners of `top`: {"alt" f32 (NaN where empty), "index" int64 (-1 where empty)[, "rgb" (3, ...) f32, "label" u8,
    "scalar" f32]}, shaped like `top`.  Payload rows are those of the points [index0, index0 + n): rgb (n, 3) fp32, labels (n)
    int64 (a label outside [0, 254] is written as 255), scalar (n) fp32; their outputs are written only in the cells those
    points won.  `out`: buffers of an earlier call to go on writing into (a fused map); fresh payload buffers are pre-filled
    with NaN / 255."""
    shape, dev = tuple(top.shape), top.device
    cells = top.numel()
    out = dict(out) if out else {}
    fills = {"alt": (torch.float32, shape, float("nan")), "index": (torch.int64, shape, -1),
             "rgb": (torch.float32, (3,) + shape, float("nan")), "label": (torch.uint8, shape, NO_LABEL),
             "scalar": (torch.float32, shape, float("nan"))}
    given = {"rgb": rgb, "label": labels, "scalar": scalar}
    for k, (dt, shp, fill) in fills.items():
        if k in ("alt", "index") or given[k] is not None:
            if k not in out:
                out[k] = torch.full(shp, fill, dtype=dt, device=dev)
            elif out[k].dtype != dt or tuple(out[k].shape) != shp or not out[k].is_contiguous():
                raise ValueError(f"gather: out['{k}'] must be a contiguous {dt} tensor of shape {shp}")
    want = {"rgb": (torch.float32, 3 * n), "label": (torch.int64, n), "scalar": (torch.float32, n)}
    args = []
    for k in ("rgb", "label", "scalar"):
        t = given[k]
        if t is not None:
            if t.dtype != want[k][0] or t.numel() != want[k][1]:
                raise ValueError(f"gather: '{k}' must hold {want[k][1]} values of {want[k][0]}, not {t.numel()} of {t.dtype}")
            t = t.contiguous()
        args.append(t)
    _lib.call("snerf_ortho_gather", top.contiguous(), cells, index0, n, Z0, Q, *args, out["alt"], out["index"],
              *(out[k] if given[k] is not None else None for k in ("rgb", "label", "scalar")), exc=ValueError)
    return out


def label_votes(cloud, labels, grid, n_classes, radius=0, votes=None, stats=None):
    """add the cloud's label votes: -> (votes (n_classes, out_h, out_w) int32 holding the u32 counts, stats); labels (N) int64"""
    g = grid_struct(grid)
    xyz = _cloud(cloud)
    labels = labels.reshape(-1)
    if labels.dtype != torch.int64 or labels.shape[0] != xyz.shape[0]:
        raise ValueError(f"label_votes: {xyz.shape[0]} int64 labels expected, got {labels.shape[0]} of {labels.dtype}")
    cells = _cells(g)
    if votes is None:
        if not 1 <= n_classes <= _lib.ORTHO_MAX_CLASSES:
            raise ValueError(f"n_classes must lie in [1, {_lib.ORTHO_MAX_CLASSES}]")
        votes = torch.zeros((n_classes, g.out_h, g.out_w), dtype=torch.int32, device=xyz.device)
    if votes.dtype != torch.int32 or votes.numel() != n_classes * cells:
        raise ValueError(f"votes must hold {n_classes} x {g.out_h} x {g.out_w} int32 words")
    stats = new_stats(xyz.device) if stats is None else stats
    _lib.call("snerf_ortho_votes", xyz, labels.contiguous(), xyz.shape[0], g, radius, n_classes, votes, stats, exc=ValueError)
    return votes, stats


def finish_votes(votes, h, w, stats=None):
    """(label (h, w) u8: the class with the most votes, the lowest on a tie, 255 without a vote; share (h, w) f32: the
    winner's share of the cell's votes, NaN without one; stats, whose word 1 holds the largest total of a cell)"""
    if votes.dtype != torch.int32 or votes.numel() % (h * w) or not votes.numel():
        raise ValueError(f"votes must hold n_classes x {h} x {w} int32 words")
    n_classes = votes.numel() // (h * w)
    label = torch.empty((h, w), dtype=torch.uint8, device=votes.device)
    share = torch.empty((h, w), dtype=torch.float32, device=votes.device)
    stats = new_stats(votes.device) if stats is None else stats
    _lib.call("snerf_ortho_votes_finish", votes.contiguous(), n_classes, h * w, label, share, stats, exc=ValueError)
    return label, share, stats


def _flat(img, key):
    t = img.get(key)
    return t.reshape(-1, t.shape[-1]) if t is not None else None


@torch.no_grad()
def ortho_products(cfgs, renderer, models, images, geo=None, roi=None, resolution=D.RESOLUTION, radius=0, dsm_radius=1,
                   sharded=False, grid=None, render_options={}, depth_mode="mean", robust=False, gt=None, water_mask=None,
                   ignore_mask=None):
    """The fused map of `images` (dicts with the evaluators' keys: "rays", "extras"[, "dsm": {"geo": GeoFrame}]).

    Per image, in the order given: lean_inference (sharded_lean_inference with `sharded`: every rank then holds the whole
    frame, and nothing is all-reduced here) for rgb, depth and, when the model has classes, the label; geo.cloud(rays, depth)
    (`geo` defaults to the image's "dsm"["geo"]); the cloud folded into the shared accumulators -- the top-surface keys with
    index0 = the running ray offset, the label votes, and the DSM's count / sum (dsm._accumulate, radius `dsm_radius`).
    The grid: `grid` (a DsmGrid), else the ROI grid of `roi` (a DsmGrid or the roi_txt meta) used as the lattice, else the
    bounds grid of the union of the clouds' exact bounds -- known only after every image has been rendered, so the frames'
    rgb, depth and labels are kept and the clouds are made again (one launch each) for the fold; nothing is rendered twice.
    Then one gather per image and the finishes.  `render_options` go to the renderer: as everywhere in evaluation it jitters the
    sample depths from torch's generator unless {"perturb": 0} (or a pinned "perturb_rand") says otherwise, so two walks give the
    same map only from the same generator state.  `depth_mode="median"` builds every cloud, hence every product, from the rays'
    median depths (SNERF_FLAG_DEPTH_MEDIAN) instead of the expected depths.

    Returns {"grid": DsmGrid, "dsm": (H, W) f32 -- the mean DSM, the bits of dsm.rasterize on the concatenated cloud --,
    "top_alt": (H, W) f32, "top_index": (H, W) int64 (index into the concatenated rays, -1 where empty), "rgb": (3, H, W) f32
    (NaN where empty)[, "label_top": (H, W) u8, "label_vote": (H, W) u8, "vote_share": (H, W) f32], "n_points", "bad_points"
    (altitudes that are not finite or beyond +-32,768 m: left out of the top surface), "bad_labels" (labels outside the
    model's classes: no vote), "max_votes"}.

    `robust=True` adds the order statistics of the views' altitudes per cell (eval/utils/fuse.py), on the top
    surface's `radius`, Z0 and Q: every cloud is made again by one launch for the count walk and once more for the scatter walk
    (nothing is rendered twice), then "median_alt" (H, W) f32 -- the lower median, an actual point --, "median_index" (H, W) int64,
    "rgb_median" (3, H, W) f32[, "label_median" (H, W) u8] gathered once per image from the median words as the top surface's are
    from its words, "alt_q1" / "alt_q3" (H, W) f32, "alt_spread" (H, W) f32 (q3 - q1, exact in the quantised altitudes: where the
    views agree) and "offers" (H, W) int32 (the points that offered themselves to a cell).  With `gt` (H, W) on the product's lattice
    (and `water_mask` / `ignore_mask`, as nadir_products takes them; robust only): "mae": {"dsm", "top_alt", "median_alt"}, each
    {"mean", "median"} of dsm.compute_mae with the same masks.  Without `robust` no fuse entry is called and the result is what
    it was."""
    from .util import lean_inference, sharded_lean_inference, with_depth_mode
    if gt is not None and not robust:
        raise ValueError("ortho_products: gt= scores the fused surfaces and needs robust=True")
    render_options = with_depth_mode(render_options, depth_mode, "ortho_products")
    images = list(images)
    if not images:
        raise ValueError("ortho_products: no image")
    model = models["coarse"]
    n_classes = model.spec.n_classes
    if n_classes > _lib.ORTHO_MAX_CLASSES:
        raise ValueError(f"ortho_products: {n_classes} classes, at most {_lib.ORTHO_MAX_CLASSES} fit a uint8 label map")
    infer = sharded_lean_inference if sharded else lean_inference
    keys = ("rgb_coarse", "depth_coarse") + (("semantic_label_coarse",) if n_classes else ())
    if grid is None and roi is not None:
        grid = roi if isinstance(roi, D.DsmGrid) else D.roi_grid(roi)

    acc = {}

    def fold(cloud, labels, index0):
        if not acc:
            acc.update(g=grid_struct(grid), top=None, tstats=new_stats(cloud.device), votes=None, vstats=new_stats(cloud.device),
                       dsm=None)
        acc["top"], _ = top_surface(cloud, acc["g"], radius, index0, acc["top"], acc["tstats"])
        if n_classes:
            acc["votes"], _ = label_votes(cloud, labels, acc["g"], n_classes, radius, acc["votes"], acc["vstats"])
        acc["dsm"] = D._accumulate(cloud, acc["g"], None, dsm_radius, acc["dsm"])

    frames, index0 = [], 0
    ext = [float("inf"), float("-inf"), float("inf"), float("-inf")]
    for img in images:
        rays, extras = _flat(img, "rays"), _flat(img, "extras")
        g_img = geo if geo is not None else (img.get("dsm") or {}).get("geo")
        if g_img is None:
            raise ValueError(f"ortho_products: image {img.get('name')!r} carries no 'dsm'['geo'] and no geo= was given")
        if index0 + rays.shape[0] > MAX_INDEX:
            raise ValueError(f"ortho_products: more than {MAX_INDEX} rays do not fit the key's 32-bit index")
        res = infer(cfgs, renderer, models, rays, extras, keys=keys, render_options=render_options)
        f = {"rays": rays, "geo": g_img, "index0": index0, "n": rays.shape[0], "rgb": res["rgb_coarse"],
             "depth": res["depth_coarse"], "labels": res.get("semantic_label_coarse")}
        cloud, b = g_img.cloud(rays, f["depth"])
        ext = [min(ext[0], b.xmin), max(ext[1], b.xmax), min(ext[2], b.ymin), max(ext[3], b.ymax)]
        if grid is not None:
            fold(cloud, f["labels"], index0)
        del cloud
        frames.append(f)
        index0 += f["n"]
    if grid is None:
        grid = D.dsm_grid_from_cloud(None, resolution, bounds=tuple(ext))
        for f in frames:
            fold(f["geo"].cloud(f["rays"], f["depth"])[0], f["labels"], f["index0"])
    h, w = acc["g"].out_h, acc["g"].out_w
    out = None
    for f in frames:
        out = gather(acc["top"], f["index0"], f["n"], rgb=f["rgb"], labels=f["labels"], out=out)
    res = {"grid": grid if isinstance(grid, D.DsmGrid) else D.DsmGrid(grid.xoff, grid.yoff, grid.res, grid.xsize, grid.ysize),
           "dsm": D._finish(*acc["dsm"], h, w), "top_alt": out["alt"], "top_index": out["index"],
           "rgb": out["rgb"], "n_points": index0}
    bad_points = int(acc["tstats"][0])
    if n_classes:
        res["label_top"] = out["label"]
        res["label_vote"], res["vote_share"], vstats = finish_votes(acc["votes"], h, w, acc["vstats"])
        bad_labels, max_votes = (int(v) for v in vstats[:2].cpu())
        if max_votes >= 2 ** 32:
            raise OverflowError(f"ortho_products: a cell received {max_votes} votes, its u32 counts could have wrapped")
        res.update(bad_labels=bad_labels, max_votes=max_votes)
    res["bad_points"] = bad_points
    if robust:
        from . import fuse as F
        words, count, _ = F.fuse_walks(lambda: ((f["geo"].cloud(f["rays"], f["depth"])[0], f["index0"]) for f in frames), acc["g"], radius)
        med = None
        for f in frames:
            med = gather(words[1], f["index0"], f["n"], rgb=f["rgb"], labels=f["labels"], out=med)
        res.update(median_alt=med["alt"], median_index=med["index"], rgb_median=med["rgb"], alt_q1=gather(words[0], 0, 1)["alt"],
                   alt_q3=gather(words[2], 0, 1)["alt"], alt_spread=F.spread(words[0], words[2]), offers=count)
        if n_classes:
            res["label_median"] = med["label"]
        if gt is not None:
            res["mae"] = {}
            for key in ("dsm", "top_alt", "median_alt"):
                mae = D.compute_mae(res[key], gt, water_mask=water_mask, ignore_mask=ignore_mask)
                res["mae"][key] = {"mean": mae["mean"], "median": mae["median"]}
    return res


def window_grid(grid):
    """the lattice of a window as a DsmGrid of its own: a DsmGrid as it is, a _lib.SnerfDsmGrid (dsm.grid_struct) by its window"""
    if isinstance(grid, D.DsmGrid):
        return grid
    return D.DsmGrid(grid.xoff + grid.ioff * grid.res, grid.yoff - grid.joff * grid.res, grid.res, grid.out_w, grid.out_h)


def _nadir_defaults(dataset, geo, roi, gt, water_mask, ignore_mask, min_alt, max_alt, sun_elevation, sun_azimuth):
    """what a loaded dataset (baseline/dataset/satnerf_dataset.py) supplies when the caller does not: its GeoFrame, its "dsm"
    entry (roi, gt, masks), the altitude range of the split's images and the sun of the first one"""
    if dataset is not None:
        geo = dataset.geo if geo is None else geo
        entry = dataset.dsm or {}
        if roi is None and gt is None:
            roi, gt = entry.get("roi"), entry.get("gt")
            water_mask = entry.get("water_mask") if water_mask is None else water_mask
            ignore_mask = entry.get("ignore_mask") if ignore_mask is None else ignore_mask
        min_alt = min(it["alt_min"] for it in dataset.items) if min_alt is None else min_alt
        max_alt = max(it["alt_max"] for it in dataset.items) if max_alt is None else max_alt
        sun_elevation = float(dataset.metas[0]["sun_elevation"]) if sun_elevation is None else sun_elevation
        sun_azimuth = float(dataset.metas[0]["sun_azimuth"]) if sun_azimuth is None else sun_azimuth
    missing = [k for k, v in (("geo", geo), ("min_alt", min_alt), ("max_alt", max_alt), ("sun_elevation", sun_elevation),
                              ("sun_azimuth", sun_azimuth)) if v is None]
    if missing:
        raise ValueError(f"nadir_products: pass {', '.join(missing)} (or a loaded dataset= to take them from)")
    return geo, roi, gt, water_mask, ignore_mask, min_alt, max_alt, sun_elevation, sun_azimuth


def _nadir_lattice(who, models, geo, grid, roi, min_alt, max_alt):
    """the lattice of a nadir map and its rays: -> (grid, its SnerfDsmGrid, rays (H W, 8), the GeoBounds of its scene x / y)"""
    from ...baseline.components import rays as R
    if grid is None:
        if roi is None:
            raise ValueError(f"{who}: pass grid= or roi= (the lattice to render)")
        grid = roi if isinstance(roi, D.DsmGrid) else D.roi_grid(roi)
    g = grid_struct(grid)
    dev = next(models["coarse"].parameters()).device
    rays, bounds = R.nadir_construct(g, geo, min_alt, max_alt, device=dev, want_bounds=True)
    return grid, g, rays, bounds


def _nadir_finish(grid, g, geo, rays, bounds, loc, n_classes, gt, water_mask, ignore_mask):
    """the products of a nadir walk that do not depend on the sun, from the frame's per-ray results `loc` (depth (n), albedo (3, n),
    beta (n)[, label (n) int64]): grid, dsm, albedo, beta, rays, planimetric_error, scene_bounds[, label][, mae]"""
    from ...baseline.components import rays as R
    h, w = g.out_h, g.out_w
    dev = rays.device
    cloud, _ = geo.cloud(rays, loc["depth"])
    east, north = (c.reshape(-1) for c in R.nadir_cell_centres(g, dev))
    off = torch.maximum((cloud[:, 0] - east).abs().max(), (cloud[:, 1] - north).abs().max())
    out = {"grid": window_grid(grid), "dsm": cloud[:, 2].to(torch.float32).reshape(h, w),
           "albedo": loc["albedo"].reshape(3, h, w), "beta": loc["beta"].reshape(h, w), "rays": rays,
           "planimetric_error": float(off), "scene_bounds": bounds}
    if n_classes:
        lab = loc["label"]
        out["label"] = torch.where((lab >= 0) & (lab < NO_LABEL), lab, torch.full_like(lab, NO_LABEL)).to(torch.uint8).reshape(h, w)
    if gt is not None:
        mae = D.compute_mae(out["dsm"], gt, water_mask=water_mask, ignore_mask=ignore_mask)
        out["mae"] = {"mean": mae["mean"], "median": mae["median"]}
    return out


def _nadir_walk(who, cfgs, renderer, models, suns, geo, grid, roi, min_alt, max_alt, t, render_options, sharded, gt, water_mask,
                ignore_mask, dataset):
    """The one walk behind nadir_products (its K = 1 case) and nadir_sun_sweep, whose docstrings state the arguments: the defaults
    and the lattice, ONE walk of util.relight_chunks over the rays under the K >= 1 `suns` ((elevation_deg, azimuth_deg) pairs; the
    first may hold None for what `dataset` supplies), the per-ray copies and the folds, the sharded gather and _nadir_finish.
    Returns _nadir_finish's products and "suns": the list, "rgb": (K, 3, H, W) f32, "sun": (K, H, W) f32."""
    from ... import ops, parallel
    from ...baseline.components import rays as R
    from . import vismaps
    from .util import relight_chunks, result_buffers, shard_options
    geo, roi, gt, water_mask, ignore_mask, min_alt, max_alt, el, az = _nadir_defaults(
        dataset, geo, roi, gt, water_mask, ignore_mask, min_alt, max_alt, suns[0][0], suns[0][1])
    suns = [(el, az)] + suns[1:]
    grid, g, rays, bounds = _nadir_lattice(who, models, geo, grid, roi, min_alt, max_alt)
    h, w = g.out_h, g.out_w
    n = _cells(g)
    K = len(suns)
    n_classes = models["coarse"].spec.n_classes
    dev = rays.device
    extras = R.nadir_extras(el, az, t, n, dev)

    lo, hi = parallel.frame_shard(n) if sharded else (0, n)
    m = hi - lo
    S = n_render_samples(cfgs.pipeline)
    keys = ("rgb", "depth") + (("semantic_label",) if n_classes else ()) + ("weights", "albedo", "sun", "beta")
    loc = {"depth": torch.empty(m, dtype=torch.float32, device=dev), "albedo": torch.empty((3, m), dtype=torch.float32, device=dev),
           "beta": torch.empty(m, dtype=torch.float32, device=dev)}
    if n_classes:
        loc["label"] = torch.empty(m, dtype=torch.int64, device=dev)
    rgb = torch.empty((K, m, 3), dtype=torch.float32, device=dev)
    sun = torch.empty((K, m), dtype=torch.float32, device=dev)
    if m:
        ops.release_workspaces()
        bufs = result_buffers(keys, min(cfgs.pipeline.render_chunk_size, m), S, n_classes, dev)
        stats = vismaps.new_stats(dev)
        for i, k, s, sl in relight_chunks(cfgs, renderer, models, rays[lo:hi], extras[lo:hi], suns, bufs,
                                          shard_options(render_options, lo, hi, n)):
            rgb[s, i:i + k].copy_(sl["rgb_coarse"])
            if s == 0:      # what no sun changes: taken from the base pass
                loc["depth"][i:i + k].copy_(sl["depth_coarse"])
                if n_classes:
                    loc["label"][i:i + k].copy_(sl["semantic_label_coarse"])
                vismaps.fold_chunk({"albedo_map": loc["albedo"], "sun_map": sun[0], "beta_map": loc["beta"]}, stats, i, m, k, S,
                                   weights=sl["weights_coarse"], albedo=sl["albedo_coarse"], sun=sl["sun_coarse"], beta=sl["beta_coarse"])
            else:
                vismaps.fold_chunk({"sun_map": sun[s]}, stats, i, m, k, S, weights=sl["weights_coarse"], sun=sl["sun_coarse"])
    if sharded:
        loc["albedo"] = loc["albedo"].t().contiguous()
        loc = {key: parallel.allgather_rows(v, n) for key, v in loc.items()}
        loc["albedo"] = loc["albedo"].t().contiguous()
        rgb = torch.stack([parallel.allgather_rows(rgb[s].contiguous(), n) for s in range(K)])
        sun = torch.stack([parallel.allgather_rows(sun[s].contiguous(), n) for s in range(K)])

    out = _nadir_finish(grid, g, geo, rays, bounds, loc, n_classes, gt, water_mask, ignore_mask)
    out["suns"] = suns
    out["rgb"] = rgb.permute(0, 2, 1).contiguous().reshape(K, 3, h, w)
    out["sun"] = sun.reshape(K, h, w)
    return out


@torch.no_grad()
def nadir_products(cfgs, renderer, models, geo=None, grid=None, roi=None, min_alt=None, max_alt=None, sun_elevation=None,
                   sun_azimuth=None, t=0, render_options={}, sharded=False, gt=None, water_mask=None, ignore_mask=None,
                   dataset=None, depth_mode="mean", normals=False):
    """The map of the lattice rendered from above: one vertical ray per cell (rays.nadir_construct between `max_alt` and
    `min_alt` metres, through `geo`, a GeoFrame), extras of the sun at (`sun_elevation`, `sun_azimuth`) degrees and the
    embedding index `t`.  The grid: `grid` (a DsmGrid, or a window of one from dsm.grid_struct), else the ROI grid of `roi`
    (a DsmGrid or the roi_txt meta), else a ValueError.  `dataset` (a loaded SatNeRFDataset) supplies what is not given: its
    geo, its "dsm" entry (roi, gt, masks), the min / max of its images' alt_min / alt_max, the sun of its first image.

    ONE walk of util.relight_chunks over the rays, under the one sun (`sharded`: over this rank's frame_shard of them, the
    results all-gathered as sharded_lean_inference does): the per-ray results are copied, albedo / sun / beta folded by
    vismaps.fold_chunk; no frame-sized per-sample tensor exists.  `render_options` as everywhere in evaluation ({"perturb": 0} for a repeatable map).
    `depth_mode="median"`: the surface ("dsm", hence "mae" and "planimetric_error") is that of the rays' median depths
    (SNERF_FLAG_DEPTH_MEDIAN); the colour, shadow and uncertainty maps do not read the depth and keep their bits.

    Returns {"grid": DsmGrid (of the window), "dsm": (H, W) f32 -- the altitude of geo.cloud(rays, depth), every cell filled --,
    "rgb": (3, H, W) f32, "albedo": (3, H, W) f32, "sun": (H, W) f32 (the shadow map), "beta": (H, W) f32[, "label": (H, W) u8
    (a model with classes; 255 for a label beyond 254)], "rays": the (H W, 8) nadir rays, "planimetric_error": the largest
    |east / north of the cloud - cell centre| in metres (the self-check of the ray construction), "scene_bounds": GeoBounds of
    the lattice's scene x / y (to_scene's stats)[, "mae": {"mean", "median"} of dsm.compute_mae(dsm, gt, water_mask,
    ignore_mask), with `gt` (H, W)]}.
    `normals=True` (single-device: a ValueError with `sharded`) adds the normals of the density field along the same rays, by a
    second walk (normals.ray_normals, on the stratified depths of `render_options`): "normal" (3, H, W) f32, east / north / up, NaN
    where the field has no gradient; "normal_angle" (H, W) f32, the angle in degrees to the raster normal of "dsm" itself
    (roofs.normals over the whole raster, radius 1); "normal_agreement": normals.normal_agreement's figures plus "bad", the NaN
    normals -- a consistency measure between the field and its own surface that needs no lidar.  False (default): nothing new runs
    and every product is what it was."""
    from .util import with_depth_mode
    if normals and sharded:
        raise ValueError("nadir_products: normals=True is a single-device walk; pass sharded=False")
    out = _nadir_walk("nadir_products", cfgs, renderer, models, [(sun_elevation, sun_azimuth)], geo, grid, roi, min_alt, max_alt, t,
                      with_depth_mode(render_options, depth_mode, "nadir_products"), sharded, gt, water_mask, ignore_mask, dataset)
    if normals:
        out.update(_nadir_normals(cfgs, renderer, models, out, geo if geo is not None else dataset.geo, t, render_options))
    del out["suns"]
    out["rgb"], out["sun"] = out["rgb"][0], out["sun"][0]
    return out


def _nadir_normals(cfgs, renderer, models, prod, geo, t, render_options):
    """the normals products of nadir_products from its walk's products `prod` (rays, dsm, grid, suns)"""
    from ...baseline.components import rays as R
    from . import normals as NM
    from . import roofs as RF
    from . import terrain as TR
    rays, dsm = prod["rays"], prod["dsm"]
    h, w = dsm.shape
    el, az = prod["suns"][0]
    opts = {k: v for k, v in (render_options or {}).items() if k != "depth_mode"}
    res = NM.ray_normals(cfgs, renderer, models, rays, R.nadir_extras(el, az, t, rays.shape[0], rays.device), opts)
    normal = NM.to_enu(geo, res["normal_n"]).t().contiguous().reshape(3, h, w)
    key, _, _ = TR.keys(dsm.contiguous())
    slope_e, slope_n, _, _, _ = RF.normals(key, torch.ones((h, w), dtype=torch.int32, device=dsm.device), 1, float(prod["grid"].resolution), radius=1)
    angle, stats = NM.normal_agreement(normal, slope_e, slope_n)
    return {"normal": normal, "normal_angle": torch.from_numpy(angle).to(torch.float32).to(dsm.device), "normal_agreement": dict(stats, bad=res["bad"])}


def sweep_suns(suns, dataset=None, who="nadir_sun_sweep"):
    """the suns of a sweep as a list of (elevation_deg, azimuth_deg) floats: `suns`, else those of the images of a loaded
    dataset's split, in split order; an empty list (or neither) is a ValueError"""
    if suns is None and dataset is not None:
        suns = [(m["sun_elevation"], m["sun_azimuth"]) for m in dataset.metas]
    suns = [(float(el), float(az)) for el, az in (suns or ())]
    if not suns:
        raise ValueError(f"{who}: no sun -- pass suns=[(elevation_deg, azimuth_deg), ...] (or a loaded dataset= to take its images' suns)")
    return suns


@torch.no_grad()
def nadir_sun_sweep(cfgs, renderer, models, suns=None, geo=None, grid=None, roi=None, min_alt=None, max_alt=None, t=0,
                    render_options={}, sharded=False, gt=None, water_mask=None, ignore_mask=None, dataset=None, depth_mode="mean"):
    """nadir_products under K suns in ONE walk over the lattice's rays (util.relight_chunks): per chunk a full pass under suns[0]
    and a relight per further sun, which re-runs only the sun-visibility branch, the sky colour and the composite on the chunk the
    workspace holds.  `suns`: (elevation_deg, azimuth_deg) pairs; None with a loaded `dataset`: the suns of
    the split's images in split order.  The lattice, `geo`, the altitudes, `t`, `sharded`, `gt` and the masks as for
    nadir_products, which `dataset` supplies likewise, and so `depth_mode` (the surface a shadow check casts from is then the median one).

    Returns the products of nadir_products that do not depend on the sun ("grid", "dsm", "albedo", "beta"[, "label"], "rays",
    "planimetric_error", "scene_bounds"[, "mae"]) and "suns": the list, "rgb": (K, 3, H, W) f32, "sun": (K, H, W) f32 (the
    shadow maps, folded by vismaps.fold_chunk), "lit_share": (H, W) f32 -- the mean of the K shadow maps, summed in fp64 in sun
    order and rounded once.  Map k has the bits of nadir_products under sun k, given the same depths ({"perturb": 0}): the jitter
    is drawn once per chunk and shared by the suns."""
    from .util import with_depth_mode
    out = _nadir_walk("nadir_sun_sweep", cfgs, renderer, models, sweep_suns(suns, dataset), geo, grid, roi, min_alt, max_alt, t,
                      with_depth_mode(render_options, depth_mode, "nadir_sun_sweep"), sharded, gt, water_mask, ignore_mask, dataset)
    total = torch.zeros_like(out["sun"][0], dtype=torch.float64)
    for plane in out["sun"]:      # in sun order, fp64; one rounding at the end
        total += plane.double()
    out["lit_share"] = (total / len(out["suns"])).to(torch.float32)
    return out
