"""Write the geo-referenced ortho products of a trained model (eval/utils/ortho.py ortho_products): the fused map of a split's
images as PNGs for the eye and GeoTIFFs for a GIS.  The reference has no counterpart.

Files under `output_dp`/ortho/{split}/:
    rgb.png, rgb.tif                     the true ortho-image: the colour of the highest point of every cell (empty cells black);
                                         uint8 by torchvision's save_image rule x * 255 + 0.5 (framework/visualize.py)
    label_top.png/.tif, label_vote.png/.tif   the class of the highest point / of the most votes (a semantic model only): the
                                         .tif holds the class ids (255 = no data), the .png the palette's colours, 255 as black
    top_alt.png/.tif, dsm.png/.tif       the top-surface altitude and the mean DSM: float32 in the .tif (NaN = no data), JET
                                         between the plane's own bounds in the .png (NaN as the colormap treats it: as 0)
    vote_share.png/.tif                  the winning class's share of a cell's votes: float32, BONE in the .png
  with robust=True (eval/utils/fuse.py) also:
    median_alt.png/.tif                  the lower median of the views' altitudes in a cell: float32, JET in the .png
    alt_spread.png/.tif                  the interquartile spread of those altitudes -- where the views agree: float32, BONE
    offers.png/.tif                      the points that offered themselves to a cell (as float32, the coverage's rule), BONE
    rgb_median.png/.tif, label_median.png/.tif   the colour and the class of the median point, written as rgb and label_top are
    fused_eval.json                      with gt=: {"mae": {"dsm", "top_alt", "median_alt"}}, each {"mean", "median"} in metres
GeoTIFFs carry ModelPixelScale, ModelTiepoint and, with the scene's zone, a GeoKeyDirectory (img_utils.save_geotiff).

export_nadir writes the map rendered from above (eval/utils/ortho.py nadir_products) by the same writers
and rules.  Files under `output_dp`/nadir/:
    rgb.png/.tif, albedo.png/.tif        the nadir ortho-image under the chosen sun and the albedo: uint8
    sun.png/.tif, beta.png/.tif          the shadow map and the uncertainty: float32 in the .tif, BONE in the .png
    dsm.png/.tif                         the rendered surface altitude, every cell filled: float32 in the .tif, JET in the .png
    label.png/.tif                       the class seen from above (a semantic model only): ids in the .tif, the palette in the .png

export_sun_sweep writes that map under a list of suns (eval/utils/ortho.py nadir_sun_sweep), again by the same
writers and rules.  Files under `output_dp`/nadir/sweep/:
    rgb_{k:03d}.png/.tif                 the nadir ortho-image under sun k: uint8
    sun_{k:03d}.png/.tif                 the shadow map under sun k: float32 in the .tif, BONE in the .png
    lit_share.png/.tif                   the mean of the shadow maps -- the share of the suns that light a cell: float32, BONE
    suns.json                            [{"index", "elevation_deg", "azimuth_deg"}], the suns in order

export_shadow_check runs the sweep and holds its learned shadow maps to the shadows its own DSM casts (eval/utils/shadow.py
shadow_check).  Files under `output_dp`/nadir/shadow/:
    cast_{k:03d}.png/.tif                the shadow the rendered DSM casts under sun k: 0 shadowed, 1 lit, 255 unknown in the .tif;
                                         black / white / grey in the .png
    disagree_{k:03d}.png                 where the thresholded learned shadow map and the cast mask differ: white; left-out cells grey
    shadow_check.json                    the suns, per sun the 8 raw words and the figures derived from them, bias and threshold

export_rectified takes the scene's OWN images and labels to the map (eval/utils/orthorect.py rectify) and, given a
model's map products on the same grid, scores them against the mosaic.  Files under `output_dp`/rectified/{split}/:
    {name}_rgb.png/.tif                  image {name} orthorectified on the DSM: uint8, cells it does not see black
    {name}_state.png/.tif                per cell 0 seen, 1 hole, 2 outside the image, 3 hidden by the DSM in the .tif; greys in the .png
    {name}_label.png/.tif                the image's labels on the map (a semantic scene only): ids in the .tif (255 = not seen)
    mosaic_rgb.png/.tif, coverage.png/.tif   the mean colour of the images that see a cell, and how many do (float32, BONE)
    mosaic_label.png/.tif, vote_share.png/.tif   the voted class and the winner's share of the votes (a semantic scene only)
    map_eval.json                        with model_products=: PSNR of its colour and, per label plane, the confusion matrix against
                                         the voted labels, accuracy, mIoU and the compared cells

export_objects labels the buildings of any of these maps and measures them (eval/utils/objects.py).  Files under
`output_dp`/objects/:
    objects.json                         per object: class, area, centroid, bbox, perimeter, altitudes, ground, height, volume
    objects_ids.png/.tif                 the object id of every cell (0 = none): float32 in the .tif, a colour per id in the .png
    objects_height.png/.tif              the height of the cell's object over the ground round it: float32 (NaN off objects), JET
    reference_objects.json, objects_eval.json   with reference=: the ground truth's objects, and detection precision / recall / F1,
                                         footprint IoU and the height error of the matched objects
    footprints.geojson                   with polygons=True: the objects' outlines as polygons in map coordinates, traced on the device
                                         (eval/utils/outline.py), the records of objects.json as properties

export_terrain puts a bare-earth terrain under any of these maps (eval/utils/terrain.py).  Files under
`output_dp`/terrain/:
    dtm.png/.tif, ndsm.png/.tif          the terrain and the height above it: float32 in the .tif (NaN = unreachable), JET in the .png
    ground.png, reach.png                the ground mask (white = ground) and the distance in cells to the ground a cell was filled from
    terrain.json                         the schedule, the counts and the parameters
    terrain_eval.json                    with reference=: DTM / nDSM errors and the ground masks' 2 x 2 table against its terrain

export_roofs fits roof planes to the buildings export_objects found (eval/utils/roofs.py).  Files under
`output_dp`/roofs/:
    pitch.png/.tif, residual.png/.tif    the slope of every building cell in degrees and its distance from its facet's plane in metres:
                                         float32 in the .tif (NaN off the roofs), JET in the .png
    aspect.png                           the orientation codes in a fixed palette (ASPECT_PALETTE)
    facets.tif                           the facet id of every cell (0 = none): int32
    roofs.json                           the facets and the per-building rows, the parameters and the counts
    roofs_eval.json                      with reference=: roof types, pitch and normals against the reference's roofs
    facets.geojson                       with polygons=True: the kept facets' outlines as polygons, the facet records as properties

export_solar measures the solar potential of any of these maps (eval/utils/solar.py).  Files under
`output_dp`/solar/:
    svf.png/.tif, sun_hours.png/.tif     the sky-view factor and the hours of direct sun per year: float32 in the .tif (NaN = a hole),
                                         BONE / JET in the .png
    insolation.png/.tif                  the global irradiation in kWh per m^2 of surface and year: float32 in the .tif, JET in the .png
    solar.json                           the parameters, the sun count and the per-facet and per-building tables

The other exports hand their keyword arguments to their products function, `depth_mode="median"` among them: the altitudes and everything
built on them are then those of the rays' median depths; at the default every file is what it was."""
import json
import os

import numpy as np
import torch
from PIL import Image

from ..framework.util import colormaps, img_utils
from ..framework.visualize import to_uint8_image
from ..parallel import world
from .utils import orthorect, vismaps
from .utils.dsm import roi_grid
from .utils.ortho import NO_LABEL, nadir_products, nadir_sun_sweep, ortho_products
from .utils.shadow import GT_HOLE_BELOW, METRICS, UNKNOWN, shadow_check


def _png(fp, chw_u8):
    Image.fromarray(chw_u8.permute(1, 2, 0).contiguous().cpu().numpy()).save(fp)


def label_colors(label, palette):
    """(H, W) uint8 labels -> (3, H, W) uint8 through `palette` ((K, 3) uint8); 255 and any label beyond the palette are black"""
    pal = torch.as_tensor(np.asarray(palette, np.uint8))
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    lut[:min(len(pal), NO_LABEL)] = pal[:NO_LABEL]
    return lut.to(label.device)[label.long()].permute(2, 0, 1).contiguous()


def _scalar_plane(fp, name, plane, cmap, grid, zone_string):
    """a float32 plane as `name`.png (`cmap` between the plane's own bounds) and `name`.tif"""
    stats = vismaps.plane_minmax(plane, vismaps.new_stats(plane.device), "user")
    _png(fp(name + ".png"), vismaps.colormap(plane, colormaps.table(cmap, plane.device), stats, "user"))
    img_utils.save_geotiff(fp(name + ".tif"), plane, grid, zone_string)


def _color_plane(fp, name, chw, grid, zone_string):
    """a float32 colour plane (3, H, W) as uint8 `name`.png and `name`.tif"""
    u8 = to_uint8_image(chw)
    _png(fp(name + ".png"), u8)
    img_utils.save_geotiff(fp(name + ".tif"), u8.permute(1, 2, 0).contiguous(), grid, zone_string)


def _label_plane(fp, name, label, palette, grid, zone_string):
    """a uint8 class plane as `name`.png (the colours of `palette`, default colormaps.DEFAULT_PALETTE) and `name`.tif (the ids)"""
    _png(fp(name + ".png"), label_colors(label, colormaps.DEFAULT_PALETTE if palette is None else palette))
    img_utils.save_geotiff(fp(name + ".tif"), label, grid, zone_string)


def _zone(zone_string, kwargs, geo=None):
    """the GeoTIFFs' UTM zone: `zone_string`, else the zone of the GeoFrame in use -- the products' geo=, their dataset's, or `geo`"""
    if zone_string is None:
        zone_string = getattr(kwargs.get("geo") or getattr(kwargs.get("dataset"), "geo", None) or geo, "zone_string", None)
    return zone_string


def _writer(*dirs):
    """-> (files, fp): on rank 0 the directory os.path.join(*dirs) exists and fp(name) is the path of `name` in it, entered into
    `files`; on every other rank fp is None -- only rank 0 writes"""
    out_dp = os.path.join(*dirs)
    files = {}
    if world()[0] != 0:
        return files, None
    os.makedirs(out_dp, exist_ok=True)
    return files, lambda name: files.setdefault(name, os.path.join(out_dp, name))


def _sun_rows(suns):
    return [{"index": k, "elevation_deg": el, "azimuth_deg": az} for k, (el, az) in enumerate(suns)]


@torch.no_grad()
def export_ortho(cfgs, renderer, models, images, output_dp, split="test", palette=None, zone_string=None, **kwargs):
    """ortho_products(cfgs, renderer, models, images, **kwargs) of the split's images, written to `output_dp`/ortho/{split}/.
    On the test split item 0 is skipped, as the evaluators do (it is also a training view).  `palette`: (K, 3) uint8, default
    colormaps.DEFAULT_PALETTE.  `zone_string`: the GeoTIFFs' UTM zone, default the zone of the GeoFrame in use.  Every rank
    computes the products (with sharded=True each renders its share of a frame); only rank 0 writes.  Returns the products
    plus "files": {name: path}."""
    todo = list(images)[1 if split == "test" else 0:]
    if not todo:
        raise ValueError(f"no {split} image to export")
    prod = ortho_products(cfgs, renderer, models, todo, **kwargs)
    zone_string = _zone(zone_string, kwargs, (todo[0].get("dsm") or {}).get("geo"))
    grid = prod["grid"]
    files, fp = _writer(output_dp, "ortho", split)
    if fp:
        _color_plane(fp, "rgb", torch.nan_to_num(prod["rgb"], nan=0.0), grid, zone_string)
        for key in ("label_top", "label_vote"):
            if key in prod:
                _label_plane(fp, key, prod[key], palette, grid, zone_string)
        planes = [("top_alt", colormaps.COLORMAP_JET), ("dsm", colormaps.COLORMAP_JET)]
        if "vote_share" in prod:
            planes.append(("vote_share", colormaps.COLORMAP_BONE))
        if "median_alt" in prod:                             # robust=True: the fused quantiles
            planes += [("median_alt", colormaps.COLORMAP_JET), ("alt_spread", colormaps.COLORMAP_BONE)]
            _color_plane(fp, "rgb_median", torch.nan_to_num(prod["rgb_median"], nan=0.0), grid, zone_string)
            if "label_median" in prod:
                _label_plane(fp, "label_median", prod["label_median"], palette, grid, zone_string)
        for key, cmap in planes:
            _scalar_plane(fp, key, prod[key], cmap, grid, zone_string)
        if "offers" in prod:
            _scalar_plane(fp, "offers", prod["offers"].to(torch.float32), colormaps.COLORMAP_BONE, grid, zone_string)
        if "mae" in prod:
            with open(fp("fused_eval.json"), "w") as f:
                json.dump({"mae": prod["mae"]}, f, indent=1)
    return dict(prod, files=files)


@torch.no_grad()
def export_nadir(cfgs, renderer, models, output_dp, palette=None, zone_string=None, **kwargs):
    """nadir_products(cfgs, renderer, models, **kwargs), written to `output_dp`/nadir/.  `palette`: (K, 3) uint8, default
    colormaps.DEFAULT_PALETTE.  `zone_string`: the GeoTIFFs' UTM zone, default the zone of the GeoFrame in use.  Every rank
    computes the products (with sharded=True each renders its share of the lattice); only rank 0 writes.  Returns the products
    plus "files": {name: path}.  With normals=True (nadir_products) also normal.png -- RGB = 0.5 + 0.5 (east, north, up), a cell
    without a normal black --, normal_up.tif (the up component) and normals.json (the agreement with the DSM's own raster normals)."""
    prod = nadir_products(cfgs, renderer, models, **kwargs)
    zone_string = _zone(zone_string, kwargs)
    grid = prod["grid"]
    files, fp = _writer(output_dp, "nadir")
    if fp:
        for key in ("rgb", "albedo"):
            _color_plane(fp, key, prod[key], grid, zone_string)
        if "label" in prod:
            _label_plane(fp, "label", prod["label"], palette, grid, zone_string)
        for key, cmap in (("dsm", colormaps.COLORMAP_JET), ("sun", colormaps.COLORMAP_BONE), ("beta", colormaps.COLORMAP_BONE)):
            _scalar_plane(fp, key, prod[key], cmap, grid, zone_string)
        if "normal" in prod:
            _png(fp("normal.png"), to_uint8_image(torch.nan_to_num(0.5 + 0.5 * prod["normal"], nan=0.0).clamp(0.0, 1.0)))
            img_utils.save_geotiff(fp("normal_up.tif"), prod["normal"][2].contiguous(), grid, zone_string)
            with open(fp("normals.json"), "w") as f:
                json.dump({"agreement_with_dsm_normals": prod["normal_agreement"], "frame": "east / north / up at the scene centre",
                           "encoding": "normal.png: RGB = 0.5 + 0.5 n; normal_up.tif: the up component"}, f, indent=1)
    return dict(prod, files=files)


@torch.no_grad()
def export_sun_sweep(cfgs, renderer, models, output_dp, zone_string=None, **kwargs):
    """nadir_sun_sweep(cfgs, renderer, models, **kwargs), written to `output_dp`/nadir/sweep/ by export_nadir's writers and rules:
    per sun k rgb_{k:03d} and sun_{k:03d} -- the files export_nadir writes as rgb and sun under that sun --, lit_share, and
    suns.json.  `zone_string`: the GeoTIFFs' UTM zone, default the zone of the GeoFrame in use.  Every rank computes the products
    (with sharded=True each renders its share of the lattice); only rank 0 writes.  Returns the products plus "files"."""
    prod = nadir_sun_sweep(cfgs, renderer, models, **kwargs)
    zone_string = _zone(zone_string, kwargs)
    grid = prod["grid"]
    files, fp = _writer(output_dp, "nadir", "sweep")
    if fp:
        for k in range(len(prod["suns"])):
            _color_plane(fp, f"rgb_{k:03d}", prod["rgb"][k], grid, zone_string)
            _scalar_plane(fp, f"sun_{k:03d}", prod["sun"][k], colormaps.COLORMAP_BONE, grid, zone_string)
        _scalar_plane(fp, "lit_share", prod["lit_share"], colormaps.COLORMAP_BONE, grid, zone_string)
        with open(fp("suns.json"), "w") as f:
            json.dump(_sun_rows(prod["suns"]), f, indent=1)
    return dict(prod, files=files)


def _state_png(fp, state):
    """a rectified image's state plane as a grey PNG: seen white, hidden mid-grey, outside dark grey, hole black"""
    lut = torch.zeros(256, dtype=torch.uint8)
    lut[orthorect.SEEN], lut[orthorect.HIDDEN], lut[orthorect.OUTSIDE] = 255, 128, 64
    _png(fp, lut.to(state.device)[state.long()].unsqueeze(0).expand(3, -1, -1))


@torch.no_grad()
def export_rectified(cfgs, dataset, output_dp, dsm=None, split="train", model_products=None, grid=None, palette=None,
                     zone_string=None, occlusion=True, bias=0.0):
    """The images of a loaded `dataset` (the `split` split of a scene: baseline/dataset/satnerf_dataset.py) orthorectified on a DSM
    (eval/utils/orthorect.py rectify), written to `output_dp`/rectified/{split}/.  `dsm` ((H, W) f32 on the
    GPU) with its `grid` (a DsmGrid or a window of one): None takes `model_products`' "dsm" and "grid" when given, else the
    scene's lidar ground truth on its ROI (altitudes below -500 m are holes).  A semantic dataset's labels are voted per cell.
    `model_products`: an ortho_products or nadir_products result ON THE SAME GRID (anything else is a ValueError); with it
    map_eval.json holds orthorect.map_agreement of its "rgb" and of each of its label planes against the mosaic.
    Files: per image {name}_rgb, {name}_state[, {name}_label], and for the split mosaic_rgb, coverage (how many images see a cell),
    [mosaic_label, vote_share], each as .png and .tif by the writers and rules of export_ortho; the state .tif holds 0 seen,
    1 hole, 2 outside, 3 hidden.  Only rank 0 writes.  Returns rectify's result plus "files"[, "map_eval"]."""
    if dataset.geo is None:
        raise ValueError("export_rectified: the dataset carries no GeoFrame (load the scene through load_scene_banks)")
    if dsm is None and model_products is not None:
        dsm, grid = model_products["dsm"], model_products["grid"]
    elif dsm is None:
        entry = dataset.dsm
        if not entry or "gt" not in entry:
            raise ValueError("export_rectified: no dsm= given and the scene has no ground-truth DSM on disk")
        gt = entry["gt"].float()
        dsm, grid = torch.where(gt < GT_HOLE_BELOW, torch.full_like(gt, float("nan")), gt), roi_grid(entry["roi"])
    elif grid is None:
        if model_products is None:
            raise ValueError("export_rectified: pass grid=, the lattice of dsm=")
        grid = model_products["grid"]
    n_classes = getattr(dataset, "semantic_n_classes", None) if "semantic" in dataset.t else None
    res = orthorect.rectify(dsm, grid, dataset.geo, orthorect.dataset_images(dataset), n_classes=n_classes, occlusion=occlusion,
                            keep_images=True, bias=bias)
    out_grid = res["grid"]
    if model_products is not None and orthorect.window_grid(model_products["grid"]) != out_grid:
        raise ValueError(f"export_rectified: the model's products lie on {orthorect.window_grid(model_products['grid'])}, the DSM on {out_grid}")
    zone_string = zone_string or dataset.geo.zone_string
    files, fp = _writer(output_dp, "rectified", split)
    if model_products is not None:
        doc = {"rgb": orthorect.map_agreement(model_products["rgb"], None, res, n_classes)} if "rgb" in model_products else {}
        if n_classes:
            for key in ("label", "label_top", "label_vote"):
                if key in model_products:
                    doc[key] = orthorect.map_agreement(None, model_products[key], res, n_classes)
        res["map_eval"] = doc
    if fp:
        kept = res["images"]
        for k, it in enumerate(dataset.items):
            _color_plane(fp, f"{it['name']}_rgb", torch.nan_to_num(kept["rgb"][k], nan=0.0), out_grid, zone_string)
            _state_png(fp(f"{it['name']}_state.png"), kept["state"][k])
            img_utils.save_geotiff(fp(f"{it['name']}_state.tif"), kept["state"][k], out_grid, zone_string)
            if "label" in kept:
                _label_plane(fp, f"{it['name']}_label", kept["label"][k], palette, out_grid, zone_string)
        _color_plane(fp, "mosaic_rgb", torch.nan_to_num(res["rgb"], nan=0.0), out_grid, zone_string)
        _scalar_plane(fp, "coverage", res["count"].to(torch.float32), colormaps.COLORMAP_BONE, out_grid, zone_string)
        if "label_vote" in res:
            _label_plane(fp, "mosaic_label", res["label_vote"], palette, out_grid, zone_string)
            _scalar_plane(fp, "vote_share", res["vote_share"], colormaps.COLORMAP_BONE, out_grid, zone_string)
        if "map_eval" in res:
            with open(fp("map_eval.json"), "w") as f:
                json.dump(res["map_eval"], f, indent=1)
    return dict(res, files=files)


def _mask_png(fp, mask):
    """a 0 / 1 / 255 mask as a grey PNG: 0 black, 1 white, 255 (unknown / left out) mid-grey"""
    lut = torch.zeros(256, dtype=torch.uint8)
    lut[1], lut[UNKNOWN] = 255, 128
    _png(fp, lut.to(mask.device)[mask.long()].unsqueeze(0).expand(3, -1, -1))


@torch.no_grad()
def export_shadow_check(cfgs, renderer, models, output_dp, zone_string=None, bias=0.0, threshold=0.5, **kwargs):
    """nadir_sun_sweep(cfgs, renderer, models, **kwargs) and shadow_check on its products (with the sweep's gt / masks when it was
    given them), written to `output_dp`/nadir/shadow/: per sun k cast_{k:03d}.png/.tif and disagree_{k:03d}.png, and
    shadow_check.json.  `zone_string`: the GeoTIFFs' UTM zone, default the zone of the GeoFrame in use.  Every rank computes the
    products; only rank 0 writes.  Returns the sweep's products, "shadow_check": the check's result, and "files"."""
    prod = nadir_sun_sweep(cfgs, renderer, models, **kwargs)
    ds = kwargs.get("dataset")
    entry = (getattr(ds, "dsm", None) or {}) if kwargs.get("gt") is None and kwargs.get("roi") is None else {}
    masks = {k: kwargs.get(k) if kwargs.get(k) is not None else entry.get(k) for k in ("gt", "water_mask", "ignore_mask")}
    chk = shadow_check(prod, bias=bias, threshold=threshold, **masks)
    zone_string = _zone(zone_string, kwargs)
    grid = prod["grid"]
    files, fp = _writer(output_dp, "nadir", "shadow")
    if fp:
        for k in range(len(chk["suns"])):
            _mask_png(fp(f"cast_{k:03d}.png"), chk["cast_model"][k])
            img_utils.save_geotiff(fp(f"cast_{k:03d}.tif"), chk["cast_model"][k], grid, zone_string)
            _mask_png(fp(f"disagree_{k:03d}.png"), chk["disagree"][k])
        doc = {"bias": bias, "threshold": threshold, "suns": _sun_rows(chk["suns"])}
        for key in ("agreement_model", "agreement_gt"):
            if key in chk:
                doc[key] = [dict({m: a[m] for m in METRICS}, words=a["words"]) for a in chk[key]]
        with open(fp("shadow_check.json"), "w") as f:
            json.dump(doc, f, indent=1)
    return dict(prod, shadow_check=chk, files=files)


def id_colors(ids):
    """(H, W) int32 object ids -> (3, H, W) uint8: every object in a colour taken from its id (three multiplicative hashes, kept
    off the dark end), the background black"""
    n = ids.long()
    rgb = torch.stack([(n * m + a) % 192 + 64 for m, a in ((97, 53), (57, 131), (151, 17))]).to(torch.uint8)
    return torch.where((n > 0).unsqueeze(0), rgb, torch.zeros_like(rgb)).contiguous()


def _reference_on(grid, reference, reference_grid, resample):
    """`reference` ({"alt"[, "label"]}) as the exports compare it: itself without `reference_grid`; with one, its planes warped from
    that lattice onto `grid` -- "alt" by `resample` (None: the default by the steps), "label" by the label default"""
    if reference is None or reference_grid is None:
        return reference
    from .utils import warp as W
    out = dict(reference)
    src = W.lattice_of(reference_grid, reference["alt"].shape)
    out["alt"] = W.warp(reference["alt"], src, grid, resample)
    if reference.get("label") is not None:
        out["label"] = W.warp(reference["label"], src, grid)
    return out


@torch.no_grad()
def export_objects(products, output_dp, classes=(3,), ground=(0,), label_key=None, alt_key=None, reference=None, zone_string=None,
                   palette=None, dtm=None, reference_grid=None, reference_resample=None, polygons=False, simplify_m=0.0, **kwargs):
    """The objects of a map (eval/utils/objects.py objects), written to `output_dp`/objects/.  `products`: what
    nadir_products, ortho_products or orthorect.rectify return ("grid" and a label and an altitude plane).  `label_key`: default the
    first of "label", "label_vote", "label_median", "label_top" present; `alt_key`: the first of "dsm", "median_alt", "top_alt".
    `classes`: the classes whose components are objects, `ground`: the classes that count as ground round an object -- the defaults
    (3,) and (0,) are the building and the ground entry of colormaps.DEFAULT_PALETTE's list; a scene with other class ids passes its
    own.  **kwargs (connectivity, ring, min_area_m2) go to objects().  `reference`: {"label", "alt"} on the same lattice -- for
    example rectify(lidar_dsm, ...)["label_vote"] with the lidar DSM -- whose objects the map's are scored against (match_objects,
    object_scores); a lattice mismatch is a ValueError that names both shapes.  `palette` is taken as the other exports take it; no
    file of this export shows class colours (an object's colour comes from its id), so it is not read.  `dtm`: a terrain plane on
    the products' lattice (export_terrain's "dtm"): the map's table gains terrain_alt, height_over_terrain, volume_over_terrain_m3.
    `reference_grid`: the lattice of `reference` (a DsmGrid or a geotransform) when it is not the products' -- its planes are first
    warped onto the products' lattice (eval/utils/warp.py), "alt" by `reference_resample` (a method name;
    default bilinear / average by the steps), "label" by the label default; without it the shapes must agree, as before.
    `polygons`: also trace the objects' outlines on the device (eval/utils/outline.py) and write
    footprints.geojson -- one Polygon per object in map coordinates, its properties the object's record of objects.json; `simplify_m`:
    the Douglas-Peucker tolerance in metres (0 = every corner of the raster outline).  Without `polygons` nothing more is launched or
    written.
    Files: objects.json ({"objects": the table as records, "stats", "parameters"}), objects_ids.tif (float32: ids are exact below
    2^24, a ValueError beyond) and objects_ids.png (each object in a colour taken from its id), objects_height.tif / .png (the height
    of the cell's object, NaN off objects; JET); with `reference` also reference_objects.json and objects_eval.json.  Only rank 0
    writes.  Returns objects()'s result plus "files"[, "reference", "eval"]."""
    from .utils import objects as OB
    from .utils.ortho import window_grid
    label_key = label_key or next((k for k in ("label", "label_vote", "label_median", "label_top") if k in products), None)
    alt_key = alt_key or next((k for k in ("dsm", "median_alt", "top_alt") if k in products), None)
    if label_key not in products or alt_key not in products:
        raise ValueError(f"export_objects: the products hold no label plane ({label_key!r}) or no altitude plane ({alt_key!r})")
    label, alt, grid = products[label_key], products[alt_key], window_grid(products["grid"])
    shape = tuple(label.shape)
    reference = _reference_on(grid, reference, reference_grid, reference_resample)
    if reference is not None and (tuple(reference["label"].shape) != shape or tuple(reference["alt"].shape) != shape):
        raise ValueError(f"export_objects: the products lie on a lattice of {tuple(label.shape)} cells, the reference on "
                         f"{tuple(reference['label'].shape)} (label) / {tuple(reference['alt'].shape)} (alt)")
    if dtm is not None and tuple(dtm.shape) != shape:
        raise ValueError(f"export_objects: the products lie on a lattice of {shape} cells, the dtm on {tuple(dtm.shape)}")
    res = OB.objects(label, alt.float(), grid, classes, ground, dtm=None if dtm is None else dtm.float(), **kwargs)
    if res["n"] >= 2 ** 24:
        raise ValueError(f"export_objects: {res['n']} objects: a float32 GeoTIFF holds ids exactly below 2^24 only")
    params = dict({"classes": [int(c) for c in classes], "ground": [int(c) for c in ground], "label_key": label_key, "alt_key": alt_key},
                  **kwargs)
    if reference is not None:
        ref = OB.objects(reference["label"], reference["alt"].float(), grid, classes, ground, **kwargs)
        pairs, inter, union = OB.match_objects(res["ids"], res["n"], ref["ids"], ref["n"])
        res = dict(res, reference=ref, eval=OB.object_scores(res["table"], ref["table"], pairs, inter, union))
    zone_string = _zone(zone_string, kwargs)
    if polygons:
        import inspect
        from .utils import outline as OL
        # the connectivity the ids were labelled with: the caller's, else the default of objects() itself
        connectivity = kwargs.get("connectivity", inspect.signature(OB.objects).parameters["connectivity"].default)
        doc, outline = OL.footprints(res["ids"], res["n"], grid, connectivity, simplify_m, zone_string, OB.table_records(res["table"]))
        res = dict(res, footprints=doc, outline_stats=outline["stats"])
    files, fp = _writer(output_dp, "objects")
    if fp:
        if polygons:
            with open(fp("footprints.geojson"), "w") as f:
                json.dump(res["footprints"], f)
        with open(fp("objects.json"), "w") as f:
            json.dump({"objects": OB.table_records(res["table"]), "stats": res["stats"], "parameters": params}, f, indent=1)
        _png(fp("objects_ids.png"), id_colors(res["ids"]))
        img_utils.save_geotiff(fp("objects_ids.tif"), res["ids"].to(torch.float32), grid, zone_string)
        _scalar_plane(fp, "objects_height", res["object_height"], colormaps.COLORMAP_JET, grid, zone_string)
        if reference is not None:
            with open(fp("reference_objects.json"), "w") as f:
                json.dump({"objects": OB.table_records(res["reference"]["table"]), "stats": res["reference"]["stats"],
                           "parameters": params}, f, indent=1)
            with open(fp("objects_eval.json"), "w") as f:
                json.dump(res["eval"], f, indent=1)
    return dict(res, files=files)


@torch.no_grad()
def export_terrain(products, output_dp, alt_key=None, label_key=None, blocked=(3,), reference=None, zone_string=None, reference_grid=None,
                   reference_resample=None, **kwargs):
    """The bare-earth terrain under a map (eval/utils/terrain.py terrain), written to `output_dp`/terrain/.
    `products`: what nadir_products, ortho_products or orthorect.rectify return ("grid" and an altitude plane).  `alt_key`: default the
    first of "dsm", "median_alt", "top_alt" present; `label_key`: default the first of "label", "label_vote", "label_median",
    "label_top" present -- with a label plane the classes `blocked` can never be ground (the default (3,) is the building entry of
    colormaps.DEFAULT_PALETTE's list; a scene with other class ids passes its own); without one nothing is blocked.  **kwargs
    (max_window_m, slope, dh0, dh_max) go to terrain's schedule.  `reference`: {"alt"[, "label"]} on the same lattice -- the lidar DSM,
    say, with the rectified ground-truth labels -- whose terrain the map's is held to (terrain_agreement); a lattice mismatch is a
    ValueError that names both shapes.  `reference_grid`, `reference_resample`: as export_objects takes them -- a reference on a
    lattice of its own is first warped onto the products'.
    Files: dtm.tif / .png and ndsm.tif / .png (JET), ground.png (white = ground), reach.png (BONE), terrain.json ({"schedule", "stats",
    "parameters"}); with `reference` also terrain_eval.json.  Only rank 0 writes.  Returns terrain()'s result plus "files"[,
    "reference", "eval"]."""
    from .utils import terrain as TR
    from .utils.ortho import window_grid
    alt_key = alt_key or next((k for k in ("dsm", "median_alt", "top_alt") if k in products), None)
    label_key = label_key or next((k for k in ("label", "label_vote", "label_median", "label_top") if k in products), None)
    if alt_key not in products or (label_key is not None and label_key not in products):
        raise ValueError(f"export_terrain: the products hold no altitude plane ({alt_key!r}) or no label plane ({label_key!r})")
    alt, grid = products[alt_key], window_grid(products["grid"])
    label = products[label_key] if label_key is not None else None
    shape = tuple(alt.shape)
    reference = _reference_on(grid, reference, reference_grid, reference_resample)
    if reference is not None:
        ref_label = reference.get("label")
        if tuple(reference["alt"].shape) != shape or (ref_label is not None and tuple(ref_label.shape) != shape):
            raise ValueError(f"export_terrain: the products lie on a lattice of {shape} cells, the reference on "
                             f"{tuple(reference['alt'].shape)} (alt)" + ("" if ref_label is None else f" / {tuple(ref_label.shape)} (label)"))
    used = tuple(blocked) if label is not None else ()
    res = TR.terrain(alt.float(), grid, label, used, **kwargs)
    params = dict({"alt_key": alt_key, "label_key": label_key, "blocked": [int(c) for c in used]}, **kwargs)
    if reference is not None:
        ref = TR.terrain(reference["alt"].float(), grid, ref_label, tuple(blocked) if ref_label is not None else (), **kwargs)
        res = dict(res, reference=ref, eval=TR.terrain_agreement(res, ref))
    zone_string = _zone(zone_string, kwargs)
    files, fp = _writer(output_dp, "terrain")
    if fp:
        _scalar_plane(fp, "dtm", res["dtm"], colormaps.COLORMAP_JET, grid, zone_string)
        _scalar_plane(fp, "ndsm", res["ndsm"], colormaps.COLORMAP_JET, grid, zone_string)
        _mask_png(fp("ground.png"), res["ground"].to(torch.uint8))
        stats = vismaps.plane_minmax(res["reach"].to(torch.float32), vismaps.new_stats(alt.device), "user")
        _png(fp("reach.png"), vismaps.colormap(res["reach"].to(torch.float32), colormaps.table(colormaps.COLORMAP_BONE, alt.device), stats,
                                                "user"))
        with open(fp("terrain.json"), "w") as f:
            json.dump({"schedule": res["schedule"], "stats": res["stats"], "parameters": params}, f, indent=1)
        if reference is not None:
            with open(fp("terrain_eval.json"), "w") as f:
                json.dump(res["eval"], f, indent=1)
    return dict(res, files=files)


# aspect.png: code -> colour.  0 flat grey; 1..8 the downslope octants N, NE, E, SE, S, SW, W, NW round the colour wheel; 9 steep white;
# 253 (hole) and 254 (degenerate) dark red; everything else (255: not an object cell) black
ASPECT_PALETTE = {0: (128, 128, 128), 1: (255, 0, 0), 2: (255, 160, 0), 3: (255, 255, 0), 4: (0, 255, 0), 5: (0, 255, 255), 6: (0, 128, 255),
                  7: (0, 0, 255), 8: (255, 0, 255), 9: (255, 255, 255), 253: (96, 0, 0), 254: (96, 0, 0)}


def aspect_colors(code):
    """(H, W) uint8 orientation codes -> (3, H, W) uint8 through ASPECT_PALETTE"""
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    for c, rgb in ASPECT_PALETTE.items():
        lut[c] = torch.tensor(rgb, dtype=torch.uint8)
    return lut.to(code.device)[code.long()].permute(2, 0, 1).contiguous()


def _roof_arcs(res, alt, ids, grid, zone_string, roofs_kwargs, want_lines, want_polygons, simplify_m, grow_m, step_m, level_deg):
    """what export_roofs adds for `lines` and for `polygons` with `shared`: the grown facet raster, its arcs, the roof lines and the
    polygons with shared borders -> the keys to merge into roofs()'s result"""
    from fractions import Fraction
    from .utils import arcs as AR
    from .utils import outline as OL
    from .utils import roofs as RF
    from .utils import terrain as TR
    from .utils.ortho import Q, Z0
    z0, q = roofs_kwargs.get("z0", Z0), roofs_kwargs.get("q", Q)
    key, _, _ = TR.keys(alt, z0=z0, q=q)
    grown, grown_cells, rounds = RF.grow(res["facet_ids"], ids, key, res["facets"], grow_m=grow_m, q=q)
    arcs = AR.arcs(grown, res["n_facets"], res["parameters"]["connectivity"], key=key)
    out = {"facet_ids_grown": grown, "grown_cells": grown_cells, "grow_rounds": rounds, "arc_stats": arcs["stats"]}
    cells = Fraction(simplify_m) / Fraction(float(grid.resolution))
    if want_lines:
        records = RF.lines(arcs, res["facets"], grid, step_m=step_m, level_deg=level_deg, simplify_cells=cells, z0=z0, q=q)
        doc = {"type": "FeatureCollection",
               "features": [{"type": "Feature", "id": k + 1, "properties": {name: v for name, v in rec.items() if name != "coordinates"},
                             "geometry": {"type": "LineString", "coordinates": rec["coordinates"]}} for k, rec in enumerate(records)]}
        if zone_string is not None:
            doc["crs"] = {"type": "name", "properties": {"name": f"urn:ogc:def:crs:EPSG::{img_utils.utm_epsg(zone_string)}"}}
        K = len(res["buildings"]["facets"])
        counts = {kind: sum(1 for rec in records if rec["kind"] == kind) for kind in RF.LINE_KINDS}
        summary = {"buildings": RF.table_records(RF.line_table(records, K)), "counts": counts, "rounds": rounds,
                   "grown_cells": [int(v) for v in grown_cells], "arcs": arcs["stats"],
                   "parameters": {"grow_m": grow_m, "step_m": step_m, "level_deg": level_deg, "simplify_m": float(simplify_m)}}
        out.update(lines=records, lines_geojson=doc, lines_summary=summary)
    if want_polygons:
        polys = OL.simplify_shared(arcs, cells)
        out.update(footprints=OL.geojson(polys, grid, zone_string, RF.table_records(res["facets"])), outline_stats=arcs["rings"]["stats"])
    return out


@torch.no_grad()
def export_roofs(products, objects_result, output_dp, alt_key=None, reference=None, zone_string=None, **kwargs):
    """The roofs of a map's buildings (eval/utils/roofs.py roofs), written to `output_dp`/roofs/.  `products`: what
    nadir_products, ortho_products or orthorect.rectify return ("grid" and an altitude plane); `objects_result`: what objects() or
    export_objects returned for them ("ids", "n", "table").  `alt_key`: default the first of "dsm", "median_alt", "top_alt" present.
    **kwargs (radius, flat_deg, wall_deg, aspect0_deg, connectivity, min_facet_m2) go to roofs().  `reference`: {"alt", "objects"} on
    the same lattice -- the lidar DSM, say, and the objects() of the rectified ground-truth labels -- whose roofs the map's are held
    to over the buildings match_objects pairs (roof_agreement); a lattice mismatch is a ValueError that names both shapes.
    Two keywords are taken out of **kwargs before roofs() sees them (the named parameters are pinned by tests/test_roofs_cpu.py):
    `polygons` (default False) and `simplify_m` (default 0.0), as export_objects takes them -- facets.geojson holds one Polygon per
    kept facet, its properties the facet's record of roofs.json; the facets are simplified one by one, so neighbours may part by up
    to the tolerance.  Without `polygons` nothing more is launched or written.
    Five more are taken out the same way: `lines` (default False), `shared` (default False), `grow_m` (0.25), `step_m` (1.0) and
    `level_deg` (5.0).  With `lines` the kept facets are grown over the dropped cells of their buildings (roofs.grow), the arcs of the
    grown raster are traced (eval/utils/arcs.py) and classified (roofs.lines): lines.geojson holds one 3-D
    LineString per roof line with its record as properties, lines.json {"buildings": roofs.line_table, "parameters", "counts",
    "rounds", "grown_cells", "arcs"}, facets_grown.tif the grown ids.  With `polygons` and `shared`, facets.geojson comes from
    outline.simplify_shared on the grown raster: neighbouring facets share their borders.  Without them nothing more is launched or
    written.
    Files: pitch.tif / .png and residual.tif / .png (JET), aspect.png (ASPECT_PALETTE), facets.tif (int32), roofs.json ({"facets",
    "buildings", "stats", "parameters"}); with `reference` also roofs_eval.json.  Only rank 0 writes.  Returns roofs()'s result plus
    "files"[, "reference", "pairs", "eval"]."""
    from .utils import objects as OB
    from .utils import roofs as RF
    from .utils.ortho import window_grid
    polygons, simplify_m = bool(kwargs.pop("polygons", False)), kwargs.pop("simplify_m", 0.0)
    lines, shared = bool(kwargs.pop("lines", False)), bool(kwargs.pop("shared", False))
    grow_m, step_m, level_deg = kwargs.pop("grow_m", 0.25), kwargs.pop("step_m", 1.0), kwargs.pop("level_deg", 5.0)
    alt_key = alt_key or next((k for k in ("dsm", "median_alt", "top_alt") if k in products), None)
    if alt_key not in products:
        raise ValueError(f"export_roofs: the products hold no altitude plane ({alt_key!r})")
    alt, grid = products[alt_key], window_grid(products["grid"])
    shape = tuple(alt.shape)
    if tuple(objects_result["ids"].shape) != shape:
        raise ValueError(f"export_roofs: the products lie on a lattice of {shape} cells, the objects on {tuple(objects_result['ids'].shape)}")
    if reference is not None and (tuple(reference["alt"].shape) != shape or tuple(reference["objects"]["ids"].shape) != shape):
        raise ValueError(f"export_roofs: the products lie on a lattice of {shape} cells, the reference on "
                         f"{tuple(reference['alt'].shape)} (alt) / {tuple(reference['objects']['ids'].shape)} (objects)")
    res = RF.roofs(alt.float(), objects_result["ids"], objects_result["n"], grid, objects_result["table"], **kwargs)
    if reference is not None:
        ro = reference["objects"]
        ref = RF.roofs(reference["alt"].float(), ro["ids"], ro["n"], grid, ro["table"], **kwargs)
        pairs = OB.match_objects(objects_result["ids"], objects_result["n"], ro["ids"], ro["n"])[0]
        res = dict(res, reference=ref, pairs=pairs, eval=RF.roof_agreement(res, ref, pairs))
    zone_string = _zone(zone_string, kwargs)
    if lines or (polygons and shared):
        res = dict(res, **_roof_arcs(res, alt.float(), objects_result["ids"], grid, zone_string, kwargs, lines, polygons and shared, simplify_m,
                                     grow_m, step_m, level_deg))
    if polygons and not shared:
        from .utils import outline as OL
        doc, outline = OL.footprints(res["facet_ids"], res["n_facets"], grid, res["parameters"]["connectivity"], simplify_m, zone_string,
                                     RF.table_records(res["facets"]))
        res = dict(res, footprints=doc, outline_stats=outline["stats"])
    files, fp = _writer(output_dp, "roofs")
    if fp:
        if polygons:
            with open(fp("facets.geojson"), "w") as f:
                json.dump(res["footprints"], f)
        if lines:
            with open(fp("lines.geojson"), "w") as f:
                json.dump(res["lines_geojson"], f)
            with open(fp("lines.json"), "w") as f:
                json.dump(res["lines_summary"], f, indent=1)
            img_utils.save_geotiff(fp("facets_grown.tif"), res["facet_ids_grown"], grid, zone_string)
        _scalar_plane(fp, "pitch", res["pitch_deg"], colormaps.COLORMAP_JET, grid, zone_string)
        _scalar_plane(fp, "residual", res["residual"], colormaps.COLORMAP_JET, grid, zone_string)
        _png(fp("aspect.png"), aspect_colors(res["code"]))
        img_utils.save_geotiff(fp("facets.tif"), res["facet_ids"], grid, zone_string)
        with open(fp("roofs.json"), "w") as f:
            json.dump({"facets": RF.table_records(res["facets"]), "buildings": RF.table_records(res["buildings"]), "stats": res["stats"],
                       "parameters": dict({"alt_key": alt_key}, **res["parameters"])}, f, indent=1)
        if reference is not None:
            with open(fp("roofs_eval.json"), "w") as f:
                json.dump(res["eval"], f, indent=1)
    return dict(res, files=files)


@torch.no_grad()
def export_solar(products, output_dp, roofs_result=None, objects_result=None, geo=None, lat_deg=None, lon_deg=None, alt_key=None,
                 zone_string=None, **kwargs):
    """The solar potential of a map (eval/utils/solar.py solar), written to `output_dp`/solar/.  `products`: what
    nadir_products, ortho_products or orthorect.rectify return ("grid" and an altitude plane); `alt_key`: default the first of "dsm",
    "median_alt", "top_alt" present.  `roofs_result`: what roofs() or export_roofs returned for them -- its slopes tilt the building
    cells (every other cell is horizontal) and its facets get a table; `objects_result`: what objects() or export_objects returned
    ("ids", "n") -- the buildings get a table.  The site's latitude and longitude: `lat_deg` / `lon_deg`, else those of the grid's
    centre through `geo`.to_scene(centre, want_lla=True) (a GeoFrame).  **kwargs (year, step_minutes, day_step, min_elevation_deg, D,
    bias, max_dist_m, suns, hours, dni, dhi, clear_sky_options) go to solar(); min_kwh_m2 to solar_table().
    Files: svf.tif / .png (BONE), sun_hours.tif / .png and insolation.tif / .png (JET), solar.json ({"parameters", "n_suns",
    "annual_dhi_kwh", "facets", "buildings"}).  Only rank 0 writes.  Returns solar()'s result plus "files", "facets" and "buildings"
    (solar_table's columns, None without the ids)."""
    from .utils import solar as SO
    from .utils.ortho import window_grid
    from .utils.roofs import table_records
    alt_key = alt_key or next((k for k in ("dsm", "median_alt", "top_alt") if k in products), None)
    if alt_key not in products:
        raise ValueError(f"export_solar: the products hold no altitude plane ({alt_key!r})")
    alt, grid = products[alt_key], window_grid(products["grid"])
    shape = tuple(alt.shape)
    for name, plane in (("roofs", None if roofs_result is None else roofs_result["slope_e"]),
                        ("objects", None if objects_result is None else objects_result["ids"])):
        if plane is not None and tuple(plane.shape) != shape:
            raise ValueError(f"export_solar: the products lie on a lattice of {shape} cells, the {name} on {tuple(plane.shape)}")
    if lat_deg is None or lon_deg is None:
        if geo is None:
            raise ValueError("export_solar: the site needs lat_deg and lon_deg, or a geo= frame to take them from")
        centre = torch.tensor([[grid.xoff + 0.5 * grid.xsize * grid.resolution, grid.yoff - 0.5 * grid.ysize * grid.resolution, 0.0]],
                              dtype=torch.float64, device=alt.device)
        lla = geo.to_scene(centre, want_lla=True)[1][0].tolist()
        lat_deg, lon_deg = lla[0] if lat_deg is None else lat_deg, lla[1] if lon_deg is None else lon_deg
    table_kw = {k: kwargs.pop(k) for k in ("min_kwh_m2",) if k in kwargs}
    slopes = (None, None) if roofs_result is None else (roofs_result["slope_e"], roofs_result["slope_n"])
    res = SO.solar(alt.float(), grid, lat_deg, lon_deg, *slopes, **kwargs)
    facets = buildings = None
    if roofs_result is not None:
        facets = SO.solar_table(res, roofs_result["facet_ids"], roofs_result["n_facets"], grid.resolution, **table_kw)
    if objects_result is not None:
        buildings = SO.solar_table(res, objects_result["ids"], objects_result["n"], grid.resolution, **table_kw)
    zone_string = _zone(zone_string, kwargs, geo)
    files, fp = _writer(output_dp, "solar")
    if fp:
        _scalar_plane(fp, "svf", res["svf"], colormaps.COLORMAP_BONE, grid, zone_string)
        _scalar_plane(fp, "sun_hours", res["sun_hours"].float(), colormaps.COLORMAP_JET, grid, zone_string)
        _scalar_plane(fp, "insolation", res["global_kwh"].float(), colormaps.COLORMAP_JET, grid, zone_string)
        with open(fp("solar.json"), "w") as f:
            json.dump({"parameters": dict({"alt_key": alt_key}, **dict(res["parameters"], **table_kw)), "n_suns": res["n_suns"],
                       "annual_dhi_kwh": res["annual_dhi_kwh"], "facets": None if facets is None else table_records(facets),
                       "buildings": None if buildings is None else table_records(buildings)}, f, indent=1)
    return dict(res, files=files, facets=facets, buildings=buildings)
