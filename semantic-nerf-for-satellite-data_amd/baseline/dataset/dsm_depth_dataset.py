"""A DSM as a dense depth prior: the columns of SatNeRFDepthDataset -- rays (R, 8), depths (R, 1), weights (R, 1), extras (R, 4), as
the depth step consumes them -- from a coarse DSM seen through the training rays, not from the sparse bundle-adjustment tie
points.  The reference has no counterpart (its depth branch is fed by points3d_fp alone); DESIGN.md section 5v.

The DSM is a single-band float GeoTIFF with ModelPixelScale / ModelTiepoint tags, read by img_utils.load_dsm_geotiff: the form
img_utils.save_geotiff writes, so a product of eval/ortho.py (export_ortho, export_nadir) can be fed back, as can a lidar or
stereo DSM in the scene's UTM zone.  Cells that are not finite, or below -500 m (a lidar product's no-data value, as in
eval/utils/shadow.py), are holes.  The rays of every `stride`-th pixel (columns 0, stride, ...; rows likewise) of every train
image are built by the ray kernel (satnerf_construct(pixels=...)), normalised with the parameters shared with the RGB banks and
cast on the DSM (eval/utils/raycast.py cast_rays); the rows that hit (TOP, WALL, START) are kept, their depth is the cast depth
and their weight the constant `depth_prior_weight`.

Out of scope: confidence weights from the DSM's own uncertainty, resampling a DSM given in another zone or projection, guiding
the training passes' sampling by the prior."""
import math
import os

import numpy as np
import torch

from ...framework.datasets import GpuRayBank
from ...framework.util import img_utils
from ..components.camera_models import construct_rpc_camera_model
from ..components.rays import construct_sun_dir, satnerf_construct
from .satnerf_dataset import read_json, refuse_unsupported, split_names

HOLE_BELOW = -500.0      # eval/utils/shadow.py GT_HOLE_BELOW
DEPTH_SOURCES = ("tie_points", "dsm", "both")


def prior_settings(pipeline_cfg):
    """(source, file, stride, weight) of the config's depth_* fields, checked: a source other than "tie_points" needs a file, a
    stride >= 1 and a positive finite weight"""
    source = getattr(pipeline_cfg, "depth_source", "tie_points")
    if source not in DEPTH_SOURCES:
        raise ValueError(f"depth_source must be one of {DEPTH_SOURCES}, got {source!r}")
    fp = str(getattr(pipeline_cfg, "depth_prior_dsm_fp", "") or "")
    stride = int(getattr(pipeline_cfg, "depth_prior_stride", 4))
    weight = float(getattr(pipeline_cfg, "depth_prior_weight", 1.0))
    if stride < 1:
        raise ValueError(f"depth_prior_stride must be >= 1, got {stride}")
    if not (math.isfinite(weight) and weight > 0.0):
        raise ValueError(f"depth_prior_weight must be positive and finite, got {weight}")
    if source != "tie_points" and not fp:
        raise ValueError(f"depth_source = {source!r} needs depth_prior_dsm_fp, the DSM GeoTIFF")
    return source, fp, stride, weight


def load_prior_dsm(fp):
    """the DSM GeoTIFF `fp` -> ((H, W) float32 ndarray with NaN holes, DsmGrid).  A file without a georeference, with pixels that are
    not square or with a raster that is not floating point is a ValueError."""
    from ...eval.utils.dsm import DsmGrid
    a, tf = img_utils.load_dsm_geotiff(fp)
    if tf is None:
        raise ValueError(f"DSM GeoTIFF {fp!r} carries no georeference (ModelPixelScale / ModelTiepoint): a depth prior needs one")
    x0, y0, sx, sy = tf
    if abs(sx - sy) > 1e-9 * sx:
        raise ValueError(f"DSM GeoTIFF {fp!r}: pixels of {sx} x {sy} m are not square")
    if a.dtype.kind != "f":
        raise ValueError(f"DSM GeoTIFF {fp!r}: expected a float raster of altitudes, got {a.dtype}")
    dsm = np.ascontiguousarray(a, np.float32)
    dsm[~np.isfinite(dsm) | (dsm < HOLE_BELOW)] = np.nan
    return dsm, DsmGrid(float(x0), float(y0), float(sx), int(dsm.shape[1]), int(dsm.shape[0]))


def strided_pixels(w, h, stride):
    """(n, 2) fp64 (col, row) of every `stride`-th pixel of a w x h image, row-major: columns 0, stride, ... < w in rows 0, stride, ... < h"""
    cols, rows = np.arange(0, int(w), int(stride), dtype=np.float64), np.arange(0, int(h), int(stride), dtype=np.float64)
    return np.stack([np.tile(cols, len(rows)), np.repeat(rows, len(cols))], 1)


def image_extras(meta, t, n):
    """(n, 4) fp32: the image's sun direction and its index `t`, as SatNeRFDepthDataset builds them"""
    return torch.hstack([construct_sun_dir(float(meta["sun_elevation"]), float(meta["sun_azimuth"]), n), t * torch.ones(n, 1)])


class DsmDepthDataset:
    def __init__(self, cfgs, device=None):
        refuse_unsupported(cfgs)
        self.cfgs = cfgs
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        _, self.dsm_fp, self.stride, self.weight = prior_settings(cfgs.pipeline)
        if not self.dsm_fp:
            raise ValueError("DsmDepthDataset needs depth_prior_dsm_fp, the DSM GeoTIFF")
        self.dataset_dp = cfgs.run.dataset_dp
        self.root = read_json(os.path.join(self.dataset_dp, "root.json"))
        if not self.root.get("zone_string"):
            raise ValueError(f"scene {self.dataset_dp!r}: root.json has no 'zone_string' (a DSM depth prior needs the scene's UTM zone)")
        self.meta_dp = os.path.join(self.dataset_dp, self.root["meta_dp"])
        self.data_names = split_names(self.root, "train", cfgs.run.dataset_limit_train_images)
        self.metas = [read_json(os.path.join(self.meta_dp, n)) for n in self.data_names]
        self.prior, self.grid = load_prior_dsm(self.dsm_fp)
        self.pixels = [strided_pixels(d["width"], d["height"], self.stride) for d in self.metas]
        self.t = None
        self.states = None      # the cast's (top, wall, start, end, outside, bad) totals over the candidate rays

    def load(self, normalization):
        from ...eval.utils import raycast
        from ...framework.components.coordinate_systems import GeoFrame
        cams = [construct_rpc_camera_model(d, self.device) for d in self.metas]
        rays = satnerf_construct(cams, [float(d["min_alt"]) for d in self.metas], [float(d["max_alt"]) for d in self.metas],
                                 pixels=self.pixels, names=self.data_names, device=self.device)
        normalization.normalize_rays_(rays)
        cast = raycast.cast_rays(rays, GeoFrame(normalization, self.root["zone_string"]), self.grid,
                                 torch.from_numpy(self.prior).to(self.device))
        keep = raycast.is_hit(cast["state"])
        self.states = torch.bincount(cast["state"].long(), minlength=6).cpu().tolist()
        if not bool(keep.any()):
            raise ValueError(f"DSM {self.dsm_fp!r}: none of the {rays.shape[0]} candidate rays meets it (states {self.states}): is it in "
                             f"the scene's zone {self.root['zone_string']}?")
        extras = torch.cat([image_extras(d, t, p.shape[0]) for t, (d, p) in enumerate(zip(self.metas, self.pixels))], 0).to(self.device)
        depths = cast["depth"][keep]
        self.t = {"rays": rays[keep].contiguous(), "depths": depths[:, None].contiguous(),
                  "weights": torch.full((depths.shape[0], 1), self.weight, dtype=torch.float32, device=self.device),
                  "extras": extras[keep].contiguous()}
        return self

    def bank(self, n_classes=5, car_cls_idx=4, seed=0):
        return GpuRayBank(self.t, n_classes=n_classes, car_cls_idx=car_cls_idx, seed=seed)
