"""Scene loader -- mirror of baseline/dataset/satnerf_dataset.py and framework/datasets.py (BaseDataset.load and the test views' t)
for a scene in the reference's on-disk layout (the output of its data_prep/): root.json, one meta JSON per image with the RPC,
8-bit RGB GeoTIFFs.  The rays of a split are built on the device in one launch (baseline/components/rays.py); the loader
returns GpuRayBanks with the reference's columns and row order: train = the images of the split concatenated in split order;
test = train_split[:1] + test_split, with `image_sizes` and the per-image dicts of `images()`.  Rays are rebuilt on every load
(the reference's on-disk ray cache is not read or written).

World coordinates: once load_scene_banks has attached the normalisation, `geo` is a GeoFrame (framework/components/
coordinate_systems.py) of the scene's zone (root.json "zone_string"), and get_latlonalt_from_nerf_prediction /
get_latlonalt_from_points answer on the device (satnerf_dataset.py:156-206).  When root.json's dsm_tif_fp and dsm_txt_fp exist
on disk, the ground-truth DSM is loaded (framework/util/img_utils.py) and every dict of `scene_images()` carries
"dsm": {"gt", "roi", "water_mask" | "ignore_mask", "geo"}; a scene without those files loads exactly as one that does not
name them."""
import json
import os

import numpy as np
import torch

from ...framework.components.coordinate_systems import init_coordinate_system
from ...framework.datasets import GpuRayBank
from ...framework.util import img_utils
from ..components.camera_models import construct_rpc_camera_model
from ..components.rays import construct_sun_dir, satnerf_construct


TRAIN_KEYS = ("rays", "rgbs", "extras", "semantic", "semantic_sparsity_mask")


def read_json(fp):
    with open(fp) as f:
        return json.load(f)


def get_file_id(filename):
    return os.path.splitext(os.path.basename(filename))[0]


# Transient-embedding index of the test views of the four DFC2019 scenes the reference evaluates on (data of its
# framework/datasets.py, taken from the original Sat-NeRF); a test view not listed here gets index 0.
VAL_T_INDEX = {
    "JAX_004_009_RGB": 5, "JAX_004_014_RGB": 0, "JAX_004_022_RGB": 0,
    "JAX_068_002_RGB": 8, "JAX_068_012_RGB": 1, "JAX_068_013_RGB": 0,
    "JAX_214_001_RGB": 18, "JAX_214_006_RGB": 8, "JAX_214_008_RGB": 2, "JAX_214_020_RGB": 0,
    "JAX_260_004_RGB": 10, "JAX_260_006_RGB": 3, "JAX_260_015_RGB": 0,
}


def split_names(root: dict, split: str, limit=False):
    if split == "train":
        names = list(root["train_split"])
        if limit:
            names = names[: int(limit)]
        return names
    return list(root["train_split"][:1]) + list(root["test_split"])


def t_indices(names, split):
    """the reference's `index` per image: the position on the train split; on the test split 0 for the first image (a training
    view) and VAL_T_INDEX of the image id (0 when it is not listed) for the others"""
    if split == "train":
        return list(range(len(names)))
    return [0] + [VAL_T_INDEX.get(get_file_id(name), 0) for name in names[1:]]


def unlisted_test_views(names):
    """the names (files or ids, in order) that VAL_T_INDEX does not list: as test views they fall back to row 0 of the embedding
    table, another image's appearance -- the views whose embedding a caller fits instead (eval/utils/embedding.py)"""
    return [name for name in names if get_file_id(name) not in VAL_T_INDEX]


def refuse_unsupported(cfgs):
    init_coordinate_system(cfgs)
    pc = cfgs.pipeline
    for key in ("epoch_subsampling_activated", "ray_subsampling_activated"):
        if getattr(pc, key, False):
            raise NotImplementedError(f"{key} is not supported on scenes loaded from disk")


class SatNeRFDataset:
    """one split of a scene; `load()` fills `self.t` (the bank's tensors, un-normalised rays) and the per-image metadata"""

    def __init__(self, cfgs, split: str, device=None):
        refuse_unsupported(cfgs)
        self.cfgs, self.split = cfgs, split
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.dataset_dp = cfgs.run.dataset_dp
        self.root = read_json(os.path.join(self.dataset_dp, "root.json"))
        self.img_dp = os.path.join(self.dataset_dp, self.root["img_dp"])
        self.meta_dp = os.path.join(self.dataset_dp, self.root["meta_dp"])
        self.data_names = split_names(self.root, split, cfgs.run.dataset_limit_train_images)
        if not self.data_names:
            raise ValueError(f"scene {self.dataset_dp!r}: the {split} split is empty")
        self.ts = t_indices(self.data_names, split)
        self.metas = [read_json(os.path.join(self.meta_dp, n)) for n in self.data_names]
        self.t = None
        self.items = None
        self.zone_string = self.root.get("zone_string")
        self.dsm_tif_fp, self.dsm_txt_fp, self.dsm_cls_fp, self.ignore_mask_fp = (
            os.path.join(self.dataset_dp, self.root[k]) if self.root.get(k) else None
            for k in ("dsm_tif_fp", "dsm_txt_fp", "dsm_cls_fp", "ignore_mask_fp"))
        self.normalization_component = None
        self.geo = None       # GeoFrame, set by attach_normalization
        self.dsm = None       # the images' "dsm" entry, when the ground truth is on disk

    def attach_normalization(self, norm):
        """the scene's normalisation -> `geo`, and the ground-truth DSM entry when its files are on disk"""
        from ...framework.components.coordinate_systems import GeoFrame
        self.normalization_component = norm
        if self.zone_string:
            self.geo = GeoFrame(norm, self.zone_string)
        if self.geo is not None and all(fp and os.path.isfile(fp) for fp in (self.dsm_tif_fp, self.dsm_txt_fp)):
            gt = img_utils.load_dsm_ground_truth(self.dsm_tif_fp, self.dsm_txt_fp, self.dsm_cls_fp, self.ignore_mask_fp)
            self.dsm = {k: v.to(self.device) for k, v in gt.items()}
            self.dsm["geo"] = self.geo
        return self

    def _need_geo(self):
        if self.geo is None:
            raise ValueError("world coordinates need the scene's normalisation and a root.json zone_string "
                             "(load the scene through load_scene_banks)")
        return self.geo

    def get_xyz_from_nerf_prediction(self, rays, depth):
        """normalised end points o + d * depth in fp64 (satnerf_dataset.py:156-171)"""
        from ...eval.extract_pointcloud import get_xyz_from_nerf_prediction
        return get_xyz_from_nerf_prediction(rays, depth)

    def get_latlonalt_from_nerf_prediction(self, rays, depth):
        """(lats, lons, alts) fp64 device tensors of the rays' end points (satnerf_dataset.py:173-187); fp32 rays and depth
        take the fused launch, anything else goes through get_xyz_from_nerf_prediction"""
        if rays.dtype == torch.float32 and depth.dtype == torch.float32:
            lla = self._need_geo().cloud(rays, depth, want_lla=True)[1]
            return lla[:, 0], lla[:, 1], lla[:, 2]
        return self.get_latlonalt_from_points(self.get_xyz_from_nerf_prediction(rays, depth))

    def get_latlonalt_from_points(self, points):
        """(lats, lons, alts) fp64 device tensors of normalised points (satnerf_dataset.py:189-206)"""
        lla = self._need_geo().points(points, want_lla=True)[1]
        return lla[:, 0], lla[:, 1], lla[:, 2]

    def _rays(self):
        cams = [construct_rpc_camera_model(d, self.device) for d in self.metas]
        sizes = [(int(d["width"]), int(d["height"])) for d in self.metas]
        return satnerf_construct(cams, [float(d["min_alt"]) for d in self.metas], [float(d["max_alt"]) for d in self.metas],
                                 sizes=sizes, names=self.data_names, device=self.device)

    def _item_extra(self, k, d, n):
        """per-image additional columns (the semantic loader's labels)"""
        return {}

    def load(self):
        rays = self._rays()
        cols = {"rgbs": [], "extras": []}
        self.items = []
        for k, (d, t) in enumerate(zip(self.metas, self.ts)):
            rgbs = img_utils.load_tensor_from_rgb_geotiff(os.path.join(self.img_dp, d["img"]))
            h, w = int(d["height"]), int(d["width"])
            if rgbs.shape[0] != h * w:
                raise ValueError(f"{self.data_names[k]}: the RGB image has {rgbs.shape[0]} pixels, the meta says {w} x {h}")
            sun = construct_sun_dir(float(d["sun_elevation"]), float(d["sun_azimuth"]), h * w)
            cols["rgbs"].append(rgbs)
            cols["extras"].append(torch.hstack([sun, t * torch.ones(h * w, 1)]))
            for key, v in self._item_extra(k, d, h * w).items():
                cols.setdefault(key, []).append(v)
            self.items.append({"name": get_file_id(d["img"]), "w": w, "h": h, "alt_min": float(d["min_alt"]),
                               "alt_max": float(d["max_alt"]), "n": h * w})
        self.t = {"rays": rays}
        for key, v in cols.items():
            self.t[key] = torch.cat(v, 0).to(self.device)
        return self

    def bank(self, n_classes=5, car_cls_idx=4, seed=0):
        """n_classes / car_cls_idx: the values a non-semantic pipeline's banks carry (SatNeRFPipeline._n_classes); the train bank carries the columns of the reference's train __getitem__ (satnerf_dataset.py:122-133,
        semantic_dataset.py:83-90); the test bank every column and `image_sizes`"""
        test = self.split != "train"
        sizes = [it["n"] for it in self.items] if test else None
        wh = [(it["w"], it["h"]) for it in self.items] if test else None
        t = self.t if test else {k: v for k, v in self.t.items() if k in TRAIN_KEYS}
        b = GpuRayBank(t, n_classes=n_classes, car_cls_idx=car_cls_idx, seed=seed, image_sizes=sizes, image_wh=wh)
        b.scene_images = self.images_of(b)
        return b

    def images_of(self, bank):
        """callable: the per-image dicts (name, rays, extras, rgbs, w, h and the label columns) of the bank's current tensors
        -- what eval_nerf_images / eval_semantic_images take"""
        items = self.items
        ds = self

        def images():
            out, lo = [], 0
            for it in items:
                hi = lo + it["n"]
                d = {"name": it["name"], "w": it["w"], "h": it["h"]}
                for key, v in bank.t.items():
                    if key != "semantic_sparsity_mask":
                        d[key] = v[lo:hi]
                if ds.dsm is not None:
                    d["dsm"] = ds.dsm
                out.append(d)
                lo = hi
            return out
        return images


def load_scene_banks(cfgs, semantic: bool, depth: bool, device=None, seed=0) -> dict:
    """the pipeline's datasets from `run.dataset_dp`, in the order of base_ray_pipeline.py:198-244 (_handle_normalization):
    train and test rays built, normalisation parameters from both (or read from norm_params.json), both normalised, then
    the depth set built and normalised with the same parameters (pipeline.depth_source: the tie points, a DSM seen through the
    training rays -- dsm_depth_dataset.py --, or both).  Returns {"rgb", "rgb_test"[, "depth"]} GpuRayBanks; the
    test bank's `scene_images()` gives the per-image dicts of the evaluation functions."""
    from ..components.normalization import StandardNormalization
    from ...parallel import world
    if semantic:
        from ...semantic.dataset.semantic_dataset import SemanticDataset as DS
    else:
        DS = SatNeRFDataset
    train, test = DS(cfgs, "train", device).load(), DS(cfgs, "test", device).load()
    norm = StandardNormalization(cfgs, rank=world()[0]).initialize([train.t["rays"], test.t["rays"]])
    for ds in (train, test):
        norm.normalize_rays_(ds.t["rays"])
        ds.attach_normalization(norm)
    out = {"rgb": train.bank(seed=seed), "rgb_test": test.bank(seed=seed + 1)}
    source = getattr(cfgs.pipeline, "depth_source", "tie_points") if depth else None
    if depth and source == "tie_points":
        from .satnerf_depth_dataset import SatNeRFDepthDataset
        out["depth"] = SatNeRFDepthDataset(cfgs, device).load(norm).bank(out["rgb"].semantic_n_classes, out["rgb"].car_cls_idx,
                                                                        seed=seed + 2)
    elif depth:
        # depth_source "dsm": the dense prior alone (a scene without points3d_fp will do); "both": the tie points' rows, then the prior's
        from .dsm_depth_dataset import DsmDepthDataset, prior_settings
        prior_settings(cfgs.pipeline)
        parts = []
        if source == "both":
            from .satnerf_depth_dataset import SatNeRFDepthDataset
            parts.append(SatNeRFDepthDataset(cfgs, device).load(norm).t)
        parts.append(DsmDepthDataset(cfgs, device).load(norm).t)
        t = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
        out["depth"] = GpuRayBank(t, n_classes=out["rgb"].semantic_n_classes, car_cls_idx=out["rgb"].car_cls_idx, seed=seed + 2)
    for b in out.values():
        b.normalization = norm
    out["rgb"].dataset, out["rgb_test"].dataset = train, test
    return out
