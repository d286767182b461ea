#!/usr/bin/env python3
"""Write a small DFC2019-format scene and the banks the REFERENCE's own loaders build from it.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_scene.py

1. tests/golden/scene_small/: the reference's on-disk layout (what its data_prep/ writes): root.json, metas/<id>_RGB.json with
   the RPC in rpcm's dict layout (JAX-like offsets about 30.3 N, 81.7 W; off-nadir linear terms, cubic and denominator terms;
   the third train image is affine and also carries the inverse lat/lon_num/den), images/<id>_RGB.tif (8-bit RGB, uncompressed),
   semantic/{own,own_no_cars,own_corrupted}/<id>_CLS.tif (8-bit labels, class 4 = "cars"), pts3d.npy (ECEF tie points, fp64)
   and the keypoints of every train image.  Odd, non-square image sizes; five images, 5,107 pixels in all.
2. tests/golden/scene_small_ref.npz: the reference's SemanticDataset (train and test split), its _handle_normalization
   sequence (base_ray_pipeline.py:198-244: parameters from the train + test rays, both normalised, the depth set loaded with
   the cached parameters) and SatNeRFDepthDataset, with sparsity_n_images = 2; the split names of dataset_limit_train_images = 2.

Shims for what is not installed: rpcm is tests/rpc_numpy.py (an fp64 numpy restatement of rpcm's RPCModel); rasterio.open is a
PIL reader returning (bands, h, w); torchvision's ToTensor is its three-line equivalent for an (h, w, c) ndarray
(torch.from_numpy(x.transpose(2, 0, 1))); utm, pymap3d, lightning, ... are inert stubs (never called on this path).  The
reference's StandardNormalization json.dump()s numpy float32 scalars, which json refuses: its write_dict_to_json is wrapped to
write float(value) -- the exact decimal of the fp32 value, so the read-back parameters are the same fp32 numbers.
Every file regenerates byte for byte."""
import importlib.abc
import importlib.machinery
import json
import os
import shutil
import sys
import tempfile
import types
import typing

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
SCENE = os.path.join(OUT, "scene_small")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rpc_numpy  # noqa: E402

STUBBED = ("toml", "gpustat", "lightning", "pytorch_lightning", "torchmetrics", "fire", "cv2", "pymap3d", "utm", "matplotlib")
AOI = "JAX_068"
TRAIN = [("013", 41, 37), ("007", 33, 29), ("009", 27, 35)]     # (image id, w, h); 013 is the first test image too
TEST = [("002", 31, 23), ("005", 25, 39)]                        # 002 -> t = 8 (predefined_val_ts), 005 -> unknown -> 0
INVERSE_ID = "009"
CLS_LABELS = {"0": "ground", "1": "trees", "2": "buildings", "3": "water", "4": "cars"}
SPARSITY = 2
N_TIE = 60


class _Inert:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return _Inert()

    def __getattr__(self, name):
        return _Inert()


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (_Inert,), {})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUBBED:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StubModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


class _Raster:
    def __init__(self, fp):
        self.fp = fp

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def read(self):
        a = np.array(Image.open(self.fp))
        return a[None] if a.ndim == 2 else np.transpose(a, (2, 0, 1))


def _install_shims():
    sys.meta_path.insert(0, _StubFinder())
    import torch.utils.data.dataset as tud
    if not hasattr(tud, "T_co"):
        tud.T_co = typing.TypeVar("T_co", covariant=True)
    rpcm = types.ModuleType("rpcm")
    rpcm.RPCModel = rpc_numpy.RPCModel
    rpcm.MaxLocalizationIterationsError = rpc_numpy.MaxLocalizationIterationsError
    sys.modules["rpcm"] = rpcm
    rasterio = types.ModuleType("rasterio")
    rasterio.open = lambda fp, mode="r": _Raster(fp)
    sys.modules["rasterio"] = rasterio
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class ToTensor:
        def __call__(self, pic):
            return torch.from_numpy(pic.transpose((2, 0, 1))).contiguous()
    tr.ToTensor = ToTensor
    tr.Resize = _Inert
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    sys.path.insert(0, REF)
    import framework.util.file_utils as fu
    write = fu.write_dict_to_json
    fu.write_dict_to_json = lambda d, fp: write({k: (float(v) if isinstance(v, np.floating) else v) for k, v in d.items()}, fp)


# ---- 1. the scene -------------------------------------------------------------------------------------------------------------
def _name(i):
    return f"{AOI}_{i}_RGB"


def _meta(i, w, h, seed):
    rpc = rpc_numpy.synthetic_rpc(seed, w=w, h=h, inverse=(i == INVERSE_ID))
    rng = np.random.default_rng(seed + 100)
    # all views look at the same area: a common centre, jittered by a few metres (the normalised model is unchanged)
    rpc["lat_offset"] = 30.3 + rng.uniform(-2e-5, 2e-5)
    rpc["lon_offset"] = -81.7 + rng.uniform(-2e-5, 2e-5)
    return {"img": _name(i) + ".tif", "height": h, "width": w, "min_alt": -25.0 + rng.uniform(-3, 3),
            "max_alt": 45.0 + rng.uniform(-3, 3), "sun_elevation": float(rng.uniform(40, 70)),
            "sun_azimuth": float(rng.uniform(100, 170)), "rpc": rpc}


def write_scene():
    if os.path.isdir(SCENE):
        shutil.rmtree(SCENE)
    for sub in ("images", "metas", "semantic/own", "semantic/own_no_cars", "semantic/own_corrupted"):
        os.makedirs(os.path.join(SCENE, sub))
    rng = np.random.default_rng(2019)
    metas = {}
    for k, (i, w, h) in enumerate(TRAIN + TEST):
        metas[i] = _meta(i, w, h, 40 + k)
    # tie points: ground points inside the footprint of every train image, ECEF fp64
    m0 = metas[TRAIN[0][0]]["rpc"]
    lat = m0["lat_offset"] + rng.uniform(-0.6, 0.6, N_TIE) * m0["lat_scale"]
    lon = m0["lon_offset"] + rng.uniform(-0.6, 0.6, N_TIE) * m0["lon_scale"]
    alt = rng.uniform(-15.0, 35.0, N_TIE)
    from framework.util.conversions import latlon_to_ecef_custom      # the reference's own conversion
    pts3d = np.stack(latlon_to_ecef_custom(lat, lon, alt), 1)
    np.save(os.path.join(SCENE, "pts3d.npy"), pts3d)
    for i, w, h in TRAIN:
        cam = rpc_numpy.RPCModel(metas[i]["rpc"])
        col, row = cam.projection(lon, lat, alt)
        col = col + rng.normal(0, 0.3, N_TIE)             # keypoint detections: noisy, so the reprojection errors differ
        row = row + rng.normal(0, 0.3, N_TIE)
        keep = np.nonzero((col >= 0) & (col <= w - 1) & (row >= 0) & (row <= h - 1) & (rng.random(N_TIE) < 0.85))[0]
        metas[i]["keypoints"] = {"2d_coordinates": np.stack([col[keep], row[keep]], 1).tolist(),
                                 "pts3d_indices": keep.tolist()}
    for i, w, h in TRAIN + TEST:
        with open(os.path.join(SCENE, "metas", _name(i) + ".json"), "w") as f:
            json.dump(metas[i], f, indent=2)
        yy, xx = np.mgrid[0:h, 0:w]
        rgb = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), rng.integers(0, 256, (h, w))], 2)
        Image.fromarray(rgb.astype(np.uint8), "RGB").save(os.path.join(SCENE, "images", _name(i) + ".tif"), compression=None)
        lab = rng.choice(4, (h, w)).astype(np.uint8)
        lab[rng.random((h, w)) < 0.08] = 4
        no_cars = np.where(lab == 4, 0, lab).astype(np.uint8)
        corrupt = lab.copy()
        flip = rng.random((h, w)) < 0.2
        corrupt[flip] = rng.choice(5, int(flip.sum()))
        for sub, a in (("own", lab), ("own_no_cars", no_cars), ("own_corrupted", corrupt)):
            Image.fromarray(a, "L").save(os.path.join(SCENE, "semantic", sub, f"{AOI}_{i}_CLS.tif"), compression=None)
    root = {"aoi_name": AOI, "img_dp": "images", "meta_dp": "metas", "dsm_txt_fp": "dsm/JAX_068_DSM.txt",
            "dsm_tif_fp": "dsm/JAX_068_DSM.tif", "zone_string": "17R", "points3d_fp": "pts3d.npy",
            "train_split": [_name(i) + ".json" for i, _, _ in TRAIN], "test_split": [_name(i) + ".json" for i, _, _ in TEST],
            "semantic_dp_own": "semantic/own", "semantic_dp_own_no_cars": "semantic/own_no_cars",
            "semantic_dp_own_corrupted": "semantic/own_corrupted", "semantic_cls_labels": CLS_LABELS}
    with open(os.path.join(SCENE, "root.json"), "w") as f:
        json.dump(root, f, indent=2)


# ---- 2. the reference's banks -------------------------------------------------------------------------------------------------
def _cfgs(cache_dp, limit=False):
    run = types.SimpleNamespace(dataset_dp=SCENE, cache_dp=cache_dp, dataset_name="scene_small", dataset_limit_train_images=limit)
    pipe = types.SimpleNamespace(use_utm_coordinate_system=False, semantic_dataset_type="own", sparsity_n_images=SPARSITY,
                                 epoch_subsampling_activated=False)
    return types.SimpleNamespace(run=run, pipeline=pipe)


def reference_banks():
    from semantic.dataset.semantic_dataset import SemanticDataset
    from baseline.dataset.satnerf_depth_dataset import SatNeRFDepthDataset
    out = {}
    with tempfile.TemporaryDirectory() as cache:
        cfgs = _cfgs(cache)
        ds = {"rgb": SemanticDataset(cfgs, "scene_small", "train"), "rgb_test": SemanticDataset(cfgs, "scene_small", "test")}
        for d in ds.values():
            d.load()
        out["raw_train_rays"] = ds["rgb"].combined_data["rays"].numpy().copy()
        out["raw_test_rays"] = ds["rgb_test"].combined_data["rays"].numpy().copy()
        # base_ray_pipeline.py _handle_normalization
        combined = torch.cat((ds["rgb"].combined_data["rays"], ds["rgb_test"].combined_data["rays"]), dim=0)
        for d in ds.values():
            d.initialize_normalization(combined_data={"rays": combined})
        for d in ds.values():
            d.save_to_cache()
            d.normalize()
        depth = SatNeRFDepthDataset(cfgs, "scene_small", "train")
        depth.initialize_normalization()
        depth.load()
        depth.normalize()
        with open(os.path.join(cache, "scene_small", "normalization", "norm_params.json")) as f:
            params = json.load(f)
        out["norm_params"] = np.array([params[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")],
                                      np.float64)
        tr = ds["rgb"].combined_data
        for key in ("rays", "rgbs", "extras", "semantic", "semantic_sparsity_mask", "semantic_no_cars"):
            out[f"train_{key}"] = tr[key].numpy()
        items = ds["rgb_test"].data
        out["test_image_sizes"] = np.array([it["rays"].shape[0] for it in items], np.int64)
        out["test_w"] = np.array([it["w"] for it in items], np.int64)
        out["test_h"] = np.array([it["h"] for it in items], np.int64)
        for key in ("rays", "rgbs", "extras", "semantic", "semantic_no_cars"):
            out[f"test_{key}"] = torch.cat([it[key] for it in items], 0).numpy()
        out["test_names"] = np.array([it["name"] for it in items])
        out["test_ts"] = np.array([int(it["extras"][0, 3]) for it in items], np.int64)
        dc = depth.combined_data
        for key in ("rays", "depths", "weights", "extras"):
            out[f"depth_{key}"] = dc[key].numpy()
        out["depth_kp_weights"] = np.asarray(depth.kp_weights)
        out["train_names"] = np.array(ds["rgb"].data_names)
        out["test_data_names"] = np.array(ds["rgb_test"].data_names)
        out["train_ts"] = np.array([int(it["extras"][0, 3]) for it in ds["rgb"].data], np.int64)
    with tempfile.TemporaryDirectory() as cache:
        out["limit2_train_names"] = np.array(SemanticDataset(_cfgs(cache, limit=2), "scene_small", "train").data_names)
    return out


def main():
    _install_shims()
    write_scene()
    out = reference_banks()
    out["sparsity_n_images"] = np.int64(SPARSITY)
    np.savez_compressed(os.path.join(OUT, "scene_small_ref.npz"), **out)
    for dp, _, files in sorted(os.walk(SCENE)):
        for f in sorted(files):
            print(os.path.relpath(os.path.join(dp, f), ROOT), os.path.getsize(os.path.join(dp, f)))
    print("tests/golden/scene_small_ref.npz", os.path.getsize(os.path.join(OUT, "scene_small_ref.npz")))


if __name__ == "__main__":
    main()
