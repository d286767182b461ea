"""CPU checks of the scene loaders (DFC2019 layout) against the reference-made fixture tests/golden/scene_small_ref.npz
(tools/gen_golden_scene.py): the numpy RPC restatement, the split / t / sparsity logic, the GeoTIFF readers, the refusals,
the norm_params.json round trip and the argument checks of the new C-ABI entries (none of them touches the GPU)."""
import ctypes as C
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch

from tests import rpc_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scene_small")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "scene_small_ref.npz"))


def _root():
    with open(os.path.join(SCENE, "root.json")) as f:
        return json.load(f)


def _meta(name):
    with open(os.path.join(SCENE, "metas", name)) as f:
        return json.load(f)


def cfgs(dataset_dp=SCENE, limit=False, sparsity=2, utm=False, sem_type="own", cache_dp=None):
    run = types.SimpleNamespace(dataset_dp=dataset_dp, dataset_limit_train_images=limit, cache_dp=cache_dp,
                                dataset_name="scene_small")
    pipe = types.SimpleNamespace(use_utm_coordinate_system=utm, semantic_dataset_type=sem_type, sparsity_n_images=sparsity,
                                 epoch_subsampling_activated=False, ray_subsampling_activated=False)
    return types.SimpleNamespace(run=run, pipeline=pipe)


def numpy_rays(meta, cols, rows):
    """the rays restated independently: rpc_numpy's localisation, an own geodetic -> ECEF statement, fp32 rounding at the end"""
    cam = rpc_numpy.RPCModel(meta["rpc"])
    cols, rows = np.asarray(cols, np.float64).ravel(), np.asarray(rows, np.float64).ravel()
    pts = []
    for alt in (float(meta["max_alt"]), float(meta["min_alt"])):
        lon, lat = cam.localization(cols, rows, alt * np.ones(cols.shape))
        pts.append(np.vstack(rpc_numpy.geodetic_to_ecef(lat, lon, alt * np.ones(cols.shape))).T)
    d = pts[1] - pts[0]
    n = np.linalg.norm(d, axis=1)
    return np.hstack([pts[0], d / n[:, None], np.zeros((len(n), 1)), n[:, None]]).astype(np.float32)


def test_numpy_restatement_reproduces_the_fixture_rays(ref):
    root = _root()
    for split, names in (("train", root["train_split"]), ("test", root["train_split"][:1] + root["test_split"])):
        out = []
        for name in names:
            m = _meta(name)
            cols, rows = np.meshgrid(np.arange(m["width"]), np.arange(m["height"]))
            out.append(numpy_rays(m, cols, rows))
        got, want = np.concatenate(out), ref[f"raw_{split}_rays"]
        # the ECEF formula is stated differently from the reference's, so an fp32 value may round the other way at a tie
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(got), np.abs(want)))
        assert ulps.max() <= 1.0 and np.mean(got == want) >= 0.999, (split, ulps.max(), np.mean(got == want))


def test_projection_of_localisation_returns_the_pixel():
    """rpcm's stopping rule is 1e-18 on the squared normalised image distance: the round trip is < 1e-9 in normalised image
    units (a few 1e-8 px at these scales) for the iterative inversion, and at rounding level for the exact inverse model"""
    root = _root()
    for name in root["train_split"] + root["test_split"]:
        m = _meta(name)
        cam = rpc_numpy.RPCModel(m["rpc"])
        cols, rows = np.meshgrid(np.arange(m["width"], dtype=np.float64), np.arange(m["height"], dtype=np.float64))
        for alt in (m["min_alt"], m["max_alt"]):
            lon, lat = cam.localization(cols.ravel(), rows.ravel(), alt * np.ones(cols.size))
            c, r = cam.projection(lon, lat, alt)
            dn = np.hypot((c - cols.ravel()) / m["rpc"]["col_scale"], (r - rows.ravel()) / m["rpc"]["row_scale"])
            assert dn.max() < 1e-9, (name, dn.max())
    assert "lat_num" in _meta("JAX_068_009_RGB.json")["rpc"]


def test_split_order_t_indices_and_limit(ref):
    from snerf_amd.baseline.dataset.satnerf_dataset import split_names, t_indices
    root = _root()
    assert split_names(root, "train") == list(ref["train_names"])
    assert split_names(root, "test") == list(ref["test_data_names"])
    assert split_names(root, "train", 2) == list(ref["limit2_train_names"])
    assert t_indices(split_names(root, "train"), "train") == list(ref["train_ts"])
    assert t_indices(split_names(root, "test"), "test") == list(ref["test_ts"])


def test_rgb_and_cls_decoding_and_sparsity_mask(ref):
    from snerf_amd.semantic.dataset.semantic_dataset import SemanticDataset
    from snerf_amd.framework.util import img_utils
    ds = SemanticDataset(cfgs(sparsity=int(ref["sparsity_n_images"])), "train", device="cpu")
    rgbs, sem, mask, nocars = [], [], [], []
    for k, d in enumerate(ds.metas):
        n = d["width"] * d["height"]
        rgbs.append(img_utils.load_tensor_from_rgb_geotiff(os.path.join(ds.img_dp, d["img"])))
        extra = ds._item_extra(k, d, n)
        sem.append(extra["semantic"])
        mask.append(extra["semantic_sparsity_mask"])
        nocars.append(extra["semantic_no_cars"])
    np.testing.assert_array_equal(torch.cat(rgbs).numpy(), ref["train_rgbs"])
    np.testing.assert_array_equal(torch.cat(sem).numpy(), ref["train_semantic"])
    np.testing.assert_array_equal(torch.cat(mask).numpy(), ref["train_semantic_sparsity_mask"])
    np.testing.assert_array_equal(torch.cat(nocars).numpy(), ref["train_semantic_no_cars"])
    assert ds.semantic_n_classes == 5 and ds.car_cls_idx == 4
    assert not ref["train_semantic_sparsity_mask"].all() and ref["train_semantic_sparsity_mask"].any()
    # the test split never masks
    dt = SemanticDataset(cfgs(sparsity=1), "test", device="cpu")
    d = dt.metas[2]
    assert dt._item_extra(2, d, d["width"] * d["height"])["semantic_sparsity_mask"].all()


def test_corrupted_type_reads_the_non_corrupted_labels():
    from snerf_amd.semantic.dataset.semantic_dataset import SemanticDataset
    ds = SemanticDataset(cfgs(sem_type="own_corrupted"), "train", device="cpu")
    assert ds.semantic_non_corrupted_dp.endswith(os.path.join("semantic", "own"))
    assert ds.semantic_no_cars_dp is None        # root.json names no semantic_dp_own_corrupted_no_cars
    d = ds.metas[0]
    ex = ds._item_extra(0, d, d["width"] * d["height"])
    assert set(ex) == {"semantic", "semantic_sparsity_mask", "semantic_non_corrupted"}
    assert (ex["semantic"] != ex["semantic_non_corrupted"]).any()


def test_refusals(tmp_path):
    from snerf_amd.baseline.dataset.satnerf_dataset import SatNeRFDataset
    from snerf_amd.semantic.dataset.semantic_dataset import SemanticDataset
    from snerf_amd.framework.util import img_utils
    with pytest.raises(NotImplementedError, match="UTM"):
        SatNeRFDataset(cfgs(utm=True), "train", device="cpu")
    c = cfgs()
    c.pipeline.epoch_subsampling_activated = True
    with pytest.raises(NotImplementedError, match="epoch_subsampling_activated"):
        SatNeRFDataset(c, "train", device="cpu")
    scene = tmp_path / "scene"
    shutil.copytree(SCENE, scene)
    root = _root()
    del root["semantic_cls_labels"]
    (scene / "root.json").write_text(json.dumps(root))
    SatNeRFDataset(cfgs(dataset_dp=str(scene)), "train", device="cpu")          # the RGB loader does not need labels
    with pytest.raises(ValueError, match="semantic_cls_labels"):
        SemanticDataset(cfgs(dataset_dp=str(scene)), "train", device="cpu")
    bad = scene / "images" / "JAX_068_013_RGB.tif"
    bad.write_bytes(b"II*\x00" + b"\x00" * 40)
    with pytest.raises(ValueError, match="JAX_068_013_RGB.tif"):
        img_utils.load_tensor_from_rgb_geotiff(str(bad))


def test_norm_params_json_is_read_and_used(tmp_path, ref):
    from snerf_amd.baseline.components.normalization import StandardNormalization, norm_params_path, KEYS
    c = cfgs(cache_dp=str(tmp_path))
    fp = norm_params_path(c)
    assert fp == os.path.join(str(tmp_path), "scene_small", "normalization", "norm_params.json")
    os.makedirs(os.path.dirname(fp))
    with open(fp, "w") as f:
        json.dump(dict(zip(KEYS, ref["norm_params"].tolist())), f, indent=4)
    norm = StandardNormalization(c).initialize([])       # the file exists: used, nothing computed
    p = ref["norm_params"]
    np.testing.assert_array_equal(norm.center_range.numpy(), np.array([p[1], p[3], p[5], max(p[0], p[2], p[4])], np.float32))
    xyz = torch.tensor([[0.5, -0.25, 1.0]], dtype=torch.float64)
    back = norm.denormalize({"xyz": xyz.clone()})
    assert torch.allclose(back[0, 0], torch.tensor(p[1] + 0.5 * max(p[0], p[2], p[4]), dtype=torch.float64), atol=1.0)
    with open(fp, "w") as f:
        json.dump({"X_scale": 1.0}, f)
    with pytest.raises(ValueError, match="lack"):
        StandardNormalization(c).initialize([])


def test_abi_rejects_bad_arguments():
    from snerf_amd import _lib
    from snerf_amd.baseline.components.camera_models import rpc_struct
    L = _lib.lib()
    dummy = C.c_void_p(0x1000)        # never dereferenced: every call below is refused before any device work
    rpc = rpc_struct(_meta("JAX_068_013_RGB.json")["rpc"])

    def table(*imgs):
        t = (_lib.SnerfRayImage * len(imgs))()
        row0 = 0
        for k, (w, h, n) in enumerate(imgs):
            t[k].rpc, t[k].min_alt, t[k].max_alt = rpc, -10.0, 30.0
            t[k].w, t[k].h, t[k].row0, t[k].n_rays = w, h, row0, n
            row0 += n
        return t

    def rays(t, n_img, n_rows, pixels=None, out=dummy, fails=dummy, dev=dummy):
        return L.snerf_rpc_rays(C.byref(t) if t is not None else None, dev, n_img, pixels, n_rows, out, fails, None)

    ok = table((4, 3, 12), (5, 2, 10))
    assert rays(None, 2, 22) == 3
    assert rays(ok, 2, 22, dev=None) == 3
    assert rays(ok, 2, 22, out=None) == 3
    assert rays(ok, 2, 22, fails=None) == 3
    assert rays(ok, 0, 22) == 1
    assert rays(ok, 2, 0) == 1
    assert rays(ok, 2, 23) == 1                                     # the table does not sum to the output rows
    assert b"22 rays" in L.snerf_last_error()
    assert rays(table((4, 3, 13), (5, 2, 10)), 2, 23) == 1          # w * h != n_rays
    assert rays(table((1 << 30, 1 << 30, 12)), 1, 12) == 1          # w * h beyond any buffer
    assert rays(table((-4, 3, 12)), 1, 12) == 1
    t = table((4, 3, 12), (5, 2, 10))
    t[1].row0 = 5
    assert rays(t, 2, 22) == 1                                       # rows not contiguous
    t = table((4, 3, 12))
    t[0].min_alt = 40.0
    assert rays(t, 1, 12) == 1
    t = table((4, 3, 12))
    t[0].rpc.col_scale = 0.0
    assert rays(t, 1, 12) == 1
    # localize / project / reprojection / bounds / normalise
    assert L.snerf_rpc_localize(C.byref(rpc), dummy, None, dummy, dummy, 4, 0, dummy, dummy, dummy, None) == 3
    assert L.snerf_rpc_localize(C.byref(rpc), dummy, dummy, dummy, dummy, -1, 0, dummy, dummy, dummy, None) == 1
    assert L.snerf_rpc_project(None, dummy, dummy, dummy, dummy, 4, dummy, dummy, None) == 3
    assert L.snerf_rpc_reprojection_error(C.byref(rpc), dummy, dummy, dummy, -2, None, dummy, None) == 1
    n = (C.c_longlong * 2)(10, 0)
    assert L.snerf_ray_bounds_workspace_bytes(n, 2) == 0
    n = (C.c_longlong * 2)(10, 3000)
    ws = L.snerf_ray_bounds_workspace_bytes(n, 2)
    assert ws == (1 + 12) * 6 * 4
    ptrs = (C.c_void_p * 2)(0x1000, 0x2000)
    assert L.snerf_ray_bounds(ptrs, n, 2, dummy, dummy, ws - 1, None) == 2
    assert L.snerf_ray_bounds(ptrs, n, 0, dummy, dummy, ws, None) == 1
    assert L.snerf_ray_bounds(ptrs, n, 2, None, dummy, ws, None) == 3
    assert L.snerf_ray_bounds((C.c_void_p * 2)(0x1000, None), n, 2, dummy, dummy, ws, None) == 3
    assert L.snerf_normalize_rows(dummy, 10, 3, 1, dummy, None) == 1
    assert L.snerf_normalize_rows(dummy, 10, 8, 2, dummy, None) == 1
    assert L.snerf_normalize_rows(None, 10, 8, 1, dummy, None) == 3
    assert L.snerf_normalize_rows(dummy, -1, 8, 1, dummy, None) == 1


def test_rpc_inputs_of_different_lengths_are_refused():
    """localization / projection refuse rows, alts (lats) whose length is neither the points' nor 1 -- before any device work"""
    from snerf_amd.baseline.components.camera_models import RPCModel
    cam = RPCModel(_meta("JAX_068_013_RGB.json")["rpc"], device="cpu")
    with pytest.raises(ValueError, match="rows: 2 values for 3 points"):
        cam.localization([1.0, 2.0, 3.0], [1.0, 2.0], 0.0)
    with pytest.raises(ValueError, match="alts: 2 values for 3 points"):
        cam.localization([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="lats: 4 values for 3 points"):
        cam.projection([-81.7] * 3, [30.3] * 4, 0.0)
