"""World clouds on the GPU (csrc/geo.hip through the C-ABI and snerf_amd's GeoFrame): stage parity with the reference's own
arrays (tests/golden/geo_cloud_small.npz, tools/gen_golden_geo.py), tails, the fused bounds, the non-finite count, the southern
flag, and the path from a scene on disk to the altitude MAE (tests/golden/scene_small_dsm).

Bars.  xyz_n and ECEF: bit-equal (two roundings per component, as torch's separate fp64 ops).  lat / lon within 1e-12 deg and alt
within 1e-6 m of the reference's ecef_to_latlon_custom, east / north within 1e-6 m of the numpy restatement of the utm series
(tests/utm_numpy.py; the utm package itself is not installed: UNPINNED): the coordinates are about 6.4e6 m, where one fp64 ulp
is 9e-10 m; alt = p / cos(lat) - N cancels two such values and the series is a few dozen operations, so 1e-6 m is three orders
above the rounding and six below the 0.5 m DSM cell.  The kernel's xyz_n and ECEF are not outputs of the ABI: the test pins
torch's fp64 ops on the device to the reference's arrays bit for bit, and the kernel to them through snerf_geo_points (entered
with the reference's xyz_n) giving bit for bit what snerf_geo_cloud gives from the rays."""
import ctypes as C
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DSM_DIR = os.path.join(GOLDEN, "scene_small_dsm")
DEV = torch.device("cuda:0")
KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "geo_cloud_small.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(DSM_DIR, "expected.json")) as f:
        return json.load(f)


def _norm(fx):
    from snerf_amd.baseline.components.normalization import StandardNormalization
    return StandardNormalization().set_params(dict(zip(KEYS, fx["norm_params"].tolist())))


@pytest.fixture(scope="module")
def frame(fx):
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    return GeoFrame(_norm(fx), str(fx["zone_string"]))


@pytest.fixture(scope="module")
def dev(fx):
    return {"rays": torch.from_numpy(fx["rays"]).to(DEV), "depth": torch.from_numpy(fx["depth"]).to(DEV),
            "xyz_n": torch.from_numpy(fx["xyz_n"]).to(DEV)}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _run(params, n, rays=None, depth=None, xyz_n=None, want_lla=True):
    """one raw launch through the C-ABI -> (enu, lla, stats words as unsigned ints, return code)"""
    from snerf_amd import _lib
    L = _lib.lib()
    enu = torch.full((n, 3), -7.0, dtype=torch.float64, device=DEV)
    lla = torch.full((n, 3), -7.0, dtype=torch.float64, device=DEV) if want_lla else None
    stats = torch.tensor([-1, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    if xyz_n is None:
        rc = L.snerf_geo_cloud(_ptr(rays), rays.shape[1], _ptr(depth), n, C.byref(params), _ptr(enu), _ptr(lla), _ptr(stats), st)
    else:
        rc = L.snerf_geo_points(_ptr(xyz_n), n, C.byref(params), _ptr(enu), _ptr(lla), _ptr(stats), st)
    torch.cuda.synchronize()
    return enu, lla, [int(w) & U64 for w in stats.cpu().tolist()], rc


@pytest.fixture(scope="module")
def full(frame, dev):
    """the whole fixture through snerf_geo_cloud, once; the tests below only read it"""
    enu, lla, stats, rc = _run(frame.params, dev["rays"].shape[0], dev["rays"], dev["depth"])
    assert rc == 0
    return {"enu": enu, "lla": lla, "stats": stats}


def _bits(t):
    return t.contiguous().view(torch.int64)


def _torch_bounds(enu):
    from snerf_amd.framework.components.coordinate_systems import GeoBounds
    fin = torch.isfinite(enu).all(1)
    e = enu[fin]
    return GeoBounds(float(e[:, 0].min()), float(e[:, 0].max()), float(e[:, 1].min()), float(e[:, 1].max()))


def test_stage_parity_with_the_reference(fx, frame, dev, full):
    from snerf_amd.eval.extract_pointcloud import get_xyz_from_nerf_prediction
    xyz_n = get_xyz_from_nerf_prediction(dev["rays"], dev["depth"])
    assert np.array_equal(xyz_n.cpu().numpy().view(np.int64), fx["xyz_n"].view(np.int64))
    ecef = _norm(fx).denormalize({"xyz": xyz_n})
    assert ecef.dtype == torch.float64 and np.array_equal(ecef.cpu().numpy().view(np.int64), fx["ecef"].view(np.int64))
    # the kernel's own steps 1 and 2: entered at step 2 with the REFERENCE's xyz_n it gives what it gives from the rays
    enu_p, lla_p, stats_p, rc = _run(frame.params, dev["xyz_n"].shape[0], xyz_n=dev["xyz_n"])
    assert rc == 0 and torch.equal(_bits(enu_p), _bits(full["enu"])) and torch.equal(_bits(lla_p), _bits(full["lla"]))
    assert stats_p == full["stats"]
    enu, lla = full["enu"].cpu().numpy(), full["lla"].cpu().numpy()
    d = {"lat": np.abs(lla[:, 0] - fx["lat"]).max(), "lon": np.abs(lla[:, 1] - fx["lon"]).max(),
         "alt": np.abs(lla[:, 2] - fx["alt"]).max(), "east": np.abs(enu[:, 0] - fx["east_restated"]).max(),
         "north": np.abs(enu[:, 1] - fx["north_restated"]).max()}
    print("geo parity maxima:", {k: float(v) for k, v in d.items()})
    assert d["lat"] <= 1e-12 and d["lon"] <= 1e-12
    assert d["alt"] <= 1e-6 and d["east"] <= 1e-6 and d["north"] <= 1e-6
    assert np.array_equal(enu[:, 2], lla[:, 2])
    assert full["stats"][4:] == [0, 0, 0, 0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_tails_bounds_and_determinism(n, frame, dev, full):
    from snerf_amd.framework.components.coordinate_systems import GeoBounds, decode_geo_stats
    rays, depth = dev["rays"][:n].contiguous(), dev["depth"][:n].contiguous()
    enu, lla, stats, rc = _run(frame.params, n, rays, depth)
    assert rc == 0
    assert torch.equal(_bits(enu), _bits(full["enu"][:n])) and torch.equal(_bits(lla), _bits(full["lla"][:n]))
    enu2, lla2, stats2, _ = _run(frame.params, n, rays, depth)
    assert torch.equal(_bits(enu), _bits(enu2)) and torch.equal(_bits(lla), _bits(lla2)) and stats == stats2
    bounds, bad = decode_geo_stats(stats)
    assert bad == 0
    if n == 0:
        assert stats == [U64, 0, U64, 0, 0, 0, 0, 0]                       # nothing was launched
        assert bounds == GeoBounds(np.inf, -np.inf, np.inf, -np.inf)
    else:
        assert bounds == _torch_bounds(enu)
    cloud, b = frame.cloud(rays, depth)
    assert torch.equal(_bits(cloud), _bits(enu)) and b == bounds
    cloud, lla3, b = frame.cloud(rays, depth, want_lla=True)
    assert torch.equal(_bits(lla3), _bits(lla)) and tuple(cloud.shape) == (n, 3)


def test_whole_fixture_bounds_are_exact(full):
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    assert decode_geo_stats(full["stats"]) == (_torch_bounds(full["enu"]), 0)


def test_non_finite_point_is_counted_and_left_out(frame, dev, full):
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    n = 257
    rays, depth = dev["rays"][:n].contiguous(), dev["depth"][:n].clone()
    depth[128] = float("nan")
    enu, lla, stats, rc = _run(frame.params, n, rays, depth)
    assert rc == 0
    bounds, bad = decode_geo_stats(stats)
    assert bad == 1 and bool(torch.isnan(enu[128]).all()) and bool(torch.isnan(lla[128]).all())
    keep = torch.arange(n, device=DEV) != 128
    assert torch.equal(_bits(enu[keep]), _bits(full["enu"][:n][keep]))
    assert bounds == _torch_bounds(enu)
    with pytest.raises(ValueError, match="1 of 257"):
        frame.cloud(rays, depth)
    depth[5] = float("inf")
    with pytest.raises(ValueError, match="2 of 257"):
        frame.points(torch.cat([dev["xyz_n"][:255], torch.full((2, 3), float("nan"), dtype=torch.float64, device=DEV)]))
    assert decode_geo_stats(_run(frame.params, n, rays, depth)[2])[1] == 2


def test_southern_flag_adds_exactly_1e7(fx, dev, full):
    from snerf_amd.framework.components.coordinate_systems import GeoFrame, decode_geo_stats
    south = GeoFrame(_norm(fx), "17M")
    assert south.params.south == 1
    n = 513
    enu, lla, stats, rc = _run(south.params, n, dev["rays"][:n].contiguous(), dev["depth"][:n].contiguous())
    ref = full["enu"][:n]
    assert rc == 0 and torch.equal(_bits(enu[:, 0]), _bits(ref[:, 0])) and torch.equal(_bits(enu[:, 2]), _bits(ref[:, 2]))
    assert torch.equal(_bits(enu[:, 1]), _bits(ref[:, 1] + 10000000.0))
    assert torch.equal(_bits(lla), _bits(full["lla"][:n]))
    b = decode_geo_stats(stats)[0]
    assert (b.ymin, b.ymax) == (float(enu[:, 1].min()), float(enu[:, 1].max()))


def test_points_equal_cloud_and_lla_is_optional(frame, dev, full):
    from snerf_amd.eval.extract_pointcloud import get_xyz_from_nerf_prediction
    n = 1000
    rays, depth = dev["rays"][:n].contiguous(), dev["depth"][:n].contiguous()
    xyz_n = get_xyz_from_nerf_prediction(rays, depth).contiguous()
    enu_p, lla_p, stats_p, rc = _run(frame.params, n, xyz_n=xyz_n)
    assert rc == 0 and torch.equal(_bits(enu_p), _bits(full["enu"][:n])) and torch.equal(_bits(lla_p), _bits(full["lla"][:n]))
    enu_c, none, stats_c, rc = _run(frame.params, n, rays, depth, want_lla=False)
    assert rc == 0 and none is None and torch.equal(_bits(enu_c), _bits(enu_p)) and stats_c == stats_p
    enu_q, _, stats_q, rc = _run(frame.params, n, xyz_n=xyz_n, want_lla=False)
    assert rc == 0 and torch.equal(_bits(enu_q), _bits(enu_p)) and stats_q == stats_p
    # rays with more columns than eight (the reference's (h*w, 11) rays): only columns 0..5 are read
    wide = torch.cat([rays, torch.full((n, 3), float("nan"), device=DEV)], 1).contiguous()
    enu_w, _, stats_w, rc = _run(frame.params, n, wide, depth, want_lla=False)
    assert rc == 0 and torch.equal(_bits(enu_w), _bits(enu_p)) and stats_w == stats_p
    cloud, b = frame.points(xyz_n)
    assert torch.equal(_bits(cloud), _bits(enu_p))


def test_bad_arguments_come_back_as_error_codes(frame, dev):
    from snerf_amd import _lib
    L = _lib.lib()
    p = frame.params
    rays, depth = dev["rays"][:8].contiguous(), dev["depth"][:8].contiguous()
    enu = torch.zeros((8, 3), dtype=torch.float64, device=DEV)
    stats = torch.tensor([-1, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
    assert L.snerf_geo_cloud(_ptr(rays), 8, _ptr(depth), 8, C.byref(p), _ptr(enu), None, None, None) != 0
    assert L.snerf_geo_cloud(_ptr(rays), 8, _ptr(depth), -1, C.byref(p), _ptr(enu), None, _ptr(stats), None) != 0
    assert L.snerf_geo_cloud(_ptr(rays), 5, _ptr(depth), 8, C.byref(p), _ptr(enu), None, _ptr(stats), None) != 0
    assert b"ray_stride" in L.snerf_last_error()
    assert L.snerf_geo_cloud(None, 8, _ptr(depth), 8, C.byref(p), _ptr(enu), None, _ptr(stats), None) != 0
    assert L.snerf_geo_points(None, 8, C.byref(p), _ptr(enu), None, _ptr(stats), None) != 0
    assert L.snerf_geo_points(_ptr(enu), 8, None, _ptr(enu), None, _ptr(stats), None) != 0
    bad = _lib.SnerfGeoParams((C.c_double * 3)(0.0, 0.0, 0.0), 0.0, p.lon0, 0, 0)
    assert L.snerf_geo_points(_ptr(enu), 8, C.byref(bad), _ptr(enu), None, _ptr(stats), None) != 0
    assert b"range" in L.snerf_last_error()
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [-1, 0, -1, 0, 0, 0, 0, 0] and not bool(enu.any())       # nothing ran
    with pytest.raises(ValueError, match="fp32"):
        frame.cloud(rays.double(), depth)
    with pytest.raises(ValueError, match="CUDA"):
        frame.cloud(rays.cpu(), depth.cpu())


# ---- from a scene on disk to the altitude MAE ---------------------------------------------------------------------------------
def _cfgs(scene, cache_dp):
    run = types.SimpleNamespace(dataset_dp=scene, dataset_limit_train_images=False, cache_dp=cache_dp, dataset_name="scene_small_dsm")
    pipe = types.SimpleNamespace(use_utm_coordinate_system=False, semantic_dataset_type="own", sparsity_n_images=2,
                                 epoch_subsampling_activated=False, ray_subsampling_activated=False)
    return types.SimpleNamespace(run=run, pipeline=pipe)


@pytest.fixture(scope="module")
def scene(tmp_path_factory, fx):
    """scene_small plus the DSM files, assembled aside; the normalisation parameters are the fixture's (the loader uses a
    norm_params.json that exists), so the loaded GeoFrame is the one the fixture's arrays were made with"""
    from snerf_amd.baseline.dataset.satnerf_dataset import load_scene_banks
    top = tmp_path_factory.mktemp("geo_scene")
    sc = str(top / "scene")
    shutil.copytree(os.path.join(GOLDEN, "scene_small"), sc)
    shutil.copytree(os.path.join(DSM_DIR, "dsm"), os.path.join(sc, "dsm"))
    shutil.copy(os.path.join(DSM_DIR, "root.json"), os.path.join(sc, "root.json"))
    cache = top / "cache" / "scene_small_dsm" / "normalization"
    os.makedirs(cache)
    with open(cache / "norm_params.json", "w") as f:
        json.dump(dict(zip(KEYS, fx["norm_params"].tolist())), f)
    banks = load_scene_banks(_cfgs(sc, str(top / "cache")), semantic=True, depth=False, device=DEV)
    return {"banks": banks, "images": banks["rgb_test"].scene_images(), "dataset": banks["rgb_test"].dataset}


def _frame_depth(fx, n_rays):
    sizes = (fx["frame_w"] * fx["frame_h"]).tolist()
    k = sizes.index(n_rays)
    lo = sum(sizes[:k])
    return torch.from_numpy(fx["depth"][lo:lo + n_rays]).to(DEV)


def test_loaded_scene_carries_the_dsm_entry(scene, fx, frame, expected):
    images = scene["images"]
    assert [im["name"] for im in images] == ["JAX_068_013_RGB", "JAX_068_002_RGB", "JAX_068_005_RGB"]
    n = expected["roi_side"]
    for im in images:
        g = im["dsm"]
        assert sorted(g) == ["geo", "gt", "roi", "water_mask"]
        assert g["gt"].is_cuda and g["gt"].dtype == torch.float32 and tuple(g["gt"].shape) == (n, n)
        assert g["roi"].is_cuda and g["roi"].tolist() == expected["roi"]
        assert g["water_mask"].is_cuda and int((g["water_mask"] == 9).sum()) == expected["water_cells"]
        assert bytes(g["geo"].params) == bytes(frame.params)
    ds = scene["dataset"]
    assert ds.zone_string == "17R" and ds.geo is images[0]["dsm"]["geo"]


def test_end_to_end_fixture_depth_to_mae(scene, fx, dev, full, expected):
    from snerf_amd.eval.utils import dsm as D
    g = scene["images"][0]["dsm"]
    out = D.compute_dsm_and_mae(dev["rays"], dev["depth"], g["gt"], g["roi"], water_mask=g["water_mask"], geo=g["geo"],
                                distributed=False)
    print("end to end:", {k: out[k] for k in ("dx", "dy", "b", "mean", "median")}, "expected",
          {k: expected[k] for k in ("dx", "dy", "b", "mean", "median")})
    assert (out["dx"], out["dy"]) == (expected["dx"], expected["dy"]) == (2, -1)
    # the bars tests/test_gpu_dsm.py holds the registration and the MAE to against its recorded values
    assert abs(out["b"] - expected["b"]) <= 1e-9 * abs(expected["b"])
    assert abs(out["mean"] - expected["mean"]) <= 1e-6 * expected["mean"]
    assert abs(out["median"] - expected["median"]) <= 1e-6 * expected["median"]
    # the fused bounds: the same device cloud through create_dsm's own reduction gives the same DSM bit for bit
    cloud, bounds = g["geo"].cloud(dev["rays"], dev["depth"])
    assert torch.equal(_bits(cloud), _bits(full["enu"]))
    plain = D.create_dsm(cloud, roi=g["roi"])
    assert torch.equal(out["dsm"].view(torch.int32), plain.view(torch.int32))
    assert torch.equal(D.create_dsm(cloud, roi=g["roi"], bounds=bounds).view(torch.int32), plain.view(torch.int32))
    assert D.dsm_grid_from_cloud(cloud, bounds=bounds) == D.dsm_grid_from_cloud(cloud) == D.DsmGrid(*expected["bounds_grid"])
    with pytest.raises(ValueError, match="either geo or to_world"):
        D.compute_dsm_and_mae(dev["rays"], dev["depth"], g["gt"], g["roi"], geo=g["geo"], to_world=lambda p: p)


def test_dataset_world_coordinate_methods(scene, fx, dev, full):
    from snerf_amd.eval.utils import dsm as D
    ds = scene["dataset"]
    lats, lons, alts = ds.get_latlonalt_from_nerf_prediction(dev["rays"], dev["depth"])
    assert torch.equal(_bits(torch.stack([lats, lons, alts], 1)), _bits(full["lla"]))
    xyz_n = ds.get_xyz_from_nerf_prediction(dev["rays"], dev["depth"])
    assert np.array_equal(xyz_n.cpu().numpy().view(np.int64), fx["xyz_n"].view(np.int64))
    la, lo, al = ds.get_latlonalt_from_points(xyz_n)
    assert torch.equal(_bits(la), _bits(lats)) and torch.equal(_bits(lo), _bits(lons)) and torch.equal(_bits(al), _bits(alts))
    assert torch.equal(_bits(D.create_dsm_cloud_from_nerf(ds, dev["rays"], dev["depth"])), _bits(full["enu"]))
    cloud, zs = D.get_utm_cloud(lats, lons, alts)                      # the zone of the first point, torch ops
    assert zs == "17R" and float((cloud - full["enu"]).abs().max()) <= 1e-6


def test_eval_nerf_images_reports_the_mae(scene, fx, tmp_path, monkeypatch):
    from snerf_amd.eval import eval_nerf as E
    from snerf_amd.eval.utils import dsm as D
    images = scene["images"]

    def infer(cfgs, renderer, models, rays, extras, keys=None, render_options=None):
        rgbs = next(im["rgbs"] for im in images if im["rays"].data_ptr() == rays.data_ptr())
        return {"rgb_coarse": (rgbs * 0.9).contiguous(), "depth_coarse": _frame_depth(fx, rays.shape[0])}
    monkeypatch.setattr(E, "lean_inference", infer)
    d = E.eval_nerf_images(None, None, None, images, output_dp=str(tmp_path / "nerf"))
    with open(tmp_path / "nerf" / "results.json") as f:
        assert json.load(f) == d
    want = {}
    for im in images[1:]:
        g = im["dsm"]
        m = D.compute_dsm_and_mae(im["rays"], _frame_depth(fx, im["rays"].shape[0]), g["gt"], g["roi"], water_mask=g["water_mask"],
                                  geo=g["geo"], distributed=False)
        want[im["name"]] = {k: float(v) for k, v in m.items() if not torch.is_tensor(v)}
        assert np.isfinite(want[im["name"]]["mean"]) and np.isfinite(want[im["name"]]["median"])
    assert sorted(want) == ["JAX_068_002_RGB", "JAX_068_005_RGB"]
    for name, m in want.items():
        assert d[name]["mae"] == m
    assert d["MAE (Mean)"] == "{:.3f}".format(sum(m["mean"] for m in want.values()) / 2)
    assert d["MAE (Median)"] == "{:.3f}".format(sum(m["median"] for m in want.values()) / 2)


def test_extract_pointcloud_returns_the_utm_cloud(scene, fx, monkeypatch):
    from snerf_amd.eval import extract_pointcloud as X
    im = scene["images"][1]
    depth = _frame_depth(fx, im["rays"].shape[0])
    monkeypatch.setattr(X, "lean_inference", lambda *a, **k: {"rgb_coarse": im["rgbs"], "depth_coarse": depth})
    models = {"coarse": types.SimpleNamespace(spec=types.SimpleNamespace(n_classes=0))}
    geo = im["dsm"]["geo"]
    out = X.extract_pointcloud(None, None, models, im["rays"], im["extras"], geo=geo)
    assert out["xyz_utm"].dtype == torch.float64 and torch.equal(_bits(out["xyz_utm"]), _bits(geo.cloud(im["rays"], depth)[0]))
    assert "xyz_utm" not in X.extract_pointcloud(None, None, models, im["rays"], im["extras"])


def test_scene_small_is_unchanged():
    from snerf_amd.baseline.dataset.satnerf_dataset import load_scene_banks
    banks = load_scene_banks(_cfgs(os.path.join(GOLDEN, "scene_small"), None), semantic=True, depth=False, device=DEV)
    images = banks["rgb_test"].scene_images()
    assert len(images) == 3 and all("dsm" not in im for im in images)
    assert all(sorted(im) == sorted(["name", "w", "h", "rays", "rgbs", "extras", "semantic", "semantic_no_cars"]) for im in images)
    assert banks["rgb_test"].dataset.dsm is None and banks["rgb_test"].dataset.geo is not None


def test_validation_step_logs_nan_for_an_empty_overlap():
    """a DSM that misses the ROI altogether ("The predicted DSM is all NaN") ends an evaluation but not a training run's
    validation: the step logs NaN"""
    from oracle import snerf_oracle as O
    from snerf_amd.eval.utils import dsm as D
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=32, n_samples=16, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    pipe._val_render_options = lambda split: {"perturb": 0}
    bank = O.batch_to_torch(O.synthetic_batch(1024, 16, seed=12))
    batch = {"rays": bank["rays"].to(DEV), "rgbs": bank["rgbs"].to(DEV), "extras": bank["extras"].to(DEV), "split": "test",
             "semantic": bank["semantic"].to(torch.uint8).to(DEV), "semantic_sparsity_mask": bank["mask"].to(DEV)}
    meta = [5000.0, 5000.0, 16, 0.5]                                   # kilometres from the cloud (|xyz| < 3)
    gt = torch.zeros((16, 16), device=DEV)
    pipe.logged.clear()
    out = pipe.validation_step(dict(batch, dsm={"gt": gt, "roi": meta}), 0)
    assert np.isnan(pipe.logged["test/mae"]) and np.isnan(out["mae"]["mean"])
    with pytest.raises(RuntimeError, match="all NaN"):
        D.compute_dsm_and_mae(batch["rays"], out["results"]["depth_coarse"], gt, meta)
