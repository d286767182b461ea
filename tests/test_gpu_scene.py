"""Scenes on disk on the device: RPC localisation / projection (csrc/satrays.hip) against the fp64 numpy restatement, the
un-normalised rays, the normalisation parameters and the final train / test / depth banks against the banks the reference's
own loaders built from tests/golden/scene_small (tests/golden/scene_small_ref.npz, tools/gen_golden_scene.py), determinism,
the non-convergence error, and the pipeline, validation and evaluation on the loaded scene."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import rpc_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scene_small")
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "scene_small_ref.npz"))


def _root():
    with open(os.path.join(SCENE, "root.json")) as f:
        return json.load(f)


def _meta(name):
    with open(os.path.join(SCENE, "metas", name)) as f:
        return json.load(f)


def cfgs(cache_dp=None, sparsity=2):
    run = types.SimpleNamespace(dataset_dp=SCENE, dataset_limit_train_images=False, cache_dp=cache_dp, dataset_name="scene_small")
    pipe = types.SimpleNamespace(use_utm_coordinate_system=False, semantic_dataset_type="own", sparsity_n_images=sparsity,
                                 epoch_subsampling_activated=False, ray_subsampling_activated=False)
    return types.SimpleNamespace(run=run, pipeline=pipe)


def ulp_report(got, want):
    """(max distance in units of the larger value's ulp, fraction of bit-equal values)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    sp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32))
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp.astype(np.float64)
    return float(d.max()) if d.size else 0.0, float(np.mean(got.view(np.int32) == want.view(np.int32)))


def assert_rays_match(got, want):
    mx, eq = ulp_report(got, want)
    assert mx <= 1.0 and eq >= 0.999, (mx, eq)


def _all_names():
    r = _root()
    return r["train_split"] + r["test_split"]


def test_localisation_and_projection_against_numpy():
    from snerf_amd.baseline.components.camera_models import RPCModel
    for name in _all_names():
        m = _meta(name)
        ref_cam = rpc_numpy.RPCModel(m["rpc"])
        cam = RPCModel(m["rpc"], device=DEV)
        cols, rows = np.meshgrid(np.arange(m["width"], dtype=np.float64), np.arange(m["height"], dtype=np.float64))
        cols, rows = cols.ravel(), rows.ravel()
        for alt in (m["min_alt"], m["max_alt"]):
            alts = alt * np.ones(cols.size)
            lon_n, lat_n = cam.localization(cols, rows, alts, return_normalized=True)
            want_lon, want_lat = ref_cam.localization(cols, rows, alts, return_normalized=True)
            assert np.abs(lon_n.cpu().numpy() - want_lon).max() <= 1e-12, name
            assert np.abs(lat_n.cpu().numpy() - want_lat).max() <= 1e-12, name
            lon, lat = cam.localization(cols, rows, alts)
            c, r = cam.projection(lon, lat, alts)
            assert np.abs(c.cpu().numpy() - cols).max() <= 1e-6 and np.abs(r.cpu().numpy() - rows).max() <= 1e-6, name
    assert "lat_num" in _meta("JAX_068_009_RGB.json")["rpc"] and "lat_num" not in _meta("JAX_068_013_RGB.json")["rpc"]


def _raw_rays(names):
    from snerf_amd.baseline.components.camera_models import construct_rpc_camera_model
    from snerf_amd.baseline.components.rays import satnerf_construct
    metas = [_meta(n) for n in names]
    return satnerf_construct([construct_rpc_camera_model(m, DEV) for m in metas], [m["min_alt"] for m in metas],
                             [m["max_alt"] for m in metas], sizes=[(m["width"], m["height"]) for m in metas], names=names,
                             device=DEV)


def test_unnormalised_rays_match_the_reference(ref):
    r = _root()
    assert_rays_match(_raw_rays(r["train_split"]).cpu().numpy(), ref["raw_train_rays"])
    assert_rays_match(_raw_rays(r["train_split"][:1] + r["test_split"]).cpu().numpy(), ref["raw_test_rays"])


def test_normalisation_parameters(ref):
    from snerf_amd.baseline.components.normalization import ray_bounds
    r = _root()
    tr, te = _raw_rays(r["train_split"]), _raw_rays(r["train_split"][:1] + r["test_split"])
    b = ray_bounds([tr, te]).cpu().numpy()
    rays = torch.cat([tr, te]).cpu()
    far = rays[:, :3] + rays[:, 7:8] * rays[:, 3:6]          # torch CPU: one rounding per operation, as the reference
    pts = torch.cat([rays[:, :3], far]).numpy()
    mn, mx = pts.min(0), pts.max(0)
    np.testing.assert_array_equal(b[0:3], mn)
    np.testing.assert_array_equal(b[3:6], mx)
    scale = (mx - mn) / np.float32(2)
    np.testing.assert_array_equal(b[6:9], scale)
    np.testing.assert_array_equal(b[9:12], mn + scale)
    assert b[12] == scale.max()
    # against the reference: equal, or 1 ulp off only where the extremal point of the reference's rays is a row that (b)
    # found rounded the other way (a tie)
    p = ref["norm_params"]
    want = np.array([p[0], p[2], p[4], p[1], p[3], p[5]], np.float32)
    got = np.concatenate([b[6:9], b[9:12]])
    golden = np.concatenate([ref["raw_train_rays"], ref["raw_test_rays"]])
    gpts = np.concatenate([golden[:, :3], (torch.from_numpy(golden[:, :3]) + torch.from_numpy(golden[:, 7:8])
                                           * torch.from_numpy(golden[:, 3:6])).numpy()])
    kpts = pts
    for k in range(3):
        if got[k] == want[k] and got[3 + k] == want[3 + k]:
            continue
        mxu, _ = ulp_report(got[[k, 3 + k]], want[[k, 3 + k]])
        assert mxu <= 1.0, (k, got, want)
        rows = {int(np.argmin(gpts[:, k])), int(np.argmax(gpts[:, k])), int(np.argmin(kpts[:, k])), int(np.argmax(kpts[:, k]))}
        rows = {r % golden.shape[0] for r in rows}
        assert any(not np.array_equal(rays.numpy()[r], golden[r]) for r in rows), f"axis {k}: parameters differ without a tie"


def _banks(tmp_path=None, depth=True, sparsity=2):
    from snerf_amd.baseline.dataset.satnerf_dataset import load_scene_banks
    return load_scene_banks(cfgs(str(tmp_path) if tmp_path is not None else None, sparsity), semantic=True, depth=depth,
                            device=DEV)


def test_banks_match_the_reference(ref, tmp_path):
    b = _banks(tmp_path)
    tr, te, dp = b["rgb"].t, b["rgb_test"].t, b["depth"].t
    assert set(tr) == {"rays", "rgbs", "extras", "semantic", "semantic_sparsity_mask"}
    assert_rays_match(tr["rays"].cpu().numpy(), ref["train_rays"])
    assert_rays_match(te["rays"].cpu().numpy(), ref["test_rays"])
    for key in ("rgbs", "extras", "semantic", "semantic_sparsity_mask"):
        np.testing.assert_array_equal(tr[key].cpu().numpy(), ref[f"train_{key}"], err_msg=key)
    for key in ("rgbs", "extras", "semantic", "semantic_no_cars"):
        np.testing.assert_array_equal(te[key].cpu().numpy(), ref[f"test_{key}"], err_msg=key)
    assert b["rgb_test"].image_sizes == list(ref["test_image_sizes"])
    assert b["rgb"].semantic_n_classes == 5 and b["rgb"].car_cls_idx == 4
    # depth set: the keypoint rays normalised with the shared parameters, depths |pts - o| in fp32, weights exp(-(e/mean e)^2)
    assert_rays_match(dp["rays"].cpu().numpy(), ref["depth_rays"])
    np.testing.assert_array_equal(dp["extras"].cpu().numpy(), ref["depth_extras"])
    # depths: bit-equal on every row whose normalised ray origin is bit-equal (a tie in the ray moves the depth with it)
    same_o = np.all(dp["rays"].cpu().numpy()[:, :3] == ref["depth_rays"][:, :3], axis=1)
    assert same_o.mean() >= 0.95, same_o.mean()
    np.testing.assert_array_equal(dp["depths"].cpu().numpy()[same_o], ref["depth_depths"][same_o])
    mx, eq = ulp_report(dp["weights"].cpu().numpy(), ref["depth_weights"])
    assert mx <= 1.0 and eq >= 0.999, ("weights", mx, eq)
    # the parameters were written in the reference's format, and a second load uses the file
    fp = os.path.join(str(tmp_path), "scene_small", "normalization", "norm_params.json")
    with open(fp) as f:
        written = json.load(f)
    assert sorted(written) == sorted(["X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset"])
    mxp, _ = ulp_report(np.array([written[k] for k in ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")]),
                        ref["norm_params"])
    assert mxp <= 1.0
    shifted = dict(written, X_offset=written["X_offset"] + 64.0)
    with open(fp, "w") as f:
        json.dump(shifted, f)
    b2 = _banks(tmp_path, depth=False)
    assert torch.equal(b2["rgb"].t["rays"][:, 1:], tr["rays"][:, 1:])
    assert not torch.equal(b2["rgb"].t["rays"][:, 0], tr["rays"][:, 0])


def test_two_loads_are_bit_identical():
    a, b = _banks(depth=True), _banks(depth=True)
    for name in ("rgb", "rgb_test", "depth"):
        for key, v in a[name].t.items():
            assert torch.equal(v, b[name].t[key]), (name, key)


def test_non_convergent_rpc_raises_and_the_process_stays_usable():
    from snerf_amd.baseline.components.camera_models import RPCModel
    from snerf_amd.baseline.components.rays import LocalizationError, satnerf_construct
    good = _meta("JAX_068_013_RGB.json")
    bad = json.loads(json.dumps(good["rpc"]))
    bad["col_den"] = [0.0] * 20            # every projection is inf / NaN: the inversion can never meet its tolerance
    cams = [RPCModel(good["rpc"], device=DEV), RPCModel(bad, device=DEV)]
    with pytest.raises(LocalizationError, match="JAX_068_BAD"):
        satnerf_construct(cams, [-20.0, -20.0], [40.0, 40.0], sizes=[(5, 3), (7, 2)], names=["JAX_068_013", "JAX_068_BAD"],
                          device=DEV)
    with pytest.raises(RuntimeError, match="did not converge"):
        cams[1].localization(np.array([1.0, 2.0]), np.array([1.0, 2.0]), np.array([0.0, 0.0]))
    rays = satnerf_construct(cams[:1], [-20.0], [40.0], sizes=[(5, 3)], device=DEV)
    torch.cuda.synchronize()
    assert torch.isfinite(rays).all()


def _pipeline_cfgs(depth, tmp_path):
    from snerf_amd.framework.configs import MainConfig
    return MainConfig(run={"max_train_steps": 6, "dataset_dp": SCENE, "cache_dp": str(tmp_path), "dataset_name": "scene_small"},
                      pipeline={"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64,
                                "n_samples": 32, "batch_size": 128, "depth_enabled": depth, "first_beta_epoch": 0,
                                "sparsity_n_images": 2, "render_chunk_size": 1 << 20})


@pytest.mark.parametrize("depth", [True, False])
def test_semantic_pipeline_trains_and_validates_on_the_scene(depth, tmp_path):
    from snerf_amd.framework.pipelines import TrainLoop, load_pipeline
    torch.manual_seed(0)
    c = _pipeline_cfgs(depth, tmp_path)
    pipe = load_pipeline(c)
    assert ("depth" in pipe.datasets) == depth
    assert pipe.datasets["rgb_test"].image_sizes == [41 * 37, 31 * 23, 25 * 39]
    loop = TrainLoop(pipe, c, DEV)
    for step in range(4):
        out = loop.step(step)
        assert torch.isfinite(out["loss"]).item(), step
    res = loop.validate()
    assert np.isfinite(res["test/psnr"]) and np.isfinite(res["test/loss"])
    assert 0.0 <= res["test/semantic_accuracy"] <= 1.0
    assert "test/ssim" in res                               # every image's shape is known: SSIM over the real frames
    assert res["test/confusion_matrix"].shape == (5, 5)


def test_satnerf_pipeline_uses_no_semantic_columns(tmp_path):
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import TrainLoop, load_pipeline
    c = MainConfig(run={"max_train_steps": 4, "dataset_dp": SCENE}, pipeline={
        "pipeline": "snerf_amd.baseline.pipelines.satnerf.SatNeRFPipeline", "fc_units": 64, "n_samples": 32, "batch_size": 128,
        "depth_enabled": False, "first_beta_epoch": 0, "render_chunk_size": 1 << 20})
    pipe = load_pipeline(c)
    assert set(pipe.datasets["rgb"].t) == {"rays", "rgbs", "extras"}
    assert "semantic" not in pipe.datasets["rgb_test"].t
    loop = TrainLoop(pipe, c, DEV)
    for step in range(2):
        assert torch.isfinite(loop.step(step)["loss"]).item()
    res = loop.validate()
    assert np.isfinite(res["test/psnr"])


def test_evaluation_takes_the_loaders_image_dicts(tmp_path):
    from snerf_amd.eval.eval_nerf import eval_nerf_images
    from snerf_amd.eval.eval_semantic import eval_semantic_images
    from snerf_amd.framework.pipelines import load_pipeline
    c = _pipeline_cfgs(False, tmp_path)
    pipe = load_pipeline(c).to(DEV)
    bank = pipe.datasets["rgb_test"]
    images = bank.scene_images()
    assert [im["name"] for im in images] == ["JAX_068_013_RGB", "JAX_068_002_RGB", "JAX_068_005_RGB"]
    assert all(im["rays"].shape[0] == im["w"] * im["h"] for im in images)
    d = eval_nerf_images(c, pipe.renderer, pipe.models, images, output_dp=str(tmp_path / "nerf"))
    assert set(k for k in d if k.startswith("JAX")) == {"JAX_068_002_RGB", "JAX_068_005_RGB"}
    assert os.path.exists(tmp_path / "nerf" / "results.json")
    s = eval_semantic_images(c, pipe.renderer, pipe.models, images, bank.semantic_n_classes, bank.car_cls_idx,
                             output_dp=str(tmp_path / "sem"))
    assert os.path.exists(tmp_path / "sem" / "results.json")
    assert "JAX_068_002_RGB" in s
