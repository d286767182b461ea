"""SSIM on the GPU (csrc/ssim.hip through snerf_amd.eval.utils.metrics): ssim_inria against the reference-made fixtures, the
kornia form's maps against the fp64 restatement element for element (borders included) in both border modes, bit
reproducibility and batch independence, the refusals, the validation step and TrainLoop.validate, two data-parallel ranks,
and the per-image evaluation eval_nerf_images."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ssim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INRIA = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("ssim_inria_"))
DEV = "cuda:0"
MEAN_TOL = 2e-7
C1, C2, EPS = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2, 1e-12


def _M():
    from snerf_amd.eval.utils import metrics
    return metrics


def _images(shape, seed):
    """a textured image pair in [0, 1], fp32 (B, C, H, W), on the CPU"""
    g = torch.Generator().manual_seed(seed)
    b, c, h, w = shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(xx / 5.0 + torch.rand(b, c, 1, 1, generator=g, dtype=torch.float64) * 6) * torch.cos(yy / 7.0)
    x = (base + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    y = (0.85 * x + 0.1 + 0.07 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    if h >= 8 and w >= 8:        # a black patch in both: den = C1 C2 there, where eps = 1e-12 moves the value by 1.1e-5
        x[..., :h // 4, :w // 4] = 0.0
        y[..., :h // 4, :w // 4] = 0.0
    return x.float(), y.float()


# ---- ssim_inria against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ws", (3, 7, 11))
@pytest.mark.parametrize("name", INRIA)
def test_ssim_inria_vs_reference_fixtures(name, ws):
    M = _M()
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    f64, f32 = z[f"f64_ws{ws}"], z[f"f32_ws{ws}"].astype(np.float64)
    gap = np.abs(f32 - f64)
    got = M.ssim_inria(x, y, ws, bool(z["size_average"]))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == f64.shape
    got = got.cpu().numpy().astype(np.float64)
    assert np.abs(got - f64).max() <= MEAN_TOL
    assert np.all(np.abs(got - f32) <= gap + MEAN_TOL)
    if not bool(z["size_average"]):                      # the batch's mean: all images have the same size
        mean = float(M.ssim_inria(x, y, ws))
        assert abs(mean - float(f64.mean())) <= MEAN_TOL


# ---- the kernel against the restatement, map element for element --------------------------------------------------------
SHAPES = [(1, 3, 64, 64), (1, 3, 37, 53), (2, 3, 1031, 17), (1, 1, 2, 2), (1, 3, 1024, 1024)]


@pytest.mark.parametrize("border", ("reflect", "zero"))
@pytest.mark.parametrize("ws", (3, 5, 11))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_vs_restatement(shape, ws, border):
    M = _M()
    x, y = _images(shape, seed=ws + 7 * shape[-1])
    k = M.kornia_window(ws)
    if border == "reflect" and ws // 2 >= min(shape[-2:]):
        with pytest.raises(ValueError, match="reflect"):
            M.ssim_sums(x.to(DEV), y.to(DEV), k, border, C1, C2, EPS)
        return
    sums, smap = M.ssim_sums(x.to(DEV), y.to(DEV), k, border, C1, C2, EPS, return_map=True)
    want = R.ssim_map(x, y, k, border, C1, C2, EPS)
    got = smap.cpu().double()
    # the kernel rounds its fp64 value to fp32 once: within one fp32 ulp of the fp64 restatement, border pixels included
    ulp = torch.from_numpy(np.spacing(np.abs(want.float().numpy()))).double()
    err = (got - want).abs()
    assert bool((err <= ulp + 1e-11).all()), (float(err.max()), [int(i) for i in np.unravel_index(int(err.argmax()), err.shape)])
    per_image = want.sum(dim=(1, 2, 3))
    assert torch.allclose(sums.cpu(), per_image, rtol=1e-12, atol=1e-9)
    if border == "reflect" and ws == 3 and shape[0] == 1:   # the module's kornia form is exactly this case
        assert abs(float(M.ssim(x.to(DEV), y.to(DEV))) - float(want.mean())) <= MEAN_TOL


def test_kornia_form_of_the_reference_call():
    """metrics.ssim on what the reference's ssim hands to kornia (an (H*W, 3) frame through .view(1, 3, H, W)) equals the
    restated kornia map's mean"""
    M = _M()
    z = np.load(os.path.join(GOLDEN, "ssim_kornia_call.npz"))
    h, w = int(z["H"]), int(z["W"])
    p, g = torch.from_numpy(z["frame_pred"]), torch.from_numpy(z["frame_gt"])
    got = M.ssim(p.to(DEV).view(1, 3, h, w), g.to(DEV).view(1, 3, h, w))
    assert got.dim() == 0 and got.dtype == torch.float32
    want = R.kornia_map(torch.from_numpy(z["image_pred"]), torch.from_numpy(z["image_gt"]), int(z["window_size"])).mean()
    assert abs(float(got) - float(want)) <= MEAN_TOL


# ---- reproducibility and batch independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("border,ws", (("reflect", 3), ("zero", 11)))
def test_bit_reproducible_and_batch_independent(border, ws):
    M = _M()
    x, y = _images((3, 3, 300, 277), seed=5)
    x, y = x.to(DEV), y.to(DEV)
    k = M.kornia_window(ws)
    s1, m1 = M.ssim_sums(x, y, k, border, C1, C2, EPS, return_map=True)
    s2, m2 = M.ssim_sums(x, y, k, border, C1, C2, EPS, return_map=True)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    assert torch.equal(m1.view(torch.int32), m2.view(torch.int32))
    for i in range(3):
        si, mi = M.ssim_sums(x[i:i + 1], y[i:i + 1], k, border, C1, C2, EPS, return_map=True)
        assert torch.equal(si.view(torch.int64), s1[i:i + 1].view(torch.int64)), i
        assert torch.equal(mi.view(torch.int32), m1[i:i + 1].view(torch.int32)), i
    per = M.ssim_inria(x, y, ws, size_average=False)
    for i in range(3):
        assert torch.equal(M.ssim_inria(x[i:i + 1], y[i:i + 1], ws).view(torch.int32), per[i].view(torch.int32)), i


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    M = _M()
    x, y = _images((1, 3, 16, 16), seed=1)
    with pytest.raises(ValueError, match="CUDA"):
        M.ssim(x, y)
    with pytest.raises(ValueError, match="CUDA"):
        M.ssim_inria(x.to(DEV), y)
    with pytest.raises(TypeError, match="float32"):
        M.ssim(x.double().to(DEV), y.double().to(DEV))
    with pytest.raises(TypeError, match="float32"):
        M.ssim_inria(x.double().to(DEV), y.double().to(DEV))
    with pytest.raises(ValueError, match="differ"):
        M.ssim(x.to(DEV), y[:, :, :8].to(DEV))
    with pytest.raises(ValueError, match="odd"):
        M.ssim_inria(x.to(DEV), y.to(DEV), 4)
    with pytest.raises(ValueError, match="reflect"):
        M.ssim(x[:, :, :1].to(DEV), y[:, :, :1].to(DEV))


# ---- validation_step and TrainLoop.validate ------------------------------------------------------------------------------
def _val_setup():
    from oracle import snerf_oracle as O
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=32, n_samples=16, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    pipe._val_render_options = lambda split: {"perturb": 0}      # no jitter: a render is a function of its rays
    return O, pipe


def _batch(O, n, seed, split="test"):
    bank = O.batch_to_torch(O.synthetic_batch(n, 16, seed=seed))
    return {"rays": bank["rays"].to(DEV), "rgbs": bank["rgbs"].to(DEV), "extras": bank["extras"].to(DEV), "split": split,
            "semantic": bank["semantic"].to(torch.uint8).to(DEV), "semantic_sparsity_mask": bank["mask"].to(DEV)}


def _restated(out, batch, h, w):
    rgb = out["results"]["rgb_coarse"].cpu()
    return float(R.kornia_map(R.frame_view(rgb, h, w), R.frame_view(batch["rgbs"].cpu(), h, w)).mean())


def test_validation_step_logs_ssim_for_every_split():
    O, pipe = _val_setup()
    for split in ("test", "train"):
        batch = _batch(O, 4096, 21, split)
        pipe.logged.clear()
        out = pipe.validation_step(batch, 0)
        key = f"{split}/ssim"
        assert key in pipe.logged and out["ssim"].dim() == 0 and out["ssim"].is_cuda
        assert abs(float(pipe.logged[key]) - _restated(out, batch, 64, 64)) <= MEAN_TOL
        assert torch.equal(out["ssim"], pipe.logged[key])
    # 4000 rays, no w / h: the shape is unknown and the key absent; with w = 50, h = 80 it is present
    batch = _batch(O, 4000, 22)
    pipe.logged.clear()
    out = pipe.validation_step(batch, 0)
    assert "ssim" not in out and "test/ssim" not in pipe.logged and "test/psnr" in pipe.logged
    pipe.logged.clear()
    out = pipe.validation_step(dict(batch, w=50, h=80), 0)
    assert abs(float(pipe.logged["test/ssim"]) - _restated(out, batch, 80, 50)) <= MEAN_TOL
    out2 = pipe.validation_step(dict(batch, w=[50], h=[80]), 0)           # the collated list form
    assert torch.equal(out2["ssim"], out["ssim"])
    with pytest.raises(ValueError, match="not 40 x 80"):
        pipe.validation_step(dict(batch, w=40, h=80), 0)


def test_validate_returns_the_mean_over_images():
    from snerf_amd.framework.datasets import GpuRayBank
    from snerf_amd.framework.pipelines import TrainLoop
    O, pipe = _val_setup()
    HW = 64 * 64
    b = O.batch_to_torch(O.synthetic_batch(3 * HW, 16, seed=33))
    pipe.datasets["rgb_test"] = GpuRayBank({"rays": b["rays"], "extras": b["extras"], "rgbs": b["rgbs"],
                                            "semantic": b["semantic"].to(torch.uint8),
                                            "semantic_sparsity_mask": b["mask"]}, device=DEV)
    per = [float(pipe.validation_step(dict(pipe.datasets["rgb_test"].image(i, HW), split="test"), i)["ssim"]) for i in range(3)]
    loop = TrainLoop(pipe, pipe.cfgs, torch.device(DEV))
    val = loop.validate(rays_per_image=HW)
    assert abs(val["test/ssim"] - sum(per) / 3) <= 2e-7
    assert len(set(per)) == 3
    # images whose shape cannot be known (3000 rays, not a square) give no test/ssim
    val = loop.validate(rays_per_image=3000, max_images=2)
    assert "test/ssim" not in val and "test/psnr" in val


_DDP_SSIM_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from snerf_amd import parallel
rank, world, dev = parallel.init_distributed(backend="gloo")
from tests.test_gpu_ssim import _val_setup, _batch
O, pipe = _val_setup()
vals = []
for n, seed, wh in ((4096, 41, None), (4000, 42, (50, 80))):
    batch = _batch(O, n, seed)
    lo, hi = parallel.frame_shard(n)
    part = {{k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in batch.items()}}
    if wh is not None:
        part["w"], part["h"] = wh
    out = pipe.validation_step(part, 0)
    vals.append(out["ssim"].cpu().view(torch.int32).item())
np.save({out!r} + f".{{rank}}.npy", np.array(vals, np.int64))
dist.barrier()
"""


def test_data_parallel_ssim_equals_single_process(tmp_path):
    """2 ranks (gloo, both on this GPU), each with its frame_shard slice of the image: validation_step's SSIM (global ray
    count from an all-reduce, then from w * h; rows all-gathered) equals the single-process value bit for bit"""
    O, pipe = _val_setup()
    single = []
    for n, seed, wh in ((4096, 41, None), (4000, 42, (50, 80))):
        batch = _batch(O, n, seed)
        if wh is not None:
            batch["w"], batch["h"] = wh
        single.append(pipe.validation_step(batch, 0)["ssim"].cpu().view(torch.int32).item())
    script = tmp_path / "worker.py"
    out = str(tmp_path / "ssim")
    script.write_text(_DDP_SSIM_WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29641", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0"), cwd=ROOT)
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    for r in range(2):
        assert np.load(out + f".{r}.npy").tolist() == single, r


# ---- eval_nerf_images ----------------------------------------------------------------------------------------------------
def _dsm_entry(pipe, batch, seed):
    """a ground-truth DSM for the image's own rendered depth (the set-up of test_gpu_dsm's validation-step test)"""
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.eval.utils.util import lean_inference
    res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, batch["rays"], batch["extras"], keys=("depth_coarse",))
    xyz = batch["rays"][:, :3].double() + batch["rays"][:, 3:6].double() * res["depth_coarse"].double()[:, None]
    ext = float((xyz[:, :2].max(0).values - xyz[:, :2].min(0).values).max())
    scale = 30.0 / ext
    to_world = lambda p: p * scale                                # noqa: E731
    bounds = D.dsm_grid_from_cloud(to_world(xyz))
    n = min(bounds.xsize, bounds.ysize) - 4
    meta = [bounds.xoff + 2 * 0.5, bounds.yoff - 2 * 0.5 - n * 0.5, n, 0.5]
    gt = D.create_dsm(to_world(xyz), roi=meta) + 0.25 * (seed % 3 + 1)
    gt = torch.where(torch.isnan(gt), torch.zeros_like(gt), gt)
    return {"gt": gt, "roi": meta, "to_world": to_world}


def test_eval_nerf_images(tmp_path):
    from snerf_amd.eval.eval_nerf import eval_nerf_images
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.eval.utils.util import lean_inference
    M = _M()
    O, pipe = _val_setup()
    images = []
    for i, (n, wh) in enumerate(((4096, None), (4096, None), (3000, (60, 50)))):
        b = _batch(O, n, 50 + i)
        img = {"name": f"img_{i}", "rays": b["rays"], "extras": b["extras"], "rgbs": b["rgbs"]}
        if wh is not None:
            img["w"], img["h"] = wh
        img["dsm"] = _dsm_entry(pipe, img, i)
        images.append(img)
    # eval_nerf_images renders with the renderer's default jitter (the reference perturbs in evaluation too): the direct
    # renders below draw the same jitter from the same seed, image by image in the same order
    torch.manual_seed(11)
    out = eval_nerf_images(pipe.cfgs, pipe.renderer, pipe.models, images, output_dp=str(tmp_path))
    torch.manual_seed(11)
    with open(tmp_path / "results.json") as f:
        assert json.load(f) == out
    assert sorted(out) == ["MAE (Mean)", "MAE (Median)", "PSNR (Mean)", "SSIM (Mean)", "img_1", "img_2"]   # img_0 skipped
    maes, psnrs, ssims = [], [], []
    for img in images[1:]:
        e = out[img["name"]]
        assert sorted(e) == ["mae", "psnr", "ssim"]
        assert re.fullmatch(r"-?\d+\.\d\d", e["psnr"]) and re.fullmatch(r"-?\d\.\d\d\d", e["ssim"])
        res = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, img["rays"], img["extras"], keys=("rgb_coarse", "depth_coarse"))
        W, H = img.get("w", 64), img.get("h", 64)
        assert e["psnr"] == "{:.2f}".format(float(M.psnr(res["rgb_coarse"], img["rgbs"])))
        s = float(M.ssim(res["rgb_coarse"].view(1, 3, H, W), img["rgbs"].view(1, 3, H, W)))
        assert e["ssim"] == "{:.3f}".format(s)
        d = img["dsm"]
        mae = D.compute_dsm_and_mae(img["rays"], res["depth_coarse"], d["gt"], d["roi"], to_world=d["to_world"])
        assert all(type(v) is float for v in e["mae"].values())
        assert e["mae"]["mean"] == mae["mean"] and e["mae"]["median"] == mae["median"]
        assert (e["mae"]["dx"], e["mae"]["dy"]) == (mae["dx"], mae["dy"]) and np.isfinite(mae["mean"])
        maes.append(mae)
        psnrs.append(float(e["psnr"]))
        ssims.append(float(e["ssim"]))
    assert out["MAE (Mean)"] == "{:.3f}".format(sum(m["mean"] for m in maes) / 2)
    assert out["MAE (Median)"] == "{:.3f}".format(sum(m["median"] for m in maes) / 2)
    assert out["PSNR (Mean)"] == "{:.2f}".format(sum(psnrs) / 2)
    assert out["SSIM (Mean)"] == "{:.3f}".format(sum(ssims) / 2)
    # the train split keeps item 0; without "dsm" entries the MAE keys are absent; a mixed split is refused
    plain = [{k: v for k, v in img.items() if k != "dsm"} for img in images]
    tr = eval_nerf_images(pipe.cfgs, pipe.renderer, pipe.models, plain, split="train")
    assert sorted(tr) == ["PSNR (Mean)", "SSIM (Mean)", "img_0", "img_1", "img_2"]
    assert all(sorted(tr[f"img_{i}"]) == ["psnr", "ssim"] for i in range(3))
    with pytest.raises(ValueError, match="dsm"):
        eval_nerf_images(pipe.cfgs, pipe.renderer, pipe.models, [images[0], images[1], plain[2]])
