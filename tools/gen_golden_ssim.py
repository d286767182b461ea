#!/usr/bin/env python3
"""Generate the golden vectors of SSIM and PSNR by running the REFERENCE's own eval/utils/metrics.py.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ssim.py

It loads eval/utils/metrics.py of the reference (read-only) with a stub `kornia` module: kornia is not installed, and the
stub's `kornia.losses.ssim` only records what it is handed (the reference's `ssim` is a one-line call of it).  `ssim_inria`,
`create_window`, `gaussian` and `psnr` are pure torch and run as written, `ssim_inria` once on fp32 images and once on the
same images as fp64 (the window is built in fp32 and cast by `type_as`).  Writes tests/golden/:
- ssim_inria_<case>.npz: x, y (fp32, (B, C, H, W)), size_average, and per window size ws in (3, 7, 11) the reference's values
  f32_ws<ws> and f64_ws<ws> (0-d, or (B,) with size_average=False);
- ssim_kornia_call.npz: an (H*W, 3) frame pair, H, W, and the (image_pred, image_gt, window_size) the reference's `ssim` hands
  to kornia when called as its validation_step / eval_nerf call it (`.view(1, 3, H, W)` / `.reshape(1, 3, H, W)`);
- ssim_misc.npz: create_window(ws, 3) for ws in (3, 7, 11), and one PSNR pair with the reference's value.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
WINDOWS = (3, 7, 11)
sys.dont_write_bytecode = True

CALLS = []


def load_metrics():
    kornia = types.ModuleType("kornia")
    losses = types.ModuleType("kornia.losses")

    def record(img1, img2, window_size, *args, **kwargs):
        CALLS.append((img1.detach().clone(), img2.detach().clone(), window_size, args, kwargs))
        return torch.zeros((), dtype=img1.dtype)

    losses.ssim = record
    kornia.losses = losses
    sys.modules["kornia"], sys.modules["kornia.losses"] = kornia, losses
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(REF, "eval", "utils", "metrics.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = load_metrics()


def image_pair(rng, b, h, w, c=3):
    """a textured image in [0, 1] and a noisy, slightly blurred, shifted-brightness prediction of it (fp32)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gt = np.empty((b, c, h, w))
    for i in range(b):
        for k in range(c):
            f = 0.5 + 0.25 * np.sin(xx / rng.uniform(2.0, 6.0) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(2.0, 6.0))
            gt[i, k] = f + 0.15 * rng.standard_normal((h, w))
    gt = np.clip(gt, 0.0, 1.0)
    pred = 0.8 * gt + 0.2 * np.roll(gt, 1, axis=-1) + 0.03 + 0.08 * rng.standard_normal(gt.shape)
    return np.clip(pred, 0.0, 1.0).astype(np.float32), gt.astype(np.float32)


def inria_case(x, y, size_average=True):
    res = {"x": x, "y": y, "size_average": np.bool_(size_average)}
    for ws in WINDOWS:
        t1, t2 = torch.from_numpy(x), torch.from_numpy(y)
        res[f"f32_ws{ws}"] = M.ssim_inria(t1, t2, ws, size_average).numpy()
        res[f"f64_ws{ws}"] = M.ssim_inria(t1.double(), t2.double(), ws, size_average).numpy()
    return res


def cases():
    rng = np.random.default_rng(20261016)
    out = {}
    out["ssim_inria_64"] = inria_case(*image_pair(rng, 1, 64, 64))
    out["ssim_inria_37x53"] = inria_case(*image_pair(rng, 1, 37, 53))
    out["ssim_inria_11"] = inria_case(*image_pair(rng, 1, 11, 11))
    out["ssim_inria_5x200"] = inria_case(*image_pair(rng, 1, 5, 200))           # narrower than every window but ws = 3
    out["ssim_inria_const"] = inria_case(np.full((1, 3, 16, 16), 0.625, np.float32), np.full((1, 3, 16, 16), 0.25, np.float32))
    out["ssim_inria_batch2"] = inria_case(*image_pair(rng, 2, 24, 31), size_average=False)
    # the reference's ssim on an (H*W, 3) frame, called as validation_step (:143-145) and eval_nerf (:87-89) call it
    H, W = 12, 20
    pred = rng.uniform(0.0, 1.0, (H * W, 3)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (H * W, 3)).astype(np.float32)
    CALLS.clear()
    M.ssim(torch.from_numpy(pred).view(1, 3, H, W), torch.from_numpy(gt).reshape(1, 3, H, W))
    (a, b, ws, args, kwargs), = CALLS
    assert not args and not kwargs
    out["ssim_kornia_call"] = {"frame_pred": pred, "frame_gt": gt, "H": np.int64(H), "W": np.int64(W),
                               "image_pred": a.numpy(), "image_gt": b.numpy(), "window_size": np.int64(ws)}
    misc = {f"window_{ws}": M.create_window(ws, 3).numpy() for ws in WINDOWS}
    p1, p2 = image_pair(rng, 1, 32, 32)
    misc.update(psnr_pred=p1, psnr_gt=p2, psnr=M.psnr(torch.from_numpy(p1), torch.from_numpy(p2)).numpy())
    out["ssim_misc"] = misc
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, res in cases().items():
        np.savez(os.path.join(OUT, name + ".npz"), **res)
        vals = {k: np.round(v, 7).tolist() for k, v in res.items() if k.startswith("f")  and k[1:3] in ("32", "64")}
        print(name, vals if vals else sorted(res))


if __name__ == "__main__":
    main()
