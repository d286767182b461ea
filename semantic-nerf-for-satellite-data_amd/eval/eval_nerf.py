"""Per-image evaluation of a trained model -- the loop of the reference's eval/eval_nerf.py:15-119 (eval_nerf_training)
without checkpoint and dataset loading: the caller hands in the configs, the renderer, the models and the split's images.

For every image: render rgb and depth (lean_inference; with sharded=True, sharded_lean_inference over the process group,
which gives every rank the whole frame), the DSM altitude MAE when the image carries a "dsm" entry (eval/utils/dsm.py; with
the entry's "geo", as the scene loader writes it, the cloud is the UTM one of the fused world-cloud launch), PSNR,
and SSIM through the reference's `.view(1, 3, H, W)` of the (H*W, 3) frames (eval/utils/metrics.py).  After each image the
per-image entries and the means are written to `output_dp`/results.json with the reference's keys and formats.

DIVERGENCES: the per-image "mae" entry holds the MAE dict's numbers as floats (the DSM and the registered DSM are dropped);
its means are taken over those floats.  PSNR and SSIM means are, as in the reference, the means of the formatted strings.
No GeoTIFF is written (`epoch` named the reference's DSM files and is accepted for its signature only).  If no image has a
"dsm" entry the MAE keys are absent; a split that mixes images with and without one is refused.

ADDITION: `fit_embedding` (NeRF-W's protocol for a view without a row in the embedding table; eval/utils/embedding.py): per image
the transient vector is fitted on a region of its pixels with the network frozen, the WHOLE frame is rendered with it and every
key above comes from that render; the entry gains "psnr_heldout" (the region's complement) and "t_fit", and the vectors are
written to `output_dp`/t_fit.json.  None (the default) changes nothing."""
import json
import math
import os

import torch

from .utils import metrics
from .utils.util import lean_inference, sharded_lean_inference, with_depth_mode
from ..baseline.pipelines.base_ray_pipeline import frame_w_h
from ..parallel import world


def _w_h(img, n):
    """w_h_from_sample (framework/util/other.py:55-65) for a whole frame of n rays; refuses a shape the view cannot take"""
    wh = frame_w_h(img)
    if wh is None:
        side = math.isqrt(n)
        wh = (side, side)
    if wh[0] * wh[1] != n:
        raise ValueError(f"image {img.get('name')!r}: {n} rays are not a {wh[0]} x {wh[1]} frame (pass 'w' and 'h')")
    return wh


def _mae_floats(mae):
    return {k: float(v) for k, v in mae.items() if not torch.is_tensor(v)}


@torch.no_grad()
def eval_nerf_images(cfgs, renderer, models, images, output_dp=None, split="test", epoch=-1, sharded=False, fit_embedding=None,
                     depth_mode="mean"):
    """images: a sequence of dicts with the reference's item keys ("name", "rays", "extras", "rgbs", optional "w", "h") and
    the optional "dsm" entry of validation_step.  On the test split item 0 is skipped (it is also a training view,
    eval_nerf.py:52-55).  Returns the dict written to results.json: {name: {["mae": {...},] "psnr": "{:.2f}",
    "ssim": "{:.3f}"}, ["MAE (Mean)", "MAE (Median)",] "PSNR (Mean)", "SSIM (Mean)"}.  With sharded=True every rank renders
    its share of each frame and computes the same values; only rank 0 writes the file.
    fit_embedding: None, or a dict of fit_image_embedding's keyword arguments (missing ones: embedding.FIT_DEFAULTS) plus "region":
    "left" (default: fit on the columns [0, w // 2), "psnr_heldout" on the others) or "all" (no held-out key).  Every rank fits the
    same vector from the same seed (no collective), so it works as it is under sharded=True.
    depth_mode: "mean" (default) or "median" -- the DSM, hence every MAE, is then that of the rays' median depths
    (SNERF_FLAG_DEPTH_MEDIAN) and the dict carries "depth_mode": "median"; at the default the key is absent.  The embedding fit, a
    training render, never takes the mode."""
    ro_depth = with_depth_mode({}, depth_mode, "eval_nerf_images")
    from .utils.dsm import compute_dsm_and_mae
    from .utils import embedding
    start = 1 if split == "test" else 0
    todo = list(images)[start:]
    if not todo:
        raise ValueError(f"no {split} image to evaluate")
    with_dsm = [img.get("dsm") is not None for img in todo]
    if any(with_dsm) and not all(with_dsm):
        raise ValueError("every image of the split needs a 'dsm' entry, or none may have one")
    infer = sharded_lean_inference if sharded else lean_inference
    stats_fp = os.path.join(output_dp, "results.json") if output_dp is not None else None
    if stats_fp is not None:
        os.makedirs(output_dp, exist_ok=True)
    per_image, d, vectors = {}, {}, {}
    region, fit_kw = embedding.fit_options(fit_embedding) if fit_embedding is not None else (None, None)
    for img in todo:
        rays = img["rays"].reshape(-1, img["rays"].shape[-1])
        extras = img["extras"].reshape(-1, img["extras"].shape[-1]) if img.get("extras") is not None else None
        rgbs = img["rgbs"].reshape(-1, 3)
        W, H = _w_h(img, rays.shape[0])
        if region is None:
            results = infer(cfgs, renderer, models, rays, extras, keys=("rgb_coarse", "depth_coarse"), render_options=ro_depth)
        else:
            fit, fit_mask, t_fit = embedding.fit_for_image(cfgs, renderer, models, img, rays, extras, W, H, region, fit_kw)
            vectors[img["name"]] = [float(v) for v in fit["t"].cpu()]
            results = infer(cfgs, renderer, models, rays, extras, keys=("rgb_coarse", "depth_coarse"),
                            render_options=with_depth_mode(embedding.vector_options(fit), depth_mode))
        rgb = results["rgb_coarse"]
        entry = {}
        if img.get("dsm") is not None:
            g = img["dsm"]
            # the depth is the whole frame on every rank (also when sharded): no all-reduce of the DSM accumulators
            mae = compute_dsm_and_mae(rays, results["depth_coarse"], g["gt"], g["roi"], to_world=g.get("to_world"),
                                      water_mask=g.get("water_mask"), ignore_mask=g.get("ignore_mask"), distributed=False,
                                      geo=g.get("geo"))
            entry["mae"] = _mae_floats(mae)
        psnr_ = metrics.psnr(rgb, rgbs)
        ssim_ = metrics.ssim(rgb.view(1, 3, H, W), rgbs.reshape(1, 3, H, W))
        entry["psnr"] = "{:.2f}".format(float(psnr_))
        entry["ssim"] = "{:.3f}".format(float(ssim_))
        if region is not None:
            if region == "left":
                entry["psnr_heldout"] = "{:.2f}".format(float(metrics.psnr(rgb, rgbs, valid_mask=~fit_mask)))
            entry["t_fit"] = t_fit
        per_image[img["name"]] = entry
        n = len(per_image)
        d = dict(per_image)
        if depth_mode != "mean":
            d["depth_mode"] = depth_mode
        if with_dsm[0]:
            d["MAE (Mean)"] = "{:.3f}".format(sum(v["mae"]["mean"] for v in per_image.values()) / n)
            d["MAE (Median)"] = "{:.3f}".format(sum(v["mae"]["median"] for v in per_image.values()) / n)
        d["PSNR (Mean)"] = "{:.2f}".format(sum(float(v["psnr"]) for v in per_image.values()) / n)
        d["SSIM (Mean)"] = "{:.3f}".format(sum(float(v["ssim"]) for v in per_image.values()) / n)
        if stats_fp is not None and world()[0] == 0:
            with open(stats_fp, "w") as f:
                json.dump(d, f, indent=4)
            if region is not None:
                with open(os.path.join(output_dp, "t_fit.json"), "w") as f:
                    json.dump(vectors, f, indent=4)
    return d
