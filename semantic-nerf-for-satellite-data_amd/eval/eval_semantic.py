"""Per-image semantic evaluation of a trained model -- the loop of the reference's eval/eval_semantic.py:23-152
(eval_semantic_nerfs) without checkpoint and dataset loading: the caller hands in the configs, the renderer, the models and
the split's images.

For every image the frame is rendered chunk by chunk and streamed into a device accumulator (eval/utils/semantic.py,
csrc/semeval.hip; with sharded=True every rank streams its share and the accumulators are all-reduced).  The image's entry
holds the semantic accuracy, the accuracy against "semantic_no_cars", the mIoU over the image's row-normalised confusion
matrix, the uncertainty (composited beta) at the car pixels and that matrix, plus the two comparisons against
"semantic_non_corrupted" when the images carry it (the reference's "corrupted" dataset types).  After each image the
entries and the six means ("{:.4f}") are written to `output_dp`/results.json; at the end the row-normalised matrix of the
split's summed counts is added as "confusion_matrix".

DIVERGENCES: no confusion-matrix PNG is written (per image nor "mean.png"; visualisers).  The reference reads
"semantic_no_cars" unconditionally; here "semantic_accuracy_wo_cars" is present iff the images carry it, and a split that mixes
images with and without it (or with and without "semantic_non_corrupted") is refused.  The uncertainty is the fp64 sum of
the car rays' composited beta over their count (the reference sums in fp32).  The accuracies are fp32 divisions, as torch
computes them on the CPU (on a GPU torch multiplies by the fp32 reciprocal of the ray count, which may differ in the last
bit).  A label outside [0, C) raises ValueError (torchmetrics raises its own error), and an empty split is refused (the
reference fails on it with a NameError).

ADDITION: `fit_embedding`, as in eval_nerf_images (eval/utils/embedding.py): per image the transient vector is fitted on a region of
the image's colours ("rgbs") with the network frozen and the frame is evaluated with it; the entry gains "t_fit" and, for region
"left", "psnr_heldout" (one more colour-only render of the frame with the vector), and the vectors go to `output_dp`/t_fit.json.
t_s, where the model has one, keeps its init.  None (the default) changes nothing."""
import json
import os

import numpy as np
import torch

from .utils.semantic import SemanticEvalAccumulator, lean_semantic_eval, normalized_confusion, sharded_lean_semantic_eval
from ..parallel import world

# eval_semantic.py:120-127, in its order
MEAN_KEYS = {
    "semantic_accuracy": "Semantic Accuracy (Mean)",
    "semantic_accuracy_wo_cars": "Semantic Accuracy with no cars (Mean)",
    "mIoU": "mIoU (Mean)",
    "semantic_accuracy_comparison_non_corrupted": "Semantic Accuracy comparison to GT (Mean)",
    "semantic_accuracy_comparison_non_corrupted_wo_cars": "Semantic Accuracy comparison to GT w/o cars (Mean)",
    "uncertainty_at_transient": "Uncertainty at transient (Mean)",
}


def semantic_results(entries: dict, split_counts=None) -> dict:
    """The dict the reference writes to results.json (eval_semantic.py:119-152), without rendering: the per-image `entries`
    ({name: image_entry()}) in order, then every mean of MEAN_KEYS as "{:.4f}" (summed over the images that have the metric,
    divided by the number of images; a NaN propagates), and with `split_counts` ((C, C) int counts summed over the split) the
    final "confusion_matrix", their row-normalised matrix."""
    if not entries:
        raise ValueError("no image to report")
    d = dict(entries)
    for key, name in MEAN_KEYS.items():
        v = 0.0
        for e in entries.values():
            if key in e:
                v += float(e[key])
        d[name] = "{:.4f}".format(v / len(entries))
    if split_counts is not None:
        d["confusion_matrix"] = normalized_confusion(split_counts).tolist()
    return d


def _rows(t, n, name, key):
    t = t.reshape(-1)
    if t.shape[0] != n:
        raise ValueError(f"image {name!r}: '{key}' has {t.shape[0]} entries for {n} rays")
    return t


@torch.no_grad()
def eval_semantic_images(cfgs, renderer, models, images, n_classes, car_cls_idx, output_dp=None, split="test", sharded=False,
                         render_options=None, fit_embedding=None):
    """images: a sequence of dicts with the reference's item keys ("name", "rays", "extras", "semantic" (H*W, 1) uint8 and the
    optional "semantic_no_cars" / "semantic_non_corrupted" of the same shape).  n_classes = len(semantic_cls_labels),
    car_cls_idx = the dataset's car class (None: no car class).  On the test split item 0 is skipped (eval_semantic.py:55-58).
    render_options are handed to every render (default: the renderer's, which jitters the samples, as the reference does).
    Returns the dict written to results.json; with sharded=True every rank renders its share of each frame and computes the
    same dict, and only rank 0 writes the file.  fit_embedding: see eval_nerf_images (the images then carry "rgbs" and, unless the
    frame is square, "w" and "h")."""
    from .eval_nerf import _w_h
    from .utils import embedding, metrics
    from .utils.util import lean_inference, sharded_lean_inference
    start = 1 if split == "test" else 0
    todo = list(images)[start:]
    if not todo:
        raise ValueError(f"no {split} image to evaluate")
    opt = {}
    for key in ("semantic_no_cars", "semantic_non_corrupted"):
        has = [img.get(key) is not None for img in todo]
        if any(has) and not all(has):
            raise ValueError(f"every image of the split needs a '{key}' entry, or none may have one")
        opt[key] = has[0]
    stats_fp = os.path.join(output_dp, "results.json") if output_dp is not None else None
    write = stats_fp is not None and world()[0] == 0
    if write:
        os.makedirs(output_dp, exist_ok=True)
    run = sharded_lean_semantic_eval if sharded else lean_semantic_eval
    entries, split_counts = {}, np.zeros((n_classes, n_classes), np.int64)
    d, vectors = {}, {}
    region, fit_kw = embedding.fit_options(fit_embedding) if fit_embedding is not None else (None, None)
    for img in todo:
        rays = img["rays"].reshape(-1, img["rays"].shape[-1])
        n = rays.shape[0]
        extras = img["extras"].reshape(-1, img["extras"].shape[-1]) if img.get("extras") is not None else None
        tg = {k: (_rows(img[k], n, img.get("name"), k) if k == "semantic" or opt[k] else None)
              for k in ("semantic", "semantic_no_cars", "semantic_non_corrupted")}
        kw = dict(car_cls_idx=car_cls_idx, n_classes=n_classes, render_options=render_options or {})
        if region is not None:
            W, H = _w_h(img, n)
            fit, fit_mask, t_fit = embedding.fit_for_image(cfgs, renderer, models, img, rays, extras, W, H, region, fit_kw)
            vectors[img["name"]] = [float(v) for v in fit["t"].cpu()]
            kw["render_options"] = embedding.vector_options(fit, render_options)
        if not sharded:
            kw["acc"] = SemanticEvalAccumulator(n_classes, car_cls_idx, rays.device)
        acc = run(cfgs, renderer, models, rays, extras, tg["semantic"], tg["semantic_no_cars"], tg["semantic_non_corrupted"],
                  **kw)
        entries[img["name"]] = acc.image_entry()
        if region is not None:
            if region == "left":
                rgb = (sharded_lean_inference if sharded else lean_inference)(
                    cfgs, renderer, models, rays, extras, keys=("rgb_coarse",), render_options=kw["render_options"])["rgb_coarse"]
                entries[img["name"]]["psnr_heldout"] = "{:.2f}".format(float(metrics.psnr(rgb, img["rgbs"].reshape(-1, 3), valid_mask=~fit_mask)))
            entries[img["name"]]["t_fit"] = t_fit
        split_counts += acc.counts()
        d = semantic_results(entries)
        if write:
            with open(stats_fp, "w") as f:
                json.dump(d, f, indent=4)
    d = semantic_results(entries, split_counts)
    if write:
        with open(stats_fp, "w") as f:
            json.dump(d, f, indent=4)
        if region is not None:
            with open(os.path.join(output_dp, "t_fit.json"), "w") as f:
                json.dump(vectors, f, indent=4)
    return d
