#!/usr/bin/env python3
"""Generate the golden vectors of the semantic evaluation by running the REFERENCE's own semantic/components/metrics.py and
eval/eval_semantic.py.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_semeval.py

The reference's import chain needs toml, gpustat, lightning, pytorch_lightning, rasterio, torchmetrics, torchvision, fire, cv2,
utm and pymap3d, none of which is installed (and torch.utils.data.dataset.T_co, which torch 2 dropped: it is defined again): they are stubbed (every attribute is an inert class), and the functions used never touch them,
with one exception -- torchmetrics' MulticlassConfusionMatrix, which the reference's loop and `confusion_matrix` call.  Its
stub RESTATES torchmetrics: bincount of target * C + pred into a (C, C) [gt][pred] matrix, a target outside [0, C) refused,
with normalize="true" fp32 division by the row sums and NaN -> 0.  The matrix values, hence the mIoU values, therefore come
from that restatement; the per-class mIoU formula, the accuracies, the uncertainty, the loop, its key set, formats, running
means and skip logic are the reference's own.  Writes tests/golden/:
- semeval_metrics_c<C>.npz: a synthetic case per class count C in (2, 5, 9, 16) with ragged N: pred (N,) int64, gt and
  gt_no_cars (N, 1) uint8, weights (N, S), beta (N, S, 1) fp32, car_idx, and the reference's semantic_accuracy without and
  with filter_idx = car_idx (acc, acc_filter, fp32), semantic_accuracy against gt_no_cars (acc_no_cars), the normalised
  matrix (cm, fp32), semantic_mIoU of it (miou, fp64) and uncertainty_at_transient (unc, fp32).  C = 2: every prediction
  correct; C = 5: a class predicted but absent from the ground truth; C = 9: no car ray (NaN); C = 16: classes absent from
  both;
- semeval_loop_<type>.npz / .json for semantic_dataset_type "own" and "own_corrupted": the fake dataset's four images
  (item 0 is skipped on the test split) with their precomputed predictions, and the results.json eval_semantic_nerfs wrote.
"""
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
STUBBED = ("toml", "gpustat", "lightning", "pytorch_lightning", "rasterio", "torchmetrics", "torchvision", "fire", "cv2", "pymap3d", "utm")


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


class MulticlassConfusionMatrix:
    """restatement of torchmetrics.classification.MulticlassConfusionMatrix (see the module docstring)"""

    def __init__(self, num_classes, normalize=None, **kwargs):
        self.num_classes, self.normalize = num_classes, normalize
        self.confmat = torch.zeros(num_classes, num_classes, dtype=torch.int64)

    def _batch(self, preds, target):
        C = self.num_classes
        preds, target = preds.reshape(-1).long(), target.reshape(-1).long()
        for t in (preds, target):
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= C):
                raise RuntimeError("labels outside [0, num_classes)")
        return torch.bincount(target * C + preds, minlength=C * C).reshape(C, C)

    def _reduce(self, confmat):
        if self.normalize != "true":
            return confmat
        cm = confmat.float()
        cm = cm / cm.sum(axis=-1, keepdim=True)
        cm[torch.isnan(cm)] = 0
        return cm

    def update(self, preds, target):
        self.confmat += self._batch(preds, target)

    def compute(self):
        return self._reduce(self.confmat)

    def __call__(self, preds, target):
        b = self._batch(preds, target)
        self.confmat += b
        return self._reduce(b)


def load_reference():
    sys.meta_path.insert(0, _StubFinder())
    import typing
    import torch.utils.data.dataset as tud
    if not hasattr(tud, "T_co"):          # framework/datasets.py imports it; torch 2.x no longer defines it
        tud.T_co = typing.TypeVar("T_co", covariant=True)
    import torchmetrics.classification
    torchmetrics.classification.MulticlassConfusionMatrix = MulticlassConfusionMatrix
    sys.path.insert(0, REF)
    import semantic.components.metrics as metrics
    import eval.eval_semantic as loop
    metrics.plot_confusion_matrix = lambda metric, labels: None      # matplotlib figure of the PNG: out of scope
    return metrics, loop


M, LOOP = load_reference()


def frame(rng, n, C, S, car, correct=0.8, absent=(), absent_pred=(), no_car=False):
    """synthetic labels, predictions and per-sample weights / beta of an n-ray frame"""
    classes = np.array([c for c in range(C) if c not in absent and not (no_car and c == car)])
    gt = rng.choice(classes, n).astype(np.uint8)
    pred = gt.astype(np.int64).copy()
    wrong = rng.random(n) >= correct
    pick = np.array([c for c in range(C) if c not in absent or c in absent_pred])
    pred[wrong] = rng.choice(pick, int(wrong.sum()))
    for c in absent_pred:                                  # a class predicted but absent from the ground truth
        pred[rng.choice(n, 3, replace=False)] = c
    gt_no_cars = gt.copy()
    if car >= 0:
        gt_no_cars[gt == car] = (car + 1) % C
    z = rng.standard_normal((n, S)) * 2.0
    w = np.exp(z) / np.exp(z).sum(1, keepdims=True) * rng.uniform(0.6, 1.0, (n, 1))
    beta = rng.uniform(0.05, 1.2, (n, S, 1))
    return {"pred": pred, "gt": gt[:, None], "gt_no_cars": gt_no_cars[:, None], "weights": w.astype(np.float32),
            "beta": beta.astype(np.float32)}


def metric_case(rng, C, n, S, car, **kw):
    f = frame(rng, n, C, S, car, **kw)
    res = {"semantic_label_coarse": torch.from_numpy(f["pred"]), "weights_coarse": torch.from_numpy(f["weights"]),
           "beta_coarse": torch.from_numpy(f["beta"])}
    gt, gnc = torch.from_numpy(f["gt"]), torch.from_numpy(f["gt_no_cars"])
    _, cm = M.confusion_matrix(res, gt, list(range(C)))
    out = dict(f, n_classes=np.int64(C), car_idx=np.int64(car),
               acc=M.semantic_accuracy(res, gt).numpy(), acc_filter=M.semantic_accuracy(res, gt, filter_idx=car).numpy(),
               acc_no_cars=M.semantic_accuracy(res, gnc).numpy(), cm=cm.numpy(), miou=np.float64(M.semantic_mIoU(cm.numpy())),
               unc=M.uncertainty_at_transient(res, gt, car).numpy())
    return out


class _Dataset:
    def __init__(self, images, C, car):
        self.images = images
        self.semantic_cls_labels = {f"class_{c}": c for c in range(C)}
        self.car_cls_idx = car

    def force_act_as_test(self):
        pass

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i]


def loop_case(rng, dataset_type):
    """four images, run through the reference's eval_semantic_nerfs with its loading and rendering replaced"""
    C, car, S = 6, 4, 6
    corrupted = "corrupted" in dataset_type
    sizes = (150, 211, 187, 240)
    frames, images, results = [], [], {}
    for i, n in enumerate(sizes):
        no_car = (not corrupted) and i == 2                   # "own": one image without a car ray (NaN, propagated)
        f = frame(rng, n, C, S, car, correct=0.75, absent=(1,) if i == 3 else (), no_car=no_car)
        img = {"name": f"img_{i}", "rays": torch.full((n, 11), float(i)), "extras": torch.zeros(n, 3),
               "semantic": torch.from_numpy(f["gt"]), "semantic_no_cars": torch.from_numpy(f["gt_no_cars"])}
        if corrupted:
            nc = f["gt"].copy()
            flip = rng.random(n) < 0.1
            nc[flip, 0] = rng.integers(0, C, int(flip.sum()))
            f["gt_non_corrupted"] = nc
            img["semantic_non_corrupted"] = torch.from_numpy(nc)
        images.append(img)
        results[i] = {"semantic_label_coarse": torch.from_numpy(f["pred"]), "weights_coarse": torch.from_numpy(f["weights"]),
                      "beta_coarse": torch.from_numpy(f["beta"])}
        frames.append(f)
    dataset = _Dataset(images, C, car)
    cfgs = types.SimpleNamespace(run=types.SimpleNamespace(run_name="run"),
                                 pipeline=types.SimpleNamespace(semantic_dataset_type=dataset_type))
    pipeline = types.SimpleNamespace(datasets={"rgb": dataset, "rgb_test": dataset}, load_datasets=lambda: None, renderer=None)
    LOOP.load_configs_from_logs = lambda dp: cfgs
    LOOP.adapt_configs_for_inference = lambda c: c
    LOOP.load_from_disk = lambda cfgs, dp, epoch, device, free: ({}, pipeline, epoch, "cpu")
    LOOP.batched_inference = lambda cfgs, renderer, models, rays, extras: results[int(rays[0, 0])]
    LOOP.save_image = lambda img, fp: None
    LOOP.plot_confusion_matrix = lambda metric, labels: None
    with tempfile.TemporaryDirectory() as tmp:
        LOOP.eval_semantic_nerfs(tmp, tmp, split="test")
        with open(os.path.join(tmp, "run", "eval_semantic", "test", "results.json"), "rb") as fh:
            text = fh.read()
    arrays = {"n_classes": np.int64(C), "car_idx": np.int64(car), "names": np.array([im["name"] for im in images])}
    for i, f in enumerate(frames):
        arrays.update({f"{k}_{i}": v for k, v in f.items()})
    return arrays, text


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    cases = {
        "semeval_metrics_c2": metric_case(rng, 2, 301, 7, 1, correct=1.0),
        "semeval_metrics_c5": metric_case(rng, 5, 437, 9, 2, absent=(3,), absent_pred=(3,)),
        "semeval_metrics_c9": metric_case(rng, 9, 389, 8, 6, no_car=True),
        "semeval_metrics_c16": metric_case(rng, 16, 515, 5, 15, absent=(4, 11)),
    }
    for name, res in cases.items():
        np.savez(os.path.join(OUT, name + ".npz"), **res)
        print(name, {k: np.round(res[k], 7).tolist() for k in ("acc", "acc_filter", "acc_no_cars", "miou", "unc")})
    for typ in ("own", "own_corrupted"):
        arrays, text = loop_case(rng, typ)
        np.savez(os.path.join(OUT, f"semeval_loop_{typ}.npz"), **arrays)
        with open(os.path.join(OUT, f"semeval_loop_{typ}.json"), "wb") as fh:
            fh.write(text)
        print(f"semeval_loop_{typ}", len(text), "bytes of results.json")


if __name__ == "__main__":
    main()
