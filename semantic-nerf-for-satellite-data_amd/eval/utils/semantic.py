"""Streaming semantic evaluation of one image on the device (csrc/semeval.hip): the per-image numbers of the reference's
eval/eval_semantic.py:65-117 -- semantic accuracies (semantic/components/metrics.py:11-29), the row-normalised confusion
matrix (torchmetrics' MulticlassConfusionMatrix(normalize="true")), the mIoU over that matrix (metrics.py:32-42) and the
uncertainty at transient (car) pixels (metrics.py:79-87).

Every render chunk is folded into a device accumulator (include/snerf_hip.h SnerfSemevalAcc: exact 64-bit integer counts and
an fp64 sum of the car rays' composited beta) as soon as it is rendered, so neither the whole-frame (N, S) weights and beta
nor a host round trip exist before the image's one host read in `image_entry`.  The host then restates the reference's
arithmetic from the exact counts:
- accuracy = f32(1) - f32(errors) / f32(n), fp32 as torch computes 1 - (sum(error) / len(targets)) (bit for bit while the
  counts stay below 2^24, where torch's fp32 sum of the 0/1 errors is exact);
- matrix = f32(counts) / f32(row sum), an empty row (NaN) set to 0, as torchmetrics does;
- mIoU = the reference's per-class formula in fp32 over that matrix, then np.nanmean;
- uncertainty = (sum over car rays of sum_s w_s beta_s) / (car rays), fp64 (the reference's fp32 sum differs by its rounding);
  no car ray gives 0/0 = NaN, as in the reference."""
import ctypes as C

import numpy as np
import torch

from ... import _lib, parallel
from ...framework.components.rendering import n_render_samples

_NCOUNT = (C.sizeof(_lib.SnerfSemevalAcc) - 8) // 8        # u64 fields before the fp64 beta sum
_MAXC = _lib.SEMEVAL_MAX_CLASSES
_ERR0 = _MAXC * _MAXC                                      # errors[4], then rays, car_rays, out_of_range


def accuracy_from_errors(errors: int, n: int) -> float:
    """semantic_accuracy (metrics.py:25-29) from the exact error count: 1 - (sum(error) / len(targets)) in fp32"""
    return float(np.float32(1) - np.float32(errors) / np.float32(n))


def normalized_confusion(counts) -> np.ndarray:
    """MulticlassConfusionMatrix(normalize="true").compute() of (C, C) int counts [gt][pred]: fp32 division by the row sums,
    NaN of an empty row -> 0"""
    counts = np.asarray(counts, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cm = counts.astype(np.float32) / counts.sum(axis=1, keepdims=True).astype(np.float32)
    cm[np.isnan(cm)] = 0
    return cm


def semantic_miou(cm: np.ndarray) -> float:
    """semantic_mIoU (metrics.py:32-42) as written: per class cm[c, c] / (row sum + column sum - cm[c, c]) in the matrix's
    dtype, a class absent from both (0 / 0) is NaN and skipped by np.nanmean (all NaN: NaN)"""
    n = cm.shape[0]
    ious = np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(n):
            ious[c] = cm[c, c] / (np.sum(cm[c, :]) + np.sum(cm[:, c]) - cm[c, c])
    if np.isnan(ious).all():
        return float("nan")
    return float(np.nanmean(ious))


def entry_from_stats(conf, errors, n, car_rays, beta_car_sum, no_cars=True, non_corrupted=False, beta=True) -> dict:
    """the reference's per-image dict (eval_semantic.py:87-117, its key order) from an image's statistics: (C, C) counts
    [gt][pred], the four error counts (SnerfSemevalAcc.errors), the ray and car-ray counts and the fp64 beta sum; the
    optional terms are present iff their flag is set"""
    cm = normalized_confusion(conf)
    e = {"semantic_accuracy": accuracy_from_errors(errors[0], n)}
    if no_cars:
        e["semantic_accuracy_wo_cars"] = accuracy_from_errors(errors[1], n)
    e["mIoU"] = semantic_miou(cm)
    if beta:
        e["uncertainty_at_transient"] = beta_car_sum / car_rays if car_rays else float("nan")
    e["confusion_matrix"] = cm.tolist()
    if non_corrupted:
        e["semantic_accuracy_comparison_non_corrupted"] = accuracy_from_errors(errors[2], n)
        e["semantic_accuracy_comparison_non_corrupted_wo_cars"] = accuracy_from_errors(errors[3], n)
    return e


def _labels(t, n, what):
    if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"{what} must be uint8 or int64, not {t.dtype}")
    if t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} entries for {n} rays")
    return t.reshape(-1).contiguous()


class SemanticEvalAccumulator:
    """Device accumulator of one image's semantic statistics (several chunks, several ranks): add() per chunk, allreduce_()
    under data parallelism, then one host read through image_entry() / counts()."""

    def __init__(self, n_classes: int, car_cls_idx=None, device="cuda"):
        n_classes, car = int(n_classes), (-1 if car_cls_idx is None else int(car_cls_idx))
        if not 1 <= n_classes <= _MAXC:
            raise ValueError(f"n_classes = {n_classes} outside [1, {_MAXC}]")
        if not -1 <= car < n_classes:
            raise ValueError(f"car_cls_idx = {car_cls_idx} outside [0, {n_classes}) (None: no car class)")
        self.n_classes, self.car_cls_idx = n_classes, car
        self.device = torch.device(device)
        self.buf = torch.zeros(_NCOUNT + 1, dtype=torch.int64, device=self.device)
        self._work = None
        self._host = None
        self.has = {"semantic_no_cars": None, "semantic_non_corrupted": None, "beta": None}

    def _seen(self, key, present):
        if self.has[key] is None:
            self.has[key] = present
        elif self.has[key] != present:
            raise ValueError(f"'{key}' was given for some chunks of the image and not for others")

    def add(self, pred, gt, gt_no_cars=None, gt_non_corrupted=None, weights=None, beta=None):
        """fold one chunk: pred (n,) int64 labels; gt, gt_no_cars, gt_non_corrupted (n,) or (n, 1) uint8 / int64 targets;
        weights (n, S) and beta (n, S, 1) fp32, given together or not at all.  Asynchronous on the current stream."""
        if not torch.is_tensor(pred) or pred.dtype != torch.int64:
            raise ValueError("pred must be an int64 tensor")
        n = pred.numel()
        if n >= 2 ** 31:
            raise ValueError(f"{n} rays in one chunk: at most 2^31 - 1")
        p = pred.reshape(-1).contiguous()
        tg = [_labels(t, n, w) if t is not None else None for t, w in
              ((gt, "gt"), (gt_no_cars, "gt_no_cars"), (gt_non_corrupted, "gt_non_corrupted"))]
        dts = {t.dtype for t in tg if t is not None}
        if len(dts) > 1:          # one label dtype per launch: widen
            tg = [t.long() if t is not None else None for t in tg]
        i64 = tg[0].dtype == torch.int64
        if (weights is None) != (beta is None):
            raise ValueError("weights and beta are given together or not at all")
        S = 1
        if weights is not None:
            if weights.dim() != 2 or weights.shape[0] != n or weights.dtype != torch.float32:
                raise ValueError(f"weights must be fp32 (n, S) with n = {n}")
            S = weights.shape[1]
            if beta.shape not in ((n, S, 1), (n, S)) or beta.dtype != torch.float32:
                raise ValueError(f"beta must be fp32 ({n}, {S}, 1)")
            weights, beta = weights.contiguous(), beta.contiguous()
        self._seen("semantic_no_cars", gt_no_cars is not None)
        self._seen("semantic_non_corrupted", gt_non_corrupted is not None)
        self._seen("beta", weights is not None)
        nbytes = 0
        if weights is not None:
            nbytes = _lib.call_size("snerf_semeval_workspace_bytes", n, S, exc=ValueError)
            if self._work is None or self._work.numel() * 8 < nbytes:
                self._work = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
            nbytes = self._work.numel() * 8
        _lib.call("snerf_semeval_accumulate", p, tg[0], tg[1], tg[2], _lib.SEMEVAL_I64 if i64 else _lib.SEMEVAL_U8, n,
                  self.n_classes, self.car_cls_idx, weights, beta, S, self.buf, self._work if weights is not None else None,
                  nbytes, exc=ValueError)
        self._host = None
        return self

    def allreduce_(self):
        """combine the ranks' accumulators: the integer counts by one SUM all-reduce, the fp64 beta sum by an all_gather summed
        in rank order (every rank holds the same bits).  Single process: nothing."""
        if parallel.world()[1] == 1:
            return self
        counts = self.buf[:_NCOUNT].clone()
        parallel.allreduce_sum_(counts)
        bsum = self.buf[_NCOUNT:].view(torch.float64)
        parts = parallel.allgather(bsum)
        total = parts[0].clone()
        for part in parts[1:]:
            total += part
        self.buf[:_NCOUNT].copy_(counts)
        bsum.copy_(total)
        self._host = None
        return self

    def _read(self):
        if self._host is None:
            h = self.buf.cpu().numpy()                         # the one host read (synchronises with the stream)
            C_ = self.n_classes
            conf = h[:_ERR0].reshape(_MAXC, _MAXC)[:C_, :C_].copy()
            e = h[_ERR0:_NCOUNT]
            self._host = {"conf": conf, "errors": [int(v) for v in e[:4]], "rays": int(e[4]), "car_rays": int(e[5]),
                          "out_of_range": int(e[6]), "beta_car_sum": float(h[_NCOUNT:].view(np.float64)[0])}
        return self._host

    def counts(self) -> np.ndarray:
        """(C, C) int64 confusion counts [gt][pred]"""
        return self._read()["conf"].copy()

    def image_entry(self) -> dict:
        """the reference's per-image dict (eval_semantic.py:87-117), in its key order; refuses targets outside [0, C)"""
        h = self._read()
        n = h["rays"]
        if n == 0:
            raise ValueError("no ray was accumulated")
        if h["out_of_range"]:
            raise ValueError(f"{h['out_of_range']} rays have a label outside [0, {self.n_classes}) "
                             "(ground truth or prediction)")
        return entry_from_stats(h["conf"], h["errors"], n, h["car_rays"], h["beta_car_sum"], self.has["semantic_no_cars"],
                                self.has["semantic_non_corrupted"], self.has["beta"])


def _slice(t, lo, hi):
    return t[lo:hi] if t is not None else None


@torch.no_grad()
def lean_semantic_eval(cfgs, renderer, models, rays, extras, semantic, semantic_no_cars=None, semantic_non_corrupted=None,
                       car_cls_idx=None, n_classes=None, render_options={}, acc=None):
    """Render the frame `rays` chunk by chunk (util.render_chunks, as lean_inference: the same per-chunk jitter from the same
    RNG state, hence the same labels) and fold every chunk's labels, weights and beta into `acc` (a new
    SemanticEvalAccumulator over n_classes, default the model's class count, if None).  The chunk-sized result buffers are
    allocated once; no (N, S) tensor of the frame exists.  Returns the accumulator (nothing is read back)."""
    from ... import ops
    from .util import render_chunks, result_buffers
    Cn = models["coarse"].spec.n_classes
    if Cn == 0:
        raise ValueError("the model has no semantic head (n_classes = 0)")
    n = rays.shape[0]
    if acc is None:
        acc = SemanticEvalAccumulator(Cn if n_classes is None else n_classes, car_cls_idx, rays.device)
    for t, what in ((semantic, "semantic"), (semantic_no_cars, "semantic_no_cars"),
                    (semantic_non_corrupted, "semantic_non_corrupted")):
        if t is not None and t.shape[0] != n:
            raise ValueError(f"{what} has {t.shape[0]} rows for {n} rays")
    ops.release_workspaces()
    bufs = result_buffers(("semantic_label", "weights", "beta"), min(cfgs.pipeline.render_chunk_size, n), n_render_samples(cfgs.pipeline),
                          Cn, rays.device)
    for i, k, v in render_chunks(cfgs, renderer, models, rays, extras, bufs, render_options):
        acc.add(v["semantic_label_coarse"], semantic[i:i + k], _slice(semantic_no_cars, i, i + k),
                _slice(semantic_non_corrupted, i, i + k), weights=v["weights_coarse"], beta=v["beta_coarse"])
    return acc


@torch.no_grad()
def sharded_lean_semantic_eval(cfgs, renderer, models, rays, extras, semantic, semantic_no_cars=None,
                               semantic_non_corrupted=None, car_cls_idx=None, n_classes=None, render_options={}):
    """lean_semantic_eval with the frame's rays sharded over the process group: every rank streams its frame_shard slice
    into its own accumulator, then allreduce_() gives every rank the frame's statistics (counts bit-equal to one process;
    the beta sum differs from it only by the grouping of its fp64 partials).  Per-ray jitter given for the whole frame is
    sliced with the rays; drawn jitter is each rank's own."""
    from .util import shard_options
    n = rays.shape[0]
    Cn = models["coarse"].spec.n_classes
    if Cn == 0:
        raise ValueError("the model has no semantic head (n_classes = 0)")
    acc = SemanticEvalAccumulator(Cn if n_classes is None else n_classes, car_cls_idx, rays.device)
    lo, hi = parallel.frame_shard(n)
    if hi > lo:
        lean_semantic_eval(cfgs, renderer, models, rays[lo:hi], extras[lo:hi] if extras is not None else None,
                           semantic[lo:hi], _slice(semantic_no_cars, lo, hi), _slice(semantic_non_corrupted, lo, hi),
                           render_options=shard_options(render_options, lo, hi, n), acc=acc)
    else:    # more ranks than rays: nothing to add, but the optional terms must match the other ranks'
        acc.has.update(semantic_no_cars=semantic_no_cars is not None,
                       semantic_non_corrupted=semantic_non_corrupted is not None, beta=True)
    return acc.allreduce_()
