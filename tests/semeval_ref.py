"""fp64 / integer restatement of the semantic evaluation's statistics (include/snerf_hip.h SnerfSemevalAcc), in numpy, from the
spec (the reference's semantic/components/metrics.py:11-87): what csrc/semeval.hip must accumulate for one image."""
import numpy as np


def stats(pred, gt, n_classes, car_idx=-1, gt_no_cars=None, gt_non_corrupted=None, weights=None, beta=None):
    """-> dict(conf (C, C) int64 [gt][pred], errors [4] (None where the target is absent), rays, car_rays, out_of_range,
    beta_car_sum (fp64; None without weights))"""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    n, C = p.shape[0], n_classes
    ok = (g >= 0) & (g < C) & (p >= 0) & (p < C)
    conf = np.bincount(g[ok] * C + p[ok], minlength=C * C).reshape(C, C).astype(np.int64)
    car = (g == car_idx) if car_idx >= 0 else np.zeros(n, bool)
    errors = [int((g != p).sum()), None, None, None]
    if gt_no_cars is not None:
        errors[1] = int((np.asarray(gt_no_cars).reshape(-1).astype(np.int64) != p).sum())
    if gt_non_corrupted is not None:
        q = np.asarray(gt_non_corrupted).reshape(-1).astype(np.int64)
        wrong = q != p
        errors[2] = int(wrong.sum())
        errors[3] = int((wrong & ~((q == car_idx) if car_idx >= 0 else np.zeros(n, bool))).sum())
    bsum = None
    if weights is not None:
        w = np.asarray(weights, np.float64).reshape(n, -1)
        b = np.asarray(beta, np.float64).reshape(n, -1)
        bsum = float(np.sum(np.sum(w * b, axis=1)[car]))
    return {"conf": conf, "errors": errors, "rays": n, "car_rays": int(car.sum()), "out_of_range": int((~ok).sum()),
            "beta_car_sum": bsum}


def accuracy(errors, n):
    """1 - errors / n in fp64"""
    return 1.0 - errors / n


def normalized(conf):
    """row-normalised matrix in fp64, empty rows 0"""
    conf = np.asarray(conf, np.float64)
    rs = conf.sum(1, keepdims=True)
    return np.divide(conf, rs, out=np.zeros_like(conf), where=rs > 0)


def miou(cm):
    """per-class IoU over the matrix in fp64, NaN classes skipped"""
    cm = np.asarray(cm, np.float64)
    d = np.diag(cm)
    den = cm.sum(1) + cm.sum(0) - d
    with np.errstate(invalid="ignore", divide="ignore"):
        ious = d / den
    return float(np.nanmean(ious)) if not np.isnan(ious).all() else float("nan")
