"""fp64 / integer restatement of the semantic evaluation's statistics (include/snerf_hip.h SnerfSemevalAcc), in numpy, from the
spec (the reference's semantic/components/metrics.py:11-87): what csrc/semeval.hip must accumulate for one image."""
import numpy as np

from tests import reduce_numpy as RN


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


def beta_car_sum_in_kernel_order(gt, car_idx, weights, beta, threads=256, max_grid=2048):
    """beta_car_sum of ONE snerf_semeval_accumulate call into a zeroed accumulator, bit for bit (csrc/semeval.hip, reduce.h).
    fma((double)w, (double)b, acc) of fp32 w and b has an exact fp64 product: one fp64 addition of float64(w) * float64(b).
      - workgroup b of the grid takes the tiles (256 rays) b, b + grid, ...;
      - thread t takes the flat elements t, t + 256, ... of a tile's (rays, S) block in ascending order and skips the rays
        whose target is not the car class (a tile without a car ray is skipped whole: the same sum);
      - the 256-way tree gives partial[b]; the reduce launch sums the partials strided over 256 threads, then the tree."""
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    n = g.shape[0]
    w = np.asarray(weights, np.float32).reshape(n, -1)
    S = w.shape[1]
    prod = (w.astype(np.float64) * np.asarray(beta, np.float32).reshape(n, S).astype(np.float64)).reshape(-1)
    car = np.repeat(g == car_idx, S)
    grid = RN.blocks_for(n, threads, max_grid)
    tiles = -(-n // threads)
    t = np.arange(threads)
    acc = np.zeros((grid, threads))
    for j in range(-(-tiles // grid)):                       # the workgroups' j-th tile
        tile = np.arange(grid) + j * grid
        for m in range(S):                                   # the threads' m-th element of it: S * 256 elements a full tile
            e = tile[:, None] * (threads * S) + m * threads + t[None, :]
            ok = e < n * S
            ec = np.where(ok, e, 0)
            acc = np.where(ok & car[ec], acc + prod[ec], acc)
    return float(RN.strided_sum(RN.tree(acc), threads))


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
