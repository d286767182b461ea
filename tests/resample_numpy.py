"""numpy restatement of snerf_resample_z (include/snerf_hip.h), operation for operation: the oracle of
tests/test_gpu_resample.py and the object tests/test_resample_cpu.py compares with the reference's sample_pdf.

Every operation is fp64 and rounded on its own (numpy never contracts), the cdf is a prefix sum of int64 masses, and the merge
is numpy's stable argsort -- so the result has no summation order and every bit of it is fixed."""
import numpy as np

EPS = 1e-5
SCALE = float(2 ** 50)
MAX_SAMPLES = 1024        # SNERF_VIS_MAX_SAMPLES: n_samples + n_importance may not exceed it


def bins(z):
    """b (N, S - 1) fp64: the interval midpoints of the coarse depths"""
    z = np.asarray(z, np.float32).astype(np.float64)
    return 0.5 * (z[:, :-1] + z[:, 1:])


def masses(weights):
    """m (N, S - 2) int64 of the interior weights: llrint((w' + 1e-5) * 2^50), w' = w where finite and > 0, else 0, at most 1"""
    w = np.asarray(weights, np.float32)[:, 1:-1]
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(w) & (w > 0)
    wd = np.minimum(np.where(keep, w, np.float32(0)).astype(np.float64), 1.0)
    return np.rint((wd + EPS) * SCALE).astype(np.int64)


def uniforms(u, n_rays, n_importance):
    """u (N, Ni) fp64 in [0, 1]: the given ones (NaN and everything <= 0 -> +0, above 1 -> 1), or i / (Ni - 1) for u = None"""
    if u is None:
        row = np.arange(n_importance, dtype=np.float64) / np.float64(n_importance - 1) if n_importance > 1 else np.zeros(1)
        return np.broadcast_to(row, (n_rays, n_importance))
    ud = np.asarray(u, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(ud > 0, np.minimum(ud, 1.0), 0.0)


def fine_samples(z, weights, n_importance, u=None, return_bins=False):
    """z_fine (N, Ni) fp32, in u's order [and k (N, Ni), the bin of each sample]"""
    z = np.asarray(z, np.float32)
    N, S = z.shape
    assert S >= 3 and n_importance >= 1 and S + n_importance <= MAX_SAMPLES
    b = bins(z)
    m = masses(weights)
    P = np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(m, 1, dtype=np.int64)], 1)      # (N, S - 1), P[:, S - 2] = T
    Pd = P.astype(np.float64)
    t = uniforms(u, N, n_importance) * Pd[:, -1:]
    # the largest j in [0, S - 3] with (double)P[j] <= t
    k = np.empty((N, n_importance), np.int64)
    for n in range(N):
        k[n] = np.clip(np.searchsorted(Pd[n, :S - 2], t[n], side="right") - 1, 0, S - 3)
    rows = np.arange(N)[:, None]
    f = (t - Pd[rows, k]) / m[rows, k].astype(np.float64)
    lo = b[rows, k]
    fine = (lo + f * (b[rows, k + 1] - lo)).astype(np.float32)
    return (fine, k) if return_bins else fine


def resample_z(z, weights, n_importance, u=None):
    """-> (z_out (N, S + Ni), z_fine (N, Ni)): the coarse depths and the fine samples merged by numpy's stable argsort"""
    z = np.asarray(z, np.float32)
    fine = fine_samples(z, weights, n_importance, u)
    both = np.concatenate([z, fine], 1)
    order = np.argsort(both, axis=1, kind="stable")
    return np.take_along_axis(both, order, 1), fine
