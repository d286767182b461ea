"""numpy restatement of the median-depth launch (SNERF_FLAG_DEPTH_MEDIAN in include/snerf_hip.h), operation for
operation: the oracle of tests/test_gpu_depth_median.py and the object tests/test_depth_median_cpu.py compares with exact arithmetic.

Every operation is fp64 and rounded on its own (numpy never contracts) and every sum is over int64 integers -- so the result has no
summation order and every bit of it is fixed."""
import numpy as np

Q = float(2 ** 50)
MAX_SAMPLES = 1024        # SNERF_VIS_MAX_SAMPLES


def bad_rays(weights, z_vals, sigmas=None):
    """(N,) bool: a weight or depth -- or, where given, a sigma -- that is not finite, or a decreasing depth"""
    w, z = np.asarray(weights, np.float32), np.asarray(z_vals, np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(w).all(1) | ~np.isfinite(z).all(1) | (z[:, 1:] < z[:, :-1]).any(1)
    if sigmas is not None:
        bad |= ~np.isfinite(np.asarray(sigmas, np.float32)).all(1)
    return bad


def masses(weights):
    """a = llrint(min(max((double)w, 0), 1) * 2^50), int64 (N, S); a zero of either sign gives +0, a NaN (a bad ray's) 0"""
    w = np.asarray(weights, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        wc = np.where(w > 0.0, np.minimum(w, 1.0), 0.0)
    return np.rint(wc * Q).astype(np.int64)


def crossing(a):
    """-> (j (N,), A_j (N,), a_j (N,), AT (N,)): the first index with 2 (A_j + a_j) >= AT, its exclusive prefix and its mass.  With
    AT == 0 that is index 0 (the caller does not use it)."""
    a = np.asarray(a, np.int64)
    incl = np.cumsum(a, 1, dtype=np.int64)
    AT = incl[:, -1]
    j = np.argmax(2 * incl >= AT[:, None], axis=1)            # the first True; one exists: 2 incl[-1] = 2 AT >= AT
    rows = np.arange(a.shape[0])
    aj = a[rows, j]
    return j, incl[rows, j] - aj, aj, AT


def ray_median(weights, z_vals, sigmas=None, return_index=False):
    """`sigmas`: the (N, S) sigmas of the pass where the launch is handed them (out->sigmas), else None.
    -> depth (N,) fp32 [, j (N,) int64: the crossing interval; -1 where the ray is bad or empty]"""
    w32, z32 = np.asarray(weights, np.float32), np.asarray(z_vals, np.float32)
    N, S = w32.shape
    assert z32.shape == (N, S) and 1 <= S <= MAX_SAMPLES and N >= 1
    bad = bad_rays(w32, z32, sigmas)
    a = masses(w32)
    a[bad] = 0                                                 # a bad ray's numbers are not used
    j, A, aj, AT = crossing(a)
    rows = np.arange(N)
    z = z32.astype(np.float64)
    last = z32[:, S - 1]
    inner = ~bad & (AT > 0) & (j < S - 1)
    ji = np.where(inner, j, 0)                                 # (a safe index for the rows that do not interpolate)
    num = (AT - 2 * A).astype(np.float64)
    den = np.where(inner, 2 * aj, 1).astype(np.float64)
    frac = num / den
    zj = z[rows, ji]
    with np.errstate(invalid="ignore", over="ignore"):         # (the rows that do not interpolate may hold anything)
        span = z[rows, np.minimum(ji + 1, S - 1)] - zj
        fs = frac * span
        depth = np.where(inner, (zj + fs).astype(np.float32), last).astype(np.float32)
    depth[bad] = np.float32(np.nan)
    if return_index:
        return depth, np.where(bad | (AT == 0), -1, j)
    return depth
