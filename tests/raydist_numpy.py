"""numpy restatement of snerf_ray_distortion (include/snerf_hip.h), operation for operation: the oracle of
tests/test_gpu_raydist.py and the object tests/test_raydist_cpu.py compares with the O(S^2) definition of the distortion loss.

Every operation is fp64 and rounded on its own (numpy never contracts) and every sum is over int64 integers -- so the result has no
summation order and every bit of it is fixed."""
import numpy as np

Q = float(2 ** 50)
ACC_SCALE = float(2 ** 40)
MAX_SAMPLES = 1024        # SNERF_VIS_MAX_SAMPLES
MAX_RAYS = 2 ** 22
NAN_BITS = 0x7FF8000000000000


def midpoints(z_vals, near, far):
    """-> (t, delta, m), each (N, S) fp64: t = (z - near) / (far - near), delta_i = t_{i+1} - t_i (0 for the last), m = t + 0.5 delta"""
    z = np.asarray(z_vals, np.float32).astype(np.float64)
    near = np.asarray(near, np.float32).astype(np.float64)[:, None]
    far = np.asarray(far, np.float32).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        t = (z - near) / (far - near)
        delta = np.zeros_like(t)
        delta[:, :-1] = t[:, 1:] - t[:, :-1]
        half = 0.5 * delta
        return t, delta, t + half


def bad_rays(weights, z_vals, near, far):
    """(N,) bool: a weight or depth that is not finite, a decreasing depth, near or far not finite, !(far > near), a t outside [-1, 2]"""
    w, z = np.asarray(weights, np.float32), np.asarray(z_vals, np.float32)
    near, far = np.asarray(near, np.float32), np.asarray(far, np.float32)
    t, _, _ = midpoints(z, near, far)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(w).all(1) | ~np.isfinite(z).all(1) | (z[:, 1:] < z[:, :-1]).any(1)
        bad |= ~np.isfinite(near) | ~np.isfinite(far) | ~(far > near)
        bad |= ~((t >= -1.0) & (t <= 2.0)).all(1)
    return bad


def clamp(weights):
    """w' = min(max((double)w, 0), 1), a zero of either sign giving +0"""
    w = np.asarray(weights, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0.0, np.minimum(w, 1.0), 0.0)


def ray_distortion(weights, z_vals, rays, return_g64=False):
    """-> (d_weights (N, S) fp32, per_ray (N,) fp64, acc (4,) uint64) of one call on a zeroed accumulator [, g (N, S) fp64: step 5's
    g_k before it is written as a float, with the same zeros]"""
    w32, z32 = np.asarray(weights, np.float32), np.asarray(z_vals, np.float32)
    rays = np.asarray(rays, np.float32)
    N, S = w32.shape
    assert z32.shape == (N, S) and rays.shape[0] == N and rays.shape[1] >= 8 and 1 <= S <= MAX_SAMPLES and 1 <= N <= MAX_RAYS
    near, far = rays[:, 6], rays[:, 7]
    bad = bad_rays(w32, z32, near, far)
    _, delta, m = midpoints(z32, near, far)
    wc = clamp(w32)
    wc[bad], m[bad], delta[bad] = 0.0, 0.0, 0.0                # a bad ray's numbers are not used: keep them out of rint
    a = np.rint(wc * Q).astype(np.int64)
    wm = wc * m
    b = np.rint(wm * Q).astype(np.int64)
    A = np.cumsum(a, 1, dtype=np.int64) - a                    # exclusive prefixes
    B = np.cumsum(b, 1, dtype=np.int64) - b
    AT, BT = a.sum(1, dtype=np.int64)[:, None], b.sum(1, dtype=np.int64)[:, None]
    Ab, Bb = A.astype(np.float64) / Q, B.astype(np.float64) / Q
    Ap, Bp = (AT - A - a).astype(np.float64) / Q, (BT - B - b).astype(np.float64) / Q
    mA = m * Ab
    x = mA - Bb
    wx = wc * x
    ww = wc * wc
    wwd = ww * delta
    third = wwd / 3.0
    e = 2.0 * wx + third
    q = np.rint(e * Q).astype(np.int64)
    with np.errstate(over="ignore"):
        L_int = q.sum(1, dtype=np.int64)                       # two's complement
    L_r = L_int.astype(np.float64) / Q
    mAp = m * Ap
    y = Bp - mAp
    xy = x + y
    c = (2.0 / 3.0) * wc
    cd = c * delta
    g64 = 2.0 * xy + cd
    with np.errstate(invalid="ignore"):
        g64[(w32 < 0) | (w32 > 1)] = 0.0
    g64[bad] = 0.0
    g = g64.astype(np.float32)
    per_ray = np.where(bad, np.float64(np.nan), L_r)
    word0 = sum(int(v) for v in np.rint(L_r[~bad] * ACC_SCALE).astype(np.int64)) % (1 << 64)
    acc = np.array([word0, N, int(bad.sum()), 0], np.uint64)
    return (g, per_ray, acc, g64) if return_g64 else (g, per_ray, acc)


def loss_chain(acc, lam):
    """the host's fp32 chain behind the launch (loss_ops.distortion_loss): -> (term fp32, scale fp32) from the summed words;
    term = (float)((lam * (acc0 * 2^-40)) / acc1), acc0 read as int64; scale = (float)(lam / acc1)"""
    acc = np.asarray(acc, np.uint64)
    a0 = np.float64(acc.view(np.int64)[0]) * (1.0 / ACC_SCALE)
    a1 = np.float64(acc.view(np.int64)[1])
    return np.float32((np.float64(lam) * a0) / a1), np.float32(np.float64(lam) / a1)
