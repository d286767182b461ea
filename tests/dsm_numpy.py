"""Vectorised numpy restatement of the DSM path (tests only): plyflatten(radius, sigma = inf), the grids of create_dsm, and the
registration + altitude MAE of compute_mae (eval/utils/dsm.py, eval/utils/dsmr.py of the reference).  Written from the spec
in snerf_amd/eval/utils/dsm.py, array at a time; tests/test_dsm_cpu.py pins it to the reference's own output
(tests/golden/dsmr_*.npz), and the GPU tests compare the HIP kernels with it."""
import math

import numpy as np

from tests import reduce_numpy as RN


def bounds_grid(cloud, resolution=0.5):
    x, y = cloud[:, 0], cloud[:, 1]
    xoff = math.floor(x.min() / resolution) * resolution
    yoff = math.ceil(y.max() / resolution) * resolution
    xsize = int(1 + math.floor((x.max() - xoff) / resolution))
    ysize = int(1 - math.floor((y.min() - yoff) / resolution))
    return xoff, yoff, resolution, xsize, ysize


def rasterize(cloud, xoff, yoff, res, xsize, ysize, radius=1):
    """(mean, count) per cell in fp64; NaN where nothing arrived"""
    cloud = np.asarray(cloud, np.float64)
    i = np.floor((cloud[:, 0] - xoff) / res)
    j = np.floor((yoff - cloud[:, 1]) / res)
    z = cloud[:, 2]
    s = np.zeros(ysize * xsize)
    c = np.zeros(ysize * xsize, np.int64)
    for ky in range(-radius, radius + 1):
        for kx in range(-radius, radius + 1):
            ii, jj = i + kx, j + ky
            ok = (ii >= 0) & (ii < xsize) & (jj >= 0) & (jj < ysize)
            cell = (jj[ok] * xsize + ii[ok]).astype(np.int64)
            np.add.at(s, cell, z[ok])
            np.add.at(c, cell, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(c > 0, s / np.maximum(c, 1), np.nan)
    return mean.reshape(ysize, xsize), c.reshape(ysize, xsize)


def _shifted(v, dx, dy):
    """out[j, i] = v[j + dy, i + dx], NaN out of range"""
    h, w = v.shape
    out = np.full((h, w), np.nan, np.float64)
    j0, j1 = max(0, -dy), min(h, h - dy)
    i0, i1 = max(0, -dx), min(w, w - dx)
    if j0 < j1 and i0 < i1:
        out[j0:j1, i0:i1] = v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    return out


def downsample2x(u):
    """out[J, I] = NaN-aware mean of u[j:j+2, i:i+2] at j = min(2J+1, H-1), i = min(2I+1, W-1), summed in the order
    (i,j), (i,j+1), (i+1,j), (i+1,j+1)"""
    u = np.asarray(u, np.float64)
    h, w = u.shape
    J = np.minimum(2 * np.arange((h + 1) // 2) + 1, h - 1)
    I = np.minimum(2 * np.arange((w + 1) // 2) + 1, w - 1)
    pad = np.full((h + 1, w + 1), np.nan)
    pad[:h, :w] = u
    s = np.zeros((J.size, I.size))
    c = np.zeros((J.size, I.size))
    for k in range(2):
        for l in range(2):
            t = pad[np.ix_(J + l, I + k)]
            f = np.isfinite(t)
            s = s + np.where(f, t, 0.0)
            c = c + f
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, s / np.maximum(c, 1), np.nan)


def mean_std(u, v, dx, dy):
    u = np.asarray(u, np.float64)
    vs = _shifted(np.asarray(v, np.float64), dx, dy)
    m = np.isfinite(u) & np.isfinite(vs)
    n = int(m.sum())
    if n == 0:
        raise ValueError("The predicted DSM is all NaN")
    a, b = u[m], vs[m]
    muu, muv = a.sum() / n, b.sum() / n
    da, db = a - muu, b - muv
    return muu, muv, math.sqrt((da * da).sum() / n), math.sqrt((db * db).sum() / n), (da * db).sum() / n


def ncc(u, v, dx, dy):
    muu, muv, sigu, sigv, xcorr = mean_std(u, v, dx, dy)
    den = sigu * sigv
    return 0.0 if den == 0.0 else xcorr / den


def compute_ncc(u, v, irange, initdx, initdy):
    best, dx, dy = -math.inf, initdx, initdy
    for y in range(initdy - irange, initdy + irange + 1):
        for x in range(initdx - irange, initdx + irange + 1):
            c = ncc(u, v, x, y)
            if c > best:
                best, dx, dy = c, x, y
    return dx, dy


def recursive_ncc(u, v, irange=5, dx=0, dy=0, trace=None):
    """trace (list): (h, w, initdx, initdy, dx, dy) per level, coarse to fine"""
    h, w = np.shape(u)
    if min(h, w) > 100:
        dx, dy = recursive_ncc(downsample2x(u), downsample2x(v), irange, dx // 2, dy // 2, trace)
        dx, dy = 2 * dx, 2 * dy
    ix, iy = dx, dy
    dx, dy = compute_ncc(u, v, irange, dx, dy)
    if trace is not None:
        trace.append((h, w, ix, iy, dx, dy))
    return dx, dy


def compute_mae(pred, gt, mask=None, init=(0, 0)):
    """{"dx", "dy", "muu", "muv", "b", "rdsm", "diff", "mean", "median"}; registration on the raw gt, difference against
    the gt with values below -500 set to 0"""
    v = np.asarray(pred, np.float32).copy()
    if mask is not None:
        v[np.asarray(mask).astype(bool)] = np.nan
    gt = np.asarray(gt, np.float32)
    trace = []
    dx, dy = recursive_ncc(gt, v, 5, init[0], init[1], trace)
    muu, muv, _, _, _ = mean_std(gt, v, dx, dy)
    b = muu - muv
    rdsm = (_shifted(v.astype(np.float64), dx, dy) + b).astype(np.float32)
    g = np.where(gt < -500.0, np.float32(0.0), gt)
    diff = rdsm - g
    a = np.abs(diff[np.isfinite(diff)]).astype(np.float64)
    return {"dx": dx, "dy": dy, "trace": trace, "muu": muu, "muv": muv, "b": b, "rdsm": rdsm, "diff": diff,
            "mean": float(a.mean()), "median": float(np.median(a))}


def shift_diff_totals(pred, gt, dx, dy, b, threads=256, max_blocks=1024):
    """(sum |diff|, finite count) of snerf_dsm_shift_diff, bit for bit (csrc/dsm.hip shift_diff_kernel, diff_total_kernel):
    rv = f32(f64(pred[j + dy, i + dx]) + b), d = rv - g in fp32 with g = 0 where gt < -500; every thread adds |f64(d)| and 1 of
    its finite cells in ascending grid-stride order, the tree sums a workgroup, one thread sums the workgroups serially"""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    rv = (_shifted(pred.astype(np.float64), dx, dy) + np.float64(b)).astype(np.float32)
    d = rv - np.where(gt < np.float32(-500.0), np.float32(0.0), gt)
    ok = np.isfinite(d)
    grid = RN.blocks_for(d.size, threads, max_blocks)
    with np.errstate(invalid="ignore"):
        s = RN.tree(RN.grid_stride_sums(np.abs(d.astype(np.float64)), ok, grid, threads))
    c = RN.tree(RN.grid_stride_sums(np.ones(d.size), ok, grid, threads))
    return RN.serial_sum(s), RN.serial_sum(c)
