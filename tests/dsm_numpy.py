"""Vectorised numpy restatement of the DSM path (tests only): plyflatten(radius, sigma = inf), the grids of create_dsm, and the
registration + altitude MAE of compute_mae (eval/utils/dsm.py, eval/utils/dsmr.py of the reference).  Written from the spec
in snerf_amd/eval/utils/dsm.py, array at a time; tests/test_dsm_cpu.py pins it to the reference's own output
(tests/golden/dsmr_*.npz), and the GPU tests compare the HIP kernels with it.  The last section holds the references of the
registration's (S, 6) table: correctly rounded sums, the summation order of pass 0, and the derived bound of pass 1
(tests/test_gpu_dsm_stats.py, tests/test_dsm_stats_cpu.py)."""
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


# ---- the (S, 6) table of snerf_dsm_ncc_search, statistic by statistic -------------------------------------------------------------
EPS = 2.0 ** -53      # unit roundoff of fp64
NCC_TILE = 32         # csrc/dsm.hip
_UP = 1.0 + 2.0 ** -40   # a plain sum of non-negative terms is low by at most ~log2(n) eps of itself: rounded up, it is a bound


def _two_sum(a, b):
    """a + b = s + e exactly (Knuth), element-wise"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker's product on Veltkamp's splitting: no fused multiply-add), element-wise, away from
    overflow and underflow"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _centred(x, n):
    """(fsum(x), hi, lo): x - mean = hi + lo element-wise, about the exact mean.  fsum(x) / n is off the exact mean by up to
    eps |mean|; the differences from it are split exactly, and their plain sum gives the remainder to ~eps sigma, which moves
    a centred sum by n (eps sigma)^2: nothing."""
    sx = math.fsum(x)
    hi, lo = _two_sum(x, np.float64(-(sx / n)))
    return sx, hi, lo - (hi.sum() + lo.sum()) / n


def _centred_sum(ah, al, bh, bl):
    """(sum (ah + al)(bh + bl), sum of the magnitudes): the hi hi products are split exactly and summed by fsum; what lies
    below them (eps of a product each) is summed plainly, an error of order eps^2"""
    p, e = _two_prod(ah, bh)
    small = float((e + (ah * bl + al * bh) + al * bl).sum())
    return math.fsum(np.append(p, small)), float(np.abs((ah + al) * (bh + bl)).sum()) * _UP


def shift_stats(u, v, cx, cy, r, exact=True):
    """((S, 6) table, (S, 5) magnitudes) of the window centre (cx, cy) +- r, y outer and x inner as compute_ncc.  Table: the
    integer count of the pairs u[j, i], v[j + y, i + x] that are both finite, sum u and sum v over them, and the centred
    sums u'u', v'v', u'v' about the exact means; every sum is math.fsum's (correctly rounded; the centred terms are formed
    error-free first, so these three are right to a few eps^2 of their magnitude).  Magnitudes: sum |u|, sum |v|,
    sum |u'u'|, sum |v'v'|, sum |u'v'|, each an upper bound (_UP).  A row without a pair is zeros.
    exact=False: the table by mean_std's plain fp64 sums (ten times faster; for a margin between correlations, not for a bar)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    S1 = 2 * r + 1
    table, mags = np.zeros((S1 * S1, 6)), np.zeros((S1 * S1, 5))
    for s in range(S1 * S1):
        vs = _shifted(v, cx - r + s % S1, cy - r + s // S1)
        m = np.isfinite(u) & np.isfinite(vs)
        n = int(m.sum())
        if n == 0:
            continue
        a, b = u[m], vs[m]
        if not exact:
            su, sv = a.sum(), b.sum()
            da, db = a - su / n, b - sv / n
            table[s] = n, su, sv, (da * da).sum(), (db * db).sum(), (da * db).sum()
            mags[s] = np.array([np.abs(a).sum(), np.abs(b).sum(), table[s, 3], table[s, 4], np.abs(da * db).sum()]) * _UP
            continue
        su, ah, al = _centred(a, n)
        sv, bh, bl = _centred(b, n)
        (suu, muu), (svv, mvv), (suv, muv) = _centred_sum(ah, al, ah, al), _centred_sum(bh, bl, bh, bl), _centred_sum(ah, al, bh, bl)
        table[s] = n, su, sv, suu, svv, suv
        mags[s] = float(np.abs(a).sum()) * _UP, float(np.abs(b).sum()) * _UP, muu, mvv, muv
    return table, mags


def ncc_tiles(u, v, cx, cy, r):
    """what the workgroups of ncc_tile_kernel stage, for every shift at once: U (tiles, 1024) and V (S, tiles, 1024) in fp64, the
    tiles in ascending blockIdx.y * gridDim.x + blockIdx.x, a tile's cells row-major, NaN outside the image"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    h, w = u.shape
    T = NCC_TILE
    ty, tx = -(-h // T), -(-w // T)

    def tiles(a):
        p = np.full((ty * T, tx * T), np.nan)
        p[:h, :w] = a
        return p.reshape(ty, T, tx, T).transpose(0, 2, 1, 3).reshape(ty * tx, T * T)

    S1 = 2 * r + 1
    return tiles(u), np.stack([tiles(_shifted(v, cx - r + s % S1, cy - r + s // S1)) for s in range(S1 * S1)])


def serial_tile_sums(terms, ok):
    """per (..., tile): the serial sum from 0.0 of terms[..., c] over a tile's cells c in ascending (row-major) order where ok"""
    a = np.zeros(terms.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(terms.shape[-1]):
            a = np.where(ok[..., c], a + terms[..., c], a)
    return a


def reduce_tiles(partial):
    """ncc_reduce_kernel: (S, tiles) per-tile partials -> (S,), reduce_numpy.strided_sum over the tiles of every shift"""
    return np.array([RN.strided_sum(p) for p in partial])


def shift_stats_pass0(u, v, cx, cy, r):
    """(S, 3): columns 0 to 2 of snerf_dsm_ncc_search's table, bit for bit.  Pass 0 is made of additions only: per 32 x 32 tile
    and shift a serial sum from 0.0 in row-major order over the pairs that are both finite (cells outside the image count as
    NaN), then block_strided_sum<256> over the tiles in ascending blockIdx.y * gridDim.x + blockIdx.x (csrc/dsm.hip
    ncc_tile_kernel pass 0, ncc_reduce_kernel)."""
    U, V = ncc_tiles(u, v, cx, cy, r)
    ok = np.isfinite(U)[None] & np.isfinite(V)
    cnt = ok.sum(-1).astype(np.float64)
    su = serial_tile_sums(np.broadcast_to(U[None], V.shape), ok)
    sv = serial_tile_sums(V, ok)
    return np.stack([reduce_tiles(cnt), reduce_tiles(su), reduce_tiles(sv)], 1)


def mean_delta(n, sabs, mu):
    """how far the kernel's mean fl(S / n), S its pass-0 sum of n values with sum |x| = sabs, can lie from the exact mean mu
    (centred_bound)"""
    return ((n - 1) * EPS * sabs / n) * (1.0 + EPS) + EPS * abs(mu)


def centred_bound(n, M, du, dv):
    """Bound on |kernel - exact| for one of columns 3 to 5 (sum a'b' over n pairs; a = b in columns 3 and 4), derived, not
    measured.  csrc/dsm.hip is compiled with contraction on, so pass 1 may or may not fuse du * dv into the accumulation: its
    columns get this bound, valid either way, where pass 0 (additions only) gets a restatement.  eps = 2^-53.

    The mean.  The kernel's sum S of n values x is some order of n - 1 fp64 additions, |S - sum x| <= (n - 1) eps sum|x| to
    first order, and its mean m = fl(S / n) adds one rounding, so with mu the exact mean
        |m - mu| <= delta = ((n - 1) eps sum|x| / n)(1 + eps) + eps |mu|                                  (mean_delta).
    Centring about m instead of mu.  sum (a - m_a)(b - m_b) = sum a'b' + n (mu_a - m_a)(mu_b - m_b) exactly (the cross terms
    vanish: sum a' = sum b' = 0): the kernel's own means add n delta_a delta_b at most.
    Rounding.  Each factor fl(x - m) carries one rounding, the product one (none when fused), the accumulation of n terms in any
    order -- serial in a tile, strided and tree over the tiles -- n - 1: (n + 2) eps M to first order, M = sum |a'b'|.  Two
    more eps M take the second-order terms and the difference between M about m and about mu, of order
    n eps (delta_b sum|a'| + delta_a sum|b'|): far below eps M at any size and offset a DSM has.  Hence
        |got - exact| <= (n + 4) eps M + n delta_a delta_b."""
    return (n + 4) * EPS * M + n * du * dv


def ncc_of_row(row):
    """the correlation of one table row, as eval/utils/dsm.py _ncc takes it (a row with pairs)"""
    n, _, _, suu, svv, suv = row
    den = math.sqrt(suu / n) * math.sqrt(svv / n)
    return 0.0 if den == 0.0 else (suv / n) / den


def ncc_error(row, b):
    """how far the correlation of a row can move when its columns 3 to 5 move by b = (b_uu, b_vv, b_uv): the largest numerator
    over the smallest denominator, less the value itself, plus 8 eps for the handful of roundings of the formula; inf when a
    variance could reach 0"""
    n, _, _, suu, svv, suv = row
    if suu <= b[0] or svv <= b[1]:
        return math.inf
    return (abs(suv) + b[2]) / math.sqrt((suu - b[0]) * (svv - b[1])) - abs(suv) / math.sqrt(suu * svv) + 8 * EPS


def stats_bounds(table, mags):
    """(S, 3): centred_bound of columns 3 to 5 from shift_stats' two arrays; 0 on a row without a pair"""
    out = np.zeros((table.shape[0], 3))
    for s, (row, mg) in enumerate(zip(table, mags)):
        n = int(row[0])
        if n:
            da, db = mean_delta(n, mg[0], row[1] / n), mean_delta(n, mg[1], row[2] / n)
            out[s] = centred_bound(n, mg[2], da, da), centred_bound(n, mg[3], db, db), centred_bound(n, mg[4], da, db)
    return out
