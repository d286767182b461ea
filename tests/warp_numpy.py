"""The raster warp of include/snerf_warp.h (csrc/warp.hip) restated in numpy: the oracle of
tests/test_gpu_warp.py, itself held to closed forms, scipy and brute-force counts by tests/test_warp_cpu.py.  A helper, not a test module.

Two restatements of the same rules.  `planes_cell` / `labels_cell` are the header's text, one destination cell at a time in Python
floats (IEEE fp64, one operation per expression).  `warp_planes` / `warp_labels` run the same operations in the same order for
every destination cell at once: the loops run over the tap slots (rows outer, columns inner), a cell whose tap is skipped keeps its
accumulators untouched.  tests/test_warp_cpu.py holds the two to each other bit for bit."""
import math
from collections import namedtuple

import numpy as np

NEAREST, BILINEAR, AVERAGE, MIN, MAX, MODE = range(6)
MAX_STEP = 64
MAX_PLANES = 16
NO_LABEL = 255
FLOAT_METHODS = (NEAREST, BILINEAR, AVERAGE, MIN, MAX)
LABEL_METHODS = (NEAREST, MODE)
NAN32 = np.array([0x7fc00000], np.uint32).view(np.float32)[0]

Map = namedtuple("Map", "off_x step_x off_y step_y src_w src_h dst_w dst_h")


# ---- one cell at a time: the header's text ------------------------------------------------------------------------------------------------
def axis_taps_cell(off, step, i, method):
    """[(k, weight)] of destination cell i on one axis, skipped taps left out"""
    off, step = float(off), float(step)
    a = off + float(i) * step
    b = off + (float(i) + 1.0) * step
    c = off + (float(i) + 0.5) * step
    if method == NEAREST:
        taps = [(math.floor(c), 1.0)]
    elif method == BILINEAR:
        t = c - 0.5
        k0 = math.floor(t)
        f = t - float(k0)
        taps = [(k0, 1.0 - f), (k0 + 1, f)]
    else:
        taps = [(k, min(float(k) + 1.0, b) - max(float(k), a)) for k in range(math.floor(a), math.ceil(b))]
    return [(k, w) for k, w in taps if w > 0.0]


def planes_cell(src, m, method, min_valid, i, j):
    """(value as np.float32, any tap outside the source) of destination cell (row j, column i) of one (src_h, src_w) float32 plane"""
    tot, num, den = 0.0, -0.0, 0.0
    best, outside = None, False
    for ky, wy in axis_taps_cell(m.off_y, m.step_y, j, method):
        for kx, wx in axis_taps_cell(m.off_x, m.step_x, i, method):
            w = wy * wx
            tot += w
            if not (0 <= ky < m.src_h and 0 <= kx < m.src_w):
                outside = True
                continue
            v = src[ky, kx]
            if not np.isfinite(v):
                continue
            den += w
            if method == MIN:
                best = v if best is None or v < best else best
            elif method == MAX:
                best = v if best is None or v > best else best
            elif method == NEAREST:
                best = v
            else:
                num += w * float(v)
    if method == NEAREST:
        return (NAN32 if best is None else best), outside
    if den > 0.0 and den >= float(min_valid) * tot:
        return (best if method in (MIN, MAX) else np.float32(num / den)), outside
    return NAN32, outside


def axis_members_cell(off, step, i):
    off, step = float(off), float(step)
    a = off + float(i) * step
    b = off + (float(i) + 1.0) * step
    c = off + (float(i) + 0.5) * step
    lo, hi = math.ceil(a - 0.5), math.ceil(b - 0.5)
    return list(range(lo, hi)) if hi > lo else [math.floor(c)]


def labels_cell(src, m, method, i, j):
    """(class, any tap or member outside the source) of destination cell (row j, column i) of a (src_h, src_w) uint8 plane"""
    if method == NEAREST:
        (kx, _), = axis_taps_cell(m.off_x, m.step_x, i, NEAREST)
        (ky, _), = axis_taps_cell(m.off_y, m.step_y, j, NEAREST)
        inside = 0 <= ky < m.src_h and 0 <= kx < m.src_w
        return (int(src[ky, kx]) if inside else NO_LABEL), not inside
    votes, outside = [0] * 256, False
    for ky in axis_members_cell(m.off_y, m.step_y, j):
        for kx in axis_members_cell(m.off_x, m.step_x, i):
            if 0 <= ky < m.src_h and 0 <= kx < m.src_w:
                if src[ky, kx] != NO_LABEL:
                    votes[int(src[ky, kx])] += 1
            else:
                outside = True
    most = max(votes)
    return (votes.index(most) if most > 0 else NO_LABEL), outside


def planes_by_cells(src, m, method, min_valid=0.5):
    """warp_planes through planes_cell: (dst (planes, dst_h, dst_w) float32, stats [3])"""
    src = np.asarray(src, np.float32).reshape(-1, m.src_h, m.src_w)
    dst = np.empty((src.shape[0], m.dst_h, m.dst_w), np.float32)
    outside = 0
    for j in range(m.dst_h):
        for i in range(m.dst_w):
            for p in range(src.shape[0]):
                dst[p, j, i], out = planes_cell(src[p], m, method, min_valid, i, j)
            outside += int(out)
    holes = int(np.isnan(dst).sum())
    return dst, [dst.size - holes, holes, outside]


def labels_by_cells(src, m, method):
    src = np.asarray(src, np.uint8).reshape(m.src_h, m.src_w)
    dst = np.empty((m.dst_h, m.dst_w), np.uint8)
    outside = 0
    for j in range(m.dst_h):
        for i in range(m.dst_w):
            dst[j, i], out = labels_cell(src, m, method, i, j)
            outside += int(out)
    holes = int((dst == NO_LABEL).sum())
    return dst, [dst.size - holes, holes, outside]


# ---- every cell at once -------------------------------------------------------------------------------------------------------------------
def axis_taps(off, step, n, method):
    """(k0 (n,) int64, slots, weight(s) -> (n,) float64 with 0 for a slot a cell does not have) of the n destination cells of an axis"""
    i = np.arange(n, dtype=np.float64)
    off, step = np.float64(off), np.float64(step)
    a = off + i * step
    b = off + (i + 1.0) * step
    c = off + (i + 0.5) * step
    if method == NEAREST:
        return np.floor(c).astype(np.int64), 1, lambda s: np.ones(n)
    if method == BILINEAR:
        t = c - 0.5
        k = np.floor(t)
        f = t - k
        return k.astype(np.int64), 2, lambda s: (1.0 - f) if s == 0 else f
    k0 = np.floor(a).astype(np.int64)
    count = np.ceil(b).astype(np.int64) - k0

    def weight(s):
        k = (k0 + s).astype(np.float64)
        return np.where(s < count, np.minimum(k + 1.0, b) - np.maximum(k, a), 0.0)
    return k0, int(count.max()), weight


def warp_planes(src, m, method, min_valid=0.5, out64=False):
    """snerf_warp_planes: src (planes, src_h, src_w) or (src_h, src_w) float32 -> (dst (planes, dst_h, dst_w) float32, stats [3]).
    `out64`: the values before their last rounding, num / den in float64 -- what the closed-form properties of tests/test_warp_cpu.py
    are held to (the rounding to float32 alone is 6e-8 relative)"""
    src = np.asarray(src, np.float32).reshape(-1, m.src_h, m.src_w)
    planes = src.shape[0]
    kx0, nx, weight_x = axis_taps(m.off_x, m.step_x, m.dst_w, method)
    ky0, ny, weight_y = axis_taps(m.off_y, m.step_y, m.dst_h, method)
    shape = (planes, m.dst_h, m.dst_w)
    tot, den = np.zeros(shape), np.zeros(shape)
    num = np.full(shape, -0.0)
    best = np.zeros(shape, np.float32)
    seen = np.zeros(shape, bool)
    outside = np.zeros(shape[1:], bool)
    for sy, sx in ((sy, sx) for sy in range(ny) for sx in range(nx)):
        wy = weight_y(sy)
        ky = ky0 + sy
        row_in = (ky >= 0) & (ky < m.src_h)
        with np.errstate(invalid="ignore", over="ignore"):           # a hole's w * v is computed and dropped
            wx = weight_x(sx)
            kx = kx0 + sx
            col_in = (kx >= 0) & (kx < m.src_w)
            taken = (wy > 0.0)[:, None] & (wx > 0.0)[None, :]
            w = wy[:, None] * wx[None, :]
            tot = np.where(taken, tot + w, tot)
            inside = row_in[:, None] & col_in[None, :]
            outside |= taken & ~inside
            v = src[:, np.clip(ky, 0, m.src_h - 1)[:, None], np.clip(kx, 0, m.src_w - 1)[None, :]]
            valid = (taken & inside)[None] & np.isfinite(v)
            den = np.where(valid, den + w, den)
            if method == MIN:
                best = np.where(valid & (~seen | (v < best)), v, best)
            elif method == MAX:
                best = np.where(valid & (~seen | (v > best)), v, best)
            elif method == NEAREST:
                best = np.where(valid, v, best)
            else:
                num = np.where(valid, num + w * v.astype(np.float64), num)
            seen |= valid
    if method == NEAREST:
        dst = np.where(seen, best, NAN32)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            value = best if method in (MIN, MAX) else (num / den) if out64 else (num / den).astype(np.float32)
        dst = np.where((den > 0.0) & (den >= np.float64(min_valid) * tot), value, np.nan if out64 else NAN32)
    dst = np.ascontiguousarray(dst, np.float64 if out64 else np.float32)
    holes = int(np.isnan(dst).sum())
    return dst, [dst.size - holes, holes, int(outside.sum())]


def axis_members(off, step, n):
    i = np.arange(n, dtype=np.float64)
    off, step = np.float64(off), np.float64(step)
    a = off + i * step
    b = off + (i + 1.0) * step
    c = off + (i + 0.5) * step
    lo, hi = np.ceil(a - 0.5).astype(np.int64), np.ceil(b - 0.5).astype(np.int64)
    some = hi > lo
    return np.where(some, lo, np.floor(c).astype(np.int64)), np.where(some, hi - lo, 1)


def warp_labels(src, m, method):
    """snerf_warp_labels: src (src_h, src_w) uint8 -> (dst (dst_h, dst_w) uint8, stats [3])"""
    src = np.asarray(src, np.uint8).reshape(m.src_h, m.src_w)
    if method == NEAREST:
        kx, _, _ = axis_taps(m.off_x, m.step_x, m.dst_w, NEAREST)
        ky, _, _ = axis_taps(m.off_y, m.step_y, m.dst_h, NEAREST)
        inside = ((ky >= 0) & (ky < m.src_h))[:, None] & ((kx >= 0) & (kx < m.src_w))[None, :]
        dst = np.where(inside, src[np.clip(ky, 0, m.src_h - 1)[:, None], np.clip(kx, 0, m.src_w - 1)[None, :]], NO_LABEL).astype(np.uint8)
        holes = int((dst == NO_LABEL).sum())
        return dst, [dst.size - holes, holes, int((~inside).sum())]
    kx0, nx = axis_members(m.off_x, m.step_x, m.dst_w)
    ky0, ny = axis_members(m.off_y, m.step_y, m.dst_h)
    votes = np.zeros((m.dst_h, m.dst_w, 256), np.int64)
    outside = np.zeros((m.dst_h, m.dst_w), bool)
    jj, ii = np.mgrid[0:m.dst_h, 0:m.dst_w]
    for sy in range(int(np.max(ny))):
        ky = ky0 + sy
        for sx in range(int(np.max(nx))):
            kx = kx0 + sx
            member = ((sy < ny) & np.ones(m.dst_h, bool))[:, None] & ((sx < nx) & np.ones(m.dst_w, bool))[None, :]
            inside = ((ky >= 0) & (ky < m.src_h))[:, None] & ((kx >= 0) & (kx < m.src_w))[None, :]
            outside |= member & ~inside
            c = src[np.clip(ky, 0, m.src_h - 1)[:, None], np.clip(kx, 0, m.src_w - 1)[None, :]]
            vote = member & inside & (c != NO_LABEL)
            np.add.at(votes, (jj[vote], ii[vote], c[vote].astype(np.int64)), 1)
    winner = votes.argmax(axis=2)                          # the first maximum: the lowest class on a tie
    dst = np.where(votes.max(axis=2) > 0, winner, NO_LABEL).astype(np.uint8)
    holes = int((dst == NO_LABEL).sum())
    return dst, [dst.size - holes, holes, int(outside.sum())]


# ---- rasters the tests share ----------------------------------------------------------------------------------------------------------------
HOLE_PATTERNS = ("none", "random", "band", "all")


def float_raster(h, w, pattern="none", planes=1, seed=0, infs=False):
    """(planes, h, w) float32 altitudes of |v| <= 100 with holes: none, 20 % at random, a NaN band across the middle, all holes; `infs`
    plants +inf and -inf"""
    rng = np.random.default_rng(1000 * seed + 31 * h + w)
    a = rng.uniform(-100.0, 100.0, (planes, h, w)).astype(np.float32)
    if pattern == "random":
        a[rng.random((planes, h, w)) < 0.2] = np.nan
    elif pattern == "band":
        a[:, h // 3:h // 3 + max(1, h // 4), :] = np.nan
        a[:, :, w // 2:w // 2 + max(1, w // 8)] = np.nan
    elif pattern == "all":
        a[:] = np.nan
    if infs:
        flat = a.reshape(planes, -1)
        flat[:, ::7] = np.inf
        flat[:, 3::11] = -np.inf
    return a


def label_raster(h, w, seed=0):
    """(h, w) uint8: blocks of the classes 0 ... 5 and 254 a few cells wide (so that majorities tie) with 255 as holes, at random
    and as a band"""
    rng = np.random.default_rng(77 * seed + 13 * h + w)
    classes = np.array([0, 1, 2, 3, 4, 5, 254], np.uint8)
    coarse = classes[rng.integers(0, len(classes), ((h + 1) // 2, (w + 2) // 3))]
    a = np.repeat(np.repeat(coarse, 2, axis=0), 3, axis=1)[:h, :w].copy()
    a[rng.random((h, w)) < 0.15] = NO_LABEL
    a[h // 2:h // 2 + max(1, h // 6), :] = NO_LABEL
    return a
