"""Restatement of snerf_dsm_segment_hit (tests only), written from include/snerf_raycast.h step by step, and an independent dense
oracle.

segment_hits -- the spec's steps 1 to 4 per segment in Python floats: IEEE fp64 + - * / with one rounding each, math.floor,
comparisons and integers, which is all the kernel uses, so every output of the kernel equals it BIT FOR BIT.

dense_oracle -- shares nothing with the walk: it samples each segment at K equal steps (K = 64 per cell of |dx| + |dy|, plus 64)
and answers with the first sample whose altitude is <= the height of the cell the sample lies in.

random_heights / random_segments -- the seeded window and segments both test files use; depth_of -- the host half of
eval/utils/raycast.py cast_rays (the depth from s)."""
import math

import numpy as np

TOP, WALL, START, END, OUTSIDE, BAD = range(6)
HIT_STATES = (TOP, WALL, START)


def _clip_axis(c0, dc, size, t0, t1):
    """one axis of step 3's slabs: (misses, t0, t1)"""
    if dc == 0.0:
        return not (c0 >= 0.0 and c0 < size), t0, t1
    ta, tb = (0.0 - c0) / dc, (size - c0) / dc
    lo, hi = (ta, tb) if ta < tb else (tb, ta)
    if lo > t0:
        t0 = lo
    if hi < t1:
        t1 = hi
    return False, t0, t1


def _entry_cell(c, size):
    f = math.floor(c)
    return 0 if f < 0 else (size - 1 if f > size - 1 else int(f))


def segment_hit(p0, p1, grid, dsm, bias=0.0):
    """one segment: (s, state, cell).  grid = (xoff, yoff, res, ioff, joff, out_w, out_h); dsm (out_h, out_w) float32"""
    xoff, yoff, res, ioff, joff, w, h = grid
    xoff, yoff, res, ioff, joff, bias = float(xoff), float(yoff), float(res), float(ioff), float(joff), float(bias)
    e0, n0, a0 = (float(v) for v in p0)
    e1, n1, a1 = (float(v) for v in p1)
    if not all(math.isfinite(v) for v in (e0, n0, a0, e1, n1, a1)):
        return math.nan, BAD, -1
    W, H = float(w), float(h)
    x0, y0 = (e0 - xoff) / res - ioff, (yoff - n0) / res - joff
    x1, y1 = (e1 - xoff) / res - ioff, (yoff - n1) / res - joff
    dx, dy, da = x1 - x0, y1 - y0, a1 - a0
    if x0 >= 0.0 and x0 < W and y0 >= 0.0 and y0 < H:
        s_a, i, j = 0.0, int(math.floor(x0)), int(math.floor(y0))
    else:
        miss, t0, t1 = _clip_axis(x0, dx, W, 0.0, 1.0)
        if miss:
            return math.nan, OUTSIDE, -1
        miss, t0, t1 = _clip_axis(y0, dy, H, t0, t1)
        if miss or t0 > t1:
            return math.nan, OUTSIDE, -1
        s_a = t0
        i, j = _entry_cell(x0 + dx * t0, w), _entry_cell(y0 + dy * t0, h)
    stepx, stepy = (1 if dx > 0.0 else -1), (1 if dy > 0.0 else -1)
    aheadx, aheady = (1 if dx > 0.0 else 0), (1 if dy > 0.0 else 0)
    first = True
    for _ in range(w + h + 2):
        s_x = math.inf if dx == 0.0 else (float(i + aheadx) - x0) / dx
        s_y = math.inf if dy == 0.0 else (float(j + aheady) - y0) / dy
        x_steps = s_x <= s_y
        s_next = s_x if x_steps else s_y
        s_b = s_next if s_next < 1.0 else 1.0
        if s_b < s_a:
            s_b = s_a
        hc = float(dsm[j, i]) + bias
        if a0 + da * s_a <= hc:
            return s_a, (START if first else WALL), j * w + i
        if a0 + da * s_b <= hc:
            t = (hc - a0) / da
            return (s_a if t < s_a else (s_b if t > s_b else t)), TOP, j * w + i
        if s_next >= 1.0:
            return math.nan, END, -1
        if x_steps:
            i += stepx
        else:
            j += stepy
        if i < 0 or i >= w or j < 0 or j >= h:
            return math.nan, OUTSIDE, -1
        s_a = s_b
        first = False
    return math.nan, OUTSIDE, -1


def segment_hits(p0, p1, grid, dsm, bias=0.0):
    """(s (n) f64, state (n) u8, cell (n) i32) of the (n, 3) end points"""
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 3), np.asarray(p1, np.float64).reshape(-1, 3)
    dsm = np.asarray(dsm, np.float32).reshape(grid[6], grid[5])
    n = len(p0)
    s, state, cell = np.empty(n, np.float64), np.empty(n, np.uint8), np.empty(n, np.int32)
    for r in range(n):
        s[r], state[r], cell[r] = segment_hit(p0[r], p1[r], grid, dsm, bias)
    return s, state, cell


def dense_oracle(p0, p1, grid, dsm, bias=0.0):
    """per segment: (s of the first sample at or under the surface (NaN: none), the sample step 1 / K)"""
    xoff, yoff, res, ioff, joff, w, h = grid
    p0, p1 = np.asarray(p0, np.float64).reshape(-1, 3), np.asarray(p1, np.float64).reshape(-1, 3)
    height = np.asarray(dsm, np.float32).reshape(h, w).astype(np.float64) + bias
    hit, step = np.full(len(p0), np.nan), np.empty(len(p0))
    for r, (a, b) in enumerate(zip(p0, p1)):
        x = (np.array([a[0], b[0]]) - xoff) / res - ioff
        y = (yoff - np.array([a[1], b[1]])) / res - joff
        K = 64 * int(math.ceil(abs(x[1] - x[0]) + abs(y[1] - y[0]))) + 64
        step[r] = 1.0 / K
        s = np.arange(K + 1, dtype=np.float64) / K
        xs, ys, alt = x[0] + (x[1] - x[0]) * s, y[0] + (y[1] - y[0]) * s, a[2] + (b[2] - a[2]) * s
        ci, cj = np.floor(xs), np.floor(ys)
        inside = (ci >= 0) & (ci < w) & (cj >= 0) & (cj < h)
        under = np.zeros(K + 1, bool)
        under[inside] = alt[inside] <= height[cj[inside].astype(np.int64), ci[inside].astype(np.int64)]      # False for NaN
        k = np.nonzero(under)[0]
        if k.size:
            hit[r] = s[k[0]]
    return hit, step


# ---- the random case both test files use -----------------------------------------------------------------------------------------
GRID = (1000.0, 2000.0, 0.5, 3, 2, 23, 17)      # a 23 x 17 window at cell (3, 2) of a 40 x 30 lattice of 0.5 m
LATTICE = (40, 30)
SEED = 7            # see tests/test_raycast_cpu.py test_the_restatement_against_the_dense_oracle on how it was chosen
N_RANDOM = 2000


def random_heights(seed=SEED):
    """(17, 23) float32: multiples of 0.25 m in [0, 6], two NaN cells, one +inf and one -inf cell"""
    rng = np.random.default_rng(seed)
    w, h = GRID[5], GRID[6]
    dsm = (rng.integers(0, 25, (h, w)) * 0.25).astype(np.float32)
    dsm[4, 7] = dsm[11, 15] = np.nan
    dsm[8, 3] = np.inf
    dsm[13, 19] = -np.inf
    return dsm


def random_segments(n=N_RANDOM, seed=SEED):
    """(p0, p1), each (n, 3) fp64 in the frame of GRID: end points inside and outside the window, over, in and under the heights; an
    eighth of the segments each vertical, horizontal (da == 0) and along a cell boundary (x or y constant on an integer)"""
    rng = np.random.default_rng(seed + 1)
    xoff, yoff, res, ioff, joff, w, h = GRID

    def points():
        x = rng.uniform(-4.0, w + 4.0, n)                     # window cell coordinates
        y = rng.uniform(-4.0, h + 4.0, n)
        return x, y, rng.uniform(-1.0, 9.0, n)
    x0, y0, a0 = points()
    x1, y1, a1 = points()
    kind = rng.integers(0, 8, n)
    vertical, level, edge_x, edge_y = kind == 0, kind == 1, kind == 2, kind == 3
    x0[vertical], y0[vertical] = rng.uniform(0.0, w, vertical.sum()), rng.uniform(0.0, h, vertical.sum())
    x1[vertical], y1[vertical] = x0[vertical], y0[vertical]
    a1[level] = a0[level]
    x0[edge_x] = x1[edge_x] = rng.integers(0, w + 1, edge_x.sum()).astype(np.float64)
    y0[edge_y] = y1[edge_y] = rng.integers(0, h + 1, edge_y.sum()).astype(np.float64)

    def world(x, y, a):
        return np.stack([xoff + (x + ioff) * res, yoff - (y + joff) * res, a], 1)
    return world(x0, y0, a0), world(x1, y1, a1)


def depth_of(s, state, near, far):
    """cast_rays' depth: near + s (far - near) in fp64 from the fp32 columns, rounded once to fp32; NaN unless TOP, WALL or START"""
    near, far = np.asarray(near, np.float32).astype(np.float64), np.asarray(far, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = near + np.asarray(s, np.float64) * (far - near)
    return np.where(np.isin(state, HIT_STATES), d, np.nan).astype(np.float32)
