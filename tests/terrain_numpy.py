"""The bare-earth terrain of include/snerf_terrain.h restated in numpy and plain Python: the oracle of tests/test_gpu_terrain.py, held
itself to scipy.ndimage and to a brute-force loop by tests/test_terrain_cpu.py.  Windows are plain clipped slices; the fill is four
literal walks per cell with Python ints and floats (IEEE doubles, one operation at a time: the kernel's bits).  The rasters of both
test files live here too."""
import math

import numpy as np

HOLE = -2 ** 31
NOT_A_KEY = 2 ** 31 - 1
FLAGGED, BLOCKED, IS_HOLE = 1, 2, 4
Z0, Q = 0.0, 2.0 ** -16

SHAPES = [(1, 1), (1, 130), (130, 1), (7, 65), (33, 64), (70, 129), (1, 300), (300, 1)]
HOLE_PATTERNS = ["none", "all", "one_valid", "hole_row_and_column", "edges", "random"]
GROUND_PATTERNS = ["none", "corner", "one_column", "row_ends", "alternating", "random"]


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def keys(alt, label=None, blocked=(), z0=Z0, q=Q):
    """-> (key int32, flags uint8, [finite but out of range, not finite, blocked])"""
    alt = np.asarray(alt, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        kq = np.rint((alt.astype(np.float64) - z0) / q)
    ok = (kq > -2.0 ** 31) & (kq < 2.0 ** 31 - 1)
    key = np.where(ok, np.where(ok, kq, 0.0).astype(np.int64), HOLE).astype(np.int32)
    flags = np.where(ok, 0, IS_HOLE).astype(np.uint8)
    n_blocked = 0
    if label is not None:
        is_blocked = np.isin(label, list(blocked))
        flags |= np.where(is_blocked, BLOCKED, 0).astype(np.uint8)
        n_blocked = int(is_blocked.sum())
    return key, flags, [int((~ok & np.isfinite(alt)).sum()), int((~np.isfinite(alt)).sum()), n_blocked]


# ---- the opening ----------------------------------------------------------------------------------------------------------------------
def valid(key):
    return (key != HOLE) & (key != NOT_A_KEY)


def _window(a, r, fold):
    """fold (np.min / np.max) over the (2 r + 1)^2 window clipped to the raster: the rectangle's extreme is the extreme over its rows
    of the extremes along them"""
    h, w = a.shape
    rows = np.stack([fold(a[:, max(0, i - r):i + r + 1], axis=1) for i in range(w)], axis=1)
    return np.stack([fold(rows[max(0, j - r):j + r + 1, :], axis=0) for j in range(h)], axis=0)


def erode(key, r):
    """-> int64 plane: the minimum of the valid keys in the window, 2^31 - 1 for "none" """
    return _window(np.where(valid(key), key.astype(np.int64), NOT_A_KEY), r, np.min)


def dilate(e, r):
    """the maximum of e over the window, ignoring "none" (2^31 - 1); -2^31 where the window holds nothing"""
    return _window(np.where(e == NOT_A_KEY, HOLE, e), r, np.max)


def open_level(key, r, threshold=0, flags=None):
    """snerf_terrain_open -> (key_out int32, flags uint8 or None, newly flagged)"""
    key = np.asarray(key, np.int32)
    ok = valid(key)
    o = dilate(erode(key, r), r)
    out = np.where(ok, o, HOLE).astype(np.int32)
    if flags is None:
        return out, None, 0
    hit = ok & (key.astype(np.int64) - out.astype(np.int64) > threshold)
    newly = hit & ((flags & FLAGGED) == 0)
    return out, (flags | np.where(hit, FLAGGED, 0).astype(np.uint8)), int(newly.sum())


def open_brute(key, r):
    """the opening cell by cell, straight from the header's words"""
    h, w = key.shape
    e = {}
    for j in range(h):
        for i in range(w):
            vals = [int(key[y, x]) for y in range(max(0, j - r), min(h, j + r + 1)) for x in range(max(0, i - r), min(w, i + r + 1))
                    if int(key[y, x]) not in (HOLE, NOT_A_KEY)]
            e[j, i] = min(vals) if vals else None
    out = np.full((h, w), HOLE, np.int32)
    for j in range(h):
        for i in range(w):
            if int(key[j, i]) in (HOLE, NOT_A_KEY):
                continue
            out[j, i] = max(e[y, x] for y in range(max(0, j - r), min(h, j + r + 1)) for x in range(max(0, i - r), min(w, i + r + 1))
                            if e[y, x] is not None)
    return out


def ground_flags(key, flags, radii, thresholds):
    """the level loop -> (flags, [newly flagged per level])"""
    src, per_level = key, []
    for r, t in zip(radii, thresholds):
        src, flags, n = open_level(src, r, t, flags)
        per_level.append(n)
    return flags, per_level


# ---- the fill -------------------------------------------------------------------------------------------------------------------------
def fill(key, flags, alt, z0=Z0, q=Q):
    """snerf_terrain_fill -> (dtm f32, ndsm f32, reach int32, [ground, filled, unreachable])"""
    h, w = key.shape
    alt = np.asarray(alt, np.float32)
    dtm, ndsm, reach = np.empty((h, w), np.float32), np.empty((h, w), np.float32), np.empty((h, w), np.int32)
    counts = [0, 0, 0]
    ground = flags == 0
    for j in range(h):
        for i in range(w):
            if ground[j, i]:
                dtm[j, i], ndsm[j, i], reach[j, i] = alt[j, i], 0.0, 0
                counts[0] += 1
                continue
            found = []
            for dj, di in ((0, -1), (0, 1), (-1, 0), (1, 0)):                 # W, E, N, S
                y, x, d = j + dj, i + di, 1
                while 0 <= y < h and 0 <= x < w and not ground[y, x]:
                    y, x, d = y + dj, x + di, d + 1
                if 0 <= y < h and 0 <= x < w:
                    found.append((d, int(key[y, x])))
            if not found:
                dtm[j, i] = ndsm[j, i] = np.nan
                reach[j, i] = -1
                counts[2] += 1
                continue
            b = min(k for _, k in found)
            num = den = 0.0
            for d, k in found:
                num += float(k - b) / float(d)
                den += 1.0 / float(d)
            t = z0 + q * (float(b) + num / den)
            a = float(alt[j, i])
            dtm[j, i] = np.float32(t)
            ndsm[j, i] = np.float32(a - t) if math.isfinite(a) else np.nan
            reach[j, i] = min(d for d, _ in found)
            counts[1] += 1
    return dtm, ndsm, reach, counts


def schedule(res, max_window_m=80.0, slope=0.15, dh0=0.3, dh_max=2.5, q=Q):
    r_max = max(1, math.ceil(max_window_m / res / 2))
    radii = [2 ** k for k in range(32) if 2 ** k < r_max] + [r_max]
    prev = [0] + radii[:-1]
    return radii, [int(np.rint(min(dh0 + slope * (r - p) * res, dh_max) / q)) for r, p in zip(radii, prev)]


def terrain(alt, res, label=None, blocked=(), **schedule_kw):
    radii, thresholds = schedule(res, **schedule_kw)
    key, flags, kstats = keys(alt, label, blocked)
    flags, per_level = ground_flags(key, flags, radii, thresholds)
    dtm, ndsm, reach, fstats = fill(key, flags, alt)
    return {"dtm": dtm, "ndsm": ndsm, "ground": flags == 0, "flags": flags, "reach": reach,
            "stats": {"out_of_range": kstats[0], "not_finite": kstats[1], "blocked": kstats[2], "flagged_per_level": per_level,
                      "ground": fstats[0], "filled": fstats[1], "unreachable": fstats[2]},
            "schedule": {"radii": radii, "thresholds": thresholds, "res": float(res)}}


# ---- the rasters ----------------------------------------------------------------------------------------------------------------------
def random_alt(h, w, seed=0):
    """altitudes in [-40, 60) m on multiples of 1/64 m: keys with both signs"""
    rng = np.random.default_rng(seed * 1000003 + h * 131 + w)
    return (np.round(rng.uniform(-40.0, 60.0, (h, w)) * 64) / 64).astype(np.float32)


def hole_mask(pattern, h, w):
    """True = a hole"""
    rng = np.random.default_rng(h * 977 + w)
    m = np.zeros((h, w), bool)
    if pattern == "all":
        m[:] = True
    elif pattern == "one_valid":
        m[:] = True
        m[h // 2, (2 * w) // 3] = False
    elif pattern == "hole_row_and_column":
        m[h // 3, :] = True
        m[:, w // 2] = True
    elif pattern == "edges":
        m[0, :] = m[-1, :] = True
        m[:, 0] = m[:, -1] = True
    elif pattern == "random":
        m = rng.random((h, w)) < 0.3
    elif pattern != "none":
        raise KeyError(pattern)
    return m


def key_raster(h, w, pattern):
    """an int32 key plane with the holes of `pattern`"""
    key, _, _ = keys(random_alt(h, w))
    return np.where(hole_mask(pattern, h, w), HOLE, key).astype(np.int32)


def ground_mask(pattern, h, w):
    """True = ground"""
    rng = np.random.default_rng(h * 31 + w * 7 + 5)
    g = np.zeros((h, w), bool)
    if pattern == "corner":
        g[-1, 0] = True
    elif pattern == "one_column":
        g[:, w // 3] = True
    elif pattern == "row_ends":
        g[:, 0] = g[:, -1] = True
    elif pattern == "alternating":
        jj, ii = np.mgrid[0:h, 0:w]
        g = (jj + ii) % 2 == 0
    elif pattern == "random":
        g = rng.random((h, w)) < 0.3
    elif pattern != "none":
        raise KeyError(pattern)
    return g


def fill_case(h, w, pattern):
    """-> (key, flags, alt): altitudes with a few holes (non-finite, out of range) that are never ground, every flag bit in use"""
    rng = np.random.default_rng(h * 13 + w)
    alt = random_alt(h, w, seed=2)
    flat = alt.reshape(-1)
    special = rng.permutation(h * w)
    for k, v in enumerate((np.nan, np.inf, 40000.0)):
        flat[special[k::17][:max(1, h * w // 40)]] = v
    key, flags, _ = keys(alt)
    g = ground_mask(pattern, h, w) & (flags == 0)
    other = np.array([FLAGGED, BLOCKED, FLAGGED | BLOCKED], np.uint8)[rng.integers(0, 3, (h, w))]
    flags = np.where(g, 0, np.where(flags != 0, flags | np.where(rng.random((h, w)) < 0.5, BLOCKED, 0).astype(np.uint8), other)).astype(np.uint8)
    return key, flags, alt


TOWN_SHAPE, TOWN_RES = (70, 129), 0.5
TOWN_SCHEDULE = dict(max_window_m=12.5, slope=0.3, dh0=0.3, dh_max=2.5)


def town(slope=0.0, shift=0):
    """70 x 129 cells at 0.5 m: the ground 10 + slope (x + y / 2) m (x east, y south, in metres) and 12 boxes of 4..19 cells a side
    with flat roofs 3..15 m (whole metres) above the highest ground under them, every box at least one cell off the raster's edge and
    at least two cells from the next.  `shift`: every box moved by that many columns.
    -> (alt f32, boxes [(j0, i0, rows, cols, roof altitude)], ground: the plane as float64, box mask)"""
    h, w = TOWN_SHAPE
    rng = np.random.default_rng(2019)
    jj, ii = np.mgrid[0:h, 0:w]
    ground = 10.0 + slope * (ii * TOWN_RES + 0.5 * jj * TOWN_RES)
    taken = np.zeros((h, w), bool)
    boxes = []
    while len(boxes) < 12:
        nj, ni = (int(v) for v in rng.integers(4, 20, 2))
        j0, i0 = int(rng.integers(1, h - nj)), int(rng.integers(2, w - ni - 2))
        if taken[max(0, j0 - 2):j0 + nj + 2, max(0, i0 - 2):i0 + ni + 2].any():
            continue
        taken[j0:j0 + nj, i0:i0 + ni] = True
        boxes.append((j0, i0, nj, ni, int(rng.integers(3, 16))))
    boxes.sort()
    alt = ground.copy()
    mask = np.zeros((h, w), bool)
    out = []
    for j0, i0, nj, ni, up in boxes:
        i0 += shift
        roof = float(ground[j0:j0 + nj, i0:i0 + ni].max()) + up
        alt[j0:j0 + nj, i0:i0 + ni] = roof
        mask[j0:j0 + nj, i0:i0 + ni] = True
        out.append((j0, i0, nj, ni, roof))
    return alt.astype(np.float32), out, ground, mask
