"""The roof planes of include/snerf_roofs.h restated in numpy and plain Python: the oracle of tests/test_gpu_roofs.py, held itself to
numpy.linalg.lstsq and scipy.ndimage.label by tests/test_roofs_cpu.py.  Windows are literal loops over the offsets (window_sums: one
cell, Python ints; window_sum_planes: the same sums for all cells at once, held to the former), the cofactors, determinants and moment
sums are Python ints (which cannot overflow, so the header's bounds are asserted rather than relied on) and the fp64 tails are Python
floats, one IEEE operation at a time in the header's order: the kernels' bits.  The rasters of both test files live here too."""
import math

import numpy as np

HOLE = -2 ** 31
NOT_A_KEY = 2 ** 31 - 1
MAX_RADIUS = 4
FLAT, STEEP, CODE_HOLE, DEGENERATE, NONE = 0, 9, 253, 254, 255
MOMENT_INIT = (0, 0, 0, 0, 0, 0, 0, 0, 0, 2 ** 64 - 1, 0, 2 ** 64 - 1, 0, 0, 0, 0)
RESIDUAL_INIT = (0, 0, 0, 0, 2 ** 64 - 1, 0, 0, 0)
DK_LIMIT, RQ_LIMIT, UNIT = 2 ** 24, 2 ** 18, 64.0
Z0, Q = 0.0, 2.0 ** -16
M64 = 2 ** 64 - 1

SHAPES = [(1, 1), (1, 130), (130, 1), (3, 3), (7, 65), (33, 64), (70, 129)]
HOLE_PATTERNS = ["none", "all", "one_valid", "hole_row_and_column", "edges", "random"]
ID_PATTERNS = ["none", "one_object", "checkerboard", "two_rectangles", "blobs"]


def valid(k):
    return k != HOLE and k != NOT_A_KEY


def tan2(deg):
    t = math.tan(math.radians(deg))
    return t * t


# ---- normals --------------------------------------------------------------------------------------------------------------------------
def window_sums(key, ids, j, i, r):
    """the nine int sums of cell (j, i)'s support: n, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd"""
    h, w = key.shape
    kc, idc = int(key[j, i]), int(ids[j, i])
    s = [0] * 9
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            y, x = j + dj, i + di
            if not (0 <= y < h and 0 <= x < w) or int(ids[y, x]) != idc or not valid(int(key[y, x])):
                continue
            d = int(key[y, x]) - kc
            for n, v in enumerate((1, di, dj, di * di, di * dj, dj * dj, d, di * d, dj * d)):
                s[n] += v
    return s


def window_sum_planes(key, ids, r):
    """window_sums for every cell at once: the loop over the window's offsets is literal, the cells go through numpy in int64 (nine
    sums of at most 81 terms below 2^34: no overflow) -> (9, h, w) int64.  Only the planes of object cells with a valid key are used."""
    h, w = key.shape
    ok = (key != HOLE) & (key != NOT_A_KEY)
    k = key.astype(np.int64)
    kp, okp = np.pad(k, r), np.pad(ok, r)
    idp = np.pad(ids.astype(np.int64), r, constant_values=-1)
    S = np.zeros((9, h, w), np.int64)
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            at = (slice(r + dj, r + dj + h), slice(r + di, r + di + w))
            same = (idp[at] == ids) & okp[at]
            d = np.where(same, kp[at] - k, 0)
            for n, v in enumerate((1, di, dj, di * di, di * dj, dj * dj)):
                S[n] += same * v
            S[6] += d
            S[7] += di * d
            S[8] += dj * d
    return S


def cramer(s):
    """-> (D, Nx, Ny) from the nine sums, with the header's bounds asserted"""
    n, sx, sy, sxx, sxy, syy, sd, sxd, syd = s
    c00, c01, c02 = sxx * syy - sxy * sxy, sxy * sy - sx * syy, sx * sxy - sxx * sy
    c11, c12, c22 = n * syy - sy * sy, sx * sy - n * sxy, n * sxx - sx * sx
    D = n * c00 + sx * c01 + sy * c02
    Nx, Ny = c01 * sd + c11 * sxd + c12 * syd, c02 * sd + c12 * sxd + c22 * syd
    assert all(abs(c) < 2 ** 20 for c in (c00, c01, c02, c11, c12, c22)) and abs(sd) < 2 ** 39 and 0 <= D < 2 ** 29
    assert abs(Nx) < 2 ** 60 and abs(Ny) < 2 ** 60
    return D, Nx, Ny


def classify(a, b, cos0, sin0, tan2_flat, tan2_wall):
    ar, br = (a * cos0) + (b * sin0), (b * cos0) - (a * sin0)
    ar2, br2 = ar * ar, br * br
    s2 = ar2 + br2
    m = abs(ar) + abs(br)
    m2 = m * m
    if s2 <= tan2_flat:
        return FLAT
    if s2 > tan2_wall:
        return STEEP
    if m2 < 2.0 * ar2:
        return 7 if ar > 0.0 else 3
    if m2 < 2.0 * br2:
        return 1 if br > 0.0 else 5
    if ar > 0.0:
        return 8 if br > 0.0 else 6
    return 2 if br > 0.0 else 4


def normals(key, ids, K, radius, q, res, cos0=1.0, sin0=0.0, tan2_flat=tan2(5.0), tan2_wall=tan2(60.0)):
    """snerf_roofs_normals -> (slope_e f32, slope_n f32, code u8, tag int32, [object cells, with a normal, degenerate, hole])"""
    assert 1 <= radius <= MAX_RADIUS
    h, w = key.shape
    se, sn = np.full((h, w), np.nan, np.float32), np.full((h, w), np.nan, np.float32)
    code, tag = np.full((h, w), NONE, np.uint8), np.full((h, w), -1, np.int32)
    stats = [0, 0, 0, 0]
    ids = np.where((ids < 0) | (ids > K), 0, ids)
    f = q / res
    sums = window_sum_planes(key, ids, radius)
    for j in range(h):
        for i in range(w):
            if int(ids[j, i]) <= 0:
                continue
            stats[0] += 1
            if not valid(int(key[j, i])):
                code[j, i] = CODE_HOLE
                stats[3] += 1
                continue
            D, Nx, Ny = cramer([int(v) for v in sums[:, j, i]])
            if D <= 0:
                code[j, i] = DEGENERATE
                stats[2] += 1
                continue
            a, b = (float(Nx) / float(D)) * f, (float(Ny) / float(D)) * f
            c = classify(a, b, cos0, sin0, tan2_flat, tan2_wall)
            se[j, i], sn[j, i], code[j, i] = np.float32(a), np.float32(-b), c
            stats[1] += 1
            if c <= 8:
                tag[j, i] = int(ids[j, i]) * 16 + c
    return se, sn, code, tag, stats


# ---- link -----------------------------------------------------------------------------------------------------------------------------
def link(tag, connectivity=4):
    """snerf_roofs_link by a sequential union-find -> (parent (h * w) int32, [0, member cells])"""
    h, w = tag.shape
    parent = np.where(tag.reshape(-1) >= 0, np.arange(h * w), -1).astype(np.int64)

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    steps = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    for j in range(h):
        for i in range(w):
            if tag[j, i] < 0:
                continue
            for dj, di in steps:
                y, x = j + dj, i + di
                if 0 <= y < h and 0 <= x < w and tag[y, x] == tag[j, i]:
                    unite(j * w + i, y * w + x)
    for c in range(h * w):
        if parent[c] >= 0:
            parent[c] = find(c)
    return parent.astype(np.int32), [0, int((tag >= 0).sum())]


def ids_from_parent(parent, h, w):
    """objects.ids_from_parent: roots numbered 1.. in raster order -> (ids (h, w) int32, count)"""
    parent = parent.reshape(-1)
    is_root = parent == np.arange(parent.size)
    rank = np.cumsum(is_root).astype(np.int32)
    ids = np.where(parent < 0, 0, rank[np.clip(parent, 0, None)])
    return ids.reshape(h, w).astype(np.int32), int(rank[-1]) if parent.size else 0


# ---- moments and residuals --------------------------------------------------------------------------------------------------------------
def _cell(fids, root, key, j, i, F):
    """-> None (no facet), "bad", or (fid, di, dj, dk, keyed, k)"""
    h, w = fids.shape
    fid = int(fids[j, i])
    if fid < 0 or fid > F:
        return "bad"
    if fid == 0:
        return None
    rt = int(root[j, i])
    if rt < 0 or rt >= h * w:
        return "bad"
    j0, i0 = divmod(rt, w)
    k, k0 = int(key[j, i]), int(key.reshape(-1)[rt])
    return fid, i - i0, j - j0, k - k0, valid(k) and valid(k0), k


def words(rows):
    """a list of rows of Python ints -> (n, words) uint64, signed sums in two's complement"""
    return np.array([[v & M64 for v in row] for row in rows], np.uint64).reshape(len(rows), -1 if len(rows) else 0)


def moments(fids, root, key, tag, F, band=None, rows=None):
    """snerf_roofs_moments -> (rows: F lists of 16 Python ints (signed sums as they are), [folded, left out, bad])"""
    h, w = fids.shape
    root = root.reshape(h, w)
    rows = [list(MOMENT_INIT) for _ in range(F)] if rows is None else rows
    stats = [0, 0, 0]
    row0, row1 = (0, h) if band is None else band
    if F == 0:
        return rows, stats
    for j in range(row0, row1):
        for i in range(w):
            c = _cell(fids, root, key, j, i, F)
            if c is None:
                continue
            if c == "bad":
                stats[2] += 1
                continue
            fid, di, dj, dk, keyed, _ = c
            r = rows[fid - 1]
            r[13] = max(r[13], max(int(tag[j, i]), 0))
            r[14] = max(r[14], int(root[j, i]))
            if not keyed or abs(dk) >= DK_LIMIT:
                r[15] += 1
                stats[1] += 1
                continue
            stats[0] += 1
            for n, v in enumerate((1, di, dj, dk, di * di, di * dj, dj * dj, di * dk, dj * dk)):
                r[n] += v
            r[9], r[10], r[11], r[12] = min(r[9], i), max(r[10], i), min(r[11], j), max(r[12], j)
            assert all(abs(v) < 2 ** 63 for v in r[:9])
    return rows, stats


def solve(row):
    """the plane of one facet from its moment words (Python ints): -> (gamma, alpha, beta) predicting dk in key units, NaNs when
    the facet is empty or its cells are collinear (D == 0).  Central moments exactly; one fp64 division per slope."""
    n, sx, sy, sk, sxx, sxy, syy, sxk, syk = (int(v) for v in row[:9])
    nan = (math.nan, math.nan, math.nan)
    if n <= 0:
        return nan
    cxx, cxy, cyy = n * sxx - sx * sx, n * sxy - sx * sy, n * syy - sy * sy
    cxk, cyk = n * sxk - sx * sk, n * syk - sy * sk
    D = cxx * cyy - cxy * cxy
    if D == 0:
        return nan
    alpha, beta = (cxk * cyy - cyk * cxy) / D, (cyk * cxx - cxk * cxy) / D
    gamma = ((float(sk) - alpha * float(sx)) - beta * float(sy)) / float(n)
    return gamma, alpha, beta


def residuals(fids, root, key, F, planes, q=Q, unit=UNIT, band=None, rows=None, residual=None):
    """snerf_roofs_residuals -> (residual f32, rows: F lists of 8 Python ints, [with, without, bad])"""
    h, w = fids.shape
    root = root.reshape(h, w)
    rows = [list(RESIDUAL_INIT) for _ in range(F)] if rows is None else rows
    out = np.full((h, w), np.nan, np.float32) if residual is None else residual
    stats = [0, 0, 0]
    row0, row1 = (0, h) if band is None else band
    for j in range(row0, row1):
        for i in range(w):
            out[j, i] = np.nan
            c = _cell(fids, root, key, j, i, F)
            if c is None:
                continue
            if c == "bad":
                stats[2] += 1
                continue
            fid, di, dj, dk, keyed, k = c
            gamma, alpha, beta = (float(v) for v in planes[fid - 1])
            if not (keyed and math.isfinite(gamma) and math.isfinite(alpha) and math.isfinite(beta)):
                stats[1] += 1
                continue
            with np.errstate(all="ignore"):
                pred = np.float64(gamma) + (np.float64(alpha) * np.float64(di))
                pred = pred + (np.float64(beta) * np.float64(dj))
                e = np.float64(dk) - pred
                out[j, i] = np.float32(np.float64(q) * e)
                t = np.rint(e / np.float64(unit))
            clamped = 0
            if not t < 262144.0:
                rq, clamped = RQ_LIMIT, 1
            elif t < -262144.0:
                rq, clamped = -RQ_LIMIT, 1
            else:
                rq = int(t)
            r = rows[fid - 1]
            r[0] += 1
            r[1] += abs(rq)
            r[2] += rq * rq
            r[3] = max(r[3], abs(rq))
            r[4], r[5] = min(r[4], k + 2 ** 31), max(r[5], k + 2 ** 31)
            r[6] += clamped
            stats[0] += 1
    return out, rows, stats


def roofs(key, ids, K, res, radius=1, flat_deg=5.0, wall_deg=60.0, aspect0_deg=0.0, connectivity=4, q=Q, unit=UNIT):
    """the whole chain on the key plane, before any facet is filtered"""
    a0 = math.radians(aspect0_deg)
    se, sn, code, tag, nstats = normals(key, ids, K, radius, q, res, math.cos(a0), math.sin(a0), tan2(flat_deg), tan2(wall_deg))
    parent, lstats = link(tag, connectivity)
    fids, F = ids_from_parent(parent, *key.shape)
    mrows, mstats = moments(fids, parent, key, tag, F)
    planes = np.array([solve(r) for r in mrows], np.float64).reshape(F, 3)
    residual, rrows, rstats = residuals(fids, parent, key, F, planes, q, unit)
    return {"slope_e": se, "slope_n": sn, "code": code, "tag": tag, "parent": parent, "fids": fids, "F": F, "moments": mrows,
            "planes": planes, "residual": residual, "residual_rows": rrows,
            "stats": {"normals": nstats, "link": lstats, "moments": mstats, "residuals": rstats}}


# ---- the rasters ----------------------------------------------------------------------------------------------------------------------
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


def key_raster(h, w, pattern, seed=0):
    """an int32 key plane: four quadrants with a plane of their own each (one of them level) under a noise of +-5 mm, keys of both
    signs, every fifth hole of the pattern stored as 2^31 - 1"""
    rng = np.random.default_rng(seed * 1000003 + h * 131 + w)
    jj, ii = np.mgrid[0:h, 0:w]
    quadrant = 2 * (jj >= (h + 1) // 2) + (ii >= (w + 1) // 2)
    gx, gy = np.array([9000, -20000, 0, 15000])[quadrant], np.array([-14000, 3000, 0, 15000])[quadrant]
    k = (-65536 + gx * ii + gy * jj + rng.integers(-300, 300, (h, w))).astype(np.int64)
    holes = hole_mask(pattern, h, w)
    k = np.where(holes, HOLE, k)
    flat = k.reshape(-1)
    at = np.flatnonzero(holes.reshape(-1))[::5]
    flat[at] = NOT_A_KEY
    return k.astype(np.int32)


def id_raster(h, w, pattern):
    """-> (ids int32, K); the random blobs carry a few ids outside [0, K], which are read as 0"""
    rng = np.random.default_rng(h * 53 + w * 3 + 1)
    jj, ii = np.mgrid[0:h, 0:w]
    if pattern == "none":
        return np.zeros((h, w), np.int32), 0
    if pattern == "one_object":
        return np.ones((h, w), np.int32), 1
    if pattern == "checkerboard":
        return (1 + (jj + ii) % 2).astype(np.int32), 2
    if pattern == "two_rectangles":
        ids = np.zeros((h, w), np.int32)
        ids[h // 5:h - h // 5, w // 6:w // 2] = 1
        ids[h // 3:h, w // 2:w - w // 7] = 2
        return ids, 2
    if pattern == "blobs":
        coarse = rng.integers(0, 6, ((h + 4) // 5, (w + 6) // 7))
        ids = np.kron(coarse, np.ones((5, 7), np.int64))[:h, :w].astype(np.int32)
        ids[rng.random((h, w)) < 0.01] = 9
        ids[rng.random((h, w)) < 0.01] = -3
        return ids, 5
    raise KeyError(pattern)


TOWN_SHAPE, TOWN_RES = (48, 64), 0.5
TOWN_BASE, TOWN_STEP = 10 * 65536, 16384


def town():
    """the 48 x 64 town of DESIGN.md section 5z at res 0.5 m, q = 2^-16 m: the ground at 10 m and five buildings whose roofs rise by
    0.25 m per cell (tan = 0.5) -> (key int32, ids int32, K = 5, alt f32: the keys' altitudes, exact in fp32)"""
    h, w = TOWN_SHAPE
    key = np.full((h, w), TOWN_BASE, np.int64)
    ids = np.zeros((h, w), np.int32)
    jj, ii = np.mgrid[0:h, 0:w]

    def put(n, rows, cols, up):
        box = (jj >= rows[0]) & (jj <= rows[1]) & (ii >= cols[0]) & (ii <= cols[1])
        ids[box] = n
        key[box] = (TOWN_BASE + up * TOWN_STEP)[box] if isinstance(up, np.ndarray) else TOWN_BASE + up * TOWN_STEP

    put(1, (4, 13), (4, 15), 0)                                                            # flat
    put(2, (4, 19), (22, 37), np.minimum(ii - 22, 37 - ii))                                # gabled
    put(3, (24, 43), (4, 23), np.minimum(np.minimum(jj - 24, 43 - jj), np.minimum(ii - 4, 23 - ii)))    # hipped
    put(4, (26, 39), (30, 43), jj - 26)                                                    # shed
    put(5, (24, 43), (48, 59), np.where(ii >= 54, 24, 0))                                  # two levels, 6 m apart
    key = key.astype(np.int32)
    return key, ids, 5, (Z0 + Q * key.astype(np.float64)).astype(np.float32)
