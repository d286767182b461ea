"""NumPy restatement of the cast-shadow entries (tests only), written from include/snerf_hip.h: the Amanatides-Woo march over a
height field in fp64, vectorised over the cells with a Python loop over the march steps, and the integer words of the agreement.
The kernel uses only fp64 + - * / and comparisons, one rounding per operation, so every array here is held to the kernels BIT FOR
BIT by tests/test_gpu_shadow.py (numpy evaluates `h0 + rise * t` as two ufunc calls: no contraction); tests/test_shadow_cpu.py
holds cast() to an independent brute-force formulation."""
import numpy as np

UNKNOWN = 255


def sun_rows(suns, res):
    """(elevation_deg, azimuth_deg) pairs -> (K, 3) fp64 rows (ux, uy, rise) = (sin az, -cos az, tan el * res)"""
    el, az = np.deg2rad(np.asarray(suns, np.float64).reshape(-1, 2)).T
    return np.stack([np.sin(az), -np.cos(az), np.tan(el) * float(res)], 1)


def cast_one(dsm, row, bias=0.0, z_top=np.inf, want_margins=False):
    """one sun: (lit (h, w) u8, dist (h, w) f32[, margins]) -- margins: per cell the smallest |dsm - hr| over the cells its march
    tested and the smallest |tMaxX - tMaxY| over its steps (inf where nothing was tested), what the brute-force comparison needs"""
    dsm = np.asarray(dsm, np.float32)
    h, w = dsm.shape
    d64 = dsm.astype(np.float64)
    ux, uy, rise = (np.float64(v) for v in row)
    bias, z_top = np.float64(bias), np.float64(z_top)
    stepx, stepy = (1 if ux > 0 else -1), (1 if uy > 0 else -1)
    inf = np.float64(np.inf)
    tdx = inf if ux == 0 else np.float64(1.0) / abs(ux)
    tdy = inf if uy == 0 else np.float64(1.0) / abs(uy)
    j, i = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:h, 0:w])
    n = h * w
    start = d64.reshape(-1)
    h0 = start + bias
    tmx, tmy = np.full(n, np.float64(0.5) * tdx), np.full(n, np.float64(0.5) * tdy)
    lit = np.where(np.isnan(start), UNKNOWN, 1).astype(np.uint8)
    dist = np.full(n, np.nan, np.float32)
    margin_h, margin_t = np.full(n, np.inf), np.full(n, np.inf)
    active = ~np.isnan(start)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(h + w + 2):
            a = np.nonzero(active)[0]
            if not a.size:
                break
            margin_t[a] = np.minimum(margin_t[a], np.abs(tmx[a] - tmy[a]))
            takex = tmx[a] <= tmy[a]
            t = np.where(takex, tmx[a], tmy[a])
            i[a] += np.where(takex, stepx, 0)
            j[a] += np.where(takex, 0, stepy)
            tmx[a] = np.where(takex, tmx[a] + tdx, tmx[a])
            tmy[a] = np.where(takex, tmy[a], tmy[a] + tdy)
            inside = (i[a] >= 0) & (i[a] < w) & (j[a] >= 0) & (j[a] < h)
            hr = h0[a] + rise * t
            go = inside & ~(hr > z_top)
            cell = np.full(a.size, np.nan)
            cell[go] = d64[j[a][go], i[a][go]]
            blocked = cell > hr                                                 # False where not inside / above z_top / NaN cell
            margin_h[a[go]] = np.fmin(margin_h[a[go]], np.abs(cell[go] - hr[go]))
            lit[a[blocked]] = 0
            dist[a[blocked]] = t[blocked].astype(np.float32)
            active[a[~go | blocked]] = False
    assert not active.any()                                                     # at most h + w + 2 steps
    out = (lit.reshape(h, w), dist.reshape(h, w))
    return out + ((margin_h.reshape(h, w), margin_t.reshape(h, w)),) if want_margins else out


def cast(dsm, rows, bias=0.0, z_top=np.inf):
    """snerf_shadow_cast: -> (lit (K, h, w) u8, dist (K, h, w) f32)"""
    res = [cast_one(dsm, r, bias, z_top) for r in np.asarray(rows, np.float64).reshape(-1, 3)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def agreement(sun, lit, valid=None, threshold=0.5, acc=None):
    """snerf_shadow_agreement: sun (K, cells) f32, lit (K, cells) u8, valid (cells) u8 or None -> acc (K, 8) uint64 (added to
    `acc` when given); the sums of words 5 / 6 wrap as int64 sums do"""
    sun, lit = np.asarray(sun, np.float32), np.asarray(lit, np.uint8)
    K = sun.shape[0]
    sun, lit = sun.reshape(K, -1), lit.reshape(K, -1)
    out = np.zeros((K, 8), np.uint64) if acc is None else np.array(acc, np.uint64).reshape(K, 8)
    ok = np.ones(sun.shape[1], bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    for k in range(K):
        counted = (lit[k] <= 1) & ok & np.isfinite(sun[k])
        s = sun[k][counted].astype(np.float64)
        on = lit[k][counted] == 1
        pred = s >= np.float64(threshold)
        q = np.rint(np.clip(s * 16777216.0, -2.0 ** 62, 2.0 ** 62)).astype(np.int64)
        words = [np.sum(on & pred), np.sum(on & ~pred), np.sum(~on & pred), np.sum(~on & ~pred), np.sum(~counted)]
        sums = [int(np.sum(q[on].astype(object))), int(np.sum(q[~on].astype(object)))]         # Python ints, then wrapped
        for c, v in enumerate([int(v) for v in words] + sums):
            out[k, c] = np.uint64((int(out[k, c]) + v) % 2 ** 64)
    return out


def metrics(words):
    """the host-side figures of one sun's 8 words (eval/utils/shadow.py derives the same): an empty denominator gives NaN"""
    w = [int(v) for v in words]
    s5, s6 = ((v - 2 ** 64 if v >= 2 ** 63 else v) for v in w[5:7])
    div = lambda a, b: a / b if b else float("nan")      # noqa: E731
    n = sum(w[:4])
    return {"n": n, "left_out": w[4], "accuracy": div(w[0] + w[3], n), "iou_shadow": div(w[3], w[1] + w[2] + w[3]),
            "mean_sun_lit": div(s5 / 2.0 ** 24, w[0] + w[1]), "mean_sun_shadow": div(s6 / 2.0 ** 24, w[2] + w[3])}
