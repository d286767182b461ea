"""NumPy restatement of the solar entries (tests only), written from include/snerf_solar.h: the horizon's Amanatides-Woo march in fp64,
vectorised over the cells with a Python loop over the march steps (as tests/shadow_numpy.py cast_one), the sky-view factor and the sun
table against the horizon planes.  The kernels use only fp64 + - * / and comparisons, one rounding per operation, so every array here
is held to the kernels BIT FOR BIT by tests/test_gpu_solar.py (numpy evaluates each operator as a ufunc of its own: no contraction);
tests/test_solar_cpu.py holds horizon_one() to an independent brute-force formulation and to the restated cast shadows."""
import numpy as np

MAX_DIRS, MAX_SECTORS, MAX_SUNS = 64, 720, 64


def horizon_one(dsm, row, bias=0.0, max_dist=np.inf, want_margins=False):
    """one direction (ux, uy): the (h, w) f32 plane[, the smallest |tMaxX - tMaxY| over each cell's steps].  There is no z_top: it is
    only an early exit of the kernel."""
    dsm = np.asarray(dsm, np.float32)
    h, w = dsm.shape
    d64 = dsm.astype(np.float64)
    ux, uy = (np.float64(v) for v in row)
    bias, max_dist = np.float64(bias), np.float64(max_dist)
    stepx, stepy = (1 if ux > 0 else -1), (1 if uy > 0 else -1)
    inf = np.float64(np.inf)
    tdx = inf if ux == 0 else np.float64(1.0) / abs(ux)
    tdy = inf if uy == 0 else np.float64(1.0) / abs(uy)
    j, i = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:h, 0:w])
    n = h * w
    start = d64.reshape(-1)
    h0 = start + bias
    tmx, tmy = np.full(n, np.float64(0.5) * tdx), np.full(n, np.float64(0.5) * tdy)
    best = np.full(n, -inf)
    margin_t = np.full(n, np.inf)
    active = ~np.isnan(start)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
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
            go = (i[a] >= 0) & (i[a] < w) & (j[a] >= 0) & (j[a] < h) & ~(t > max_dist)
            g = a[go]
            sl = (d64[j[g], i[g]] - h0[g]) / t[go]
            better = sl > best[g]                                               # False for a NaN cell
            best[g[better]] = sl[better]
            active[a[~go]] = False
    assert not active.any()                                                     # at most h + w + 2 steps
    out = np.where(np.isnan(start), np.nan, best).astype(np.float32).reshape(h, w)
    return (out, margin_t.reshape(h, w)) if want_margins else out


def horizon(dsm, rows, bias=0.0, max_dist=np.inf):
    """snerf_solar_horizon: -> (n_dirs, h, w) f32"""
    return np.stack([horizon_one(dsm, r, bias, max_dist) for r in np.asarray(rows, np.float64).reshape(-1, 2)])


def svf(hor, res):
    """snerf_solar_svf: (n_dirs, h, w) f32 -> (h, w) f32"""
    hor = np.asarray(hor, np.float32)
    res = np.float64(res)
    acc = np.zeros(hor.shape[1:], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(hor.shape[0]):
            T = hor[d].astype(np.float64) / res
            T = np.where(T > 0.0, T, 0.0)
            acc = acc + 1.0 / (1.0 + T * T)
        out = (acc / np.float64(hor.shape[0])).astype(np.float32)
    out[np.isnan(hor[0])] = np.nan
    return out


def irradiate(hor, table, slope_e=None, slope_n=None, direct=None, count=None):
    """snerf_solar_irradiate over a table of ANY length (the accumulators run on, as over the kernel's calls of at most 64 rows):
    -> (direct (h, w) f64, count (h, w) u32), continued from `direct` / `count` when given"""
    hor = np.asarray(hor, np.float32)
    n_dirs, shape = hor.shape[0], hor.shape[1:]
    H = hor.astype(np.float64)
    hole = np.isnan(hor[0])
    gx = np.zeros(shape) if slope_e is None else np.asarray(slope_e, np.float32).astype(np.float64)
    gy = np.zeros(shape) if slope_n is None else np.asarray(slope_n, np.float32).astype(np.float64)
    a = np.zeros(shape) if direct is None else np.array(direct, np.float64)
    n = np.zeros(shape, np.uint32) if count is None else np.array(count, np.uint32)
    table = np.asarray(table, np.float64).reshape(-1, 7)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, len(table), MAX_SUNS):                               # one call: NaN is written at its end
            for sector, frac, rise, east, north, up, weight in table[k0:k0 + MAX_SUNS]:
                s = int(sector)
                Hk = H[s] if frac == 0.0 else ((1.0 - frac) * H[s]) + (frac * H[(s + 1) % n_dirs])
                lit = (rise >= Hk) & ~hole
                c = (up - (gx * east)) - (gy * north)
                a = np.where(hole, a, a + np.where(lit & (c > 0.0), c * weight, 0.0))
                n = n + lit.astype(np.uint32)
            a = np.where(hole | np.isnan(gx) | np.isnan(gy), np.nan, a)
    return a, n
