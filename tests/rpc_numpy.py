"""fp64 numpy restatement of rpcm's RPCModel (rpcm/rpc_model.py): the polynomial, the rational function, the projection and
the localisation (inverse model when the dict carries one, else the iterative inversion).  rpcm is not installed here; this
module is the stand-in for it in tools/gen_golden_scene.py (which runs the reference's loaders on top of it) and the CPU
oracle of tests/test_scene_cpu.py and tests/test_gpu_scene.py.

As rpcm, `localization_iterative` updates EVERY point of the call until the last one has met the tolerance, and raises
MaxLocalizationIterationsError when the points are still above it after 101 updates (the loop tests `n > 100` at its
top).  The device kernels do the same per call: one launch counts the updates, the next runs every point that many
(DESIGN.md §5g).  `geodetic_to_ecef` is an independent statement of the WGS84 geodetic -> ECEF conversion, for the CPU
oracle of the rays."""
import numpy as np


class MaxLocalizationIterationsError(Exception):
    pass


def apply_poly(poly, x, y, z):
    """RPC00B term order with x = lat (P), y = lon (L), z = alt (H)"""
    out = 0
    out += poly[0]
    out += poly[1] * y + poly[2] * x + poly[3] * z
    out += poly[4] * y * x + poly[5] * y * z + poly[6] * x * z
    out += poly[7] * y * y + poly[8] * x * x + poly[9] * z * z
    out += poly[10] * x * y * z
    out += poly[11] * y * y * y
    out += poly[12] * y * x * x + poly[13] * y * z * z + poly[14] * y * y * x
    out += poly[15] * x * x * x
    out += poly[16] * x * z * z + poly[17] * y * y * z + poly[18] * x * x * z
    out += poly[19] * z * z * z
    return out


def apply_rfm(num, den, x, y, z):
    return apply_poly(num, x, y, z) / apply_poly(den, x, y, z)


class RPCModel:
    def __init__(self, d, dict_format="rpcm"):
        if dict_format != "rpcm":
            raise ValueError("only the rpcm dict layout is restated")
        self.__dict__ = dict(d)

    def projection(self, lon, lat, alt):
        nlon = (np.asarray(lon) - self.lon_offset) / self.lon_scale
        nlat = (np.asarray(lat) - self.lat_offset) / self.lat_scale
        nalt = (np.asarray(alt) - self.alt_offset) / self.alt_scale
        col = apply_rfm(self.col_num, self.col_den, nlat, nlon, nalt)
        row = apply_rfm(self.row_num, self.row_den, nlat, nlon, nalt)
        col = col * self.col_scale + self.col_offset
        row = row * self.row_scale + self.row_offset
        return col, row

    def localization(self, col, row, alt, return_normalized=False):
        ncol = (np.asarray(col) - self.col_offset) / self.col_scale
        nrow = (np.asarray(row) - self.row_offset) / self.row_scale
        nalt = (np.asarray(alt) - self.alt_offset) / self.alt_scale
        if not hasattr(self, "lat_num"):
            lon, lat = self.localization_iterative(ncol, nrow, nalt)
        else:
            lon = apply_rfm(self.lon_num, self.lon_den, nrow, ncol, nalt)
            lat = apply_rfm(self.lat_num, self.lat_den, nrow, ncol, nalt)
        if not return_normalized:
            lon = lon * self.lon_scale + self.lon_offset
            lat = lat * self.lat_scale + self.lat_offset
        return lon, lat

    def localization_iterative(self, col, row, alt):
        """normalised (col, row, alt) -> normalised (lon, lat)"""
        Xf = np.vstack([col, row]).T
        lon = -(col ** 0)
        lat = -(col ** 0)
        EPS = 2
        x0 = apply_rfm(self.col_num, self.col_den, lat, lon, alt)
        y0 = apply_rfm(self.row_num, self.row_den, lat, lon, alt)
        x1 = apply_rfm(self.col_num, self.col_den, lat, lon + EPS, alt)
        y1 = apply_rfm(self.row_num, self.row_den, lat, lon + EPS, alt)
        x2 = apply_rfm(self.col_num, self.col_den, lat + EPS, lon, alt)
        y2 = apply_rfm(self.row_num, self.row_den, lat + EPS, lon, alt)
        n = 0
        while not np.all((x0 - col) ** 2 + (y0 - row) ** 2 < 1e-18):
            if n > 100:
                raise MaxLocalizationIterationsError("Max localization iterations (100) exceeded")
            X0 = np.vstack([x0, y0]).T
            X1 = np.vstack([x1, y1]).T
            X2 = np.vstack([x2, y2]).T
            e1 = X1 - X0
            e2 = X2 - X0
            u = Xf - X0
            a1 = np.divide(np.sum(np.multiply(u, e1), axis=1), np.sum(np.multiply(e1, e1), axis=1)).squeeze()
            a2 = np.divide(np.sum(np.multiply(u, e2), axis=1), np.sum(np.multiply(e2, e2), axis=1)).squeeze()
            lon = lon + a1 * EPS
            lat = lat + a2 * EPS
            EPS = 0.1
            x0 = apply_rfm(self.col_num, self.col_den, lat, lon, alt)
            y0 = apply_rfm(self.row_num, self.row_den, lat, lon, alt)
            x1 = apply_rfm(self.col_num, self.col_den, lat, lon + EPS, alt)
            y1 = apply_rfm(self.row_num, self.row_den, lat, lon + EPS, alt)
            x2 = apply_rfm(self.col_num, self.col_den, lat + EPS, lon, alt)
            y2 = apply_rfm(self.row_num, self.row_den, lat + EPS, lon, alt)
            n += 1
        return lon, lat


WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563


def geodetic_to_ecef(lat_deg, lon_deg, h):
    """WGS84 geodetic (degrees, metres) -> ECEF (metres), with the prime-vertical radius N = a / sqrt(1 - e^2 sin^2(phi))"""
    phi, lam = np.deg2rad(lat_deg), np.deg2rad(lon_deg)
    e2 = WGS84_F * (2.0 - WGS84_F)
    s = np.sin(phi)
    N = WGS84_A / np.sqrt(1.0 - e2 * s * s)
    r = (N + h) * np.cos(phi)
    return r * np.cos(lam), r * np.sin(lam), (N * (1.0 - e2) + h) * s


def synthetic_rpc(seed, lat0=30.3, lon0=-81.7, w=41, h=37, inverse=False, off_nadir=0.25):
    """a JAX-like RPC (offsets about 30.3 N, 81.7 W; scales of a small crop) with off-nadir linear terms, non-trivial cubic and
    denominator terms; with inverse=True an affine forward model (off-nadir terms only) and lat/lon_num/den, its exact inverse
    (least squares over the crop)"""
    rng = np.random.default_rng(seed)
    d = {"row_offset": h / 2.0 + rng.uniform(-2, 2), "col_offset": w / 2.0 + rng.uniform(-2, 2),
         "lat_offset": lat0 + rng.uniform(-1e-3, 1e-3), "lon_offset": lon0 + rng.uniform(-1e-3, 1e-3),
         "alt_offset": 10.0 + rng.uniform(-5, 5), "row_scale": h / 2.0 + 3.0, "col_scale": w / 2.0 + 3.0,
         "lat_scale": 4e-4 * (1 + rng.uniform(-0.1, 0.1)), "lon_scale": 4.5e-4 * (1 + rng.uniform(-0.1, 0.1)),
         "alt_scale": 60.0 + rng.uniform(-10, 10)}
    col_num = np.zeros(20)
    row_num = np.zeros(20)
    col_num[1], col_num[2], col_num[3] = 1.0 + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), off_nadir * rng.uniform(0.5, 1)
    row_num[1], row_num[2], row_num[3] = rng.uniform(-0.05, 0.05), -(1.0 + rng.uniform(-0.05, 0.05)), off_nadir * rng.uniform(-1, 1)
    col_num[0], row_num[0] = rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01)
    col_num[4:] = rng.uniform(-3e-3, 3e-3, 16)
    row_num[4:] = rng.uniform(-3e-3, 3e-3, 16)
    col_den = np.zeros(20)
    row_den = np.zeros(20)
    col_den[0] = row_den[0] = 1.0
    col_den[1:] = rng.uniform(-1e-3, 1e-3, 19)
    row_den[1:] = rng.uniform(-1e-3, 1e-3, 19)
    if inverse:
        # an affine forward model, so that a polynomial inverse is exact and the round trip is a test of the arithmetic
        col_num[4:] = row_num[4:] = col_den[1:] = row_den[1:] = 0.0
    d.update(col_num=col_num.tolist(), row_num=row_num.tolist(), col_den=col_den.tolist(), row_den=row_den.tolist())
    if inverse:
        fwd = RPCModel(d)
        g = np.linspace(-1.1, 1.1, 9)
        L, P, H = [a.ravel() for a in np.meshgrid(g, g, g)]
        c, r = fwd.projection(L * d["lon_scale"] + d["lon_offset"], P * d["lat_scale"] + d["lat_offset"],
                              H * d["alt_scale"] + d["alt_offset"])
        nc, nr = (c - d["col_offset"]) / d["col_scale"], (r - d["row_offset"]) / d["row_scale"]
        ones = np.ones_like(nc)
        # terms of apply_poly(poly, x = nrow, y = ncol, z = nalt): a polynomial inverse, denominator 1
        A = np.stack([apply_poly(np.eye(20)[k], nr, nc, H) * ones for k in range(20)], 1)
        den = np.zeros(20)
        den[0] = 1.0
        d["lon_num"] = np.linalg.lstsq(A, L, rcond=None)[0].tolist()
        d["lat_num"] = np.linalg.lstsq(A, P, rcond=None)[0].tolist()
        d["lon_den"] = den.tolist()
        d["lat_den"] = den.tolist()
    return d
