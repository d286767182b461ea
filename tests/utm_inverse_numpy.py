"""numpy restatements around the world -> scene direction of the world-cloud kernel (tests only; the forward ones are
tests/utm_numpy.py).

to_latlon -- the `utm` package's inverse series (utm/conversion.py to_latlon), restated from its published formulas in fp64, in
the operation order of csrc/geo.hip's utm_to_latlon.  The package itself is not installed where these tests run: parity with it
is UNPINNED; what pins the restatement is kruger_inverse.
kruger_inverse -- Newton's method on tests/utm_numpy.kruger (the independent four-term Krueger n-series), six steps from the
series' answer with a finite-difference Jacobian: the (lat, lon) that kruger maps onto the given (east, north).
latlon_to_ecef, to_scene -- framework/util/conversions.py latlon_to_ecef_custom and StandardNormalization.normalize_xyz on fp64."""
import math

import numpy as np

from tests import utm_numpy as U

K0, E, E_P2, R, M1 = U.K0, U.E, U.E_P2, U.R, U.M1
_E = (1.0 - math.sqrt(1.0 - E)) / (1.0 + math.sqrt(1.0 - E))
_E2 = _E * _E
_E3 = _E2 * _E
_E4 = _E3 * _E
_E5 = _E4 * _E
P2 = 3.0 / 2.0 * _E - 27.0 / 32.0 * _E3 + 269.0 / 512.0 * _E5
P3 = 21.0 / 16.0 * _E2 - 55.0 / 32.0 * _E4
P4 = 151.0 / 96.0 * _E3 - 417.0 / 128.0 * _E5
P5 = 1097.0 / 512.0 * _E4


def to_latlon(east, north, zone, south=False):
    """(lat, lon) in degrees of the points (east, north) of UTM zone `zone`; `south`: the northing carries the 1e7 offset"""
    east, north = np.asarray(east, np.float64), np.asarray(north, np.float64)
    x = east - 500000.0
    y = north - 10000000.0 if south else north
    m = y / K0
    mu = m / (R * M1)
    p = mu + P2 * np.sin(2.0 * mu) + P3 * np.sin(4.0 * mu) + P4 * np.sin(6.0 * mu) + P5 * np.sin(8.0 * mu)
    ps, pc = np.sin(p), np.cos(p)
    pt = ps / pc
    pt2 = pt * pt
    pt4 = pt2 * pt2
    eps = 1.0 - E * (ps * ps)
    n = R / np.sqrt(eps)
    r = (1.0 - E) / eps
    c = E_P2 * (pc * pc)
    c2 = c * c
    d = x / (n * K0)
    d2 = d * d
    d3 = d2 * d
    d4 = d3 * d
    d5 = d4 * d
    d6 = d5 * d
    lat = (p - (pt / r) * (d2 / 2.0 - d4 / 24.0 * (5.0 + 3.0 * pt2 + 10.0 * c - 4.0 * c2 - 9.0 * E_P2))
           + d6 / 720.0 * (61.0 + 90.0 * pt2 + 298.0 * c + 45.0 * pt4 - 252.0 * E_P2 - 3.0 * c2))
    lon = (d - d3 / 6.0 * (1.0 + 2.0 * pt2 + c)
           + d5 / 120.0 * (5.0 - 2.0 * c + 28.0 * pt2 - 3.0 * c2 + 8.0 * E_P2 + 24.0 * pt4)) / pc
    lon = U.wrap(lon + U.central_meridian_rad(zone))
    return lat * (180.0 / np.pi), lon * (180.0 / np.pi)


def kruger_inverse(east, north, zone, south=False, steps=6, h=1e-6):
    """the (lat, lon) degrees with U.kruger(lat, lon) = (east, north): Newton from to_latlon's answer, the 2 x 2 Jacobian by
    forward differences of `h` degrees.  Longitudes are not wrapped: keep away from +-180 degrees."""
    east, north = np.asarray(east, np.float64), np.asarray(north, np.float64)
    lat, lon = to_latlon(east, north, zone, south)
    for _ in range(steps):
        e0, n0 = U.kruger(lat, lon, zone, south)
        e1, n1 = U.kruger(lat + h, lon, zone, south)
        e2, n2 = U.kruger(lat, lon + h, zone, south)
        a, b, c, d = (e1 - e0) / h, (e2 - e0) / h, (n1 - n0) / h, (n2 - n0) / h      # d(e, n) / d(lat, lon)
        re, rn = east - e0, north - n0
        det = a * d - b * c
        lat = lat + (d * re - b * rn) / det
        lon = lon + (a * rn - c * re) / det
    return lat, lon


def ground_distance(lat_a, lon_a, lat_b, lon_b):
    """metres between two nearby geodetic points (degrees): the meridional and prime-vertical radii of the utm package's
    ellipsoid at the first point"""
    phi = np.radians(lat_a)
    w = 1.0 - E * np.sin(phi) ** 2
    rm, rn = R * (1.0 - E) / w ** 1.5, R / np.sqrt(w)
    dlon = U.wrap(np.radians(lon_b) - np.radians(lon_a))
    return np.hypot(np.radians(lat_b - lat_a) * rm, dlon * rn * np.cos(phi))


def latlon_to_ecef(lat, lon, alt):
    """framework/util/conversions.py latlon_to_ecef_custom, the operation order of csrc/geo_dev.h"""
    rad_lat = lat * (np.pi / 180.0)
    rad_lon = lon * (np.pi / 180.0)
    a = 6378137.0
    finv = 298.257223563
    f = 1.0 / finv
    e2 = 1.0 - (1.0 - f) * (1.0 - f)
    sl, cl = np.sin(rad_lat), np.cos(rad_lat)
    v = a / np.sqrt(1.0 - e2 * sl * sl)
    return (v + alt) * cl * np.cos(rad_lon), (v + alt) * cl * np.sin(rad_lon), (v * (1.0 - e2) + alt) * sl


def to_scene(enu, centre, rng, zone, south=False):
    """the world -> scene chain on (n, 3) (east, north, alt): -> (xyz_n (n, 3), lat, lon)"""
    enu = np.asarray(enu, np.float64)
    lat, lon = to_latlon(enu[:, 0], enu[:, 1], zone, south)
    x, y, z = latlon_to_ecef(lat, lon, enu[:, 2])
    xyz = np.stack([x, y, z], 1)
    return (xyz - np.asarray(centre, np.float64)) / float(rng), lat, lon


def region(name, n=20000, seed=0):
    """the point sets of tests/test_geo_inverse_cpu.py: (lat, lon, zone) uniform over "jax" (the fixture's neighbourhood, up to
    0.7 deg from the meridian of zone 17), "mid" (lat -60 .. 70, within 1.5 deg) or "edge" (lat -60 .. 70, within 3 deg)"""
    rng = np.random.default_rng(seed)
    lat_lo, lat_hi, half = {"jax": (30.0, 30.6, 0.7), "mid": (-60.0, 70.0, 1.5), "edge": (-60.0, 70.0, 3.0)}[name]
    lat = rng.uniform(lat_lo, lat_hi, n)
    lon = -81.0 + rng.uniform(-half, half, n)
    return lat, lon, 17


def ecef_to_latlon(x, y, z):
    """framework/util/conversions.py ecef_to_latlon_custom, the operation order of csrc/geo_dev.h: -> (lat, lon, alt)"""
    a = 6378137.0
    e = 8.1819190842622e-2
    asq = a * a
    esq = e * e
    b = np.sqrt(asq * (1.0 - esq))
    bsq = b * b
    ep = np.sqrt((asq - bsq) / bsq)
    p = np.sqrt(x * x + y * y)
    th = np.arctan2(a * z, b * p)
    lon = np.arctan2(y, x)
    st, ct = np.sin(th), np.cos(th)
    lat = np.arctan2(z + (ep * ep) * b * (st * st * st), p - esq * a * (ct * ct * ct))
    sl = np.sin(lat)
    n = a / np.sqrt(1.0 - esq * (sl * sl))
    return lat * 180.0 / np.pi, lon * 180.0 / np.pi, p / np.cos(lat) - n


def to_world(xyz_n, centre, rng, zone, south=False):
    """the scene -> world chain on (n, 3) normalised points: -> (n, 3) (east, north, alt)"""
    ecef = np.asarray(xyz_n, np.float64) * float(rng) + np.asarray(centre, np.float64)
    lat, lon, alt = ecef_to_latlon(ecef[:, 0], ecef[:, 1], ecef[:, 2])
    east, north = U.from_latlon(lat, lon, zone, south)
    return np.stack([east, north, alt], 1)


def round_trip_residual(enu, centre, rng, zone, south=False):
    """max |to_world(to_scene(enu)) - enu| over points and components, metres: what the two restated series and the geodetic
    pair leave of a UTM point taken into the scene and back, without the code under test"""
    enu = np.asarray(enu, np.float64)
    back = to_world(to_scene(enu, centre, rng, zone, south)[0], centre, rng, zone, south)
    return float(np.abs(back - enu).max())
