"""numpy restatements around the world-cloud kernel (tests and fixture generation only).

from_latlon -- the `utm` package's series (utm/conversion.py from_latlon), restated from its published formulas in fp64, in the
package's operation order.  The package itself is not installed where these tests run: parity with it is UNPINNED; what pins
the restatement is `kruger`, an independent four-term Krueger n-series (Karney 2011, eqs. 35-36 truncated at n^4) on the WGS84
ellipsoid, which tests/test_geo_cpu.py compares it with.  The Norway / Svalbard zone exceptions are not handled."""
import math

import numpy as np

K0 = 0.9996
E = 0.00669438
E2 = E * E
E3 = E2 * E
E_P2 = E / (1.0 - E)
R = 6378137.0
M1 = 1.0 - E / 4.0 - 3.0 * E2 / 64.0 - 5.0 * E3 / 256.0
M2 = 3.0 * E / 8.0 + 3.0 * E2 / 32.0 + 45.0 * E3 / 1024.0
M3 = 15.0 * E2 / 256.0 + 45.0 * E3 / 1024.0
M4 = 35.0 * E3 / 3072.0
ZONE_LETTERS = "CDEFGHJKLMNPQRSTUVWXX"


def zone_number(lat, lon):
    return int((lon + 180) / 6) % 60 + 1


def zone_letter(lat):
    if -80 <= lat <= 84:
        return ZONE_LETTERS[int(lat + 80) >> 3]
    return None


def central_meridian_rad(zone):
    return math.radians((zone - 1) * 6 - 180 + 3)


def wrap(v):
    """(v + pi) % (2 pi) - pi, into [-pi, pi)"""
    return np.mod(v + np.pi, 2.0 * np.pi) - np.pi


def from_latlon(lat, lon, zone, south=False):
    """(east, north) of points at (lat, lon) degrees in UTM zone `zone`; + 1e7 on the northing with `south`"""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    lat_rad = lat * (np.pi / 180.0)
    lon_rad = lon * (np.pi / 180.0)
    ls, lc = np.sin(lat_rad), np.cos(lat_rad)
    t = ls / lc
    t2 = t * t
    t4 = t2 * t2
    n = R / np.sqrt(1.0 - E * (ls * ls))
    c = E_P2 * (lc * lc)
    a = lc * wrap(lon_rad - central_meridian_rad(zone))
    a2 = a * a
    a3 = a2 * a
    a4 = a3 * a
    a5 = a4 * a
    a6 = a5 * a
    m = R * (M1 * lat_rad - M2 * np.sin(2.0 * lat_rad) + M3 * np.sin(4.0 * lat_rad) - M4 * np.sin(6.0 * lat_rad))
    east = K0 * n * (a + a3 / 6.0 * (1.0 - t2 + c) + a5 / 120.0 * (5.0 - 18.0 * t2 + t4 + 72.0 * c - 58.0 * E_P2)) + 500000.0
    north = K0 * (m + n * t * (a2 / 2.0 + a4 / 24.0 * (5.0 - t2 + 9.0 * c + 4.0 * (c * c))
                               + a6 / 720.0 * (61.0 - 58.0 * t2 + t4 + 600.0 * c - 330.0 * E_P2)))
    if south:
        north = north + 10000000.0
    return east, north


def kruger(lat, lon, zone, south=False):
    """transverse Mercator by the Krueger series in the third flattening n, four terms, WGS84 (a, 1/f = 298.257223563)"""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    a, f = 6378137.0, 1.0 / 298.257223563
    n = f / (2.0 - f)
    e = math.sqrt(f * (2.0 - f))
    A = a / (1.0 + n) * (1.0 + n ** 2 / 4.0 + n ** 4 / 64.0)
    alpha = (n / 2.0 - 2.0 * n ** 2 / 3.0 + 5.0 * n ** 3 / 16.0 + 41.0 * n ** 4 / 180.0,
             13.0 * n ** 2 / 48.0 - 3.0 * n ** 3 / 5.0 + 557.0 * n ** 4 / 1440.0,
             61.0 * n ** 3 / 240.0 - 103.0 * n ** 4 / 140.0,
             49561.0 * n ** 4 / 161280.0)
    phi = np.radians(lat)
    lam = wrap(np.radians(lon) - central_meridian_rad(zone))
    tau = np.tan(phi)
    sigma = np.sinh(e * np.arctanh(e * tau / np.sqrt(1.0 + tau * tau)))
    taup = tau * np.sqrt(1.0 + sigma * sigma) - sigma * np.sqrt(1.0 + tau * tau)
    xi = np.arctan2(taup, np.cos(lam))
    eta = np.arcsinh(np.sin(lam) / np.sqrt(taup * taup + np.cos(lam) ** 2))
    x, y = eta.copy(), xi.copy()
    for j, al in enumerate(alpha, start=1):
        y = y + al * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        x = x + al * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    east = K0 * A * x + 500000.0
    north = K0 * A * y + (10000000.0 if south else 0.0)
    return east, north
