"""CPU-side checks of the world -> scene direction: the numpy restatement of the utm package's to_latlon
series (tests/utm_inverse_numpy.py) against the inverse of the independent Krueger n-series, its round trip through the forward
restatement, the southern flag, the wrap across +-180 degrees, and the host's argument checks.

The `utm` package is not installed where this suite runs: parity with the package itself is UNPINNED.  Point sets: 20,000
uniform points each, seed 0 (utm_inverse_numpy.region).  Measured -> bar, in metres on the ground:
    series inverse vs kruger_inverse    jax 4.4e-5 -> 1e-4    mid (+-1.5 deg) 1.8e-4 -> 5e-4    edge (+-3 deg) 1.26e-2 -> 3e-2
    from_latlon(to_latlon(E, N))        jax 4.4e-5 -> 1e-4    mid (+-1.5 deg) 8.4e-4 -> 2e-3    edge (+-3 deg) 1.26e-2 -> 3e-2
These are the truncation of series of this order; the bars are about twice the measured values, to cover other seeds and
latitudes.  kruger_inverse itself returns kruger's input to 1e-8 m (measured 3.7e-9 m: northings reach 7.8e6 m, where one fp64
ulp is 9e-10 m, and the series is a few dozen operations)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import utm_inverse_numpy as V
from tests import utm_numpy as U

SERIES_BARS = {"jax": 1e-4, "mid": 5e-4, "edge": 3e-2}
ROUND_TRIP_BARS = {"jax": 1e-4, "mid": 2e-3, "edge": 3e-2}


@pytest.fixture(scope="module")
def sets():
    out = {}
    for name in SERIES_BARS:
        lat, lon, zone = V.region(name)
        e, n = U.kruger(lat, lon, zone)
        out[name] = {"lat": lat, "lon": lon, "zone": zone, "east": e, "north": n}
    return out


@pytest.mark.parametrize("name", list(SERIES_BARS))
def test_series_inverse_against_the_kruger_inverse(name, sets):
    s = sets[name]
    lat_k, lon_k = V.kruger_inverse(s["east"], s["north"], s["zone"])
    e, n = U.kruger(lat_k, lon_k, s["zone"])
    closes = float(np.hypot(e - s["east"], n - s["north"]).max())
    truth = float(V.ground_distance(s["lat"], s["lon"], lat_k, lon_k).max())
    lat_s, lon_s = V.to_latlon(s["east"], s["north"], s["zone"])
    d = float(V.ground_distance(lat_k, lon_k, lat_s, lon_s).max())
    print(f"{name}: kruger_inverse closes to {closes:.3e} m ({truth:.3e} m from the sampled points); series vs it {d:.3e} m")
    assert closes <= 1e-8 and truth <= 1e-8
    assert d <= SERIES_BARS[name]


@pytest.mark.parametrize("name", list(ROUND_TRIP_BARS))
def test_forward_of_inverse_round_trip(name, sets):
    """from_latlon(to_latlon(E, N)) = (E, N): what the nadir rays rely on (the cloud of a nadir ray lands on its cell centre)"""
    s = sets[name]
    lat, lon = V.to_latlon(s["east"], s["north"], s["zone"])
    e, n = U.from_latlon(lat, lon, s["zone"])
    d = float(np.hypot(e - s["east"], n - s["north"]).max())
    print(f"{name}: from_latlon(to_latlon) residual {d:.3e} m")
    assert d <= ROUND_TRIP_BARS[name]


def test_southern_flag_removes_exactly_1e7(sets):
    s = sets["mid"]
    lat, lon = V.to_latlon(s["east"], s["north"], 17)
    lat_s, lon_s = V.to_latlon(s["east"], s["north"] + 10000000.0, 17, south=True)
    # north + 1e7 is rounded once: the flag takes 1e7 off THAT number, bit for bit
    back = (s["north"] + 10000000.0) - 10000000.0
    lat_b, lon_b = V.to_latlon(s["east"], back, 17)
    assert np.array_equal(lat_s, lat_b) and np.array_equal(lon_s, lon_b)
    assert float(np.abs(lat_s - lat).max()) <= 1e-13 and float(np.abs(lon_s - lon).max()) <= 1e-13
    # a southern point: forward with the flag, back with the flag
    e, n = U.from_latlon(-33.9, 18.4, 34, south=True)
    la, lo = V.to_latlon(e, n, 34, south=True)
    assert abs(float(la) + 33.9) <= 1e-8 and abs(float(lo) - 18.4) <= 1e-8


def test_longitudes_wrap_across_the_date_line():
    """zones 1 and 60 touch +-180 degrees: a point just beyond the date line comes back on ITS side of it, in [-180, 180).
    The points lie within 3.01 degrees of their meridians: the zone-edge bar of the series, 3e-2 m."""
    lat = np.array([10.0, -20.0, 45.0])
    for zone, lon in ((1, np.array([-179.9, 179.99, -179.5])), (60, np.array([179.9, -179.99, 179.5]))):
        e, n = U.from_latlon(lat, lon, zone)
        la, lo = V.to_latlon(e, n, zone)
        assert np.all(lo >= -180.0) and np.all(lo < 180.0)
        d = float(V.ground_distance(lat, lon, la, lo).max())
        print(f"zone {zone}: {d:.3e} m")
        assert d <= 3e-2
        assert np.array_equal(np.sign(lo), np.sign(lon))


def test_constants_are_the_packages():
    assert V._E == (1.0 - np.sqrt(1.0 - U.E)) / (1.0 + np.sqrt(1.0 - U.E)) and abs(V._E - 1.6792203889e-3) < 1e-12
    assert V.P2 > V.P3 > V.P4 > V.P5 > 0.0
    # the footpoint series inverts the meridian arc of the forward restatement to the round-trip bar (2e-3 m; 1 deg <= 111.7 km)
    lat = np.linspace(-80.0, 84.0, 165)
    _, n = U.from_latlon(lat, np.full_like(lat, -81.0), 17)
    la, lo = V.to_latlon(np.full_like(lat, 500000.0), n, 17)
    assert float(np.abs(la - lat).max()) * 111.7e3 <= 2e-3 and np.array_equal(lo, np.full_like(lat, -81.0))


def test_params_mirror_and_direction_word():
    from snerf_amd import _lib
    names = [f[0] for f in _lib.SnerfGeoParams._fields_]
    assert names == ["centre", "range", "lon0", "south", "direction"]
    assert C.sizeof(_lib.SnerfGeoParams) == 48 and _lib.SnerfGeoParams.direction.offset == 44
    assert (_lib.GEO_TO_WORLD, _lib.GEO_TO_SCENE) == (0, 1)
    assert _lib.ABI_VERSION == 6


class _Norm:
    @staticmethod
    def calculate_center_range():
        return (768000.0, -5450000.0, 3200000.0), 300.0


def test_host_argument_checks():
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    from snerf_amd.framework.util import conversions as Cv
    frame = GeoFrame(_Norm, "17R")
    assert frame.params.direction == 0
    with pytest.raises(ValueError, match="CUDA"):
        frame.to_scene(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        frame.to_scene(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        Cv.latlon_from_utm(torch.zeros(4), torch.zeros(4), "17R")
    with pytest.raises(ValueError, match="CUDA"):
        Cv.lonlat_from_utm(torch.zeros(4), torch.zeros(4), "17R")
    ds = type("D", (), {"geo": frame})()
    with pytest.raises(ValueError, match="CUDA"):
        Cv.convert_utm_to_local(ds, torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="CUDA"):
        Cv.convert_local_to_utm(ds, torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="GeoFrame"):
        Cv.convert_utm_to_local(type("D", (), {"geo": None})(), torch.zeros((4, 3)))
    assert frame.params.direction == 0                       # the frame keeps its forward params


def test_nadir_argument_checks():
    from snerf_amd.baseline.components import rays as R
    from snerf_amd.eval.utils.dsm import DsmGrid
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    frame = GeoFrame(_Norm, "17R")
    grid = DsmGrid(435000.0, 3355000.0, 0.5, 4, 3)
    with pytest.raises(ValueError, match="min_alt"):
        R.nadir_construct(grid, frame, 10.0, 10.0)
    with pytest.raises(ValueError, match="min_alt"):
        R.nadir_construct(grid, frame, 10.0, -5.0)
    with pytest.raises(ValueError, match="min_alt"):
        R.nadir_construct(grid, frame, float("nan"), 5.0)
    with pytest.raises(ValueError, match="empty"):
        R.nadir_construct(DsmGrid(435000.0, 3355000.0, 0.5, 0, 3), frame, -10.0, 10.0)
    e, n = R.nadir_cell_centres(grid)
    assert e.dtype == n.dtype == torch.float64 and tuple(e.shape) == tuple(n.shape) == (3, 4)
    assert e[0].tolist() == [435000.25, 435000.75, 435001.25, 435001.75] and n[:, 0].tolist() == [3354999.75, 3354999.25, 3354998.75]
    assert torch.equal(e[0], e[2]) and torch.equal(n[:, 0], n[:, 3])
    # a window of the lattice: its cell (0, 0) is the lattice's cell (joff, ioff)
    from snerf_amd.eval.utils.dsm import grid_struct
    ew, nw = R.nadir_cell_centres(grid_struct(grid, (2, 1, 2, 2)))
    assert torch.equal(ew, e[1:3, 2:4]) and torch.equal(nw, n[1:3, 2:4])
    x = R.nadir_extras(40.0, 150.0, 3, 5)
    assert tuple(x.shape) == (5, 4) and x.dtype == torch.float32 and x.is_contiguous()
    assert torch.equal(x[:, :3], R.construct_sun_dir(40.0, 150.0, 5)) and x[:, 3].tolist() == [3.0] * 5
