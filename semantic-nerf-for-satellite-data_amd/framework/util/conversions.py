"""UTM helpers -- mirror of framework/util/conversions.py:7-40,104-150 (utm_from_latlon, utm_from_lonlat, latlon_from_utm,
lonlat_from_utm, convert_utm_to_local, convert_local_to_utm, split_zone_string, zonestring_to_hemisphere) on device tensors.  The
reference hands numpy arrays to the `utm` package; this build does not carry it, so the package's from_latlon series is restated
here (fp64 torch ops on the tensors' device, the operation order of csrc/geo.hip) -- parity with the package is UNPINNED, see
DESIGN.md section 5h.  The evaluation path does not go through utm_from_latlon: a frame's cloud is one launch of csrc/geo.hip
(framework/components/coordinate_systems.py GeoFrame); it serves callers that already hold lat / lon.

The way back (UTM -> lat / lon -> scene) exists on the device only: latlon_from_utm, lonlat_from_utm and the two convert_*
functions are launches of csrc/geo.hip (snerf_geo_points) on CUDA tensors, a CPU tensor is an error.

With zone_string=None the zone number comes from the FIRST point, int((lon + 180) / 6) % 60 + 1, and the letter from the first
latitude (bands C..X of 8 degrees from 80 S, X reaching 84 N), as the package picks them.  NOT handled: the package's
exceptions for Norway (32V) and Svalbard (31X-37X)."""
import math

import torch

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


def split_zone_string(zone_string):
    return int(zone_string[:-1]), zone_string[-1]


def zonestring_to_hemisphere(zonestring):
    zone_number, zone_letter = split_zone_string(zonestring)
    return str(zone_number) + ("N" if zone_letter >= "N" else "S")


def zone_is_south(zone_string) -> bool:
    return split_zone_string(zone_string)[1].upper() < "N"


def latlon_to_zone_number(lat, lon) -> int:
    return int((lon + 180) / 6) % 60 + 1


def latitude_to_zone_letter(lat) -> str:
    if not -80.0 <= lat <= 84.0:
        raise ValueError(f"latitude {lat} is outside the UTM bands (80 S .. 84 N)")
    return ZONE_LETTERS[int(lat + 80) >> 3]


def zone_central_meridian(zone_number: int) -> float:
    """central meridian of a zone in radians"""
    if not 1 <= zone_number <= 60:
        raise ValueError(f"UTM zone number {zone_number} outside [1, 60]")
    return math.radians((zone_number - 1) * 6 - 180 + 3)


def utm_from_latlon(lats, lons, zone_string=None):
    """(easts, norths, zone_string) of points at (lats, lons) degrees; tensors in, fp64 tensors on the same device out"""
    lats = torch.as_tensor(lats).double()
    lons = torch.as_tensor(lons).double().to(lats.device)
    if zone_string is None:
        if lats.numel() == 0:
            raise ValueError("utm_from_latlon: no point to take the zone from; pass zone_string")
        lat0, lon0 = float(lats.reshape(-1)[0]), float(lons.reshape(-1)[0])
        zone_string = str(latlon_to_zone_number(lat0, lon0)) + latitude_to_zone_letter(lat0)
    number, _ = split_zone_string(zone_string)
    lat_rad = lats * (math.pi / 180.0)
    lon_rad = lons * (math.pi / 180.0)
    ls, lc = torch.sin(lat_rad), torch.cos(lat_rad)
    t = ls / lc
    t2 = t * t
    t4 = t2 * t2
    n = R / torch.sqrt(1.0 - E * (ls * ls))
    c = E_P2 * (lc * lc)
    a = lc * (torch.remainder(lon_rad - zone_central_meridian(number) + math.pi, 2.0 * math.pi) - math.pi)
    a2 = a * a
    a3 = a2 * a
    a4 = a3 * a
    a5 = a4 * a
    a6 = a5 * a
    m = R * (M1 * lat_rad - M2 * torch.sin(2.0 * lat_rad) + M3 * torch.sin(4.0 * lat_rad) - M4 * torch.sin(6.0 * lat_rad))
    easts = K0 * n * (a + a3 / 6.0 * (1.0 - t2 + c) + a5 / 120.0 * (5.0 - 18.0 * t2 + t4 + 72.0 * c - 58.0 * E_P2)) + 500000.0
    norths = K0 * (m + n * t * (a2 / 2.0 + a4 / 24.0 * (5.0 - t2 + 9.0 * c + 4.0 * (c * c))
                                + a6 / 720.0 * (61.0 - 58.0 * t2 + t4 + 600.0 * c - 330.0 * E_P2)))
    if zone_is_south(zone_string):
        norths = norths + 10000000.0
    return easts, norths, zone_string


def utm_from_lonlat(lons, lats, zone_string=None):
    return utm_from_latlon(lats, lons, zone_string)


def _zone_frame(zone_string):
    """a GeoFrame of the zone alone (centre 0, range 1): its lat / lon do not depend on a scene's normalisation"""
    from ..components.coordinate_systems import GeoFrame

    class _Unit:
        @staticmethod
        def calculate_center_range():
            return (0.0, 0.0, 0.0), 1.0
    return GeoFrame(_Unit, zone_string)


def latlon_from_utm(easts, norths, zone_string):
    """(lats, lons) in degrees of the UTM points (easts, norths) of `zone_string` (utm.to_latlon); CUDA tensors in, fp64
    tensors of the inputs' shape out"""
    if not (torch.is_tensor(easts) and easts.is_cuda and torch.is_tensor(norths) and norths.is_cuda):
        raise ValueError("latlon_from_utm runs on the device: pass CUDA tensors")
    if easts.shape != norths.shape:
        raise ValueError(f"latlon_from_utm: easts {tuple(easts.shape)} and norths {tuple(norths.shape)} differ in shape")
    e, n = easts.double().reshape(-1), norths.double().reshape(-1)
    _, lla, _ = _zone_frame(zone_string).to_scene(torch.stack([e, n, torch.zeros_like(e)], 1), want_lla=True)
    return lla[:, 0].reshape(easts.shape), lla[:, 1].reshape(easts.shape)


def lonlat_from_utm(easts, norths, zone_string):
    lats, lons = latlon_from_utm(easts, norths, zone_string)
    return lons, lats


def _dataset_geo(dataset):
    geo = getattr(dataset, "geo", None)
    if geo is None:
        raise ValueError("the dataset carries no GeoFrame (`geo`): load a scene with a zone_string")
    return geo


def convert_utm_to_local(dataset, utm_points):
    """un-normalised UTM (N, 3) (east, north, alt) -> the loaded dataset's normalised scene coordinates (N, 3) f64"""
    return _dataset_geo(dataset).to_scene(utm_points)[0]


def convert_local_to_utm(dataset, xyz):
    """normalised scene coordinates (N, 3) -> un-normalised UTM (N, 3) f64 (east, north, alt)"""
    return _dataset_geo(dataset).points(xyz)[0]
