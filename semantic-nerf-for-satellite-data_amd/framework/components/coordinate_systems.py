"""Coordinate systems of the scene loaders (the reference's framework/components/coordinate_systems.py offers a custom ECEF
system and a UTM one).  Scenes load and TRAIN in the custom ECEF system only, and its conversions run on the device inside
the ray and reprojection kernels (csrc/satrays.hip, csrc/geo_dev.h: latlon_to_ecef, ecef_to_latlon); asking for the UTM system
for training is an error, not a silent switch to ECEF.

GeoFrame takes a loaded scene's predictions back to the world for EVALUATION: normalised ECEF end points -> ECEF -> lat / lon /
alt -> UTM (east, north, alt), one launch of csrc/geo.hip per frame, which also folds the east / north bounds the DSM grid
needs (the reference: satnerf_dataset.py:156-206, normalization.py:50-58, conversions.py:61-83,111-150, eval/utils/dsm.py:18-36,
all numpy on the host).  GeoFrame.to_scene is the way back, UTM (east, north, alt) -> lat / lon -> ECEF -> normalised scene
coordinates (the reference's conversions.py:7-24 convert_utm_to_local), the same entry point with `direction` = 1: it is what
casts a vertical ray per map cell (baseline/components/rays.py nadir_construct).  Both UTM series are the
`utm` package's, restated; the package is not part of this build, so parity with it is UNPINNED (DESIGN.md sections 5h, 5l).  DIVERGENCE: the zone is the scene's (root.json "zone_string"), where the reference's
get_utm_cloud lets `utm` pick it from the first point -- the same zone unless a scene straddles a zone edge."""
import ctypes as C
import struct
from collections import namedtuple

import torch

from ... import _lib
from ..util.conversions import split_zone_string, zone_central_meridian, zone_is_south

CUSTOM_ECEF = "custom_ecef"

# east / north extremes of a cloud's finite points (floats); of to_scene's output: its scene x / y extremes
GeoBounds = namedtuple("GeoBounds", "xmin xmax ymin ymax")


def init_coordinate_system(cfgs) -> str:
    """the datasets' coordinate system: CUSTOM_ECEF, or an error for `use_utm_coordinate_system`"""
    if getattr(cfgs.pipeline, "use_utm_coordinate_system", False):
        raise NotImplementedError("use_utm_coordinate_system = true: training in the UTM coordinate system is not supported; "
                                  "scenes load in the custom ECEF system only (GeoFrame converts predictions to UTM for "
                                  "evaluation)")
    return CUSTOM_ECEF


def key_to_double(key: int) -> float:
    """inverse of the kernels' order-preserving key of a double (csrc/reduce.h order_key)"""
    bits = key ^ (1 << 63) if key >> 63 else ~key & (2 ** 64 - 1)
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def decode_geo_stats(words):
    """8 stats words (ints, unsigned) -> (GeoBounds, non-finite count); +-inf bounds when no point was finite"""
    u = [int(w) & (2 ** 64 - 1) for w in words]
    inf = float("inf")
    if u[0] == _lib.GEO_STATS_INIT[0]:
        return GeoBounds(inf, -inf, inf, -inf), u[4]
    return GeoBounds(*(key_to_double(k) for k in u[:4])), u[4]


class GeoFrame:
    """normalised scene coordinates -> UTM (cloud, points) and back (to_scene), from a StandardNormalization (centre, range) and
    a zone string ("17R")"""

    def __init__(self, normalization, zone_string: str):
        center, rng = normalization.calculate_center_range()
        number, _ = split_zone_string(zone_string)
        self.zone_string = zone_string
        self.params = _lib.SnerfGeoParams((C.c_double * 3)(*[float(v) for v in center]), float(rng), zone_central_meridian(number),
                                          int(zone_is_south(zone_string)), _lib.GEO_TO_WORLD)

    @staticmethod
    def _outputs(n, dev, want_lla):
        enu = torch.empty((n, 3), dtype=torch.float64, device=dev)
        lla = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_lla else None
        # int64 holds the unsigned words bit for bit (2^64 - 1 = -1)
        return enu, lla, torch.tensor([-1, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int64, device=dev)

    @staticmethod
    def _result(enu, lla, stats):
        bounds, bad = decode_geo_stats(stats.cpu().tolist())
        if bad:
            raise ValueError(f"GeoFrame: {bad} of {enu.shape[0]} point(s) are not finite")
        return (enu, bounds) if lla is None else (enu, lla, bounds)

    def cloud(self, rays, depth, want_lla=False):
        """rays (R, >= 6) fp32 (normalised), depth (R,) fp32 -> (cloud (R, 3) f64 (east, north, alt)[, lla (R, 3) f64
        (lat deg, lon deg, alt)], GeoBounds).  Raises ValueError naming the count when points are not finite."""
        if not (torch.is_tensor(rays) and rays.is_cuda and torch.is_tensor(depth) and depth.is_cuda):
            raise ValueError("GeoFrame runs on the device: pass CUDA tensors")
        rays = rays.reshape(-1, rays.shape[-1])
        depth = depth.reshape(-1)
        if rays.dtype != torch.float32 or depth.dtype != torch.float32:
            raise ValueError("GeoFrame.cloud: fp32 rays and depth (the kernel widens them to fp64, as rays.double() does)")
        if rays.shape[1] < 6 or depth.shape[0] != rays.shape[0]:
            raise ValueError(f"GeoFrame.cloud: rays {tuple(rays.shape)} and depth {tuple(depth.shape)} do not match")
        rays, depth = rays.contiguous(), depth.contiguous()
        out = self._outputs(rays.shape[0], rays.device, want_lla)
        _lib.call("snerf_geo_cloud", rays, rays.shape[1], depth, rays.shape[0], self.params, *out)
        return self._result(*out)

    def points(self, xyz_n, want_lla=False):
        """normalised points (N, 3) -> as `cloud`; computed in fp64 (an fp32 input is widened first)"""
        if not (torch.is_tensor(xyz_n) and xyz_n.is_cuda):
            raise ValueError("GeoFrame runs on the device: pass CUDA tensors")
        if xyz_n.dim() != 2 or xyz_n.shape[1] != 3:
            raise ValueError("GeoFrame.points: (N, 3) points")
        xyz_n = xyz_n.double().contiguous()
        out = self._outputs(xyz_n.shape[0], xyz_n.device, want_lla)
        _lib.call("snerf_geo_points", xyz_n, xyz_n.shape[0], self.params, *out)
        return self._result(*out)

    def to_scene(self, enu, want_lla=False):
        """UTM points (N, 3) (east, north, alt) in the frame's zone -> (xyz_n (N, 3) f64 normalised scene coordinates[, lla
        (N, 3) f64 (lat deg, lon deg, alt)], GeoBounds of scene x / y); the inverse of `points`, computed in fp64 (an fp32 input
        is widened first).  Raises ValueError naming the count when points are not finite."""
        if not (torch.is_tensor(enu) and enu.is_cuda):
            raise ValueError("GeoFrame runs on the device: pass CUDA tensors")
        if enu.dim() != 2 or enu.shape[1] != 3:
            raise ValueError("GeoFrame.to_scene: (N, 3) points")
        enu = enu.double().contiguous()
        # the frame keeps its forward params: the inverse call uses a copy
        p = _lib.SnerfGeoParams.from_buffer_copy(self.params)
        p.direction = _lib.GEO_TO_SCENE
        out = self._outputs(enu.shape[0], enu.device, want_lla)
        _lib.call("snerf_geo_points", enu, enu.shape[0], p, *out)
        return self._result(*out)
