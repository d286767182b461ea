"""StandardNormalization -- mirror of baseline/components/normalization.py and framework/components/normalization.py.
Parameters: per axis, min and max over the origins and the fp32 far points o + far * d of every ray of the train AND test
banks (base_ray_pipeline.py:198-244); scale = (max - min) / 2 and offset = min + scale in fp32, center = offsets,
range = max(scales).  Computed on the device by snerf_ray_bounds (exact min / max); normalise = (o - center) / range,
near / range, far / range in correctly rounded fp32 (snerf_normalize_rows).

With run.cache_dp set the parameters live in <cache_dp>/<dataset_name>/normalization/norm_params.json in the reference's key
format; a file that already exists is USED (as the reference does), so a run reproduces the rays of a run that the reference
normalised.  The values are written as the exact decimal of their fp32 value (the reference's json.dump of numpy float32
scalars is refused by json), so a round trip is exact.  Only rank 0 writes; every rank computes the same parameters."""
import ctypes as C
import json
import os

import numpy as np
import torch

from ... import _lib

KEYS = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")


def norm_params_path(cfgs):
    r = cfgs.run
    if not r.cache_dp:
        return None
    return os.path.join(r.cache_dp, r.dataset_name or "", "normalization", "norm_params.json")


def ray_bounds(ray_tensors) -> torch.Tensor:
    """(13,) fp32 on the rays' device: min[3], max[3], scale[3], offset[3], range"""
    ray_tensors = [t for t in ray_tensors]
    dev = ray_tensors[0].device
    for t in ray_tensors:
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 8 or not t.is_contiguous() or t.device != dev:
            raise ValueError("ray_bounds: contiguous (R, 8) fp32 ray tensors on one device")
    n = (C.c_longlong * len(ray_tensors))(*[int(t.shape[0]) for t in ray_tensors])
    ptrs = (C.c_void_p * len(ray_tensors))(*[t.data_ptr() for t in ray_tensors])
    ws = torch.empty(_lib.call_size("snerf_ray_bounds_workspace_bytes", n, len(ray_tensors)), dtype=torch.uint8, device=dev)
    out = torch.empty(13, dtype=torch.float32, device=dev)
    _lib.call("snerf_ray_bounds", ptrs, n, len(ray_tensors), out, ws, ws.numel())
    return out


def normalize_rows_(rows: torch.Tensor, center_range: torch.Tensor, bounds: bool):
    if rows.dtype != torch.float32 or not rows.is_contiguous() or rows.dim() != 2:
        raise ValueError("normalize_rows_: contiguous 2-d fp32 rows")
    cr = center_range.to(device=rows.device, dtype=torch.float32).contiguous()
    _lib.call("snerf_normalize_rows", rows, rows.shape[0], rows.shape[1], bounds, cr)
    return rows


class StandardNormalization:
    def __init__(self, cfgs=None, cache_fp=None, rank=0):
        self.cache_fp = cache_fp if cache_fp is not None else (norm_params_path(cfgs) if cfgs is not None else None)
        self.rank = rank
        self.center_range = None     # (4,) fp32 tensor: center[3], range
        self.norm_params = None

    def initialize(self, ray_tensors):
        """read the cached parameters when the file exists, else compute them from the rays (and write them on rank 0)"""
        if self.cache_fp is not None and os.path.exists(self.cache_fp):
            with open(self.cache_fp) as f:
                self.set_params(json.load(f))
            return self
        b = ray_bounds(ray_tensors)
        self.center_range = b[9:13].clone()
        h = b.cpu().numpy()
        self.norm_params = {"X_scale": float(h[6]), "X_offset": float(h[9]), "Y_scale": float(h[7]), "Y_offset": float(h[10]),
                            "Z_scale": float(h[8]), "Z_offset": float(h[11])}
        if self.cache_fp is not None and self.rank == 0:
            # written aside and renamed into place: a rank that looks for the file meanwhile sees none or a whole one
            os.makedirs(os.path.dirname(self.cache_fp), exist_ok=True)
            tmp = f"{self.cache_fp}.{os.getpid()}.tmp"
            with open(tmp, "w") as f:
                json.dump(self.norm_params, f, indent=4)
            os.replace(tmp, self.cache_fp)
        return self

    def set_params(self, d: dict):
        missing = [k for k in KEYS if k not in d]
        if missing:
            raise ValueError(f"normalization parameters lack {missing}")
        self.norm_params = {k: float(d[k]) for k in KEYS}
        center, rng = self.calculate_center_range()
        self.center_range = torch.cat([center, rng.reshape(1)])
        return self

    def calculate_center_range(self):
        """(center (3,), range ()) as fp32 tensors: the offsets, and the largest of the three scales"""
        p = self.norm_params
        center = torch.tensor([p[f"{axis}_offset"] for axis in "XYZ"], dtype=torch.float32)
        scales = torch.tensor([p[f"{axis}_scale"] for axis in "XYZ"], dtype=torch.float32)
        return center, scales.max()

    def normalize_rays_(self, rays: torch.Tensor):
        """origins, near and far of (R, 8) rays, in place"""
        return normalize_rows_(rays, self.center_range, bounds=True)

    def normalize_xyz(self, xyz: torch.Tensor):
        """(N, 3) fp32 points, in place on the device (normalize_xyz of the reference)"""
        return normalize_rows_(xyz, self.center_range, bounds=False)

    def denormalize(self, item: dict) -> torch.Tensor:
        """normalised (N, 3) points item["xyz"] back to ECEF: xyz * range + center (two roundings, in xyz's dtype)"""
        if "xyz" not in item:
            raise ValueError("denormalize: only an 'xyz' entry can be denormalised")
        xyz = item["xyz"]
        center, rng = (t.to(xyz.device) for t in self.calculate_center_range())
        return xyz * rng + center
