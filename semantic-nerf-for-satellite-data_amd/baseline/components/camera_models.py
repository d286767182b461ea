"""RPC camera model -- mirror of baseline/components/camera_models.py with rpcm.RPCModel's arithmetic on the device
(csrc/satrays.hip; the spec is in include/snerf_hip.h).  An RPC is built from a meta JSON's "rpc" dict in rpcm's __dict__ layout
(row/col/lat/lon/alt _offset and _scale, row/col_num/den, optional inverse lat/lon_num/den)."""
import numpy as np
import torch

from ... import _lib

_OFFSETS = ("row_offset", "col_offset", "lat_offset", "lon_offset", "alt_offset",
            "row_scale", "col_scale", "lat_scale", "lon_scale", "alt_scale")
_FORWARD = ("row_num", "row_den", "col_num", "col_den")
_INVERSE = ("lat_num", "lat_den", "lon_num", "lon_den")


def rpc_struct(d: dict) -> "_lib.SnerfRpc":
    """the C mirror of an rpcm dict; missing or mis-sized terms are refused"""
    s = _lib.SnerfRpc()
    for k in _OFFSETS:
        if k not in d:
            raise ValueError(f"RPC dict has no {k!r}")
        setattr(s, k, float(d[k]))
    inv = [k in d for k in _INVERSE]
    if any(inv) and not all(inv):
        raise ValueError("RPC dict has only part of the inverse model (lat_num, lat_den, lon_num, lon_den)")
    for k in _FORWARD + (_INVERSE if all(inv) else ()):
        v = np.asarray(d.get(k), dtype=np.float64) if k in d else None
        if v is None or v.shape != (20,):
            raise ValueError(f"RPC dict: {k!r} must hold 20 coefficients")
        getattr(s, k)[:] = v.tolist()
    s.has_inverse = 1 if all(inv) else 0
    return s


def struct_to_device(s, device) -> torch.Tensor:
    """the bytes of a ctypes struct (or array of structs) as a device tensor (the kernels read the table from device memory)"""
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(device)


class RPCModel:
    """rpcm.RPCModel's interface on the device: localization / projection take and return fp64 tensors on `device`"""

    def __init__(self, d: dict, device=None):
        self.d = d
        self.struct = rpc_struct(d)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = struct_to_device(self.struct, self.device)
        return self._dev

    def _f64(self, x, n=None, what="values"):
        """a contiguous fp64 vector on the device; with n: n values, a single value broadcast to n, anything else refused (the
        kernels read n values of every input)"""
        t = torch.as_tensor(x, dtype=torch.float64, device=self.device).reshape(-1)
        if n is not None and t.numel() != n:
            if t.numel() != 1:
                raise ValueError(f"{what}: {t.numel()} values for {n} points")
            t = t.expand(n)
        return t.contiguous()

    def localization(self, cols, rows, alts, return_normalized=False):
        """(lon, lat); raises MaxLocalizationIterationsError-like RuntimeError when a point does not converge (reads one int
        back from the device)"""
        c = self._f64(cols)
        r, a = self._f64(rows, c.numel(), "rows"), self._f64(alts, c.numel(), "alts")
        lon, lat = torch.empty_like(c), torch.empty_like(c)
        fails = torch.zeros(2, dtype=torch.int32, device=self.device)       # failed points, the call's update count
        _lib.call("snerf_rpc_localize", self.struct, self.dev, c, r, a, c.numel(), bool(return_normalized), lon, lat, fails)
        if int(fails[0].item()):
            raise RuntimeError(f"RPC localization: {int(fails[0].item())} points did not converge in 100 iterations "
                               "(rpcm: MaxLocalizationIterationsError)")
        return lon, lat

    def projection(self, lons, lats, alts):
        lon = self._f64(lons)
        lat, a = self._f64(lats, lon.numel(), "lats"), self._f64(alts, lon.numel(), "alts")
        col, row = torch.empty_like(lon), torch.empty_like(lon)
        _lib.call("snerf_rpc_project", self.struct, self.dev, lon, lat, a, lon.numel(), col, row)
        return col, row

    def reprojection_error(self, xyz_ecef, pts2d):
        """|pts2d - projection(geodetic(xyz_ecef))| per point, fp64, the geodetic conversion being the reference's custom one
        (satnerf_depth_dataset.py:150-159)"""
        x = torch.as_tensor(xyz_ecef, dtype=torch.float64, device=self.device).reshape(-1, 3).contiguous()
        p = torch.as_tensor(pts2d, dtype=torch.float64, device=self.device).reshape(-1, 2).contiguous()
        if x.shape[0] != p.shape[0]:
            raise ValueError(f"{x.shape[0]} points for {p.shape[0]} image coordinates")
        err = torch.empty(x.shape[0], dtype=torch.float64, device=self.device)
        _lib.call("snerf_rpc_reprojection_error", self.struct, self.dev, x, p, x.shape[0], None, err)
        return err


def construct_rpc_camera_model(d: dict, device=None) -> RPCModel:
    """from a meta dict (its "rpc" entry), as baseline/components/camera_models.py:25-39 with scale_factor = 1"""
    if "rpc" not in d:
        raise ValueError("meta dict has no 'rpc' entry")
    return RPCModel(d["rpc"], device=device)
