"""Surface normals from the density field: n = -sum_i w_i grad sigma(x_i) / |sum_i w_i grad sigma(x_i)| along a ray
(Ref-NeRF's weight-averaged density normal), from ops.density_grad_into -- a training forward and the backward between a cotangent on
sigma and the sample positions (csrc/normals.hip, include/snerf_normals.h).  Unlike a raster normal (eval/utils/roofs.py: normals) it
has no lattice bias, exists for oblique views and walls, is defined per point of a cloud, and states the geometry a second time,
independently of the DSM.

ray_normals walks a frame; to_enu turns scene directions into east / north / up; normal_agreement compares a normal raster with the
normals of a DSM's raster gradients."""
import math

import numpy as np
import torch

from ...framework.components.rendering import z_steps_on

WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563


@torch.no_grad()
def ray_normals(cfgs, renderer, models, rays, extras, render_options=None, chunk=None):
    """One frame -> {"normal_n" (R, 3) f32: unit normals in normalised scene coordinates, NaN where the gradient is zero or not finite;
    "grad_norm" (R) f64: |sum_i w_i grad sigma(x_i)|; "depth" (R) f32: the expected depth of the same pass; "bad": the number of NaN
    normals (a Python int: the one host synchronisation)}.  A chunk walk of its own: every chunk is a TRAINING forward (the
    activations are kept) and the xyz-only backward, on a leased training workspace, so `chunk` defaults to the training batch size
    (cfgs.pipeline.batch_size), not render_chunk_size.  `render_options`: "perturb" / "perturb_rand" / "given_z_vals" as everywhere
    in evaluation; {"perturb": 0} for a repeatable frame."""
    from ... import ops
    from ...semantic.components.rendering import _pass_operands
    from .util import _chunk_options
    opts0 = dict(render_options) if render_options else {}
    n = rays.shape[0]
    chunk = int(chunk if chunk is not None else cfgs.pipeline.batch_size)
    if chunk < 1:
        raise ValueError(f"ray_normals: chunk = {chunk} must be >= 1")
    model = models["coarse"]
    dev = rays.device
    S = renderer.N_samples
    grad = torch.empty((n, 3), dtype=torch.float64, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    ops.release_workspaces()
    packed = ops.pack_params(model.spec, dict(model.named_parameters()))
    weights = None
    for i in range(0, n, chunk):
        k = min(chunk, n - i)
        opts = _chunk_options(opts0, i, chunk, n)
        opts["packed_params"] = packed
        r, e = rays[i:i + k], extras[i:i + k]
        u = opts.get("perturb_rand")
        if u is None and opts.get("given_z_vals") is None and opts.get("perturb", 1.0) > 0:
            u = torch.rand(k, S, device=dev, dtype=torch.float32)
        sun_d, rays_t, rays_t_s, params, _ = _pass_operands(models, model, e, opts)
        pin = ops.PassInputs(sun_d=sun_d, rays=r, z_vals=opts.get("given_z_vals"), z_steps=z_steps_on(dev, S), u=u)
        Sk = pin.z_vals.shape[1] if pin.z_vals is not None else S
        if weights is None or tuple(weights.shape) != (k, Sk):
            weights = torch.empty((k, Sk), dtype=torch.float32, device=dev)
        ops.density_grad_into(model.spec, params, pin, rays_t, rays_t_s, out={"grad": grad[i:i + k], "depth": depth[i:i + k], "weights": weights},
                              packed=packed)
    ops.release_workspaces()
    norm = torch.linalg.vector_norm(grad, dim=1)
    ok = torch.isfinite(norm) & (norm > 0)
    normal = torch.where(ok[:, None], -grad / torch.where(ok, norm, torch.ones_like(norm))[:, None],
                         torch.full_like(grad, float("nan"))).to(torch.float32)
    return {"normal_n": normal, "grad_norm": norm, "depth": depth, "bad": int((~ok).sum())}


def ecef_to_geodetic(x, y, z):
    """WGS84 latitude and longitude (radians) of an ECEF point, fp64 on the host (Bowring's iteration to convergence)"""
    e2 = WGS84_F * (2.0 - WGS84_F)
    lon = math.atan2(y, x)
    p = math.hypot(x, y)
    lat = math.atan2(z, p * (1.0 - e2))
    for _ in range(16):
        s = math.sin(lat)
        N = WGS84_A / math.sqrt(1.0 - e2 * s * s)
        new = math.atan2(z + e2 * N * s, p)
        if abs(new - lat) < 1e-15:
            lat = new
            break
        lat = new
    return lat, lon


def enu_rotation(geo):
    """(3, 3) fp64 numpy: rows east, north, up at the scene centre of `geo` (a GeoFrame), in ECEF axes"""
    lat, lon = ecef_to_geodetic(*[float(v) for v in geo.params.centre])
    sl, cl, sp, cp = math.sin(lon), math.cos(lon), math.sin(lat), math.cos(lat)
    return np.array([[-sl, cl, 0.0], [-sp * cl, -sp * sl, cp], [cp * cl, cp * sl, sp]], dtype=np.float64)


def to_enu(geo, normal_n):
    """Directions in normalised scene coordinates -> east / north / up at the scene centre, (R, 3) of the input's kind (tensor, on its
    device, or numpy) and dtype.  The normalisation is one centre and one range, hence isotropic: a direction in scene coordinates is
    the direction in ECEF, and one fp64 rotation does the rest.  East / north are the local geodetic ones: the UTM grid's convergence
    at the scene (a fraction of a degree) is ignored."""
    R = enu_rotation(geo)
    if torch.is_tensor(normal_n):
        Rt = torch.from_numpy(R).to(normal_n.device)
        return (normal_n.double() @ Rt.t()).to(normal_n.dtype)
    a = np.asarray(normal_n)
    return (a.astype(np.float64) @ R.T).astype(a.dtype)


def normal_agreement(normal_enu, dsm_gradient_east, dsm_gradient_north):
    """Per-cell angle (degrees) between a normal raster `normal_enu` -- (3, H, W), or (R, 3) with R = H W; east / north / up -- and the
    raster normal (-g_e, -g_n, 1) / |.| of a DSM's gradients (rise per metre east / north: roofs.normals' slope_e / slope_n), same
    number of cells.  -> (angle, of the gradients' shape, f64, NaN where either normal is not finite; {"cells": compared cells,
    "mean_deg", "median_deg", "share_under_15deg"}, None for the three without a compared cell).  Tensors or numpy alike; the result
    is numpy."""
    def arr(v):
        return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)
    ge, gn = arr(dsm_gradient_east), arr(dsm_gradient_north)
    nd = arr(normal_enu)
    if nd.shape == (3,) + ge.shape:
        nd = np.moveaxis(nd, 0, -1)
    nd = nd.reshape(-1, 3)
    if nd.shape[0] != ge.size or gn.shape != ge.shape:
        raise ValueError(f"normal_agreement: {nd.shape[0]} normals against gradients of shapes {ge.shape} and {gn.shape}")
    ref = np.stack([-ge.reshape(-1), -gn.reshape(-1), np.ones(ge.size)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = ref / np.linalg.norm(ref, axis=1, keepdims=True)
        nn = nd / np.linalg.norm(nd, axis=1, keepdims=True)
        cos = np.clip((ref * nn).sum(1), -1.0, 1.0)
        # atan2 of |a x b| and a . b keeps its accuracy at small angles, where acos loses half the digits
        ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(ref, nn), axis=1), (ref * nn).sum(1)))
    ang = np.where(np.isfinite(cos), ang, np.nan)
    ok = np.isfinite(ang)
    stats = {"cells": int(ok.sum()), "mean_deg": None, "median_deg": None, "share_under_15deg": None}
    if ok.any():
        stats.update(mean_deg=float(ang[ok].mean()), median_deg=float(np.median(ang[ok])), share_under_15deg=float((ang[ok] < 15.0).mean()))
    return ang.reshape(ge.shape), stats
