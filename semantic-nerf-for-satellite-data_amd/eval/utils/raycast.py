"""Rays on a DSM: where the ray of a view meets a height field -- the way back from the map lattice into an image.  Every other
geometry product of this project lives on the lattice (the DSM from clouds, the nadir DSM, cast shadows, orthorectified images);
this module takes a DSM (lidar, a stereo product, the model's own nadir DSM) into a view.  The reference has no counterpart; the
spec is include/snerf_raycast.h, the stage is the kernel of csrc/raycast.hip, torch is plumbing.  All
functions take and return device tensors; there is no CPU fallback.

segment_hits is the entry on device tensors: (n, 3) fp64 UTM end points against the prism height field of a window.

cast_rays casts the rays of a loaded scene: the two end points o + d * near and o + d * far go to UTM through GeoFrame.cloud (the
rays' own near and far columns as the depth: no new geodesy), the segment between the two UTM points is marched, and the contact
parameter s becomes a depth in the rays' units, near + s (far - near).
APPROXIMATION: the ray is straight in ECEF and the march takes it as straight in UTM.  On the fixture scene (tests/golden/scene_small,
rays 69 to 73 m long), measured with the numpy restatements under tests/, the two differ by at most 4.6e-5 m horizontally and
5.8e-6 m in altitude; the curvature bound L^2 / R is 8e-4 m there.  A contact is therefore placed along the true ray to within that
deviation over the sine of the angle between the ray and the surface.

guide_rays narrows the [near, far] of the rays that hit to a band around the hit (eval/utils/util.py guided_lean_inference renders
inside it), view_depth_error compares a rendered depth with the cast depth in metres.

Out of scope: bilinear (non-prism) height fields, a max-mip acceleration of the walk, per-ray sample counts, guiding the training
passes' own sampling.  Which band (front_m, back_m) and which sample count a trained scene needs is UNMEASURED: both stay
required arguments."""
import math
from dataclasses import dataclass

import torch

from ... import _lib
from . import dsm as D
from . import shadow

TOP, WALL, START, END, OUTSIDE, BAD = (_lib.HIT_TOP, _lib.HIT_WALL, _lib.HIT_START, _lib.HIT_END, _lib.HIT_OUTSIDE, _lib.HIT_BAD)
STATES = ("top", "wall", "start", "end", "outside", "bad")
MAX_SEGMENTS = 2 ** 31


@dataclass
class DsmGuide:
    """What guided_lean_inference and extract_pointcloud(guide=) take: the DSM to cast the rays on (`dsm` on `grid`, in `frame`'s UTM
    zone, `bias` metres added to it), the band round the hit in metres along the ray (`front_m`, `back_m`: no defaults) and the
    samples per ray inside it (`n_samples`)."""
    frame: object
    grid: object
    dsm: torch.Tensor
    front_m: float
    back_m: float
    n_samples: int
    bias: float = 0.0


def is_hit(state):
    """the rows whose segment touches the surface: TOP, WALL or START"""
    return state <= START


def _points(p, what):
    if not (torch.is_tensor(p) and p.is_cuda):
        raise ValueError(f"segment_hits: {what} must be a GPU tensor (the HIP path has no CPU fallback)")
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float64:
        raise ValueError(f"segment_hits: {what} must be (n, 3) float64 (east, north, alt), not {tuple(p.shape)} of {p.dtype}")
    return p.contiguous()


@torch.no_grad()
def segment_hits(p0, p1, grid, dsm, bias=0.0, want_cells=False):
    """snerf_dsm_segment_hit: the segments p0 -> p1 ((n, 3) fp64 UTM (east, north, alt) on the GPU) against `dsm` ((H, W) fp32 on the
    GPU, row 0 = the north edge, NaN = a hole) whose lattice is `grid` (a DsmGrid of H x W cells, or a window of one from
    dsm.grid_struct); `bias` metres are added to every cell's height.  Returns (s (n) f64 -- the contact's parameter in [0, 1], NaN
    without one --, state (n) u8 -- TOP, WALL, START, END, OUTSIDE or BAD --[, cell (n) int32 -- j * W + i of the contact cell, -1
    without one]).  One launch on the current stream, no synchronisation."""
    dsm = shadow._dsm(dsm, "segment_hits")
    p0, p1 = _points(p0, "p0"), _points(p1, "p1")
    if p0.shape != p1.shape or p0.device != dsm.device or p1.device != dsm.device:
        raise ValueError(f"segment_hits: p0 {tuple(p0.shape)} and p1 {tuple(p1.shape)} must match and live on the DSM's device")
    n = p0.shape[0]
    if n > MAX_SEGMENTS:
        raise ValueError(f"segment_hits: {n} segments in one call (at most 2^31)")
    g = D.grid_struct(grid)
    if (g.out_h, g.out_w) != tuple(dsm.shape):
        raise ValueError(f"segment_hits: a DSM of {dsm.shape[0]} x {dsm.shape[1]} cells on a window of {g.out_h} x {g.out_w}")
    bias = float(bias)
    if not math.isfinite(bias):
        raise ValueError(f"segment_hits: bias = {bias} must be finite")
    s = torch.empty(n, dtype=torch.float64, device=dsm.device)
    state = torch.empty(n, dtype=torch.uint8, device=dsm.device)
    cell = torch.empty(n, dtype=torch.int32, device=dsm.device) if want_cells else None
    if n:
        _lib.call("snerf_dsm_segment_hit", p0, p1, n, g, dsm, bias, s, state, cell, exc=ValueError)
    return (s, state, cell) if want_cells else (s, state)


def _rays(rays, who, gpu=True):
    if not torch.is_tensor(rays) or (gpu and not rays.is_cuda):
        raise ValueError(f"{who}: the rays must be a GPU tensor (the HIP path has no CPU fallback)")
    if rays.dim() != 2 or rays.shape[1] < 8 or rays.dtype != torch.float32:
        raise ValueError(f"{who}: the rays must be (n, >= 8) float32 (origin, direction, near, far), not {tuple(rays.shape)} of {rays.dtype}")
    return rays


@torch.no_grad()
def cast_rays(rays, frame, grid, dsm, bias=0.0, want_points=False):
    """`rays` ((n, >= 8) fp32, normalised: origin, direction, near, far) of a scene whose GeoFrame is `frame`, against `dsm` on `grid`
    (as for segment_hits, in the frame's UTM zone).  Returns {"depth" (n) f32 -- near + s (far - near), evaluated in fp64 from the
    fp32 columns and rounded once; NaN unless the state is TOP, WALL or START --, "state" (n) u8, "cell" (n) int32[, with
    `want_points`: "points" (hits, 3) f64 -- GeoFrame.cloud(rays, depth) of the hit rows, in their order]}.  The march takes the ray as
    straight in UTM (the module docstring carries the measured deviation)."""
    rays = _rays(rays, "cast_rays").contiguous()
    near, far = rays[:, 6].contiguous(), rays[:, 7].contiguous()
    p0, _ = frame.cloud(rays, near)
    p1, _ = frame.cloud(rays, far)
    s, state, cell = segment_hits(p0, p1, grid, dsm, bias, want_cells=True)
    lo, hi = near.double(), far.double()
    depth = torch.where(is_hit(state), lo + s * (hi - lo), torch.full_like(s, math.nan)).float()
    out = {"depth": depth, "state": state, "cell": cell}
    if want_points:
        rows = is_hit(state)
        out["points"] = (frame.cloud(rays[rows], depth[rows])[0] if bool(rows.any())
                         else torch.empty((0, 3), dtype=torch.float64, device=rays.device))
    return out


def _metres(v, what, who):
    v = float(v)
    if math.isnan(v) or v < 0.0:
        raise ValueError(f"{who}: {what} = {v} must be a distance in metres >= 0 (inf leaves that end alone)")
    return v


def _range(rng, who):
    rng = float(rng)
    if not (math.isfinite(rng) and rng > 0.0):
        raise ValueError(f"{who}: range = {rng} must be the scene's normalisation range in metres, positive and finite")
    return rng


@torch.no_grad()
def guide_rays(rays, cast, front_m, back_m, range):
    """A copy of `rays` whose near and far columns are narrowed to a band round the hit of cast_rays (`cast`): on rows with state TOP,
    WALL or START  near' = max(near, depth - front_m / range), far' = min(far, depth + back_m / range)  (fp32); every other row is
    returned bit for bit.  `front_m`, `back_m`: metres in front of and behind the surface along the ray, required (which band a real
    scene needs is unmeasured); `range`: the normalisation range in metres per unit of depth (GeoFrame.params.range).  Returns (the
    guided rays, the number of guided rows)."""
    rays = _rays(rays, "guide_rays", gpu=False)       # plain torch: it runs where the rays live
    front, back, rng = _metres(front_m, "front_m", "guide_rays"), _metres(back_m, "back_m", "guide_rays"), _range(range, "guide_rays")
    depth, state = cast["depth"], cast["state"]
    if depth.shape[0] != rays.shape[0] or state.shape[0] != rays.shape[0]:
        raise ValueError(f"guide_rays: a cast of {depth.shape[0]} rows for {rays.shape[0]} rays")
    hit = is_hit(state)
    out = rays.clone()
    near, far = rays[:, 6], rays[:, 7]
    out[:, 6] = torch.where(hit, torch.maximum(near, depth - front / rng), near)
    out[:, 7] = torch.where(hit, torch.minimum(far, depth + back / rng), far)
    return out, int(hit.sum())


@torch.no_grad()
def view_depth_error(pred_depth, cast, range):
    """A rendered depth ((n) or (n, 1) f32, e.g. depth_coarse) against the DSM seen through the same rays (`cast` of cast_rays):
    {"mean", "median": |pred - dsm depth| in metres over the hit rows where the prediction is finite (NaN without one), "n": their
    count}"""
    rng = _range(range, "view_depth_error")
    pred = pred_depth.reshape(-1)
    if pred.shape[0] != cast["depth"].shape[0]:
        raise ValueError(f"view_depth_error: {pred.shape[0]} depths against a cast of {cast['depth'].shape[0]} rows")
    rows = is_hit(cast["state"]) & torch.isfinite(pred)
    err = (pred[rows].double() - cast["depth"][rows].double()).abs() * rng
    n = int(err.numel())
    return {"mean": float(err.mean()) if n else math.nan, "median": float(err.median()) if n else math.nan, "n": n}
