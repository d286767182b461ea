"""Bare-earth terrain on the map: a DTM under a DSM, the height above ground nDSM = DSM - DTM and the ground mask -- what a user of
a satellite 3-D model, and DFC2019 with its AGL rasters, ask for.  The reference has no counterpart; the spec is
include/snerf_terrain.h, the stages are the kernels of csrc/terrain.hip, torch is plumbing.  The raster
functions take and return device tensors.

  schedule        the radii and thresholds of a progressive morphological filter (Zhang et al. 2003): windows that double up to the
                  widest building, a threshold that grows with the step of the radius;
  keys            snerf_terrain_keys: altitudes to integer keys and the initial flags (holes; cells blocked by their class);
  opening         snerf_terrain_open: one grey-scale opening of a key plane, with or without the flag update;
  ground_flags    the level loop: every level opens the level before it and flags what stands out by more than its threshold;
  fill            snerf_terrain_fill: the terrain under every cell that is not ground, from the nearest ground W, E, N and S;
  terrain         the four above in one call;
  terrain_agreement   two terrains on one lattice: DTM and nDSM errors, the 2 x 2 table of the ground masks (torch, any device).

Everything the filter writes is integer and the fill's fp64 arithmetic is fixed operation by operation: the planes are
bit-reproducible.  The defaults of `schedule` are parameters, not claims: what a real scene needs is unmeasured."""
import ctypes as C
import math

import torch

from ... import _lib
from . import ortho as OR
from .objects import class_table

HOLE = _lib.TERRAIN_HOLE
MAX_RADIUS = _lib.TERRAIN_MAX_RADIUS
FLAGGED, BLOCKED, IS_HOLE = _lib.TERRAIN_FLAGGED, _lib.TERRAIN_BLOCKED, _lib.TERRAIN_IS_HOLE


def schedule(res, max_window_m=80.0, slope=0.15, dh0=0.3, dh_max=2.5, q=OR.Q):
    """-> (radii, thresholds), two lists of Python ints.  The radii are 1, 2, 4, ... below r_max = ceil(max_window_m / res / 2), then
    r_max (the widest window, 2 r_max + 1 cells, spans max_window_m); the threshold of level k is
    rint(min(dh0 + slope (r_k - r_{k-1}) res, dh_max) / q) keys, with r_0 = 0.  `res`: metres per cell; `slope`: the steepest ground
    (rise over run); dh0, dh_max: metres."""
    res, max_window_m = float(res), float(max_window_m)
    if not (res > 0.0 and math.isfinite(res) and max_window_m > 0.0 and math.isfinite(max_window_m)):
        raise ValueError(f"terrain.schedule: res and max_window_m must be positive and finite, got {res!r} and {max_window_m!r}")
    if not (slope >= 0.0 and dh0 >= 0.0 and dh_max >= 0.0 and q > 0.0):
        raise ValueError(f"terrain.schedule: slope, dh0 and dh_max must be >= 0 and q > 0, got {slope!r}, {dh0!r}, {dh_max!r}, {q!r}")
    r_max = max(1, math.ceil(max_window_m / res / 2))
    if r_max > MAX_RADIUS:
        raise ValueError(f"terrain.schedule: a window of {max_window_m} m at {res} m per cell needs a radius of {r_max} cells; the limit "
                         f"is {MAX_RADIUS} (SNERF_TERRAIN_MAX_RADIUS)")
    radii, r = [], 1
    while r < r_max:
        radii.append(r)
        r *= 2
    radii.append(r_max)
    thresholds, last = [], 0
    for r in radii:
        thresholds.append(int(round(min(dh0 + slope * (r - last) * res, dh_max) / q)))      # round(): half to even, as rint
        last = r
    return radii, thresholds


def _raster(t, dtype, name, shape=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"terrain: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype or t.dim() != 2 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"terrain: {name} must be a 2-D {dtype} raster{'' if shape is None else f' of shape {tuple(shape)}'}, got "
                         f"{t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _sizes(h, w):
    if h * w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"terrain: a raster of {h} x {w} cells: between 1 and 2^31 - 1 cells are taken")


def workspace(h, w, device):
    """the scratch of `opening` and `fill` for an (h, w) raster: snerf_terrain_workspace_bytes bytes on `device`"""
    n = _lib.lib().snerf_terrain_workspace_bytes(int(h), int(w))
    if n < 0:
        _lib.check(1, "snerf_terrain_workspace_bytes", ValueError)
    return torch.empty(n, dtype=torch.uint8, device=device)


def _workspace(ws, h, w, device):
    if ws is None:
        return workspace(h, w, device)
    need = _lib.lib().snerf_terrain_workspace_bytes(int(h), int(w))
    if not (torch.is_tensor(ws) and ws.is_cuda and ws.is_contiguous() and ws.numel() * ws.element_size() >= need):
        raise ValueError(f"terrain: ws must be a contiguous GPU tensor of at least {need} bytes")
    return ws


def keys(alt, label=None, blocked=(), z0=OR.Z0, q=OR.Q):
    """snerf_terrain_keys -> (key (H, W) int32, flags (H, W) uint8, stats (3) int64: altitudes finite but out of key range,
    non-finite altitudes, blocked cells).  `label` (H, W) uint8 with `blocked`, the classes that can never be ground; without a
    label plane no cell is blocked."""
    alt = _raster(alt, torch.float32, "alt")
    h, w = alt.shape
    _sizes(h, w)
    table = None
    if label is not None:
        label = _raster(label, torch.uint8, "label", alt.shape)
        table = class_table(blocked, "blocked")
    elif len(tuple(blocked)):
        raise ValueError("terrain: `blocked` names classes but no label plane was given")
    key = torch.empty((h, w), dtype=torch.int32, device=alt.device)
    flags = torch.empty((h, w), dtype=torch.uint8, device=alt.device)
    stats = torch.zeros(3, dtype=torch.int64, device=alt.device)
    _lib.call("snerf_terrain_keys", alt, label, h, w, table, z0, q, key, flags, stats, exc=ValueError)
    return key, flags, stats


def opening(key, radius, threshold=0, flags=None, out=None, ws=None, stats=None):
    """snerf_terrain_open -> (key_out (H, W) int32, stats (1) int64: the cells newly flagged).  With `flags` ((H, W) uint8, updated in
    place) bit 0 is set where key - key_out > threshold; without, a plain opening.  `out`, `ws`, `stats`: buffers of the caller's."""
    key = _raster(key, torch.int32, "key")
    h, w = key.shape
    _sizes(h, w)
    if int(radius) != radius or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"terrain: radius = {radius!r} outside [1, {MAX_RADIUS}]")
    if int(threshold) != threshold or threshold < 0:
        raise ValueError(f"terrain: threshold = {threshold!r} must be an integer >= 0 (in keys)")
    if flags is not None:
        flags = _raster(flags, torch.uint8, "flags", key.shape)
    out = torch.empty_like(key) if out is None else _raster(out, torch.int32, "out", key.shape)
    if out.data_ptr() == key.data_ptr():
        raise ValueError("terrain: out must not alias key")
    ws = _workspace(ws, h, w, key.device)
    stats = torch.zeros(1, dtype=torch.int64, device=key.device) if stats is None else stats
    _lib.call("snerf_terrain_open", key, h, w, int(radius), int(threshold), out, flags, ws, stats, exc=ValueError)
    return out, stats


def ground_flags(key, flags, radii, thresholds, ws=None):
    """the level loop of the filter: level k opens the surface level k - 1 left (level 1 opens `key`) by radius r_k and flags the
    cells that stood more than threshold_k above the opened surface; two key planes take turns.  `flags` is updated in place.
    -> (flags, per_level: a (levels) int64 tensor of the cells each level newly flagged).  `key` is left as it is."""
    key = _raster(key, torch.int32, "key")
    flags = _raster(flags, torch.uint8, "flags", key.shape)
    if len(radii) != len(thresholds) or not len(radii):
        raise ValueError(f"terrain: {len(radii)} radii and {len(thresholds)} thresholds: one threshold per radius, at least one level")
    h, w = key.shape
    ws = _workspace(ws, h, w, key.device)
    planes = (torch.empty_like(key), torch.empty_like(key))
    per_level = torch.zeros(len(radii), dtype=torch.int64, device=key.device)
    src = key
    for k, (r, t) in enumerate(zip(radii, thresholds)):
        dst = planes[k & 1]
        opening(src, r, t, flags=flags, out=dst, ws=ws, stats=per_level[k:k + 1])
        src = dst
    return flags, per_level


def fill(key, flags, alt, z0=OR.Z0, q=OR.Q, ws=None, reach=True):
    """snerf_terrain_fill -> (dtm (H, W) f32, ndsm (H, W) f32, reach (H, W) int32 or None, stats (3) int64: ground, filled and
    unreachable cells)"""
    key = _raster(key, torch.int32, "key")
    flags = _raster(flags, torch.uint8, "flags", key.shape)
    alt = _raster(alt, torch.float32, "alt", key.shape)
    h, w = key.shape
    _sizes(h, w)
    ws = _workspace(ws, h, w, key.device)
    dtm, ndsm = torch.empty_like(alt), torch.empty_like(alt)
    rch = torch.empty_like(key) if reach else None
    stats = torch.zeros(3, dtype=torch.int64, device=key.device)
    _lib.call("snerf_terrain_fill", key, flags, alt, h, w, z0, q, dtm, ndsm, rch, ws, stats, exc=ValueError)
    return dtm, ndsm, rch, stats


def terrain(alt, grid, label=None, blocked=(), z0=OR.Z0, q=OR.Q, **schedule_kw):
    """The terrain under the altitude plane `alt` ((H, W) f32 on the GPU) of the lattice `grid` (a DsmGrid or a _lib.SnerfDsmGrid
    window: its resolution sets the schedule).  `label` with `blocked`: classes that can never be ground (buildings, say) -- what a
    semantic model adds to a plain ground filter.  **schedule_kw go to schedule().
    -> {"dtm", "ndsm" (H, W) f32, "ground" (H, W) bool, "flags" (H, W) uint8, "reach" (H, W) int32: the distance in cells to the
    nearest ground used, 0 on ground, -1 where no direction finds any, "stats": {"out_of_range", "not_finite", "blocked",
    "flagged_per_level", "ground", "filled", "unreachable"} as Python ints, "schedule": {"radii", "thresholds", "res"}}.
    Reading the stats is the one host synchronisation."""
    res = float(OR.window_grid(grid).resolution)
    radii, thresholds = schedule(res, q=q, **schedule_kw)
    alt = _raster(alt, torch.float32, "alt")
    ws = workspace(*alt.shape, alt.device)
    key, flags, kstats = keys(alt, label, blocked, z0, q)
    flags, per_level = ground_flags(key, flags, radii, thresholds, ws=ws)
    dtm, ndsm, reach, fstats = fill(key, flags, alt, z0, q, ws=ws)
    k, f = [int(v) for v in kstats.cpu()], [int(v) for v in fstats.cpu()]
    return {"dtm": dtm, "ndsm": ndsm, "ground": flags == 0, "flags": flags, "reach": reach,
            "stats": {"out_of_range": k[0], "not_finite": k[1], "blocked": k[2], "flagged_per_level": [int(v) for v in per_level.cpu()],
                      "ground": f[0], "filled": f[1], "unreachable": f[2]},
            "schedule": {"radii": radii, "thresholds": thresholds, "res": res}}


def terrain_agreement(a, b):
    """two terrains ({"dtm", "ndsm", "ground"}, as terrain() returns them) on one lattice, a the model's and b the reference's, over
    the cells where both DTMs are finite -> {"cells", "dtm_mae", "dtm_median_abs", "dtm_bias" (a - b), "ndsm_mae" (over the cells
    where both nDSMs are finite too), "ndsm_cells": fp64 (None without a cell); "ground_table": [[both ground, a only], [b only,
    neither]], "ground_accuracy", "ground_iou": from the integer table (None where the denominator is 0)}.  Plain torch: any device."""
    if tuple(a["dtm"].shape) != tuple(b["dtm"].shape):
        raise ValueError(f"terrain_agreement: the terrains differ in shape: {tuple(a['dtm'].shape)} and {tuple(b['dtm'].shape)}")
    both = torch.isfinite(a["dtm"]) & torch.isfinite(b["dtm"])
    d = (a["dtm"].double() - b["dtm"].double())[both]
    n = int(d.numel())
    out = {"cells": n, "dtm_mae": float(d.abs().mean()) if n else None, "dtm_median_abs": float(d.abs().median()) if n else None,
           "dtm_bias": float(d.mean()) if n else None}
    nb = both & torch.isfinite(a["ndsm"]) & torch.isfinite(b["ndsm"])
    dn = (a["ndsm"].double() - b["ndsm"].double())[nb]
    out["ndsm_cells"] = int(dn.numel())
    out["ndsm_mae"] = float(dn.abs().mean()) if dn.numel() else None
    ga, gb = a["ground"].bool()[both], b["ground"].bool()[both]
    tt, tf, ft, ff = (int((x & y).sum()) for x, y in ((ga, gb), (ga, ~gb), (~ga, gb), (~ga, ~gb)))
    out["ground_table"] = [[tt, tf], [ft, ff]]
    out["ground_accuracy"] = (tt + ff) / n if n else None
    out["ground_iou"] = tt / (tt + tf + ft) if tt + tf + ft else None
    return out
