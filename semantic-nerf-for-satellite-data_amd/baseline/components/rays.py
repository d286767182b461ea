"""Ray construction of the scene loaders -- mirror of baseline/components/rays.py.  satnerf_construct builds the rays of
every image of a split in ONE launch of csrc/satrays.hip (snerf_rpc_rays): per pixel, rpcm localisation at max_alt and at
min_alt, custom ECEF in fp64, and the un-normalised fp32 row [o(3), d(3), near = 0, far] that the reference returns after
`.type(FloatTensor)`.

nadir_construct casts one VERTICAL ray per cell of a map lattice (a DsmGrid of eval/utils/dsm.py): from the cell centre at max_alt
straight down to min_alt, taken into the scene by GeoFrame.to_scene (csrc/geo.hip, direction 1).  The
reference has no counterpart; its rays are already normalised, ready for the renderer."""
import numpy as np
import torch

from ... import _lib
from .camera_models import RPCModel, struct_to_device


def construct_sun_dir(sun_elevation_deg: float, sun_azimuth_deg: float, n_rays: int) -> torch.Tensor:
    """(n_rays, 3) fp32 unit sun direction (east, north, up components), evaluated in fp64 and rounded once"""
    el, az = np.deg2rad(np.array([sun_elevation_deg, sun_azimuth_deg], dtype=np.float64))
    horizontal = np.cos(el)
    unit = np.array([np.sin(az) * horizontal, np.cos(az) * horizontal, np.sin(el)], dtype=np.float64).astype(np.float32)
    return torch.from_numpy(unit).reshape(1, 3).expand(n_rays, 3).contiguous()


class LocalizationError(RuntimeError):
    """rpcm's MaxLocalizationIterationsError: a pixel of the named image did not converge in 100 iterations"""


def satnerf_construct(cameras, min_alts, max_alts, sizes=None, pixels=None, names=None, device=None, check=True):
    """Rays of several images, concatenated in order, as one (R, 8) fp32 tensor on `device`.
    cameras: RPCModel per image; sizes: (w, h) per image (grid: ray i at row = i // w, col = i % w, the reference's
    np.meshgrid(arange(w), arange(h)) flattened) -- or pixels: one (n_k, 2) fp64 (col, row) array per image (keypoints).
    check: read back the per-image count of points that did not converge and raise LocalizationError naming the image
    (the one host synchronisation; check=False returns (rays, counters) and leaves the read to the caller: raise_on_failures)."""
    n_img = len(cameras)
    if n_img == 0:
        raise ValueError("satnerf_construct: no image")
    if (sizes is None) == (pixels is None):
        raise ValueError("satnerf_construct: pass either sizes (pixel grids) or pixels (explicit coordinates)")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    table = (_lib.SnerfRayImage * n_img)()
    row0 = 0
    pix = None
    if pixels is not None:
        pix = torch.from_numpy(np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in pixels], 0)).to(device)
    for k, cam in enumerate(cameras):
        e = table[k]
        e.rpc = cam.struct if isinstance(cam, RPCModel) else cam
        e.min_alt, e.max_alt = float(min_alts[k]), float(max_alts[k])
        if sizes is not None:
            w, h = int(sizes[k][0]), int(sizes[k][1])
            e.w, e.h, n = w, h, w * h
        else:
            n = int(np.asarray(pixels[k]).reshape(-1, 2).shape[0])
        e.row0, e.n_rays = row0, n
        row0 += n
    rays = torch.empty((row0, 8), dtype=torch.float32, device=device)
    fails = torch.zeros(3 * n_img, dtype=torch.int32, device=device)     # failures per image, then update counts
    _lib.call("snerf_rpc_rays", table, struct_to_device(table, device), n_img, pix, row0, rays, fails)
    if not check:
        return rays, fails
    raise_on_failures(fails, names)
    return rays


def raise_on_failures(fails: torch.Tensor, names=None):
    f = fails.cpu().numpy()[: len(fails) // 3]
    bad = np.nonzero(f)[0]
    if len(bad):
        k = int(bad[0])
        who = names[k] if names is not None else f"#{k}"
        raise LocalizationError(f"image {who}: {int(f[k])} pixels did not converge in 100 RPC localisation iterations "
                                "(rpcm: MaxLocalizationIterationsError)")


def nadir_cell_centres(grid, device=None):
    """(east (H, W), north (H, W)) fp64 tensors on `device` (default: the CPU) of the cell centres of `grid` -- a DsmGrid, or a
    window of one as eval/utils/dsm.py grid_struct makes it.  Cell (j, i) of the window has its centre at
    E = xoff + (ioff + i + 1/2) res, N = yoff - (joff + j + 1/2) res: row 0 is the north edge, the convention of csrc/lattice.h."""
    from ...eval.utils.dsm import grid_struct
    g = grid_struct(grid)
    i = torch.arange(g.out_w, dtype=torch.float64, device=device) + float(g.ioff)
    j = torch.arange(g.out_h, dtype=torch.float64, device=device) + float(g.joff)
    east = g.xoff + (i + 0.5) * g.res
    north = g.yoff - (j + 0.5) * g.res
    return east.reshape(1, -1).expand(g.out_h, g.out_w), north.reshape(-1, 1).expand(g.out_h, g.out_w)


def nadir_construct(grid, geo, min_alt, max_alt, device=None, want_bounds=False):
    """One vertical ray per cell of `grid` (see nadir_cell_centres), row-major over the lattice: (H * W, 8) fp32, contiguous,
    [o(3), d(3), near = 0, far] in `geo`'s normalised scene coordinates -- o is the cell centre at max_alt, o + far * d the cell
    centre at min_alt.  The 2 H W points (E, N, max_alt), (E, N, min_alt) go through ONE GeoFrame.to_scene launch; d = p_bot -
    p_top and its norm are fp64 torch ops on the device, rounded once to fp32.  `want_bounds`: also return the GeoBounds of the
    points' scene x / y (a lattice inside the normalised box stays within about [-1, 1])."""
    from ...eval.utils.dsm import grid_struct
    min_alt, max_alt = float(min_alt), float(max_alt)
    if not min_alt < max_alt:
        raise ValueError(f"nadir_construct: min_alt = {min_alt} must lie below max_alt = {max_alt}")
    g = grid_struct(grid)
    if g.out_h <= 0 or g.out_w <= 0:
        raise ValueError(f"nadir_construct: the lattice is empty ({g.out_h} x {g.out_w} cells)")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    east, north = (t.reshape(-1) for t in nadir_cell_centres(g, device))
    cells = east.shape[0]
    pts = torch.empty((2, cells, 3), dtype=torch.float64, device=device)
    pts[:, :, 0] = east
    pts[:, :, 1] = north
    pts[0, :, 2] = max_alt
    pts[1, :, 2] = min_alt
    xyz, bounds = geo.to_scene(pts.reshape(-1, 3))
    top, bot = xyz[:cells], xyz[cells:]
    d = bot - top
    norm = torch.linalg.vector_norm(d, dim=1, keepdim=True)
    rays = torch.cat([top, d / norm, torch.zeros_like(norm), norm], 1).to(torch.float32).contiguous()
    return (rays, bounds) if want_bounds else rays


def nadir_extras(sun_elevation_deg: float, sun_azimuth_deg: float, t, n_rays: int, device=None) -> torch.Tensor:
    """(n_rays, 4) fp32 extras of nadir rays, the loaders' columns: the sun direction and the constant embedding index `t`"""
    sun = construct_sun_dir(sun_elevation_deg, sun_azimuth_deg, n_rays)
    return torch.hstack([sun, float(t) * torch.ones(n_rays, 1)]).to(device).contiguous()
