"""Digital surface model (DSM) and its altitude MAE on the device -- the reference's eval/utils/dsm.py:40-266 and
eval/utils/dsmr.py, from an (E, N, alt) point cloud to {"mean", "median"}.  Every stage is a HIP kernel of csrc/dsm.hip;
torch is plumbing (allocation, masks, the median's selection).  All functions take and return device tensors.

Rasterisation -- plyflatten(cloud, xoff, yoff, res, xsize, ysize, radius=1, sigma=inf) as dsm.py:75-77 calls it.  A point
(x, y, z) has the cell i = floor((x - xoff)/res), j = floor((yoff - y)/res) (fp64, row 0 at the north edge) and adds z with
weight 1 to every cell (i+kx, j+ky), |kx|, |ky| <= radius, inside the grid, also when its own cell lies outside; a cell is the
mean of what it received, NaN if nothing; float32 (ysize, xsize).  The kernel accumulates round((z - Z0)/Q) in int64 and
the count in u32 per cell with integer atomics and writes f32(Z0 + Q*sum/count): the DSM is bit-reproducible run to run, and
data-parallel ranks combine exactly by a SUM all-reduce of the accumulators.  Z0 and Q are constants (not taken from the
data, so all ranks agree); |z - Z0| is off its exact value by at most Q/2 = 3e-8 before the fp32 rounding.  Accumulator
overflow raises OverflowError, it never wraps.  plyflatten (a C extension) is not available here: parity with it is
UNPINNED; the tests pin the kernels to the spec through a numpy restatement.  Finite `sigma` is out of scope (the reference
only ever passes inf).  Which cells a point reaches is cell_window() of csrc/lattice.h, shared with the ortho products
(eval/utils/ortho.py), which also go through grid_struct, cloud_f64, cell_count and new_stats below.

Grids -- the cloud-bounds grid of create_dsm without roi_txt (dsm.py:66-72, resolution 0.5) and the ROI grid of the
roi_txt arithmetic (dsm.py:58-63: xsize = ysize = int(meta[2]), the ROI is square; yoff += size * res).

MAE -- compute_dsm_and_mae_from_latlon -> compute_mae (dsm.py:112-266).  The reference rasterises on the bounds grid and gdal
crops it to the ROI; here the ROI is rasterised directly with the cell indices of the bounds lattice shifted by the integer
ROI offset, which equals "bounds grid, then crop" bit for bit (points outside the ROI still feed its edge cells, cells outside
the bounds grid receive nothing).  DIVERGENCE: an ROI corner off that lattice (by more than 1e-6 res) or an ROI resolution
other than the DSM's raises ValueError where gdal would resample (a cloud is rasterised on the lattice asked for, never resampled; a
ground-truth RASTER on another lattice is warped by eval/utils/warp.py when the loader is given resample=).  ROI cells beyond the cloud are NaN.  The prediction is set
to NaN where the water mask is 9 or the ignore mask is non-zero, BEFORE registration (dsm.py:205-224).  Registration is
dsmr.compute_shift(gt, pred, scaling=False) + apply_shift on the RAW cropped ground truth (compute_shift reads the gdal crop
from disk, dsm.py:236); the difference uses the ground truth with values below -500 set to 0 (not NaN, dsm.py:229-231).

Registration (dsmr.py:6-250) -- recursive_ncc: while min(H, W) > 100 recurse on downsample2x of both images with the search
centre floor-halved (Python //), double the result on the way up; every level searches (dx, dy) in centre +- irange, y
outer, x inner, a strict > against a maximum starting at -inf (the first maximum wins, a NaN correlation never wins).
downsample2x copies the reference's off-by-one: out[J, I] is the NaN-aware mean of u[j:j+2, i:i+2] at j = min(2J+1, H-1),
i = min(2I+1, W-1) (the loop's last write wins), size ceil(H/2) x ceil(W/2), fp64 below level 0.  NCC = mean_std in fp64
over the pixels where u[j, i] and v[j+dy, i+dx] are both finite (out of range = NaN), two passes (means, then centred
sums), sig = sqrt(sum/count), ncc = xcorr/(sigu sigv); a zero variance gives 0 (the reference catches ZeroDivisionError); an
empty overlap raises ("The predicted DSM is all NaN").  One small read-back per level picks the argmax on the host.
apply_shift: b = muu - muv at the chosen shift (a = 1), rdsm[j, i] = f32(v[j+dy, i+dx] + b), NaN out of range.
MAE: diff = rdsm - gt; mean = nanmean|diff| (fp64 sum, fixed order), median = nanmedian|diff| as numpy takes it (the mean of
the two middle values for an even count).  The reference formats both with "{:.3f}"; the raw floats are returned.

World clouds (dsm.py:18-36,105-110) -- with `geo` (a GeoFrame, framework/components/coordinate_systems.py: the loader puts
one into every image's "dsm" entry) compute_dsm_and_mae turns rays and depth into the UTM (east, north, alt) cloud in ONE launch
of csrc/geo.hip, which also folds the cloud's east / north bounds; create_dsm and dsm_grid_from_cloud take those `bounds` and
run no reduction of their own.  The bounds are exact (integer atomic min / max), so the DSM is bit for bit the one of the same
cloud without them.  get_utm_cloud and create_dsm_cloud_from_nerf mirror the reference's helpers on device tensors.  The UTM
series is the `utm` package's, restated; parity with the package is UNPINNED.  DIVERGENCE: the fused path
uses the scene's zone (root.json), the reference the zone of the cloud's first point.  Without `geo` the cloud comes in a metric
east/north/up frame as before, optionally through a caller's `to_world(xyz_n) -> (E, N, alt)`.

Out of scope: writing error GeoTIFFs (arrays out; eval/ortho.py writes the DSM of a fused map as a GeoTIFF, the ground truth is
READ by framework/util/img_utils.py); training in
the UTM coordinate system; the Norway / Svalbard UTM zone exceptions.  An off-lattice ROI of create_dsm raises ValueError; an off-lattice
ground truth raises unless resample= is given (framework/util/img_utils.py, eval/utils/warp.py mae_between).  SSIM is eval/utils/metrics.py; eval/eval_nerf.py reports PSNR, SSIM and this MAE per image."""
import math
from collections import namedtuple

import torch

from ... import _lib
from ...parallel import allreduce_, world

Z0 = 0.0            # quantisation origin of the rasteriser's integer accumulators (metres)
Q = 2.0 ** -24      # quantisation step (metres): 6e-8, below the fp32 spacing of any altitude above 0.5
RESOLUTION = 0.5    # create_dsm's resolution without roi_txt (dsm.py:65)
IRANGE = 5          # recursive_ncc's search radius (dsmr.py:134)

DsmGrid = namedtuple("DsmGrid", "xoff yoff resolution xsize ysize")


# ---- grids -----------------------------------------------------------------------------------------------------------------
def dsm_grid_from_cloud(cloud, resolution=RESOLUTION, distributed=False, bounds=None):
    """create_dsm's cloud-bounds grid (dsm.py:66-72).  `distributed`: the bounds of the union of every rank's cloud.
    `bounds`: the cloud's (xmin, xmax, ymin, ymax) when the caller already holds them (GeoFrame's fused launch): no reduction
    over the cloud runs here."""
    import torch.distributed as dist
    if bounds is not None and not (distributed and world()[1] > 1):
        xmin, xmax, ymin, ymax = (float(v) for v in bounds)
    else:
        if bounds is not None:
            ext = torch.tensor([-bounds[0], bounds[1], -bounds[2], bounds[3]], dtype=torch.float64, device=cloud.device)
        elif cloud.shape[0]:
            c = cloud.double()
            ext = torch.stack([-c[:, 0].min(), c[:, 0].max(), -c[:, 1].min(), c[:, 1].max()])
        else:
            ext = torch.full((4,), -math.inf, dtype=torch.float64, device=cloud.device)
        if distributed:
            allreduce_(ext, dist.ReduceOp.MAX)
        xmin, xmax, ymin, ymax = (-float(ext[0]), float(ext[1]), -float(ext[2]), float(ext[3]))
    if not all(math.isfinite(v) for v in (xmin, xmax, ymin, ymax)):
        raise ValueError("dsm_grid_from_cloud: the cloud is empty or not finite")
    xoff = math.floor(xmin / resolution) * resolution
    xsize = int(1 + math.floor((xmax - xoff) / resolution))
    yoff = math.ceil(ymax / resolution) * resolution
    ysize = int(1 - math.floor((ymin - yoff) / resolution))
    return DsmGrid(xoff, yoff, resolution, xsize, ysize)


def roi_grid(meta):
    """the roi_txt grid (dsm.py:58-63): meta = (xoff, yoff, size, resolution); square, yoff moved to the north edge"""
    meta = [float(m) for m in (meta.tolist() if hasattr(meta, "tolist") else meta)][:4]
    xoff, yoff, size, res = meta
    n = int(size)
    return DsmGrid(xoff, yoff + n * res, res, n, n)


# ---- rasterisation -----------------------------------------------------------------------------------------------------------
def grid_struct(lattice, window=None):
    """a DsmGrid cropped to window = (ioff, joff, out_w, out_h) (the whole extent without one), or a ready _lib.SnerfDsmGrid
    (a window of a lattice), -> _lib.SnerfDsmGrid"""
    if isinstance(lattice, _lib.SnerfDsmGrid):
        return lattice
    ioff, joff, w, h = window if window is not None else (0, 0, lattice.xsize, lattice.ysize)
    return _lib.SnerfDsmGrid(float(lattice.xoff), float(lattice.yoff), float(lattice.resolution), int(lattice.xsize),
                             int(lattice.ysize), int(ioff), int(joff), int(w), int(h))


def cell_count(g, what="DSM"):
    """out_h * out_w of a _lib.SnerfDsmGrid; the accumulators of a window are indexed with 31 bits"""
    if g.out_h * g.out_w > 2 ** 31 - 1:
        raise ValueError(f"{what} of {g.out_h} x {g.out_w} cells is too large")
    return g.out_h * g.out_w


def cloud_f64(cloud):
    """the (N, 3) (east, north, alt) cloud as the kernels of the lattice read it: fp64, contiguous"""
    xyz = cloud.to(torch.float64).contiguous()
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("the cloud must be (N, 3)")
    return xyz


def new_stats(device):
    """a zeroed stats block (4 u64 words, held as int64)"""
    return torch.zeros(4, dtype=torch.int64, device=device)


def _accumulate(cloud, lattice, window, radius, acc=None):
    """integer accumulators (count i32-as-u32, sum i64) and stats (u64[4]) of `cloud` on `lattice` cropped to
    window = (ioff, joff, out_w, out_h) (see grid_struct); `acc`: the (count, total, stats) of earlier calls to go on adding to"""
    g = grid_struct(lattice, window)
    cells = cell_count(g)
    xyz = cloud_f64(cloud)
    if acc is None:
        acc = (torch.zeros(cells, dtype=torch.int32, device=xyz.device), torch.zeros(cells, dtype=torch.int64, device=xyz.device),
               new_stats(xyz.device))
    count, total, stats = acc
    _lib.call("snerf_dsm_accumulate", xyz, xyz.shape[0], g, radius, Z0, Q, count, total, stats)
    return count, total, stats


def _finish(count, total, stats, h, w):
    dsm = torch.empty(h * w, dtype=torch.float32, device=count.device)
    _lib.call("snerf_dsm_finish", count, total, h * w, Z0, Q, dsm, stats)
    kmax, bad, cmax, _ = (int(x) for x in stats.cpu())
    if bad:
        raise OverflowError(f"rasterize: {bad} point(s) with an altitude that is not finite or beyond 2^62 quantisation steps")
    if kmax * cmax >= 2 ** 63:
        raise OverflowError(f"rasterize: int64 cell sums could overflow (max |z - z0|/q = {kmax}, max count = {cmax})")
    return dsm.view(h, w)


def _rasterize_window(cloud, lattice, window, radius, distributed):
    count, total, stats = _accumulate(cloud, lattice, window, radius)
    if distributed:
        allreduce_(count)
        allreduce_(total)
        allreduce_(stats)   # summed maxima bound the global maximum: a conservative overflow check
    return _finish(count, total, stats, window[3], window[2])


def rasterize(cloud, grid, radius=1, distributed=False):
    """plyflatten(cloud, *grid, radius, sigma=inf) -> float32 (ysize, xsize), NaN where no point reached.
    `distributed`: every rank passes its own points and receives the DSM of their union (a collective)."""
    if radius < 0:
        raise ValueError("radius must be >= 0")
    return _rasterize_window(cloud, grid, (0, 0, grid.xsize, grid.ysize), radius, distributed)


def create_dsm(cloud, roi=None, resolution=RESOLUTION, radius=1, distributed=False, bounds=None):
    """create_dsm (dsm.py:40-109) on an (E, N, alt) cloud: the cloud-bounds grid, or, with `roi` (a DsmGrid from roi_grid,
    or the roi_txt meta), that grid cropped to the ROI as compute_mae's gdal crop does (see the module docstring).
    `bounds`: the cloud's precomputed (xmin, xmax, ymin, ymax), see dsm_grid_from_cloud."""
    bounds = dsm_grid_from_cloud(cloud, resolution, distributed, bounds=bounds)
    if roi is None:
        return rasterize(cloud, bounds, radius, distributed)
    if not isinstance(roi, DsmGrid):
        roi = roi_grid(roi)
    res = bounds.resolution
    if abs(roi.resolution - res) > 1e-9 * res:
        raise ValueError(f"ROI resolution {roi.resolution} != DSM resolution {res}: resampling is not supported")
    fi, fj = (roi.xoff - bounds.xoff) / res, (bounds.yoff - roi.yoff) / res
    ioff, joff = round(fi), round(fj)
    if abs(fi - ioff) > 1e-6 or abs(fj - joff) > 1e-6:
        raise ValueError(f"ROI corner ({roi.xoff}, {roi.yoff}) is off the DSM lattice ({bounds.xoff} + k {res}, "
                         f"{bounds.yoff} - k {res}): resampling is not supported")
    return _rasterize_window(cloud, bounds, (ioff, joff, roi.xsize, roi.ysize), radius, distributed)


# ---- registration ------------------------------------------------------------------------------------------------------------
def _image(t):
    if t.dim() != 2:
        raise ValueError("DSMs are 2-d (H, W) tensors")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.float()
    return t.contiguous()


def downsample2x(u):
    """dsmr.downsample2x (dsmr.py:17-47) of an (H, W) image -> float64 (ceil(H/2), ceil(W/2))"""
    u = _image(u)
    h, w = u.shape
    out = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.float64, device=u.device)
    _lib.call("snerf_dsm_downsample2x", u, u.dtype == torch.float64, h, w, out)
    return out


def _workspace(h, w, radius, device):
    return torch.empty(_lib.call_size("snerf_dsm_workspace_bytes", h, w, radius, exc=ValueError), dtype=torch.uint8, device=device)


def _shift_stats(u, v, cx, cy, radius):
    """host (S, 6) float64: (count, sum u, sum v, centred sum u^2, v^2, uv) of every shift of the window, y outer"""
    if u.dtype != v.dtype:
        v = v.to(u.dtype)
    h, w = u.shape
    S = (2 * radius + 1) ** 2
    stats = torch.empty((S, 6), dtype=torch.float64, device=u.device)
    ws = _workspace(h, w, radius, u.device)
    _lib.call("snerf_dsm_ncc_search", u, v, u.dtype == torch.float64, h, w, cx, cy, radius, stats, ws, ws.numel())
    return stats.cpu().tolist()


def _ncc(row):
    count, su, sv, suu, svv, suv = row
    if count == 0:
        raise RuntimeError("The predicted DSM is all NaN")
    sigu, sigv = math.sqrt(suu / count), math.sqrt(svv / count)
    den = sigu * sigv
    return 0.0 if den == 0.0 else (suv / count) / den


def compute_ncc(u, v, irange, initdx, initdy):
    """dsmr.compute_ncc: the (dx, dy) of centre +- irange maximising the NCC (first maximum, y outer, x inner)"""
    rows = _shift_stats(u, v, initdx, initdy, irange)
    best, dx, dy = -math.inf, initdx, initdy
    n = 2 * irange + 1
    for s, row in enumerate(rows):
        c = _ncc(row)
        if c > best:
            best, dx, dy = c, initdx - irange + s % n, initdy - irange + s // n
    return dx, dy


def recursive_ncc(u, v, irange=IRANGE, dx=0, dy=0, trace=None):
    """dsmr.recursive_ncc (dsmr.py:127-144); `trace` (a list) receives (h, w, initdx, initdy, dx, dy) per level, coarse first"""
    u, v = _image(u), _image(v)
    levels = [(u, v)]
    while min(levels[-1][0].shape) > 100:
        levels.append((downsample2x(levels[-1][0]), downsample2x(levels[-1][1])))
    centres = [(dx, dy)]
    for _ in levels[1:]:
        centres.append((centres[-1][0] // 2, centres[-1][1] // 2))
    cx, cy = centres[-1]
    for k in range(len(levels) - 1, -1, -1):
        lu, lv = levels[k]
        ix, iy = cx, cy
        fx, fy = compute_ncc(lu, lv, irange, cx, cy)
        if trace is not None:
            trace.append((lu.shape[0], lu.shape[1], ix, iy, fx, fy))
        cx, cy = (2 * fx, 2 * fy) if k else (fx, fy)
    return cx, cy


def compute_shift(gt, pred, irange=IRANGE, init=(0, 0), trace=None):
    """dsmr.compute_shift(gt, pred, scaling=False) on arrays -> (dx, dy, a, b), with b = muu - muv at the shift found"""
    u, v = _image(gt), _image(pred)
    dx, dy = recursive_ncc(u, v, irange, init[0], init[1], trace)
    count, su, sv = _shift_stats(u, v, dx, dy, 0)[0][:3]
    if count == 0:
        raise RuntimeError("The predicted DSM is all NaN")
    return dx, dy, 1, su / count - sv / count


def _shift_diff(pred, gt, dx, dy, b, want_rdsm=True, want_diff=True):
    pred, gt = _image(pred).float(), _image(gt).float()
    if pred.shape != gt.shape:
        raise ValueError("prediction and ground truth must have the same shape")
    h, w = pred.shape
    rdsm = torch.empty_like(pred) if want_rdsm else None
    diff = torch.empty_like(pred) if want_diff else None
    totals = torch.empty(2, dtype=torch.float64, device=pred.device)
    ws = _workspace(h, w, 0, pred.device)
    _lib.call("snerf_dsm_shift_diff", pred, gt, h, w, dx, dy, b, rdsm, diff, totals, ws, ws.numel())
    return rdsm, diff, totals


def apply_shift(pred, dx=0, dy=0, a=1, b=0.0):
    """dsmr.apply_shift_ with c = d = 0: out[j, i] = f32(a * pred[j+dy, i+dx] + b); only a = 1 (scaling=False)"""
    if a != 1:
        raise ValueError("apply_shift: only a = 1 (the reference's scaling=False) is supported")
    pred = _image(pred).float()
    rdsm, _, _ = _shift_diff(pred, pred, dx, dy, b, want_diff=False)
    return rdsm


def nanmedian_numpy(x):
    """numpy's nanmedian of a float32 tensor: the mean of the two middle values when the finite count is even"""
    a = x[torch.isfinite(x)].reshape(-1)
    n = a.numel()
    if n == 0:
        return math.nan
    lo = torch.kthvalue(a, (n + 1) // 2).values
    if n % 2:
        return float(lo)
    hi = torch.kthvalue(a, n // 2 + 1).values
    return float((lo + hi) / 2)


def compute_mae(pred_dsm, gt_dsm, water_mask=None, ignore_mask=None, init=(0, 0)):
    """compute_mae (dsm.py:160-266) on arrays of the ROI: {"mean", "median", "dx", "dy", "b", "rdsm", "diff"}"""
    pred, gt = _image(pred_dsm).float(), _image(gt_dsm).float()
    if pred.shape != gt.shape:
        raise ValueError(f"predicted DSM {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ in shape")
    nan = torch.tensor(float("nan"), device=pred.device)
    if water_mask is not None:
        pred = torch.where(water_mask.to(pred.device) == 9, nan, pred)
    if ignore_mask is not None:
        pred = torch.where(ignore_mask.to(pred.device) != 0, nan, pred)
    dx, dy, _, b = compute_shift(gt, pred, init=init)
    rdsm, diff, totals = _shift_diff(pred, gt, dx, dy, b)
    s, n = totals.cpu().tolist()
    return {"mean": s / n if n else math.nan, "median": nanmedian_numpy(diff.abs()), "dx": dx, "dy": dy, "b": b,
            "rdsm": rdsm, "diff": diff}


def get_utm_cloud(lats, lons, alts):
    """get_utm_cloud (dsm.py:18-30) on device tensors: ((N, 3) f64 (east, north, alt), zone_string), the zone taken from the
    first point as the reference's utm_from_latlon without a zone does"""
    from ...framework.util.conversions import utm_from_latlon
    easts, norths, zone_string = utm_from_latlon(lats, lons)
    return torch.stack([easts, norths, alts.double()], 1), zone_string


def create_dsm_cloud_from_nerf(dataset, rays, depths):
    """create_dsm_cloud_from_nerf (dsm.py:33-36): the UTM cloud of a frame, one launch through the dataset's GeoFrame (the
    scene's zone; see the module docstring)"""
    return dataset._need_geo().cloud(rays, depths)[0]


def compute_dsm_and_mae(rays, depth, gt_dsm, roi_meta, to_world=None, water_mask=None, ignore_mask=None,
                        resolution=RESOLUTION, radius=1, distributed=None, geo=None):
    """compute_dsm_and_mae (dsm.py:112-157) without files: rays + depth -> xyz (get_xyz_from_nerf_prediction, fp64) ->
    to_world (identity by default) -> the DSM on the ROI -> compute_mae.  Returns the MAE dict plus "dsm".
    `geo` (a GeoFrame; excludes to_world): fp32 rays and depth -> the UTM cloud and its bounds in one launch instead.
    `distributed` (default: whenever a process group of more than one rank is up): each rank passes its own rays and the
    integer accumulators are all-reduced, so every rank gets the same DSM and MAE (a collective)."""
    from ..extract_pointcloud import get_xyz_from_nerf_prediction
    bounds = None
    if geo is not None:
        if to_world is not None:
            raise ValueError("compute_dsm_and_mae: pass either geo or to_world, not both")
        cloud, bounds = geo.cloud(rays, depth)
    else:
        xyz = get_xyz_from_nerf_prediction(rays.reshape(-1, rays.shape[-1]), depth.reshape(-1))
        cloud = to_world(xyz) if to_world is not None else xyz
    if distributed is None:
        distributed = world()[1] > 1
    dsm = create_dsm(cloud.to(torch.float64), roi=roi_grid(roi_meta), resolution=resolution, radius=radius,
                     distributed=distributed, bounds=bounds)
    out = compute_mae(dsm, gt_dsm, water_mask=water_mask, ignore_mask=ignore_mask)
    out["dsm"] = dsm
    return out
