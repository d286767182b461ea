"""Solar potential on the map: how much sun every cell, roof facet and building of a DSM gets -- sun hours, sky view and insolation.
The reference has no counterpart; the spec is include/snerf_solar.h, the device stages are the kernels of
csrc/solar.hip, torch is plumbing.  The device stages take and return device tensors; there is no CPU fallback for them.

The method is the horizon map of GRASS r.horizon / r.sun: horizon() marches once per cell and azimuth sector over the height field (the
walk of cast_shadows, fp64) and keeps the steepest slope seen, in metres per cell of horizontal travel -- the unit of a sun row's
`rise`.  A sun is visible from a cell iff its rise is at least the horizon slope at its azimuth, interpolated linearly between the two
neighbouring sectors: D = 64 marches replace one march per sun of a year.  For a sun exactly on a sector the test IS the cast shadow
(tests/test_solar_cpu.py holds the two restatements to each other); between sectors it is an approximation whose disagreement with
cast_shadows is measured by tools/solar_timing.py.  sky_view() is the cosine-weighted sky-view factor of a horizontal surface from
the same planes; irradiate() sums weight * cos(incidence) over the visible suns on the surface the slopes describe.

Suns from dates: sun_position() evaluates NOAA's general solar position series (fractional year -> equation of time and declination
-> hour angle -> elevation and azimuth) in numpy fp64, without refraction; its (elevation_deg, azimuth_deg) pairs are the `suns` of
cast_shadows, nadir_sun_sweep, export_sun_sweep and export_shadow_check.  pvlib, astral, ephem, skyfield and astropy are not among
this project's dependencies: parity with them is UNPINNED; tests/test_solar_cpu.py holds the series to astronomy (solstice
declinations, the extremes of the equation of time, the equinoxes, solar noon).  clear_sky() is a simple published clear-sky rule
(Kasten-Young air mass, Meinel's direct normal irradiance, the diffuse part a fixed share of it); its coefficients are parameters, not
claims, and every consumer takes caller-supplied weights instead -- a typical-meteorological-year series, say.

Out of scope: refraction, reflected irradiance and anisotropic-sky diffuse models, measured weather, a per-cell sun position (one
position serves the map), soft shadows, a max-mip or line-sweep horizon, rank-sharded rasters, PV module models and panel layout."""
import ctypes as C
import datetime
import math

import numpy as np
import torch

from ... import _lib
from .shadow import _dsm

MAX_DIRS = _lib.SOLAR_MAX_DIRS
MAX_SECTORS = _lib.SOLAR_MAX_SECTORS
MAX_SUNS = _lib.SOLAR_MAX_SUNS
QUANT = 2.0 ** 16          # solar_table adds values quantised to 2^-16 of their unit
SNAP = 1e-9                # sun_table: a sun this close (in sectors) to a sector stands on it


# ---- suns from dates ----------------------------------------------------------------------------------------------------------------
def _utc_fields(when):
    """datetimes -> (year, day of year from 1, hours of the UTC day) as arrays; a naive datetime counts as UTC"""
    single = isinstance(when, datetime.datetime)
    out = []
    for t in ([when] if single else list(when)):
        if t.tzinfo is not None:
            t = t.astimezone(datetime.timezone.utc).replace(tzinfo=None)
        out.append((t.year, t.timetuple().tm_yday, t.hour + t.minute / 60.0 + (t.second + t.microsecond * 1e-6) / 3600.0))
    a = np.asarray(out, np.float64).reshape(-1, 3)
    return a[:, 0].astype(np.int64), a[:, 1], a[:, 2], single


def _days_in(year):
    year = np.asarray(year)
    return np.where((year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0)), 366.0, 365.0)


def solar_terms(year, day_of_year, hours):
    """NOAA's general solar position series: -> (declination_deg, equation_of_time_min) at `hours` UTC of day `day_of_year` (from 1)"""
    g = 2.0 * np.pi / _days_in(year) * (np.asarray(day_of_year, np.float64) - 1.0 + (np.asarray(hours, np.float64) - 12.0) / 24.0)
    eqtime = 229.18 * (0.000075 + 0.001868 * np.cos(g) - 0.032077 * np.sin(g) - 0.014615 * np.cos(2 * g) - 0.040849 * np.sin(2 * g))
    decl = (0.006918 - 0.399912 * np.cos(g) + 0.070257 * np.sin(g) - 0.006758 * np.cos(2 * g) + 0.000907 * np.sin(2 * g)
            - 0.002697 * np.cos(3 * g) + 0.00148 * np.sin(3 * g))
    return np.rad2deg(decl), eqtime


def _position(year, doy, hours, lat_deg, lon_deg):
    decl_deg, eqtime = solar_terms(year, doy, hours)
    decl, lat = np.deg2rad(decl_deg), math.radians(float(lat_deg))
    ha = np.deg2rad((hours * 60.0 + eqtime + 4.0 * float(lon_deg)) / 4.0 - 180.0)      # true solar time (minutes) -> hour angle
    up = math.sin(lat) * np.sin(decl) + math.cos(lat) * np.cos(decl) * np.cos(ha)
    east = -np.cos(decl) * np.sin(ha)
    north = math.cos(lat) * np.sin(decl) - math.sin(lat) * np.cos(decl) * np.cos(ha)
    return np.rad2deg(np.arcsin(np.clip(up, -1.0, 1.0))), np.rad2deg(np.arctan2(east, north)) % 360.0


def sun_position(when, lat_deg, lon_deg):
    """The sun over (lat_deg, lon_deg) (degrees, north and east positive) at `when` -- a UTC datetime or a sequence of them; a naive
    datetime counts as UTC: (elevation_deg, azimuth_deg), azimuth clockwise from north (rays.construct_sun_dir's convention), floats
    for one datetime, else fp64 arrays.  No refraction; the elevation may be negative.  zip() of the two arrays is a `suns` list."""
    if not (math.isfinite(lat_deg) and -90.0 <= lat_deg <= 90.0 and math.isfinite(lon_deg)):
        raise ValueError(f"sun_position: latitude {lat_deg} must lie in [-90, 90] and longitude {lon_deg} be finite")
    year, doy, hours, single = _utc_fields(when)
    el, az = _position(year, doy, hours, lat_deg, lon_deg)
    return (float(el[0]), float(az[0])) if single else (el, az)


def sun_path(lat_deg, lon_deg, year, step_minutes=60, day_step=1, min_elevation_deg=5.0):
    """The suns of `year` above `min_elevation_deg`: every `day_step`-th day from 1 January, sampled at the middle of every
    `step_minutes` interval of the UTC day.  -> (suns (K, 2) fp64 rows (elevation_deg, azimuth_deg) in time order, hours (K,)): every
    sun stands for step_minutes / 60 hours of each of the days_in_year / sampled_days days its day stands for, so hours.sum() is the
    year's time above the threshold."""
    step_minutes, day_step = int(step_minutes), int(day_step)
    if step_minutes < 1 or 1440 % step_minutes or day_step < 1:
        raise ValueError(f"sun_path: step_minutes = {step_minutes} must divide 1440 and day_step = {day_step} be >= 1")
    if not (math.isfinite(min_elevation_deg) and 0.0 <= min_elevation_deg < 90.0):
        raise ValueError(f"sun_path: min_elevation_deg = {min_elevation_deg} must lie in [0, 90): a sun row needs rise > 0")
    n_days = int(_days_in(int(year)))
    days = np.arange(1, n_days + 1, day_step, dtype=np.float64)
    hours = (np.arange(1440 // step_minutes, dtype=np.float64) + 0.5) * (step_minutes / 60.0)
    doy, hr = (a.reshape(-1) for a in np.meshgrid(days, hours, indexing="ij"))
    el, az = _position(np.full(doy.shape, int(year)), doy, hr, lat_deg, lon_deg)
    keep = (el >= float(min_elevation_deg)) & (el > 0.0)
    suns = np.stack([el[keep], az[keep]], 1)
    return suns, np.full(len(suns), (step_minutes / 60.0) * (n_days / len(days)))


def clear_sky(elevation_deg, solar_constant=1353.0, transmittance=0.7, exponent=0.678, diffuse_share=0.1):
    """A clear sky at sea level: (dni, dhi) in W/m^2 -- Kasten and Young's (1989) relative air mass
    AM = 1 / (cos z + 0.50572 (96.07995 - z)^-1.6364), Meinel's direct normal irradiance solar_constant * transmittance^(AM^exponent),
    and the diffuse horizontal irradiance as the fixed share `diffuse_share` of it; zero at and below the horizon.  The coefficients
    are parameters, not claims: pass measured weights to irradiate() / solar() where they exist."""
    el = np.asarray(elevation_deg, np.float64)
    z = 90.0 - np.clip(el, 0.0, 90.0)
    am = 1.0 / (np.cos(np.deg2rad(z)) + 0.50572 * (96.07995 - z) ** -1.6364)
    dni = np.where(el > 0.0, float(solar_constant) * float(transmittance) ** (am ** float(exponent)), 0.0)
    return dni, float(diffuse_share) * dni


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def direction_rows(D):
    """the (D, 2) fp64 rows (ux, uy) = (sin a, -cos a) of the azimuths a = 360 d / D; the four axis directions are exact 0 / +-1"""
    D = int(D)
    if D < 1:
        raise ValueError(f"direction_rows: D = {D} must be >= 1")
    az = np.deg2rad(360.0 * np.arange(D, dtype=np.float64) / D)
    rows = np.stack([np.sin(az), -np.cos(az)], 1)
    for quarter, row in enumerate(((0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0))):
        if (quarter * D) % 4 == 0:
            rows[quarter * D // 4] = row
    return rows


def _suns(suns, who):
    pairs = np.asarray([(float(el), float(az)) for el, az in suns], np.float64).reshape(-1, 2)
    if not len(pairs):
        raise ValueError(f"{who}: no sun")
    if not (np.isfinite(pairs).all() and (pairs[:, 0] > 0.0).all() and (pairs[:, 0] <= 90.0).all()):
        raise ValueError(f"{who}: every sun needs a finite azimuth and an elevation in (0, 90] degrees")
    return pairs


def _res(res, who):
    res = float(res)
    if not (math.isfinite(res) and res > 0.0):
        raise ValueError(f"{who}: res = {res} must be positive and finite")
    return res


def sun_table(suns, weights, D, res):
    """(elevation_deg, azimuth_deg) pairs and their weights -> the (K, 7) fp64 rows (sector, frac, rise, east, north, up, weight) of
    snerf_solar_irradiate against the planes of direction_rows(D): the sun stands at x = azimuth D / 360 sectors, sector = floor(x),
    frac = x - sector in [0, 1); within 1e-9 sectors of a sector it stands on it (frac = 0); sector D is sector 0.  rise = tan(el) res,
    (east, north, up) = (cos el sin az, cos el cos az, sin el).  numpy fp64."""
    pairs, res, D = _suns(suns, "sun_table"), _res(res, "sun_table"), int(D)
    wt = np.asarray(weights, np.float64).reshape(-1)
    if D < 1 or D > MAX_SECTORS:
        raise ValueError(f"sun_table: D = {D} outside [1, {MAX_SECTORS}]")
    if wt.shape != (len(pairs),) or not (np.isfinite(wt).all() and (wt >= 0.0).all()):
        raise ValueError(f"sun_table: {len(pairs)} suns need {len(pairs)} finite weights >= 0")
    el, az = np.deg2rad(pairs).T
    x = (pairs[:, 1] % 360.0) * D / 360.0
    near = np.rint(x)
    x = np.where(np.abs(x - near) <= SNAP, near, x)
    sector = np.floor(x)
    frac = x - sector
    sector = np.where(sector >= D, sector - D, sector)
    return np.stack([sector, frac, np.tan(el) * res, np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el), wt], 1)


# ---- the device stages --------------------------------------------------------------------------------------------------------------
def _planes(horizon, who):
    if not (torch.is_tensor(horizon) and horizon.is_cuda):
        raise ValueError(f"{who}: the horizon must be a GPU tensor (the HIP path has no CPU fallback)")
    if horizon.dim() != 3 or horizon.dtype != torch.float32 or not horizon.numel() or horizon.shape[0] > MAX_SECTORS:
        raise ValueError(f"{who}: the horizon must be a non-empty (D, H, W) float32 tensor with D <= {MAX_SECTORS}, not "
                         f"{tuple(horizon.shape)} of {horizon.dtype}")
    return horizon.contiguous()


def horizon_rows(dsm, rows, bias=0.0, max_dist=math.inf, z_top=None):
    """horizon on ready-made (D, 2) fp64 rows (ux, uy), D >= 1, `max_dist` in cells: one snerf_solar_horizon per 64 rows"""
    dsm = _dsm(dsm, "horizon")
    rows = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(-1, 2))
    D = len(rows)
    if not D:
        raise ValueError("horizon: no direction")
    h, w = dsm.shape
    if z_top is None:      # the largest finite altitude (-inf for a DSM without one), as cast_rows takes it
        z_top = float(torch.where(torch.isfinite(dsm), dsm, torch.full_like(dsm, -math.inf)).max())
    out = torch.empty((D, h, w), dtype=torch.float32, device=dsm.device)
    for k in range(0, D, MAX_DIRS):
        part = np.ascontiguousarray(rows[k:k + MAX_DIRS])
        _lib.call("snerf_solar_horizon", dsm, h, w, part.ctypes.data_as(C.c_void_p), len(part), bias, z_top, max_dist, out[k:k + len(part)],
                  exc=ValueError)
    return out


def horizon(dsm, res, D=64, bias=0.0, max_dist_m=None, z_top=None):
    """The horizon planes of `dsm` ((H, W) f32 on the GPU, row 0 = the north edge, NaN = a hole) at `res` metres per cell: (D, H, W)
    f32, plane d towards the azimuth 360 d / D -- the steepest slope from the cell to any cell its ground track crosses, in metres per
    cell of horizontal travel (tan(horizon angle) * res); -inf where the track crosses nothing, NaN where the cell is a hole.  `bias`
    (metres) lifts the start of every march, as in cast_shadows.  `max_dist_m` bounds the search (None: the whole raster).  `z_top`
    only ends marches early: None takes the largest finite altitude (one host read); any value at or above it gives the same bits."""
    res = _res(res, "horizon")
    max_dist = math.inf if max_dist_m is None else float(max_dist_m) / res
    return horizon_rows(dsm, direction_rows(D), bias, max_dist, z_top)


def sky_view(horizon, res):
    """The cosine-weighted sky-view factor of a horizontal surface, the mean over the sectors of cos^2(horizon angle): (H, W) f32 in
    (0, 1], 1 = nothing stands above the cell's own altitude, NaN on holes"""
    horizon, res = _planes(horizon, "sky_view"), _res(res, "sky_view")
    D, h, w = horizon.shape
    out = torch.empty((h, w), dtype=torch.float32, device=horizon.device)
    _lib.call("snerf_solar_svf", horizon, D, h, w, res, out, exc=ValueError)
    return out


def irradiate_rows(horizon, table, slope_e=None, slope_n=None, direct=None, lit_count=None):
    """irradiate on ready-made (K, 7) fp64 rows (sun_table), K >= 1: one snerf_solar_irradiate per 64 rows, in order.  -> (direct_acc
    (H, W) f64 -- the sum of weight * (up - slope_e east - slope_n north) over the visible suns in front of the surface, NOT yet
    divided by sqrt(1 + slope_e^2 + slope_n^2) -- and lit_count (H, W) int32 holding the u32 counts), continued from `direct` /
    `lit_count` when given"""
    horizon = _planes(horizon, "irradiate")
    table = np.ascontiguousarray(np.asarray(table, np.float64).reshape(-1, 7))
    if not len(table):
        raise ValueError("irradiate: no sun")
    D, h, w = horizon.shape
    if (slope_e is None) != (slope_n is None):
        raise ValueError("irradiate: slope_e and slope_n are both None or both given")
    if slope_e is not None:
        for name, s in (("slope_e", slope_e), ("slope_n", slope_n)):
            if not (torch.is_tensor(s) and s.is_cuda) or s.dtype != torch.float32 or tuple(s.shape) != (h, w):
                raise ValueError(f"irradiate: {name} must be a ({h}, {w}) float32 GPU tensor")
        slope_e, slope_n = slope_e.contiguous(), slope_n.contiguous()
    if direct is None:
        direct = torch.zeros((h, w), dtype=torch.float64, device=horizon.device)
    if lit_count is None:
        lit_count = torch.zeros((h, w), dtype=torch.int32, device=horizon.device)
    if (direct.dtype, lit_count.dtype) != (torch.float64, torch.int32) or tuple(direct.shape) != (h, w) or tuple(lit_count.shape) != (h, w) \
            or not (direct.is_contiguous() and lit_count.is_contiguous()):
        raise ValueError(f"irradiate: the accumulators must be contiguous ({h}, {w}) float64 and int32 tensors")
    for k in range(0, len(table), MAX_SUNS):
        part = np.ascontiguousarray(table[k:k + MAX_SUNS])
        _lib.call("snerf_solar_irradiate", horizon, D, h, w, slope_e, slope_n, part.ctypes.data_as(C.c_void_p), len(part), direct, lit_count,
                  exc=ValueError)
    return direct, lit_count


def surface_factor(slope_e, slope_n):
    """sqrt(1 + slope_e^2 + slope_n^2) in fp64: a cell's surface area over its plan area, 1 / cos(tilt)"""
    return torch.sqrt(1.0 + slope_e.double() ** 2 + slope_n.double() ** 2)


def irradiate(horizon, res, suns, weights, slope_e=None, slope_n=None):
    """`suns` ((elevation_deg, azimuth_deg) pairs, any number) with `weights` against the horizon planes: -> (direct, lit_count).
    direct (H, W) f64: the sum of weight * cos(incidence) over the suns a cell sees, per m^2 of the surface slope_e / slope_n describe
    (rise per metre east / north, as roofs.normals gives them; None = horizontal) -- weights of W/m^2 x hours give Wh/m^2; NaN on holes
    and where a slope is NaN.  lit_count (H, W) int32: the suns the cell sees, in front of the surface or behind it."""
    horizon = _planes(horizon, "irradiate")
    direct, lit = irradiate_rows(horizon, sun_table(suns, weights, horizon.shape[0], res), slope_e, slope_n)
    if slope_e is not None:
        direct = direct / surface_factor(slope_e, slope_n)
    return direct, lit


# ---- everything in one call -----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def solar(alt, grid, lat_deg, lon_deg, slope_e=None, slope_n=None, year=2021, step_minutes=60, day_step=1, min_elevation_deg=5.0, D=64,
          bias=0.0, max_dist_m=None, suns=None, hours=None, dni=None, dhi=None, clear_sky_options=None):
    """The solar potential of the map `alt` ((H, W) f32 on the GPU) on `grid` at (lat_deg, lon_deg): the suns of sun_path(year, ...)
    under clear_sky(**clear_sky_options), or the caller's `suns` with `hours` (the hours each stands for) and, optionally, `dni` / `dhi`
    (W/m^2 per sun: measured weather).  slope_e / slope_n: the surface of every cell (roofs()'s planes); NaN slopes -- cells outside
    buildings -- count as horizontal; None: horizontal everywhere.
    Returns {"svf", "sun_hours", "direct_kwh", "diffuse_kwh", "global_kwh": (H, W) planes -- f32, f64, f64, f64, f64; NaN on holes --,
    "surface_factor" (H, W) f64, "horizon" (D, H, W) f32, "lit_count", "n_suns", "annual_dhi_kwh", "parameters"}.  sun_hours: the hours
    of the suns a cell sees; direct_kwh: kWh per m^2 of surface and year; diffuse_kwh = annual DHI * svf * (1 + cos tilt) / 2 (an
    isotropic sky); global_kwh their sum."""
    res = _res(grid.resolution, "solar")
    alt = _dsm(alt, "solar")
    if suns is None:
        if hours is not None or dni is not None or dhi is not None:
            raise ValueError("solar: hours, dni and dhi belong to caller-supplied suns")
        suns, hours = sun_path(lat_deg, lon_deg, year, step_minutes, day_step, min_elevation_deg)
    elif hours is None:
        raise ValueError("solar: caller-supplied suns need the hours each one stands for")
    suns = _suns(suns, "solar")
    hours = np.asarray(hours, np.float64).reshape(-1)
    sky = clear_sky(suns[:, 0], **(clear_sky_options or {}))
    dni = sky[0] if dni is None else np.asarray(dni, np.float64).reshape(-1)
    dhi = sky[1] if dhi is None else np.asarray(dhi, np.float64).reshape(-1)
    if not (hours.shape == dni.shape == dhi.shape == (len(suns),)):
        raise ValueError(f"solar: {len(suns)} suns need as many hours, dni and dhi values")
    if slope_e is not None and slope_n is not None:
        flat = torch.isnan(slope_e) | torch.isnan(slope_n)
        slope_e, slope_n = (torch.where(flat, torch.zeros_like(s), s).float().contiguous() for s in (slope_e, slope_n))
    hor = horizon(alt, res, D, bias, max_dist_m)
    svf = sky_view(hor, res)
    direct, lit = irradiate_rows(hor, sun_table(suns, dni * hours / 1000.0, D, res), slope_e, slope_n)
    factor = surface_factor(slope_e, slope_n) if slope_e is not None else torch.ones_like(direct)
    direct = direct / factor
    table = sun_table(suns, hours, D, res)      # a horizontal unit surface under the hours as weights: the hours of the visible suns
    table[:, 3:6] = (0.0, 0.0, 1.0)
    sun_hours = irradiate_rows(hor, table)[0]
    annual_dhi = float((dhi * hours).sum() / 1000.0)
    diffuse = annual_dhi * svf.double() * (1.0 + 1.0 / factor) / 2.0
    params = {"lat_deg": float(lat_deg), "lon_deg": float(lon_deg), "year": int(year), "step_minutes": int(step_minutes),
              "day_step": int(day_step), "min_elevation_deg": float(min_elevation_deg), "D": int(D), "bias": float(bias),
              "max_dist_m": None if max_dist_m is None else float(max_dist_m), "resolution": res}
    return {"svf": svf, "sun_hours": sun_hours, "direct_kwh": direct, "diffuse_kwh": diffuse, "global_kwh": direct + diffuse,
            "surface_factor": factor, "horizon": hor, "lit_count": lit, "n_suns": len(suns), "annual_dhi_kwh": annual_dhi,
            "parameters": params}


def solar_table(result, ids, n, res, min_kwh_m2=1000.0):
    """Per id 1 .. n of the plane `ids` ((H, W) integers: facet or building ids, 0 = none; ids outside [1, n] are left out) the columns
    "cells", "valid_cells" (with a finite global_kwh), "plan_m2", "surface_m2", "mean_kwh_m2" / "min_kwh_m2" / "max_kwh_m2" (global_kwh
    per m^2 of surface; the mean is weighted by surface), "annual_mwh" (over the surface), "mean_sun_hours", "mean_svf" and
    "good_m2" (the surface whose global_kwh is at least `min_kwh_m2`), as numpy arrays of length n; NaN where an id has no valid
    cell.  Every sum is over values quantised to 2^-16 of their unit and added as integers (index_add_ on int64): no figure depends
    on the order of the additions.  Works on the device the planes live on."""
    res, n = _res(res, "solar_table"), int(n)
    g = result["global_kwh"].double().reshape(-1)
    dev = g.device
    idx = torch.as_tensor(ids).to(dev).reshape(-1).long()
    if idx.numel() != g.numel() or n < 0:
        raise ValueError(f"solar_table: {idx.numel()} ids for {g.numel()} cells, n = {n}")
    member = (idx >= 1) & (idx <= n)
    ok = member & torch.isfinite(g)
    slot = torch.where(ok, idx, torch.zeros_like(idx))
    cell = res * res
    factor = result["surface_factor"].double().reshape(-1).to(dev)

    def total(values):
        q = torch.where(ok, torch.round(torch.nan_to_num(values.double(), nan=0.0, posinf=0.0, neginf=0.0) * QUANT), torch.zeros_like(g))
        return torch.zeros(n + 1, dtype=torch.int64, device=dev).index_add_(0, slot, q.long())[1:].cpu().numpy() / QUANT

    count = lambda m: torch.zeros(n + 1, dtype=torch.int64, device=dev).index_add_(0, torch.where(m, idx, torch.zeros_like(idx)),  # noqa: E731
                                                                                   m.long())[1:].cpu().numpy()
    cells, valid = count(member), count(ok)
    surface = total(factor * cell)
    energy = total(g * factor * cell)                       # kWh per cell
    with np.errstate(invalid="ignore", divide="ignore"):
        some = valid > 0
        nan = np.where(some, 0.0, np.nan)
        ext = {}
        for name, red, init in (("min_kwh_m2", "amin", math.inf), ("max_kwh_m2", "amax", -math.inf)):
            buf = torch.full((n + 1,), init, dtype=torch.float64, device=dev)
            buf.scatter_reduce_(0, slot, torch.where(ok, g, torch.full_like(g, init)), red)
            ext[name] = buf[1:].cpu().numpy() + nan
        return {"cells": cells, "valid_cells": valid, "plan_m2": valid * cell, "surface_m2": surface,
                "mean_kwh_m2": energy / surface + nan, "min_kwh_m2": ext["min_kwh_m2"], "max_kwh_m2": ext["max_kwh_m2"],
                "annual_mwh": energy / 1000.0, "mean_sun_hours": total(result["sun_hours"].reshape(-1).to(dev)) / valid + nan,
                "mean_svf": total(result["svf"].reshape(-1).to(dev)) / valid + nan,
                "good_m2": total(torch.where(g >= float(min_kwh_m2), factor * cell, torch.zeros_like(g)))}
