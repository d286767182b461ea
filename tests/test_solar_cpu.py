"""CPU-side checks of the solar potential (include/snerf_solar.h, csrc/solar.hip, eval/utils/solar.py): the new
header's prototypes and constants against the binding (_lib.HEADER_SIGNATURES), every refusal of the three entries through the binding
(none reaches a launch), the restatement (tests/solar_numpy.py, the oracle of tests/test_gpu_solar.py) against a brute-force
formulation, an analytic wall and the restated cast shadows, sun_position against astronomy, and the host tables on hand-made input."""
import ctypes as C
import datetime
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import solar as SO            # the feature under test: every test of this file needs it
from tests import shadow_numpy as SN
from tests import solar_numpy as N
from tests.test_gpu_shadow import _make_dsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_solar.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_solar_horizon": ["dsm", "h", "w", "dirs_host", "n_dirs", "bias", "z_top", "max_dist", "horizon_out", "stream"],
    "snerf_solar_svf": ["horizon", "n_dirs", "h", "w", "res", "svf_out", "stream"],
    "snerf_solar_irradiate": ["horizon", "n_dirs", "h", "w", "slope_e", "slope_n", "suns_host", "n_suns", "direct_acc", "lit_count", "stream"],
}
S2 = math.sqrt(0.5)


def test_the_new_header_matches_its_binding_rows():
    """include/snerf_solar.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py), then the constants; the main header, the
    main table, the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_solar.h", NAMES)
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SNERF_SOLAR_\w+) (\d+)", text)}
    assert consts == {"SNERF_SOLAR_MAX_DIRS": 64, "SNERF_SOLAR_MAX_SECTORS": 720, "SNERF_SOLAR_MAX_SUNS": 64}
    assert (_lib.SOLAR_MAX_DIRS, _lib.SOLAR_MAX_SECTORS, _lib.SOLAR_MAX_SUNS) == (SO.MAX_DIRS, SO.MAX_SECTORS, SO.MAX_SUNS) == \
        (N.MAX_DIRS, N.MAX_SECTORS, N.MAX_SUNS) == (64, 720, 64)


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
GOOD_DIRS = (1.0, 0.0, S2, -S2)
GOOD_SUNS = (0.0, 0.0, 0.5, 0.0, 0.6, 0.8, 1.0, 1.0, 0.25, 0.1, 0.6, 0.0, 0.8, 0.0)


def _rows(vals, **change):
    v = list(vals)
    for k, x in change.items():
        v[int(k[1:])] = x
    return (C.c_double * len(v))(*v)


def _call(symbol, **kw):
    """an entry through the binding with dummy device addresses (the rows, which ARE read, are host arrays): (rc, message)"""
    L = _lib.lib()
    a = dict(dsm=DUMMY, h=3, w=4, dirs_host=_rows(GOOD_DIRS), n_dirs=2, bias=0.0, z_top=math.inf, max_dist=math.inf, horizon_out=DUMMY,
             horizon=DUMMY, res=0.5, svf_out=DUMMY, slope_e=None, slope_n=None, suns_host=_rows(GOOD_SUNS), n_suns=2, direct_acc=DUMMY,
             lit_count=DUMMY)
    a.update(kw)
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


inf, nan = math.inf, math.nan
SIZE_REFUSALS = [({"h": 0}, 1, "h = 0"), ({"w": -1}, 1, "w = -1"), ({"h": 1 << 16, "w": 1 << 15}, 1, "2^31")]
HORIZON_REFUSALS = [
    ({"dsm": None}, 3, "null"), ({"dirs_host": None}, 3, "null"), ({"horizon_out": None}, 3, "null"),
    ({"n_dirs": 0}, 1, "n_dirs = 0"), ({"n_dirs": 65}, 1, "n_dirs = 65"), ({"bias": inf}, 1, "bias"), ({"bias": nan}, 1, "bias"),
    ({"z_top": nan}, 1, "z_top"), ({"max_dist": 0.0}, 1, "max_dist"), ({"max_dist": -1.0}, 1, "max_dist"), ({"max_dist": nan}, 1, "max_dist"),
    ({"dirs_host": _rows(GOOD_DIRS, r2=nan)}, 1, "direction 1 is not finite"), ({"dirs_host": _rows(GOOD_DIRS, r1=inf)}, 1, "direction 0 is not finite"),
    ({"dirs_host": _rows(GOOD_DIRS, r0=1.0 + 1e-8)}, 1, "direction 0: (ux, uy)"), ({"dirs_host": _rows(GOOD_DIRS, r0=1.0 + 6e-10)}, 1, "not a unit vector"),
]
SVF_REFUSALS = [
    ({"horizon": None}, 3, "null"), ({"svf_out": None}, 3, "null"), ({"n_dirs": 0}, 1, "n_dirs = 0"), ({"n_dirs": 721}, 1, "n_dirs = 721"),
    ({"res": 0.0}, 1, "res > 0"), ({"res": -0.5}, 1, "res > 0"), ({"res": inf}, 1, "res > 0"), ({"res": nan}, 1, "res > 0"),
]
IRRADIATE_REFUSALS = [
    ({"horizon": None}, 3, "null"), ({"suns_host": None}, 3, "null"), ({"direct_acc": None}, 3, "null"), ({"lit_count": None}, 3, "null"),
    ({"slope_e": DUMMY}, 3, "both null or both set"), ({"slope_n": DUMMY}, 3, "both null or both set"),
    ({"n_dirs": 0}, 1, "n_dirs = 0"), ({"n_dirs": 721}, 1, "n_dirs = 721"), ({"n_suns": 0}, 1, "n_suns = 0"), ({"n_suns": 65}, 1, "n_suns = 65"),
    ({"suns_host": _rows(GOOD_SUNS, r13=nan)}, 1, "sun 1 is not finite"), ({"suns_host": _rows(GOOD_SUNS, r2=inf)}, 1, "sun 0 is not finite"),
    ({"suns_host": _rows(GOOD_SUNS, r7=2.0)}, 1, "sun 1: sector"), ({"suns_host": _rows(GOOD_SUNS, r0=-1.0)}, 1, "sun 0: sector"),
    ({"suns_host": _rows(GOOD_SUNS, r0=0.5)}, 1, "sun 0: sector"), ({"suns_host": _rows(GOOD_SUNS, r0=1e300)}, 1, "sun 0: sector"),
    ({"suns_host": _rows(GOOD_SUNS, r8=1.0)}, 1, "sun 1: frac"), ({"suns_host": _rows(GOOD_SUNS, r1=-0.1)}, 1, "sun 0: frac"),
    ({"suns_host": _rows(GOOD_SUNS, r2=0.0)}, 1, "sun 0: rise"), ({"suns_host": _rows(GOOD_SUNS, r9=-0.1)}, 1, "sun 1: rise"),
    ({"suns_host": _rows(GOOD_SUNS, r4=0.61)}, 1, "sun 0: (east, north, up)"), ({"suns_host": _rows(GOOD_SUNS, r12=-0.8)}, 1, "sun 1: up"),
    ({"suns_host": _rows(GOOD_SUNS, r6=-1.0)}, 1, "sun 0: weight"),
]
CASES = ([("snerf_solar_horizon", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + HORIZON_REFUSALS]
         + [("snerf_solar_svf", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + SVF_REFUSALS]
         + [("snerf_solar_irradiate", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + IRRADIATE_REFUSALS])


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{s[12:]}-{n}" for n, (s, _, _, _) in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **dict(kw))
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_python_refuses_host_tensors_and_bad_parameters():
    dsm, hor = torch.zeros(5, 7), torch.zeros(4, 5, 7)
    with pytest.raises(ValueError, match="GPU tensor"):
        SO.horizon(dsm, 0.5)
    with pytest.raises(ValueError, match="GPU tensor"):
        SO.sky_view(hor, 0.5)
    with pytest.raises(ValueError, match="GPU tensor"):
        SO.irradiate(hor, 0.5, [(30.0, 100.0)], [1.0])
    with pytest.raises(ValueError, match="GPU tensor"):
        SO.solar(dsm, type("G", (), {"resolution": 0.5})(), 30.0, -81.0)
    with pytest.raises(ValueError, match="res"):
        SO.horizon(dsm, 0.0)
    for el in (0.0, -3.0, 90.0001, math.nan):
        with pytest.raises(ValueError, match=r"elevation in \(0, 90\]"):
            SO.sun_table([(45.0, 10.0), (el, 10.0)], [1.0, 1.0], 64, 0.5)
    with pytest.raises(ValueError, match="no sun"):
        SO.sun_table([], [], 64, 0.5)
    with pytest.raises(ValueError, match="weights"):
        SO.sun_table([(45.0, 10.0)], [-1.0], 64, 0.5)
    with pytest.raises(ValueError, match="weights"):
        SO.sun_table([(45.0, 10.0)], [1.0, 2.0], 64, 0.5)
    with pytest.raises(ValueError, match="D = 721"):
        SO.sun_table([(45.0, 10.0)], [1.0], 721, 0.5)
    with pytest.raises(ValueError, match="D = 0"):
        SO.direction_rows(0)
    with pytest.raises(ValueError, match="step_minutes"):
        SO.sun_path(30.0, -81.0, 2021, step_minutes=7)
    with pytest.raises(ValueError, match="min_elevation_deg"):
        SO.sun_path(30.0, -81.0, 2021, min_elevation_deg=-1.0)
    with pytest.raises(ValueError, match="latitude"):
        SO.sun_position(datetime.datetime(2021, 6, 21, 12), 91.0, 0.0)
    import inspect
    from snerf_amd.eval import ortho as EO
    assert list(inspect.signature(EO.export_solar).parameters) == ["products", "output_dp", "roofs_result", "objects_result", "geo", "lat_deg",
                                                                   "lon_deg", "alt_key", "zone_string", "kwargs"]
    p = inspect.signature(SO.sun_path).parameters
    assert [p[k].default for k in ("step_minutes", "day_step", "min_elevation_deg")] == [60, 1, 5.0]
    p = inspect.signature(SO.horizon).parameters
    assert [p[k].default for k in ("D", "bias", "max_dist_m", "z_top")] == [64, 0.0, None, None]


# ---- the restatement's horizon --------------------------------------------------------------------------------------------------------
def _brute(dsm, row, bias=0.0, max_dist=np.inf):
    """Per start cell and per cell of the window, analytically (the slab method of tests/test_shadow_cpu.py _brute): does the ground
    track x0 + t (ux, uy), t > 0, pass through the cell's interior, and at which t does it enter?  The horizon is the maximum over the
    entered cells of (altitude - start) / entry.  No marching, no accumulated tMax: every entry distance is one division."""
    h, w = dsm.shape
    d64 = dsm.astype(np.float64)
    ux, uy = row
    ci, cj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    out = np.full((h, w), np.nan)

    def slab(lo, x0, u):
        if u == 0.0:
            inside = (lo < x0) & (x0 < lo + 1.0)
            return np.where(inside, -np.inf, np.inf), np.where(inside, np.inf, -np.inf)
        a, b = (lo - x0) / u, (lo + 1.0 - x0) / u
        return np.minimum(a, b), np.maximum(a, b)

    for j0 in range(h):
        for i0 in range(w):
            if np.isnan(d64[j0, i0]):
                continue
            ax, bx = slab(ci, i0 + 0.5, ux)
            ay, by = slab(cj, j0 + 0.5, uy)
            enter, leave = np.maximum(ax, ay), np.minimum(bx, by)
            crossed = (leave > enter) & (enter > 0.0) & (enter <= max_dist) & ~np.isnan(d64)
            crossed[j0, i0] = False
            out[j0, i0] = ((d64[crossed] - (d64[j0, i0] + bias)) / enter[crossed]).max() if crossed.any() else -np.inf
    return out


@pytest.mark.parametrize("shape,seed,max_dist", [((9, 11), 11, np.inf), ((16, 17), 12, np.inf), ((16, 17), 13, 4.25)], ids=["9x11", "16x17", "16x17-4.25"])
def test_the_restatement_agrees_with_the_brute_force_formulation(shape, seed, max_dist):
    """random DSMs (10 % NaN holes) under 8 random directions and a bias.  The two agree wherever the smallest |tMaxX - tMaxY| along
    the march exceeds 1e-9 (a track through a lattice corner enters the cell beside it or not by the last bit; fewer than 1 % of the
    pairs may be left out by that rule) -- to 2e-7 relative: the march accumulates tMax, one rounding per step, and the plane is fp32."""
    rng = np.random.default_rng(seed)
    dsm = rng.uniform(0.0, 12.0, shape).astype(np.float32)
    dsm[rng.random(shape) < 0.1] = np.nan
    az = np.deg2rad(rng.uniform(0.0, 360.0, 8))
    kept = total = 0
    for row in np.stack([np.sin(az), -np.cos(az)], 1):
        got, mt = N.horizon_one(dsm, row, 0.25, max_dist, want_margins=True)
        want = _brute(dsm, row, 0.25, max_dist)
        assert np.array_equal(np.isnan(got), np.isnan(dsm)) and np.array_equal(np.isnan(want), np.isnan(dsm))
        keep = (mt > 1e-9) & ~np.isnan(dsm)
        kept += int(keep.sum())
        total += int((~np.isnan(dsm)).sum())
        assert np.array_equal(np.isinf(got[keep]), np.isinf(want[keep]))
        fin = keep & np.isfinite(got)
        assert fin.sum() > 0 and np.allclose(got[fin], want[fin], rtol=2e-7, atol=0.0)
    print(f"{shape}: {total - kept} of {total} pairs left out")
    assert total - kept < 0.01 * total


def test_an_analytic_wall_and_the_search_distance():
    """A wall of height Hm, d cells east of a ground cell at 0, direction due east (ux = 1: the entries are t = 0.5, 1.5, ...): the
    wall's cell is entered at t = d - 0.5 and everything else on the way is ground (slope 0), so the horizon is exactly
    Hm / (d - 0.5) -- the wall's near face, half a cell before its centre.  Under a max_dist short of the wall the ground's 0.0
    remains; on the wall itself and east of it the ground beyond lies below: a negative slope, largest at the raster's far end."""
    Hm, col = 15.0, 12
    dsm = np.zeros((3, 20), np.float32)
    dsm[:, col] = Hm
    hor = N.horizon_one(dsm, (1.0, 0.0))
    for d in range(1, col + 1):
        assert hor[1, col - d] == np.float32(Hm / (d - 0.5)), d
    assert hor[1, col] == np.float32(-Hm / 6.5) and hor[1, col + 1] == 0.0 and hor[1, 19] == -np.inf
    near = N.horizon_one(dsm, (1.0, 0.0), max_dist=4.0)             # entries up to t = 3.5: the wall is seen from 4 cells or fewer
    assert (near[1, :col - 4] == 0.0).all() and near[1, col - 4] == np.float32(Hm / 3.5) and near[1, col - 5] == 0.0
    assert N.horizon_one(dsm, (-1.0, 0.0))[1, 0] == -np.inf and N.horizon_one(dsm, (-1.0, 0.0))[1, 19] == np.float32(Hm / 6.5)
    assert np.array_equal(N.horizon_one(dsm, (0.0, 1.0))[:2], np.zeros((2, 20), np.float32))        # along the wall: level ground
    biased = N.horizon_one(dsm, (1.0, 0.0), bias=3.0)
    assert biased[1, col - 2] == np.float32((Hm - 3.0) / 1.5) and biased[1, 0] == np.float32((Hm - 3.0) / 11.5)


RES = 0.5
AZIMUTHS = (0.0, 90.0, 45.0, 33.3, 201.7, 270.0)
ELEVATIONS = (2.0, 11.0, 35.0, 45.0, 62.5)


def _consistency(dsm, rows):
    """(pairs, pairs in the band |rise - H| <= 2^-22 |H|, disagreements outside it) of lit == (rise >= H) over the rows (ux, uy, rise)"""
    pairs = band = wrong = 0
    planes = {}
    for ux, uy, rise in rows:
        if (ux, uy) not in planes:
            planes[(ux, uy)] = N.horizon_one(dsm, (ux, uy)).astype(np.float64)
        H = planes[(ux, uy)]
        lit = SN.cast_one(dsm, (ux, uy, rise))[0]
        known = lit != SN.UNKNOWN
        assert np.array_equal(known, ~np.isnan(H))
        with np.errstate(invalid="ignore"):
            close = known & np.isfinite(H) & (np.abs(rise - H) <= 2.0 ** -22 * np.abs(H))      # a -inf horizon is never close
            differ = known & ~close & ((lit == 1) != (rise >= H))
        pairs, band, wrong = pairs + int(known.sum()), band + int(close.sum()), wrong + int(differ.sum())
    return pairs, band, wrong


@pytest.mark.parametrize("kind", ("random", "holes", "tower", "wall", "flat"))
def test_the_horizon_decides_what_the_cast_shadow_decides(kind):
    """the claim that makes the method valid, on the two restatements: a cell is lit under a sun iff the sun's rise is at least the
    horizon slope towards it (the fp32 plane), on every (cell, sun) pair outside the band |rise - H| <= 2^-22 |H| -- the cast kernel
    compares c > h0 + rise t, the horizon (c - h0) / t with rise, and the plane is rounded to fp32.  Nothing falls in the band here."""
    dsm = _make_dsm(kind, 33, 64)
    rows = [tuple(r) for r in SN.sun_rows([(el, az) for az in AZIMUTHS for el in ELEVATIONS], RES)]
    pairs, band, wrong = _consistency(dsm, rows)
    print(f"{kind}: {pairs} pairs, {band} in the band, {wrong} disagree")
    assert pairs == int((~np.isnan(dsm)).sum()) * 30 and pairs >= 57000 and band == 0 and wrong == 0


def test_the_horizon_decides_it_on_exact_ties_too():
    """heights quantised to 0.25 m under the snapped axis directions and the exact diagonal, rises 0.125 .. 1.0: (c - h0) / t == rise
    occurs exactly.  Equality is lit on both sides (the cast kernel blocks on >, the sun table is lit on >=); at most 2 % of the pairs
    may lie in the band, none outside it may disagree."""
    dsm = (np.random.default_rng(3).integers(0, 40, (33, 64)) * 0.25).astype(np.float32)
    dirs = [tuple(r) for r in SO.direction_rows(4)] + [(S2, -S2)]
    pairs, band, wrong = _consistency(dsm, [(ux, uy, rise) for ux, uy in dirs for rise in (0.125, 0.25, 0.5, 1.0)])
    print(f"quantised: {pairs} pairs, {band} in the band, {wrong} disagree")
    assert pairs == 42240 and 0 < band <= 0.02 * pairs and wrong == 0


def test_sky_view_restated():
    flat = N.horizon(np.full((5, 7), 3.0, np.float32), SO.direction_rows(16))
    assert (flat[:, 2, 3] == 0.0).all() and (N.svf(flat, RES) == 1.0).all()            # level ground round a cell; -inf at the edges
    assert (N.svf(np.full((8, 2, 3), -np.inf, np.float32), RES) == 1.0).all()
    for T in (0.5, 1.0, 3.0):
        assert (N.svf(np.full((64, 2, 3), np.float32(T * RES)), RES) == np.float32(1.0 / (1.0 + T * T))).all()
    hole = np.zeros((4, 2, 2), np.float32)
    hole[:, 0, 1] = np.nan
    assert np.array_equal(np.isnan(N.svf(hole, RES)), [[False, True], [False, False]])
    pit = np.full((9, 9), 10.0, np.float32)
    pit[4, 4] = 0.0
    s = N.svf(N.horizon(pit, SO.direction_rows(64)), RES)
    assert s[4, 4] < 0.01 and s[0, 0] == 1.0


def test_irradiate_restated():
    hor = np.zeros((4, 1, 3), np.float32)
    hor[1, 0, 1], hor[2, 0, 1] = 1.0, 3.0            # the middle cell: slopes 0, 1, 3, 0 towards N, E, S, W
    hor[:, 0, 2] = np.nan
    table = SO.sun_table([(45.0, 90.0), (45.0, 135.0), (45.0, 0.0)], [2.0, 4.0, 8.0], 4, 1.0)
    assert table[:, 0].tolist() == [1.0, 1.0, 0.0] and table[:, 1].tolist() == [0.0, 0.5, 0.0] and np.allclose(table[:, 2], 1.0, rtol=0, atol=2e-16)
    table[:, 2] = 1.0                                # tan(45 deg) is 1 - 2^-53 in fp64; the tie below is meant exactly
    direct, count = N.irradiate(hor, table)
    up = math.sin(math.radians(45.0))
    # cell 0 sees all three; the middle cell: rise = 1 >= 1 on the sector (equality is lit), 1 < 2 between the sectors
    assert count.tolist() == [[3, 2, 0]] and direct[0, 0] == (2.0 * up + 4.0 * up) + 8.0 * up and direct[0, 1] == 2.0 * up + 8.0 * up
    assert np.isnan(direct[0, 2])
    # a surface that falls to the north at 45 degrees (it rises 1 m per metre south: slope_n = -1) turns its back on a southern sun
    table = SO.sun_table([(30.0, 180.0), (30.0, 0.0)], [1.0, 1.0], 4, 1.0)
    se, sn = np.zeros((1, 3), np.float32), np.full((1, 3), -1.0, np.float32)
    direct, count = N.irradiate(hor, table, se, sn)
    north_sun = math.sin(math.radians(30.0)) + math.cos(math.radians(30.0))
    assert count.tolist() == [[2, 1, 0]] and abs(direct[0, 0] - north_sun) < 1e-15 and abs(direct[0, 1] - north_sun) < 1e-15
    sn[0, 0] = np.nan
    direct, count = N.irradiate(hor, table, se, sn)
    assert np.isnan(direct[0, 0]) and count[0, 0] == 2


# ---- suns from dates ------------------------------------------------------------------------------------------------------------------
def _noon_terms(year=2021):
    days = np.arange(1, 366, dtype=np.float64)
    return SO.solar_terms(np.full(365, year), days, np.full(365, 12.0))


def test_the_declination_and_the_equation_of_time_are_the_suns():
    decl, eot = _noon_terms()
    assert abs(decl.max() - 23.44) <= 0.1 and abs(decl.min() + 23.44) <= 0.1
    assert 170 <= int(decl.argmax()) + 1 <= 174 and 353 <= int(decl.argmin()) + 1 <= 357          # 21 June, 21 December
    lo, hi = int(eot.argmin()) + 1, int(eot.argmax()) + 1
    print(f"declination {decl.max():.3f} / {decl.min():.3f}, equation of time {eot.min():.2f} on day {lo}, {eot.max():.2f} on day {hi}")
    assert 38 <= lo <= 48 and -14.6 <= eot.min() <= -13.9 and 300 <= hi <= 310 and 16.1 <= eot.max() <= 16.7
    for month, day in ((3, 20), (9, 22)):
        doy = datetime.date(2021, month, day).timetuple().tm_yday
        assert abs(decl[doy - 1]) <= 0.7, (month, day, decl[doy - 1])


@pytest.mark.parametrize("lat,lon", [(30.3, -81.7), (52.5, 13.4), (64.1, -21.9), (35.7, 139.7)])
def test_solar_noon(lat, lon):
    """at local solar noon north of the declination the sun stands due south at 90 - (lat - decl), and the day is symmetric about it
    -- up to what the declination moves between the two instants: at most 23.44 deg * 2 pi / 365.25 = 0.4035 degrees a day, and an
    elevation moves by no more than the declination does; 0.01 degrees for the equation of time's drift (at most 30 s a day)"""
    for month, day in ((1, 15), (3, 20), (6, 21), (9, 1), (11, 30)):
        doy = datetime.date(2021, month, day).timetuple().tm_yday
        guess = 12.0 - lon / 15.0
        _, eot = SO.solar_terms(2021, doy, guess % 24.0)
        noon = guess - float(eot) / 60.0                                                   # true solar time 12:00 in UTC hours
        base = datetime.datetime(2021, month, day)
        at = lambda hrs: SO.sun_position(base + datetime.timedelta(hours=hrs), lat, lon)   # noqa: E731
        decl, _ = SO.solar_terms(2021, doy, noon % 24.0)
        el, az = at(noon)
        assert abs(az - 180.0) <= 0.5 and abs(el - (90.0 - (lat - float(decl)))) <= 0.05, (month, day, el, az)
        for dt in (1.0, 3.5):
            (e1, a1), (e2, a2) = at(noon - dt), at(noon + dt)
            assert abs(e1 - e2) <= 0.4035 * 2.0 * dt / 24.0 + 0.01 and e1 < el and e2 < el and a1 < 180.0 < a2


def test_sun_position_takes_datetimes():
    utc = datetime.datetime(2021, 6, 21, 17, 30)
    one = SO.sun_position(utc, 30.3, -81.7)
    assert isinstance(one[0], float) and one == SO.sun_position(utc.replace(tzinfo=datetime.timezone.utc), 30.3, -81.7)
    local = utc.replace(tzinfo=datetime.timezone.utc).astimezone(datetime.timezone(datetime.timedelta(hours=-4)))
    assert one == SO.sun_position(local, 30.3, -81.7)
    el, az = SO.sun_position([utc, utc + datetime.timedelta(hours=6)], 30.3, -81.7)
    assert el.dtype == np.float64 and (el[0], az[0]) == one and el[1] < el[0] and az[1] > 270.0
    assert 75.0 < one[0] < 84.0                                                            # 13:30 local in Jacksonville at midsummer
    # the pairs are a `suns` list as cast_shadows takes it
    from snerf_amd.eval.utils import shadow as S
    assert S.sun_rows(list(zip(el[:1], az[:1])), 0.5).shape == (1, 3)


def test_sun_path():
    lat, lon = 30.3, -81.7
    suns, hours = SO.sun_path(lat, lon, 2021)
    assert suns.shape == (len(hours), 2) and (suns[:, 0] >= 5.0).all() and (hours == 1.0).all()
    fine, fine_hours = SO.sun_path(lat, lon, 2021, step_minutes=5)
    # the midpoint rule on an indicator: each of a day's two crossings is off by at most half a step, 730 crossings of either sign
    assert abs(hours.sum() - fine_hours.sum()) <= 0.01 * fine_hours.sum()
    coarse, coarse_hours = SO.sun_path(lat, lon, 2021, step_minutes=120, day_step=30)
    assert (coarse[:, 0] >= 5.0).all() and np.allclose(coarse_hours, 2.0 * 365 / 13) and abs(coarse_hours.sum() - fine_hours.sum()) <= 0.05 * fine_hours.sum()
    # without a threshold the sun is up half the year (no refraction, the disc's centre): 4380 h to 1 %.  Exactly so on the equator;
    # further north the longer summer half of the orbit adds to it (a percent at 64 degrees)
    for la in (0.0, 30.3):
        above = SO.sun_path(la, lon, 2021, step_minutes=10, min_elevation_deg=0.0)[1].sum()
        assert abs(above - 4380.0) <= 44.0, (la, above)
    low = SO.sun_path(lat, lon, 2021, min_elevation_deg=30.0)[1].sum()
    assert low < hours.sum() < 4380.0
    assert SO.sun_path(lat, lon, 2020)[1][0] == 1.0 and len(SO.sun_path(lat, lon, 2020, day_step=366)[1]) < 24


def test_clear_sky():
    dni, dhi = SO.clear_sky(np.array([-5.0, 0.0, 5.0, 30.0, 90.0]))
    assert dni[0] == dni[1] == 0.0 and (np.diff(dni[1:]) > 0.0).all() and np.array_equal(dhi, 0.1 * dni)
    assert abs(dni[4] - 1353.0 * 0.7) < 1.0 and 750.0 < dni[3] < 900.0                      # air mass 1 at the zenith, 2 at 30 degrees
    assert SO.clear_sky(90.0, solar_constant=1000.0, transmittance=1.0, diffuse_share=0.2) == (1000.0, 200.0)


def test_direction_rows_and_sun_table():
    for D in (1, 2, 4, 16, 64, 70, 720):
        rows = SO.direction_rows(D)
        assert rows.shape == (D, 2) and np.abs((rows ** 2).sum(1) - 1.0).max() <= 1e-15 and rows[0].tolist() == [0.0, -1.0]
        if D % 4 == 0:
            assert rows[D // 4].tolist() == [1.0, 0.0] and rows[D // 2].tolist() == [0.0, 1.0] and rows[3 * D // 4].tolist() == [-1.0, 0.0]
    assert np.allclose(SO.direction_rows(64)[8], [S2, -S2], rtol=0, atol=1e-15)
    rng = np.random.default_rng(5)
    suns = np.stack([rng.uniform(1.0, 89.0, 500), rng.uniform(-720.0, 720.0, 500)], 1)
    for D in (16, 64, 70):
        t = SO.sun_table(suns, np.ones(500), D, 0.5)
        assert (t[:, 1] >= 0.0).all() and (t[:, 1] < 1.0).all() and (t[:, 0] >= 0).all() and (t[:, 0] < D).all() and (t[:, 0] == np.floor(t[:, 0])).all()
        assert np.abs((t[:, 3:6] ** 2).sum(1) - 1.0).max() <= 1e-15 and (t[:, 5] > 0.0).all()
        assert np.allclose((t[:, 0] + t[:, 1]) * 360.0 / D, suns[:, 1] % 360.0, rtol=0, atol=1e-9)
        # a sun exactly on a sector stands on it
        on = SO.sun_table([(30.0, 360.0 * d / D) for d in range(D)], np.ones(D), D, 0.5)
        assert on[:, 0].tolist() == list(range(D)) and (on[:, 1] == 0.0).all()
    # the last sector wraps to the first: a sun between D - 1 and 0, one at 360 degrees and one a hair below it
    t = SO.sun_table([(30.0, 359.0), (30.0, 360.0), (30.0, 360.0 - 1e-13), (30.0, -1.0)], np.ones(4), 64, 0.5)
    assert t[:, 0].tolist() == [63.0, 0.0, 0.0, 63.0] and t[1, 1] == t[2, 1] == 0.0 and abs(t[0, 1] - (1.0 - 64.0 / 360.0)) < 1e-12
    hor = np.zeros((64, 1, 1), np.float32)
    hor[0] = 10.0                                                                           # a sun in the last sector reads plane 0
    assert N.irradiate(hor, t[:1])[1][0, 0] == 0 and N.irradiate(np.roll(hor, 32, 0), t[:1])[1][0, 0] == 1
    # (east, north, up) is construct_sun_dir's vector, the row's (ux, uy, rise) what sun_rows gives
    from snerf_amd.baseline.components.rays import construct_sun_dir
    from snerf_amd.eval.utils import shadow as S
    for el, az in ((35.0, 33.3), (12.25, 270.0), (80.0, 359.0)):
        row = SO.sun_table([(el, az)], [1.0], 64, 0.3)[0]
        assert np.abs(row[3:6] - construct_sun_dir(el, az, 1)[0].double().numpy()).max() <= 2e-7
        assert row[2] == S.sun_rows([(el, az)], 0.3)[0, 2]


def test_solar_table_on_hand_made_planes():
    nan = math.nan
    ids = torch.tensor([[1, 1, 2, 0], [1, 2, 2, 9]])
    res = {"global_kwh": torch.tensor([[1000.0, 1500.0, 800.0, 5000.0], [nan, 1200.0, 400.0, 7000.0]], dtype=torch.float64),
           "surface_factor": torch.tensor([[1.0, 1.25, 1.0, 1.0], [1.0, 2.0, 1.0, 1.0]], dtype=torch.float64),
           "sun_hours": torch.tensor([[3000.0, 3500.0, 2000.0, 0.0], [nan, 2500.0, 1500.0, 0.0]], dtype=torch.float64),
           "svf": torch.tensor([[1.0, 0.5, 0.75, 1.0], [nan, 0.25, 0.5, 1.0]])}
    t = SO.solar_table(res, ids, 3, 2.0, min_kwh_m2=1000.0)
    assert t["cells"].tolist() == [3, 3, 0] and t["valid_cells"].tolist() == [2, 3, 0] and t["plan_m2"].tolist() == [8.0, 12.0, 0.0]
    assert t["surface_m2"].tolist() == [4.0 + 5.0, 4.0 + 8.0 + 4.0, 0.0]
    assert t["annual_mwh"].tolist() == [(1000.0 * 4 + 1500.0 * 5) / 1000, (800.0 * 4 + 1200.0 * 8 + 400.0 * 4) / 1000, 0.0]
    assert t["mean_kwh_m2"][0] == 11500.0 / 9.0 and t["mean_kwh_m2"][1] == 14400.0 / 16.0 and np.isnan(t["mean_kwh_m2"][2])
    assert t["min_kwh_m2"].tolist()[:2] == [1000.0, 400.0] and t["max_kwh_m2"].tolist()[:2] == [1500.0, 1200.0] and np.isnan(t["min_kwh_m2"][2])
    assert t["mean_sun_hours"].tolist()[:2] == [3250.0, 2000.0] and t["mean_svf"].tolist()[:2] == [0.75, 0.5] and np.isnan(t["mean_svf"][2])
    assert t["good_m2"].tolist() == [9.0, 8.0, 0.0]
    assert SO.solar_table(res, ids, 3, 2.0, min_kwh_m2=1300.0)["good_m2"].tolist() == [5.0, 0.0, 0.0]
    # the order of the cells does not matter: a permutation gives the same words
    perm = torch.randperm(8, generator=torch.Generator().manual_seed(1))
    shuffled = {k: v.reshape(-1)[perm].reshape(2, 4) for k, v in res.items()}
    again = SO.solar_table(shuffled, ids.reshape(-1)[perm].reshape(2, 4), 3, 2.0)
    assert all(np.array_equal(again[k], t[k], equal_nan=True) for k in t)
    from snerf_amd.eval.utils.roofs import table_records
    rec = table_records(t)
    assert rec[0]["id"] == 1 and rec[2]["mean_kwh_m2"] is None and rec[1]["cells"] == 3
    with pytest.raises(ValueError, match="8 cells"):
        SO.solar_table(res, ids[:1], 3, 2.0)
