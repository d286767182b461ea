"""Solar potential on the map (include/snerf_solar.h, csrc/solar.hip, eval/utils/solar.py, eval/ortho.py export_solar; DESIGN.md section
5zb) on an MI355X.  The kernels do only fp64 + - * / and integer work, so every comparison with the numpy restatement
(tests/solar_numpy.py, itself held to a brute-force formulation and to the restated cast shadows by tests/test_solar_cpu.py) is bit for
bit: torch.equal on the counts, the bit patterns on the float planes."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import shadow as S
from snerf_amd.eval.utils import solar as SO
from snerf_amd.framework.util import img_utils
from tests import roofs_numpy as RN
from tests import shadow_numpy as SN
from tests import solar_numpy as N
from tests.test_gpu_fill import _filled, run_filled
from tests.test_gpu_shadow import HAND, KINDS, SHAPES, _make_dsm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 0.5
S2 = math.sqrt(0.5)
HAND_DIRS = np.asarray(HAND, np.float64)[:, :2]
# the 16 sectors, and the hand-made rows of tests/test_gpu_shadow.py: exact zeros and exact ties in all four quadrants
DIRS = np.concatenate([SO.direction_rows(16), HAND_DIRS])
# the subset the largest shape runs (the restatement loops over h + w steps in Python): off the axes, a tie row, two infinite tDeltas
DIRS_LARGE = np.concatenate([SO.direction_rows(16)[[3, 13]], HAND_DIRS[[0, 5, 2]]])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(got, want, what=""):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    assert np.array_equal(g, w), (what, int((g != w).sum()), g.size)


# ---- the horizon ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_horizon_matches_the_restatement_bit_for_bit(shape, kind):
    h, w = shape
    dsm = _make_dsm(kind, h, w)
    rows = DIRS_LARGE if h * w > 4096 else DIRS
    t = _dev(dsm)
    got = SO.horizon_rows(t, rows)                        # z_top: the default (the largest finite altitude); the restatement has none
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(rows), h, w)
    want = N.horizon(dsm, rows)
    _same(got, want, "bias 0, no max_dist")
    assert np.array_equal(np.isnan(want), np.broadcast_to(np.isnan(dsm), want.shape))
    _same(SO.horizon_rows(t, rows, bias=0.75, max_dist=3.5), N.horizon(dsm, rows, 0.75, 3.5), "bias 0.75, max_dist 3.5")
    _same(SO.horizon_rows(t, rows, bias=-0.5, max_dist=math.inf, z_top=math.inf), N.horizon(dsm, rows, -0.5), "bias -0.5")
    if kind == "flat":
        assert bool(((want == 0.0) | (want == -np.inf)).all())
    if kind in ("tower", "wall") and w >= 5:
        assert bool((want > 0.0).any())


def test_z_top_is_only_an_early_exit():
    dsm = _make_dsm("holes", 33, 64)
    t = _dev(dsm)
    top = float(np.nanmax(dsm))
    for bias in (0.0, 0.75, -3.0):
        want = N.horizon(dsm, DIRS, bias)
        for z in (math.inf, top, None, top + 100.0):
            _same(SO.horizon_rows(t, DIRS, bias, math.inf, z), want, (bias, z))
    _same(SO.horizon(t, RES, 16, max_dist_m=5.0), N.horizon(dsm, SO.direction_rows(16), 0.0, 10.0), "the public entry: metres to cells")


def test_64_directions_in_one_call_equal_64_calls_and_70_are_cut():
    dsm = _make_dsm("holes", 16, 17)
    t = _dev(dsm)
    rows = SO.direction_rows(64)
    all_ = SO.horizon_rows(t, rows)
    _same(all_, N.horizon(dsm, rows))
    for d in range(64):
        _same(SO.horizon_rows(t, rows[d:d + 1])[0], all_[d], d)
    _same(SO.horizon(t, RES, 70), N.horizon(dsm, SO.direction_rows(70)), "D = 70")
    with pytest.raises(ValueError, match="n_dirs = 65"):               # the library itself refuses what the host layer cuts
        r = np.ascontiguousarray(SO.direction_rows(70)[:65])
        _lib.call("snerf_solar_horizon", t, 16, 17, r.ctypes.data, 65, 0.0, math.inf, math.inf, torch.empty((65, 16, 17), device=DEV), exc=ValueError)


# ---- the horizon against the cast shadows, on the device -------------------------------------------------------------------------------
def _device_consistency(dsm, dirs, rises):
    """(pairs, in the band, disagreements outside it) of cast_shadows' lit against irradiate's lit_count under one sun at frac = 0"""
    t = _dev(dsm)
    hor = SO.horizon_rows(t, np.asarray(dirs, np.float64))
    H = hor.cpu().numpy().astype(np.float64)
    pairs = band = wrong = 0
    for d, (ux, uy) in enumerate(dirs):
        for rise in rises:
            lit = S.cast_rows(t, [(ux, uy, rise)])[0].cpu().numpy()
            _, count = SO.irradiate_rows(hor, [(float(d), 0.0, rise, 0.0, 0.0, 1.0, 1.0)])
            count = count.cpu().numpy()
            known = lit != SN.UNKNOWN
            assert bool(((count == 0) | (count == 1)).all()) and bool((count[~known] == 0).all())
            assert np.array_equal(count == 1, known & (rise >= H[d]))                     # what the kernel decides IS rise >= H
            with np.errstate(invalid="ignore"):
                close = known & np.isfinite(H[d]) & (np.abs(rise - H[d]) <= 2.0 ** -22 * np.abs(H[d]))
            differ = known & ~close & ((lit == 1) != (count == 1))
            pairs, band, wrong = pairs + int(known.sum()), band + int(close.sum()), wrong + int(differ.sum())
    return pairs, band, wrong


@pytest.mark.parametrize("kind", ("random", "holes", "tower", "wall", "flat"))
def test_the_horizon_decides_what_cast_shadows_decides(kind):
    """the claim of tests/test_solar_cpu.py on the device, with its inputs and caps: nothing in the band, no disagreement"""
    dsm = _make_dsm(kind, 33, 64)
    az = np.deg2rad((0.0, 90.0, 45.0, 33.3, 201.7, 270.0))
    dirs = [tuple(r) for r in np.stack([np.sin(az), -np.cos(az)], 1)]
    rises = [float(np.tan(np.deg2rad(el)) * RES) for el in (2.0, 11.0, 35.0, 45.0, 62.5)]
    pairs, band, wrong = _device_consistency(dsm, dirs, rises)
    print(f"{kind}: {pairs} pairs, {band} in the band, {wrong} disagree")
    assert pairs == int((~np.isnan(dsm)).sum()) * 30 and band == 0 and wrong == 0


def test_the_horizon_decides_it_on_exact_ties_too():
    dsm = (np.random.default_rng(3).integers(0, 40, (33, 64)) * 0.25).astype(np.float32)
    dirs = [tuple(r) for r in SO.direction_rows(4)] + [(S2, -S2)]
    pairs, band, wrong = _device_consistency(dsm, dirs, (0.125, 0.25, 0.5, 1.0))
    print(f"quantised: {pairs} pairs, {band} in the band, {wrong} disagree")
    assert pairs == 42240 and 0 < band <= 0.02 * pairs and wrong == 0


# ---- the sky-view factor --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planes(D):
    """the horizon planes of a DSM with holes at D sectors (the smaller raster at 720: the restatement marches in Python)"""
    return N.horizon(_make_dsm("holes", *((16, 17) if D > 64 else (33, 64))), SO.direction_rows(D))


@pytest.mark.parametrize("D", (1, 8, 64, 720))
def test_sky_view_is_the_restatements(D):
    hor = _planes(D)
    got = SO.sky_view(_dev(hor), RES)
    _same(got, N.svf(hor, RES))
    _same(SO.sky_view(_dev(hor), 2.0), N.svf(hor, 2.0), "res 2")
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(hor[0])) and float(torch.nan_to_num(got, nan=0.5).max()) <= 1.0


def test_sky_view_exact_cases():
    flat = SO.horizon(torch.full((5, 7), 3.0, device=DEV), RES, 16)
    assert bool((SO.sky_view(flat, RES) == 1.0).all())
    assert bool((SO.sky_view(torch.full((8, 2, 3), -math.inf, device=DEV), RES) == 1.0).all())
    for T in (0.5, 1.0, 3.0):
        got = SO.sky_view(torch.full((64, 2, 3), T * RES, device=DEV), RES)
        assert bool((got == float(np.float32(1.0 / (1.0 + T * T)))).all()), T


# ---- irradiate ------------------------------------------------------------------------------------------------------------------------
def _table(K, D, seed):
    """K random suns against D sectors; every fourth stands exactly on a sector (frac == 0)"""
    rng = np.random.default_rng(seed)
    suns = np.stack([rng.uniform(1.0, 80.0, K), rng.uniform(0.0, 360.0, K)], 1)
    suns[::4, 1] = 360.0 * rng.integers(0, D, len(suns[::4])) / D
    table = SO.sun_table(suns, rng.uniform(0.0, 900.0, K), D, RES)
    assert (table[::4, 1] == 0.0).all() and (K < 3 or (table[:, 1] > 0.0).any())
    return table


def _slopes(h, w, seed):
    rng = np.random.default_rng(seed)
    se, sn = (rng.uniform(-1.5, 1.5, (h, w)).astype(np.float32) for _ in range(2))
    se[1, 2], sn[3, 4] = np.nan, np.nan
    return se, sn


@pytest.mark.parametrize("with_slopes", (False, True), ids=("horizontal", "slopes"))
@pytest.mark.parametrize("K", (1, 3, 64, 130))
def test_irradiate_is_the_restatements(K, with_slopes):
    """one call for K <= 64, three for 130: the accumulators run on over the calls as the restatement's running sum does"""
    hor = _planes(64)
    h, w = hor.shape[1:]
    table = _table(K, 64, K)
    se, sn = _slopes(h, w, K) if with_slopes else (None, None)
    d_se, d_sn = (_dev(se), _dev(sn)) if with_slopes else (None, None)
    direct, count = SO.irradiate_rows(_dev(hor), table, d_se, d_sn)
    want_direct, want_count = N.irradiate(hor, table, se, sn)
    assert direct.dtype == torch.float64 and count.dtype == torch.int32
    _same(direct, want_direct)
    assert torch.equal(count.cpu(), torch.from_numpy(want_count.view(np.int32)))
    hole = np.isnan(hor[0])
    bad = hole | (np.isnan(se) | np.isnan(sn) if with_slopes else False)
    assert np.array_equal(np.isnan(want_direct), bad) and bool((want_count[hole] == 0).all()) and hole.any()
    if with_slopes:
        assert want_count[1, 2] == N.irradiate(hor, table)[1][1, 2]                       # a NaN slope: NaN, and counted all the same
    # continued from given accumulators: two halves of the table equal the whole
    if K > 1:
        cut = K // 2
        part = SO.irradiate_rows(_dev(hor), table[:cut], d_se, d_sn)
        direct2, count2 = SO.irradiate_rows(_dev(hor), table[cut:], d_se, d_sn, *part)
        _same(direct2, want_direct)
        assert torch.equal(count2, count)


def test_irradiate_edge_cases():
    """frac == 0 rows read one plane only (-inf beside them gives no NaN); a hole keeps its count; a sun behind the surface is counted
    lit and adds nothing; equality is lit"""
    hor = np.zeros((4, 2, 3), np.float32)
    hor[1] = -np.inf                                   # the plane beside sector 0 and sector 2
    hor[3] = -np.inf
    hor[2, 0, 1] = 0.5                                 # a tie with rise = 0.5
    hor[:, 1, 2] = np.nan
    up30, c30 = math.sin(math.radians(30.0)), math.cos(math.radians(30.0))
    table = np.array([[0.0, 0.0, 0.5, 0.0, c30, up30, 2.0],        # from the north, on sector 0
                      [2.0, 0.0, 0.5, 0.0, -c30, up30, 4.0],       # from the south, on sector 2: a tie on cell (0, 1)
                      [0.0, 0.5, 0.5, S2 * c30, S2 * c30, up30, 8.0]])   # between 0 and 1: 0.5 * 0 + 0.5 * -inf
    count0 = torch.full((2, 3), 7, dtype=torch.int32, device=DEV)
    direct, count = SO.irradiate_rows(_dev(hor), table, lit_count=count0)
    want = N.irradiate(hor, table, count=np.full((2, 3), 7, np.uint32))
    _same(direct, want[0])
    assert count.cpu().tolist() == want[1].tolist() == [[10, 10, 10], [10, 10, 7]]
    d = direct.cpu().numpy()
    assert np.isnan(d[1, 2]) and np.isfinite(np.delete(d.reshape(-1), 5)).all() and d[0, 0] == (2.0 * up30 + 4.0 * up30) + 8.0 * up30
    # a surface that falls to the north at 45 degrees: the southern sun at 30 degrees stands behind it
    se, sn = torch.zeros((2, 3), device=DEV), torch.full((2, 3), -1.0, device=DEV)
    direct, count = SO.irradiate_rows(_dev(hor), table[:2], se, sn)
    assert count.cpu().tolist() == [[2, 2, 2], [2, 2, 0]] and direct[0, 0].item() == 2.0 * (up30 + c30)
    _same(direct, N.irradiate(hor, table[:2], se.cpu().numpy(), sn.cpu().numpy())[0])
    # the public entry divides by the surface factor
    pub, _ = SO.irradiate(_dev(hor), 1.0, [(30.0, 0.0)], [2.0], se, sn)
    assert abs(pub[0, 0].item() - 2.0 * (up30 + c30) / math.sqrt(2.0)) < 1e-12
    with pytest.raises(ValueError, match="n_suns = 65"):
        big = np.ascontiguousarray(np.repeat(table[:1], 65, 0))
        _lib.call("snerf_solar_irradiate", _dev(hor), 4, 2, 3, None, None, big.ctypes.data, 65, torch.zeros((2, 3), dtype=torch.float64, device=DEV),
                  count0, exc=ValueError)


# ---- unwritten memory -----------------------------------------------------------------------------------------------------------------
def test_no_output_depends_on_bytes_the_library_did_not_write():
    """the three entries under the fills of tests/test_gpu_fill.py: horizon_out and svf_out are pure outputs (filled before the call),
    direct_acc and lit_count accumulators the caller zeroes; two runs under each fill and the three fills are bit-identical, and
    equal the restatement"""
    h, w = 33, 64
    dsm = _make_dsm("holes", h, w)
    t = _dev(dsm)
    rows = np.ascontiguousarray(DIRS)
    D = len(rows)
    table = np.ascontiguousarray(_table(64, D, 9))
    se, sn = _slopes(h, w, 9)
    d_se, d_sn = _dev(se), _dev(sn)

    def run(fill):
        hor, svf = _filled((D, h, w), torch.float32, fill), _filled((h, w), torch.float32, fill)
        _lib.call("snerf_solar_horizon", t, h, w, rows.ctypes.data, D, 0.0, math.inf, math.inf, hor)
        _lib.call("snerf_solar_svf", hor, D, h, w, RES, svf)
        direct, count = torch.zeros((h, w), dtype=torch.float64, device=DEV), torch.zeros((h, w), dtype=torch.int32, device=DEV)
        _lib.call("snerf_solar_irradiate", hor, D, h, w, d_se, d_sn, table.ctypes.data, 64, direct, count)
        return {"horizon": hor, "svf": svf, "direct": direct, "count": count}

    r = run_filled(run)[0xFF]
    want = N.horizon(dsm, rows)
    _same(r["horizon"], want)
    _same(r["svf"], N.svf(want, RES))
    want_direct, want_count = N.irradiate(want, table, se, sn)
    _same(r["direct"], want_direct)
    assert torch.equal(r["count"].cpu(), torch.from_numpy(want_count.view(np.int32)))


# ---- end to end: the town of tests/roofs_numpy.py ---------------------------------------------------------------------------------------
LAT, LON = 30.3, -81.7
COARSE = dict(day_step=30, step_minutes=120)


@pytest.fixture(scope="module")
def town():
    from snerf_amd.eval.utils import roofs as RF
    from tests.test_gpu_roofs import GRID, _town_objects
    key, ids, K, alt = RN.town()
    objects = _town_objects(alt, ids)
    roofs = RF.roofs(_dev(alt), objects["ids"], objects["n"], GRID, objects["table"])
    return {"alt": _dev(alt), "ids": ids, "grid": GRID, "objects": objects, "roofs": roofs}


def test_the_town_end_to_end(town):
    roofs = town["roofs"]
    res = SO.solar(town["alt"], town["grid"], LAT, LON, roofs["slope_e"], roofs["slope_n"], **COARSE)
    suns, hours = SO.sun_path(LAT, LON, 2021, **COARSE)
    assert res["n_suns"] == len(suns) > 40 and tuple(res["horizon"].shape) == (64,) + RN.TOWN_SHAPE
    for k in ("svf", "sun_hours", "direct_kwh", "diffuse_kwh", "global_kwh"):
        assert tuple(res[k].shape) == RN.TOWN_SHAPE and bool(torch.isfinite(res[k]).all()), k
    assert res["svf"].dtype == torch.float32 and res["direct_kwh"].dtype == torch.float64
    # the planes are the restatement's: the horizon and svf bit for bit, the counts exactly
    alt = town["alt"].cpu().numpy()
    want_hor = N.horizon(alt, SO.direction_rows(64))
    _same(res["horizon"], want_hor)
    _same(res["svf"], N.svf(want_hor, RES))
    se, sn = (torch.nan_to_num(roofs[k], nan=0.0).cpu().numpy() for k in ("slope_e", "slope_n"))
    dni, dhi = SO.clear_sky(suns[:, 0])
    want_direct, want_count = N.irradiate(want_hor, SO.sun_table(suns, dni * hours / 1000.0, 64, RES), se, sn)
    assert torch.equal(res["lit_count"].cpu(), torch.from_numpy(want_count.view(np.int32)))
    # (the division by the surface factor is torch's: its sqrt and quotient are held to 2 ulp, not to the bit)
    assert np.allclose(res["direct_kwh"].cpu().numpy(), want_direct / np.sqrt(1.0 + se.astype(np.float64) ** 2 + sn.astype(np.float64) ** 2),
                       rtol=4.5e-16, atol=0.0)
    zenith = lambda hrs: np.concatenate([SO.sun_table(suns, hrs, 64, RES)[:, :3], np.tile([0.0, 0.0, 1.0], (len(suns), 1)), hrs[:, None]], 1)  # noqa: E731
    _same(res["sun_hours"], N.irradiate(want_hor, zenith(hours))[0])                      # the hours as weights on a level unit surface
    assert np.allclose(res["sun_hours"].cpu().numpy(), want_count * hours[0], rtol=1e-12, atol=0.0)
    assert torch.equal(res["global_kwh"], res["direct_kwh"] + res["diffuse_kwh"])
    # the hipped roof's south-facing facet gets strictly more direct sun than its north-facing one (codes 5 and 1 of building 3)
    t = roofs["facets"]
    facet = {int(c): k + 1 for k, (o, c) in enumerate(zip(t["object"].tolist(), t["code"].tolist())) if o == 3}
    fid = roofs["facet_ids"]
    south, north = (res["direct_kwh"][fid == facet[c]] for c in (5, 1))
    assert south.numel() == north.numel() == 90 and float(south.mean()) > float(north.mean()) and float(south.min()) > float(north.max())
    # the upper level of the two-level building is the highest flat roof in town: svf is exactly 1; beside the 6 m step it is not
    ids = torch.from_numpy(town["ids"]).to(DEV)
    cols = torch.arange(RN.TOWN_SHAPE[1], device=DEV).expand(RN.TOWN_SHAPE)
    upper, beside = (ids == 5) & (cols >= 54), (ids == 5) & (cols == 53)
    # (an endless wall beside a cell leaves it half the sky; this one is 20 cells long and 12 cells high, and the roofs to the west
    # take a little of the other half)
    assert bool((res["svf"][upper] == 1.0).all()) and bool((res["svf"][beside] < 1.0).all()) and 0.4 < float(res["svf"][33, 53]) < 0.6
    assert float(res["sun_hours"][beside].max()) < float(res["sun_hours"][upper].min()) and abs(float(res["sun_hours"][upper].min()) - hours.sum()) < 1e-9
    # caller-supplied suns with unequal hours
    h2 = hours * np.linspace(0.5, 1.5, len(hours))
    own = SO.solar(town["alt"], town["grid"], LAT, LON, suns=suns, hours=h2, dni=dni, dhi=dhi)
    _same(own["sun_hours"], N.irradiate(want_hor, zenith(h2))[0])
    assert float(own["sun_hours"][upper].max()) == float(own["sun_hours"].max()) and abs(float(own["sun_hours"].max()) - h2.sum()) < 1e-9
    # the tables: the buildings' and the facets'
    b = SO.solar_table(res, town["objects"]["ids"], 5, RES)
    assert b["cells"].tolist() == [120, 256, 400, 196, 240] and b["valid_cells"].tolist() == b["cells"].tolist()
    assert b["surface_m2"][0] == 30.0 and b["surface_m2"][1] > 64.0 and b["mean_svf"][4] < 1.0 and (b["annual_mwh"] > 0).all()


def _read_all(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_export_solar_on_the_town(town, tmp_path):
    products = {"dsm": town["alt"], "grid": town["grid"]}
    before = EO.export_roofs(products, town["objects"], str(tmp_path / "a"), zone_string="17R")
    out = EO.export_solar(products, str(tmp_path), roofs_result=town["roofs"], objects_result=town["objects"], lat_deg=LAT, lon_deg=LON,
                          zone_string="17R", **COARSE)
    after = EO.export_roofs(products, town["objects"], str(tmp_path / "b"), zone_string="17R")
    assert _read_all(tmp_path / "a" / "roofs") == _read_all(tmp_path / "b" / "roofs") and set(before["files"]) == set(after["files"])
    names = {"svf.tif", "svf.png", "sun_hours.tif", "sun_hours.png", "insolation.tif", "insolation.png", "solar.json"}
    d = tmp_path / "solar"
    assert set(out["files"]) == names == set(os.listdir(d)) and all(os.path.getsize(p) > 0 for p in out["files"].values())
    grid = town["grid"]
    for name, plane in (("svf", out["svf"]), ("sun_hours", out["sun_hours"].float()), ("insolation", out["global_kwh"].float())):
        arr, tf = img_utils.load_dsm_geotiff(out["files"][name + ".tif"])
        assert arr.dtype == np.float32 and tf == (grid.xoff, grid.yoff, 0.5, 0.5), name
        _same(arr, plane, name)
    doc = json.load(open(out["files"]["solar.json"]))
    assert doc["n_suns"] == out["n_suns"] and doc["parameters"]["lat_deg"] == LAT and doc["parameters"]["alt_key"] == "dsm"
    assert doc["parameters"]["day_step"] == 30 and doc["parameters"]["D"] == 64
    assert [r["cells"] for r in doc["buildings"]] == [120, 256, 400, 196, 240] and len(doc["facets"]) == town["roofs"]["n_facets"] == 10
    assert [r["annual_mwh"] for r in doc["buildings"]] == out["buildings"]["annual_mwh"].tolist()
    assert [r["mean_kwh_m2"] for r in doc["facets"]] == out["facets"]["mean_kwh_m2"].tolist()
    # the site from the grid's centre through a GeoFrame: zone 17R, 16 m east of the central meridian, 4,100 km north of the equator
    from snerf_amd.framework.util.conversions import _zone_frame
    geo = EO.export_solar(products, str(tmp_path / "geo"), geo=_zone_frame("17R"), **COARSE)
    p = geo["parameters"]
    assert abs(p["lon_deg"] + 81.0) < 1e-3 and 36.9 < p["lat_deg"] < 37.2 and geo["facets"] is None and geo["buildings"] is None
    with pytest.raises(ValueError, match="lat_deg and lon_deg"):
        EO.export_solar(products, str(tmp_path / "none"), **COARSE)
