"""CPU-side checks of the roof planes (include/snerf_roofs.h, csrc/roofs.hip, eval/utils/roofs.py): the new
header's prototypes and constants against the binding (_lib.HEADER_SIGNATURES), the restatement (tests/roofs_numpy.py, the oracle of
tests/test_gpu_roofs.py) against numpy.linalg.lstsq, exact integer planes and scipy.ndimage.label, the host tables on hand-made words,
the synthetic town's exact facts, and every refusal of the four entries through the binding (none reaches a launch)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import roofs as RF            # the feature under test: every test of this file needs it
from tests import roofs_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_roofs.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_roofs_normals": ["key", "ids", "h", "w", "K", "radius", "q", "res", "cos0", "sin0", "tan2_flat", "tan2_wall", "slope_e", "slope_n",
                            "code", "tag", "stats", "stream"],
    "snerf_roofs_link": ["tag", "h", "w", "connectivity", "parent", "stats", "stream"],
    "snerf_roofs_moments": ["fids", "root", "key", "tag", "h", "w", "F", "row0", "row1", "rows", "stats", "stream"],
    "snerf_roofs_residuals": ["fids", "root", "key", "h", "w", "F", "planes", "q", "unit", "row0", "row1", "residual", "rows", "stats", "stream"],
}


def test_the_new_header_matches_its_binding_rows():
    """include/snerf_roofs.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py), then the constants; the main header, the
    main table, the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_roofs.h", NAMES)
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SNERF_ROOFS_\w+) (\d+)", text)}
    assert consts["SNERF_ROOFS_MAX_RADIUS"] == _lib.ROOFS_MAX_RADIUS == RF.MAX_RADIUS == N.MAX_RADIUS == 4
    assert consts["SNERF_ROOFS_MAX_SIDE"] == _lib.ROOFS_MAX_SIDE == RF.MAX_SIDE == 8192
    assert consts["SNERF_ROOFS_MAX_OBJECTS"] == _lib.ROOFS_MAX_OBJECTS == RF.MAX_OBJECTS == 2 ** 27
    assert (consts["SNERF_ROOFS_MOMENT_WORDS"], consts["SNERF_ROOFS_RESIDUAL_WORDS"]) == (_lib.ROOFS_MOMENT_WORDS, _lib.ROOFS_RESIDUAL_WORDS) == \
        (len(N.MOMENT_INIT), len(N.RESIDUAL_INIT)) == (16, 8)
    codes = tuple(consts["SNERF_ROOFS_" + n] for n in ("FLAT", "STEEP", "HOLE", "DEGENERATE", "NONE"))
    assert codes == (_lib.ROOFS_FLAT, _lib.ROOFS_STEEP, _lib.ROOFS_HOLE, _lib.ROOFS_DEGENERATE, _lib.ROOFS_NONE) == \
        (RF.FLAT, RF.STEEP, RF.HOLE, RF.DEGENERATE, RF.NONE) == (N.FLAT, N.STEEP, N.CODE_HOLE, N.DEGENERATE, N.NONE) == (0, 9, 253, 254, 255)
    assert (N.Z0, N.Q, N.UNIT, N.HOLE) == (RF.OR.Z0, RF.OR.Q, RF.UNIT, _lib.TERRAIN_HOLE)
    assert tuple(v % 2 ** 64 for v in RF._MOMENT_INIT) == N.MOMENT_INIT and tuple(v % 2 ** 64 for v in RF._RESIDUAL_INIT) == N.RESIDUAL_INIT


# ---- the restatement's normals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_the_restatements_normals_are_least_squares_planes(radius):
    """Cramer's rule on the integer sums against numpy.linalg.lstsq on the same support, to 1e-9 relative; the sums of all cells at
    once (numpy, int64) against the literal loop in Python ints"""
    h, w = 12, 17
    key = N.key_raster(h, w, "random")
    ids, K = N.id_raster(h, w, "blobs")
    ids = np.where((ids < 0) | (ids > K), 0, ids)
    planes = N.window_sum_planes(key, ids, radius)
    checked = 0
    for j in range(h):
        for i in range(w):
            if ids[j, i] <= 0 or not N.valid(int(key[j, i])):
                continue
            sums = N.window_sums(key, ids, j, i, radius)
            assert sums == [int(v) for v in planes[:, j, i]]
            D_, Nx, Ny = N.cramer(sums)
            pts = [(di, dj, int(key[j + dj, i + di]) - int(key[j, i])) for dj in range(-radius, radius + 1) for di in range(-radius, radius + 1)
                   if 0 <= j + dj < h and 0 <= i + di < w and ids[j + dj, i + di] == ids[j, i] and N.valid(int(key[j + dj, i + di]))]
            A = np.array([[1.0, di, dj] for di, dj, _ in pts])
            if np.linalg.matrix_rank(A) < 3:
                assert D_ == 0
                continue
            assert D_ > 0
            sol = np.linalg.lstsq(A, np.array([float(d) for _, _, d in pts]), rcond=None)[0]
            scale = max(abs(sol[1]), abs(sol[2]), 1.0)
            assert abs(Nx / D_ - sol[1]) <= 1e-9 * scale and abs(Ny / D_ - sol[2]) <= 1e-9 * scale
            checked += 1
    assert checked > 40


def test_integer_planes_come_back_exactly_on_partial_supports():
    """keys alpha i + beta j + gamma: Nx = alpha D and Ny = beta D exactly whatever the non-collinear support, so the slopes are
    alpha q / res and -beta q / res to the bit; a collinear or single-cell support is degenerate"""
    h, w = 9, 20
    jj, ii = np.mgrid[0:h, 0:w]
    ids, K = N.id_raster(h, w, "blobs")
    ids = np.where((ids < 0) | (ids > K), 0, ids)
    for alpha, beta in ((7001, -3999), (0, 12345), (-2 ** 20, 2 ** 19 + 1)):
        key = np.where(N.hole_mask("random", h, w), N.HOLE, alpha * ii + beta * jj - 4242).astype(np.int32)
        for radius in (1, 4):
            seen = 0
            for j in range(h):
                for i in range(w):
                    if ids[j, i] <= 0 or not N.valid(int(key[j, i])):
                        continue
                    D_, Nx, Ny = N.cramer(N.window_sums(key, ids, j, i, radius))
                    assert (Nx, Ny) == (alpha * D_, beta * D_)
                    seen += D_ > 0
            se, sn, code, tag, stats = N.normals(key, ids, K, radius, N.Q, 0.5)
            has = code <= 9
            assert has.sum() == stats[1] == seen > 30
            assert (se[has] == np.float32(alpha * N.Q / 0.5)).all() and (sn[has] == np.float32(-beta * N.Q / 0.5)).all()
    # a single row: every support is collinear; a single cell; a lone object cell among others
    line = np.arange(10, dtype=np.int32).reshape(1, 10) * 100
    assert (N.normals(line, np.ones((1, 10), np.int32), 1, 2, N.Q, 0.5)[2] == N.DEGENERATE).all()
    assert N.normals(np.zeros((1, 1), np.int32), np.ones((1, 1), np.int32), 1, 1, N.Q, 0.5)[4] == [1, 0, 1, 0]
    lone = np.zeros((3, 3), np.int32)
    lone[1, 1] = 1
    out = N.normals(np.zeros((3, 3), np.int32), lone, 1, 1, N.Q, 0.5)
    assert out[2][1, 1] == N.DEGENERATE and (out[2] == N.NONE).sum() == 8 and (out[3] == -1).all() and np.isnan(out[0]).all()


def test_the_orientation_codes():
    """the octants of a plane that falls to each of 16 compass directions, flat and steep, and a rotated aspect0"""
    t5, t60 = N.tan2(5.0), N.tan2(60.0)
    def gradient(fall_deg):
        # a surface that falls to (east, north) = (sin f, cos f) rises by a = -sin f per metre east and b = cos f per metre south
        return -0.5 * math.sin(math.radians(fall_deg)), 0.5 * math.cos(math.radians(fall_deg))

    for k in range(16):
        for off in (-5.0, 5.0):
            fall = (22.5 * k + off) % 360.0                  # where the surface falls to, clockwise from north; never on a bin edge
            a, b = gradient(fall)
            assert N.classify(a, b, 1.0, 0.0, t5, t60) == 1 + int(((fall + 22.5) % 360.0) // 45.0), (k, off)
            # bins turned clockwise by aspect0: the code of a surface that falls to fall - aspect0 between unturned bins
            for a0 in (30.0, -100.0):
                r = math.radians(a0)
                assert N.classify(a, b, math.cos(r), math.sin(r), t5, t60) == N.classify(*gradient(fall - a0), 1.0, 0.0, t5, t60), (k, off, a0)
    assert N.classify(0.0, 0.0, 1.0, 0.0, t5, t60) == 0 and N.classify(0.05, 0.05, 1.0, 0.0, t5, t60) == 0
    assert N.classify(math.sqrt(t5), 0.0, 1.0, 0.0, t5, t60) in (0, 7) and N.classify(1.8, 0.0, 1.0, 0.0, t5, t60) == 9
    assert N.classify(0.5, 0.0, 1.0, 0.0, t5, t60) == 7 and N.classify(-0.5, 0.0, 1.0, 0.0, t5, t60) == 3
    assert N.classify(0.0, 0.5, 1.0, 0.0, t5, t60) == 1 and N.classify(0.0, -0.5, 1.0, 0.0, t5, t60) == 5
    assert RF.OCTANTS == ("N", "NE", "E", "SE", "S", "SW", "W", "NW")


# ---- the restatement's link -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_restatements_link_is_scipys_label_per_tag(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (1, 40), (9, 1), (13, 21), (33, 64)):
        tag = rng.integers(-1, 4, (h, w)).astype(np.int32) * 16 + np.where(rng.random((h, w)) < 0.5, 3, 7)
        tag[tag < 0] = -1
        parent, stats = N.link(tag, connectivity)
        assert stats == [0, int((tag >= 0).sum())] and parent.dtype == np.int32 and parent.shape == (h * w,)
        want = np.full(h * w, -1, np.int64)
        for value in np.unique(tag[tag >= 0]):
            lab, n = ndimage.label(tag == value, structure=structure)
            flat = lab.reshape(-1)
            for c in range(1, n + 1):
                cells = np.flatnonzero(flat == c)
                want[cells] = cells.min()
        assert np.array_equal(parent, want), (h, w)
        fids, F = N.ids_from_parent(parent, h, w)
        assert F == len(np.unique(parent[parent >= 0])) and (fids.reshape(-1)[parent < 0] == 0).all()
        roots = np.flatnonzero(parent == np.arange(h * w))
        assert fids.reshape(-1)[roots].tolist() == list(range(1, F + 1))


# ---- the host tables --------------------------------------------------------------------------------------------------------------------
GRID = D.DsmGrid(1000.0, 2000.0, 0.5, 40, 30)


def _moment_row(cells, root, tag, w=40, left_out=0):
    """the 16 words of a facet from its cells [(j, i, k)] and its root cell's (j0, i0, k0)"""
    j0, i0, k0 = root
    row = list(N.MOMENT_INIT)
    for j, i, k in cells:
        di, dj, dk = i - i0, j - j0, k - k0
        for n, v in enumerate((1, di, dj, dk, di * di, di * dj, dj * dj, di * dk, dj * dk)):
            row[n] += v
        row[9], row[10], row[11], row[12] = min(row[9], i), max(row[10], i), min(row[11], j), max(row[12], j)
    row[13], row[14], row[15] = tag, j0 * w + i0, left_out
    return row


def test_facet_table_on_hand_made_words():
    """a 4 x 3 facet on the plane k = 655360 + 16384 i - 8192 j (0.25 m per cell east, 0.125 m down per cell south: the slopes 0.5
    east and 0.25 north), a level one, a strip one cell wide and an empty row"""
    cells = [(j, i, 655360 + 16384 * i - 8192 * j) for j in range(5, 8) for i in range(10, 14)]
    level = [(j, i, 700000) for j in range(20, 22) for i in range(3, 6)]
    strip = [(9, i, 655360 + 100 * i) for i in range(20, 26)]
    rows = N.words([_moment_row(cells, cells[0], 2 * 16 + 6), _moment_row(level, level[0], 2 * 16 + 0), _moment_row(strip, strip[0], 3 * 16 + 7, left_out=2),
                    list(N.MOMENT_INIT)])
    root_key = np.array([cells[0][2], 700000, strip[0][2], 0])
    t = RF.facet_table(rows.view(np.int64), GRID, root_key=root_key)
    assert t["object"].tolist() == [2, 2, 3, 0] and t["code"].tolist() == [6, 0, 7, 0] and t["area_cells"].tolist() == [12, 6, 6, 0]
    assert t["left_out"].tolist() == [0, 0, 2, 0] and t["area_m2"].tolist() == [3.0, 1.5, 1.5, 0.0]
    assert t["plane"][0].tolist() == [0.0, 16384.0, -8192.0] and t["plane"][1].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(t["plane"][2]).all() and np.isnan(t["plane"][3]).all()                   # collinear cells; no cells
    assert t["plane"].tolist()[0] == list(N.solve(_moment_row(cells, cells[0], 0))) == list(RF.solve(_moment_row(cells, cells[0], 0)))
    assert (t["slope_e"][0], t["slope_n"][0]) == (0.5, 0.25) and (t["slope_e"][1], abs(t["slope_n"][1])) == (0.0, 0.0)
    s = math.sqrt(0.3125)
    assert t["pitch_deg"][0] == np.degrees(np.arctan(s)) and t["pitch_deg"][1] == 0.0 and np.isnan(t["pitch_deg"][2])
    # rises to the east and to the north: falls to the south-west, atan2(-0.5, -0.25) clockwise from north
    assert t["azimuth_deg"][0] == math.degrees(math.atan2(-0.5, -0.25)) % 360.0 and 180.0 < t["azimuth_deg"][0] < 270.0
    assert np.isnan(t["azimuth_deg"][1]) and t["surface_m2"][0] == 3.0 * math.sqrt(1.3125) and t["surface_m2"][1] == 1.5
    assert (t["east"][0], t["north"][0]) == (1000.0 + 12.0 * 0.5, 2000.0 - 6.5 * 0.5) and t["bbox"][0].tolist() == [1005.0, 1996.0, 1007.0, 1997.5]
    assert np.isnan(t["bbox"][3]).all() and t["root"].tolist() == [5 * 40 + 10, 20 * 40 + 3, 9 * 40 + 20, 0]
    # the plane at the centroid (i = 11.5, j = 6): 655360 + 16384 * 11.5 - 8192 * 6 keys
    assert t["alt"][0] == (655360 + 16384 * 11.5 - 8192 * 6) / 65536 and t["alt"][1] == 700000 / 65536
    assert np.isnan(RF.facet_table(rows.view(np.int64), GRID)["alt"]).all()                    # without the roots' keys
    # residual words: n, sum |rq|, sum rq^2, max |rq|, min and max key + 2^31, clamped
    bias = 2 ** 31
    res_rows = N.words([[12, 24, 96, 4, 655360 + bias, 700000 + bias, 1, 0], [6, 0, 0, 0, 700000 + bias, 700000 + bias, 0, 0],
                        list(N.RESIDUAL_INIT), list(N.RESIDUAL_INIT)])
    t = RF.facet_table(rows.view(np.int64), GRID, root_key=root_key, residual_rows=res_rows.view(np.int64))
    step = 64.0 / 65536
    assert t["rms_m"][0] == step * math.sqrt(8.0) and t["mean_abs_m"][0] == step * 2.0 and t["max_abs_m"][0] == step * 4.0
    assert t["clamped"].tolist() == [1, 0, 0, 0] and t["residual_cells"].tolist() == [12, 6, 0, 0]
    assert (t["eave_alt"][0], t["ridge_alt"][0]) == (10.0, 700000 / 65536) and np.isnan(t["rms_m"][2]) and np.isnan(t["eave_alt"][3])
    with pytest.raises(ValueError, match="4 rows but 1 residual rows"):
        RF.facet_table(rows.view(np.int64), GRID, residual_rows=res_rows[:1].view(np.int64))
    # filter_facets: the small one and the ones without a plane go; the ids are compacted in order
    fids = torch.tensor([[0, 1, 2, 3], [4, 2, 1, 0]], dtype=torch.int32)
    kept_ids, kept = RF.filter_facets(fids, t, min_facet_m2=2.0)
    assert kept_ids.tolist() == [[0, 1, 0, 0], [0, 0, 1, 0]] and kept["area_cells"].tolist() == [12] and kept_ids.dtype == torch.int32
    kept_ids, kept = RF.filter_facets(fids, t)
    assert kept_ids.tolist() == [[0, 1, 2, 0], [0, 2, 1, 0]] and kept["code"].tolist() == [6, 0] and set(kept) == set(t)
    records = RF.table_records(kept)
    assert records[0]["id"] == 1 and records[1]["azimuth_deg"] is None and records[0]["plane"] == [0.0, 16384.0, -8192.0]


def _facets(rows):
    """a facet table from (object, code, area_m2, pitch, azimuth, rms, cells, eave, ridge) tuples"""
    cols = ("object", "code", "area_m2", "pitch_deg", "azimuth_deg", "rms_m", "residual_cells", "eave_alt", "ridge_alt")
    return {c: np.array([r[k] for r in rows], np.int64 if c in ("object", "code", "residual_cells") else np.float64) for k, c in enumerate(cols)}


def test_roof_table_on_hand_made_facets():
    nan = math.nan
    facets = _facets([
        (1, 0, 40.0, 0.0, nan, 0.25, 160, 20.0, 20.0), (1, 0, 10.0, 0.0, nan, 0.5, 40, 23.0, 23.0), (1, 3, 5.0, 30.0, 90.0, 0.0, 20, 20.0, 21.0),
        (2, 7, 30.0, 35.0, 270.0, 0.3, 120, 14.0, 18.0),                                           # shed
        (3, 2, 20.0, 40.0, 45.0, 0.0, 80, 11.0, 15.0), (3, 6, 25.0, 42.0, 225.0, 0.0, 100, 11.0, 15.5), (3, 4, 2.0, 10.0, 135.0, 0.0, 8, 12.0, 12.5),
        (4, 1, 10.0, 30.0, 0.0, 0.0, 40, 10.0, 12.0), (4, 3, 10.0, 30.0, 90.0, 0.0, 40, 10.0, 12.0), (4, 5, 10.0, 30.0, 180.0, 0.0, 40, 10.0, 12.0),
        (4, 7, 10.0, 30.0, 270.0, 0.0, 40, 10.0, 12.0),                                            # hipped
        (5, 1, 10.0, 30.0, 0.0, 0.0, 40, 10.0, 12.0), (5, 3, 10.0, 30.0, 90.0, 0.0, 40, 10.0, 12.0),   # two, not opposed
        (7, 2, 12.0, 20.0, 45.0, 0.0, 48, 9.0, 10.0), (7, 0, 12.0, 0.0, nan, 0.0, 48, 10.0, 10.0),
    ])
    objects = {"area_cells": np.arange(7), "ground_alt": np.array([10.0, 8.0, 5.0, 4.0, 4.0, 3.0, nan])}
    b = RF.roof_table(facets, objects)
    assert b["roof_type"].tolist() == ["flat", "shed", "gabled", "hipped", "complex", "none", "shed"]
    assert b["levels"].tolist() == [2, 0, 0, 0, 0, 0, 0] and b["facets"].tolist() == [3, 1, 3, 4, 2, 0, 2]
    assert b["flat_facets"].tolist() == [2, 0, 0, 0, 0, 0, 1] and b["pitched_facets"].tolist() == [1, 1, 3, 4, 2, 0, 1]
    assert b["pitched_share"][0] == 5.0 / 55.0 and b["flat_share"][0] == 50.0 / 55.0 and b["facet_area_m2"].tolist()[:3] == [55.0, 30.0, 47.0]
    assert b["pitch_deg"].tolist()[:4] == [0.0, 35.0, 42.0, 30.0] and b["azimuth_deg"][1] == 270.0 and b["azimuth_deg"][2] == 225.0
    assert b["pitch_mean_deg"][2] == (20.0 * 40.0 + 25.0 * 42.0 + 2.0 * 10.0) / 47.0
    assert b["rms_m"][0] == math.sqrt((160 * 0.0625 + 40 * 0.25) / 220) and b["rms_m"][1] == 0.3
    assert (b["eave_height"][0], b["ridge_height"][0]) == (10.0, 13.0) and (b["eave_height"][2], b["ridge_height"][2]) == (6.0, 10.5)
    assert np.isnan(b["pitch_deg"][5]) and np.isnan(b["eave_height"][6]) and b["roof_type"][5] == "none"
    # the thresholds are parameters.  Building 1 at a stricter flat share: its one pitched facet holds 9 % of the area, below the major
    # share, so nothing counts ("complex") until that is lowered too ("shed"); building 3 with its small third facet counted
    assert RF.roof_table(facets, objects, flat_share=0.05)["roof_type"][0] == "complex"
    assert RF.roof_table(facets, objects, flat_share=0.05, major_share=0.05)["roof_type"][0] == "shed"
    assert RF.roof_table(facets, objects, major_share=0.01)["roof_type"][2] == "complex"


def test_roof_agreement_on_hand_made_maps():
    nan = math.nan

    def roof(types, pitch, azimuth, se, sn):
        return {"buildings": {"roof_type": np.array(types, dtype=object), "pitch_deg": np.array(pitch), "azimuth_deg": np.array(azimuth)},
                "slope_e": torch.tensor(se), "slope_n": torch.tensor(sn)}

    a = roof(["flat", "gabled", "shed"], [0.0, 30.0, 20.0], [nan, 90.0, 10.0], [[0.0, 1.0, nan]], [[0.0, 0.0, 0.5]])
    b = roof(["gabled", "flat", "shed", "shed"], [28.0, 0.0, 25.0, 20.0], [100.0, nan, 350.0, 200.0], [[0.0, 0.0, 0.5]], [[0.0, 1.0, nan]])
    s = RF.roof_agreement(a, b, torch.tensor([[1, 2], [2, 1], [3, 3]]))
    assert s["pairs"] == 3 and s["types"] == ["flat", "gabled", "shed"] and s["type_table"] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert s["type_agreement"] == 1.0 and [p["pitch_error_deg"] for p in s["per_pair"]] == [0.0, 2.0, -5.0] and s["pitch_mae_deg"] == 7.0 / 3
    assert [p["azimuth_agrees"] for p in s["per_pair"]] == [None, True, True]                  # 10 against 350 degrees: 20 apart
    # normals (0, 0, 1) against (0, 0, 1): 0 degrees; (-1, 0, 1) against (0, -1, 1): 60 degrees; the third cell has no pair
    assert s["normal_cells"] == 2 and abs(s["normal_angle_mean_deg"] - 30.0) < 1e-9 and s["normal_angle_median_deg"] == 0.0
    s = RF.roof_agreement(a, b, [[1, 1], [3, 4]])
    assert s["types"] == ["flat", "gabled", "shed"] and s["type_table"] == [[0, 1, 0], [0, 0, 0], [0, 0, 1]] and s["type_agreement"] == 0.5
    assert [p["azimuth_agrees"] for p in s["per_pair"]] == [None, False]
    e = RF.roof_agreement(a, b, np.zeros((0, 2), np.int64))
    assert e["pairs"] == 0 and e["type_agreement"] is None and e["pitch_mae_deg"] is None and e["type_table"] == []
    with pytest.raises(ValueError, match=r"\(1, 3\) and \(1, 2\)"):
        RF.roof_agreement(a, roof([], [], [], [[0.0, 0.0]], [[0.0, 0.0]]), [])


# ---- the town -------------------------------------------------------------------------------------------------------------------------
def test_the_town():
    """the facts of DESIGN.md section 5z at r = 1, flat 5 degrees, wall 60 degrees, 4-connectivity, from the restatement and the host
    tables"""
    key, ids, K, alt = N.town()
    assert key.shape == N.TOWN_SHAPE and K == 5 and np.array_equal(np.rint((alt.astype(np.float64) - N.Z0) / N.Q), key)
    r = N.roofs(key, ids, K, N.TOWN_RES)
    assert r["stats"]["normals"] == [1212, 1212, 0, 0]                                        # no cell is degenerate
    per_building = {n: sorted((int(row[13]) & 15, row[0]) for row in r["moments"] if int(row[13]) >> 4 == n) for n in range(1, 6)}
    assert per_building[1] == [(0, 120)] and per_building[2] == [(3, 128), (7, 128)] and per_building[4] == [(1, 196)]
    assert [f for f in per_building[3] if f[1] > 1] == [(1, 90), (3, 90), (5, 90), (7, 90)]
    assert sorted(f for f in per_building[3] if f[1] == 1) == [(2, 1)] * 10 + [(4, 1)] * 10 + [(6, 1)] * 10 + [(8, 1)] * 10
    assert per_building[5] == [(0, 100), (0, 100)] and int(((r["code"] == 9) & (ids == 5)).sum()) == 40 == int((r["code"] == 9).sum())
    grid = D.DsmGrid(500000.0, 4100000.0, N.TOWN_RES, N.TOWN_SHAPE[1], N.TOWN_SHAPE[0])
    root_key = np.array([key.reshape(-1)[row[14]] for row in r["moments"]])
    table = RF.facet_table(N.words(r["moments"]).view(np.int64), grid, root_key=root_key, residual_rows=N.words(r["residual_rows"]).view(np.int64))
    assert np.array_equal(table["plane"].view(np.uint64), r["planes"].view(np.uint64))
    fids, kept = RF.filter_facets(torch.from_numpy(r["fids"]), table, min_facet_m2=4.0)
    assert len(kept["object"]) == 10 and int((fids > 0).sum()) == 1132
    # exactly planar: every residual word of a kept facet is 0; every pitch is exactly 0 or atan(1/2)
    assert all(r["residual_rows"][k][1:4] == [0, 0, 0] and r["residual_rows"][k][6] == 0 for k, row in enumerate(r["moments"]) if row[0] > 1)
    assert (kept["rms_m"] == 0.0).all() and (kept["max_abs_m"] == 0.0).all()
    steep = math.degrees(math.atan(0.5))
    assert all(p == (0.0 if c == 0 else steep) for p, c in zip(kept["pitch_deg"].tolist(), kept["code"].tolist()))
    assert (kept["surface_m2"] == kept["area_m2"] * np.where(kept["code"] == 0, 1.0, math.sqrt(1.25))).all()
    objects = {"area_cells": np.array([120, 256, 400, 196, 240]), "ground_alt": np.full(5, 10.0)}
    b = RF.roof_table(kept, objects)
    assert b["roof_type"].tolist() == ["flat", "gabled", "hipped", "shed", "flat"] and b["levels"].tolist() == [1, 0, 0, 0, 2]
    # the hipped roof's apex cells (2.25 m) lie on the hip lines, which are no kept facet: its ridge is the kept facets' 2.0 m
    assert b["ridge_height"].tolist() == [0.0, 1.75, 2.0, 3.25, 6.0] and b["eave_height"].tolist() == [0.0] * 5


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(key=DUMMY, ids=DUMMY, h=3, w=4, K=2, radius=1, q=2.0 ** -16, res=0.5, cos0=1.0, sin0=0.0, tan2_flat=0.01, tan2_wall=3.0,
             slope_e=DUMMY, slope_n=DUMMY, code=DUMMY, tag=DUMMY, stats=DUMMY, connectivity=4, parent=DUMMY, fids=DUMMY, root=DUMMY, F=2,
             row0=0, row1=3, rows=DUMMY, planes=DUMMY, unit=64.0, residual=DUMMY)
    a.update(kw)
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


inf, nan = math.inf, math.nan
SIZE_REFUSALS = [
    ({"stats": None}, 3, "null"),
    ({"h": 0}, 1, "h = 0"), ({"w": 0}, 1, "w = 0"), ({"h": -5}, 1, "h = -5"), ({"h": 8193}, 1, "at most 8192"), ({"w": 8193}, 1, "at most 8192"),
    ({"h": 2 ** 31 - 1, "w": 2 ** 31 - 1}, 1, "at most 8192"),
]
NORMALS_REFUSALS = [
    ({"key": None}, 3, "null"), ({"ids": None}, 3, "null"), ({"slope_e": None}, 3, "null"), ({"slope_n": None}, 3, "null"),
    ({"code": None}, 3, "null"), ({"tag": None}, 3, "null"),
    ({"K": -1}, 1, "K = -1"), ({"K": 2 ** 27}, 1, "[0, 2^27)"), ({"K": 2 ** 40}, 1, "[0, 2^27)"),
    ({"radius": 0}, 1, "radius = 0"), ({"radius": 5}, 1, "radius = 5"), ({"radius": -1}, 1, "radius = -1"),
    ({"q": 0.0}, 1, "q > 0"), ({"q": -1.0}, 1, "q > 0"), ({"q": inf}, 1, "q > 0"), ({"q": nan}, 1, "q > 0"),
    ({"res": 0.0}, 1, "res > 0"), ({"res": nan}, 1, "res > 0"), ({"res": inf}, 1, "res > 0"),
    ({"cos0": nan}, 1, "cos0 and sin0 must be finite"), ({"sin0": inf}, 1, "cos0 and sin0 must be finite"),
    ({"tan2_flat": nan}, 1, "tan2_flat"), ({"tan2_flat": -0.1}, 1, "tan2_flat"), ({"tan2_wall": inf}, 1, "tan2_flat"),
    ({"tan2_wall": nan}, 1, "tan2_flat"), ({"tan2_flat": 4.0}, 1, "tan2_flat <= tan2_wall"),
]
LINK_REFUSALS = [
    ({"tag": None}, 3, "null"), ({"parent": None}, 3, "null"), ({"connectivity": 6}, 1, "connectivity = 6"), ({"connectivity": 0}, 1, "connectivity = 0"),
]
BAND_REFUSALS = [
    ({"F": -1}, 1, "F = -1"), ({"F": 2 ** 27}, 1, "[0, 2^27)"), ({"row0": -1}, 1, "row0 = -1"), ({"row1": 4}, 1, "row1 = 4"),
    ({"row0": 2, "row1": 1}, 1, "row0 = 2"),
]
MOMENTS_REFUSALS = [
    ({"fids": None}, 3, "null"), ({"root": None}, 3, "null"), ({"key": None}, 3, "null"), ({"tag": None}, 3, "null"), ({"rows": None}, 3, "null"),
]
RESIDUALS_REFUSALS = [
    ({"fids": None}, 3, "null"), ({"root": None}, 3, "null"), ({"key": None}, 3, "null"), ({"planes": None}, 3, "null"),
    ({"residual": None}, 3, "null"), ({"rows": None}, 3, "null"),
    ({"q": 0.0}, 1, "q > 0"), ({"q": nan}, 1, "q > 0"), ({"unit": 0.0}, 1, "unit > 0"), ({"unit": -64.0}, 1, "unit > 0"),
    ({"unit": inf}, 1, "unit > 0"), ({"unit": nan}, 1, "unit > 0"),
]
CASES = ([("snerf_roofs_normals", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + NORMALS_REFUSALS]
         + [("snerf_roofs_link", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + LINK_REFUSALS]
         + [("snerf_roofs_moments", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + BAND_REFUSALS + MOMENTS_REFUSALS]
         + [("snerf_roofs_residuals", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + BAND_REFUSALS + RESIDUALS_REFUSALS])


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{s[12:]}-{n}" for n, (s, _, _, _) in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **dict(kw))
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_empty_problems_launch_nothing():
    """F == 0 with null rows and planes, and an empty band, are accepted and return before a launch: the dummy addresses are never
    touched"""
    assert _call("snerf_roofs_moments", F=0, rows=None)[0] == 0 and _call("snerf_roofs_moments", row0=2, row1=2)[0] == 0
    assert _call("snerf_roofs_residuals", row0=3, row1=3)[0] == 0 and _call("snerf_roofs_residuals", F=0, rows=None, planes=None, row0=1, row1=1)[0] == 0


def test_python_refuses_host_tensors_and_bad_parameters():
    key, ids = torch.zeros((3, 4), dtype=torch.int32), torch.ones((3, 4), dtype=torch.int32)
    alt = torch.zeros((3, 4))
    planes = torch.zeros((2, 3), dtype=torch.float64)
    grid = D.DsmGrid(0.0, 0.0, 0.5, 4, 3)
    with pytest.raises(ValueError, match="key must be a GPU tensor"):
        RF.normals(key, ids, 1, 0.5)
    with pytest.raises(ValueError, match="tag must be a GPU tensor"):
        RF.link(key)
    with pytest.raises(ValueError, match="fids must be a GPU tensor"):
        RF.facet_rows(ids, 2, key.reshape(-1), key, key)
    with pytest.raises(ValueError, match="fids must be a GPU tensor"):
        RF.residuals(ids, 2, key.reshape(-1), key, planes)
    with pytest.raises(ValueError, match="alt must be a GPU tensor"):
        RF.roofs(alt, ids, 1, grid, {"area_cells": np.zeros(1), "ground_alt": np.zeros(1)})
    import inspect
    from snerf_amd.eval import ortho as EO
    assert list(inspect.signature(EO.export_roofs).parameters) == ["products", "objects_result", "output_dp", "alt_key", "reference", "zone_string",
                                                                   "kwargs"]
    p = inspect.signature(RF.roofs).parameters
    assert [p[k].default for k in ("radius", "flat_deg", "wall_deg", "aspect0_deg", "connectivity", "min_facet_m2")] == [1, 5.0, 60.0, 0.0, 4, 4.0]
