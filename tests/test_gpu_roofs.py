"""The roof planes on the GPU (csrc/roofs.hip through eval/utils/roofs.py and eval/ortho.py export_roofs), bit for
bit against the numpy restatement tests/roofs_numpy.py: the normals at the shapes, radii, hole and id patterns where a tile edge, a
halo or a partial wave can go wrong; facets, moment words and residuals on the same rasters, banded and whole; and a synthetic town whose
facets, pitches, roof types and files are known exactly."""
import functools
import hashlib
import importlib
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import roofs as RF
from snerf_amd.eval.utils import terrain as TR
from snerf_amd.framework.util import img_utils
from tests import roofs_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 0.5
SHAPE_IDS = [f"{h}x{w}" for h, w in N.SHAPES]
FILL = 0x5B


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared references stay read-only


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _filled(shape, dtype, fill=FILL):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.reshape(-1).view(torch.uint8).fill_(fill)
    return t


def _u64(rows):
    """rows of Python ints -> the int64 view of their u64 words, as the device tensors hold them"""
    return N.words(rows).view(np.int64)


@functools.lru_cache(maxsize=None)
def _case(h, w, holes, idp):
    key = N.key_raster(h, w, holes)
    ids, K = N.id_raster(h, w, idp)
    key.setflags(write=False)
    ids.setflags(write=False)
    return key, ids, K


# ---- normals --------------------------------------------------------------------------------------------------------------------------
def _normals_raw(key, ids, K, radius, cos0=1.0, sin0=0.0, tf=N.tan2(5.0), tw=N.tan2(60.0)):
    """the entry itself on outputs pre-filled with a byte pattern: an unwritten word shows"""
    h, w = key.shape
    se, sn = _filled((h, w), torch.float32), _filled((h, w), torch.float32)
    code, tag = _filled((h, w), torch.uint8), _filled((h, w), torch.int32)
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    _lib.call("snerf_roofs_normals", _dev(key), _dev(ids), h, w, K, radius, N.Q, RES, cos0, sin0, tf, tw, se, sn, code, tag, stats)
    return se, sn, code, tag, stats


def _same_normals(got, want, what):
    assert got[4].tolist() == want[4], what
    for k in range(4):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", N.SHAPES, ids=SHAPE_IDS)
def test_normals_are_the_restatements(shape, radius):
    h, w = shape
    normal_cells = 0
    for holes in N.HOLE_PATTERNS:
        for idp in N.ID_PATTERNS:
            key, ids, K = _case(h, w, holes, idp)
            want = N.normals(key, ids, K, radius, N.Q, RES)
            _same_normals(_normals_raw(key, ids, K, radius), want, (holes, idp))
            assert want[4][0] == want[4][1] + want[4][2] + want[4][3]
            normal_cells += want[4][1]
    assert normal_cells > 0 or min(h, w) < 3                    # a single row or column is collinear


def test_normals_under_a_rotated_aspect0_and_through_the_host_layer():
    """the octant bins turned by 30 and by -100 degrees: the gradients stay, the codes move; the host wrapper gives the entry's bits,
    and at K == 0 the constants without a launch"""
    key, ids, K = _case(33, 64, "random", "blobs")
    plain = N.normals(key, ids, K, 2, N.Q, RES)
    moved = 0
    for deg in (30.0, -100.0):
        a0 = math.radians(deg)
        want = N.normals(key, ids, K, 2, N.Q, RES, math.cos(a0), math.sin(a0))
        _same_normals(_normals_raw(key, ids, K, 2, math.cos(a0), math.sin(a0)), want, deg)
        _same_normals(RF.normals(_dev(key), _dev(ids), K, RES, radius=2, aspect0_deg=deg), want, deg)
        assert np.array_equal(_bits(want[0]), _bits(plain[0])) and np.array_equal(_bits(want[1]), _bits(plain[1]))
        moved += int((want[2] != plain[2]).sum())
    assert moved > 0
    # other thresholds: everything with a normal flat, or nothing flat and nothing steep
    for flat_deg, wall_deg in ((89.0, 89.5), (0.0, 89.9)):
        want = N.normals(key, ids, K, 1, N.Q, RES, 1.0, 0.0, N.tan2(flat_deg), N.tan2(wall_deg))
        _same_normals(RF.normals(_dev(key), _dev(ids), K, RES, flat_deg=flat_deg, wall_deg=wall_deg), want, flat_deg)
    se, sn, code, tag, stats = RF.normals(_dev(key), _dev(ids), 0, RES)
    assert bool(torch.isnan(se).all()) and bool(torch.isnan(sn).all()) and bool((code == 255).all()) and bool((tag == -1).all())
    assert stats.tolist() == [0, 0, 0, 0]
    _same_normals((se, sn, code, tag, stats), N.normals(key, ids, 0, 1, N.Q, RES), "K = 0")
    _same_normals(_normals_raw(key, ids, 0, 1), N.normals(key, ids, 0, 1, N.Q, RES), "K = 0 through the entry")


def test_an_integer_plane_comes_back_exactly():
    """keys alpha i + beta j + gamma under holes and ragged ids: every cell with a normal has the slopes alpha q / res and
    -beta q / res to the bit, whatever its support"""
    h, w = 33, 64
    jj, ii = np.mgrid[0:h, 0:w]
    ids, K = N.id_raster(h, w, "blobs")
    for alpha, beta in ((7001, -3999), (0, 12345), (-65536, 1)):
        key = np.where(N.hole_mask("random", h, w), N.HOLE, alpha * ii + beta * jj - 4242).astype(np.int32)
        se, sn, code, tag, stats = RF.normals(_dev(key), _dev(ids), K, RES, radius=3)
        has = code.cpu().numpy() <= 9
        assert has.sum() == stats[1].item() > 1000
        assert (se.cpu().numpy()[has] == np.float32(alpha * N.Q / RES)).all() and (sn.cpu().numpy()[has] == np.float32(-beta * N.Q / RES)).all()


# ---- facets: link, moments, residuals -------------------------------------------------------------------------------------------------
SMALL = {"holes": N.HOLE_PATTERNS, "ids": N.ID_PATTERNS}
LARGE = {"holes": ["none", "hole_row_and_column", "random"], "ids": ["one_object", "checkerboard", "two_rectangles", "blobs"]}


@functools.lru_cache(maxsize=None)
def _chain(h, w, holes, idp, connectivity):
    key, ids, K = _case(h, w, holes, idp)
    return N.roofs(key, ids, K, RES, radius=1, connectivity=connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", N.SHAPES, ids=SHAPE_IDS)
def test_facets_moments_and_residuals_are_the_restatements(shape, connectivity):
    h, w = shape
    patterns = SMALL if h * w <= 2200 else LARGE
    left_out = nan_planes = facets = clamped = 0
    for holes in patterns["holes"]:
        for idp in patterns["ids"]:
            key, ids, K = _case(h, w, holes, idp)
            want = _chain(h, w, holes, idp, connectivity)
            what = (holes, idp)
            d_key, d_tag = _dev(key), _dev(want["tag"])
            parent, lstats = RF.link(d_tag, connectivity)
            assert lstats.tolist() == want["stats"]["link"] and lstats[0].item() == 0, what            # no guard trips
            assert np.array_equal(parent.cpu().numpy(), want["parent"]), what
            fids, F = OB.ids_from_parent(parent, h, w)
            assert F == want["F"] and np.array_equal(fids.cpu().numpy(), want["fids"]), what
            rows, mstats = RF.facet_rows(fids, F, parent, d_key, d_tag)
            assert mstats.tolist() == want["stats"]["moments"], what
            assert np.array_equal(rows.cpu().numpy(), _u64(want["moments"]).reshape(F, 16)), what
            planes = RF.facet_table(rows, D.DsmGrid(0.0, 0.0, RES, w, h))["plane"]
            assert np.array_equal(planes.view(np.uint64), want["planes"].view(np.uint64)), what       # the host solve, too
            out = _filled((h, w), torch.float32)
            residual, rrows, rstats = RF.residuals(fids, F, parent, d_key, _dev(planes), out=out)
            assert rstats.tolist() == want["stats"]["residuals"], what
            assert np.array_equal(_bits(residual), _bits(want["residual"])), what
            assert np.array_equal(rrows.cpu().numpy(), _u64(want["residual_rows"]).reshape(F, 8)), what
            if F and h > 1:
                # the southern band first, then the northern one, into one set of accumulators
                cut = h // 2
                b_rows, b_stats = RF.facet_rows(fids, F, parent, d_key, d_tag, band=(cut, h))
                RF.facet_rows(fids, F, parent, d_key, d_tag, rows=b_rows, stats=b_stats, band=(0, cut))
                assert torch.equal(b_rows, rows) and torch.equal(b_stats, mstats), what
                b_out = _filled((h, w), torch.float32)
                _, c_rows, c_stats = RF.residuals(fids, F, parent, d_key, _dev(planes), band=(cut, h), out=b_out)
                RF.residuals(fids, F, parent, d_key, _dev(planes), rows=c_rows, stats=c_stats, band=(0, cut), out=b_out)
                assert torch.equal(c_rows, rrows) and torch.equal(c_stats, rstats), what
                assert torch.equal(b_out.view(torch.int32), residual.view(torch.int32)), what
            left_out += want["stats"]["moments"][1]
            nan_planes += int(np.isnan(want["planes"][:, 0]).sum())
            clamped += sum(r[6] for r in want["residual_rows"])
            facets += F
    if h * w > 400:
        # the cases hold what they are for: many facets, some of them without a plane (a NaN row of `planes`)
        assert nan_planes > 0 and facets > 100 and left_out == clamped == 0


def test_fids_roots_and_planes_the_chain_never_makes():
    """ids beyond [0, F], roots beyond the raster, a facet whose root is a hole, planes with an infinity: ignored or left out and
    counted, never read out of bounds"""
    h, w = 7, 65
    key, ids, K = _case(h, w, "random", "one_object")
    want = _chain(h, w, "random", "one_object", 4)
    F = want["F"]
    rng = np.random.default_rng(5)
    fids, root = want["fids"].copy(), want["parent"].reshape(h, w).copy()
    fids[rng.random((h, w)) < 0.05] = F + 1
    fids[rng.random((h, w)) < 0.05] = -2
    root[rng.random((h, w)) < 0.05] = h * w
    root[rng.random((h, w)) < 0.05] = -1
    hole_at = np.flatnonzero(~np.vectorize(N.valid)(key.reshape(-1)))[0]
    root[fids == 1] = hole_at
    # the largest facet: cells at and beyond the |dk| bound of 2^24 on both sides, and one just inside it
    big = 1 + int(np.argmax([r[0] for r in want["moments"]]))
    planes = want["planes"].copy()
    planes[[k for k in range(1, F, 3) if k != big - 1], 1] = np.inf
    key = key.copy()
    cells = np.flatnonzero((fids == big).reshape(-1) & (np.arange(h * w) != want["moments"][big - 1][14]))
    assert len(cells) >= 8 and np.isfinite(planes[big - 1]).all() and big != 1
    k0 = int(key.reshape(-1)[want["moments"][big - 1][14]])
    for c, dk in zip(cells[:5], (2 ** 24, -2 ** 24, 2 ** 24 - 1, 2 ** 25 + 12345, -2 ** 26)):
        key.reshape(-1)[c] = k0 + dk
    m_rows, m_stats = N.moments(fids, root, key, want["tag"], F)
    residual, r_rows, r_stats = N.residuals(fids, root, key, F, planes)
    assert m_stats[2] > 0 and m_stats[1] > 0 and r_stats[1] > 0 and r_stats[2] == m_stats[2]
    assert m_rows[big - 1][15] >= 4 and r_rows[big - 1][6] >= 2 and r_rows[big - 1][3] == 2 ** 18       # a residual is clamped by its own size, not by dk's
    rows, mstats = RF.facet_rows(_dev(fids), F, _dev(root), _dev(key), _dev(want["tag"]))
    assert mstats.tolist() == m_stats and np.array_equal(rows.cpu().numpy(), _u64(m_rows).reshape(F, 16))
    got, rrows, rstats = RF.residuals(_dev(fids), F, _dev(root), _dev(key), _dev(planes), out=_filled((h, w), torch.float32))
    assert rstats.tolist() == r_stats and np.array_equal(_bits(got), _bits(residual))
    assert np.array_equal(rrows.cpu().numpy(), _u64(r_rows).reshape(F, 8))
    # F == 0: nothing is launched, the residual plane is NaN
    got, rrows, rstats = RF.residuals(_dev(np.zeros((h, w), np.int32)), 0, _dev(root), _dev(key), torch.zeros((0, 3), dtype=torch.float64, device=DEV))
    assert bool(torch.isnan(got).all()) and tuple(rrows.shape) == (0, 8) and rstats.tolist() == [0, 0, 0]


# ---- the town -------------------------------------------------------------------------------------------------------------------------
GRID = D.DsmGrid(500000.0, 4100000.0, N.TOWN_RES, N.TOWN_SHAPE[1], N.TOWN_SHAPE[0])
TOWN_FACETS = [(1, 0, 120), (2, 7, 128), (2, 3, 128), (3, 1, 90), (5, 0, 100), (5, 0, 100), (3, 7, 90), (3, 3, 90), (4, 1, 196), (3, 5, 90)]


def _town_objects(alt, ids):
    """what objects() returns, for the town's own numbering of its five buildings (raster order would swap the last two): the words
    and the table of its id plane"""
    label = np.where(ids > 0, 3, 0).astype(np.uint8)
    d_ids = _dev(ids)
    rows, stats = OB.object_rows(d_ids, 5, _dev(label), _dev(alt), ground=(0,))
    table = OB.object_table(rows, GRID)
    assert table["area_cells"].tolist() == [120, 256, 400, 196, 240] and table["ground_alt"].tolist() == [10.0] * 5
    return {"ids": d_ids, "n": 5, "table": table, "stats": [int(v) for v in stats.cpu()]}


def _check_town(res):
    key, ids, K, alt = N.town()
    want = N.roofs(key, ids, K, N.TOWN_RES)
    t = res["facets"]
    assert res["n_facets"] == 10 and list(zip(t["object"].tolist(), t["code"].tolist(), t["area_cells"].tolist())) == TOWN_FACETS
    assert res["stats"] == {"object_cells": 1212, "normals": 1212, "degenerate": 0, "holes": 0, "facet_cells": 1172, "facets_found": 50,
                            "folded": 1172, "left_out": 0, "residual_cells": 1132, "without_residual": 40}
    for k in ("slope_e", "slope_n"):
        assert np.array_equal(_bits(res[k]), _bits(want[k])), k
    assert np.array_equal(res["code"].cpu().numpy(), want["code"])
    # the kept facets are the restatement's ten facets of 16 cells or more, renumbered in order
    big = np.array([0] + [1 if r[0] >= 16 else 0 for r in want["moments"]])
    lut = np.where(big > 0, np.cumsum(big), 0)
    assert np.array_equal(res["facet_ids"].cpu().numpy(), lut[want["fids"]])
    # exactly planar: every residual word and every residual 0; every pitch 0 or atan(1/2)
    assert (t["rms_m"] == 0.0).all() and (t["max_abs_m"] == 0.0).all() and (t["mean_abs_m"] == 0.0).all() and (t["clamped"] == 0).all()
    residual = res["residual"].cpu().numpy()
    kept = res["facet_ids"].cpu().numpy() > 0
    assert (residual[kept] == 0.0).all() and np.isnan(residual[~kept]).all() and kept.sum() == 1132
    steep = math.degrees(math.atan(0.5))
    assert all(p == (0.0 if c == 0 else steep) for p, c in zip(t["pitch_deg"].tolist(), t["code"].tolist()))
    assert [a for a in t["azimuth_deg"].tolist() if not math.isnan(a)] == [270.0, 90.0, 0.0, 270.0, 90.0, 0.0, 180.0]
    assert t["eave_alt"].tolist() == [10.0, 10.0, 10.0, 10.0, 10.0, 16.0, 10.0, 10.0, 10.0, 10.0]
    assert t["ridge_alt"][1] == 10.0 + 7 * 0.25 and t["ridge_alt"][8] == 10.0 + 13 * 0.25
    b = res["buildings"]
    assert b["roof_type"].tolist() == ["flat", "gabled", "hipped", "shed", "flat"] and b["levels"].tolist() == [1, 0, 0, 0, 2]
    assert b["facets"].tolist() == [1, 2, 4, 1, 2] and b["rms_m"].tolist() == [0.0] * 5
    assert b["pitched_share"].tolist() == [0.0, 1.0, 1.0, 1.0, 0.0] and b["pitch_deg"].tolist() == [0.0, steep, steep, steep, 0.0]
    assert b["eave_height"].tolist() == [0.0] * 5 and b["ridge_height"].tolist() == [0.0, 1.75, 2.0, 3.25, 6.0]


def test_the_town_end_to_end():
    key, ids, K, alt = N.town()
    assert np.array_equal(TR.keys(_dev(alt))[0].cpu().numpy(), key)
    objects = _town_objects(alt, ids)
    res = RF.roofs(_dev(alt), objects["ids"], objects["n"], GRID, objects["table"])
    _check_town(res)
    assert res["parameters"] == {"radius": 1, "flat_deg": 5.0, "wall_deg": 60.0, "aspect0_deg": 0.0, "connectivity": 4, "min_facet_m2": 4.0}
    again = RF.roofs(_dev(alt), objects["ids"], objects["n"], GRID, objects["table"])
    assert all(torch.equal(_dev(_bits(again[k])), _dev(_bits(res[k]))) for k in ("slope_e", "slope_n", "code", "facet_ids", "residual", "pitch_deg"))
    # with every facet kept: the 40 single cells on the hip lines, which have no plane, are dropped all the same
    every = RF.roofs(_dev(alt), objects["ids"], objects["n"], GRID, objects["table"], min_facet_m2=0.0)
    assert every["n_facets"] == 10 and every["stats"]["facets_found"] == 50


def test_export_roofs_on_the_town(tmp_path):
    key, ids, K, alt = N.town()
    objects = _town_objects(alt, ids)
    products = {"dsm": _dev(alt), "grid": GRID}
    out = EO.export_roofs(products, objects, str(tmp_path), reference={"alt": _dev(alt), "objects": objects}, zone_string="17R")
    names = {"pitch.tif", "pitch.png", "aspect.png", "facets.tif", "residual.tif", "residual.png", "roofs.json", "roofs_eval.json"}
    assert set(out["files"]) == names and all(os.path.isfile(p) and os.path.getsize(p) > 0 for p in out["files"].values())
    assert os.path.dirname(out["files"]["pitch.tif"]) == os.path.join(str(tmp_path), "roofs")
    _check_town(out)
    _check_town(out["reference"])
    facets, transform = img_utils.load_dsm_geotiff(out["files"]["facets.tif"])
    assert facets.dtype == np.int32 and np.array_equal(facets, out["facet_ids"].cpu().numpy()) and transform == (GRID.xoff, GRID.yoff, 0.5, 0.5)
    pitch, _ = img_utils.load_dsm_geotiff(out["files"]["pitch.tif"])
    assert pitch.dtype == np.float32 and np.array_equal(pitch.view(np.uint32), _bits(out["pitch_deg"]))
    residual, _ = img_utils.load_dsm_geotiff(out["files"]["residual.tif"])
    assert np.array_equal(residual.view(np.uint32), _bits(out["residual"]))
    doc = json.load(open(out["files"]["roofs.json"]))
    assert doc["stats"] == out["stats"] and doc["parameters"] == dict({"alt_key": "dsm"}, **out["parameters"])
    assert [f["area_cells"] for f in doc["facets"]] == [n for _, _, n in TOWN_FACETS] and len(doc["buildings"]) == 5
    assert [b["roof_type"] for b in doc["buildings"]] == ["flat", "gabled", "hipped", "shed", "flat"]
    ev = json.load(open(out["files"]["roofs_eval.json"]))
    assert ev == json.loads(json.dumps(out["eval"]))
    assert ev["pairs"] == 5 and ev["type_agreement"] == 1.0 and ev["pitch_mae_deg"] == 0.0
    assert all(p["type_a"] == p["type_b"] and p["pitch_error_deg"] == 0.0 and p["azimuth_agrees"] in (True, None) for p in ev["per_pair"])
    assert sorted(ev["types"]) == ["flat", "gabled", "hipped", "shed"] and sum(map(sum, ev["type_table"])) == 5
    assert ev["normal_cells"] == 1212 and ev["normal_angle_mean_deg"] == 0.0 and ev["normal_angle_median_deg"] == 0.0
    with pytest.raises(ValueError, match=r"\(48, 64\).*\(48, 63\)"):
        EO.export_roofs(products, objects, str(tmp_path), reference={"alt": _dev(alt[:, :-1]), "objects": objects})


# ---- isolation ------------------------------------------------------------------------------------------------------------------------
def _digests(files):
    return {name: hashlib.sha256(open(p, "rb").read()).hexdigest() for name, p in sorted(files.items())}


def test_the_other_map_exports_do_not_know_the_roofs(tmp_path, monkeypatch):
    """export_objects and export_terrain write the same bytes without the roofs module and after it was imported and used, and call no
    roofs entry"""
    key, ids, K, alt = N.town()
    label = np.where(ids > 0, 3, 0).astype(np.uint8)
    products = {"dsm": _dev(alt), "label": _dev(label), "grid": GRID}
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (called.append(name), real(name, *a, **kw))[1])

    def exports(sub):
        o = EO.export_objects(products, str(tmp_path / sub), zone_string="17R")
        t = EO.export_terrain(products, str(tmp_path / sub), zone_string="17R", max_window_m=12.5, slope=0.3)
        return _digests(o["files"]), _digests(t["files"])

    name = RF.__name__
    package = sys.modules[name.rpartition(".")[0]]
    monkeypatch.delitem(sys.modules, name)
    monkeypatch.delattr(package, "roofs")
    before = exports("before")
    assert name not in sys.modules and called and not [c for c in called if c.startswith("snerf_roofs")]
    fresh = importlib.import_module(name)
    objects = _town_objects(alt, ids)
    assert fresh.roofs(_dev(alt), objects["ids"], objects["n"], GRID, objects["table"])["n_facets"] == 10
    assert [c for c in called if c.startswith("snerf_roofs")] == ["snerf_roofs_normals", "snerf_roofs_link", "snerf_roofs_moments",
                                                                  "snerf_roofs_residuals"]
    del called[:]
    after = exports("after")
    assert after == before and len(before[0]) == 5 and len(before[1]) == 7
    assert called and not [c for c in called if c.startswith("snerf_roofs")]
