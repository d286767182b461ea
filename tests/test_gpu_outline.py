"""The outlines on the GPU (csrc/outline.hip through eval/utils/outline.py and eval/ortho.py export_objects / export_roofs; DESIGN.md
section 5ze), bit for bit against the numpy restatement tests/outline_numpy.py: every entry and rings() at both connectivities on the
random shapes, on the structured rasters where a ring is as long as the raster, and on the hand-made ones; what the guards leave
unwritten; a successor map that is no permutation; and the two GeoJSON exports on the synthetic town."""
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import outline as OL       # the feature under test: every test of this file needs it
from tests import objects_numpy as ON
from tests import outline_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
GRID = D.DsmGrid(500000.0, 4100000.0, 0.5, 130, 96)
RASTERS = list(N.labels())


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared references stay read-only


def _filled(*shape, dtype=torch.int32):
    return torch.full(shape, SENTINEL if dtype == torch.int32 else 0x5A, dtype=dtype, device=DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _rows(t):
    return t.cpu().numpy().view(np.uint64)


# ---- entry by entry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTERS)
def test_every_entry_is_the_restatements(name, connectivity):
    """sides, the offsets, link, rank_rings, the rows between, emit: every output buffer starts from a sentinel and ends as the
    restatement's array -- exactly the specified words are written -- and every guard word is 0"""
    ids_np, K = N.ids_of(name, connectivity)
    want = N.trace_of(name, connectivity)
    E, V, R = want["E"], want["V"], want["n_rings"]
    h, w = ids_np.shape
    ids = _dev(ids_np)
    buf = _filled(h * w, dtype=torch.uint8)
    side_bits, stats = OL.sides(ids, K, out=buf)
    assert side_bits is buf and stats.tolist() == want["sides_stats"]
    _same(side_bits, want["sides"], "sides")
    offsets, got_E = OL.offsets_of(side_bits)
    assert got_E == E
    _same(offsets, want["offsets"], "offsets")
    slot, nxt, flags, stats = OL.link(ids, side_bits, offsets, K, connectivity, E, out=(_filled(E), _filled(E), _filled(E)))
    assert stats.tolist() == [0, E]
    for got, key in ((slot, "slot"), (nxt, "next"), (flags, "flags")):
        _same(got, want[key], key)
    ring, rank, ordinal, totals, stats = OL.rank_rings(nxt, flags, out=(_filled(E), _filled(E), _filled(E), _filled(E, 2)))
    assert stats.tolist() == [0, E]
    for got, key in ((ring, "ring"), (rank, "rank"), (ordinal, "ordinal"), (totals, "totals")):
        _same(got, want[key], key)
    ring_row, vertex_offset, n_rings, got_V = OL.ring_rows(ring, totals)
    assert (n_rings, got_V) == (R, V)
    _same(ring_row, want["ring_row"], "ring_row")
    _same(vertex_offset, want["vertex_offset"], "vertex_offset")
    vertices, rows, stats = OL.emit(ids, slot, flags, ring, ordinal, ring_row, vertex_offset, R, V, vertices=_filled(V, 2))
    assert stats.tolist() == [0, V]
    _same(vertices, want["vertices"], "vertices")
    assert np.array_equal(_rows(rows), want["rows"])
    if E == 0:
        assert all(t.numel() == 0 for t in (slot, nxt, flags, ring, rank, ordinal, totals, vertices, rows))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTERS)
def test_rings_is_the_restatements_twice(name, connectivity):
    ids_np, K = N.ids_of(name, connectivity)
    t = N.trace_of(name, connectivity)
    want = N.rings_of(t)
    ids = _dev(ids_np)
    first, second = OL.rings(ids, K, connectivity), OL.rings(ids, K, connectivity)
    for key in ("vertices", "ring_start", "ring_object", "ring_area2", "ring_edges", "ring_bbox"):
        assert first[key].dtype == want[key].dtype and np.array_equal(first[key], want[key]), key
        assert np.array_equal(first[key], second[key]), key
    s = t["sides_stats"]
    assert first["stats"] == second["stats"] == {"bad_ids": 0, "object_cells": s[1], "edges": t["E"], "corners": t["V"], "rings": t["n_rings"]}
    assert list(OL.polygons(first)) == list(range(1, K + 1))


def test_ids_beyond_k_are_counted_and_left_out():
    ids_np = np.array(N.ids_of("random_7x65", 4)[0])
    K = N.ids_of("random_7x65", 4)[1]
    ids_np[2, 5], ids_np[6, 64] = -7, K + 1
    want = N.trace(ids_np, K, 4)
    got = OL.rings(_dev(ids_np), K, 4)
    assert got["stats"]["bad_ids"] == want["sides_stats"][0] == 2 and np.array_equal(got["vertices"], want["vertices"])
    assert np.array_equal(got["ring_area2"], N.rings_of(want)["ring_area2"])


def test_buffers_of_the_caller_are_checked_before_any_launch():
    """a buffer that is too short, of another type or not contiguous never reaches an entry"""
    ids_np, K = N.ids_of("random_7x65", 4)
    t = N.trace_of("random_7x65", 4)
    E = t["E"]
    ids, side_bits, offsets = _dev(ids_np), _dev(t["sides"]), _dev(t["offsets"])
    with pytest.raises(ValueError, match=f"next must hold {E} contiguous"):
        OL.link(ids, side_bits, offsets, K, 4, E, out=(_filled(E), _filled(E - 1), _filled(E)))
    with pytest.raises(ValueError, match=f"flags must hold {E} contiguous"):
        OL.link(ids, side_bits, offsets, K, 4, E, out=(_filled(E), _filled(E), _filled(E).long()))
    with pytest.raises(ValueError, match="E = -1 is negative"):
        OL.link(ids, side_bits, offsets, K, 4, -1)
    nxt, flags = _dev(t["next"]), _dev(t["flags"])
    with pytest.raises(ValueError, match=f"totals must hold {2 * E} contiguous"):
        OL.rank_rings(nxt, flags, out=(_filled(E), _filled(E), _filled(E), _filled(E)))
    with pytest.raises(ValueError, match=f"rank must hold {E} contiguous"):
        OL.rank_rings(nxt, flags, out=(_filled(E), _filled(2 * E)[::2], _filled(E), _filled(E, 2)))
    with pytest.raises(ValueError, match="4-byte aligned GPU tensor of at least"):
        OL.rank_rings(nxt, flags, workspace=torch.empty(24 * E + 1, dtype=torch.uint8, device=DEV)[1:])
    with pytest.raises(ValueError, match="4-byte aligned GPU tensor of at least"):
        OL.rank_rings(nxt, flags, workspace=torch.empty(24 * E - 4, dtype=torch.uint8, device=DEV))


# ---- the guards: counted, and nothing lands out of place ----------------------------------------------------------------------------------
def test_link_with_offsets_of_other_sides():
    """offsets that run 5 ahead from the raster's middle on, and an E two short: the edges whose own or whose successor's index leaves
    [0, E) are counted and not written -- their words keep the sentinel -- and everything else is as the restatement has it"""
    ids_np, K = N.ids_of("random_33x64", 8)
    t = N.trace_of("random_33x64", 8)
    offsets = t["offsets"].copy()
    offsets[len(offsets) // 2:] += 5
    E = t["E"] - 2
    want = N.link(ids_np, t["sides"], offsets, K, 8, E, fill=SENTINEL)
    assert want[3][0] > 0 and want[3][0] + want[3][1] == t["E"] and (want[0] == SENTINEL).any()
    got = OL.link(_dev(ids_np), _dev(t["sides"]), _dev(offsets), K, 8, E, out=(_filled(E), _filled(E), _filled(E)))
    assert got[3].tolist() == want[3]
    for g, wnt, key in zip(got[:3], want[:3], ("slot", "next", "flags")):
        _same(g, wnt, key)


def test_emit_with_too_few_vertices_and_rows():
    """V three short, one ring row out of range and one vertex offset next to 2^63 (tested before anything is added to it): counted, and
    the words beyond stay unwritten"""
    ids_np, K = N.ids_of("random_33x64", 4)
    t = N.trace_of("random_33x64", 4)
    V, R = t["V"] - 3, t["n_rings"]
    ring_row = t["ring_row"].copy()
    ring_row[np.flatnonzero(ring_row == 7)] = R                      # ring 7 points past the rows
    vertex_offset = t["vertex_offset"].copy()
    vertex_offset[11] = 2 ** 63 - 2
    want = N.emit(ids_np, t["slot"], t["flags"], t["ring"], t["ordinal"], ring_row, vertex_offset, R, V, fill=SENTINEL)
    assert want[2][0] > 3 and (want[0] == SENTINEL).any() and want[1][7].tolist() == N.ROW_INIT
    got = OL.emit(_dev(ids_np), *(_dev(t[k]) for k in ("slot", "flags", "ring", "ordinal")), _dev(ring_row), _dev(vertex_offset), R, V,
                  vertices=_filled(V, 2))
    assert got[2].tolist() == want[2]
    _same(got[0], want[0], "vertices")
    assert np.array_equal(_rows(got[1]), want[1])


def test_a_successor_map_that_is_no_permutation(monkeypatch):
    """two edges that share a successor and an index equal to E: the rounds are fixed, an index out of range is read as the edge's own
    and never dereferenced, the entry returns with a guard word that is not 0 -- a counted refusal -- and its words are the
    restatement's all the same; rings() raises"""
    t = N.trace_of("random_7x65", 8)
    E = t["E"]
    nxt = t["next"].copy()
    nxt[10] = nxt[11]
    nxt[E - 1] = E
    want = N.rank(nxt, t["flags"])
    assert want[4][0] > 0
    got = OL.rank_rings(_dev(nxt), _dev(t["flags"]), out=(_filled(E), _filled(E), _filled(E), _filled(E, 2)))
    assert got[4].tolist() == want[4] and got[4][0] > 0
    for g, wnt, key in zip(got[:4], want[:4], ("ring", "rank", "ordinal", "totals")):
        _same(g, wnt, key)
    real = OL.link

    def broken(*args, **kw):
        slot, linked, flags, stats = real(*args, **kw)
        linked[10] = linked[11]
        return slot, linked, flags, stats

    monkeypatch.setattr(OL, "link", broken)
    ids_np, K = N.ids_of("random_7x65", 8)
    with pytest.raises(RuntimeError, match="no permutation"):
        OL.rings(_dev(ids_np), K, 8)


# ---- the exports ------------------------------------------------------------------------------------------------------------------------------
def _shoelace(ring):
    a = np.asarray(ring, np.float64)
    x, y = a[:, 0] - a[0, 0], a[:, 1] - a[0, 1]
    return 0.5 * float((x[:-1] * y[1:] - x[1:] * y[:-1]).sum())


def _check_features(fp, n, records):
    doc = json.load(open(fp))
    assert doc["type"] == "FeatureCollection" and doc["crs"]["properties"]["name"] == "urn:ogc:def:crs:EPSG::32617"
    assert len(doc["features"]) == n == len(records) and n >= 3
    for f, rec in zip(doc["features"], json.loads(json.dumps(records))):
        rings = f["geometry"]["coordinates"]
        assert f["properties"] == rec and f["id"] == rec["id"] and all(r[0] == r[-1] for r in rings)
        assert _shoelace(rings[0]) > 0 and sum(_shoelace(r) for r in rings) == rec["area_m2"], rec["id"]
    return doc


def test_export_objects_with_polygons_on_the_town(tmp_path):
    label, alt, boxes = ON.town()
    products = {"label": _dev(label), "dsm": _dev(alt), "grid": GRID}
    plain = EO.export_objects(products, str(tmp_path / "plain"), classes=(3, 4), zone_string="17R")
    names = {"objects.json", "objects_ids.tif", "objects_ids.png", "objects_height.tif", "objects_height.png"}
    assert set(plain["files"]) == names == set(os.listdir(tmp_path / "plain" / "objects")) and "footprints" not in plain
    out = EO.export_objects(products, str(tmp_path / "poly"), classes=(3, 4), zone_string="17R", polygons=True)
    assert set(out["files"]) == names | {"footprints.geojson"} == set(os.listdir(tmp_path / "poly" / "objects"))
    for name in names:
        assert open(out["files"][name], "rb").read() == open(plain["files"][name], "rb").read(), name
    doc = _check_features(out["files"]["footprints.geojson"], out["n"], OB.table_records(out["table"]))
    assert out["n"] == 4 and out["outline_stats"] == {"bad_ids": 0, "object_cells": 120 + 153 + 720 + 4, "edges": 44 + 52 + 108 + 8,
                                                      "corners": 16, "rings": 4}
    j0, i0, nj, ni, _ = boxes[0]
    e0, n1 = GRID.xoff + 0.5 * i0, GRID.yoff - 0.5 * j0
    assert doc["features"][0]["geometry"]["coordinates"] == [[[e0, n1], [e0, n1 - 0.5 * nj], [e0 + 0.5 * ni, n1 - 0.5 * nj], [e0 + 0.5 * ni, n1],
                                                              [e0, n1]]]
    # rectangles have nothing to lose below half their short side; the 2 x 2 blob keeps its 4 corners at any tolerance
    simple = EO.export_objects(products, str(tmp_path / "simple"), classes=(3, 4), zone_string="17R", polygons=True, simplify_m=0.45)
    assert simple["footprints"] == out["footprints"]


def test_export_roofs_with_polygons_on_the_town(tmp_path):
    label, alt, _ = ON.town()
    objects = OB.objects(_dev(label), _dev(alt), GRID, classes=(3, 4), ground=(0,))
    products = {"dsm": _dev(alt), "grid": GRID}
    plain = EO.export_roofs(products, objects, str(tmp_path / "plain"), zone_string="17R")
    names = {"pitch.tif", "pitch.png", "aspect.png", "facets.tif", "residual.tif", "residual.png", "roofs.json"}
    assert set(plain["files"]) == names == set(os.listdir(tmp_path / "plain" / "roofs")) and "footprints" not in plain
    out = EO.export_roofs(products, objects, str(tmp_path / "poly"), zone_string="17R", polygons=True)
    assert set(out["files"]) == names | {"facets.geojson"} == set(os.listdir(tmp_path / "poly" / "roofs"))
    for name in names:
        assert open(out["files"][name], "rb").read() == open(plain["files"][name], "rb").read(), name
    from snerf_amd.eval.utils import roofs as RF
    _check_features(out["files"]["facets.geojson"], out["n_facets"], RF.table_records(out["facets"]))
    assert out["outline_stats"]["rings"] >= out["n_facets"] and out["outline_stats"]["bad_ids"] == 0
