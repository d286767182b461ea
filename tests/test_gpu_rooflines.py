"""Roof lines on the GPU (csrc/rooflines.hip through eval/utils/roofs.py grow, eval/utils/arcs.py and eval/ortho.py export_roofs;
DESIGN.md section 5zf), bit for bit against the numpy restatement tests/rooflines_numpy.py: every arc entry into poison-filled buffers
on the rasters of the restatement (among them 2 x 130, whose shared arc crosses two wave boundaries, 1 x 1, an all-zero raster and the
bullseye, whose rings have no node), the growth on the town, on a strip that takes several batches and with max_rq = 0 on noisy keys,
what the guards leave unwritten, and the export on the town end to end."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import arcs as AR          # the feature under test: every test of this file needs it
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import outline as OL
from snerf_amd.eval.utils import roofs as RF
from tests import roofs_numpy as RN
from tests import rooflines_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
RASTERS = list(N.rasters())


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared references stay read-only


def _filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


def _outline(ids, K, connectivity):
    side_bits, _ = OL.sides(ids, K)
    offsets, E = OL.offsets_of(side_bits)
    slot, nxt, flags, _ = OL.link(ids, side_bits, offsets, K, connectivity, E)
    ring, rank, _, totals, _ = OL.rank_rings(nxt, flags)
    return side_bits, offsets, E, slot, flags, ring, rank, totals


# ---- the arcs, entry by entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RASTERS)
def test_every_arc_entry_is_the_restatements(name):
    """first, the ring bases, mark, the sums between, fold: every output buffer starts from a sentinel and ends as the restatement's
    array -- exactly the specified words are written -- and every guard word is 0"""
    ids_np, K, connectivity = N.rasters()[name]
    want = N.trace_of(name)
    E, A, V = want["E"], want["A"], want["V"]
    ids, key = _dev(ids_np), _dev(N.key_of(name))
    side_bits, offsets, got_E, slot, flags, ring, rank, totals = _outline(ids, K, connectivity)
    assert got_E == E
    node, first_word, stats = AR.first(ids, K, slot, ring, rank, out=_filled(E))
    assert stats.tolist() == want["first_stats"]
    _same(node, want["node"], "node")
    _same(first_word, want["first"], "first")
    ring_row, ring_base, n_rings = AR.ring_base_of(ring, totals)
    assert n_rings == want["n_rings"]
    _same(ring_row, want["ring_row"], "ring_row")
    _same(ring_base, want["ring_base"], "ring_base")
    got = AR.mark(ids, K, side_bits, offsets, slot, flags, ring, rank, totals, node, first_word, ring_row, ring_base,
                  out=tuple(_filled(E) for _ in range(6)))
    assert got[6].tolist() == want["mark_stats"] and want["mark_stats"][:2] == [0, E]
    for g, k in zip(got[:6], ("left", "twin", "pos_of", "order", "hf", "vf")):
        _same(g, want[k], k)
    left, twin, pos_of, order, hf, vf = got[:6]
    arc_of, ordinal, last, vertex_offset, got_A, got_V = AR.between(order, hf, vf, node)
    assert (got_A, got_V) == (A, V)
    for g, k in ((arc_of, "arc_of"), (ordinal, "ordinal"), (last, "last"), (vertex_offset, "vertex_offset")):
        _same(g, want[k], k)
    vertices, rows, stats = AR.fold(ids, key, slot, ring, left, twin, pos_of, node, ring_row, order, hf, vf, arc_of, ordinal, last,
                                    vertex_offset, A, V, n_rings, vertices=_filled(V, 2))
    assert stats.tolist() == want["fold_stats"] == [0, V]
    _same(vertices, want["vertices"], "vertices")
    assert np.array_equal(rows.cpu().numpy().view(np.uint64), want["rows"])
    if E == 0:
        assert A == 0 and all(t.numel() == 0 for t in (node, left, order, arc_of, vertices, rows))


def test_the_shared_arc_of_two_rows_crosses_two_waves():
    """2 x 130: the arc between the rows has 130 edges on consecutive positions, so a wave holds its fold over a boundary; without a key
    plane the key words stay 0"""
    ids_np, K, _ = N.rasters()["two_rows_2x130"]
    got = AR.arcs(_dev(ids_np), K)
    want = N.arcs_of(N.trace(ids_np, K, 4))
    assert sorted(got["edges"].tolist()) == [130, 130, 132, 132] and got["stats"]["arcs"] == 4
    for k in ("arc_start", "vertices", "right", "left", "edges", "twin", "closed", "owner", "key_edges", "key_sum_right", "key_sum_left"):
        assert np.array_equal(got[k], want[k]), k
    assert not got["key_edges"].any() and not got["key_sum_left"].any()


@pytest.mark.parametrize("name", ["blobs_37x53", "bullseye-4", "checkerboard_5x7", "random_33x64-8", "one_cell", "all_zero"])
def test_arcs_is_the_restatements(name):
    ids_np, K, connectivity = N.rasters()[name]
    t = N.trace_of(name)
    want = N.arcs_of(t)
    got = AR.arcs(_dev(ids_np), K, connectivity, key=_dev(N.key_of(name)))
    for k in ("arc_start", "vertices", "right", "left", "edges", "twin", "closed", "owner", "key_edges", "key_sum_right", "key_sum_left",
              "arc_ring", "ring_first", "ring_edges"):
        assert np.array_equal(got[k], want[k]), k
    assert len(got["ring_arcs"]) == len(want["ring_arcs"]) and all(np.array_equal(a, b) for a, b in zip(got["ring_arcs"], want["ring_arcs"]))
    for k in ("vertices", "ring_start", "ring_object", "ring_area2", "ring_edges"):
        assert np.array_equal(got["rings"][k], want["rings"][k]), k
    assert got["stats"] == {"edges": t["E"], "arcs": t["A"], "vertices": t["V"], "rings": t["n_rings"], "breaks": t["mark_stats"][2],
                            "twin_edges": t["mark_stats"][3]}


def test_fold_into_too_few_rows_and_vertices():
    """A two short and V three short, with the vertex offsets of the full problem: the positions of the missing arcs, the twins that
    point into them and the vertices beyond V are counted, and nothing lands out of place"""
    name = "blobs_37x53"
    ids_np, K, connectivity = N.rasters()[name]
    t = N.trace_of(name)
    o = t["outline"]
    A, V = t["A"] - 2, t["V"] - 3
    args = (o["slot"], o["ring"], t["left"], t["twin"], t["pos_of"], t["node"], t["ring_row"], t["order"], t["hf"], t["vf"], t["arc_of"],
            t["ordinal"], t["last"], t["vertex_offset"][:A])
    want = N.fold(ids_np, N.key_of(name), *args, A, V, t["n_rings"], fill=SENTINEL)
    assert want[2][0] > 3 and (want[0] == SENTINEL).any()
    got = AR.fold(_dev(ids_np), _dev(N.key_of(name)), *(_dev(a) for a in args), A, V, t["n_rings"], vertices=_filled(V, 2))
    assert got[2].tolist() == want[2]
    _same(got[0], want[0], "vertices")
    assert np.array_equal(got[1].cpu().numpy().view(np.uint64), want[1])


# ---- the growth ---------------------------------------------------------------------------------------------------------------------------
def _grow_entry(fids, ids, key, root, planes, F, unit, max_rq, rounds):
    h, w = fids.shape
    a, b = _filled(h, w), _filled(h, w)
    stats = torch.zeros(rounds + 1, dtype=torch.int64, device=DEV)
    _lib.call("snerf_roofs_grow", _dev(fids), _dev(ids), _dev(key), _dev(np.asarray(root, np.int32)), _dev(np.asarray(planes, np.float64)), h, w, F,
              unit, max_rq, rounds, a, b, stats)
    return (a if rounds & 1 else b), (b if rounds & 1 else a), stats.tolist()


def test_grow_on_the_town():
    t = N.town()
    assert t["rounds"] == 1 and t["counts"][:2] == [80, 0] and int(((t["grown"] == 0) & (t["ids"] > 0)).sum()) == 0
    grown, gained, rounds = RF.grow(_dev(t["fids"]), _dev(t["ids"]), _dev(t["key"]), t["table"])
    _same(grown, t["grown"], "grown")
    assert rounds == 1 and int(gained.sum()) == 80
    assert np.array_equal(gained, np.bincount(t["grown"].reshape(-1), minlength=11)[1:] - np.bincount(t["fids"].reshape(-1), minlength=11)[1:])
    # the entry itself, one round and two: every word of the result buffer is written
    for rounds in (1, 2):
        want, stats = N.grow_rounds(t["fids"], t["ids"], t["key"], t["root"], t["planes"], t["F"], RN.UNIT, 256, rounds)
        result, _, got = _grow_entry(t["fids"], t["ids"], t["key"], t["root"], t["planes"], t["F"], RN.UNIT, 256, rounds)
        assert got == stats and got[:rounds] == [80, 0][:rounds]
        _same(result, want, "grown")


def _strip():
    """9 x 70, one building on one exact plane, its facet on the first 8 columns only: the facet must spread 62 columns"""
    jj, ii = np.mgrid[0:9, 0:70]
    key = (655360 + 100 * ii + 50 * jj).astype(np.int32)
    ids = np.ones((9, 70), np.int32)
    fids = np.zeros((9, 70), np.int32)
    fids[:, :8] = 1
    table = {"object": np.array([1]), "plane": np.array([[0.0, 100.0, 50.0]]), "root": np.array([0])}
    return key, ids, fids, table


def test_grow_over_several_batches():
    key, ids, fids, table = _strip()
    want, used, counts = N.grow(fids, ids, key, table["root"], table["plane"], 1)
    assert used == 62 and counts[:62] == [9] * 62 and len(counts) == 64 and (want == 1).all()
    grown, gained, rounds = RF.grow(_dev(fids), _dev(ids), _dev(key), table)
    _same(grown, want, "grown")
    assert rounds == 62 and gained.tolist() == [9 * 62]
    short, _, rounds = RF.grow(_dev(fids), _dev(ids), _dev(key), table, max_rounds=11)
    _same(short, N.grow(fids, ids, key, table["root"], table["plane"], 1, max_rounds=11)[0], "grown in 11 rounds")
    assert rounds == 11 and int((short == 1).sum()) == 9 * 19


def test_grow_with_no_misfit_allowed_on_noisy_keys():
    """max_rq = 0: a cell joins only where its key lies within half a step of the plane, so only some cells are assigned and the
    growth stops at them; holes are never takers"""
    key, ids, fids, table = _strip()
    rng = np.random.default_rng(7)
    noisy = (key + rng.integers(-80, 81, key.shape)).astype(np.int32)
    noisy[:, :8] = key[:, :8]
    noisy[4, 30] = RN.HOLE
    want, used, counts = N.grow(fids, ids, noisy, table["root"], table["plane"], 1, max_rq=0)
    assigned = int((want == 1).sum()) - 72
    assert 0 < assigned < 9 * 62 - 1 and want[4, 30] == 0
    grown, gained, rounds = RF.grow(_dev(fids), _dev(ids), _dev(noisy), table, grow_m=0.0)
    _same(grown, want, "grown")
    assert rounds == used and gained.tolist() == [assigned]


def test_facet_ids_out_of_range_are_counted_and_never_used():
    """words outside [0, F] and a facet root outside the raster: counted in every round, copied, no candidates; roofs.grow raises"""
    t = N.town()
    fids = t["fids"].copy()
    fids[5, 16], fids[30, 10], fids[0, 0] = t["F"] + 3, -5, 2 ** 31 - 1
    root = np.asarray(t["root"]).copy()
    assert t["table"]["object"][3] == 3
    root[3] = 48 * 64                                               # a facet of the hipped roof: one past the raster
    want, stats = N.grow_rounds(fids, t["ids"], t["key"], root, t["planes"], t["F"], RN.UNIT, 256, 3)
    assert stats[3] >= 9 and want[5, 16] == t["F"] + 3 and want[30, 10] == -5 and want[0, 0] == 2 ** 31 - 1
    result, other, got = _grow_entry(fids, t["ids"], t["key"], root, t["planes"], t["F"], RN.UNIT, 256, 3)
    assert got == stats
    _same(result, want, "grown")
    _same(other, N.grow_rounds(fids, t["ids"], t["key"], root, t["planes"], t["F"], RN.UNIT, 256, 2)[0], "the round before")
    with pytest.raises(RuntimeError, match="guard trip"):
        RF.grow(_dev(fids), _dev(t["ids"]), _dev(t["key"]), t["table"])
    nothing = RF.grow(_dev(np.zeros((48, 64), np.int32)), _dev(t["ids"]), _dev(t["key"]), {"object": [], "plane": np.zeros((0, 3)), "root": []})
    assert not nothing[0].any() and nothing[1].size == 0 and nothing[2] == 0


# ---- the export -------------------------------------------------------------------------------------------------------------------------------
def _town_objects(t):
    label = np.where(t["ids"] > 0, 3, 0).astype(np.uint8)
    d_ids = _dev(t["ids"])
    rows, _ = OB.object_rows(d_ids, 5, _dev(label), _dev(t["alt"]), ground=(0,))
    return {"ids": d_ids, "n": 5, "table": OB.object_table(rows, t["grid"])}


def _digests(files):
    return {name: hashlib.sha256(open(p, "rb").read()).hexdigest() for name, p in sorted(files.items())}


def _by_building(records):
    out = {}
    for rec in records:
        out.setdefault(rec["object"], {}).setdefault(rec["kind"], []).append(rec["length_m"])
    return {n: {k: sorted(v) for k, v in kinds.items()} for n, kinds in out.items()}


def test_export_roofs_with_lines_on_the_town(tmp_path, monkeypatch):
    """arcs() and export_roofs(lines=True, polygons=True, shared=True) end to end: the files, the GeoJSON, the kinds and lengths of
    tests/test_rooflines_cpu.py; without the new keywords export_roofs writes the bytes it wrote before, launches none of the new
    entries, and so do the other exports"""
    t = N.town()
    objects = _town_objects(t)
    products = {"dsm": _dev(t["alt"]), "label": _dev(np.where(t["ids"] > 0, 3, 0).astype(np.uint8)), "grid": t["grid"]}
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (called.append(name), real(name, *a, **kw))[1])
    new = ("snerf_roofs_grow", "snerf_arcs_first", "snerf_arcs_mark", "snerf_arcs_fold")
    plain = EO.export_roofs(products, objects, str(tmp_path / "plain"), zone_string="17R")
    poly = EO.export_roofs(products, objects, str(tmp_path / "poly"), zone_string="17R", polygons=True)
    other = EO.export_objects(products, str(tmp_path / "plain"), classes=(3,), zone_string="17R")
    before = _digests(plain["files"]), _digests(poly["files"]), _digests(other["files"])
    names = {"pitch.tif", "pitch.png", "aspect.png", "facets.tif", "residual.tif", "residual.png", "roofs.json"}
    assert set(plain["files"]) == names and not [c for c in called if c in new]
    out = EO.export_roofs(products, objects, str(tmp_path / "lines"), zone_string="17R", lines=True, polygons=True, shared=True)
    assert [c for c in called if c in new] == list(new)
    added = {"lines.geojson", "lines.json", "facets_grown.tif", "facets.geojson"}
    assert set(out["files"]) == names | added == set(os.listdir(tmp_path / "lines" / "roofs"))
    assert all(os.path.getsize(p) > 0 for p in out["files"].values())
    for name in names:
        assert open(out["files"][name], "rb").read() == open(plain["files"][name], "rb").read(), name
    _same(out["facet_ids_grown"], t["grown"], "grown")
    assert out["grow_rounds"] == 1 and int(out["grown_cells"].sum()) == 80
    assert out["arc_stats"] == {"edges": 530, "arcs": 24, "vertices": 204, "rings": 10, "breaks": 22, "twin_edges": 222}
    doc = json.load(open(out["files"]["lines.geojson"]))
    assert doc["type"] == "FeatureCollection" and doc["crs"]["properties"]["name"] == "urn:ogc:def:crs:EPSG::32617"
    assert len(doc["features"]) == len(out["lines"]) == 28
    for f, rec in zip(doc["features"], json.loads(json.dumps(out["lines"]))):
        assert f["geometry"]["type"] == "LineString" and f["geometry"]["coordinates"] == rec["coordinates"]
        assert all(len(c) == 3 for c in f["geometry"]["coordinates"]) and f["properties"]["kind"] == rec["kind"]
    by = _by_building([f["properties"] for f in doc["features"]])
    assert by[1] == {"flat_edge": [22.0]} and by[2] == {"ridge": [8.0], "eave": [8.0, 8.0], "rake": [4.0] * 4}
    assert by[4] == {"eave": [7.0], "top": [7.0], "rake": [7.0, 7.0]} and by[5]["step"] == [10.0] and set(by[5]) == {"step", "flat_edge"}
    assert by[3]["ridge"] == [0.5] and len(by[3]["hip"]) == 4 and "valley" not in by[3] and "crease" not in by[3]
    ridge = next(r for r in out["lines"] if r["object"] == 2 and r["kind"] == "ridge")
    assert all(abs(c[2] - 11.875) <= 1e-9 for c in ridge["coordinates"])
    summary = json.load(open(out["files"]["lines.json"]))
    assert summary["rounds"] == 1 and sum(summary["grown_cells"]) == 80 and summary["counts"]["hip"] == 4 and summary["counts"]["step"] == 1
    assert [b["ridge"] for b in summary["buildings"]] == [0.0, 8.0, 0.5, 0.0, 0.0] and summary["parameters"]["grow_m"] == 0.25
    shared = json.load(open(out["files"]["facets.geojson"]))
    assert len(shared["features"]) == out["n_facets"] == 10
    # the polygons tile the buildings: their areas add up to the building cells, which the facets alone (1132 cells) do not
    def area(ring):
        a = np.asarray(ring, np.float64) - np.asarray(ring[0], np.float64)
        return 0.5 * float((a[:-1, 0] * a[1:, 1] - a[1:, 0] * a[:-1, 1]).sum())
    total = sum(area(r) for f in shared["features"] for r in f["geometry"]["coordinates"])
    assert total == 1212 * 0.25
    # the old paths after the new ones were used: the same bytes
    del called[:]
    again = (_digests(EO.export_roofs(products, objects, str(tmp_path / "plain2"), zone_string="17R")["files"]),
             _digests(EO.export_roofs(products, objects, str(tmp_path / "poly2"), zone_string="17R", polygons=True)["files"]),
             _digests(EO.export_objects(products, str(tmp_path / "plain2"), classes=(3,), zone_string="17R")["files"]))
    assert again == before and called and not [c for c in called if c in new]
