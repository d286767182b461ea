"""CPU-side checks of the roof lines (include/snerf_rooflines.h, csrc/rooflines.hip, eval/utils/arcs.py, roofs.grow / lines, outline.
simplify_shared): the new header's prototypes and constants against the binding, every refusal of the four entries
through the binding (none reaches a launch), the two restatements of tests/rooflines_numpy.py against each other and against facts that
know nothing of tracing (the rings' edge counts, the twin involution, Euler's relation with scipy's labels), the town's numbers, and the
host side: the roof lines of the town, the gap-free simplification, and export_roofs' unchanged parameter list."""
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy import ndimage

from snerf_amd import _lib
from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import arcs as AR          # the feature under test: every test of this file needs it
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import outline as OL
from snerf_amd.eval.utils import roofs as RF
from tests import outline_numpy as ON
from tests import roofs_numpy as RN
from tests import rooflines_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_rooflines.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_roofs_grow": ["fids", "ids", "key", "facet_root", "planes", "h", "w", "F", "unit", "max_rq", "rounds", "a", "b", "stats", "stream"],
    "snerf_arcs_first": ["ids", "slot", "ring", "rank", "h", "w", "K", "E", "node", "first", "stats", "stream"],
    "snerf_arcs_mark": ["ids", "sides", "offsets", "slot", "flags", "ring", "rank", "totals", "node", "first", "ring_row", "ring_base", "h", "w",
                        "K", "E", "n_rings", "left", "twin", "pos_of", "order", "hf", "vf", "stats", "stream"],
    "snerf_arcs_fold": ["ids", "key", "slot", "ring", "left", "twin", "pos_of", "node", "ring_row", "order", "hf", "vf", "arc_of", "ordinal",
                        "last", "vertex_offset", "h", "w", "E", "A", "n_rings", "V", "vertices", "rows", "stats", "stream"],
}
# the rasters of the issue: outline_numpy's named rasters at 4 and 8, the 5 x 7 checkerboard, two_rectangles and blobs at 37 x 53, and
# the GPU tests' extra ones (2 x 130, 1 x 1, all zero)
RASTERS = list(N.rasters())


# ---- header and binding -------------------------------------------------------------------------------------------------------------------
def test_the_new_header_matches_its_binding_rows():
    """include/snerf_rooflines.h against _lib.LATER_HEADER_SIGNATURES["snerf_rooflines.h"], as tests/test_outline_cpu.py holds its
    header to its rows: names, order, return type, per parameter class, width and signedness, the stream marker; lib() and call() serve
    the rows; the ABI stays 6 and the main header names nothing of this one"""
    from tests.test_abi_cpu import _c_type, _table_type
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(snerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        protos[name] = (_c_type(ret), [(_c_type(t), n) for t, n in (re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(","))])
    rows = _lib.LATER_HEADER_SIGNATURES["snerf_rooflines.h"]
    assert list(rows) == list(protos) == list(NAMES)
    for symbol, (ret, params) in protos.items():
        restype, argtypes = rows[symbol]
        assert _table_type(restype) == ret == ("int", 4, True), (symbol, restype, ret)
        assert len(argtypes) == len(params) and [n for _, n in params] == NAMES[symbol], (symbol, params)
        for k, (t, (want, pname)) in enumerate(zip(argtypes, params)):
            got = _table_type(t)
            assert got == want or (want[0] == "pointer" and got == ("pointer", None)), (symbol, k, pname, t, want)
            assert (t is _lib.c_stream) == (pname == "stream"), (symbol, k, pname)
        fn = getattr(_lib.lib(), symbol)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes) and symbol in _lib._PLANS
        assert symbol not in _lib.SIGNATURES and symbol not in _lib.EXPORTED_SYMBOLS
        assert all(symbol not in other for other in list(_lib.HEADER_SIGNATURES.values()) + list(_lib.ADDED_HEADER_SIGNATURES.values()))
    wide = {n for _, params in protos.values() for (t, n) in params if t == ("int", 8, True)}
    assert wide == {"F", "max_rq", "K", "E", "A", "n_rings", "V"}
    assert list(_lib.LATER_HEADER_SIGNATURES) == ["snerf_outline.h", "snerf_rooflines.h"]
    assert len(_lib.EXPORTED_SYMBOLS) == 53 and _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    main = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    assert not [word for word in ["snerf_rooflines", "SNERF_ARCS_", "SNERF_GROW_"] + list(protos) if word in main]
    assert '#include "snerf_hip.h"' in text


def test_the_constants():
    consts = {k: int(v) for k, v in re.findall(r"#define (SNERF_\w+) (\d+)", open(HEADER).read())}
    assert consts == {"SNERF_ARCS_ROW_WORDS": 12, "SNERF_ARCS_NO_FIRST": 2 ** 31 - 1, "SNERF_GROW_MAX_ROUNDS": 64}
    assert _lib.ARCS_ROW_WORDS == AR.ROW_WORDS == N.ROW_WORDS == 12 and _lib.ARCS_NO_FIRST == AR.NO_FIRST == N.NO_FIRST == 2 ** 31 - 1
    assert _lib.GROW_MAX_ROUNDS == N.MAX_ROUNDS == 64 and RF.GROW_BATCH == 8


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
BASE = dict({name: (k + 1) * DUMMY for k, name in enumerate(
    ["fids", "ids", "key", "facet_root", "planes", "a", "b", "stats", "slot", "ring", "rank", "node", "first", "sides", "offsets", "flags",
     "totals", "ring_row", "ring_base", "left", "twin", "pos_of", "order", "hf", "vf", "arc_of", "ordinal", "last", "vertex_offset",
     "vertices", "rows"])}, h=6, w=8, F=4, unit=64.0, max_rq=256, rounds=8, K=3, E=10, n_rings=2, A=3, V=8)


def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(BASE, **kw)
    rc = getattr(L, symbol)(*[a[n] for n in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


inf, nan = math.inf, math.nan
CELLS = [({"h": 0}, 1, ">= 1"), ({"w": -1}, 1, ">= 1"), ({"h": 16384, "w": 32768}, 1, "below 2^29"),
         ({"h": 2 ** 31 - 1, "w": 2 ** 31 - 1}, 1, "below 2^29")]
IDS = [({"K": -1}, 1, "K = -1"), ({"K": 2 ** 31}, 1, "K = 2147483648")]
COUNTS = [({"E": -1}, 1, "E = -1"), ({"E": 193}, 1, "E = 193")]
CASES = (
    [("snerf_roofs_grow", {p: None}, 3, "null") for p in ("fids", "ids", "key", "facet_root", "planes", "a", "b", "stats")]
    + [("snerf_roofs_grow",) + c for c in [
        ({"h": 0}, 1, ">= 1"), ({"w": -3}, 1, ">= 1"), ({"h": 8193}, 1, "at most 8192"), ({"w": 2 ** 31 - 1}, 1, "at most 8192"),
        ({"F": -1}, 1, "F = -1"), ({"F": 2 ** 27}, 1, "[0, 2^27)"), ({"rounds": 0}, 1, "rounds = 0"), ({"rounds": 65}, 1, "rounds = 65"),
        ({"rounds": -1}, 1, "rounds = -1"), ({"unit": 0.0}, 1, "unit > 0"), ({"unit": -64.0}, 1, "unit > 0"), ({"unit": inf}, 1, "unit > 0"),
        ({"unit": nan}, 1, "unit > 0"), ({"max_rq": -1}, 1, "max_rq = -1")]]
    + [("snerf_arcs_first", {p: None}, 3, "null") for p in ("ids", "slot", "ring", "rank", "node", "first", "stats")]
    + [("snerf_arcs_first",) + c for c in CELLS + IDS + COUNTS]
    + [("snerf_arcs_mark", {p: None}, 3, "null") for p in NAMES["snerf_arcs_mark"][:12] + NAMES["snerf_arcs_mark"][17:24]]
    + [("snerf_arcs_mark",) + c for c in CELLS + IDS + COUNTS + [({"n_rings": -1}, 1, "n_rings = -1"), ({"n_rings": 193}, 1, "n_rings = 193")]]
    + [("snerf_arcs_fold", {p: None}, 3, "null") for p in ["ids"] + NAMES["snerf_arcs_fold"][2:16] + NAMES["snerf_arcs_fold"][22:25]]
    + [("snerf_arcs_fold",) + c for c in CELLS + COUNTS + [
        ({"A": -1}, 1, "A = -1"), ({"A": 193}, 1, "A = 193"), ({"n_rings": 193}, 1, "n_rings = 193"), ({"V": -1}, 1, "V = -1"),
        ({"V": 385}, 1, "V = 385")]]
)


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{c[0][6:]}-{n}" for n, c in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **kw)
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_the_empty_problem_launches_nothing():
    """E = 0 is accepted by the three arc entries with null buffers (there is no device here to launch on); a null key is accepted by
    fold's checks; V may reach 8 h w, two vertices an edge"""
    none = {p: None for p in BASE if isinstance(BASE[p], int) and BASE[p] >= DUMMY and p not in ("ids", "sides", "offsets", "stats")}
    for symbol in ("snerf_arcs_first", "snerf_arcs_mark", "snerf_arcs_fold"):
        assert _call(symbol, **dict(none, E=0, A=0, V=0, n_rings=0))[0] == 0, symbol
    assert _call("snerf_arcs_fold", key=None, V=385)[1].endswith("(V = 385, h = 6, w = 8)")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _agree(a, b):
    for key, want in b.items():
        got = a[key]
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), key
        else:
            assert got == want, key


@pytest.mark.parametrize("name", RASTERS)
def test_the_two_restatements_agree_bit_for_bit(name):
    """every entry over whole arrays (positions, cumulative sums, row folds: the oracle of the GPU tests) against a sequential walk
    that follows `next` round each ring, cuts at the nodes and pairs the twins through a dictionary of reversed segments"""
    ids, K, connectivity = N.rasters()[name]
    a = N.trace_of(name)
    _agree(a, N.walk(ids, K, connectivity, key=N.key_of(name)))
    E = a["E"]
    assert a["first_stats"][0] == 0 and a["mark_stats"][:2] == [0, E] and a["fold_stats"] == [0, a["V"]]
    assert sorted(a["order"].tolist()) == list(range(E)) and np.array_equal(a["order"][a["pos_of"]], np.arange(E))


def _components(ids, K):
    """the 4-connected components of every id value, numbered 1.. -> (ids, count)"""
    n = ON.normalised(ids, K)
    out, count = np.zeros(n.shape, np.int32), 0
    for v in range(1, K + 1):
        lab, m = ndimage.label(n == v)
        out[lab > 0] = lab[lab > 0] + count
        count += m
    return out, count


@pytest.mark.parametrize("name", RASTERS)
def test_the_arcs_against_facts_that_know_nothing_of_tracing(name):
    """per id the arcs with that id on the right add up to the rings' edges; the twin map is an involution with equal edges and swapped
    ids; a twin's vertex list is the arc's reversed (a closed arc's up to where it starts); Euler's relation V' - A + F = 1 + C with
    V' = nodes + closed arcs, A = distinct arcs, F = scipy's 4-connected components of every id value on the padded raster and C = the
    components of the cracks drawn on the (2 h + 1) x (2 w + 1) lattice"""
    ids, K, connectivity = N.rasters()[name]
    t = N.trace_of(name)
    a = N.arcs_of(t)
    rings = ON.rings_of(t["outline"])
    n_arcs = a["n_arcs"]
    per_id = np.zeros(K + 1, np.int64)
    np.add.at(per_id, a["right"], a["edges"])
    want = np.zeros(K + 1, np.int64)
    np.add.at(want, rings["ring_object"], rings["ring_edges"])
    assert np.array_equal(per_id, want) and int(a["edges"].sum()) == t["E"]
    twin = a["twin"]
    has = twin >= 0
    assert np.array_equal(has, a["left"] > 0) and np.array_equal(twin[twin[has]], np.flatnonzero(has))
    assert np.array_equal(a["edges"][twin[has]], a["edges"][has]) and np.array_equal(a["right"][twin[has]], a["left"][has])
    assert np.array_equal(a["closed"][twin[has]], a["closed"][has]) and int((a["owner"] & has).sum()) * 2 == int(has.sum())
    assert (t["rows"][:, 6].astype(np.int64) == a["edges"] * t["rows"][:, 5].astype(np.int64)).all()
    for k in np.flatnonzero(has).tolist():
        mine, theirs = OL.arc_points(a, k), OL.arc_points(a, int(twin[k]))[::-1]
        if a["closed"][k]:
            at = theirs.index(mine[0])
            theirs = theirs[at:] + theirs[:at]
        assert mine == theirs, k
    n = ON.normalised(ids, K)
    h, w = n.shape
    P = np.pad(n, 1)
    faces = sum(ndimage.label(P == v)[1] for v in np.unique(P).tolist())
    cracks = np.zeros((2 * h + 3, 2 * w + 3), bool)                  # vertices at even, edges at odd positions of the padded lattice
    vert = P[:, 1:] != P[:, :-1]                                      # between columns i - 1 and i of row j: a vertical crack
    horz = P[1:, :] != P[:-1, :]
    jj, ii = np.nonzero(vert)
    for dj in (0, 1, 2):
        cracks[2 * jj + dj, 2 * ii + 2] = True
    jj, ii = np.nonzero(horz)
    for di in (0, 1, 2):
        cracks[2 * jj + 2, 2 * ii + di] = True
    C = ndimage.label(cracks)[1]
    nodes = int(N.nodes(ids, K).sum())
    distinct = n_arcs - int(has.sum()) // 2
    closed = int(a["closed"].sum()) - int((a["closed"] & has).sum()) // 2
    assert nodes + closed - distinct + faces == 1 + C, (nodes, closed, distinct, faces, C)
    if name == "checkerboard_5x7":
        # every vertex but the raster's four corners (two cracks each) is a node: every arc is one edge, but for the four arcs of two
        # edges that turn round those corners
        assert nodes == 6 * 8 - 4 and sorted(a["edges"].tolist()) == [1] * (n_arcs - 4) + [2] * 4 and n_arcs == t["E"] - 4


# ---- the town ---------------------------------------------------------------------------------------------------------------------------
def test_the_town_grows_in_one_round_and_has_17_arcs():
    """after filter_facets(min_facet_m2 = 4) 80 building cells carry no facet; one round assigns all of them and the second none; the
    grown raster has 10 nodes and 17 distinct arcs with the edge counts of DESIGN.md section 5zf"""
    t = N.town()
    assert t["F"] == 10 and int(((t["fids"] == 0) & (t["ids"] > 0)).sum()) == 80
    assert t["counts"][:2] == [80, 0] and t["rounds"] == 1 and int(((t["grown"] == 0) & (t["ids"] > 0)).sum()) == 0
    assert np.array_equal(t["grown"][t["fids"] > 0], t["fids"][t["fids"] > 0])              # a kept cell is never changed
    assert all(ndimage.label(t["grown"] == n)[1] == 1 for n in range(1, 11))                 # a grown facet stays one component
    tr = N.trace(t["grown"], t["F"], 4, key=t["key"])
    _agree(tr, N.walk(t["grown"], t["F"], 4, key=t["key"]))
    a = N.arcs_of(tr)
    assert int(N.nodes(t["grown"], t["F"]).sum()) == 10 and a["n_arcs"] == 24
    owner, obj = a["owner"], t["table"]["object"]
    assert int(owner.sum()) == 17
    inner = owner & (a["left"] > 0)
    outer = owner & (a["left"] == 0) & ~a["closed"]
    closed = owner & a["closed"]
    assert sorted(a["edges"][closed].tolist()) == [44, 56] and sorted(obj[a["right"][closed] - 1].tolist()) == [1, 4]
    assert sorted(a["edges"][inner].tolist()) == [1, 16, 18, 18, 19, 19, 20]
    assert sorted(a["edges"][outer].tolist()) == [18, 20, 20, 22, 32, 32, 32, 32]
    # V' - A + F = 1 + C: 12 - 17 + 11 = 1 + 5
    assert 10 + 2 - 17 + 11 == 1 + 5
    # the keys on both sides of the step: 20 edges, 6 m = 24 * 16384 key units apart
    step = int(np.flatnonzero(inner & (a["edges"] == 20))[0])
    assert a["key_edges"][step] == 20 and abs(int(a["key_sum_right"][step] - a["key_sum_left"][step])) == 20 * 24 * RN.TOWN_STEP


def _town_lines(**kw):
    t = N.town()
    a = N.arcs_of(N.trace(t["grown"], t["F"], 4, key=t["key"]))
    return RF.lines(a, t["table"], t["grid"], **kw), a


def _by_building(records):
    out = {}
    for rec in records:
        out.setdefault(rec["object"], {}).setdefault(rec["kind"], []).append(rec["length_m"])
    return {n: {k: sorted(v) for k, v in kinds.items()} for n, kinds in out.items()}


def test_the_roof_lines_of_the_town():
    records, _ = _town_lines(simplify_cells=0)
    by = _by_building(records)
    assert by[2] == {"ridge": [8.0], "eave": [8.0, 8.0], "rake": [4.0] * 4}
    ridge = next(r for r in records if r["object"] == 2 and r["kind"] == "ridge")
    assert ridge["pitch_deg"] == 0.0 and all(abs(c[2] - 11.875) <= 1e-9 for c in ridge["coordinates"])
    assert by[4] == {"eave": [7.0], "top": [7.0], "rake": [7.0, 7.0]}
    assert by[1] == {"flat_edge": [22.0]}
    assert by[5]["step"] == [10.0] and set(by[5]) == {"step", "flat_edge"}
    step = next(r for r in records if r["kind"] == "step")
    assert step["step_m"] == 6.0 and all(c[2] == 16.0 for c in step["coordinates"])
    assert by[3]["ridge"] == [0.5] and len(by[3]["hip"]) == 4 and "valley" not in by[3] and "crease" not in by[3]
    assert all(r["step_m"] is None for r in records if r["kind"] != "step")
    # an eave's height over the cells across it: the gable's eaves lie 0.125 m below the ground the roof model meets there
    eave = next(r for r in records if r["object"] == 2 and r["kind"] == "eave")
    assert abs(eave["height_m"] + 0.125) <= 1e-9 and abs(eave["pitch_deg"]) <= 1e-9
    table = RF.line_table(records, 5)
    assert table["lines"].tolist() == [1, 7, 13, 4, 3] and table["ridge"].tolist() == [0.0, 8.0, 0.5, 0.0, 0.0]
    assert table["step"].tolist() == [0.0, 0.0, 0.0, 0.0, 10.0] and table["flat_edge"].tolist() == [22.0, 0.0, 0.0, 0.0, 32.0]
    assert set(table) == {"lines"} | set(RF.LINE_KINDS) and not table["valley"].any() and not table["crease"].any()
    # the thresholds are parameters: with a step of 7 m allowed the two flats meet in a crease, and at 30 degrees nothing is pitched
    assert _by_building(_town_lines(step_m=7.0)[0])[5].get("crease") == [10.0]
    level = _by_building(_town_lines(level_deg=30.0)[0])
    assert "ridge" not in level[2] and "eave" not in level[2] and level[2]["crease"] == [8.0]
    with pytest.raises(ValueError, match="no altitudes"):
        RF.lines(_town_lines()[1], dict(N.town()["table"], alt=np.full(10, np.nan)), N.town()["grid"])


# ---- gap-free simplification ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1, 2.5])
@pytest.mark.parametrize("which", ["town", "blobs"])
def test_simplify_shared_keeps_neighbours_gap_free(which, tol):
    """on the grown town and on the 4-connected components of blobs 37 x 53 (polygons() takes one outer ring per id, so the blobs'
    ids are split into their components first): every directed segment with a left id > 0 has its reverse in that id's polygon, and
    every dropped vertex lies within the tolerance of the segment that replaced it"""
    if which == "town":
        t = N.town()
        ids, K = t["grown"], t["F"]
    else:
        ids, K = _components(*RN.id_raster(37, 53, "blobs"))
    a = N.arcs_of(N.trace(ids, K, 4))
    out = OL.simplify_shared(a, tol)
    full = OL.simplify_shared(a, 0)
    assert list(out) == list(full) == list(range(1, K + 1))
    t2 = Fraction(tol) ** 2
    segments, vertices = {}, {}
    for n, rings in out.items():
        lists = [[tuple(v) for v in ring.tolist()] for ring in rings]
        segments[n] = {(u, v) for pts in lists for u, v in zip(pts, pts[1:] + pts[:1])}
        vertices[n] = {u for pts in lists for u in pts}
    shared = dropped = 0
    for k in range(len(a["right"])):
        R, L = int(a["right"][k]), int(a["left"][k])
        pts = OL.arc_points(a, k)
        # the arc's kept vertices: an inner vertex of an arc lies on no other arc of R's rings, and an open arc's ends (nodes) stay
        if a["closed"][k]:
            kept = [i for i, p in enumerate(pts) if p in vertices[R]]
            if len(kept) < 3:
                continue                                            # a hole that fell below 3 vertices was dropped
            pairs = list(zip(kept, kept[1:] + [kept[0] + len(pts)]))
            pts = pts + pts
        else:
            kept = [i for i, p in enumerate(pts) if i in (0, len(pts) - 1) or p in vertices[R]]
            pairs = list(zip(kept, kept[1:]))
        for i, j in pairs:
            u, v = pts[i], pts[j]
            assert (u, v) in segments[R], (k, u, v)
            if L > 0:
                assert (v, u) in segments[L], (k, u, v)
                shared += 1
            for q in pts[i + 1:j]:
                assert OL._dist2(q, u, v) <= t2, (k, q, u, v)
                dropped += 1
    assert shared > 0 and dropped > 0


@pytest.mark.parametrize("name", ["blobs", "checkerboard", "two_rectangles_37x53", "bullseye-4", "random_33x64-4", "random_33x64-8",
                                  "saddle-4", "spiral-4", "two_rows_2x130", "one_cell", "all_zero", "town"])
def test_simplify_shared_at_tolerance_0_is_polygons_of_rings(name):
    """vertex for vertex: the arcs' concatenation without the nodes that are no corners, turned to the ring's start"""
    if name == "town":
        t = N.town()
        ids, K, connectivity = t["grown"], t["F"], 4
    elif name in ("blobs", "checkerboard"):                           # one polygon per id: the components of the id values
        ids, K = _components(*(RN.id_raster(37, 53, "blobs") if name == "blobs" else RN.id_raster(5, 7, "checkerboard")))
        connectivity = 4
    else:
        ids, K, connectivity = N.rasters()[name]
    tr = N.trace(ids, K, connectivity)
    a = N.arcs_of(tr)
    want = OL.polygons(ON.rings_of(tr["outline"]))
    got = OL.simplify_shared(a, 0)
    assert list(got) == list(want)
    for n in want:
        assert len(got[n]) == len(want[n]) and all(x.dtype == np.int64 and np.array_equal(x, y) for x, y in zip(got[n], want[n])), n
    with pytest.raises(ValueError, match="negative"):
        OL.simplify_shared(a, -1)


def test_simplify_shared_puts_a_region_back_that_collapses():
    """a 1 x 6 sliver between two large facets falls to a 2-gon at 2 cells: its arcs (and with them its neighbours' copies) are put back
    unsimplified, and the neighbours still match it segment for segment"""
    ids = np.zeros((12, 14), np.int32)
    ids[2:10, 2:12] = 1
    ids[5, 4:10] = 2
    a = N.arcs_of(N.trace(ids, 2, 4))
    out = OL.simplify_shared(a, 2)
    assert out[2][0].tolist() == [[4, 5], [10, 5], [10, 6], [4, 6]] and out[1][0].tolist() == [[2, 2], [12, 2], [12, 10], [2, 10]]
    assert sorted(map(tuple, out[1][1].tolist())) == sorted(map(tuple, out[2][0].tolist()))


# ---- the export's parameters ------------------------------------------------------------------------------------------------------------------
def test_export_roofs_keeps_its_parameter_list(monkeypatch):
    """the five new keywords are taken out of **kwargs before roofs() sees them, as polygons and simplify_m are; a host tensor is still
    the first thing export_roofs refuses, with or without them"""
    assert list(inspect.signature(EO.export_roofs).parameters) == ["products", "objects_result", "output_dp", "alt_key", "reference", "zone_string",
                                                                   "kwargs"]
    products = {"dsm": torch.zeros((4, 5)), "grid": D.DsmGrid(0.0, 0.0, 0.5, 5, 4)}
    objects = {"ids": torch.zeros((4, 5), dtype=torch.int32), "n": 0, "table": {"area_cells": np.zeros(0), "ground_alt": np.zeros(0)}}
    new = {"lines": True, "shared": True, "grow_m": 0.5, "step_m": 2.0, "level_deg": 3.0}
    for kw in ({}, new, dict(new, polygons=True, simplify_m=1.0)):
        with pytest.raises(ValueError, match="alt must be a GPU tensor"):
            EO.export_roofs(products, objects, "unused", **kw)
    seen = {}

    class Stop(Exception):
        pass

    def roofs(*args, **kwargs):
        seen.update(kwargs)
        raise Stop

    monkeypatch.setattr(RF, "roofs", roofs)
    with pytest.raises(Stop):
        EO.export_roofs(products, objects, "unused", radius=2, **new)
    assert seen == {"radius": 2}
    assert inspect.signature(RF.grow).parameters["grow_m"].default == 0.25 and inspect.signature(RF.lines).parameters["step_m"].default == 1.0
    assert inspect.signature(RF.lines).parameters["level_deg"].default == 5.0
