"""CPU-side checks of the outlines (include/snerf_outline.h, csrc/outline.hip, eval/utils/outline.py): the new
header's prototypes and constants against the binding (_lib.LATER_HEADER_SIGNATURES), every refusal of the five entries through the binding
(none reaches a launch), the two restatements of tests/outline_numpy.py against each other and against facts that know nothing of
boundary tracing (areas, perimeters, scipy's hole counts, the object table's bounding boxes), and the host side: polygons, the exact
Douglas-Peucker, map coordinates and GeoJSON."""
import ctypes as C
import functools
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from snerf_amd import _lib
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import outline as OL       # the feature under test: every test of this file needs it
from tests import objects_numpy as ON
from tests import outline_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_outline.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_outline_sides": ["ids", "h", "w", "K", "sides", "stats", "stream"],
    "snerf_outline_link": ["ids", "sides", "offsets", "h", "w", "K", "connectivity", "E", "slot", "next", "flags", "stats", "stream"],
    "snerf_outline_workspace_bytes": ["E"],
    "snerf_outline_rank": ["next", "flags", "E", "ring", "rank", "ordinal", "totals", "workspace", "workspace_bytes", "stats", "stream"],
    "snerf_outline_emit": ["ids", "slot", "flags", "ring", "ordinal", "ring_row", "vertex_offset", "h", "w", "E", "n_rings", "V", "vertices",
                           "rows", "stats", "stream"],
}
RASTERS = list(N.labels())
GRID = D.DsmGrid(500000.0, 4100000.0, 0.5, 130, 96)


# ---- header and binding -------------------------------------------------------------------------------------------------------------------
def test_the_new_header_matches_its_binding_rows():
    """include/snerf_outline.h against _lib.LATER_HEADER_SIGNATURES["snerf_outline.h"], as tests/test_warp_cpu.py holds its header to its
    table: names, order, return type, per parameter class, width and signedness, the stream marker; lib() and call() serve the rows; the
    older tables are what they were; the main header names nothing of this one"""
    from tests.abi_header import FROZEN
    from tests.test_abi_cpu import _c_type, _table_type
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(snerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        protos[name] = (_c_type(ret), [(_c_type(t), n) for t, n in (re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(","))])
    rows = _lib.LATER_HEADER_SIGNATURES["snerf_outline.h"]
    assert list(rows) == list(protos) == list(NAMES)
    for symbol, (ret, params) in protos.items():
        restype, argtypes = rows[symbol]
        want_ret = ("int", 8, True) if symbol == "snerf_outline_workspace_bytes" else ("int", 4, True)
        assert _table_type(restype) == ret == want_ret, (symbol, restype, ret)
        assert len(argtypes) == len(params) and [n for _, n in params] == NAMES[symbol], (symbol, params)
        for k, (t, (want, pname)) in enumerate(zip(argtypes, params)):
            got = _table_type(t)
            assert got == want or (want[0] == "pointer" and got == ("pointer", None)), (symbol, k, pname, t, want)
            assert (t is _lib.c_stream) == (pname == "stream"), (symbol, k, pname)
        fn = getattr(_lib.lib(), symbol)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes) and symbol in _lib._PLANS
        assert symbol not in _lib.SIGNATURES and symbol not in _lib.EXPORTED_SYMBOLS
        assert all(symbol not in other for other in list(_lib.HEADER_SIGNATURES.values()) + list(_lib.ADDED_HEADER_SIGNATURES.values()))
    # K, E, n_rings, V and workspace_bytes are 64-bit; h, w and connectivity are ints
    wide = {n for _, params in protos.values() for (t, n) in params if t == ("int", 8, True)}
    assert wide == {"K", "E", "n_rings", "V", "workspace_bytes"}
    assert {h: list(r) for h, r in _lib.HEADER_SIGNATURES.items()} == FROZEN and list(_lib.HEADER_SIGNATURES) == list(FROZEN)
    assert list(_lib.ADDED_HEADER_SIGNATURES) == ["snerf_warp.h"] and list(_lib.ADDED_HEADER_SIGNATURES["snerf_warp.h"]) == ["snerf_warp_planes",
                                                                                                                              "snerf_warp_labels"]
    assert len(_lib.EXPORTED_SYMBOLS) == 53 and _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    main = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    own = ["snerf_outline"] + list(protos) + re.findall(r"^#define (SNERF_[A-Z0-9]+_)", text, flags=re.M)
    assert "SNERF_OUTLINE_" in own and not [word for word in own if word in main]
    assert '#include "snerf_hip.h"' in text


def test_the_constants():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SNERF_OUTLINE_\w+) (\d+)", text)}
    assert consts == {"SNERF_OUTLINE_ROW_WORDS": 8, "SNERF_OUTLINE_MAX_CELLS": 2 ** 29, "SNERF_OUTLINE_CORNER": 1}
    assert _lib.OUTLINE_ROW_WORDS == OL.ROW_WORDS == N.ROW_WORDS == 8 and _lib.OUTLINE_MAX_CELLS == OL.MAX_CELLS == 2 ** 29
    assert _lib.OUTLINE_CORNER == OL.CORNER == N.CORNER == 1
    assert [v % 2 ** 64 for v in OL._ROW_INIT] == N.ROW_INIT and len(N.ROW_INIT) == 8


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
BASE = dict(ids=DUMMY, sides=2 * DUMMY, offsets=3 * DUMMY, h=6, w=8, K=3, connectivity=4, E=10, slot=4 * DUMMY, next=5 * DUMMY, flags=6 * DUMMY,
            stats=7 * DUMMY, ring=8 * DUMMY, rank=9 * DUMMY, ordinal=10 * DUMMY, totals=11 * DUMMY, workspace=12 * DUMMY, workspace_bytes=240,
            ring_row=13 * DUMMY, vertex_offset=14 * DUMMY, n_rings=2, V=8, vertices=15 * DUMMY, rows=16 * DUMMY)


def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(BASE, **kw)
    names = NAMES[symbol]
    args = [a[n] for n in names if n != "stream"] + ([None] if "stream" in names else [])
    rc = getattr(L, symbol)(*args)
    return rc, L.snerf_last_error().decode()


SIZES = [({"h": 0}, 1, ">= 1"), ({"w": -1}, 1, ">= 1"), ({"h": 16384, "w": 32768}, 1, "below 2^29"),
         ({"h": 2 ** 31 - 1, "w": 2 ** 31 - 1}, 1, "below 2^29")]
IDS = [({"K": -1}, 1, "K = -1"), ({"K": 2 ** 31}, 1, "K = 2147483648")]
CASES = (
    [("snerf_outline_sides", {p: None}, 3, "null") for p in ("ids", "sides", "stats")]
    + [("snerf_outline_sides",) + c for c in SIZES + IDS]
    + [("snerf_outline_link", {p: None}, 3, "null") for p in ("ids", "sides", "offsets", "slot", "next", "flags", "stats")]
    + [("snerf_outline_link",) + c for c in SIZES + IDS]
    + [("snerf_outline_link", {"connectivity": 6}, 1, "connectivity = 6"), ("snerf_outline_link", {"connectivity": 0}, 1, "connectivity = 0"),
       ("snerf_outline_link", {"E": -1}, 1, "E = -1"), ("snerf_outline_link", {"E": 193}, 1, "E = 193")]
    + [("snerf_outline_rank", {p: None}, 3, "null") for p in ("next", "flags", "ring", "rank", "ordinal", "totals", "workspace", "stats")]
    + [("snerf_outline_rank", {"E": -1}, 1, "E = -1"), ("snerf_outline_rank", {"E": 2 ** 31}, 1, "E = 2147483648"),
       ("snerf_outline_rank", {"workspace": 12 * DUMMY + 2}, 1, "4-byte aligned"), ("snerf_outline_rank", {"workspace_bytes": 239}, 1, "240 are needed"), ("snerf_outline_rank", {"workspace_bytes": -1}, 1, "240 are needed")]
    + [("snerf_outline_emit", {p: None}, 3, "null")
       for p in ("ids", "slot", "flags", "ring", "ordinal", "ring_row", "vertex_offset", "vertices", "rows", "stats")]
    + [("snerf_outline_emit",) + c for c in SIZES]
    + [("snerf_outline_emit", {"E": -1}, 1, "E = -1"), ("snerf_outline_emit", {"E": 193}, 1, "E = 193"),
       ("snerf_outline_emit", {"n_rings": -1}, 1, "n_rings = -1"), ("snerf_outline_emit", {"n_rings": 193}, 1, "n_rings = 193"),
       ("snerf_outline_emit", {"V": -1}, 1, "V = -1"), ("snerf_outline_emit", {"V": 193}, 1, "V = 193")]
)


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{c[0][14:]}-{n}" for n, c in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **kw)
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_the_workspace_size_and_the_empty_problem():
    """24 bytes an edge; -1 with a message beyond [0, 2^31); E = 0 is accepted by every entry that takes it, with null buffers, and
    launches nothing (there is no device here to launch on)"""
    L = _lib.lib()
    assert [L.snerf_outline_workspace_bytes(E) for E in (0, 1, 192, 2 ** 31 - 1)] == [0, 24, 4608, 24 * (2 ** 31 - 1)]
    for E in (-1, 2 ** 31):
        assert L.snerf_outline_workspace_bytes(E) == -1 and f"E = {E}" in L.snerf_last_error().decode()
        with pytest.raises(ValueError, match="snerf_outline_workspace_bytes"):
            OL.workspace_bytes(E)
    assert OL.workspace_bytes(10) == 240
    none = dict(slot=None, next=None, flags=None, ring=None, rank=None, ordinal=None, totals=None, workspace=None, workspace_bytes=0,
                ring_row=None, vertex_offset=None, vertices=None, rows=None, E=0, n_rings=0, V=0)
    for symbol in ("snerf_outline_link", "snerf_outline_rank", "snerf_outline_emit"):
        assert _call(symbol, **none)[0] == 0, symbol


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTERS)
def test_the_two_restatements_agree_bit_for_bit(name, connectivity):
    """every entry over whole arrays (the oracle of the GPU tests; the ranking round by round) against plain loops and a walk along `next`
    from each ring's lowest edge, where a corner is an edge whose predecessor has another heading"""
    ids, K = N.ids_of(name, connectivity)
    a, b = N.trace_of(name, connectivity), N.walk(ids, K, connectivity)
    for key, want in b.items():
        got = a[key]
        if isinstance(want, np.ndarray):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), key
        else:
            assert got == want, key
    E, V = a["E"], a["V"]
    assert a["link_stats"] == [0, E] and a["rank_stats"] == [0, E] and a["emit_stats"] == [0, V] and a["sides_stats"][2:] == [E, V]
    assert sorted(a["next"].tolist()) == list(range(E))                         # a permutation
    assert a["totals"][:, 0].sum() == E and a["totals"][:, 1].sum() == V


def test_ids_beyond_k_count_as_background():
    ids = np.array([[1, 7, 1], [-3, 2, 2]], np.int32)
    t = N.trace(ids, 2, 4)
    clean = N.trace(np.array([[1, 0, 1], [0, 2, 2]], np.int32), 2, 4)
    assert t["sides_stats"] == [2] + clean["sides_stats"][1:] and t["sides_stats"][1] == 4
    assert all(np.array_equal(t[k], clean[k]) for k in ("sides", "slot", "next", "flags", "ring", "rank", "vertices", "rows"))
    w = N.walk(ids, 2, 4)
    assert w["sides_stats"] == t["sides_stats"] and np.array_equal(w["vertices"], t["vertices"])


@functools.lru_cache(maxsize=None)
def _object_words(name, connectivity):
    """per object (area, min i, max i, min j, max j, perimeter) from the plain loops of tests/objects_numpy.py: (K, 6) int64"""
    ids, K = N.ids_of(name, connectivity)
    label = N.labels()[name]
    rows, _ = ON.rows_loop(ids, K, label, np.zeros(label.shape, np.float32), ground=(0,), ring=0)
    return np.array([[row[k] for k in (0, 3, 4, 5, 6, 14)] for row in rows], np.int64).reshape(K, 6)


def _per_object(obj, values, K):
    out = np.zeros(K + 1, np.int64)
    np.add.at(out, obj, values)
    return out[1:]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTERS)
def test_the_rings_against_independent_facts(name, connectivity):
    """with the ids of tests/objects_numpy.py at the same connectivity, for EVERY object of every raster: one ring of positive area; the
    rings' doubled areas add up to twice the cell count; their edges to the perimeter word; the outer ring's bounding box is the
    table's; the outer ring's corners alone give its area"""
    ids, K = N.ids_of(name, connectivity)
    r = N.rings_of(N.trace_of(name, connectivity))
    words = _object_words(name, connectivity)
    obj, area2 = r["ring_object"], r["ring_area2"]
    assert (area2 != 0).all() and ((obj >= 1) & (obj <= K)).all()
    outer = area2 > 0
    assert _per_object(obj, outer.astype(np.int64), K).tolist() == [1] * K
    cells = np.bincount(ids.reshape(-1), minlength=K + 1)[1:]
    assert np.array_equal(_per_object(obj, area2, K), 2 * cells) and np.array_equal(cells, words[:, 0])
    assert np.array_equal(_per_object(obj, r["ring_edges"], K), words[:, 5])
    outer_of = np.zeros(K + 1, np.int64)
    outer_of[obj[outer]] = np.flatnonzero(outer)
    outer_of = outer_of[1:]
    want_bbox = np.stack([words[:, 1], words[:, 2] + 1, words[:, 3], words[:, 4] + 1], 1)
    assert np.array_equal(r["ring_bbox"][outer_of].reshape(K, 4), want_bbox)
    for n, k in enumerate(outer_of.tolist(), 1):
        v = r["vertices"][r["ring_start"][k]:r["ring_start"][k + 1]].astype(np.int64)
        x, y = v[:, 0], v[:, 1]
        assert int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum()) == int(area2[k]), n


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTERS)
def test_the_holes_are_the_enclosed_components_of_the_complement(name, connectivity):
    """for EVERY object: as many rings of negative area as scipy.ndimage.label finds components of the complement, under the dual
    connectivity, that do not reach the outside -- counted on the object's bounding box with a margin of one cell, which holds every
    hole (scipy is what the check is made of: without it the test fails, it does not skip)"""
    from scipy import ndimage
    ids, K = N.ids_of(name, connectivity)
    r = N.rings_of(N.trace_of(name, connectivity))
    words = _object_words(name, connectivity)
    holes = _per_object(r["ring_object"], (r["ring_area2"] < 0).astype(np.int64), K)
    dual = ndimage.generate_binary_structure(2, 2 if connectivity == 4 else 1)
    for n in range(1, K + 1):
        _, i0, i1, j0, j1, _ = words[n - 1].tolist()
        outside = np.pad(ids[j0:j1 + 1, i0:i1 + 1] != n, 1, constant_values=True)
        assert ndimage.label(outside, structure=dual)[1] - 1 == holes[n - 1], n
    assert name != "bullseye" or holes.tolist() == [1, 0]



def test_the_hand_made_rasters():
    b = N.rings_of(N.trace_of("bullseye", 4))
    assert b["ring_object"].tolist() == [1, 1, 2] and b["ring_area2"].tolist() == [2 * 49, -2 * 25, 2] and b["ring_edges"].tolist() == [28, 20, 4]
    assert b["ring_bbox"].tolist() == [[1, 8, 1, 8], [2, 7, 2, 7], [4, 5, 4, 5]]
    assert b["vertices"][:4].tolist() == [[1, 1], [8, 1], [8, 8], [1, 8]]                       # clockwise on the screen from the north-west
    assert b["vertices"][4:8].tolist() == [[2, 2], [2, 7], [7, 7], [7, 2]]                      # the hole the other way; its lowest edge's tail (3, 2) is no corner
    s4, s8 = N.rings_of(N.trace_of("saddle", 4)), N.rings_of(N.trace_of("saddle", 8))
    assert s4["ring_area2"].tolist() == [2, 2] and s4["ring_object"].tolist() == [1, 2]
    assert s8["ring_area2"].tolist() == [4] and s8["ring_edges"].tolist() == [8]
    assert s8["vertices"].tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]      # through the shared corner twice
    assert [N.trace_of(n, 4)["E"] for n in ("row_31", "row_32")] == [64, 66] and [N.rounds(E) for E in (1, 2, 3, 64, 65, 66)] == [1, 1, 2, 6, 7, 7]
    assert N.trace_of("one_class", 4)["E"] == 640 and N.trace_of("one_class", 4)["V"] == 4 and N.trace_of("no_member", 8)["E"] == 0


def test_the_ranking_counts_what_is_no_permutation():
    """two edges that share a successor, and an index equal to E: the guard word is not 0, every output stays inside its range"""
    nxt = np.array([1, 2, 0, 1, 5, 4, 7, 6], np.int32)          # 3 -> 1 as 0 -> 1; 7 would be E - 1, 8 is E
    bad = nxt.copy()
    bad[6] = 8
    flags = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.int32)
    for case in (nxt, bad):
        ring, rank, ordinal, totals, stats = N.rank(case, flags)
        assert stats[0] > 0 or stats[1] != len(case)
        assert ((ring >= 0) & (ring < len(case))).all()
    assert N.rank(bad, flags)[4][0] > 0
    good = N.rank(np.array([1, 2, 0, 4, 3], np.int32), np.array([1, 1, 0, 1, 1], np.int32))
    assert good[0].tolist() == [0, 0, 0, 3, 3] and good[1].tolist() == [0, 1, 2, 0, 1] and good[2].tolist() == [0, 1, 2, 0, 1]
    assert good[3].tolist() == [[3, 2], [0, 0], [0, 0], [2, 2], [0, 0]] and good[4] == [0, 5]


# ---- polygons ---------------------------------------------------------------------------------------------------------------------------------
def test_polygons_order_the_outer_ring_first():
    polys = OL.polygons(N.rings_of(N.trace_of("bullseye", 4)))
    assert list(polys) == [1, 2] and [len(p) for p in polys.values()] == [2, 1]
    assert polys[1][0].tolist() == [[1, 1], [8, 1], [8, 8], [1, 8]] and polys[1][1].tolist() == [[2, 2], [2, 7], [7, 7], [7, 2]]
    assert polys[2][0].tolist() == [[4, 4], [5, 4], [5, 5], [4, 5]]
    assert OL.polygons(N.rings_of(N.trace_of("no_member", 4))) == {}


def test_polygons_refuse_ids_of_another_connectivity():
    """two cells joined at a corner are one object at connectivity 8; traced at 4 they fall into two outer rings"""
    ids, K = N.ids_of("saddle", 8)
    assert K == 1
    with pytest.raises(ValueError, match="object 1 has 2 rings of positive area: the ids are not the components of this connectivity"):
        OL.polygons(N.rings_of(N.trace(ids, K, 4)))
    assert len(OL.polygons(N.rings_of(N.trace(ids, K, 8)))[1]) == 1


def _seg_dist2(p, a, b):
    """brute force, independent of the module: the squared distance of p from the segment a b as a Fraction"""
    (px, py), (ax, ay), (bx, by) = p, a, b
    dx, dy = bx - ax, by - ay
    if dx == 0 and dy == 0:
        return Fraction((px - ax) ** 2 + (py - ay) ** 2)
    t = Fraction((px - ax) * dx + (py - ay) * dy, dx * dx + dy * dy)
    t = min(max(t, Fraction(0)), Fraction(1))
    return (px - ax - t * dx) ** 2 + (py - ay - t * dy) ** 2


def _within(dropped, kept, t):
    closed = kept + kept[:1]
    return all(min(_seg_dist2(p, a, b) for a, b in zip(closed, closed[1:])) <= t * t for p in dropped)


def test_simplify_leaves_a_rectangle_alone():
    """4 corners, short side 6: the corner off the diagonal lies 6 * 17 / sqrt(6^2 + 17^2) = 5.66 cells from it, above any tolerance
    below half the short side"""
    ids = np.zeros((12, 25), np.int32)
    ids[3:9, 4:21] = 1
    polys = OL.polygons(N.rings_of(N.trace(ids, 1, 4)))
    assert polys[1][0].tolist() == [[4, 3], [21, 3], [21, 9], [4, 9]]
    for tol in (0, 0.5, 1, Fraction(5, 2), 2.999):
        out = OL.simplify(polys, tol)
        assert list(out) == [1] and len(out[1]) == 1 and out[1][0].tolist() == polys[1][0].tolist(), tol
    assert OL.simplify(polys, 0) is polys
    with pytest.raises(ValueError, match="negative"):
        OL.simplify(polys, -1)


def test_simplify_takes_the_staircase_off_a_diamond():
    """|i - c| + |j - c| <= r: 8 r + 4 corners, the concave ones 1 / sqrt(2) cells inside the line through the convex ones.  At one cell
    no concave corner survives and at most the two corners of each tip do; every dropped corner lies within the cell of what is kept"""
    r, c = 9, 10
    jj, ii = np.mgrid[0:21, 0:21]
    ids = (np.abs(ii - c) + np.abs(jj - c) <= r).astype(np.int32)
    polys = OL.polygons(N.rings_of(N.trace(ids, 1, 4)))
    ring = [tuple(v) for v in polys[1][0].tolist()]
    assert len(ring) == 8 * r + 4
    out = [tuple(v) for v in OL.simplify(polys, 1)[1][0].tolist()]
    tips = {(c, c - r), (c + 1, c - r), (c + r + 1, c), (c + r + 1, c + 1), (c + 1, c + r + 1), (c, c + r + 1), (c - r, c + 1), (c - r, c)}
    assert 4 <= len(out) <= 8 and set(out) <= tips and out[0] == ring[0]
    assert [p for p in ring if p in out] == out                                     # a subsequence: the order is the ring's
    assert _within([p for p in ring if p not in out], out, Fraction(1))
    x, y = np.array(out)[:, 0], np.array(out)[:, 1]
    area2 = int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())
    assert 0 < area2 and abs(area2 - 2 * int(ids.sum())) <= 2 * (8 * r + 4)        # within a cell-wide band along the outline


@pytest.mark.parametrize("tol", [Fraction(1, 2), 1, Fraction(3, 2), 2.25])
def test_simplify_keeps_every_dropped_vertex_within_the_tolerance(tol):
    """every ring of the random 33 x 64 raster at connectivity 8 (321 rings, holes and pinched rings among them), each as a polygon of
    its own: the kept vertices are a subsequence that starts at the ring's first vertex, and every dropped one lies within `tol` of the
    kept closed chain -- by brute force over all kept segments, in exact fractions.  A condition, not a measurement."""
    polys = OL.polygons(N.rings_of(N.trace_of("random_33x64", 8)))
    rings = [ring for ring_list in polys.values() for ring in ring_list]
    assert len(rings) == 321
    t, fewer = Fraction(tol), 0
    for k, ring in enumerate(rings):
        pts = [tuple(v) for v in ring.tolist()]
        kept = [tuple(v) for v in OL.simplify({1: [ring]}, tol)[1][0].tolist()]
        rest = iter(pts)
        assert kept[0] == pts[0] and len(kept) >= 3 and all(p in rest for p in kept), k           # `in` consumes: a subsequence
        assert _within([p for p in pts if p not in kept], kept, t), k
        fewer += len(pts) - len(kept)
    assert fewer > 0


def test_simplify_drops_a_hole_and_keeps_an_outer_ring_that_collapse():
    """the bullseye at 4 cells: the 7 x 7 outer ring stays (its off-diagonal corners lie 4.95 cells from the diagonal), the 5 x 5 hole
    (3.54) falls to 2 vertices and is dropped, the single cell falls to 2 as well and is kept as it was"""
    polys = OL.polygons(N.rings_of(N.trace_of("bullseye", 4)))
    out = OL.simplify(polys, 4)
    assert list(out) == [1, 2] and [len(v) for v in out.values()] == [1, 1]
    assert out[1][0].tolist() == polys[1][0].tolist() and out[2][0].tolist() == polys[2][0].tolist() == [[4, 4], [5, 4], [5, 5], [4, 5]]
    assert [len(v) for v in OL.simplify(polys, 3.5).values()] == [2, 1]


# ---- map coordinates and GeoJSON ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _town():
    label, alt, boxes = ON.town()
    parent, _ = ON.link(label, (3, 4), 4)
    ids, K = ON.ids_of(parent, *label.shape)
    rows, _ = ON.rows_loop(ids, K, label, alt, ground=(0,), ring=2)
    table = OB.object_table(ON.words(rows), GRID)
    return ids, K, table, boxes


def test_the_town_in_map_coordinates():
    """four boxes: every footprint is the 4 corners of the object table's bounding box, from the north-west corner in the tracing order
    (clockwise on the north-up map)"""
    ids, K, table, boxes = _town()
    assert K == 4
    polys = OL.to_map(OL.polygons(N.rings_of(N.trace(ids, K, 4))), GRID)
    assert list(polys) == [1, 2, 3, 4]
    for n, ring_list in polys.items():
        e0, n0, e1, n1 = table["bbox"][n - 1]
        assert len(ring_list) == 1 and ring_list[0].dtype == np.float64
        assert ring_list[0].tolist() == [[e0, n1], [e1, n1], [e1, n0], [e0, n0]], n
    j0, i0, nj, ni, _ = boxes[0]
    assert polys[1][0][0].tolist() == [GRID.xoff + i0 * 0.5, GRID.yoff - j0 * 0.5]
    # a window of a larger lattice gives the same coordinates through its offsets
    window = D.grid_struct(D.DsmGrid(GRID.xoff - 10 * 0.5, GRID.yoff + 4 * 0.5, 0.5, 200, 150), (10, 4, 130, 96))
    again = OL.to_map(OL.polygons(N.rings_of(N.trace(ids, K, 4))), window)
    assert all(np.array_equal(again[n][0], polys[n][0]) for n in polys)


def _shoelace(ring):
    a = np.asarray(ring, np.float64)
    x, y = a[:, 0] - a[0, 0], a[:, 1] - a[0, 1]
    return 0.5 * float((x[:-1] * y[1:] - x[1:] * y[:-1]).sum())


def test_geojson_is_a_feature_collection():
    ids, K, table, _ = _town()
    polys = OL.polygons(N.rings_of(N.trace(ids, K, 4)))
    doc = json.loads(json.dumps(OL.geojson(polys, GRID, "17R", OB.table_records(table))))
    assert doc["type"] == "FeatureCollection" and doc["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::32617"}}
    assert [f["id"] for f in doc["features"]] == [1, 2, 3, 4] == [f["properties"]["id"] for f in doc["features"]]
    for f, rec in zip(doc["features"], json.loads(json.dumps(OB.table_records(table)))):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and f["properties"] == rec
        rings = f["geometry"]["coordinates"]
        assert all(r[0] == r[-1] and len(r) >= 4 for r in rings)
        assert _shoelace(rings[0]) == rec["area_m2"] > 0                                  # counter-clockwise in (east, north); exact here
        e0, n0, e1, n1 = rec["bbox"]
        assert rings[0] == [[e0, n1], [e0, n0], [e1, n0], [e1, n1], [e0, n1]]              # the traced ring from its first vertex, reversed
    assert "crs" not in OL.geojson(polys, GRID) and OL.geojson(polys, GRID)["features"][2]["properties"] == {"id": 3}
    assert json.loads(json.dumps(OL.geojson({}, GRID, "17R")))["features"] == []
    # holes run the other way, and the southern hemisphere has its own codes
    b = OL.geojson(OL.polygons(N.rings_of(N.trace_of("bullseye", 4))), D.DsmGrid(0.0, 100.0, 2.0, 10, 9), "21H")
    assert b["crs"]["properties"]["name"] == "urn:ogc:def:crs:EPSG::32721"
    outer, hole = b["features"][0]["geometry"]["coordinates"]
    assert _shoelace(outer) == 49 * 4.0 and _shoelace(hole) == -25 * 4.0 and outer[0] == [2.0, 98.0]


def test_the_exports_grew_at_the_end_and_default_to_no_polygons():
    import inspect
    from snerf_amd.eval import ortho as EO
    p = inspect.signature(EO.export_objects).parameters
    assert p["polygons"].default is False and p["simplify_m"].default == 0.0 and list(p)[-3:] == ["polygons", "simplify_m", "kwargs"]
    # export_roofs keeps its pinned parameter list (tests/test_roofs_cpu.py): it takes the two keywords out of **kwargs, before any
    # device work -- a host tensor is still the first thing it refuses, with or without them
    assert list(inspect.signature(EO.export_roofs).parameters) == ["products", "objects_result", "output_dp", "alt_key", "reference", "zone_string",
                                                                   "kwargs"]
    import torch
    products = {"dsm": torch.zeros((4, 5)), "grid": D.DsmGrid(0.0, 0.0, 0.5, 5, 4)}
    objects = {"ids": torch.zeros((4, 5), dtype=torch.int32), "n": 0, "table": {"area_cells": np.zeros(0), "ground_alt": np.zeros(0)}}
    for kw in ({}, {"polygons": True, "simplify_m": 1.0}):
        with pytest.raises(ValueError, match="alt must be a GPU tensor"):
            EO.export_roofs(products, objects, "unused", **kw)
