"""CPU-side checks of the objects on the map (include/snerf_objects.h, csrc/objects.hip, eval/utils/objects.py):
the new header's prototypes and constant against the binding (_lib.HEADER_SIGNATURES), the restatement's labelling
(tests/objects_numpy.py, the oracle of tests/test_gpu_objects.py) against scipy.ndimage.label, the table arithmetic on hand-made
rows, the matching and the scores on CPU tensors, and every refusal of the two entries through the binding (none reaches a launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB           # the feature under test: every test of this file needs it
from tests import objects_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_objects.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_objects_link": ["label", "h", "w", "member_host", "connectivity", "parent", "stats", "stream"],
    "snerf_objects_stats": ["ids", "label", "alt", "h", "w", "K", "ground_host", "ring", "z0", "q", "row0", "row1", "rows", "stats",
                            "stream"],
}


def test_the_new_header_matches_its_binding_rows():
    """include/snerf_objects.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py), then the constants; the main header, the
    main table, the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_objects.h", NAMES)
    text = open(HEADER).read()
    assert int(re.search(r"#define SNERF_OBJECTS_ROW_WORDS (\d+)", text).group(1)) == _lib.OBJECTS_ROW_WORDS == OB.ROW_WORDS == N.ROW_WORDS == 16
    assert OB.MAX_RING == _lib.ORTHO_MAX_RADIUS == 7 and OB.NO_LABEL == N.NO_LABEL == 255
    # the initial row words of the header's table, in the host layer (int64 holding the u64) and in the restatement
    assert [v % 2 ** 64 for v in OB._ROW_INIT] == N.ROW_INIT and len(N.ROW_INIT) == 16


# ---- the restatement's labelling against scipy ------------------------------------------------------------------------------------------
def _rasters():
    out = {f"random_{h}x{w}": N.random_label(h, w) for h, w in N.RANDOM_SHAPES}
    out.update(N.structured())
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_restatement_labels_as_scipy_does(connectivity):
    """for every participating class and both connectivities: the same partition as scipy.ndimage.label, every root the minimum
    index of its component, -1 exactly off the classes"""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for name, label in _rasters().items():
        h, w = label.shape
        parent, stats = N.link(label, (3, 4), connectivity)
        assert stats == [0, int(np.isin(label, (3, 4)).sum())], name
        assert np.array_equal(parent < 0, ~np.isin(label, (3, 4)).reshape(-1)), name
        n_roots = 0
        for cls in (3, 4):
            want, n = ndimage.label(label == cls, structure=structure)
            want = want.reshape(-1)
            n_roots += n
            for k in range(1, n + 1):
                cells = np.flatnonzero(want == k)
                assert (parent[cells] == cells.min()).all(), (name, cls, k)
        ids, K = N.ids_of(parent, h, w)
        assert K == n_roots and ids.max(initial=0) == K and np.array_equal(ids.reshape(-1) > 0, parent >= 0), name
        roots = np.flatnonzero(parent == np.arange(h * w))
        assert np.array_equal(ids.reshape(-1)[roots], np.arange(1, K + 1)), name      # the raster order of the roots


def test_the_structured_rasters_are_what_their_names_say():
    count = lambda label, c: N.ids_of(N.link(label, (3, 4), c)[0], *label.shape)[1]      # noqa: E731
    s = N.structured()
    assert s["serpentine"].shape == (33, 67) and count(s["serpentine"], 4) == count(s["serpentine"], 8) == 1
    assert s["checkerboard"].shape == (16, 70) and count(s["checkerboard"], 4) == 560 and count(s["checkerboard"], 8) == 1
    assert s["spiral"].shape == (65, 65) and count(s["spiral"], 4) == 1 and int((s["spiral"] == 3).sum()) > 1500
    assert s["one_class"].shape == (64, 256) and count(s["one_class"], 4) == 1
    assert s["comb"].shape == (40, 129) and count(s["comb"], 4) == 1 and count(s["comb"][:-1], 4) == 65
    assert count(s["alternating_columns"], 4) == count(s["alternating_columns"], 8) == 66        # two classes are never merged
    assert count(s["no_member"], 8) == 0
    parent, _ = N.link(s["serpentine"], (4,), 4)                                                 # class 3 takes no part: nothing
    assert (parent == -1).all()


def test_ids_from_parent_is_the_restatements():
    label = N.random_label(33, 64)
    parent, _ = N.link(label, (3, 4), 8)
    want, K = N.ids_of(parent, 33, 64)
    got, k = OB.ids_from_parent(torch.from_numpy(parent), 33, 64)
    assert k == K and got.dtype == torch.int32 and np.array_equal(got.numpy(), want)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_object_table_on_hand_made_rows():
    """a 3 x 2-cell object (3 columns, 2 rows) at columns 4..6, rows 1..2 of a sub-window at res = 0.5, with negative k"""
    q, bias = OB.OR.Q, 2 ** 31
    ks = [-3 * 65536, -3 * 65536, -2 * 65536, -3 * 65536, -3 * 65536, -4 * 65536]            # altitudes -3, -3, -2, -3, -3, -4 m
    ring_k = [-10 * 65536] * 7 + [-17 * 65536]                                              # 8 ring pairs: mean -10.875, min -17
    row = [6, 2 * (4 + 5 + 6), 3 * (1 + 2), 4, 6, 1, 2, 6, sum(ks), min(ks) + bias, max(ks) + bias, 8, sum(ring_k), min(ring_k) + bias, 10, 3]
    holes = [2, 0, 0, 0, 1, 0, 0, 0, 0, 2 ** 64 - 1, 0, 0, 0, 2 ** 64 - 1, 6, 4]               # two cells, no altitude, no ring pair
    rows = N.words([row, holes])
    grid = D.grid_struct(D.DsmGrid(1000.0, 2000.0, 0.5, 40, 30), (10, 20, 12, 8))             # the window starts at column 10, row 20
    t = OB.object_table(torch.from_numpy(rows.view(np.int64)), grid)
    assert t["class"].tolist() == [3, 4] and t["area_cells"].tolist() == [6, 2] and t["holes"].tolist() == [0, 2]
    assert t["area_m2"].tolist() == [1.5, 0.5] and t["perimeter_m"].tolist() == [5.0, 3.0]
    x0, y0 = 1000.0 + 10 * 0.5, 2000.0 - 20 * 0.5
    assert t["east"][0] == x0 + 5.5 * 0.5 and t["north"][0] == y0 - 2.0 * 0.5
    assert t["bbox"][0].tolist() == [x0 + 4 * 0.5, y0 - 3 * 0.5, x0 + 7 * 0.5, y0 - 1 * 0.5]
    assert (t["alt_mean"][0], t["alt_min"][0], t["alt_max"][0]) == (-3.0, -4.0, -2.0)
    assert (t["ground_alt"][0], t["ground_min"][0]) == (-10.875, -17.0)
    assert (t["height"][0], t["height_max"][0]) == (7.875, 8.875)
    assert t["volume_m3"][0] == (q * sum(ks) + 6 * 10.875) * 0.25 == 6 * 0.25 * 7.875
    for key in ("alt_mean", "alt_min", "alt_max", "ground_alt", "ground_min", "height", "height_max", "volume_m3"):
        assert math.isnan(t[key][1]), key
    # a DsmGrid is taken as it is
    t2 = OB.object_table(rows.view(np.int64), D.DsmGrid(x0, y0, 0.5, 12, 8))
    assert all(np.array_equal(t[k], t2[k], equal_nan=True) for k in t)
    ids = torch.tensor([[0, 1, 1], [2, 2, 0]], dtype=torch.int32)
    kept_ids, kept = OB.filter_objects(ids, t, min_area_m2=1.0)
    assert kept_ids.tolist() == [[0, 1, 1], [0, 0, 0]] and kept["class"].tolist() == [3] and kept_ids.dtype == torch.int32
    kept_ids, kept = OB.filter_objects(ids, {k: v[::-1] for k, v in t.items()}, min_area_m2=1.0)      # object 2 is the large one now
    assert kept_ids.tolist() == [[0, 0, 0], [1, 1, 0]] and kept["class"].tolist() == [3]
    recs = OB.table_records(t)
    assert recs[0]["id"] == 1 and recs[0]["height"] == 7.875 and recs[1]["height"] is None and recs[1]["bbox"][0] == t["bbox"][1, 0]


# ---- matching and scores ----------------------------------------------------------------------------------------------------------------
def _box_map(boxes, h=40, w=60):
    """boxes [(j0, i0, rows, cols)] -> (ids int32 tensor, n) in the order given (which is their raster order here)"""
    ids = torch.zeros((h, w), dtype=torch.int32)
    for k, (j0, i0, nj, ni) in enumerate(boxes):
        ids[j0:j0 + nj, i0:i0 + ni] = k + 1
    return ids, len(boxes)


def _table(classes, heights, areas):
    return {"class": np.array(classes, np.int64), "height": np.array(heights, np.float64), "area_cells": np.array(areas, np.int64)}


def test_matching_and_scores():
    a, n_a = _box_map([(5, 5, 10, 10), (25, 30, 6, 8)])
    ta = _table([3, 3], [6.0, 9.0], [100, 48])
    pairs, inter, union = OB.match_objects(a, n_a, a, n_a)
    assert pairs.tolist() == [[1, 1], [2, 2]] and inter.tolist() == union.tolist() == [100, 48]
    s = OB.object_scores(ta, ta, pairs, inter, union)
    assert (s["n_a"], s["n_b"], s["matched"], s["precision"], s["recall"], s["f1"], s["iou_mean"]) == (2, 2, 2, 1.0, 1.0, 1.0, 1.0)
    assert (s["height_mae"], s["height_median_abs"], s["height_bias"], s["area_ratio_mean"]) == (0.0, 0.0, 0.0, 1.0)
    assert s["class_confusions"] == [] and s["per_class"] == {3: {"n_a": 2, "n_b": 2, "matched": 2, "precision": 1.0, "recall": 1.0, "f1": 1.0}}
    # shifted by 2 columns: IoU 80 / 120 matches; by 4 columns: 60 / 140 does not
    b2, _ = _box_map([(5, 7, 10, 10)])
    pairs, inter, union = OB.match_objects(a, n_a, b2, 1)
    assert pairs.tolist() == [[1, 1]] and inter.tolist() == [80] and union.tolist() == [120]
    s = OB.object_scores(ta, _table([3], [7.5], [100]), pairs, inter, union)
    assert (s["matched"], s["precision"], s["recall"]) == (1, 0.5, 1.0) and s["f1"] == 2 * 0.5 / 1.5 and s["iou_mean"] == 80 / 120
    assert (s["height_mae"], s["height_bias"], s["height_median_abs"]) == (1.5, -1.5, 1.5)
    b4, _ = _box_map([(5, 9, 10, 10)])
    pairs, inter, union = OB.match_objects(a, n_a, b4, 1)
    assert pairs.shape == (0, 2) and inter.numel() == union.numel() == 0
    s = OB.object_scores(ta, _table([3], [7.5], [100]), pairs, inter, union)
    assert (s["matched"], s["precision"], s["recall"], s["f1"], s["iou_mean"], s["height_mae"]) == (0, 0.0, 0.0, 0.0, None, None)
    # a class mismatch is reported and does not count; a NaN height leaves the height figures
    pairs, inter, union = OB.match_objects(a, n_a, a, n_a)
    s = OB.object_scores(ta, _table([3, 4], [math.nan, 9.0], [100, 48]), pairs, inter, union)
    assert s["matched"] == 1 and s["class_confusions"] == [{"a": 2, "b": 2, "class_a": 3, "class_b": 4}]
    assert s["height_pairs"] == 0 and s["height_mae"] is None and s["iou_mean"] == 1.0
    assert s["per_class"][3] == {"n_a": 2, "n_b": 1, "matched": 1, "precision": 0.5, "recall": 1.0, "f1": 2 * 0.5 / 1.5}
    assert s["per_class"][4] == {"n_a": 0, "n_b": 1, "matched": 0, "precision": 0.0, "recall": 0.0, "f1": 0.0}
    # an empty side: no division error
    none, _ = _box_map([])
    empty = _table([], [], [])
    for ids_a, na, tab_a, ids_b, nb, tab_b in ((none, 0, empty, a, n_a, ta), (a, n_a, ta, none, 0, empty), (none, 0, empty, none, 0, empty)):
        pairs, inter, union = OB.match_objects(ids_a, na, ids_b, nb)
        s = OB.object_scores(tab_a, tab_b, pairs, inter, union)
        assert pairs.shape == (0, 2) and (s["matched"], s["precision"], s["recall"], s["f1"]) == (0, 0.0, 0.0, 0.0) and s["per_class"].keys() <= {3}
    with pytest.raises(ValueError, match=r"\(40, 60\) and \(40, 61\)"):
        OB.match_objects(a, n_a, torch.zeros((40, 61), dtype=torch.int32), 0)


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
def _classes(*cs):
    t = (C.c_ubyte * 256)()
    for c in cs:
        t[c] = 1
    return t


def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(label=DUMMY, h=3, w=4, member_host=_classes(3), connectivity=4, parent=DUMMY, stats=DUMMY, ids=DUMMY, alt=DUMMY, K=2,
             ground_host=_classes(0), ring=2, z0=0.0, q=2.0 ** -16, row0=0, row1=3, rows=DUMMY)
    a.update(kw)
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


SIZE_REFUSALS = [
    ({"label": None}, 3, "null"), ({"stats": None}, 3, "null"),
    ({"h": 0}, 1, "h = 0"), ({"w": 0}, 1, "w = 0"), ({"h": -5}, 1, "h = -5"), ({"h": 32768, "w": 65536}, 1, "below 2^31"),
    ({"h": 2 ** 31 - 1, "w": 2 ** 31 - 1}, 1, "below 2^31"),
]
LINK_REFUSALS = [
    ({"member_host": None}, 3, "null"), ({"parent": None}, 3, "null"),
    ({"connectivity": 3}, 1, "connectivity = 3"), ({"connectivity": 0}, 1, "connectivity = 0"), ({"connectivity": 6}, 1, "connectivity = 6"),
    ({"member_host": _classes(3, 255)}, 1, "member_host[255]"),
]
STATS_REFUSALS = [
    ({"ids": None}, 3, "null"), ({"alt": None}, 3, "null"), ({"ground_host": None}, 3, "null"), ({"rows": None}, 3, "null"),
    ({"K": -1}, 1, "K = -1"), ({"K": 2 ** 31}, 1, "K = 2147483648"),
    ({"ring": 8}, 1, "ring = 8"), ({"ring": -1}, 1, "ring = -1"),
    ({"h": 20000, "w": 20000, "ring": 2, "row1": 3}, 1, "below 2^32"), ({"h": 46340, "w": 46340, "ring": 1, "row1": 3}, 1, "below 2^32"),
    ({"row0": -1}, 1, "row0 = -1"), ({"row1": 4}, 1, "row1 = 4"), ({"row0": 2, "row1": 1}, 1, "row0 = 2"),
    ({"q": 0.0}, 1, "q > 0"), ({"q": -1.0}, 1, "q > 0"), ({"q": math.inf}, 1, "q > 0"), ({"q": math.nan}, 1, "q > 0"),
    ({"z0": math.nan}, 1, "z0 finite"), ({"z0": math.inf}, 1, "z0 finite"),
    ({"ground_host": _classes(0, 255)}, 1, "ground_host[255]"),
    ({"K": 0, "ring": 9}, 1, "ring = 9"),                                 # an empty problem does not excuse a bad argument
]
CASES = ([("snerf_objects_link", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + LINK_REFUSALS]
         + [("snerf_objects_stats", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + STATS_REFUSALS])


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{s[14:]}-{n}" for n, (s, _, _, _) in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **dict(kw))
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_an_empty_problem_is_accepted_and_launches_nothing():
    """K == 0 or an empty band with good arguments returns SNERF_OK before the launch: the dummy addresses are never handed to a
    kernel, and no GPU is needed for it"""
    assert _call("snerf_objects_stats", K=0)[0] == 0 and _call("snerf_objects_stats", K=0, rows=None)[0] == 0
    assert _call("snerf_objects_stats", row0=2, row1=2)[0] == 0
    assert _call("snerf_objects_stats", h=20000, w=20000, ring=1, K=0)[0] == 0          # 3.6e9 pairs: below the bound


def test_python_refusals():
    label = torch.zeros((3, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="label must be a GPU tensor"):
        OB.components(label, (3,))
    with pytest.raises(ValueError, match="ids must be a GPU tensor"):
        OB.object_rows(torch.zeros((3, 4), dtype=torch.int32), 1, label, torch.zeros(3, 4), (0,))
    for bad in ((255,), (-1,), (256,), (2.5,)):
        with pytest.raises(ValueError, match="class ids in"):
            OB.class_table(bad)
    assert list(OB.class_table((0, 3, 254))).count(1) == 3 and OB.class_table((3,))[3] == 1
    assert OB.new_rows(2, "cpu").tolist() == [list(OB._ROW_INIT)] * 2 and OB.new_rows(0, "cpu").shape == (0, 16)
