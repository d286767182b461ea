"""CPU-side checks of the bare-earth terrain (include/snerf_terrain.h, csrc/terrain.hip, eval/utils/terrain.py):
the new header's prototypes and constants against the binding (_lib.HEADER_SIGNATURES), the restatement's opening
(tests/terrain_numpy.py, the oracle of tests/test_gpu_terrain.py) against scipy.ndimage and against a brute-force loop, the schedule
on hand-computed values, the synthetic town's exact properties, terrain_agreement on hand-made tensors, the objects' tables without a
DTM, and every refusal of the four entries through the binding (none reaches a launch)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import terrain as TR          # the feature under test: every test of this file needs it
from tests import terrain_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_terrain.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_terrain_workspace_bytes": ["h", "w"],
    "snerf_terrain_keys": ["alt", "label", "h", "w", "blocked_host", "z0", "q", "key", "flags", "stats", "stream"],
    "snerf_terrain_open": ["key_in", "h", "w", "radius", "threshold", "key_out", "flags", "ws", "stats", "stream"],
    "snerf_terrain_fill": ["key", "flags", "alt", "h", "w", "z0", "q", "dtm", "ndsm", "reach", "ws", "stats", "stream"],
}


def test_the_new_header_matches_its_binding_rows():
    """include/snerf_terrain.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py), then the constants; the main header, the
    main table, the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_terrain.h", NAMES, returns={"snerf_terrain_workspace_bytes": ("int", 8, True)})
    text = open(HEADER).read()
    consts = {k: v for k, v in re.findall(r"#define (SNERF_TERRAIN_\w+) (\(?-?[\d \-]+\)?)", text)}
    assert eval(consts["SNERF_TERRAIN_HOLE"]) == _lib.TERRAIN_HOLE == TR.HOLE == N.HOLE == -2 ** 31
    assert int(consts["SNERF_TERRAIN_MAX_RADIUS"]) == _lib.TERRAIN_MAX_RADIUS == TR.MAX_RADIUS == 512
    assert (int(consts["SNERF_TERRAIN_FLAGGED"]), int(consts["SNERF_TERRAIN_BLOCKED"]), int(consts["SNERF_TERRAIN_IS_HOLE"])) == \
        (_lib.TERRAIN_FLAGGED, _lib.TERRAIN_BLOCKED, _lib.TERRAIN_IS_HOLE) == (N.FLAGGED, N.BLOCKED, N.IS_HOLE) == (1, 2, 4)
    assert (N.Z0, N.Q) == (TR.OR.Z0, TR.OR.Q)
    assert _lib.lib().snerf_terrain_workspace_bytes(70, 129) == 16 * 70 * 129 and _lib.lib().snerf_terrain_workspace_bytes(1, 1) == 16


# ---- the restatement's opening ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3, 7, 40])
def test_the_restatements_opening_is_scipys_on_hole_free_rasters(radius):
    """grey_erosion then grey_dilation with a flat square, mode="constant" with a cval beyond the keys: the window clipped to the
    raster.  Radius 40 is larger than the 33-row raster."""
    ndimage = pytest.importorskip("scipy.ndimage")
    size = (2 * radius + 1, 2 * radius + 1)
    for h, w in N.SHAPES[:6]:
        key = N.key_raster(h, w, "none").astype(np.int64)
        e = ndimage.grey_erosion(key, size=size, mode="constant", cval=2 ** 40)
        want = ndimage.grey_dilation(e, size=size, mode="constant", cval=-2 ** 40)
        got, flags, n = N.open_level(key.astype(np.int32), radius)
        assert flags is None and n == 0 and got.dtype == np.int32 and np.array_equal(got, want), (h, w)
        assert np.array_equal(N.erode(key.astype(np.int32), radius), e), (h, w)


@pytest.mark.parametrize("pattern", N.HOLE_PATTERNS)
def test_with_holes_the_opening_is_the_brute_force_loops(pattern):
    for (h, w), radii in (((7, 65), (1, 3, 40)), ((1, 130), (2,)), ((33, 64), (7,)), ((1, 1), (1,))):
        key = N.key_raster(h, w, pattern)
        if pattern == "random":
            key.reshape(-1)[::11] = N.NOT_A_KEY                       # 2^31 - 1 is no key: read as a hole, stored back as the hole
        for r in radii:
            got, _, _ = N.open_level(key, r)
            assert np.array_equal(got, N.open_brute(key, r)), (h, w, r)
            assert np.array_equal(got == N.HOLE, ~N.valid(key)) and (got[N.valid(key)] <= key[N.valid(key)]).all()


def test_the_flag_update_of_the_restatement():
    key = np.array([[10, 10, 50, 10, 10, N.HOLE, 10]], np.int32)
    flags = np.array([[0, 2, 0, 0, 1, 4, 0]], np.uint8)
    out, f, n = N.open_level(key, 1, 39, flags)
    assert out.tolist() == [[10, 10, 10, 10, 10, N.HOLE, 10]] and f.tolist() == [[0, 2, 1, 0, 1, 4, 0]] and n == 1
    assert N.open_level(key, 1, 40, flags)[1].tolist() == flags.tolist()          # strictly above the threshold only
    pre = np.array([[0, 2, 1, 0, 1, 4, 0]], np.uint8)
    assert N.open_level(key, 1, 0, pre)[2] == 0                                    # already flagged: not newly


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------
def test_schedule_on_hand_computed_values():
    # r_max = ceil(12.5 / 0.5 / 2) = 13; steps 1, 1, 2, 4, 5 cells -> 0.45, 0.45, 0.6, 0.9, 1.05 m -> x 65536, rounded
    assert TR.schedule(0.5, max_window_m=12.5, slope=0.3, dh0=0.3, dh_max=2.5) == ([1, 2, 4, 8, 13], [29491, 29491, 39322, 58982, 68813])
    assert N.schedule(0.5, **N.TOWN_SCHEDULE) == TR.schedule(0.5, **N.TOWN_SCHEDULE)
    # the defaults at 0.5 m: r_max = 80; the steps 1, 1, 2, 4, 8, 16, 32, 16 -> 0.375, 0.375, 0.45, 0.6, 0.9, 1.5, 2.5 (capped), 1.5
    radii, thresholds = TR.schedule(0.5)
    assert radii == [1, 2, 4, 8, 16, 32, 64, 80] and thresholds == [24576, 24576, 29491, 39322, 58982, 98304, 163840, 98304]
    assert all(type(v) is int for v in radii + thresholds)
    assert TR.schedule(1.0, max_window_m=16.0)[0] == [1, 2, 4, 8]                  # r_max a power of two: once
    assert TR.schedule(1.0, max_window_m=1.0)[0] == [1] and TR.schedule(2.0, max_window_m=6.0)[0] == [1, 2]
    assert TR.schedule(1.0, max_window_m=1024.0)[0][-1] == 512
    with pytest.raises(ValueError, match="512"):
        TR.schedule(1.0, max_window_m=1026.0)
    with pytest.raises(ValueError, match="positive and finite"):
        TR.schedule(0.0)


# ---- the town -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.0, 0.05, 0.1])
def test_the_town(slope):
    """the schedule max_window_m = 12.5, slope = 0.3, dh0 = 0.3, dh_max = 2.5 (radii 1, 2, 4, 8, 13) on the 12 boxes.  The cells that
    are not ground are EXACTLY the boxes.  Flat: the DTM has the ground's bits everywhere, the nDSM is +0 off the boxes.  Sloped: every
    row or column pair of ground cells interpolates a plane exactly, so only the quantisation is left: the DTM lies within q of the
    plane's quantised altitude (measured in the restatement: 1.24e-5 m at both slopes; q = 1.53e-5 m)."""
    alt, boxes, ground, mask = N.town(slope)
    assert alt.shape == N.TOWN_SHAPE and len(boxes) == 12 and mask.sum() == sum(b[2] * b[3] for b in boxes)
    for j0, i0, nj, ni, roof in boxes:
        assert 4 <= nj <= 19 and 4 <= ni <= 19 and j0 >= 1 and i0 >= 1 and j0 + nj <= 69 and i0 + ni <= 128
        assert 3.0 <= round(roof - ground[j0:j0 + nj, i0:i0 + ni].max(), 9) <= 15.0       # whole metres, up to the sum's rounding
    out = N.terrain(alt, N.TOWN_RES, **N.TOWN_SCHEDULE)
    assert out["schedule"]["radii"] == [1, 2, 4, 8, 13]
    assert np.array_equal(~out["ground"], mask)
    s = out["stats"]
    assert (s["unreachable"], s["filled"], s["ground"]) == (0, int(mask.sum()), int((~mask).sum())) and sum(s["flagged_per_level"]) == mask.sum()
    assert (out["reach"][mask] >= 1).all() and (out["reach"][~mask] == 0).all()
    plane32 = ground.astype(np.float32)
    if slope == 0.0:
        assert np.array_equal(out["dtm"].view(np.uint32), plane32.view(np.uint32))
        assert (out["ndsm"][~mask].view(np.uint32) == 0).all()
        for j0, i0, nj, ni, roof in boxes:
            assert (out["ndsm"][j0:j0 + nj, i0:i0 + ni] == np.float32(roof - 10.0)).all()
    else:
        quantised = N.Z0 + N.Q * np.rint((plane32.astype(np.float64) - N.Z0) / N.Q)
        err = np.abs(out["dtm"].astype(np.float64) - quantised).max()
        print(f"slope {slope}: max |dtm - quantised plane| = {err:.3e} m (q = {N.Q:.3e})")
        assert err < N.Q
        assert np.array_equal(out["dtm"][~mask].view(np.uint32), plane32[~mask].view(np.uint32))


# ---- terrain_agreement ------------------------------------------------------------------------------------------------------------------
def test_terrain_agreement_on_hand_made_tensors():
    nan = math.nan
    a = {"dtm": torch.tensor([[1.0, 2.0, 3.0], [nan, 5.0, 6.0]]), "ndsm": torch.tensor([[0.0, 1.0, nan], [0.0, 2.0, 0.0]]),
         "ground": torch.tensor([[True, False, True], [True, False, True]])}
    b = {"dtm": torch.tensor([[1.5, 2.0, 2.0], [4.0, nan, 6.0]]), "ndsm": torch.tensor([[0.0, 3.0, 0.0], [0.0, 2.0, 0.5]]),
         "ground": torch.tensor([[True, True, False], [True, False, False]])}
    s = TR.terrain_agreement(a, b)             # the cells (0,0), (0,1), (0,2), (1,2): differences -0.5, 0, 1, 0
    assert s["cells"] == 4 and s["dtm_mae"] == 0.375 and s["dtm_bias"] == 0.125 and s["dtm_median_abs"] == 0.0
    assert s["ndsm_cells"] == 3 and s["ndsm_mae"] == (0.0 + 2.0 + 0.5) / 3
    assert s["ground_table"] == [[1, 2], [1, 0]] and s["ground_accuracy"] == 0.25 and s["ground_iou"] == 0.25
    assert all(type(v) is int for row in s["ground_table"] for v in row)
    same = TR.terrain_agreement(a, a)
    assert same["cells"] == 5 and same["dtm_mae"] == 0.0 and same["ground_table"] == [[3, 0], [0, 2]] and same["ground_iou"] == 1.0
    none = {"dtm": torch.full((2, 3), nan), "ndsm": torch.full((2, 3), nan), "ground": torch.zeros((2, 3), dtype=torch.bool)}
    e = TR.terrain_agreement(a, none)
    assert e["cells"] == 0 and e["dtm_mae"] is None and e["ndsm_mae"] is None and e["ground_accuracy"] is None and e["ground_iou"] is None
    with pytest.raises(ValueError, match=r"\(2, 3\) and \(2, 4\)"):
        TR.terrain_agreement(a, {"dtm": torch.zeros(2, 4)})


# ---- the objects without a DTM ------------------------------------------------------------------------------------------------------------
OBJECT_KEYS = ["class", "area_cells", "area_m2", "east", "north", "bbox", "perimeter_m", "alt_mean", "alt_min", "alt_max", "ground_alt",
               "ground_min", "height", "height_max", "volume_m3", "holes"]


def test_the_object_table_gains_its_terrain_columns_only_with_a_dtm():
    import inspect
    from tests import objects_numpy as ON
    q, bias = OB.OR.Q, 2 ** 31
    ks = [13 * 65536] * 6
    row = [6, 30, 9, 4, 6, 1, 2, 6, sum(ks), ks[0] + bias, ks[0] + bias, 8, 8 * 10 * 65536, 10 * 65536 + bias, 10, 3]
    rows = ON.words([row])
    grid = D.DsmGrid(1000.0, 2000.0, 0.5, 40, 30)
    t = OB.object_table(rows.view(np.int64), grid)
    assert list(t) == OBJECT_KEYS
    terrain_row = [6, 30, 9, 4, 6, 1, 2, 6, 6 * 10 * 65536 + 3 * 65536, 10 * 65536 + bias, 11 * 65536 + bias, 0, 0, 2 ** 64 - 1, 10, 3]
    t2 = OB.object_table(rows.view(np.int64), grid, terrain_rows=ON.words([terrain_row]).view(np.int64))
    assert list(t2) == OBJECT_KEYS + ["terrain_alt", "height_over_terrain", "volume_over_terrain_m3"]
    assert all(np.array_equal(t[k], t2[k]) for k in OBJECT_KEYS)
    assert (t2["terrain_alt"][0], t2["height_over_terrain"][0], t2["volume_over_terrain_m3"][0]) == (10.5, 2.5, 6 * 2.5 * 0.25)
    with pytest.raises(ValueError, match="1 rows but 2 terrain rows"):
        OB.object_table(rows.view(np.int64), grid, terrain_rows=ON.words([terrain_row, terrain_row]).view(np.int64))
    assert inspect.signature(OB.objects).parameters["dtm"].default is None
    from snerf_amd.eval import ortho as EO
    assert inspect.signature(EO.export_objects).parameters["dtm"].default is None
    assert list(inspect.signature(EO.export_terrain).parameters)[:7] == ["products", "output_dp", "alt_key", "label_key", "blocked", "reference",
                                                                         "zone_string"]


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
def _classes(*cs):
    t = (C.c_ubyte * 256)()
    for c in cs:
        t[c] = 1
    return t


def _call(symbol, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(alt=DUMMY, label=DUMMY, h=3, w=4, blocked_host=_classes(3), z0=0.0, q=2.0 ** -16, key=DUMMY, flags=DUMMY, stats=DUMMY,
             key_in=DUMMY, radius=2, threshold=5, key_out=2 * DUMMY, ws=DUMMY, dtm=DUMMY, ndsm=DUMMY, reach=DUMMY)
    a.update(kw)
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


SIZE_REFUSALS = [
    ({"stats": None}, 3, "null"),
    ({"h": 0}, 1, "h = 0"), ({"w": 0}, 1, "w = 0"), ({"h": -5}, 1, "h = -5"), ({"h": 32768, "w": 65536}, 1, "below 2^31"),
    ({"h": 2 ** 31 - 1, "w": 2 ** 31 - 1}, 1, "below 2^31"),
]
QUANT_REFUSALS = [
    ({"q": 0.0}, 1, "q > 0"), ({"q": -1.0}, 1, "q > 0"), ({"q": math.inf}, 1, "q > 0"), ({"q": math.nan}, 1, "q > 0"),
    ({"z0": math.nan}, 1, "z0 finite"), ({"z0": math.inf}, 1, "z0 finite"),
]
KEYS_REFUSALS = [
    ({"alt": None}, 3, "null"), ({"key": None}, 3, "null"), ({"flags": None}, 3, "null"),
    ({"label": None}, 3, "both given or both null"), ({"blocked_host": None}, 3, "both given or both null"),
    ({"blocked_host": _classes(3, 255)}, 1, "blocked_host[255]"),
]
OPEN_REFUSALS = [
    ({"key_in": None}, 3, "null"), ({"key_out": None}, 3, "null"), ({"ws": None}, 3, "null"),
    ({"radius": 0}, 1, "radius = 0"), ({"radius": 513}, 1, "radius = 513"), ({"radius": -1}, 1, "radius = -1"),
    ({"threshold": -1}, 1, "threshold = -1"), ({"key_out": DUMMY}, 1, "must not alias"),
]
FILL_REFUSALS = [
    ({"key": None}, 3, "null"), ({"flags": None}, 3, "null"), ({"alt": None}, 3, "null"), ({"dtm": None}, 3, "null"),
    ({"ndsm": None}, 3, "null"), ({"ws": None}, 3, "null"),
]
CASES = ([("snerf_terrain_keys", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + QUANT_REFUSALS + KEYS_REFUSALS]
         + [("snerf_terrain_open", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + OPEN_REFUSALS]
         + [("snerf_terrain_fill", kw, code, needle) for kw, code, needle in SIZE_REFUSALS + QUANT_REFUSALS + FILL_REFUSALS])


@pytest.mark.parametrize("symbol,kw,code,needle", CASES, ids=[f"{s[14:]}-{n}" for n, (s, _, _, _) in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, kw, code, needle):
    rc, msg = _call(symbol, **dict(kw))
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)


def test_workspace_bytes_refuses_bad_sizes():
    L = _lib.lib()
    for h, w, needle in ((0, 4, "h = 0"), (3, -1, "w = -1"), (32768, 65536, "below 2^31"), (2 ** 31 - 1, 2 ** 31 - 1, "below 2^31")):
        assert L.snerf_terrain_workspace_bytes(h, w) == -1
        msg = L.snerf_last_error().decode()
        assert msg.startswith("snerf_terrain_workspace_bytes: ") and needle in msg
    assert L.snerf_terrain_workspace_bytes(46340, 46340) == 16 * 46340 * 46340         # the largest square: beyond 32 bits


def test_there_is_no_empty_problem_and_python_refuses_host_tensors():
    """h, w >= 1 is required, so no accepted call is empty: the smallest problem is one cell (tests/test_gpu_terrain.py runs it).  The
    host layer refuses by name what is not on the GPU, and bad parameters before any call."""
    alt = torch.zeros((3, 4))
    key, flags = torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="alt must be a GPU tensor"):
        TR.keys(alt)
    with pytest.raises(ValueError, match="key must be a GPU tensor"):
        TR.opening(key, 1)
    with pytest.raises(ValueError, match="key must be a GPU tensor"):
        TR.ground_flags(key, flags, [1], [0])
    with pytest.raises(ValueError, match="key must be a GPU tensor"):
        TR.fill(key, flags, alt)
    with pytest.raises(ValueError, match="alt must be a GPU tensor"):
        TR.terrain(alt, D.DsmGrid(0.0, 0.0, 0.5, 4, 3))
    with pytest.raises(ValueError, match="512"):
        TR.terrain(alt, D.DsmGrid(0.0, 0.0, 0.05, 4, 3))                           # 80 m at 5 cm: a radius of 800
    assert (TR.FLAGGED, TR.BLOCKED, TR.IS_HOLE) == (1, 2, 4)
