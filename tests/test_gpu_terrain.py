"""The bare-earth terrain on the GPU (csrc/terrain.hip through eval/utils/terrain.py and eval/ortho.py export_terrain; DESIGN.md
section 5y), bit for bit against the numpy restatement tests/terrain_numpy.py: the keys, one level of the filter at the shapes, hole
patterns, radii and widths where a van Herk pass can go wrong, the fill on every ground pattern, and a synthetic town whose ground
mask, DTM and files are known exactly."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.eval.utils import terrain as TR
from snerf_amd.framework.util import img_utils
from tests import terrain_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII = (1, 2, 3, 31, 32, 33, 64, 200, 512)      # 200: beyond both sides of every raster here; 512: the limit
SHAPE_IDS = [f"{h}x{w}" for h, w in N.SHAPES]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared references stay read-only


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _filled(shape, dtype, fill):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.reshape(-1).view(torch.uint8).fill_(fill)
    return t


# ---- keys -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", N.SHAPES, ids=SHAPE_IDS)
def test_keys_are_the_restatements(shape):
    h, w = shape
    rng = np.random.default_rng(h + 3 * w)
    for pattern in N.HOLE_PATTERNS:
        alt = N.random_alt(h, w)
        holes = N.hole_mask(pattern, h, w)
        alt[holes] = np.array([np.nan, np.inf, -np.inf, 40000.0, -40000.0, 32768.0, -32768.0, 3.4e38], np.float32)[rng.integers(0, 8, int(holes.sum()))]
        label = rng.integers(0, 6, (h, w)).astype(np.uint8)
        label[rng.random((h, w)) < 0.1] = 255
        for lab, blocked in ((None, ()), (label, (3, 5)), (label, ())):
            want_key, want_flags, want_stats = N.keys(alt, lab, blocked)
            key, flags, stats = TR.keys(_dev(alt), None if lab is None else _dev(lab), blocked)
            assert stats.tolist() == want_stats, (pattern, blocked)
            assert np.array_equal(key.cpu().numpy(), want_key) and np.array_equal(flags.cpu().numpy(), want_flags), (pattern, blocked)
        if pattern != "none" and h * w > 1:
            assert want_stats[0] + want_stats[1] == holes.sum()
    # the two ends of the key range: the last fp32 below 32768 m is a key, 2^31 and -2^31 steps are not
    edge = np.array([[32767.998, 32768.0, -32767.998, -32768.0]], np.float32)
    key, flags, stats = TR.keys(_dev(edge))
    assert np.array_equal(key.cpu().numpy(), N.keys(edge)[0]) and flags.tolist() == [[0, 4, 0, 4]] and stats.tolist() == [2, 0, 0]


# ---- open -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _open_want(h, w, pattern, r, threshold):
    key = N.key_raster(h, w, pattern)
    rng = np.random.default_rng(r + h)
    flags = np.where(N.valid(key), rng.integers(0, 4, (h, w)), N.IS_HOLE | (rng.integers(0, 2, (h, w)) * 2)).astype(np.uint8)      # pre-set bits
    plain, _, _ = N.open_level(key, r)
    out, new_flags, newly = N.open_level(key, r, threshold, flags)
    for a in (key, flags, plain, out, new_flags):
        a.setflags(write=False)
    return key, flags, plain, out, new_flags, newly


def _check_open(h, w, pattern, r, threshold):
    key, flags, plain, want, want_flags, newly = _open_want(h, w, pattern, r, threshold)
    d_key = _dev(key)
    got, stats = TR.opening(d_key, r, out=_filled((h, w), torch.int32, 0x7B), ws=_filled((16 * h * w,), torch.uint8, 0xFF))
    assert np.array_equal(got.cpu().numpy(), plain) and stats.tolist() == [0], (h, w, pattern, r, "plain")
    d_flags = _dev(flags)
    got, stats = TR.opening(d_key, r, threshold, flags=d_flags)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(want, plain), (h, w, pattern, r)
    assert np.array_equal(d_flags.cpu().numpy(), want_flags) and stats.tolist() == [newly], (h, w, pattern, r, "flags")
    assert np.array_equal(want_flags & 6, flags & 6) and np.array_equal(want_flags & flags & 1, flags & 1)       # pre-set bits stay
    assert torch.equal(d_key, _dev(key))
    return newly


@pytest.mark.parametrize("shape", N.SHAPES, ids=SHAPE_IDS)
def test_one_level_is_the_restatements(shape):
    """every hole pattern and radius, with and without flags; the threshold (4 m, and 0 on the random pattern) leaves some cells
    unflagged and finds some already flagged: stats[0] counts the new ones only"""
    h, w = shape
    newly = 0
    for pattern in N.HOLE_PATTERNS:
        for r in RADII:
            newly += _check_open(h, w, pattern, r, 0 if pattern == "random" else 4 * 65536)
    assert newly > 0 or h * w == 1


@pytest.mark.parametrize("r", [3, 32])
def test_one_level_at_the_block_edges(r):
    """widths (and heights) of 2r, 2r + 1, 2r + 2 and 4r + 2 cells: a whole block, one cell less, one more, two blocks"""
    for n in (2 * r, 2 * r + 1, 2 * r + 2, 4 * r + 2):
        for h, w in ((5, n), (n, 5), (n, n) if r == 3 else (n, 66)):
            for pattern in ("none", "random"):
                _check_open(h, w, pattern, r, 0)
                _check_open(h, w, pattern, max(1, r - 1), 65536)


# ---- fill -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fill_want(h, w, pattern):
    key, flags, alt = N.fill_case(h, w, pattern)
    out = N.fill(key, flags, alt)
    for a in (key, flags, alt) + out[:3]:
        a.setflags(write=False)
    return key, flags, alt, out


FILL_CASES = [(h, w, p) for h, w in ((1, 1), (7, 65), (33, 64), (1, 300), (300, 1)) for p in N.GROUND_PATTERNS] + \
             [(70, 129, "random"), (70, 129, "row_ends"), (70, 129, "corner")]


@pytest.mark.parametrize("h,w,pattern", FILL_CASES, ids=[f"{h}x{w}-{p}" for h, w, p in FILL_CASES])
def test_the_fill_is_the_restatements(h, w, pattern):
    key, flags, alt, (dtm, ndsm, reach, counts) = _fill_want(h, w, pattern)
    got = TR.fill(_dev(key), _dev(flags), _dev(alt))
    assert got[3].tolist() == counts and sum(counts) == h * w
    assert np.array_equal(_bits(got[0]), dtm.view(np.uint32)) and np.array_equal(_bits(got[1]), ndsm.view(np.uint32))
    assert np.array_equal(got[2].cpu().numpy(), reach)
    if pattern == "none":
        assert counts == [0, 0, h * w] and bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[1]).all()) and bool((got[2] == -1).all())
    if pattern == "row_ends" and w == 300:
        assert reach.max() == 149 and counts[2] == 0                   # a run of 298 cells between the two ends of the row
    without = TR.fill(_dev(key), _dev(flags), _dev(alt), reach=False)
    assert without[2] is None and torch.equal(without[0].view(torch.int32), got[0].view(torch.int32))


# ---- the town -------------------------------------------------------------------------------------------------------------------------
GRID = D.DsmGrid(500000.0, 4100000.0, N.TOWN_RES, N.TOWN_SHAPE[1], N.TOWN_SHAPE[0])


@functools.lru_cache(maxsize=None)
def _town_want(slope, shift=0):
    alt, boxes, ground, mask = N.town(slope, shift)
    return alt, boxes, ground, mask, N.terrain(alt, N.TOWN_RES, **N.TOWN_SCHEDULE)


def _same_terrain(got, want):
    assert got["schedule"] == want["schedule"] and got["stats"] == want["stats"]
    for k in ("dtm", "ndsm"):
        assert np.array_equal(_bits(got[k]), want[k].view(np.uint32)), k
    for k in ("ground", "flags", "reach"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("slope", [0.0, 0.05, 0.1])
def test_the_town(slope):
    alt, boxes, ground, mask, want = _town_want(slope)
    got = TR.terrain(_dev(alt), GRID, **N.TOWN_SCHEDULE)
    _same_terrain(got, want)
    assert got["ground"].dtype == torch.bool and np.array_equal(~got["ground"].cpu().numpy(), mask) and got["stats"]["unreachable"] == 0
    dtm = got["dtm"].cpu().numpy()
    plane32 = ground.astype(np.float32)
    if slope == 0.0:
        assert np.array_equal(dtm.view(np.uint32), plane32.view(np.uint32))
        assert (got["ndsm"].cpu().numpy()[~mask].view(np.uint32) == 0).all()
    else:
        quantised = N.Z0 + N.Q * np.rint((plane32.astype(np.float64) - N.Z0) / N.Q)
        assert np.abs(dtm.astype(np.float64) - quantised).max() < N.Q
    again = TR.terrain(_dev(alt), GRID, **N.TOWN_SCHEDULE)
    assert all(torch.equal(_dev(_bits(again[k])), _dev(_bits(got[k]))) for k in ("dtm", "ndsm", "flags", "reach"))


def test_blocked_classes_are_never_ground():
    """a roof as wide as the raster survives every window; its class takes it out of the ground all the same"""
    alt = np.full((20, 40), 10.0, np.float32)
    alt[:, 10:] = 18.0
    label = np.zeros((20, 40), np.uint8)
    label[:, 10:] = 3
    kw = dict(max_window_m=4.0, slope=0.3)
    for lab, blocked in ((None, ()), (label, (3,))):
        want = N.terrain(alt, 0.5, lab, blocked, **kw)
        got = TR.terrain(_dev(alt), D.DsmGrid(0.0, 0.0, 0.5, 40, 20), None if lab is None else _dev(lab), blocked, **kw)
        _same_terrain(got, want)
    assert got["stats"]["blocked"] == 20 * 30 and got["stats"]["ground"] == 20 * 10 and float(got["ndsm"].max()) == 8.0
    with pytest.raises(ValueError, match="no label plane"):
        TR.terrain(_dev(alt), D.DsmGrid(0.0, 0.0, 0.5, 40, 20), None, (3,))


def test_no_output_depends_on_bytes_the_library_did_not_write():
    from tests.test_gpu_fill import run_filled
    alt, _, _, _, want = _town_want(0.05)
    radii, thresholds = want["schedule"]["radii"], want["schedule"]["thresholds"]
    h, w = alt.shape
    d_alt = _dev(alt)

    def run(fill):
        ws = _filled((16 * h * w,), torch.uint8, fill)
        key, flags = _filled((h, w), torch.int32, fill), _filled((h, w), torch.uint8, fill)
        stats = torch.zeros(3, dtype=torch.int64, device=DEV)
        TR._lib.call("snerf_terrain_keys", d_alt, None, h, w, None, N.Z0, N.Q, key, flags, stats)
        planes = [_filled((h, w), torch.int32, fill) for _ in range(2)]
        src, per_level = key, torch.zeros(len(radii), dtype=torch.int64, device=DEV)
        for k, (r, t) in enumerate(zip(radii, thresholds)):
            TR._lib.call("snerf_terrain_open", src, h, w, r, t, planes[k & 1], flags, ws, per_level[k:k + 1])
            src = planes[k & 1]
        wide = _filled((h, w), torch.int32, fill)
        TR._lib.call("snerf_terrain_open", key, h, w, 512, 0, wide, None, ws, torch.zeros(1, dtype=torch.int64, device=DEV))
        ws.view(torch.uint8).fill_(fill)
        dtm, ndsm, reach = _filled((h, w), torch.float32, fill), _filled((h, w), torch.float32, fill), _filled((h, w), torch.int32, fill)
        fstats = torch.zeros(3, dtype=torch.int64, device=DEV)
        TR._lib.call("snerf_terrain_fill", key, flags, d_alt, h, w, N.Z0, N.Q, dtm, ndsm, reach, ws, fstats)
        return {"key": key, "flags": flags, "opened": src, "wide": wide, "per_level": per_level, "dtm": dtm, "ndsm": ndsm, "reach": reach,
                "fstats": fstats}

    r = run_filled(run)[0xFF]
    assert np.array_equal(_bits(r["dtm"]), want["dtm"].view(np.uint32)) and np.array_equal(r["flags"].cpu().numpy(), want["flags"])
    assert r["per_level"].tolist() == want["stats"]["flagged_per_level"] and bool(torch.isfinite(r["dtm"]).all())
    assert np.array_equal(r["wide"].cpu().numpy(), N.open_level(r["key"].cpu().numpy(), 512)[0])


# ---- the files ------------------------------------------------------------------------------------------------------------------------
def test_export_terrain_on_the_town(tmp_path):
    alt, boxes, ground, mask, want = _town_want(0.0)
    ref_alt, _, _, ref_mask, ref_want = _town_want(0.0, 1)
    products = {"dsm": _dev(alt), "grid": GRID}
    out = EO.export_terrain(products, str(tmp_path), reference={"alt": _dev(ref_alt)}, zone_string="17R", **N.TOWN_SCHEDULE)
    names = {"dtm.tif", "dtm.png", "ndsm.tif", "ndsm.png", "ground.png", "reach.png", "terrain.json", "terrain_eval.json"}
    assert set(out["files"]) == names and all(os.path.isfile(p) and os.path.getsize(p) > 0 for p in out["files"].values())
    assert os.path.dirname(out["files"]["dtm.tif"]) == os.path.join(str(tmp_path), "terrain")
    _same_terrain(out, want)
    _same_terrain(out["reference"], ref_want)
    raster, transform = img_utils.load_dsm_geotiff(out["files"]["dtm.tif"])
    assert raster.dtype == np.float32 and np.array_equal(raster.view(np.uint32), want["dtm"].view(np.uint32))
    assert transform == (GRID.xoff, GRID.yoff, 0.5, 0.5)
    ndsm, _ = img_utils.load_dsm_geotiff(out["files"]["ndsm.tif"])
    assert np.array_equal(ndsm.view(np.uint32), want["ndsm"].view(np.uint32))
    doc = json.load(open(out["files"]["terrain.json"]))
    assert doc["schedule"] == want["schedule"] and doc["stats"] == want["stats"]
    assert doc["parameters"] == dict({"alt_key": "dsm", "label_key": None, "blocked": []}, **N.TOWN_SCHEDULE)
    ev = json.load(open(out["files"]["terrain_eval.json"]))
    assert ev == json.loads(json.dumps(TR.terrain_agreement(out, out["reference"]))) == json.loads(json.dumps(out["eval"]))
    both, either = int((~mask & ~ref_mask).sum()), int((~mask | ~ref_mask).sum())
    assert ev["cells"] == alt.size and ev["dtm_mae"] == 0.0 and ev["ground_table"][0][0] == both and ev["ground_iou"] == both / either
    # a label plane is picked up, and its buildings are blocked
    label = np.where(mask, 3, 0).astype(np.uint8)
    with_label = EO.export_terrain(dict(products, label=_dev(label)), str(tmp_path / "l"), **N.TOWN_SCHEDULE)
    assert with_label["stats"]["blocked"] == mask.sum() and np.array_equal(with_label["ground"].cpu().numpy(), ~mask)
    assert json.load(open(with_label["files"]["terrain.json"]))["parameters"]["blocked"] == [3]
    with pytest.raises(ValueError, match=r"\(70, 129\).*\(70, 128\)"):
        EO.export_terrain(products, str(tmp_path), reference={"alt": _dev(ref_alt[:, :-1])})


def test_objects_over_the_terrain():
    alt, boxes, ground, mask, want = _town_want(0.0)
    label = np.where(mask, 3, 0).astype(np.uint8)
    dtm = TR.terrain(_dev(alt), GRID, **N.TOWN_SCHEDULE)["dtm"]
    plain = OB.objects(_dev(label), _dev(alt), GRID, classes=(3,), ground=(0,))
    out = OB.objects(_dev(label), _dev(alt), GRID, classes=(3,), ground=(0,), dtm=dtm)
    t, p = out["table"], plain["table"]
    assert out["n"] == plain["n"] == 12 and set(t) - set(p) == {"terrain_alt", "height_over_terrain", "volume_over_terrain_m3"}
    assert all(np.array_equal(t[k], p[k], equal_nan=True) for k in p) and torch.equal(out["ids"], plain["ids"]) and out["stats"] == plain["stats"]
    for k, (j0, i0, nj, ni, roof) in enumerate(boxes):                 # the boxes are sorted in raster order, as the ids are
        assert t["terrain_alt"][k] == 10.0 and t["height_over_terrain"][k] == roof - 10.0
        assert t["volume_over_terrain_m3"][k] == nj * ni * 0.25 * (roof - 10.0)
