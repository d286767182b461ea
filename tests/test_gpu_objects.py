"""The objects on the map on the GPU (csrc/objects.hip through eval/utils/objects.py and eval/ortho.py export_objects; DESIGN.md
section 5x), bit for bit against the numpy restatement tests/objects_numpy.py: the labelling at the shapes and on the structured
rasters where a union-find can go wrong, the per-object words at every ring and in row bands, the two extremes of the wave
reduction, and a synthetic town whose table, files and scores are known exactly."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import objects as OB
from snerf_amd.framework.util import img_utils
from tests import objects_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = (3, 4)
SENTINEL = 0x5A5A5A5A


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the shared references stay read-only


@functools.lru_cache(maxsize=None)
def _rasters():
    out = {f"random_{h}x{w}": N.random_label(h, w) for h, w in N.RANDOM_SHAPES}
    out.update(N.structured())
    return out


@functools.lru_cache(maxsize=None)
def _want_parent(name, connectivity):
    parent, stats = N.link(_rasters()[name], CLASSES, connectivity)
    parent.setflags(write=False)
    return parent, stats


RASTER_NAMES = [f"random_{h}x{w}" for h, w in N.RANDOM_SHAPES] + ["serpentine", "spiral", "checkerboard", "one_class", "comb",
                                                                    "alternating_columns", "no_member"]


# ---- link -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", RASTER_NAMES)
def test_link_is_the_restatements(name, connectivity):
    label = _rasters()[name]
    h, w = label.shape
    want, want_stats = _want_parent(name, connectivity)
    parent = torch.full((h * w,), SENTINEL, dtype=torch.int32, device=DEV)          # every word is rewritten
    got, stats = OB.link(_dev(label), CLASSES, connectivity, parent=parent)
    assert got is parent and stats.tolist() == want_stats                            # [0]: no guard trip
    assert np.array_equal(got.cpu().numpy(), want)
    ids, K = OB.components(_dev(label), CLASSES, connectivity)
    want_ids, want_K = N.ids_of(want, h, w)
    assert K == want_K and ids.dtype == torch.int32 and np.array_equal(ids.cpu().numpy(), want_ids)


def test_link_gives_equal_bits_twice_where_every_union_collides():
    label = _dev(_rasters()["one_class"])
    first, s1 = OB.link(label, CLASSES, 8)
    second, s2 = OB.link(label, CLASSES, 8)
    assert torch.equal(first, second) and s1.tolist() == s2.tolist() == [0, 64 * 256] and int(first.max()) == 0


def test_no_member_cell_at_all():
    label = _dev(_rasters()["no_member"])
    ids, K = OB.components(label, CLASSES, 4)
    assert K == 0 and not ids.any()
    parent, stats = OB.link(label, CLASSES, 4)
    assert (parent == -1).all() and stats.tolist() == [0, 0]
    rows, stats = OB.object_rows(ids, 0, label, torch.zeros(label.shape, device=DEV), (0,))
    assert tuple(rows.shape) == (0, 16) and stats.tolist() == [0, 0, 0, 0]


# ---- stats ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stats_case(h, w):
    """a random raster with its restated ids, altitudes that hold every special value, and two cells with ids outside [0, K]"""
    rng = np.random.default_rng(h * 7 + w)
    label = N.random_label(h, w, seed=1)
    ids, K = N.ids_of(N.link(label, CLASSES, 4)[0], h, w)
    alt = (np.round(rng.uniform(-40.0, 60.0, (h, w)) * 64) / 64).astype(np.float32)
    flat = alt.reshape(-1)
    special = rng.permutation(h * w)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 40000.0, -40000.0, 32768.0, -32768.0, 3.4e38)):
        flat[special[k::29][:max(1, h * w // 60)]] = v
    ids = ids.copy()
    ids.reshape(-1)[special[-1]], ids.reshape(-1)[special[-2]] = -1, K + 1
    for a in (label, ids, alt):
        a.setflags(write=False)
    return label, ids, K, alt


@pytest.mark.parametrize("ring", [0, 1, 2, 7])
@pytest.mark.parametrize("shape", [(7, 65), (33, 64), (70, 129)])
def test_rows_are_the_restatements_whole_and_in_two_bands(shape, ring):
    h, w = shape
    label, ids, K, alt = _stats_case(h, w)
    want_rows, want_stats = N.rows_loop(ids, K, label, alt, (0,), ring)
    want = N.words(want_rows)
    assert K > 1 and want_stats[2] == 2 and min(want_stats[:2]) > 0 and (want_stats[3] > 0) == (ring > 0)
    d_ids, d_label, d_alt = _dev(ids), _dev(label), _dev(alt)
    rows, stats = OB.object_rows(d_ids, K, d_label, d_alt, (0,), ring)
    assert stats.tolist() == want_stats
    assert np.array_equal(rows.cpu().numpy().view(np.uint64), want)
    cut = h // 2 + 1
    banded, bstats = OB.object_rows(d_ids, K, d_label, d_alt, (0,), ring, band=(cut, h))          # the southern band first
    banded, bstats = OB.object_rows(d_ids, K, d_label, d_alt, (0,), ring, rows=banded, stats=bstats, band=(0, cut))
    assert torch.equal(banded, rows) and bstats.tolist() == want_stats


@pytest.mark.parametrize("name,connectivity", [("one_class", 4), ("checkerboard", 4)])
def test_the_two_extremes_of_the_wave_reduction(name, connectivity):
    """one object of 16,384 cells (every lane of every wave in one row of words) and 560 single-cell objects (every lane its own)"""
    label = _rasters()[name]
    h, w = label.shape
    jj, ii = np.mgrid[0:h, 0:w]
    alt = ((jj * 3 - ii) / 16.0).astype(np.float32)                     # negative and positive, multiples of 2^-4
    ids, K = OB.components(_dev(label), CLASSES, connectivity)
    assert K == {"one_class": 1, "checkerboard": 560}[name]
    want_rows, want_stats = N.rows_loop(ids.cpu().numpy(), K, label, alt, (0,), 1)
    rows, stats = OB.object_rows(ids, K, _dev(label), _dev(alt), (0,), 1)
    assert stats.tolist() == want_stats and np.array_equal(rows.cpu().numpy().view(np.uint64), N.words(want_rows))


def test_python_refusals_on_device_tensors():
    label = torch.zeros((3, 4), dtype=torch.uint8, device=DEV)
    ids, alt = torch.zeros((3, 4), dtype=torch.int32, device=DEV), torch.zeros((3, 4), device=DEV)
    with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
        OB.components(label, (3,), 3)
    with pytest.raises(ValueError, match="class ids in"):
        OB.components(label, (255,))
    with pytest.raises(ValueError, match="ring = 8"):
        OB.object_rows(ids, 1, label, alt, (0,), ring=8)
    with pytest.raises(ValueError, match="alt must be a 2-D"):
        OB.object_rows(ids, 1, label, alt.double(), (0,))
    with pytest.raises(ValueError, match="row1 = 4"):
        OB.object_rows(ids, 1, label, alt, (0,), band=(0, 4))
    with pytest.raises(ValueError, match=r"shape \(2, 16\)"):
        OB.object_rows(ids, 2, label, alt, (0,), rows=OB.new_rows(3, DEV))


# ---- the town -------------------------------------------------------------------------------------------------------------------------
GRID = D.DsmGrid(500000.0, 4100000.0, 0.5, 130, 96)


def test_the_town():
    label, alt, boxes = N.town()
    out = OB.objects(_dev(label), _dev(alt), GRID, classes=CLASSES, ground=(0,))
    t = out["table"]
    assert out["n"] == 4 and t["class"].tolist() == [3, 3, 3, 4] and out["stats"][:3] == [0, 0, 0]
    res = 0.5
    for k, (j0, i0, nj, ni, z) in enumerate(boxes):
        assert t["area_cells"][k] == nj * ni and t["area_m2"][k] == nj * ni * res * res and t["holes"][k] == 0
        assert (t["alt_mean"][k], t["alt_min"][k], t["alt_max"][k], t["ground_alt"][k], t["ground_min"][k]) == (z, z, z, 3.0, 3.0)
        assert t["height"][k] == t["height_max"][k] == z - 3.0
        assert t["volume_m3"][k] == nj * ni * res * res * (z - 3.0)
        assert t["east"][k] == GRID.xoff + (i0 + ni / 2) * res and t["north"][k] == GRID.yoff - (j0 + nj / 2) * res
        assert t["bbox"][k].tolist() == [GRID.xoff + i0 * res, GRID.yoff - (j0 + nj) * res, GRID.xoff + (i0 + ni) * res, GRID.yoff - j0 * res]
        assert t["perimeter_m"][k] == 2 * (nj + ni) * res
    assert t["height"][:3].tolist() == [6.0, 12.5, 20.0] and t["height"][3] == 1.5
    ids = out["ids"].cpu().numpy()
    for k, (j0, i0, nj, ni, _) in enumerate(boxes):
        assert (ids[j0:j0 + nj, i0:i0 + ni] == k + 1).all()
    assert (ids > 0).sum() == sum(b[2] * b[3] for b in boxes) + 4
    oh = out["object_height"].cpu().numpy()
    assert oh.dtype == np.float32 and np.array_equal(np.isnan(oh), ids == 0) and oh[boxes[2][0], boxes[2][1]] == 20.0
    # the 2 x 2 blob (1 m2) is dropped at 2 m2 and the ids stay 1..3 in raster order
    kept = OB.objects(_dev(label), _dev(alt), GRID, classes=CLASSES, ground=(0,), min_area_m2=2.0)
    assert kept["n"] == 3 and kept["table"]["class"].tolist() == [3, 3, 3]
    assert np.array_equal(kept["ids"].cpu().numpy(), np.where(ids == 4, 0, ids))
    # a window of a larger lattice gives the same coordinates through its offsets
    window = D.grid_struct(D.DsmGrid(GRID.xoff - 10 * res, GRID.yoff + 4 * res, res, 200, 150), (10, 4, 130, 96))
    t2 = OB.objects(_dev(label), _dev(alt), window, classes=CLASSES, ground=(0,))["table"]
    assert all(np.array_equal(t[k], t2[k]) for k in t)


def test_export_objects_on_the_town(tmp_path):
    label, alt, boxes = N.town()
    ref_label, ref_alt, _ = N.town(shift=1)
    products = {"label": _dev(label), "dsm": _dev(alt), "grid": GRID}
    out = EO.export_objects(products, str(tmp_path), reference={"label": _dev(ref_label), "alt": _dev(ref_alt)}, zone_string="17R")
    names = {"objects.json", "objects_ids.tif", "objects_ids.png", "objects_height.tif", "objects_height.png", "reference_objects.json",
             "objects_eval.json"}
    assert set(out["files"]) == names and all(os.path.isfile(p) and os.path.getsize(p) > 0 for p in out["files"].values())
    assert os.path.dirname(out["files"]["objects.json"]) == os.path.join(str(tmp_path), "objects")
    doc = json.load(open(out["files"]["objects.json"]))
    assert out["n"] == 3 and doc["objects"] == json.loads(json.dumps(OB.table_records(out["table"]))) and doc["stats"] == out["stats"]
    assert doc["parameters"] == {"classes": [3], "ground": [0], "label_key": "label", "alt_key": "dsm"}
    assert [o["height"] for o in doc["objects"]] == [6.0, 12.5, 20.0] and [o["id"] for o in doc["objects"]] == [1, 2, 3]
    raster, transform = img_utils.load_dsm_geotiff(out["files"]["objects_ids.tif"])
    assert raster.dtype == np.float32 and np.array_equal(raster, out["ids"].cpu().numpy()) and transform == (GRID.xoff, GRID.yoff, 0.5, 0.5)
    height, _ = img_utils.load_dsm_geotiff(out["files"]["objects_height.tif"])
    assert np.array_equal(height, out["object_height"].cpu().numpy(), equal_nan=True)
    ev = json.load(open(out["files"]["objects_eval.json"]))
    assert (ev["n_a"], ev["n_b"], ev["matched"], ev["precision"], ev["recall"], ev["f1"]) == (3, 3, 3, 1.0, 1.0, 1.0)
    ious = [nj * (ni - 1) / (nj * (ni + 1)) for _, _, nj, ni, _ in boxes]      # a one-column shift of an nj x ni box
    assert ev["iou_mean"] == float(np.mean(np.array(ious)))
    assert ev["height_mae"] == ev["height_bias"] == ev["height_median_abs"] == 0.0 and ev["area_ratio_mean"] == 1.0
    assert ev["class_confusions"] == [] and ev["per_class"]["3"]["matched"] == 3
    assert len(json.load(open(out["files"]["reference_objects.json"]))["objects"]) == 3
    with pytest.raises(ValueError, match=r"\(96, 130\).*\(96, 129\)"):
        EO.export_objects(products, str(tmp_path), reference={"label": _dev(ref_label[:, :-1]), "alt": _dev(ref_alt[:, :-1])})
