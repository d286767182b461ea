"""CPU-side checks of the orthorectifier (include/snerf_orthorect.h, csrc/orthorect.hip, eval/utils/orthorect.py):
the extension header's prototype, constants and struct layout against the binding (_lib.HEADER_SIGNATURES), the refusals of the
entry through the binding (none reaches a launch) and of the Python layer, map_agreement (plain torch: it runs on CPU tensors), and the numpy restatement
(tests/orthorect_numpy.py, the oracle of tests/test_gpu_orthorect.py) on the fixture scene: the five images of
tests/golden/scene_small on a 2 m lattice over their corners, the DSM a plane with one 30 m block."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import orthorect as R          # the feature under test: every test of this file needs it
from tests import orthorect_numpy as N
from tests import shadow_numpy as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_orthorect.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {"snerf_orthorectify": ["dsm", "grid", "lon0", "south", "images_host", "images_dev", "n_images", "rgbs", "labels", "n_rows", "n_classes",
                                "visible", "sum", "count", "votes", "col_row", "rgb_out", "label_out", "state_out", "stats", "stream"]}


def test_header_constants_and_layout_match_the_binding():
    src = open(HEADER).read()
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define SNERF_RECT_MAX_IMAGES (\d+)", src).group(1)) == _lib.RECT_MAX_IMAGES == _lib.SHADOW_MAX_SUNS
    for name, value in (("SEEN", 0), ("HOLE", 1), ("OUTSIDE", 2), ("HIDDEN", 3)):
        assert int(re.search(rf"#define SNERF_RECT_{name} (\d+)", src).group(1)) == getattr(_lib, "RECT_" + name) == value
        assert getattr(N, name) == getattr(R, name) == value
    assert C.sizeof(_lib.SnerfRectImage) == C.sizeof(_lib.SnerfRpc) + 16 == 1384      # the static_assert of csrc/orthorect.hip
    assert _lib.SnerfRectImage.row0.offset == 1368 and _lib.SnerfRectImage.w.offset == 1376 and _lib.SnerfRectImage.h.offset == 1380
    assert N.NO_LABEL == R.NO_LABEL == _lib.ORTHO_NO_LABEL and N.Q == R.Q == 2.0 ** -24


def test_extension_header_matches_its_binding_row():
    """include/snerf_orthorect.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py); the main header, the main table,
    the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_orthorect.h", NAMES)
    assert len(NAMES["snerf_orthorectify"]) == 21


@pytest.fixture(scope="module")
def case():
    """the fixture scene on its lattice: col_row of the restatement's first half, the numpy cast under the view rows, and the
    restatement's second half with and without the occlusion"""
    sc = N.fixture_scene()
    grid = N.fixture_lattice()
    dsm = N.block_dsm(grid)
    rows = N.fixture_rows()
    col_row = np.stack([N.project_cells(grid, dsm, m["rpc"], N.ZONE) for m in sc["metas"]])
    lit, _ = SN.cast(dsm, rows)
    vis = lit.reshape(len(rows), -1)
    args = (col_row, dsm, sc["images"], sc["rgbs"], sc["labels"], N.N_CLASSES)
    return {"scene": sc, "grid": grid, "dsm": dsm, "rows": rows, "col_row": col_row, "visible": vis, "args": args,
            "with": N.sample_and_fuse(*args, vis), "without": N.sample_and_fuse(*args, None)}


def test_the_block_hides_cells_and_the_lattice_reaches_beyond_the_images(case):
    state = case["with"]["state"]
    n, cells = state.shape
    assert (n, cells) == (5, case["grid"][5] * case["grid"][6]) and cells > 1500          # about one cell per pixel
    totals = np.stack([(state == s).sum(1) for s in range(4)], 1)
    print("per image (seen, hole, outside, hidden):", totals.tolist())
    assert (totals.sum(1) == cells).all()                                                 # the four states partition the cells
    assert totals[:, N.HIDDEN].max() >= 20 and totals[:, N.OUTSIDE].max() >= 20
    assert (totals[:, N.HOLE] == 0).all()
    assert case["with"]["acc"]["stats"].tolist() == totals.sum(0).tolist()
    # a hole is a hole for every image, whatever the projection would say
    holes = N.block_dsm(case["grid"], holes=True)
    col_row = np.stack([N.project_cells(case["grid"], holes, m["rpc"], N.ZONE) for m in case["scene"]["metas"]])
    out = N.sample_and_fuse(col_row, holes, *case["args"][2:], case["visible"])
    bad = ~np.isfinite(holes).reshape(-1)
    assert bad.sum() == 3 and (out["state"][:, bad] == N.HOLE).all() and (out["state"][:, ~bad] != N.HOLE).all()
    assert np.isnan(col_row[:, :, bad]).all() and np.isnan(out["rgb"][:, :, bad]).all() and (out["label"][:, bad] == N.NO_LABEL).all()
    assert (out["acc"]["count"][bad] == 0).all()


def test_outputs_of_a_cell_follow_from_its_state(case):
    out = case["with"]
    seen = out["state"] == N.SEEN
    assert (np.isfinite(out["rgb"]).all(1) == seen).all()
    assert ((out["label"] != N.NO_LABEL) == seen).all()                  # the fixture's labels lie in 0..4
    assert (out["acc"]["count"] == seen.sum(0)).all()
    assert (out["acc"]["votes"].sum(0) == seen.sum(0)).all()
    rgb = out["rgb"][seen.repeat(3).reshape(5, -1, 3).transpose(0, 2, 1)]
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0                         # a bilinear mean of pixels in [0, 1]
    m = N.mosaic(out["acc"])
    none = out["acc"]["count"] == 0
    assert none.any() and np.isnan(m["rgb"][:, none]).all() and (m["label"][none] == N.NO_LABEL).all() and np.isnan(m["share"][none]).all()
    assert np.isfinite(m["rgb"][:, ~none]).all() and (m["label"][~none] < N.N_CLASSES).all()
    assert ((m["share"][~none] > 0.0) & (m["share"][~none] <= 1.0)).all()
    # the mean of the per-image planes, to the quantisation of the sums (2^-25 per image) and one fp32 rounding
    mean = np.nansum(out["rgb"].astype(np.float64), 0)[:, ~none] / out["acc"]["count"][~none]
    assert np.abs(m["rgb"][:, ~none] - mean).max() <= 2.0 ** -24 + 2.0 ** -25


def test_image_order_and_a_cut_into_two_calls_leave_the_accumulators_unchanged(case):
    col_row, dsm, images, rgbs, labels, C_ = case["args"]
    vis, want = case["visible"], case["with"]["acc"]
    order = [3, 0, 4, 2, 1]
    perm = N.sample_and_fuse(col_row[order], dsm, [images[k] for k in order], rgbs, labels, C_, vis[order])
    acc = N.new_acc(col_row.shape[2], C_)
    N.sample_and_fuse(col_row[:2], dsm, images[:2], rgbs, labels, C_, vis[:2], acc=acc)
    N.sample_and_fuse(col_row[2:], dsm, images[2:], rgbs, labels, C_, vis[2:], acc=acc)
    for got in (perm["acc"], acc):
        for key in ("sum", "count", "votes", "stats"):
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert np.array_equal(perm["state"], case["with"]["state"][order])


def test_without_the_occlusion_hidden_cells_are_seen_and_nothing_else_changes(case):
    a, b = case["with"], case["without"]
    hidden = a["state"] == N.HIDDEN
    assert hidden.sum() >= 20 and (b["state"][hidden] == N.SEEN).all() and np.array_equal(a["state"][~hidden], b["state"][~hidden])
    assert not (b["state"] == N.HIDDEN).any()
    keep = ~hidden
    assert np.array_equal(a["label"][keep], b["label"][keep])
    for ch in range(3):
        assert np.array_equal(a["rgb"][:, ch][keep].view(np.uint32), b["rgb"][:, ch][keep].view(np.uint32))
    untouched = ~hidden.any(0)
    for key in ("sum", "votes"):
        assert np.array_equal(a["acc"][key][:, untouched], b["acc"][key][:, untouched]), key
    assert np.array_equal(b["acc"]["count"] - a["acc"]["count"], hidden.sum(0))
    # a cell is hidden exactly where the march towards the satellite is blocked, among the cells inside the image
    inside = b["state"] == N.SEEN
    assert np.array_equal(hidden, inside & (case["visible"] == 0))


def _angle_deg(a, b):
    """between two lines of sight given as rows (ux, uy, rise) at the same resolution: their directions are (ux, uy, rise / res)"""
    va, vb = (np.array([r[0], r[1], r[2] / N.RES]) for r in (a, b))
    return math.degrees(math.acos(min(1.0, float(va @ vb / (np.linalg.norm(va) * np.linalg.norm(vb))))))


def test_view_rows_are_unit_vectors_that_rise_and_one_direction_per_image_is_close(case):
    rows = case["rows"]
    assert rows.shape == (5, 3) and np.isfinite(rows).all()
    assert np.abs(np.hypot(rows[:, 0], rows[:, 1]) - 1.0).max() <= 1e-12 and (rows[:, 2] > 0.0).all()
    worst = 0.0
    for m, centre in zip(case["scene"]["metas"], rows):
        w, h = m["width"], m["height"]
        for px in ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0)):
            worst = max(worst, _angle_deg(centre, N.view_row(m["rpc"], w, h, m["min_alt"], m["max_alt"], N.ZONE, N.RES, pixel=px)))
    print(f"one direction per image: the line of sight at an image corner is at most {worst:.4f} degrees from the one at its centre")
    assert 0.0 <= worst < 5.0          # a sanity bound, not a bar: 80 m of scene under a satellite hundreds of km away
    # scaling the resolution scales the rise and nothing else
    fine = N.fixture_rows(0.5)
    assert np.array_equal(fine[:, :2], rows[:, :2]) and np.abs(fine[:, 2] * 4.0 - rows[:, 2]).max() <= 1e-12


def _call(**kw):
    """snerf_orthorectify through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    table = (_lib.SnerfRectImage * 2)()
    for k in range(2):
        for f in ("row_scale", "col_scale", "lat_scale", "lon_scale", "alt_scale"):
            setattr(table[k].rpc, f, 1.0)
        table[k].row0, table[k].w, table[k].h = 20 * k, 5, 4
    if "image" in kw:
        kw.pop("image")(table[1])
    a = dict(dsm=DUMMY, grid=_lib.SnerfDsmGrid(1000.0, 2000.0, 0.5, 4, 3, 0, 0, 4, 3), lon0=-1.4137166941154069, south=0, host=table,
             dev=DUMMY, n_images=2, rgbs=DUMMY, labels=DUMMY, n_rows=40, n_classes=5, visible=None, sum=DUMMY, count=DUMMY, votes=DUMMY,
             col_row=None, rgb_out=None, label_out=None, state_out=None, stats=DUMMY)
    a.update(kw)
    grid = C.byref(a["grid"]) if a["grid"] is not None else None
    rc = L.snerf_orthorectify(a["dsm"], grid, a["lon0"], a["south"], a["host"], a["dev"], a["n_images"], a["rgbs"], a["labels"],
                              a["n_rows"], a["n_classes"], a["visible"], a["sum"], a["count"], a["votes"], a["col_row"], a["rgb_out"],
                              a["label_out"], a["state_out"], a["stats"], None)
    return rc, L.snerf_last_error().decode()


def _grid(**kw):
    g = _lib.SnerfDsmGrid(1000.0, 2000.0, 0.5, 4, 3, 0, 0, 4, 3)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _set(**kw):
    def edit(im):
        for k, v in kw.items():
            setattr(im.rpc if k.endswith("_scale") else im, k, v)
    return edit


@pytest.mark.parametrize("kw,code,needle", [
    ({"dsm": None}, 3, "null"), ({"grid": None}, 3, "null"), ({"host": None}, 3, "null"), ({"dev": None}, 3, "null"),
    ({"rgbs": None}, 3, "null"), ({"sum": None}, 3, "null"), ({"count": None}, 3, "null"), ({"stats": None}, 3, "null"),
    ({"votes": None}, 3, "labels and votes"), ({"labels": None}, 3, "labels and votes"),
    ({"grid": _grid(res=0.0)}, 1, "res > 0"), ({"grid": _grid(res=math.nan)}, 1, "res > 0"), ({"grid": _grid(out_h=0)}, 1, "positive sizes"),
    ({"grid": _grid(joff=2 ** 31 - 3)}, 1, "int32"), ({"grid": _grid(out_w=1 << 16, out_h=1 << 15)}, 1, "2^31"),
    ({"n_images": 0}, 1, "n_images = 0"), ({"n_images": 65}, 1, "n_images = 65"),
    ({"n_classes": 0}, 1, "n_classes = 0"), ({"n_classes": 256}, 1, "n_classes = 256"), ({"n_rows": 0}, 1, "n_rows"),
    ({"lon0": 3.2}, 1, "central meridian"), ({"lon0": math.nan}, 1, "central meridian"), ({"south": 2}, 1, "south = 2"),
    ({"image": _set(w=0)}, 1, "image 1 has a bad size"), ({"image": _set(h=-3)}, 1, "image 1 has a bad size"),
    ({"image": _set(row0=-1)}, 1, "image 1: rows"), ({"image": _set(row0=21)}, 1, "image 1: rows"),
    ({"image": _set(row0=2 ** 63 - 4)}, 1, "image 1: rows"),
    ({"image": _set(lon_scale=0.0)}, 1, "RPC 1 has a zero"), ({"image": _set(alt_scale=math.inf)}, 1, "RPC 1 has a zero"),
], ids=lambda v: None if callable(v) or isinstance(v, dict) else str(v))
def test_the_entry_refuses_bad_arguments_before_any_launch(kw, code, needle):
    rc, msg = _call(**dict(kw))
    assert rc == code and msg.startswith("snerf_orthorectify: ") and needle in msg, (rc, msg)


def test_python_refusals():
    dsm = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="must be a GPU tensor"):
        R.rectify(dsm, _grid(), None, [{}])
    with pytest.raises(ValueError, match="no image"):
        R.visibility(dsm, np.zeros((0, 3)))
    with pytest.raises(ValueError, match="0 cameras and 0 sizes"):
        R.view_rows([], 0.0, 1.0, [], None, 1.0)
    with pytest.raises(ValueError, match="1 cameras and 2 sizes"):
        R.view_rows([None], 0.0, 1.0, [(3, 3), (3, 3)], None, 1.0)
    with pytest.raises(ValueError, match="res = 0.0"):
        R.view_rows([None], 0.0, 1.0, [(3, 3)], None, 0.0)
    with pytest.raises(ValueError, match="2 alt_max values for 1 images"):
        R.view_rows([None], 0.0, [1.0, 2.0], [(3, 3)], None, 1.0)
    with pytest.raises(ValueError, match="image 0 needs finite alt_min < alt_max"):
        R.view_rows([None], 5.0, 5.0, [(3, 3)], None, 1.0)
    mosaic = {"rgb": torch.zeros(3, 4, 5)}
    with pytest.raises(ValueError, match="a colour map"):
        R.map_agreement(torch.zeros(3, 5, 4), None, mosaic, 5)
    with pytest.raises(ValueError, match="no voted labels"):
        R.map_agreement(None, torch.zeros(4, 5, dtype=torch.uint8), mosaic, 5)
    with pytest.raises(ValueError, match="a label map"):
        R.map_agreement(None, torch.zeros(5, 4, dtype=torch.uint8), dict(mosaic, label_vote=torch.zeros(4, 5, dtype=torch.uint8)), 5)


def test_map_agreement_counts_and_figures():
    from snerf_amd.eval.utils import metrics
    from snerf_amd.eval.utils.semantic import normalized_confusion, semantic_miou
    g = torch.Generator().manual_seed(3)
    h, w, n_classes = 9, 7, 5
    ref_rgb, rgb = torch.rand((3, h, w), generator=g), torch.rand((3, h, w), generator=g)
    ref_rgb[:, 0, 0], rgb[1, 2, 3], rgb[:, 0, 0] = math.nan, math.inf, math.nan
    ref_label = torch.randint(0, n_classes, (h, w), generator=g).to(torch.uint8)
    label = torch.randint(0, n_classes, (h, w), generator=g).to(torch.uint8)
    ref_label[1, :3], label[2, 4], label[3, 3] = 255, 255, 7                          # no vote; no prediction; beyond the classes
    out = R.map_agreement(rgb, label, {"rgb": ref_rgb, "label_vote": ref_label}, n_classes)
    both = torch.ones(h, w, dtype=torch.bool)
    both[0, 0] = both[2, 3] = False
    assert out["psnr_cells"] == h * w - 2
    want = float(metrics.psnr(rgb.permute(1, 2, 0)[both], ref_rgb.permute(1, 2, 0)[both]))
    assert math.isfinite(want) and abs(out["psnr"] - want) <= 1e-5 * abs(want)
    conf = np.zeros((n_classes, n_classes), np.int64)
    for r, p in zip(ref_label.reshape(-1).tolist(), label.reshape(-1).tolist()):
        if r < n_classes and p < n_classes:
            conf[r, p] += 1
    assert out["confusion"] == conf.tolist() and out["label_cells"] == int(conf.sum()) == h * w - 5
    assert out["accuracy"] == float(np.trace(conf)) / conf.sum() and out["mIoU"] == semantic_miou(normalized_confusion(conf))
    empty = R.map_agreement(None, torch.full((h, w), 255, dtype=torch.uint8), {"rgb": ref_rgb, "label_vote": ref_label}, n_classes)
    assert empty["label_cells"] == 0 and math.isnan(empty["accuracy"]) and math.isnan(empty["mIoU"])
    assert sorted(R.map_agreement(rgb, None, {"rgb": ref_rgb}, n_classes)) == ["psnr", "psnr_cells"]
