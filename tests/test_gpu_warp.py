"""The raster warp on the device (include/snerf_warp.h, csrc/warp.hip, eval/utils/warp.py) against its numpy
restatement (tests/warp_numpy.py, itself held to closed forms by tests/test_warp_cpu.py): every word and every count bit for bit, NaN
positions included; then the ground truth read from files at another resolution, and the exports with a reference on a lattice of its
own.  Every output is pre-filled with a poison pattern: a word the library does not write shows."""
import json
import os

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval import ortho as EO
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import warp as W
from snerf_amd.framework.util import img_utils
from tests import terrain_numpy as TN
from tests import warp_numpy as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = {v: k for k, v in W.METHODS.items()}

# (source (h, w), destination (h, w), step_x, step_y, off_x, off_y, holes, planes, +-inf planted)
CASES = [
    ((1, 1), (1, 1), 1.0, 1.0, 0.0, 0.0, "none", 1, False),                   # one cell onto itself
    ((1, 1), (4, 63), 0.37, 0.37, -3.3, -0.2, "none", 1, False),              # a one-cell source under a fine destination
    ((7, 65), (9, 130), 0.5, 0.5, 0.0, 0.0, "random", 3, False),              # twice as fine, the same extent
    ((7, 65), (5, 65), 1.0, 1.0, 0.5, -0.25, "band", 1, True),                # step 1 off the lattice
    ((7, 65), (4, 64), 1.0, 1.0, -2.0, 3.0, "random", 3, False),              # a whole-cell shift through the kernel
    ((33, 64), (9, 63), 0.37, 0.37, 1.7, -1.2, "random", 1, True),
    ((33, 64), (5, 64), 2.0, 3.0, 0.0, 0.0, "none", 3, False),                # integer steps; the east half beyond the source
    ((33, 64), (9, 65), 2.0, 2.0, -7.5, -3.0, "band", 1, False),
    ((33, 64), (1, 64), 0.5, 0.5, 0.0, 0.0, "all", 3, False),                 # nothing but holes
    ((70, 129), (9, 130), 34 / 13, 34 / 13, -1.3, 0.4, "random", 3, True),    # more than one tile row and column
    ((70, 129), (4, 1), 2.0, 3.0, 60.25, 20.5, "random", 1, False),           # a single column
    ((70, 129), (5, 63), 0.5, 0.37, 100.0, 69.0, "none", 1, False),           # over the south-east corner
    ((70, 129), (4, 65), 1.0, 2.0, 200.0, 0.0, "none", 1, False),             # wholly beyond the source
    ((192, 128), (3, 2), 64.0, 64.0, 0.0, 0.0, "random", 1, True),            # the largest step, 64 taps per axis
    ((192, 128), (3, 2), 64.0, 64.0, -0.5, 0.25, "random", 3, False),         # ... and 65, part of them outside
]
IDS = [f"{k}-{c[0][0]}x{c[0][1]}-to-{c[1][0]}x{c[1][1]}" for k, c in enumerate(CASES)]


def _map(case):
    (sh, sw), (dh, dw), step_x, step_y, off_x, off_y = case[:6]
    return N.Map(off_x, step_x, off_y, step_y, sw, sh, dw, dh)


def _struct(m):
    return _lib.SnerfWarpMap(*m)


def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.reshape(-1).view(torch.uint8).fill_(0xA5)
    return t


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _planes(src, m, method, min_valid=0.5):
    """snerf_warp_planes by the table on a device tensor (planes, h, w): (dst, stats as a list)"""
    dst = _poisoned((src.shape[0], m.dst_h, m.dst_w), torch.float32)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    _lib.call("snerf_warp_planes", src, src.shape[0], _struct(m), method, min_valid, dst, stats)
    return dst, stats.tolist()


def _labels(src, m, method):
    dst = _poisoned((m.dst_h, m.dst_w), torch.uint8)
    stats = torch.zeros(3, dtype=torch.int64, device=DEV)
    _lib.call("snerf_warp_labels", src, _struct(m), method, dst, stats)
    return dst, stats.tolist()


# ---- bit for bit against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planes_are_the_restatements(case):
    (sh, sw), _, _, _, _, _, pattern, planes, infs = case
    m = _map(case)
    host = N.float_raster(sh, sw, pattern, planes=planes, seed=len(pattern) + planes, infs=infs)
    src = torch.from_numpy(host).to(DEV)
    for method in N.FLOAT_METHODS:
        for min_valid in ((0.5,) if method == N.NEAREST else (0.25, 0.5, 1.0)):
            want, want_stats = N.warp_planes(host, m, method, min_valid)
            got, stats = _planes(src, m, method, min_valid)
            assert np.array_equal(_bits(got), want.view(np.uint32)), (NAMES[method], min_valid)
            assert stats == want_stats and sum(stats[:2]) == want.size, (NAMES[method], min_valid, stats, want_stats)
    # the host layer on the same map: lattices that give these steps and offsets exactly (powers of two only)
    if all(float(v).is_integer() for v in (m.off_x * 4, m.off_y * 4, m.step_x * 4, m.step_y * 4)):
        a = W.Lattice(1000.0, 2000.0, 1.0, 1.0, sw, sh)
        b = W.Lattice(1000.0 + m.off_x, 2000.0 - m.off_y, m.step_x, m.step_y, m.dst_w, m.dst_h)
        got, stats = W.warp(src, a, b, "average", min_valid=0.25, return_stats=True)
        want, want_stats = N.warp_planes(host, m, N.AVERAGE, 0.25)
        assert np.array_equal(_bits(got), want.view(np.uint32)) and stats == want_stats


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_labels_are_the_restatements(case):
    """the classes 0 ... 5 and 254 in blocks a few cells wide, so that majorities tie, 255 as holes"""
    (sh, sw) = case[0]
    m = _map(case)
    host = N.label_raster(sh, sw, seed=case[7])
    src = torch.from_numpy(host).to(DEV)
    for method in N.LABEL_METHODS:
        want, want_stats = N.warp_labels(host, m, method)
        got, stats = _labels(src, m, method)
        assert np.array_equal(got.cpu().numpy(), want), NAMES[method]
        assert stats == want_stats and sum(stats[:2]) == want.size, (NAMES[method], stats, want_stats)


def test_ties_occur_and_go_to_the_lowest_class():
    """two classes in a checkerboard under 2 x 2 destination cells: every vote ties; a third of the cells hold no label at all"""
    jj, ii = np.mgrid[0:66, 0:130]
    host = np.where((ii + jj) % 2 == 0, 5, 2).astype(np.uint8)
    host[:, 40:84] = 255
    m = N.Map(0.0, 2.0, 0.0, 2.0, 130, 66, 65, 33)
    got, stats = _labels(torch.from_numpy(host).to(DEV), m, N.MODE)
    want = np.full((33, 65), 2, np.uint8)
    want[:, 20:42] = 255
    assert np.array_equal(got.cpu().numpy(), want) and stats == [33 * 43, 33 * 22, 0]
    assert np.array_equal(N.warp_labels(host, m, N.MODE)[0], want)


def test_more_tiles_and_cells_than_workgroups():
    """a launch has at most 1024 workgroups: 2,052 tiles of the planes and of the nearest label, and 4,550 cells of the majority (four
    per workgroup pass), are strided over"""
    m = N.Map(1.5, 0.9, -0.25, 0.008, 64, 33, 65, 4100)
    host = N.float_raster(33, 64, "random", seed=8)
    src = torch.from_numpy(host).to(DEV)
    for method in N.FLOAT_METHODS:
        want, want_stats = N.warp_planes(host, m, method)
        got, stats = _planes(src, m, method)
        assert np.array_equal(_bits(got), want.view(np.uint32)) and stats == want_stats, NAMES[method]
    lab = N.label_raster(33, 64, seed=8)
    want, want_stats = N.warp_labels(lab, m, N.NEAREST)
    got, stats = _labels(torch.from_numpy(lab).to(DEV), m, N.NEAREST)
    assert np.array_equal(got.cpu().numpy(), want) and stats == want_stats
    m = N.Map(-1.0, 1.7, 0.5, 0.45, 129, 70, 65, 70)
    lab = N.label_raster(70, 129, seed=8)
    want, want_stats = N.warp_labels(lab, m, N.MODE)
    got, stats = _labels(torch.from_numpy(lab).to(DEV), m, N.MODE)
    assert np.array_equal(got.cpu().numpy(), want) and stats == want_stats


def test_a_large_step_passes_where_one_cell_is_read():
    """SNERF_WARP_MAX_STEP bounds the area methods and the majority; nearest and bilinear read one and four cells at any step"""
    host = N.float_raster(70, 129, "random", seed=9)
    m = N.Map(-3.5, 65.5, 1.25, 70.0, 129, 70, 3, 2)
    src = torch.from_numpy(host).to(DEV)
    for method in (N.NEAREST, N.BILINEAR):
        got, stats = _planes(src, m, method)
        want, want_stats = N.warp_planes(host, m, method)
        assert np.array_equal(_bits(got), want.view(np.uint32)) and stats == want_stats
    lab = N.label_raster(70, 129)
    got, stats = _labels(torch.from_numpy(lab).to(DEV), m, N.NEAREST)
    want, want_stats = N.warp_labels(lab, m, N.NEAREST)
    assert np.array_equal(got.cpu().numpy(), want) and stats == want_stats
    with pytest.raises(RuntimeError, match="SNERF_WARP_MAX_STEP"):
        _planes(src, m, N.AVERAGE)
    with pytest.raises(RuntimeError, match="SNERF_WARP_MAX_STEP"):
        _labels(torch.from_numpy(lab).to(DEV), m, N.MODE)


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_plane_by_plane_give_the_same_bits():
    m = N.Map(-1.3, 34 / 13, 0.4, 1.7, 129, 70, 47, 40)
    host = N.float_raster(70, 129, "random", planes=3, seed=11, infs=True)
    src = torch.from_numpy(host).to(DEV)
    for method in N.FLOAT_METHODS:
        first, stats = _planes(src, m, method, 0.25)
        again, stats2 = _planes(src, m, method, 0.25)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)) and stats == stats2
        singles = [_planes(src[p:p + 1].contiguous(), m, method, 0.25) for p in range(3)]
        assert torch.equal(torch.cat([s[0] for s in singles]).view(torch.int32), first.view(torch.int32))
        assert [sum(s[1][k] for s in singles) for k in (0, 1)] == stats[:2] and all(s[1][2] == stats[2] for s in singles)
    lab = torch.from_numpy(N.label_raster(70, 129, seed=11)).to(DEV)
    for method in N.LABEL_METHODS:
        first, stats = _labels(lab, m, method)
        again, stats2 = _labels(lab, m, method)
        assert torch.equal(first, again) and stats == stats2


def test_the_kernel_on_an_integer_shift_is_the_slice_of_warp():
    """warp() launches nothing for a whole-cell shift and returns a slice; the kernels, asked directly, give the same bits"""
    m = N.Map(-2.0, 1.0, 3.0, 1.0, 65, 33, 70, 29)
    host = N.float_raster(33, 65, "random", planes=3, seed=12)
    host[0, 5, 7] = -0.0
    src = torch.from_numpy(host).to(DEV)
    a, b = W.Lattice(1000.0, 2000.0, 0.5, 0.5, 65, 33), W.Lattice(999.0, 1998.5, 0.5, 0.5, 70, 29)
    wm = W.warp_map(a, b)
    assert (wm.off_x, wm.step_x, wm.off_y, wm.step_y) == (-2.0, 1.0, 3.0, 1.0)
    sliced, slice_stats = W.warp(src, a, b, return_stats=True)
    for method in N.FLOAT_METHODS:
        got, stats = _planes(src, m, method)
        assert torch.equal(got.view(torch.int32), sliced.view(torch.int32)) and stats == slice_stats, NAMES[method]
    lab = torch.from_numpy(N.label_raster(33, 65, seed=12)).to(DEV)
    sliced, slice_stats = W.warp(lab, a, b, return_stats=True)
    for method in N.LABEL_METHODS:
        got, stats = _labels(lab, m, method)
        assert torch.equal(got, sliced) and stats == slice_stats, NAMES[method]


# ---- the ground truth, end to end -------------------------------------------------------------------------------------------------------------
def _as_map(wm):
    return N.Map(wm.off_x, wm.step_x, wm.off_y, wm.step_y, wm.src_w, wm.src_h, wm.dst_w, wm.dst_h)


def test_a_ground_truth_at_another_resolution(tmp_path):
    """a DSM on a 1 m lattice whose corner lies 0.25 m off the 0.5 m ROI lattice, and a class raster beside it"""
    rng = np.random.default_rng(21)
    jj, ii = np.mgrid[0:40, 0:44]
    gt = (20.0 + 0.3 * ii - 0.2 * jj + rng.normal(0.0, 0.5, (40, 44))).astype(np.float32)
    gt[5:8, 10:14] = np.nan
    cls = rng.choice(np.array([2, 5, 9, 17], np.uint8), (40, 44))
    lidar = D.DsmGrid(354000.25, 4100039.75, 1.0, 44, 40)
    tif, cls_fp, txt = str(tmp_path / "gt.tif"), str(tmp_path / "cls.tif"), str(tmp_path / "roi.txt")
    img_utils.save_geotiff(tif, gt, lidar)
    img_utils.save_geotiff(cls_fp, cls, lidar)
    with open(txt, "w") as f:
        f.write("354002.0\n4100003.0\n64\n0.5\n")
    with pytest.raises(ValueError, match="resampling is not supported"):
        img_utils.load_dsm_ground_truth(tif, txt, cls_fp)
    roi = D.roi_grid([354002.0, 4100003.0, 64, 0.5])
    m = _as_map(W.warp_map(lidar, roi))
    assert (m.off_x, m.step_x, m.off_y, m.step_y) == (1.75, 0.5, 4.75, 0.5) and (m.dst_w, m.dst_h) == (64, 64)
    out = img_utils.load_dsm_ground_truth(tif, txt, cls_fp, resample=True)
    assert not out["gt"].is_cuda and out["gt"].dtype == torch.float32 and out["water_mask"].dtype == torch.uint8
    want, _ = N.warp_planes(gt, m, N.BILINEAR)
    assert np.array_equal(out["gt"].numpy().view(np.uint32), want[0].view(np.uint32)) and np.isnan(want).any() and np.isfinite(want).any()
    assert np.array_equal(out["water_mask"].numpy(), N.warp_labels(cls, m, N.NEAREST)[0]) and out["roi"].tolist() == [354002.0, 4100003.0, 64.0, 0.5]
    named = img_utils.load_dsm_ground_truth(tif, txt, None, ignore_mask_fp=cls_fp, resample="nearest", device=DEV)
    assert np.array_equal(named["gt"].numpy().view(np.uint32), N.warp_planes(gt, m, N.NEAREST)[0][0].view(np.uint32))
    assert np.array_equal(named["ignore_mask"].numpy(), out["water_mask"].numpy()) and "water_mask" not in named


def test_mae_between_two_lattices():
    """a prediction at 0.25 m against a ground truth at 0.5 m that is its 2 x 2 block mean: the MAE of the warped prediction, which
    is that of compute_mae on the prediction warped beforehand, and zero up to the float32 rounding of the block mean"""
    rng = np.random.default_rng(22)
    jj, ii = np.mgrid[0:96, 0:112]
    pred = (30.0 + 4.0 * np.sin(ii / 9.0) * np.cos(jj / 7.0) + rng.normal(0.0, 0.2, (96, 112))).astype(np.float32)
    fine, coarse = D.DsmGrid(354000.0, 4100000.0, 0.25, 112, 96), D.DsmGrid(354000.0, 4100000.0, 0.5, 56, 48)
    gt = pred.astype(np.float64).reshape(48, 2, 56, 2).mean(axis=(1, 3)).astype(np.float32)
    mask = np.zeros((48, 56), np.uint8)
    mask[10:14, 20:30] = 9
    p, g, w = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(mask).to(DEV)
    got = W.mae_between(p, fine, g, coarse, water_mask=w)
    warped = W.warp(p, fine, coarse)
    assert np.array_equal(_bits(warped), N.warp_planes(pred, _as_map(W.warp_map(fine, coarse)), N.AVERAGE)[0][0].view(np.uint32))
    want = D.compute_mae(warped, g, water_mask=w)
    assert (got["mean"], got["median"], got["dx"], got["dy"], got["b"]) == (want["mean"], want["median"], want["dx"], want["dy"], want["b"])
    assert torch.equal(got["diff"].view(torch.int32), want["diff"].view(torch.int32))
    print(f"mae_between: mean {got['mean']:.3e}, shift ({got['dx']}, {got['dy']})")
    assert (got["dx"], got["dy"]) == (0, 0) and got["mean"] < 1e-5 and torch.isnan(got["diff"][10:14, 20:30]).all()
    with pytest.raises(ValueError, match="differ in shape"):
        D.compute_mae(p, g)


# ---- the exports with a reference on a lattice of its own -------------------------------------------------------------------------------------
GRID = D.DsmGrid(500000.0, 4100000.0, 0.5, 129, 70)
COARSE = D.DsmGrid(500000.0, 4100000.0, 1.0, 65, 35)


def _town():
    alt, boxes, ground, mask = TN.town(0.0)
    ref = np.pad(alt, ((0, 0), (0, 1)), mode="edge").reshape(35, 2, 65, 2).max(axis=(1, 3)).astype(np.float32)      # a 1 m DSM of the town
    ref_label = np.pad(np.where(mask, 3, 0).astype(np.uint8), ((0, 0), (0, 1)), mode="edge")[::2, ::2].copy()
    return alt, np.where(mask, 3, 0).astype(np.uint8), ref, ref_label


def test_export_terrain_with_a_reference_at_half_the_resolution(tmp_path):
    alt, label, ref, ref_label = _town()
    products = {"dsm": torch.from_numpy(alt).to(DEV), "grid": GRID}
    coarse = {"alt": torch.from_numpy(ref).to(DEV)}
    with pytest.raises(ValueError, match=r"\(70, 129\).*\(35, 65\)"):
        EO.export_terrain(products, str(tmp_path / "no"), reference=coarse, **TN.TOWN_SCHEDULE)
    assert not os.path.exists(str(tmp_path / "no"))
    out = EO.export_terrain(products, str(tmp_path / "a"), reference=coarse, reference_grid=COARSE, **TN.TOWN_SCHEDULE)
    warped = {"alt": W.warp(coarse["alt"], COARSE, GRID)}
    assert tuple(warped["alt"].shape) == (70, 129) and torch.isfinite(warped["alt"]).all()
    same = EO.export_terrain(products, str(tmp_path / "b"), reference=warped, **TN.TOWN_SCHEDULE)
    assert set(out["files"]) == set(same["files"]) and "terrain_eval.json" in out["files"]
    assert sorted(os.listdir(str(tmp_path / "a" / "terrain"))) == sorted(os.listdir(str(tmp_path / "b" / "terrain"))) == sorted(out["files"])
    assert open(out["files"]["terrain_eval.json"], "rb").read() == open(same["files"]["terrain_eval.json"], "rb").read()
    assert json.load(open(out["files"]["terrain_eval.json"]))["cells"] == 70 * 129
    named = EO.export_terrain(products, str(tmp_path / "c"), reference=coarse, reference_grid=COARSE, reference_resample="nearest",
                              **TN.TOWN_SCHEDULE)
    nearest = N.warp_planes(ref, _as_map(W.warp_map(COARSE, GRID)), N.NEAREST)[0][0]
    want = EO.export_terrain(products, str(tmp_path / "d"), reference={"alt": torch.from_numpy(nearest).to(DEV)}, **TN.TOWN_SCHEDULE)
    assert named["eval"] == want["eval"]


def test_export_objects_with_a_reference_at_half_the_resolution(tmp_path):
    alt, label, ref, ref_label = _town()
    products = {"dsm": torch.from_numpy(alt).to(DEV), "label": torch.from_numpy(label).to(DEV), "grid": GRID}
    coarse = {"alt": torch.from_numpy(ref).to(DEV), "label": torch.from_numpy(ref_label).to(DEV)}
    with pytest.raises(ValueError, match=r"\(70, 129\).*\(35, 65\)"):
        EO.export_objects(products, str(tmp_path / "no"), reference=coarse)
    out = EO.export_objects(products, str(tmp_path / "a"), reference=coarse, reference_grid=COARSE)
    warped = {"alt": W.warp(coarse["alt"], COARSE, GRID), "label": W.warp(coarse["label"], COARSE, GRID)}
    assert np.array_equal(warped["label"].cpu().numpy(), N.warp_labels(ref_label, _as_map(W.warp_map(COARSE, GRID)), N.NEAREST)[0])
    same = EO.export_objects(products, str(tmp_path / "b"), reference=warped)
    assert set(out["files"]) == set(same["files"]) and "objects_eval.json" in out["files"]
    for name in ("objects_eval.json", "reference_objects.json", "objects.json"):
        assert open(out["files"][name], "rb").read() == open(same["files"][name], "rb").read(), name
    assert out["reference"]["n"] == same["reference"]["n"] >= 1 and out["eval"] == same["eval"]
