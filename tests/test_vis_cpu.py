"""Visualisation maps without a GPU: the numpy restatement (tests/vis_ref.py) against the fixtures the reference's own visualisers
made (tests/golden/vis_*.npz, tools/gen_golden_vis.py), the binding table's rows against the header, the visualiser lists of
the pipelines, and run_visualizer's split / index rule and output paths."""
import os
import re

import numpy as np
import pytest

from tests import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("vis_5x7_s3", "vis_16x17_s64", "vis_9x29_s65")
SUMS = ("albedo", "sun", "sky", "beta", "beta_semantic")
CMAPS = ("sun", "beta", "depth", "rgb_diff_distance", "sem_error", "alts")


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def planar(ref):
    """the reference's (3, H, W) / (H, W) map -> (3, n) / (n,)"""
    return ref.reshape(3, -1) if ref.ndim == 3 else ref.reshape(-1)


def check_maps_against_fixture(z, got, report=None):
    """`got`: {product: planar array} -- weighted sums within the derived bound, everything else exact (rgb_diff_distance: 2 ulp)"""
    for k in SUMS:
        if k not in got:
            continue
        ref, bound = planar(z[f"ref_{k}"]).astype(np.float64), R.sum_bound(z["weights"], z[k])
        err = np.abs(got[k].astype(np.float64) - ref)
        if report is not None:
            report[k] = float((err / bound).max())
        assert (err <= bound).all(), (k, float((err / bound).max()))
    for k in ("rgb_diff", "sem_color", "sem_error", "sem_shaded"):
        if k in got:
            assert np.array_equal(got[k], planar(z[f"ref_{k}"])), k
    if "rgb_diff_distance" in got:
        ref = planar(z["ref_rgb_diff_distance"])
        assert (np.abs(got["rgb_diff_distance"].astype(np.float64) - ref) <= 2 * np.spacing(ref)).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_maps(name):
    z = load(name)
    w = z["weights"]
    got = {k: R.weighted_sum(w, z[k]) for k in SUMS}
    got["rgb_diff"] = R.rgb_diff(z["rgb"], z["rgbs"])
    got["rgb_diff_distance"] = R.rgb_diff_distance(z["rgb"], z["rgbs"])
    got["sem_color"], bad = R.sem_color(z["label"], z["palette"])
    got["sem_shaded"] = R.sem_shaded(z["label"], z["palette"], got["sun"])
    got["sem_error"] = R.sem_error(z["label"], z["semantic"])
    assert bad == 0
    check_maps_against_fixture(z, got)
    H, W = int(z["h"]), int(z["w"])
    assert z["ref_albedo"].shape == (3, H, W) and z["ref_sun"].shape == (H, W) and z["ref_sem_shaded"].dtype == np.uint8
    assert np.array_equal(z["ref_rgb"], z["rgb"].reshape(H, W, 3).transpose(2, 0, 1)) and np.array_equal(z["ref_depth"].ravel(), z["depth"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_colormap_indices(name):
    z = load(name)
    for k in CMAPS:
        plane = z[f"cmap_{k}"]
        assert plane.dtype == (np.float64 if k == "alts" else np.float32)
        assert np.array_equal(R.colormap_index(plane), z[f"idx_{k}"]), k
        assert np.array_equal(R.colormap_index(plane, tuple(z[f"bounds_{k}"])), z[f"idxb_{k}"]), k
        assert z[f"idx_{k}"].min() == 0 and z[f"idx_{k}"].max() >= 254


def test_restatement_nan_inf_constant_and_bad_labels():
    z = load("vis_nan_const")
    for dt in ("float32", "float64"):
        for k in (f"nan_{dt}", f"const_{dt}", f"zero_{dt}"):
            assert z[f"cmap_{k}"].dtype == np.dtype(dt)
            assert np.array_equal(R.colormap_index(z[f"cmap_{k}"]), z[f"idx_{k}"]), k
        assert np.array_equal(R.colormap_index(z[f"cmap_const_{dt}"], (0.0, 1.0)), z[f"idxb_const_{dt}"])
        assert (z[f"idx_const_{dt}"] == 0).all() and (z[f"idxb_const_{dt}"] == 95).all()          # trunc(255 * 0.375)
        p = z[f"cmap_nan_{dt}"]
        assert np.isnan(p).sum() == 1 and np.isinf(p).sum() == 1
        lo, hi = R.minmax(p)
        assert hi == float(np.finfo(p.dtype).max) and lo == float(np.nanmin(p))
    b = load("vis_badlabel")
    col, bad = R.sem_color(b["label"], b["palette"])
    assert bad == 3 and (col[:, [3, 10, 17]] == 0).all() and (col[:, 0] == b["palette"][b["label"][0]]).all()


def _header_counts():
    src = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"\b(snerf_vis_[a-z_]+)\s*\(([^()]*)\)\s*;", src)}


def test_binding_table_has_the_vis_entries():
    import ctypes as C
    from snerf_amd import _lib
    counts = _header_counts()
    assert set(counts) == {"snerf_vis_fold", "snerf_vis_minmax", "snerf_vis_colormap"}
    for name, n in counts.items():
        restype, args = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(args) == n and args[-1] is _lib.c_stream, name
        assert hasattr(_lib.lib(), name)
    assert C.sizeof(_lib.SnerfVisIn) == 12 * 8 + 8 and C.sizeof(_lib.SnerfVisOut) == 11 * 8
    assert C.sizeof(_lib.SnerfVisStats) == (2 * _lib.VIS_SLOTS + 8) * 8
    L = _lib.lib()
    assert L.snerf_vis_fold(None, None, 0, 1, 0, 0, None, None) != 0 and b"null" in L.snerf_last_error()
    vin, vout = _lib.SnerfVisIn(), _lib.SnerfVisOut()
    stats = (C.c_uint64 * 24)()
    assert L.snerf_vis_fold(C.byref(vin), C.byref(vout), 5, 1, 3, 7, stats, None) != 0 and b"outside a frame" in L.snerf_last_error()
    vin.sun = 16
    assert L.snerf_vis_fold(C.byref(vin), C.byref(vout), 5, 1, 0, 7, stats, None) != 0 and b"need weights" in L.snerf_last_error()
    vin.weights = 16
    assert L.snerf_vis_fold(C.byref(vin), C.byref(vout), 5, 2000, 0, 7, stats, None) != 0 and b"n_samples" in L.snerf_last_error()
    assert L.snerf_vis_fold(C.byref(vin), C.byref(vout), 0, 8, 0, 7, stats, None) == 0                    # no rays: nothing launched
    assert L.snerf_vis_colormap(16, 7, 5, stats, 0, 0.0, 1.0, 16, 16, None) != 0 and b"dtype" in L.snerf_last_error()
    assert L.snerf_vis_colormap(16, 0, 5, None, 0, 0.0, 1.0, 16, 16, None) != 0
    assert L.snerf_vis_minmax(16, 0, 5, stats, 8, None) != 0 and b"slot" in L.snerf_last_error()


def test_create_visualizers_names():
    from snerf_amd.baseline.pipelines.satnerf import SatNeRFPipeline
    from snerf_amd.semantic.pipelines.rs_semantic import RSSemanticPipeline
    from snerf_amd.eval.utils.vismaps import PRODUCTS
    base = ["rgb", "depth", "albedo", "sun", "beta", "RGB_Diff_Distance"]
    assert [v._name() for v in SatNeRFPipeline.create_visualizers(None)] == base
    sem = RSSemanticPipeline.create_visualizers(None)
    assert [v._name() for v in sem] == base + ["semantic_rendering", "semantic_error", "semantic_rendering_shaded"]
    assert all(p in PRODUCTS for v in sem for p in v.products) and all(v.products for v in sem)


def test_split_index_rule_and_paths():
    from snerf_amd.framework.visualize import output_path, split_and_index, to_uint8_image
    import torch
    assert split_and_index("test", 0) == ("train", 0)               # the first test image is the first train image
    assert split_and_index("test", 1) == ("test", 0) and split_and_index("test", 5) == ("test", 4)
    assert split_and_index("train", 0) == ("train", 0) and split_and_index("train", 3) == ("train", 3)
    assert output_path("/x/run", "train", "sun", "JAX_068_013_RGB", -1) == "/x/run/visualization/train/sun/JAX_068_013_RGB_-1.png"
    x = np.array([[[0.0, 0.5, 1.0, 0.999, 0.25]]] * 3, np.float32)
    assert np.array_equal(to_uint8_image(torch.from_numpy(x)).numpy(), R.to_uint8_image(x))
    assert R.to_uint8_image(x)[0, 0].tolist() == [0, 128, 255, 255, 64]


def test_colour_tables():
    from snerf_amd.framework.util import colormaps as cm
    for t in cm.TABLES.values():
        assert t.shape == (256, 3) and t.dtype == np.uint8
    jet, bone = cm.TABLES[cm.COLORMAP_JET], cm.TABLES[cm.COLORMAP_BONE]
    # band 0 of the written image is the map's blue: jet starts blue (band 0 high) and ends red (band 2 high)
    assert jet[0, 0] > 100 and jet[0, 2] == 0 and jet[255, 2] > 100 and jet[255, 0] == 0
    assert bone[0].tolist() == [0, 0, 0] and bone[255].tolist() == [255, 255, 255] and (np.diff(bone.astype(int), axis=0) >= 0).all()
    assert cm.DEFAULT_PALETTE.shape == (6, 3) and cm.DEFAULT_PALETTE.dtype == np.uint8
