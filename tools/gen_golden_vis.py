#!/usr/bin/env python3
"""Generate the golden vectors of the visualisation maps by running the REFERENCE's own `_visualize` methods
(baseline/components/visualize.py, semantic/components/visualize.py) and framework/util/other.py visualize_image_numpy on
synthetic result dicts.

Run where the reference is (it never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_vis.py

The reference's import chain is stubbed as in tools/gen_golden_semeval.py (every missing package is an inert module), with one
difference: cv2.applyColorMap returns its index array, so the fixtures pin the QUANTISATION (nan_to_num, the normalisation, the
truncation) and not OpenCV's colour tables, which are not installed (parity with cv2's tables is UNPINNED).

Writes tests/golden/vis_<case>.npz.  Inputs: weights (N, S), albedo / sky (N, S, 3), sun / beta / beta_semantic (N, S, 1), rgb, rgbs
(N, 3), depth (N,), label (N,) int64, semantic (N, 1) uint8, palette (K, 3) uint8 -- the palette the reference used, recorded as
an input -- and h, w.  Expected (the reference's outputs, as it shapes them): ref_albedo, ref_sky (3, H, W), ref_sun, ref_beta,
ref_beta_semantic, ref_depth (H, W), ref_rgb (3, H, W), ref_rgb_diff (3, H, W), ref_rgb_diff_distance (H, W), ref_sem_color,
ref_sem_shaded (3, H, W) uint8, ref_sem_error (H, W), and idx_<plane> (H, W) uint8: visualize_image_numpy's index of the plane
cmap_<plane> (a copy of the reference's map, or a synthetic one), with idxb_<plane> / bounds_<plane> for explicit cmap_bounds.
Cases: (H, W, S, C) = (5, 7, 3, 6), (16, 17, 64, 6), (9, 29, 65, 2); `nan` (a NaN and a +inf in a scalar map), `const` (ma == mi),
`badlabel` (a label outside the palette: the reference cannot index it, so that case carries inputs only and is checked against
tests/vis_ref.py).

Truncating products can flip by one where the value before truncation sits on an integer.  sem_shaded is computed from a sum that
the kernel forms in another order than torch, so the generator ASSERTS for every pixel and band that the reference's product
float(palette) * sun is farther from an integer than 255 * (S * 2^-23 * sum |fl32(w_s sun_s)|), and draws another seed otherwise:
the tests can then demand equality with no pixel excluded.  The colormap indices are checked on the recorded cmap_<plane> itself
(the same input bits for both sides), where the arithmetic is restated operation by operation and no margin is needed."""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SNERF_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
CANDIDATES = ("toml", "gpustat", "lightning", "pytorch_lightning", "rasterio", "torchmetrics", "torchvision", "fire", "cv2", "pymap3d",
           "utm", "plyflatten", "affine", "sklearn", "pycocotools", "matplotlib", "seaborn", "shapely", "skimage", "geojson", "srtm4",
           "rpcm", "osgeo", "pyproj", "pandas", "scipy", "tqdm", "kornia", "lpips", "cmcrameri", "numba", "json5", "yaml", "imageio", "tifffile")


STUBBED = ()


class _Inert:
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        return _Inert()

    def __getattr__(self, name):
        return _Inert()


class _StubModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (_Inert,), {})
        setattr(self, name, cls)
        return cls


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUBBED:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _StubModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def load_reference():
    import importlib.util
    global STUBBED
    STUBBED = tuple(m for m in CANDIDATES if importlib.util.find_spec(m) is None)      # only what is not installed
    sys.meta_path.insert(0, _StubFinder())
    import typing
    import torch.utils.data.dataset as tud
    if not hasattr(tud, "T_co"):
        tud.T_co = typing.TypeVar("T_co", covariant=True)
    import cv2
    cv2.COLORMAP_BONE, cv2.COLORMAP_JET = 1, 2
    cv2.applyColorMap = lambda x, cmap: x               # the index array: the table is not pinned
    sys.path.insert(0, REF)
    import framework.util.other as other
    import baseline.components.visualize as vb
    import semantic.components.visualize as vs
    return other, vb, vs


OTHER, VB, VS = load_reference()
from tests import vis_ref as R  # noqa: E402


def synth(rng, H, W, S, C):
    n = H * W
    z = rng.standard_normal((n, S)) * 2.0
    w = (np.exp(z) / np.exp(z).sum(1, keepdims=True) * rng.uniform(0.6, 1.0, (n, 1))).astype(np.float32)
    f = lambda *shape: rng.uniform(0.02, 0.98, shape).astype(np.float32)      # noqa: E731
    label = rng.integers(0, C, n).astype(np.int64)
    gt = np.where(rng.random(n) < 0.7, label, rng.integers(0, C, n)).astype(np.uint8)[:, None]
    return {"weights": w, "albedo": f(n, S, 3), "sun": f(n, S, 1), "sky": f(n, S, 3), "beta": f(n, S, 1) + np.float32(0.05),
            "beta_semantic": f(n, S, 1), "rgb": f(n, 3), "rgbs": f(n, 3), "depth": rng.uniform(0.3, 1.7, n).astype(np.float32),
            "label": label, "semantic": gt, "h": np.int64(H), "w": np.int64(W)}


def run_reference(c, palette):
    """the reference's visualisers on the case's tensors -> {ref_*: array}"""
    H, W = int(c["h"]), int(c["w"])
    t = lambda k: torch.from_numpy(c[k])                 # noqa: E731
    results = {f"{k}_coarse": t(k) for k in ("weights", "albedo", "sun", "sky", "beta", "beta_semantic", "rgb", "depth")}
    results["semantic_label_coarse"] = t("label")
    sample = {"rgbs": t("rgbs"), "semantic": t("semantic"), "h": H, "w": W, "rays": torch.zeros(H * W, 8)}
    VS.SEMANTIC_CLASS_COLOR_MAPPING = torch.from_numpy(palette)
    out = {}
    for name in ("albedo", "sun", "sky", "beta", "beta_semantic", "depth", "rgb"):
        v = VB.FactorVisualization(None, False, False, factor_name=name)
        out[f"ref_{name}"] = v._visualize(None, None, sample, results, W, H, "_coarse").numpy()
    kw = dict(send_to_tensorboard=False, save_as_tif=False)
    for key, v in (("rgb_diff", VB.RGBDiffVisualization(None, **kw)), ("rgb_diff_distance", VB.RGBDiffDistanceVisualization(None, **kw)),
                   ("sem_color", VS.SemanticColorVisualization(None, **kw)), ("sem_shaded", VS.SemanticColorShadingVisualization(None, **kw)),
                   ("sem_error", VS.SemanticErrorVisualization(None, **kw))):
        out[f"ref_{key}"] = v._visualize(None, None, sample, results, W, H, "_coarse").numpy()
    return out


def shaded_margin_ok(c, palette, ref):
    """every pixel and band of sem_shaded: the reference's product before truncation is farther from an integer than the sum
    bound scaled by 255"""
    H, W = int(c["h"]), int(c["w"])
    pre = palette[c["label"]].astype(np.float32) * ref["ref_sun"].reshape(-1, 1).astype(np.float32)       # (n, 3) fp32
    assert np.array_equal(pre.astype(np.uint8).T.reshape(3, H, W), ref["ref_sem_shaded"])
    bound = 255.0 * R.sum_bound(c["weights"], c["sun"])[:, None]
    dist = np.abs(pre.astype(np.float64) - np.rint(pre.astype(np.float64)))
    return bool((dist > bound).all())


def add_cmap(out, name, plane, bounds=None):
    out[f"cmap_{name}"] = plane
    out[f"idx_{name}"] = OTHER.visualize_image_numpy(plane)
    if bounds is not None:
        out[f"bounds_{name}"] = np.array(bounds, np.float64)
        out[f"idxb_{name}"] = OTHER.visualize_image_numpy(plane, cmap_bounds=tuple(float(b) for b in bounds))


def case(seed, H, W, S, C, palette):
    for attempt in range(64):
        rng = np.random.default_rng(seed + 1000 * attempt)
        c = synth(rng, H, W, S, C)
        ref = run_reference(c, palette)
        if shaded_margin_ok(c, palette, ref):
            break
    else:
        raise RuntimeError("no seed keeps sem_shaded off the integers")
    out = dict(c, palette=palette, seed=np.int64(seed + 1000 * attempt), **ref)
    for name in ("sun", "beta", "depth", "rgb_diff_distance", "sem_error"):
        p = ref[f"ref_{name}"]
        lo, hi = float(p.min()), float(p.max())
        add_cmap(out, name, p, bounds=(lo - 0.25 * (hi - lo) - 0.01, hi + 0.5 * (hi - lo) + 0.01))
    alts = (rng.uniform(-25.0, 40.0, (H, W))).astype(np.float64)             # an altitude plane: fp64, as GeoFrame.cloud gives
    add_cmap(out, "alts", alts, bounds=(-30.0, 45.0))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    # the palette the reference used: its own table, read as data and recorded as an input
    import data_prep.prepare_annotations as PA
    ref_palette = np.asarray(PA.SEMANTIC_CLASS_COLOR_MAPPING, np.uint8)
    cases = {"vis_5x7_s3": case(11, 5, 7, 3, 6, ref_palette), "vis_16x17_s64": case(12, 16, 17, 64, 6, ref_palette),
             "vis_9x29_s65": case(13, 9, 29, 65, 2, ref_palette[:2].copy())}
    rng = np.random.default_rng(99)
    nan = {}
    for dt in (np.float32, np.float64):
        p = rng.uniform(-3.0, 5.0, (6, 11)).astype(dt)
        p[2, 3], p[4, 7], p[0, 0] = np.nan, np.inf, -0.0
        with np.errstate(over="ignore", invalid="ignore"):
            add_cmap(nan, f"nan_{np.dtype(dt).name}", p)
        add_cmap(nan, f"const_{np.dtype(dt).name}", np.full((4, 9), 0.375, dt), bounds=(0.0, 1.0))
        add_cmap(nan, f"zero_{np.dtype(dt).name}", np.zeros((3, 5), dt))
    cases["vis_nan_const"] = nan
    bad = synth(np.random.default_rng(5), 4, 6, 5, 4)
    bad["label"][[3, 10, 17]] = (4, 9, -1)                                     # outside a palette of 4 colours
    cases["vis_badlabel"] = dict(bad, palette=ref_palette[:4].copy())
    for name, res in cases.items():
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **res)
        print(name, os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes", "seed", res.get("seed"))


if __name__ == "__main__":
    main()
