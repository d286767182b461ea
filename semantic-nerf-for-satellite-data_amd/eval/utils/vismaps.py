"""Streaming visualisation maps of one image on the device (csrc/vismaps.hip): the planes the reference's visualisers make from
the whole frame's (N, S, .) tensors -- sum(weights[..., None] * factor, -2) of framework/visualize.py's callers
(baseline/components/visualize.py FactorVisualization, semantic/components/visualize.py SemanticColorShadingVisualization), the
RGB differences, the coloured label map and the label error -- folded chunk by chunk as lean_semantic_eval folds the metrics:
render a chunk into chunk-sized buffers, fold it into the frame's planes (include/snerf_hip.h snerf_vis_fold), keep nothing per
sample.  The stats block (exact min / max of every scalar plane, the count of labels outside the palette) stays on the device;
the colormap (visualize_image_numpy, snerf_vis_colormap) reads its bounds there, so nothing is read back between fold and image."""
import ctypes as C

import numpy as np
import torch

from ... import _lib, parallel
from ...framework.components.coordinate_systems import key_to_double
from ...framework.components.rendering import n_render_samples

# product -> (render results it needs, per-ray inputs it needs)
PRODUCTS = {
    "rgb": (("rgb",), ()), "depth": (("depth",), ()),
    "albedo": (("weights", "albedo"), ()), "sun": (("weights", "sun"), ()), "sky": (("weights", "sky"), ()),
    "beta": (("weights", "beta"), ()), "beta_semantic": (("weights", "beta_semantic"), ()),
    "rgb_diff": (("rgb",), ("rgbs",)), "rgb_diff_distance": (("rgb",), ("rgbs",)),
    "sem_color": (("semantic_label",), ("palette",)), "sem_shaded": (("semantic_label", "weights", "sun"), ("palette",)),
    "sem_error": (("semantic_label",), ("semantic",)),
}
SEMANTIC_PRODUCTS = ("sem_color", "sem_shaded", "sem_error")
BASELINE_PRODUCTS = ("rgb", "depth", "albedo", "sun", "sky", "beta", "rgb_diff", "rgb_diff_distance")
# product -> (plane of SnerfVisOut, bands, dtype); "rgb" is the per-ray result itself, kept (n, 3)
_PLANES = {"depth": ("depth_map", 1, torch.float32), "albedo": ("albedo_map", 3, torch.float32),
           "sun": ("sun_map", 1, torch.float32), "sky": ("sky_map", 3, torch.float32), "beta": ("beta_map", 1, torch.float32),
           "beta_semantic": ("beta_semantic_map", 1, torch.float32), "rgb_diff": ("rgb_diff", 3, torch.float32),
           "rgb_diff_distance": ("rgb_diff_distance", 1, torch.float32), "sem_color": ("sem_color", 3, torch.uint8),
           "sem_shaded": ("sem_shaded", 3, torch.uint8), "sem_error": ("sem_error", 1, torch.float32)}
SLOT = dict(_lib.VIS_SLOT)                       # product of a scalar fp32 plane -> its slot of the stats block
_NWORDS = C.sizeof(_lib.SnerfVisStats) // 8
_BAD = 2 * _lib.VIS_SLOTS                        # word of bad_labels
_SIGN = -(2 ** 63)


def new_stats(device) -> torch.Tensor:
    """a zeroed SnerfVisStats as int64 words"""
    return torch.zeros(_NWORDS, dtype=torch.int64, device=device)


def decode_stats(words) -> dict:
    """host copy of the stats words -> {"bounds": {slot name: (min, max) or None}, "bad_labels": int}"""
    w = np.asarray(words).astype(np.int64).view(np.uint64)
    out = {}
    for name, s in SLOT.items():
        lo, hi = int(w[2 * s]), int(w[2 * s + 1])
        out[name] = (key_to_double((~lo) & (2 ** 64 - 1)), key_to_double(hi)) if lo and hi else None
    return {"bounds": out, "bad_labels": int(w[_BAD])}


def fold_chunk(planes: dict, stats: torch.Tensor, row0: int, n: int, m: int, S: int, **inputs):
    """one snerf_vis_fold launch: `inputs` by SnerfVisIn field name (tensors or None), `planes` by SnerfVisOut field name (the
    frame's planes, (bands, n) or (n,)), rows [row0, row0 + m).  Asynchronous on the current stream."""
    vin, vout = _lib.SnerfVisIn(), _lib.SnerfVisOut()
    keep = []
    for k, t in inputs.items():
        if k not in _lib.VIS_IN_FIELDS:
            raise KeyError(f"fold_chunk: unknown input '{k}'")
        if t is None:
            continue
        want = (torch.int64,) if k == "label" else (torch.uint8,) if k == "palette" else (torch.uint8, torch.int64) if k == "semantic_gt" else (torch.float32,)
        if not t.is_cuda or t.dtype not in want:
            raise ValueError(f"fold_chunk: '{k}' must be a GPU tensor of {want}, not {t.dtype} on {t.device}")
        per = {"weights": S, "albedo": 3 * S, "sky": 3 * S, "sun": S, "beta": S, "beta_semantic": S, "rgb": 3, "rgbs_gt": 3}.get(k, 1)
        if k != "palette" and t.numel() != m * per:
            raise ValueError(f"fold_chunk: '{k}' has {t.numel()} elements for {m} rays (x {per})")
        t = t.contiguous()
        keep.append(t)
        setattr(vin, k, t.data_ptr())
    pal, gt = inputs.get("palette"), inputs.get("semantic_gt")
    if pal is not None:
        if pal.dim() != 2 or pal.shape[1] != 3:
            raise ValueError("palette must be (K, 3) uint8")
        vin.n_palette = pal.shape[0]
    if gt is not None:
        vin.gt_dtype = _lib.VIS_I64 if gt.dtype == torch.int64 else _lib.VIS_U8
    for k, t in planes.items():
        if k not in _lib.VIS_OUT_FIELDS:
            raise KeyError(f"fold_chunk: unknown plane '{k}'")
        if t is None:
            continue
        bands = 3 if k in ("albedo_map", "sky_map", "rgb_diff", "sem_color", "sem_shaded") else 1
        dt = torch.uint8 if k in ("sem_color", "sem_shaded") else torch.float32
        if not t.is_cuda or t.dtype != dt or t.numel() != bands * n or not t.is_contiguous():
            raise ValueError(f"fold_chunk: plane '{k}' must be a contiguous {dt} GPU tensor of {bands} x {n}")
        setattr(vout, k, t.data_ptr())
    if stats.dtype != torch.int64 or stats.numel() != _NWORDS or not stats.is_cuda:
        raise ValueError("stats must come from new_stats()")
    _lib.call("snerf_vis_fold", vin, vout, m, S, row0, n, stats, device=stats.device, exc=ValueError)
    del keep


def _plane_dtype(plane):
    if plane.dtype == torch.float32:
        return _lib.VIS_F32
    if plane.dtype == torch.float64:
        return _lib.VIS_F64
    raise ValueError(f"a scalar plane is fp32 or fp64, not {plane.dtype}")


def plane_minmax(plane: torch.Tensor, stats: torch.Tensor, slot="user"):
    """fold the exact nan_to_num min / max of `plane` into a slot of the stats block (snerf_vis_minmax)"""
    p = plane.reshape(-1).contiguous()
    _lib.call("snerf_vis_minmax", p, _plane_dtype(p), p.numel(), stats, SLOT[slot] if isinstance(slot, str) else int(slot),
              exc=ValueError)
    return stats


def colormap(plane: torch.Tensor, table: torch.Tensor, stats: torch.Tensor = None, slot=None, cmap_bounds=None) -> torch.Tensor:
    """visualize_image_numpy on the device: (..., ) fp32 / fp64 plane -> (3, ...) uint8 through the (256, 3) uint8 `table`.
    Bounds: explicit `cmap_bounds` (mi, ma), else the `slot` of `stats`, else the plane's own (folded into a fresh block here)."""
    shape = tuple(plane.shape)
    p = plane.reshape(-1).contiguous()
    if table.shape != (256, 3) or table.dtype != torch.uint8:
        raise ValueError("the colour table is (256, 3) uint8")
    out = torch.empty((3,) + shape, dtype=torch.uint8, device=p.device)
    lo = hi = 0.0
    if cmap_bounds is not None:
        lo, hi = float(cmap_bounds[0]), float(cmap_bounds[1])
        s, stats = -1, None
    else:
        if stats is None or slot is None:
            stats, slot = plane_minmax(p, new_stats(p.device), "user"), "user"
        s = SLOT[slot] if isinstance(slot, str) else int(slot)
    _lib.call("snerf_vis_colormap", p, _plane_dtype(p), p.numel(), stats, s, lo, hi, table.contiguous(), out, exc=ValueError)
    return out


class FrameMaps:
    """the planes of one image: `planes[product]` ((3, n) or (n,) planar; "rgb" (n, 3) as rendered), `stats` (device words of
    SnerfVisStats), `n` rays.  Nothing is read back until decode() / check_labels()."""

    def __init__(self, planes, stats, n):
        self.planes, self.stats, self.n = planes, stats, n

    def __contains__(self, product):
        return product in self.planes

    def __getitem__(self, product):
        return self.planes[product]

    def decode(self) -> dict:
        return decode_stats(self.stats.cpu().numpy())

    def check_labels(self):
        bad = self.decode()["bad_labels"]
        if bad:
            raise ValueError(f"{bad} rays have a label outside the palette")
        return self


def _needs(products, model, rgbs, semantic, palette):
    spec = model.spec
    keys, unknown = [], [p for p in products if p not in PRODUCTS]
    if unknown:
        raise KeyError(f"lean_frame_maps: unknown products {unknown} (known: {sorted(PRODUCTS)})")
    given = {"rgbs": rgbs, "semantic": semantic, "palette": palette}
    for p in products:
        if p in SEMANTIC_PRODUCTS and spec.n_classes == 0:
            raise ValueError(f"'{p}' needs a semantic head: the model has none (n_classes = 0)")
        if p == "beta_semantic" and not getattr(spec, "use_separate_beta_for_s", False):
            raise ValueError("'beta_semantic' needs a model with use_separate_beta_for_s")
        for k in PRODUCTS[p][0]:
            if k not in keys:
                keys.append(k)
        for a in PRODUCTS[p][1]:
            if given[a] is None:
                raise ValueError(f"'{p}' needs the argument `{a}`")
    return keys


@torch.no_grad()
def lean_frame_maps(cfgs, renderer, models, rays, extras, rgbs=None, semantic=None, palette=None, products=BASELINE_PRODUCTS,
                    render_options={}):
    """Render the frame `rays` chunk by chunk (util.render_chunks, as lean_semantic_eval: the same per-chunk jitter from the same
    RNG state, chunk-sized result buffers allocated once) and fold every chunk into the frame's planes of the requested
    `products` (PRODUCTS).  Only the per-sample results a requested product needs are rendered; no (N, S) tensor of the frame
    exists.  rgbs (n, 3) fp32, semantic (n,) / (n, 1) uint8 or int64 and palette (K, 3) uint8 are needed by the products that
    read them.  Returns a FrameMaps; nothing is read back."""
    from ... import ops
    from .util import render_chunks, result_buffers
    model = models["coarse"]
    products = tuple(products)
    keys = _needs(products, model, rgbs, semantic, palette)
    n, dev = rays.shape[0], rays.device
    S, Cn = n_render_samples(cfgs.pipeline), model.spec.n_classes
    for t, what in ((rgbs, "rgbs"), (semantic, "semantic")):
        if t is not None and t.shape[0] != n:
            raise ValueError(f"{what} has {t.shape[0]} rows for {n} rays")
    if semantic is not None and semantic.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"semantic must be uint8 or int64, not {semantic.dtype}")
    ops.release_workspaces()
    bufs = result_buffers(keys, min(cfgs.pipeline.render_chunk_size, n), S, Cn, dev)
    planes = {}
    for p in products:
        if p == "rgb":
            planes[p] = torch.empty((n, 3), dtype=torch.float32, device=dev)
        else:
            _, bands, dt = _PLANES[p]
            planes[p] = torch.empty((bands, n) if bands > 1 else (n,), dtype=dt, device=dev)
    out = {_PLANES[p][0]: v for p, v in planes.items() if p != "rgb"}
    stats = new_stats(dev)
    want = lambda *ps: any(p in products for p in ps)           # noqa: E731
    pal = palette.to(dev).contiguous() if palette is not None and want("sem_color", "sem_shaded") else None
    sem = semantic.reshape(-1) if semantic is not None and want("sem_error") else None
    gt_rgb = rgbs if want("rgb_diff", "rgb_diff_distance") else None
    for i, k, sl in render_chunks(cfgs, renderer, models, rays, extras, bufs, render_options):
        g = lambda key: sl.get(key + "_coarse")                  # noqa: E731
        if "rgb" in planes:
            planes["rgb"][i:i + k].copy_(g("rgb"))
        if out:
            fold_chunk(out, stats, i, n, k, S, weights=g("weights"),
                       albedo=g("albedo") if want("albedo") else None, sun=g("sun"), sky=g("sky") if want("sky") else None,
                       beta=g("beta") if want("beta") else None, beta_semantic=g("beta_semantic"),
                       depth=g("depth") if want("depth") else None, rgb=g("rgb") if gt_rgb is not None else None,
                       rgbs_gt=gt_rgb[i:i + k] if gt_rgb is not None else None,
                       label=g("semantic_label"), semantic_gt=sem[i:i + k] if sem is not None else None, palette=pal)
    return FrameMaps(planes, stats, n)


def allreduce_stats_(stats: torch.Tensor) -> torch.Tensor:
    """combine the ranks' stats blocks on the device: the min / max words are unsigned keys whose order a flip of the top bit
    turns into int64 order, so one MAX all-reduce serves; bad_labels by a SUM.  Single process: nothing."""
    if parallel.world()[1] == 1:
        return stats
    import torch.distributed as dist
    keys = stats[:_BAD] ^ _SIGN
    parallel.allreduce_(keys, op=dist.ReduceOp.MAX)
    bad = stats[_BAD:_BAD + 1].clone()
    parallel.allreduce_sum_(bad)
    stats[:_BAD].copy_(keys ^ _SIGN)
    stats[_BAD:_BAD + 1].copy_(bad)
    return stats


@torch.no_grad()
def sharded_lean_frame_maps(cfgs, renderer, models, rays, extras, rgbs=None, semantic=None, palette=None,
                            products=BASELINE_PRODUCTS, render_options={}):
    """lean_frame_maps with the frame's rays sharded over the process group, as sharded_lean_inference: every rank folds rows
    frame_shard(n), the planes are all-gathered (one all_gather per plane) and the stats combined by allreduce_stats_, so every
    rank holds the frame's planes and bounds -- bit-equal to one process (a ray's values do not depend on its chunk)."""
    from .util import shard_options
    n, dev = rays.shape[0], rays.device
    products = tuple(products)
    _needs(products, models["coarse"], rgbs, semantic, palette)
    lo, hi = parallel.frame_shard(n)
    cut = lambda t: t[lo:hi] if t is not None else None         # noqa: E731
    if hi > lo:
        local = lean_frame_maps(cfgs, renderer, models, rays[lo:hi], cut(extras), cut(rgbs), cut(semantic), palette, products,
                                shard_options(render_options, lo, hi, n))
        planes, stats = local.planes, local.stats
    else:        # more ranks than rays
        planes, stats = {}, new_stats(dev)
        for p in products:
            bands, dt = (3, torch.float32) if p == "rgb" else _PLANES[p][1:]
            planes[p] = torch.empty((0, 3) if p == "rgb" else (bands, 0) if bands > 1 else (0,), dtype=dt, device=dev)
    full = {}
    for p, v in planes.items():
        if p == "rgb" or v.dim() == 1:
            full[p] = parallel.allgather_rows(v, n)
        else:
            full[p] = parallel.allgather_rows(v.t().contiguous(), n).t().contiguous()
    return FrameMaps(full, allreduce_stats_(stats), n)
