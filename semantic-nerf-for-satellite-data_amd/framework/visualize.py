"""Visualisers -- mirror of framework/visualize.py: BaseVisualization, ImageVisualization and the run_visualizer loop.

Where the reference's `_visualize` reads the whole frame's render results (batched_inference: every (N, S, .) tensor of the
image), `results` here is a FrameMaps (eval/utils/vismaps.py): the planes one streaming fold of the image made, shared by every
visualiser of that image.  `_visualize` returns DEVICE tensors built from those planes, in the reference's shapes: (H, W) for a
one-band map, (3, H, W) for three bands.  A visualiser names the products it reads in `products`.

visualize_image_cmap_and_save writes a PNG through PIL: a 2-D map goes through the colormap kernel (visualize_image: nan_to_num,
min / max normalisation, * 255 truncated, the cmap's table; bounds read on the device), a 3-band uint8 map is written as it is,
and a 3-band float map as torchvision's save_image writes it -- x * 255 + 0.5, clamped to [0, 255], uint8.  torchvision is not
part of this build: that rule is RESTATED from torchvision.utils.save_image.  (The reference divides a map whose max exceeds 1
by 255 first; its uint8 maps therefore come back as x / 255 * 255 + 0.5 truncated = x: written as they are.)

OUT OF SCOPE: TensorBoard and the Tensorboard*Summary stacks, .tif writing with RPC tags (`_save`), the confusion
matrix figure."""
import abc
import os

import torch

from .util import colormaps


def w_h_from_sample(sample):
    """framework/util/other.py:55-65: (W, H) from the sample's "w" / "h", else a square frame"""
    if "h" in sample and "w" in sample:
        w, h = sample["w"], sample["h"]
        if isinstance(w, (list, tuple)):
            w, h = w[0], h[0]
    else:
        w = h = int(torch.sqrt(torch.tensor(sample["rays"].reshape(-1, sample["rays"].shape[-1]).shape[0]).float()))
    return int(w), int(h)


class BaseVisualization:
    products = ()          # the lean_frame_maps products the visualiser reads

    def __init__(self, cfgs, send_to_tensorboard: bool) -> None:
        super().__init__()
        self.cfgs = cfgs
        self.send_to_tensorboard = send_to_tensorboard

    @abc.abstractmethod
    def run(self, pipeline, dataset, sample, results, sample_idx: int = 0, split: str = "test", epoch: int = 0,
            source_fp: str = None, logger=None, force_output_fp=None):
        pass


class ImageVisualization(BaseVisualization):
    def __init__(self, cfgs, send_to_tensorboard: bool, save_as_tif: bool) -> None:
        super().__init__(cfgs, send_to_tensorboard)
        self._save_as_tif = save_as_tif

    def run(self, pipeline, dataset, sample, results, sample_idx: int = 0, split: str = "test", epoch: int = 0,
            source_fp: str = None, logger=None, force_output_fp=None):
        """the reference sends the map to TensorBoard and writes a .tif here: both out of scope; returns the map"""
        return self.visualize(pipeline, dataset, sample, results)[0]

    def visualize(self, pipeline, dataset, sample, results):
        W, H = w_h_from_sample(sample)
        viz_output = self._visualize(pipeline, dataset, sample, results, W, H, "_coarse")
        if viz_output is None:
            return None, None, None
        if len(viz_output.shape) == 3:
            assert viz_output.shape[0] in [1, 3, 4], "Wrong channel order in visualization. Needs to be [C, W, H]"
        return viz_output, W, H

    @abc.abstractmethod
    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        pass

    def _stats_slot(self):
        """the slot of the fold's stats block that holds this map's bounds (None: the map's own bounds are folded first)"""
        return None

    def colored(self, img, results=None):
        """visualize_image of a 2-D map: (3, H, W) uint8 on the device"""
        from ..eval.utils.vismaps import colormap
        tab = colormaps.table(self._get_visualize_color_scheme(), img.device)
        slot = self._stats_slot()
        if results is not None and slot is not None:
            return colormap(img, tab, stats=results.stats, slot=slot, cmap_bounds=self._get_visualize_color_range())
        return colormap(img, tab, cmap_bounds=self._get_visualize_color_range())

    def visualize_image_cmap_and_save(self, pipeline, dataset, sample, results, save_to_fp):
        from PIL import Image
        W, H = w_h_from_sample(sample)
        img = self._visualize(pipeline, dataset, sample, results, W, H, "_coarse")
        if img is None:
            return None
        if len(img.shape) == 2:
            img = self.colored(img, results)
        elif img.dtype != torch.uint8:
            img = to_uint8_image(img)
        Image.fromarray(img.permute(1, 2, 0).contiguous().cpu().numpy()).save(save_to_fp)
        return save_to_fp

    def _get_visualize_color_scheme(self):
        return colormaps.COLORMAP_JET

    def _get_visualize_color_range(self):
        return None

    @abc.abstractmethod
    def _name(self) -> str:
        pass


def to_uint8_image(img):
    """torchvision.utils.save_image's conversion of a float image, restated: x * 255 + 0.5, clamp to [0, 255], uint8 (a map
    whose max exceeds 1 is divided by 255 first, as visualize_image_cmap_and_save does)"""
    img = img.to(torch.float32)
    if img.numel() and img.max() > 1:
        img = img / 255.0
    return img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def split_and_index(split: str, img_idx: int):
    """run_visualizer's rule (framework/visualize.py:278-286): on the test split the first image is the first TRAIN image
    (index 0 of "train") and the others count from 0"""
    if split == "test":
        return ("train", img_idx) if img_idx == 0 else ("test", img_idx - 1)
    return split, img_idx


def output_path(run_dp, img_split, name, image_name, epoch):
    return os.path.join(run_dp, "visualization", img_split, name, f"{image_name}_{epoch}.png")


@torch.no_grad()
def run_visualizer(pipeline, output_dp=None, split="test", epoch=-1, create_visualizers_fn=None, max_items=1000000,
                   render_options_fn=lambda pipeline, split: pipeline._val_render_options(split), palette=None, sharded=False,
                   images=None, depth_mode="mean"):
    """The reference's run_visualizer loop over a loaded pipeline (the reference loads it from its log folder first): for every
    image of the split's `scene_images()` (or `images`), one lean_frame_maps fold of the products the visualisers name, then
    every visualiser writes {output_dp or cfgs.run.run_dp}/visualization/{split}/{name}/{image}_{epoch}.png.  Returns the
    paths written.  With `sharded`, every rank folds its rows and rank 0 writes.  `depth_mode="median"`: the depth and altitude
    maps show the rays' median depths (SNERF_FLAG_DEPTH_MEDIAN), whatever the pipeline's config says; "mean" leaves the options of
    `render_options_fn` as they are."""
    from .. import parallel
    from ..eval.utils.util import with_depth_mode
    from ..eval.utils.vismaps import SEMANTIC_PRODUCTS, lean_frame_maps, sharded_lean_frame_maps
    assert create_visualizers_fn is not None and callable(create_visualizers_fn), \
        "create_visualizers_fn needs to be set to a function returning the visualizers that should be run"
    cfgs = pipeline.cfgs
    visualizers = create_visualizers_fn(cfgs)
    dataset_name = "rgb_test" if split == "test" else "rgb"
    bank = pipeline.datasets[dataset_name]
    dataset = getattr(bank, "dataset", bank)
    if images is None:
        images = bank.scene_images()
    products = []
    for v in visualizers:
        products += [p for p in v.products if p not in products]
    dev = next(pipeline.models["coarse"].parameters()).device
    if palette is None and any(p in SEMANTIC_PRODUCTS for p in products):
        palette = torch.from_numpy(colormaps.DEFAULT_PALETTE)
    if palette is not None:
        palette = torch.as_tensor(palette, dtype=torch.uint8).to(dev)
    render_options = with_depth_mode(render_options_fn(pipeline, split), depth_mode, "run_visualizer")
    run_dp = output_dp if output_dp is not None else cfgs.run.run_dp
    fold = sharded_lean_frame_maps if sharded else lean_frame_maps
    written = []
    for img_idx, img in enumerate(images[:max_items]):
        rays = img["rays"].to(dev)
        results = fold(cfgs, pipeline.renderer, pipeline.models, rays.reshape(-1, rays.shape[-1]), img["extras"].to(dev),
                       rgbs=img["rgbs"].to(dev).reshape(-1, 3) if "rgbs" in img else None,
                       semantic=img["semantic"].to(dev) if "semantic" in img else None, palette=palette, products=products,
                       render_options=render_options)
        img_split, _ = split_and_index(split, img_idx)
        for v in visualizers:
            fp = output_path(run_dp, img_split, v._name(), img["name"], epoch)
            if parallel.world()[0] == 0:
                os.makedirs(os.path.dirname(fp), exist_ok=True)
                if v.visualize_image_cmap_and_save(pipeline, dataset, img, results, save_to_fp=fp) is not None:
                    written.append(fp)
    return written
