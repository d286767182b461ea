"""Visualisers of the baseline models -- mirror of baseline/components/visualize.py (AltsVisualization, FactorVisualization,
RGBDiffVisualization, RGBDiffDistanceVisualization), reading the planes of one streaming fold (eval/utils/vismaps.py) in place
of the frame's (N, S, .) render results.  TensorboardSummaryVisualization is out of scope."""
import torch

from ...framework.util import colormaps
from ...framework.visualize import ImageVisualization

# FactorVisualization's shape rules (:88-108) by factor: a (N, S, 3) result is composited into (3, H, W), a (N, S, 1) one into
# (H, W); a (N, 3) result becomes (3, H, W), a (N,) one (H, W)
FACTORS = ("rgb", "depth", "albedo", "sun", "beta", "sky", "beta_semantic")
_BANDS = {"rgb": 3, "albedo": 3, "sky": 3}


class AltsVisualization(ImageVisualization):
    products = ("depth",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        rays = sample["rays"].reshape(-1, sample["rays"].shape[-1])
        _, _, alts = dataset.get_latlonalt_from_nerf_prediction(rays.to(results["depth"].device), results["depth"])
        return alts.view(H, W)          # (H, W) fp64, on the device

    def _name(self) -> str:
        return "alts"

    def _get_visualize_color_scheme(self):
        return colormaps.COLORMAP_JET


class FactorVisualization(ImageVisualization):
    def __init__(self, cfgs, send_to_tensorboard: bool, save_as_tif: bool, factor_name: str, viz_name: str = None,
                 cmap=colormaps.COLORMAP_BONE) -> None:
        super().__init__(cfgs, send_to_tensorboard, save_as_tif)
        self.factor_name = factor_name
        self.viz_name = viz_name if viz_name is not None else factor_name
        self.cmap = cmap
        self.products = (factor_name,) if factor_name in FACTORS else ()

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        if self.factor_name not in results:
            return None                 # the reference logs "trying to visualize non-existent factor" and returns None
        plane = results[self.factor_name]
        if self.factor_name == "rgb":
            return plane.view(H, W, 3).permute(2, 0, 1)       # (3, H, W)
        if _BANDS.get(self.factor_name) == 3:
            return plane.view(3, H, W)
        return plane.view(H, W)

    def _stats_slot(self):
        return self.factor_name if self.factor_name not in _BANDS else None

    def _name(self) -> str:
        return self.viz_name

    def _get_visualize_color_scheme(self):
        return self.cmap


class RGBDiffVisualization(ImageVisualization):
    products = ("rgb_diff",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        return results["rgb_diff"].view(3, H, W)

    def _name(self) -> str:
        return "RGB_Diff"


class RGBDiffDistanceVisualization(RGBDiffVisualization):
    products = ("rgb_diff_distance",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        return results["rgb_diff_distance"].view(H, W)

    def _stats_slot(self):
        return "rgb_diff_distance"

    def _name(self) -> str:
        return "RGB_Diff_Distance"

    def _get_visualize_color_scheme(self):
        return colormaps.COLORMAP_BONE
