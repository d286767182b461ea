"""Visualisers of the semantic model -- mirror of semantic/components/visualize.py (SemanticColorVisualization,
SemanticColorShadingVisualization, SemanticErrorVisualization, get_semantic_class_color_mapping), reading the planes of one
streaming fold (eval/utils/vismaps.py).  The palette is an argument of the fold (run_visualizer's `palette`); the default is
the project's own (framework/util/colormaps.py DEFAULT_PALETTE).  The Tensorboard*Summary stacks, the confusion-matrix figure
and the DINO / neighbour / density-reg visualisers are out of scope."""
import torch

from ...framework.util import colormaps
from ...framework.visualize import ImageVisualization

SEMANTIC_CLASS_COLOR_MAPPING = None


def get_semantic_class_color_mapping():
    global SEMANTIC_CLASS_COLOR_MAPPING
    if SEMANTIC_CLASS_COLOR_MAPPING is None:
        SEMANTIC_CLASS_COLOR_MAPPING = torch.from_numpy(colormaps.DEFAULT_PALETTE.copy())
    return SEMANTIC_CLASS_COLOR_MAPPING


class SemanticColorVisualization(ImageVisualization):
    products = ("sem_color",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        return results["sem_color"].view(3, H, W)       # (3, H, W) uint8

    def _name(self) -> str:
        return "semantic_rendering"


class SemanticColorShadingVisualization(ImageVisualization):
    products = ("sem_shaded",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        return results["sem_shaded"].view(3, H, W)      # (3, H, W) uint8

    def _name(self) -> str:
        return "semantic_rendering_shaded"


class SemanticErrorVisualization(ImageVisualization):
    products = ("sem_error",)

    def _visualize(self, pipeline, dataset, sample, results, W, H, typ):
        return results["sem_error"].view(H, W)          # (H, W) fp32: 0 where the label is right, 1 where it is wrong

    def _stats_slot(self):
        return "sem_error"

    def _name(self) -> str:
        return "semantic_error"

    def _get_visualize_color_scheme(self):
        return colormaps.COLORMAP_BONE
