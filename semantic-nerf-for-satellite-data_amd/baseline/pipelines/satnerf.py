"""Sat-NeRF pipeline + config -- mirror of baseline/pipelines/satnerf.py:23-132 and the config chain
NeRFConfig (baseline/pipelines/nerf.py:63-88) <- SNeRFConfig (snerf.py:67-68) <- SatNeRFConfig."""
from typing import List, Literal, Optional, Union

import numpy as np
import torch
from pydantic import BaseModel, model_validator

from ...framework.datasets import GpuRayBank
from ..components.loss import SNerfLoss, SatNerfLoss, DepthLoss
from ..components.rendering import SatNeRFRendering
from ..components.training_step import SatNeRFTrainingStep
from ..models.satnerf import SatNeRF
from .base_ray_pipeline import BaseRayPipeline


class NeRFConfig(BaseModel):
    pipeline: Optional[str] = None
    precision: int = 32
    mfma_precision: Literal["f16x2", "f16x1", "bf16", "auto"] = "f16x2"  # build extension: ops.mfma_mode
    use_utm_coordinate_system: Union[bool, int] = False
    version: int = 1
    n_samples: int = 64
    use_fine_network: Union[bool, int] = False
    n_importance: int = 0
    depth_mode: Literal["mean", "median"] = "mean"  # build extension: what validation and evaluation read as a ray's depth; training never takes it
    render_chunk_size: int = 5120
    batch_size: int = 1024
    learnrate: float = 5e-4
    noise_std: float = 0.0
    activation_function: Literal["siren", "relu"] = "siren"
    mapping_pos_n_freq: int = 10
    mapping_dir_n_freq: int = 4
    fc_units: int = 512
    fc_layers: int = 8
    fc_skips: List[int] = [4]
    ray_subsampling_activated: Union[bool, int] = False
    ray_subsampling_amount: float = 1.0
    # build extension: the weight of the distortion loss on the main pass's ray weights (0 = off: no launch,
    # no tensor, no log key) and the epoch it starts at
    lambda_dist: float = 0.0
    dist_start_epoch: int = 0

    @model_validator(mode="after")
    def _check_n_importance(self):
        """n_importance fine samples per ray are merged with the n_samples coarse ones (ops.resample_z): the pdf is over the
        interior weights, and a ray holds at most 1024 samples (include/snerf_hip.h: snerf_resample_z)"""
        if self.n_importance < 0:
            raise ValueError(f"n_importance must be >= 0, got {self.n_importance}")
        if self.n_importance > 0:
            if self.n_samples < 3:
                raise ValueError(f"n_importance > 0 needs n_samples >= 3, got n_samples = {self.n_samples}")
            if self.n_samples + self.n_importance > 1024:
                raise ValueError(f"n_samples + n_importance must be <= 1024, got {self.n_samples} + {self.n_importance}")
        return self

    @model_validator(mode="after")
    def _check_lambda_dist(self):
        if not self.lambda_dist >= 0:
            raise ValueError(f"lambda_dist must be >= 0, got {self.lambda_dist}")
        if self.dist_start_epoch < 0:
            raise ValueError(f"dist_start_epoch must be >= 0, got {self.dist_start_epoch}")
        if self.lambda_dist > 0 and self.n_samples + max(self.n_importance, 0) > 1024:
            raise ValueError(f"lambda_dist > 0 needs n_samples + n_importance <= 1024, got {self.n_samples} + {self.n_importance}")
        return self


class SNeRFConfig(NeRFConfig):
    sc_lambda: float = 0.05


class SatNeRFConfig(SNeRFConfig):
    fc_use_full_features: Union[bool, int] = False
    depth_enabled: Union[bool, int] = True
    depth_supervision_drop: float = 0.25
    ds_lambda: int = 1000
    first_beta_epoch: int = 2
    t_embedding_vocab: int = 50
    t_embedding_tau: int = 4
    ds_noweights: Union[bool, int] = False
    # build extension: what feeds the depth branch of a scene loaded from disk -- the bundle-adjustment tie
    # points (the reference), a DSM GeoTIFF seen through every depth_prior_stride-th pixel's ray (baseline/dataset/
    # dsm_depth_dataset.py), or both; depth_prior_weight is the constant weight of the prior's rows
    depth_source: Literal["tie_points", "dsm", "both"] = "tie_points"
    depth_prior_dsm_fp: str = ""
    depth_prior_stride: int = 4
    depth_prior_weight: float = 1.0

    @model_validator(mode="after")
    def _check_depth_prior(self):
        from ..dataset.dsm_depth_dataset import prior_settings
        prior_settings(self)
        return self


class SatNeRFPipeline(BaseRayPipeline):
    def __init__(self, cfgs, ckpt_info=None) -> None:
        super().__init__(cfgs, ckpt_info)
        if self.cfgs.pipeline.depth_enabled:
            self.ds_drop = np.round(self.cfgs.pipeline.depth_supervision_drop * self.cfgs.run.max_train_steps)

    def _n_classes(self):
        return 5

    _semantic_scene = False     # which loader reads a scene from disk (RSSemanticPipeline: the semantic one)

    def _init_datasets(self) -> dict:
        r = self.cfgs.run
        if r.dataset_dp:
            from ..dataset.satnerf_dataset import load_scene_banks
            return load_scene_banks(self.cfgs, semantic=self._semantic_scene, depth=bool(self.cfgs.pipeline.depth_enabled),
                                    seed=r.synthetic_seed)
        d = {"rgb": GpuRayBank.synthetic(r.synthetic_rays, r.synthetic_images, self._n_classes(), r.synthetic_seed),
             "rgb_test": GpuRayBank.synthetic(4096, r.synthetic_images, self._n_classes(), r.synthetic_seed + 1)}
        if self.cfgs.pipeline.depth_enabled:
            d["depth"] = GpuRayBank.synthetic(max(r.synthetic_rays // 8, self.cfgs.pipeline.batch_size),
                                              r.synthetic_images, self._n_classes(), r.synthetic_seed + 2, depth=True)
        return d

    def _init_loss(self):
        self.loss = SatNerfLoss(lambda_sc=self.cfgs.pipeline.sc_lambda)
        self.loss_without_beta = SNerfLoss(lambda_sc=self.cfgs.pipeline.sc_lambda)
        if self.cfgs.pipeline.depth_enabled:
            self.depth_loss = DepthLoss(lambda_ds=self.cfgs.pipeline.ds_lambda)

    def _init_models(self) -> dict:
        pc = self.cfgs.pipeline
        return {"coarse": SatNeRF(self.cfgs, layers=pc.fc_layers, feat=pc.fc_units, skips=pc.fc_skips,
                                  siren=pc.activation_function == "siren", t_embedding_dims=pc.t_embedding_tau),
                "t": torch.nn.Embedding(pc.t_embedding_vocab, pc.t_embedding_tau)}

    def _init_renderer(self):
        return SatNeRFRendering(self.cfgs)

    def _init_training_step(self):
        return SatNeRFTrainingStep()

    @staticmethod
    def create_visualizers(cfgs) -> list:
        """the reference's _init_visualizers list (satnerf.py:74-108) without its TensorBoard summary: what run_visualizer's
        create_visualizers_fn returns.  `_init_visualizers` itself keeps returning []: validation draws nothing."""
        from ..components import visualize
        from ...framework.util.colormaps import COLORMAP_BONE
        kw = dict(save_as_tif=True, send_to_tensorboard=True)
        return [visualize.FactorVisualization(cfgs, factor_name="rgb", **kw),
                visualize.FactorVisualization(cfgs, factor_name="depth", **kw),
                visualize.FactorVisualization(cfgs, factor_name="albedo", **kw),
                visualize.FactorVisualization(cfgs, factor_name="sun", cmap=COLORMAP_BONE, **kw),
                visualize.FactorVisualization(cfgs, factor_name="beta", cmap=COLORMAP_BONE, **kw),
                visualize.RGBDiffDistanceVisualization(cfgs, **kw)]

    @classmethod
    def init_config(cls, cfg_information):
        return SatNeRFConfig(**cfg_information)
