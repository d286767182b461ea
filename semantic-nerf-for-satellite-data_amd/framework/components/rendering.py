"""Renderer base -- mirror of framework/components/rendering.py:119-174 (BaseRenderer).

Stratified sampling (reference sample_rays, :84-116) is fused into the HIP pass: render_rays only
draws the jitter tensor (the reference calls torch.rand_like with perturb=1.0 on every call, train
and eval alike) and hands it down; z_vals / xyz never materialise on the host side.

With `n_importance` > 0 (the reference's sample_pdf, :8-51, which its BaseRenderer never calls) a render first runs a proposal
pass on the stratified depths and resamples them on the device (ops.resample_z); everything else then runs on the merged
n_samples + n_importance depths through the `given_z_vals` seam."""
import abc
import functools

import torch

from .rays import ray_component_fn


@functools.lru_cache(maxsize=16)
def _host_linspace(n: int):
    # computed on the host like the CPU reference does (torch.linspace(0, 1, S)); GPU linspace may
    # differ in the last bit, which would break bit-exact z_vals.
    return torch.linspace(0, 1, n)


_Z_STEPS_DEV: dict = {}


def z_steps_on(device, n: int) -> torch.Tensor:
    """The host's linspace on `device`, copied ONCE per (device, n).  (Copied per call it was the step's one blocking call: a
    host-to-device copy from pageable memory returns when the stream has reached it, i.e. the host waited a whole step behind
    the device here every step and the device then idled ~0.13 ms while the host caught up -- tools/host_timeline.py.)"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device.type, device.index, n)
    t = _Z_STEPS_DEV.get(key)
    if t is None:
        t = _Z_STEPS_DEV[key] = _host_linspace(n).to(device)
    return t


def bare_key(key: str) -> str:
    return key[:-len("_coarse")] if key.endswith("_coarse") else key


def _bare_results(who: str, out: dict) -> dict:
    """`out` under its keys without the '_coarse' postfix, which every key must carry"""
    for k in out:
        if not k.endswith("_coarse"):
            raise KeyError(f"{who}: result keys end in '_coarse', got '{k}'")
    return {bare_key(k): v for k, v in out.items()}


DEPTH_MODES = ("mean", "median")


def depth_mode_of(render_options, who: str) -> str:
    """render_options["depth_mode"]: what 'depth' is -- "mean" (default: the expected depth sum w_i z_i) or "median" (the depth at
    which half of the ray's weight lies in front: SNERF_FLAG_DEPTH_MEDIAN, inference passes only).  Anything else is a ValueError."""
    mode = (render_options or {}).get("depth_mode", "mean")
    if mode not in DEPTH_MODES:
        raise ValueError(f"{who}: render_options['depth_mode'] must be one of {DEPTH_MODES}, got {mode!r}")
    return mode


def n_render_samples(pipeline_cfg) -> int:
    """S' = n_samples + n_importance: the samples per ray of every rendering pass and the columns of every per-sample result.
    THE place that names it: the renderer and everything that sizes a buffer for its results ask here."""
    return int(pipeline_cfg.n_samples) + max(int(getattr(pipeline_cfg, "n_importance", 0) or 0), 0)


class BaseRenderer:
    def __init__(self, cfgs) -> None:
        super().__init__()
        self.cfgs = cfgs
        self.N_samples = cfgs.pipeline.n_samples
        self.n_render_samples = n_render_samples(cfgs.pipeline)
        self.N_importance = self.n_render_samples - self.N_samples

    def _importance_depths(self, models, rays, extras, opts):
        """n_importance > 0 and no depths given: opts["given_z_vals"] = the merged depths of a proposal pass (no gradient)"""
        if self.N_importance > 0 and opts.get("given_z_vals") is None:
            from ...semantic.components.rendering import importance_depths
            importance_depths(self, models, "coarse", rays, extras, opts)

    def render_rays(self, models: dict, rays: torch.Tensor, extras: torch.Tensor, epoch=None, progress=1.0,
                    render_options={}):
        if depth_mode_of(render_options, "render_rays") != "mean":
            # render_rays is the differentiable render (ops.render_pass); the median has no gradient and rides on inference passes only
            raise ValueError("render_rays: render_options['depth_mode'] = 'median' is a mode of the inference renders "
                             "(render_rays_into, render_chunks, lean_inference); the training path does not take it")
        rays_d = ray_component_fn(rays, "directions")
        opts = dict(render_options) if render_options else {}
        if "perturb_rand" not in opts and opts.get("perturb", 1.0) > 0:
            opts["perturb_rand"] = torch.rand(rays.shape[0], self.N_samples, device=rays.device, dtype=torch.float32)
        self._importance_depths(models, rays, extras, opts)
        model_results = self._model_rendering(models, "coarse", self.cfgs, rays, extras, None, None, rays_d,
                                              epoch=epoch, progress=progress, render_options=opts)
        # "_coarse" postfix as in the reference (no fine network is ever built)
        return {f"{k}_coarse": v for k, v in model_results.items()}

    @torch.no_grad()
    def render_rays_into(self, models: dict, rays: torch.Tensor, extras: torch.Tensor, out: dict, render_options={}):
        """Inference-only render_rays that fills the preallocated tensors of `out` (keys as render_rays returns them,
        e.g. 'rgb_coarse', 'depth_coarse', 'semantic_label_coarse') and computes nothing else.  Returns the pass's
        workspace buffer so that a caller can hand it back through render_options['workspace'] for the next chunk.
        render_options['depth_mode'] = "median" makes 'depth_coarse' the median depth (the final pass takes the flag, a proposal
        pass does not); the scratch tensors that pass may need ride in render_options['depth_scratch'], a dict, like the workspace."""
        from ...semantic.components.rendering import fused_model_rendering_into
        depth_mode_of(render_options, "render_rays_into")      # (before anything is drawn or launched)
        opts = dict(render_options) if render_options else {}
        if "perturb_rand" not in opts and opts.get("perturb", 1.0) > 0:
            opts["perturb_rand"] = torch.rand(rays.shape[0], self.N_samples, device=rays.device, dtype=torch.float32)
        self._importance_depths(models, rays, extras, opts)
        return fused_model_rendering_into(self, models, "coarse", rays, extras, opts, _bare_results("render_rays_into", out))

    @torch.no_grad()
    def relight_rays_into(self, models: dict, extras: torch.Tensor, out: dict, render_options={}):
        """The rays render_rays_into rendered last into render_options['workspace'] (the workspace it returned), under the sun of
        `extras`: only the sun-dependent part of the pass runs again, on the base pass's depths, and every result has the bits
        render_rays_into gives under that sun.  `out` as for render_rays_into, main-pass results only.  Returns the workspace."""
        from ...semantic.components.rendering import fused_model_relighting_into
        depth_mode_of(render_options, "relight_rays_into")
        return fused_model_relighting_into(self, models, "coarse", extras, dict(render_options) if render_options else {},
                                           _bare_results("relight_rays_into", out))

    @abc.abstractmethod
    def _model_rendering(self, models: dict, typ: str, cfgs, rays, extras, xyz, z_vals, rays_d, epoch=None,
                         progress=1.0, render_options=None) -> dict:
        pass
