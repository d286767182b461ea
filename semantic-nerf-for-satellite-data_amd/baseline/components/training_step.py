"""Sat-NeRF training step -- mirror of baseline/components/training_step.py:19-59 (loss gating)."""
import torch

from ...framework.components.training_step import BaseTrainingStep


def _distortion_lambda(pipeline) -> float:
    """the weight of the distortion loss on the main pass's weights at this epoch (a build extension):
    `lambda_dist` (default 0: off) from `dist_start_epoch` (default 0) on; 0.0 while it is off"""
    pc = pipeline.cfgs.pipeline
    lam = float(getattr(pc, "lambda_dist", 0.0) or 0.0)
    if lam > 0 and pipeline.get_current_epoch() >= int(getattr(pc, "dist_start_epoch", 0) or 0):
        return lam
    return 0.0


def _key_is_configured(pc, key: str) -> bool:
    """the config names `key` itself (a pydantic config: the key was given, not defaulted; any other object: it has the attribute)"""
    given = getattr(pc, "model_fields_set", None)
    return key in given if given is not None else hasattr(pc, key)


def main_pass(pipeline, batch):
    """the step's main forward on the batch's rays; while the distortion loss is on it also returns the depths (`z_vals_coarse`)"""
    data = {"rays": batch["rgb"]["rays"], "extras": batch["rgb"]["extras"]}
    if _distortion_lambda(pipeline) > 0:
        return pipeline(data, {"return_z_vals": True})
    return pipeline(data)


def color_and_depth_losses(pipeline, batch, results, more_plans=()):
    """colour loss by epoch (SNerfLoss before `first_beta_epoch`, SatNerfLoss after) + the depth-supervision branch while
    `train_steps < ds_drop`; the log keys and the gate order are the reference's (they are what its TensorBoard shows).
    `more_plans`: plans of further loss modules on the SAME rendered tensors (the semantic step's: loss_ops.run_plans evaluates them
    with the colour loss in one fused call); their terms come back in the same dict, their sum in the same total.
    With `lambda_dist` > 0 from `dist_start_epoch` on (a build extension; both default to 0) the distortion loss of the MAIN pass's
    weights along its depths joins the total as `coarse_distortion` -- not the solar-correction pass's, not the depth rays'."""
    from ...loss_ops import run_plans
    pc = pipeline.cfgs.pipeline
    with_beta = pipeline.get_current_epoch() >= pc.first_beta_epoch
    color = pipeline.loss if with_beta else pipeline.loss_without_beta
    if hasattr(color, "plan"):
        total, terms = run_plans([color.plan(results, batch["rgb"]["rgbs"])] + list(more_plans), results)
    else:      # a foreign colour loss module: called as the reference calls it, the other modules' plans on their own
        total, terms = color(results, batch["rgb"]["rgbs"])
        if more_plans:
            t2, d2 = run_plans(list(more_plans), results)
            total = total + t2
            terms.update(d2)
    pipeline.log("train/beta_loss_activated", 1.0 if with_beta else 0.0)
    lam = _distortion_lambda(pipeline)
    if lam > 0:
        from ...loss_ops import distortion_loss
        if "z_vals_coarse" not in results:
            raise KeyError("the distortion loss reads the main pass's depths: render it with render_options['return_z_vals'] "
                           "(baseline/components/training_step.py main_pass)")
        dist_total, dist_term = distortion_loss(results["weights_coarse"], results["z_vals_coarse"], batch["rgb"]["rays"], lam)
        total = total + dist_total
        terms["coarse_distortion"] = dist_term
        pipeline.log("train/distortion_loss_activated", 1.0)
    elif _key_is_configured(pc, "lambda_dist"):
        pipeline.log("train/distortion_loss_activated", 0.0)
    if not pc.depth_enabled:
        return total, terms
    depth_on = pipeline.train_steps < pipeline.ds_drop
    pipeline.log("train/depth_loss_activated", 1.0 if depth_on else 0.0)
    if depth_on:
        d = batch["depth"]
        rendered = pipeline({"rays": d["rays"], "extras": d["extras"]})      # a second full forward on the depth rays
        targets = d["depths"][:, 0].reshape(-1)
        ray_weights = 1.0 if pc.ds_noweights else d["weights"].reshape(-1)
        depth_total, depth_terms = pipeline.depth_loss(rendered, targets, ray_weights)
        total = total + depth_total
        terms.update(depth_terms)
    return total, terms


class SatNeRFTrainingStep(BaseTrainingStep):
    def training_step(self, pipeline, batch, batch_idx):
        results = main_pass(pipeline, batch)
        loss, loss_dict = color_and_depth_losses(pipeline, batch, results)
        return results, loss, loss_dict
