"""Fit the transient embedding of an image that has no row of its own (NeRF-W's evaluation protocol).

A training view owns a row of models["t"]; a test view does not.  The loader gives it the row VAL_T_INDEX lists and row 0 when
the image is not listed (baseline/dataset/satnerf_dataset.py: unlisted_test_views), i.e. the appearance of another date.  Here the
network is frozen and the image's (tau,) vector is optimised on part of its pixels; the frame is then rendered with
render_options["t_vector"] (semantic/components/rendering.py: transient_rows).

One fit step is ONE main pass on a fixed subset of rays with unjittered depths: a training forward, the colour term of the S-NeRF
loss (loss_ops.fused_loss, plain MSE), the library's embedding-only backward (ops._RenderPass.backward takes it when no parameter
needs a gradient: SNERF_FLAG_EMBED_GRAD -- no weight-gradient launch, no trunk), snerf_embedding_backward's fixed-order sum over
the rays, one snerf_adam_step on the vector.  The solar-correction pass reads no transient code and is not run.  The run is
deterministic: the same seed gives the same subset, every launch sums in a fixed order.

DEFAULTS: steps / lr / rays_per_fit are keyword arguments without defaults in fit_image_embedding; FIT_DEFAULTS is what
eval_nerf_images / eval_semantic_images fill in (how they were chosen)."""
import torch

from ... import _lib, loss_ops, ops
from ...framework.components.rays import extras_component_fn
from ...framework.components.rendering import depth_mode_of, z_steps_on

FIT_DEFAULTS = {"steps": 100, "lr": 0.05, "rays_per_fit": 4096}
_ADAM = (0.9, 0.999, 1e-8)      # torch.optim.Adam's betas and eps


def region_mask(w: int, h: int, region: str = "left") -> torch.Tensor:
    """(h * w,) bool, row-major: the pixels a fit may read.  "left": columns [0, w // 2) of every row (NeRF-W fits on the left
    half and reports on the right); "all": every pixel."""
    if region == "all":
        return torch.ones(h * w, dtype=torch.bool)
    if region != "left":
        raise ValueError(f"fit region must be 'left' or 'all', got {region!r}")
    return (torch.arange(w) < w // 2).repeat(h)


def fit_subset(n: int, fit_mask, rays_per_fit: int, seed: int = 0) -> torch.Tensor:
    """the ONE subset of a fit: a seeded randperm prefix of the rays `fit_mask` ((n,) bool, None = all) allows, as int64 indices
    (host generator: the same on every rank and every device)"""
    allowed = torch.arange(n) if fit_mask is None else torch.nonzero(fit_mask.reshape(-1).cpu(), as_tuple=False).reshape(-1)
    if fit_mask is not None and fit_mask.numel() != n:
        raise ValueError(f"fit_mask has {fit_mask.numel()} entries for {n} rays")
    if allowed.numel() == 0:
        raise ValueError("fit_mask allows no ray")
    g = torch.Generator().manual_seed(int(seed))
    return allowed[torch.randperm(allowed.numel(), generator=g)[:int(rays_per_fit)]]


def initial_vector(table: torch.Tensor, init="mean", n_train=None) -> torch.Tensor:
    """(tau,) fp32 start of a fit from the (n_embed, tau) table: "mean" = the fp64 mean of rows [0, n_train) (None: every row),
    rounded once; an int = that row; a tensor = used as given"""
    if torch.is_tensor(init):
        if tuple(init.shape) != (table.shape[1],):
            raise ValueError(f"init vector must have shape ({table.shape[1]},), got {tuple(init.shape)}")
        return init.detach().to(device=table.device, dtype=torch.float32).clone()
    if isinstance(init, str):
        if init != "mean":
            raise ValueError(f"init must be 'mean', a row index or a ({table.shape[1]},) tensor, got {init!r}")
        n = table.shape[0] if n_train is None else int(n_train)
        if not 0 < n <= table.shape[0]:
            raise ValueError(f"n_train = {n} outside (0, {table.shape[0]}]")
        return table.detach()[:n].double().mean(0).float()
    r = int(init)
    if not 0 <= r < table.shape[0]:
        raise ValueError(f"init row {r} outside [0, {table.shape[0]})")
    return table.detach()[r].clone()


def best_iterate(losses) -> int:
    """index of the lowest loss, the earliest of equals -- iterate 0 is the start, so a fit never reports a worse fit-region loss
    than its start; a NaN loss never wins"""
    best = 0
    for k, v in enumerate(losses):
        if v < losses[best] or (losses[best] != losses[best] and v == v):
            best = k
    return best


def fit_image_embedding(cfgs, renderer, models, rays, extras, rgbs, *, fit_mask=None, init="mean", steps, lr, rays_per_fit, seed=0,
                        n_train=None, render_options={}):
    """Fit models["t"]'s vector for the image (rays (n, 8), extras (n, 4), rgbs (n, 3)) with the network frozen.  Returns
    {"t": (tau,) fp32, ["t_s": (tau,) -- its init: fitting t_s from labels is not done,] "loss": [steps + 1 floats, the colour loss
    of iterate 0 .. steps on the fit subset], "best_step": index of the returned iterate, "rays": size of the subset}.
    render_options: "packed_params" (the packed weights, else packed here once) and "t_s_vector" (instead of the t_s init)."""
    opts = render_options or {}
    if depth_mode_of(opts, "fit_image_embedding") != "mean":
        raise ValueError("fit_image_embedding: render_options['depth_mode'] = 'median' is a mode of inference passes; the fit runs "
                         "training passes, and the median depth has no gradient")
    if getattr(renderer, "N_importance", 0) > 0:
        # the fit builds its own PassInputs on the stratified depths: it would fit on other depths than the frame is rendered with
        raise NotImplementedError("fit_image_embedding: n_importance > 0 is not supported (the fit runs on the n_samples stratified "
                                  "depths, the render on the resampled ones); fit with n_importance = 0")
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    dev = rays.device
    rays = rays.reshape(-1, rays.shape[-1])
    n = rays.shape[0]
    idx = fit_subset(n, fit_mask, rays_per_fit, seed).to(dev)
    r_fit = rays.index_select(0, idx).contiguous()
    e_fit = extras.reshape(n, -1).index_select(0, idx).contiguous()
    gt = rgbs.reshape(n, 3).index_select(0, idx).to(torch.float32).contiguous()
    model = models["coarse"]
    spec = model.spec
    if not (spec.n_classes > 0 and spec.use_tj_instead_of_beta):
        # semantic/models/rs_semantic.py:283-301: t is appended to the colour head's input only under use_tj_instead_of_beta (else it
        # feeds beta and, with use_tj_for_s, the semantic head); the gradient of the colour loss is then exactly zero
        raise ValueError("fit_image_embedding: the colour head of this model does not read the transient embedding "
                         "(use_tj_instead_of_beta is off), so the colour loss cannot fit it")
    frozen = {k: p.detach() for k, p in model.named_parameters()}      # no parameter needs a gradient: the embedding-only backward
    packed = opts.get("packed_params")
    if packed is None:
        packed = ops.pack_params(spec, frozen)
    tau = models["t"].weight.shape[1]
    # the vector lives in a buffer of whole float4s (snerf_adam_step's granule), with its gradient and the two Adam moments
    n4 = (tau + 3) // 4 * 4
    state = torch.zeros(4, n4, dtype=torch.float32, device=dev)
    state[0, :tau] = initial_vector(models["t"].weight, init, n_train)
    vec = state[0, :tau]
    t_s = None
    if "t_s" in models:
        t_s = opts.get("t_s_vector")
        if t_s is None:
            t_s = initial_vector(models["t_s"].weight, init, n_train)
    sun_d = extras_component_fn(e_fit, "sun_d")
    zeros = torch.zeros(idx.shape[0], dtype=torch.int64, device=dev)
    lspec = loss_ops.LossSpec(color_mode=1)
    trace = torch.empty(steps + 1, tau, dtype=torch.float32, device=dev)
    losses = torch.empty(steps + 1, dtype=torch.float32, device=dev)

    def colour_loss(leaf):
        pin = ops.PassInputs(sun_d=sun_d, rays=r_fit, z_steps=z_steps_on(dev, renderer.N_samples))      # perturb 0: no jitter
        rows = ops._EmbedRows.apply(leaf.view(1, tau), zeros)
        rows_s = ops._EmbedRows.apply(t_s.view(1, tau), zeros) if t_s is not None else None
        res = ops.render_pass(spec, frozen, pin, rows, rows_s, packed=packed)
        return loss_ops.fused_loss(lspec, {"rgb_coarse": res["rgb"]}, {"gt_rgb": gt}, sync=False)[0]

    for k in range(steps + 1):
        trace[k] = vec
        with torch.enable_grad():      # (the evaluators call this under no_grad; the last iterate is only evaluated, by the same training forward)
            leaf = vec.detach().clone().requires_grad_(True)
            loss = colour_loss(leaf)
            losses[k] = loss.detach()
            if k == steps:
                break
            state[1, :tau] = torch.autograd.grad(loss, leaf)[0]
        _lib.call("snerf_adam_step", state[0], state[1], state[2], state[3], n4, float(lr), _ADAM[0], _ADAM[1], _ADAM[2], k + 1, 1.0)
    hist = [float(v) for v in losses.cpu()]
    best = best_iterate(hist)
    out = {"t": trace[best].clone(), "loss": hist, "best_step": best, "rays": int(idx.shape[0])}
    if t_s is not None:
        out["t_s"] = t_s.detach().clone()
    return out


def fit_options(fit_embedding):
    """eval_*_images' `fit_embedding` dict -> (region, driver keyword arguments): "region" split off, FIT_DEFAULTS filled in"""
    kw = dict(FIT_DEFAULTS)
    kw.update(fit_embedding)
    region = kw.pop("region", "left")
    if region not in ("left", "all"):
        raise ValueError(f"fit_embedding['region'] must be 'left' or 'all', got {region!r}")
    return region, kw


def fit_for_image(cfgs, renderer, models, img, rays, extras, w, h, region, kw, packed=None):
    """the per-image step of the evaluators: (fit result, fit mask (n,) bool on the rays' device, the "t_fit" entry)"""
    mask = region_mask(w, h, region)
    kw = dict(kw)
    ro = dict(kw.pop("render_options", None) or {})
    if packed is not None:
        ro.setdefault("packed_params", packed)
    fit = fit_image_embedding(cfgs, renderer, models, rays, extras, img["rgbs"].reshape(-1, 3), fit_mask=mask, render_options=ro, **kw)
    entry = {"region": region, "steps": int(kw["steps"]), "best_step": fit["best_step"], "loss_first": fit["loss"][0],
             "loss_best": fit["loss"][fit["best_step"]]}
    return fit, mask.to(rays.device), entry


def vector_options(fit, render_options=None):
    """render options that render with a fit's vectors"""
    ro = dict(render_options or {})
    ro["t_vector"] = fit["t"]
    if "t_s" in fit:
        ro["t_s_vector"] = fit["t_s"]
    return ro
