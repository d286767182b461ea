"""Semantic renderer -- mirror of semantic/components/rendering.py:12-80 (RSSemanticRendering).

ts -> int64 happens on the device (the reference round-trips through a CPU LongTensor, :35-40; same
values), the embedding lookup is ops.embed_rows (one launch forward, one deterministic launch backward
for the nn.Embedding gradient), and both passes -- main and, if sc_lambda > 0, the solar-correction pass on o + sun_d*z --
run as fused HIP passes that share one packed copy of the weights."""
import os

import torch

from ... import ops
from ...framework.components.rendering import BaseRenderer, depth_mode_of, z_steps_on
from ...framework.components.rays import extras_component_fn
from ..models.rs_semantic import inference as rs_semantic_inference


# main and solar-correction passes on two HIP streams (set SNERF_OVERLAP_SC=0 to serialise them)
OVERLAP_SC_PASS = os.environ.get("SNERF_OVERLAP_SC", "1") != "0"
if OVERLAP_SC_PASS and hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
    # the two passes deliberately run (and back-propagate) on two streams; autograd synchronises the accumulation itself
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
_SIDE_STREAMS = {}


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def transient_rows(models, name, ts, opts):
    """The rays' rows of the transient embedding `name` ("t" / "t_s"): models[name](ts), or -- render_options["t_vector"] /
    ["t_s_vector"], a (tau,) fp32 GPU tensor -- that ONE vector for every ray, whatever `ts` says (an image without a row of its
    own: eval/utils/embedding.py fits one).  The vector goes through the same Function as a (1, tau) table under a zero index, so
    its gradient is snerf_embedding_backward's fixed-order sum over the rays."""
    v = opts.get(name + "_vector")
    if v is None:
        return ops.embed_rows(models[name], ts)
    tau = models[name].weight.shape[1]
    if v.dim() != 1 or v.shape[0] != tau or v.dtype != torch.float32 or not v.is_cuda:
        raise ValueError(f"render_options['{name}_vector'] must be a ({tau},) float32 GPU tensor, got {tuple(v.shape)} {v.dtype} on {v.device}")
    return ops._EmbedRows.apply(v.view(1, tau), torch.zeros_like(ts))


def _pass_operands(models, model, extras, opts):
    """what the fused entry points hand to a pass of `model`: -> (sun_d, rays_t, rays_t_s, params, packed) -- the sun columns of
    `extras`, the rays' transient rows (launched before the pack), the parameters, and their pack (render_options["packed_params"],
    else packed here)"""
    sun_d = extras_component_fn(extras, "sun_d")
    ts = extras_component_fn(extras, "ts").squeeze(-1).long()
    rays_t = transient_rows(models, "t", ts, opts)
    rays_t_s = transient_rows(models, "t_s", ts, opts) if "t_s" in models else None
    params = dict(model.named_parameters())
    packed = opts.get("packed_params")
    if packed is None:
        packed = ops.pack_params(model.spec, params)
    return sun_d, rays_t, rays_t_s, params, packed


@torch.no_grad()
def importance_depths(renderer, models, typ, rays, extras, opts: dict):
    """The depths of a render with n_importance > 0, left in opts["given_z_vals"]: a PROPOSAL pass -- the geometry pass
    (trunk, sigma, composite; no head launch and no embedding lookup) on the stratified depths (opts["perturb_rand"]), which gives
    weights and depths with the bits of the inference main pass; opts["proposal_pass"] = "full" runs that main pass instead, asked
    for the same two results -- and ops.resample_z, which draws
    n_importance fine samples per ray from those weights and merges them with the coarse depths: (N, n_samples + n_importance),
    no gradient (sample_pdf's callers detach the samples).  The uniforms are opts["importance_rand"] (N, n_importance); absent,
    they are drawn when opts["perturb"] (default 1.0) > 0 and are the regular grid of the reference's det=True otherwise, as in
    NeRF.  Two launches more than the pass itself, all on the current stream: nothing waits for the host.  The pack of the
    weights is left in opts["packed_params"] for the passes that follow; an inference workspace given in opts["workspace"] is
    used and handed on, otherwise one is leased for the length of the pass."""
    model = models[typ]
    spec = model.spec
    N, S, Ni, dev = rays.shape[0], renderer.N_samples, renderer.N_importance, rays.device
    proposal = opts.get("proposal_pass", "geometry")
    if proposal not in ("geometry", "full"):
        raise ValueError(f"render_options['proposal_pass'] must be 'geometry' or 'full', got {proposal!r}")
    geometry = proposal == "geometry"
    if geometry:
        # weights and depths depend on no head: the geometry pass (SNERF_FLAG_GEOMETRY) gives their bits without the head launches, and
        # reads neither the sun nor an embedding -- no lookup is launched for the proposal
        sun_d = rays_t = rays_t_s = None
        params = dict(model.named_parameters())
        packed = opts.get("packed_params")
        if packed is None:
            packed = ops.pack_params(spec, params)
    else:      # "full": the inference main pass asked for the same two results
        sun_d, rays_t, rays_t_s, params, packed = _pass_operands(models, model, extras, opts)
    opts["packed_params"] = packed
    out = {"weights": ops._empty((N, S), dtype=torch.float32, device=dev), "z_vals": ops._empty((N, S), dtype=torch.float32, device=dev)}
    pin = ops.PassInputs(sun_d=sun_d, rays=rays, z_steps=z_steps_on(dev, S), u=opts.get("perturb_rand"))
    ws, lease = opts.get("workspace"), None
    if ws is None and "workspace" not in opts:      # a training render: the lease pool, like the passes that follow
        with torch.cuda.device(dev):
            lease = ops.lease_workspace(dev, ops._lib.call_size("snerf_workspace_bytes", spec.desc(N, S, ops._lib.FLAG_GEOMETRY if geometry else 0)))
        ws = lease.t
    elif ws is None:                                # the first chunk of a walk: sized for the rendering pass that follows
        ws = ops._empty(ops._lib.call_size("snerf_workspace_bytes", spec.desc(N, S + Ni)), dtype=torch.uint8, device=dev)
    ws = ops.render_pass_into(spec, params, pin, rays_t, rays_t_s, out, packed=packed, workspace=ws, geometry=geometry)
    if lease is not None:
        lease.release()      # stream order makes the reuse safe
    else:
        opts["workspace"] = ws
    u = opts.get("importance_rand")
    if u is None and opts.get("perturb", 1.0) > 0:
        u = torch.rand(N, Ni, device=dev, dtype=torch.float32)
    opts["given_z_vals"] = ops.resample_z(out["z_vals"], out["weights"], Ni, u)


def fused_model_rendering(renderer, models, typ, rays, extras, render_options, inference_func, default_inference):
    if inference_func is not default_inference:
        raise NotImplementedError(
            "only the library's own inference() can be injected: sampling, encoding, MLP and compositing are one "
            "fused HIP pass (snerf_forward); a foreign per-sample inference callable has nothing to plug into")
    cfgs = renderer.cfgs
    opts = render_options or {}
    if depth_mode_of(opts, "fused_model_rendering") != "mean":
        raise ValueError("fused_model_rendering: depth_mode = 'median' is a mode of the inference passes (fused_model_rendering_into); "
                         "the differentiable passes do not take it")
    model = models[typ]
    sun_d, rays_t, rays_t_s, params, packed = _pass_operands(models, model, extras, opts)
    pin = ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=opts.get("given_z_vals"),
                         z_steps=z_steps_on(rays.device, renderer.N_samples), u=opts.get("perturb_rand"))
    do_sc = cfgs.pipeline.sc_lambda > 0
    z_given = opts.get("given_z_vals")
    side = _side_stream(rays.device) if (do_sc and OVERLAP_SC_PASS) else None
    if side is not None:
        # The solar-correction pass only shares z_vals with the main pass.  Sample z first (tiny kernel), then run the
        # two independent MLP passes on two HIP streams: their GEMM launches interleave on the CUs and fill each
        # other's ramp-up / tail.  autograd replays each pass's backward on the stream of its forward.
        if z_given is None:
            z_given = ops.sample_z(rays, z_steps_on(rays.device, renderer.N_samples), opts.get("perturb_rand"))
            pin = ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=z_given)
        main = torch.cuda.current_stream(rays.device)
        side.wait_stream(main)      # (before the main pass is issued: the side stream waits for the weights pack and z, not for that pass)
        # The main pass is CREATED first: autograd runs the younger node first, so in the backward the solar-correction pass -- the
        # shorter one, done ~2 ms before the main pass -- adds its gradients into the optimiser's bucket first and the main pass's
        # unpack only waits for an event that completed long ago.  The other way round the short pass queued behind the long one's
        # unpack at the very end of the step: two cross-stream hand-overs (~15-25 us each) and its unpack kernels, all exposed.
        result = ops.render_pass(model.spec, params, pin, rays_t, rays_t_s, packed=packed)
        with torch.cuda.stream(side):
            sc = ops.render_pass(model.spec, params, ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=z_given), rays_t,
                                 rays_t_s, sc_pass=True, packed=packed)
        main.wait_stream(side)
        for v in sc.values():
            v.record_stream(main)
    else:
        result = ops.render_pass(model.spec, params, pin, rays_t, rays_t_s, packed=packed)
        if do_sc:
            sc = ops.render_pass(model.spec, params, ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=result["z_vals"]),
                                 rays_t, rays_t_s, sc_pass=True, packed=packed)
    z_vals = result.pop("z_vals")
    if do_sc:
        result["weights_sc"] = sc["weights"]
        result["transparency_sc"] = sc["transparency"]
        result["sun_sc"] = sc["sun"]
    if opts.get("return_z_vals"):
        result["z_vals"] = z_vals
    return result


_SC_KEYS = {"weights_sc": "weights", "transparency_sc": "transparency", "sun_sc": "sun"}


def _depth_mode_kwargs(who, opts, out):
    """depth_mode= / scratch= of an ops *_into pass that writes `out`: render_options["depth_mode"] where the pass is asked for
    'depth' (a pass that hands out no depth has nothing to rewrite and runs as it is), with the scratch dict of
    render_options["depth_scratch"]; {} at the default, so that a default render calls ops exactly as before."""
    if depth_mode_of(opts, who) == "mean" or "depth" not in out:
        return {}
    return {"depth_mode": "median", "scratch": opts.get("depth_scratch")}


@torch.no_grad()
def fused_model_rendering_into(renderer, models, typ, rays, extras, render_options, out: dict):
    """Inference-only twin of fused_model_rendering: writes just the results named in `out` (un-suffixed keys) into
    the given tensors.  The solar-correction pass runs only if one of its three results is asked for -- a point-cloud
    or image render (rgb / depth / label) does half the work of render_rays.
    render_options["geometry_only"] = True runs the geometry pass instead of the main pass: `out` may then name ops.GEOMETRY_KEYS
    only (KeyError for anything else, the solar-correction keys included), each result has the bits of the main pass, and neither
    the sun nor an embedding is looked up.
    render_options["depth_mode"] = "median": the main (or geometry) pass takes SNERF_FLAG_DEPTH_MEDIAN where `out` names 'depth'; the
    solar-correction pass never does."""
    opts = render_options or {}
    depth_kw = _depth_mode_kwargs("fused_model_rendering_into", opts, out)
    if opts.get("geometry_only"):
        for k in out:      # (before anything is looked up)
            if k in _SC_KEYS or k not in ops.GEOMETRY_KEYS:
                raise KeyError(f"fused_model_rendering_into(geometry_only): '{k}' is not a result of a geometry pass "
                               f"(have {sorted(ops.GEOMETRY_KEYS)})")
    model = models[typ]
    if opts.get("geometry_only"):
        params = dict(model.named_parameters())
        packed = opts.get("packed_params")
        if packed is None:
            packed = ops.pack_params(model.spec, params)
        pin = ops.PassInputs(rays=rays, z_vals=opts.get("given_z_vals"), z_steps=z_steps_on(rays.device, renderer.N_samples),
                             u=opts.get("perturb_rand"))
        return ops.geometry_pass_into(model.spec, params, pin, out, packed=packed, workspace=opts.get("workspace"), **depth_kw)
    sun_d, rays_t, rays_t_s, params, packed = _pass_operands(models, model, extras, opts)
    main_out = {k: v for k, v in out.items() if k not in _SC_KEYS}
    sc_out = {_SC_KEYS[k]: v for k, v in out.items() if k in _SC_KEYS}
    ws = opts.get("workspace")
    z = opts.get("given_z_vals")
    if sc_out and z is None:   # both passes must share the depths
        z = ops.sample_z(rays, z_steps_on(rays.device, renderer.N_samples), opts.get("perturb_rand"))
    pin = ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=z, z_steps=z_steps_on(rays.device, renderer.N_samples),
                         u=opts.get("perturb_rand"))
    if main_out:
        ws = ops.render_pass_into(model.spec, params, pin, rays_t, rays_t_s, main_out, packed=packed, workspace=ws, **depth_kw)
    if sc_out:
        ws = ops.render_pass_into(model.spec, params, ops.PassInputs(sun_d=sun_d, rays=rays, z_vals=z), rays_t, rays_t_s,
                                  sc_out, sc_pass=True, packed=packed, workspace=ws)
    return ws


@torch.no_grad()
def fused_model_relighting_into(renderer, models, typ, extras, render_options, out: dict):
    """The chunk that render_options["workspace"] holds -- the workspace fused_model_rendering_into returned for its main pass --
    under the sun (and embedding index) of `extras`: ops.relight_pass_into, which re-runs only what depends on the sun.  `out` takes
    the main pass's keys; a solar-correction key ('weights_sc', ...) is a KeyError: that pass samples along the sun ray itself and
    leaves nothing a new sun could reuse.  render_options["depth_mode"] as for fused_model_rendering_into, whatever the base pass's
    mode was.  Returns the workspace."""
    opts = render_options or {}
    depth_kw = _depth_mode_kwargs("fused_model_relighting_into", opts, out)
    for k in out:
        if k in _SC_KEYS:
            raise KeyError(f"fused_model_relighting_into: '{k}' belongs to the solar-correction pass, which cannot be relit "
                           "(it samples along the sun ray); render it with fused_model_rendering_into")
    ws = opts.get("workspace")
    if ws is None:
        raise ValueError("fused_model_relighting_into: render_options['workspace'] must be the workspace of the base pass")
    model = models[typ]
    allowed = set(ops.output_keys(model.spec, False)) | {"z_vals"} | ({"semantic_label"} if model.spec.n_classes > 0 else set())
    for k in out:
        if k not in allowed:
            raise KeyError(f"fused_model_relighting_into: '{k}' is not a result of the main pass (have {sorted(allowed)})")
    sun_d, rays_t, rays_t_s, params, packed = _pass_operands(models, model, extras, opts)
    return ops.relight_pass_into(model.spec, params, sun_d, rays_t, rays_t_s, out, ws, packed=packed, n_samples=renderer.n_render_samples,
                                 **depth_kw)


class RSSemanticRendering(BaseRenderer):
    def __init__(self, cfgs, inference=rs_semantic_inference):
        super().__init__(cfgs)
        self.inference_func = inference

    def _model_rendering(self, models, typ, cfgs, rays, extras, xyz, z_vals, rays_d, epoch=None, progress=1.0,
                         render_options={}) -> dict:
        return fused_model_rendering(self, models, typ, rays, extras, render_options, self.inference_func,
                                     rs_semantic_inference)
