"""batched_inference -- mirror of eval/utils/util.py:13-42: no-grad, render_chunk_size rays at a time."""
from collections import defaultdict

import torch

from ...framework.components.rendering import bare_key as _bare, depth_mode_of, n_render_samples, z_steps_on

_PER_RAY_OPTIONS = ("perturb_rand", "given_z_vals", "importance_rand")   # (N, S) / (N, S') / (N, Ni) tensors a caller may pin for the whole frame


def with_depth_mode(render_options, depth_mode, who="depth_mode"):
    """`render_options` for a consumer's depth_mode= argument: unchanged (the same object) at "mean", so that the default walk is the
    walk it always was; a copy that carries {"depth_mode": "median"} otherwise.  Anything else is a ValueError."""
    depth_mode_of({"depth_mode": depth_mode}, who)
    if depth_mode == "mean":
        return render_options
    opts = dict(render_options) if render_options else {}
    opts["depth_mode"] = depth_mode
    return opts


def _chunk_options(render_options, i, chunk, n):
    """render options of the chunk starting at ray i: per-ray tensors given for the whole frame are sliced"""
    opts = dict(render_options) if render_options else {}
    for k in _PER_RAY_OPTIONS:
        v = opts.get(k)
        if torch.is_tensor(v) and v.shape[0] == n and n > chunk:
            opts[k] = v[i:i + chunk]
    return opts


@torch.no_grad()
def batched_inference(cfgs, renderer, models, rays, extras, render_options={}, epoch=None, show_tqdm=False):
    chunk = cfgs.pipeline.render_chunk_size
    parts = defaultdict(list)
    steps = range(0, rays.shape[0], chunk)
    if show_tqdm:
        from tqdm import tqdm
        steps = tqdm(steps)
    for i in steps:
        r = renderer.render_rays(models, rays[i:i + chunk], extras[i:i + chunk] if extras is not None else None,
                                 epoch=epoch, render_options=_chunk_options(render_options, i, chunk, rays.shape[0]))
        for k, v in r.items():
            parts[k].append(v)
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in parts.items()}


_KEY_SHAPES = {  # per-ray trailing shape of the render_rays results (S = n_render_samples: n_samples + n_importance, C = classes)
    "rgb": lambda S, C: (3,), "depth": lambda S, C: (), "weights": lambda S, C: (S,), "transparency": lambda S, C: (S,),
    "albedo": lambda S, C: (S, 3), "sun": lambda S, C: (S, 1), "sky": lambda S, C: (S, 3), "beta": lambda S, C: (S, 1),
    "sigmas": lambda S, C: (S,), "beta_semantic": lambda S, C: (S, 1), "semantic_logits": lambda S, C: (C,),
    "semantic_label": lambda S, C: (), "weights_sc": lambda S, C: (S,), "transparency_sc": lambda S, C: (S,),
    "sun_sc": lambda S, C: (S, 1),
}


def result_buffers(keys, rows, S, n_classes, device) -> dict:
    """uninitialised render_rays_into result tensors of `rows` rays for the results `keys` (with or without the `_coarse`
    postfix), under their `_coarse` names"""
    return {_bare(k) + "_coarse": torch.empty((rows,) + _KEY_SHAPES[_bare(k)](S, n_classes),
                                              dtype=torch.int64 if _bare(k) == "semantic_label" else torch.float32, device=device)
            for k in keys}


def shard_options(render_options, lo, hi, n):
    """render options of the rays [lo, hi) of an n-ray frame: per-ray tensors given for the whole frame are sliced"""
    return _chunk_options(render_options, lo, hi - lo, n) if n > hi - lo else render_options


def render_chunks(cfgs, renderer, models, rays, extras, buffers, render_options, frame_sized=False, show_tqdm=False):
    """The chunk loop of the lean evaluators: renders `rays` render_chunk_size rays at a time into `buffers` (result_buffers)
    with render_rays_into, the weights packed once and the inference workspace carried from chunk to chunk, and yields
    (i, k, views) after the chunk of k rays starting at ray i: views = buffers[key][i:i + k] of frame-sized buffers,
    buffers[key][:k] of chunk-sized ones.  The order of the render calls, and with it the jitter drawn from torch's generator,
    is the chunks' order.  A caller allocates its buffers after ops.release_workspaces(): full-frame inference has its own
    memory profile, and the idle TRAINING workspaces (8-20 GB each, held outside torch's allocator by the lease pool) go back
    to torch first, so that the frame's tensors and the inference workspace can use that memory."""
    if frame_sized:      # a sun axis of one: the same memory
        buffers = {key: v[None] for key, v in buffers.items()}
    for i, k, _, views in relight_chunks(cfgs, renderer, models, rays, extras, (None,), buffers, render_options, frame_sized, show_tqdm):
        yield i, k, views


@torch.no_grad()
def lean_inference(cfgs, renderer, models, rays, extras, keys=("rgb_coarse", "depth_coarse", "semantic_label_coarse"),
                   render_options={}, show_tqdm=False):
    """Full-frame inference for image / point-cloud extraction (eval/extract_pointcloud.py:66-79 calls
    batched_inference and then reads only rgb and depth): the full-frame result tensors are allocated once, every
    chunk of render_chunk_size rays writes its rows in place, only the requested results are produced (no per-sample
    tensors unless asked for), the solar-correction pass is skipped unless one of its results is requested, and the
    weights are packed once for all chunks."""
    from ... import ops
    for k in keys:
        if _bare(k) not in _KEY_SHAPES:
            raise KeyError(f"lean_inference: unknown result '{k}'")
    ops.release_workspaces()
    out = result_buffers(keys, rays.shape[0], n_render_samples(cfgs.pipeline), models["coarse"].spec.n_classes, rays.device)
    for _ in render_chunks(cfgs, renderer, models, rays, extras, out, render_options, frame_sized=True, show_tqdm=show_tqdm):
        pass
    return out


def sun_extras(extras, sun, device=None):
    """`extras` (n, 4) with its sun columns replaced by the direction of `sun` = (elevation_deg, azimuth_deg): the reference's
    convention (baseline/components/rays.py construct_sun_dir: fp64, rounded once), the embedding index column kept"""
    from ...baseline.components import rays as R
    from ...framework.components.rays import extras_component_fn
    el, az = sun
    e = extras.clone()
    extras_component_fn(e, "sun_d", R.construct_sun_dir(float(el), float(az), 1).to(e.device))
    return e


def relight_chunks(cfgs, renderer, models, rays, extras, suns, buffers, render_options, frame_sized=False, show_tqdm=False):
    """render_chunks over a list of suns, the chunk loop run ONCE: per chunk one base pass under suns[0] (render_rays_into: it
    draws the chunk's jitter, so all suns of a sweep share their depths) and one relight per further sun (relight_rays_into on
    the base pass's workspace: only the sun-dependent part of the pass).  `suns`: (elevation_deg, azimuth_deg) pairs; the sun
    columns of `extras` are replaced by each in turn (sun_extras).  Yields (i, k, sun_index, views) after every pass, suns in
    order within a chunk.  `buffers`: chunk-sized result_buffers, reused for every sun -- views = buffers[key][:k], to be consumed
    before the next yield -- or, with frame_sized, tensors with a leading sun axis, (K, n, ...): views = buffers[key][s, i:i + k].
    Every sun is asked for the same results, those of `buffers`.  A sun of None stands for `extras` as they are, None included:
    render_chunks is the walk under that one sun.  The walk owns the pack of the weights (once), the workspace carried from pass
    to pass, the chunk steps and the per-chunk options.
    A single-sun walk (suns == (None,)) whose results all lie in ops.GEOMETRY_KEYS (depth, weights, transparency, sigmas, z_vals)
    runs every chunk as a geometry pass (render_options["geometry_only"]): the same bits without the head launches.  A walk with
    more suns never does: its base pass must leave a workspace that can be relit.
    render_options["depth_mode"] = "median" reaches every pass of the walk that writes 'depth' -- geometry passes and relights
    included -- and the scratch tensors those passes may need (ops.render_pass_into: scratch=) are allocated for the first chunk and
    carried in render_options["depth_scratch"], like the workspace."""
    from ... import ops
    median = depth_mode_of(render_options, "relight_chunks") != "mean"
    scratch = (render_options or {}).get("depth_scratch") if median else None
    if median and scratch is None:
        scratch = {}
    suns = list(suns)
    if not suns:
        raise ValueError("relight_chunks: no sun")
    geometry_walk = suns == [None] and len(buffers) > 0 and all(_bare(key) in ops.GEOMETRY_KEYS for key in buffers)
    chunk = cfgs.pipeline.render_chunk_size
    n = rays.shape[0]
    model = models["coarse"]
    packed = ops.pack_params(model.spec, dict(model.named_parameters()))
    ws = None
    steps = range(0, n, chunk)
    if show_tqdm:
        from tqdm import tqdm
        steps = tqdm(steps)
    for i in steps:
        k = min(chunk, n - i)
        opts = _chunk_options(render_options, i, chunk, n)
        opts["packed_params"] = packed
        if median:
            opts["depth_scratch"] = scratch
        if geometry_walk:
            opts["geometry_only"] = True
        ex = extras[i:i + chunk] if extras is not None else None
        for s, sun in enumerate(suns):
            views = {key: v[s, i:i + k] if frame_sized else v[:k] for key, v in buffers.items()}
            opts["workspace"] = ws
            e = ex if sun is None else sun_extras(ex, sun)
            if s == 0:
                ws = renderer.render_rays_into(models, rays[i:i + chunk], e, views, opts)
            else:
                ws = renderer.relight_rays_into(models, e, views, opts)
            yield i, k, s, views


@torch.no_grad()
def lean_relight(cfgs, renderer, models, rays, extras, suns, keys=("rgb_coarse",), render_options={}, show_tqdm=False):
    """lean_inference under every sun of `suns` ((elevation_deg, azimuth_deg) pairs) for the cost of one walk plus the
    sun-dependent part per further sun: each result of `keys` stacked over the suns, (K, N, ...).  Entry k has the bits of
    lean_inference with the sun columns of `extras` set to sun k -- given the same depths, i.e. {"perturb": 0} or a pinned
    "perturb_rand" (the jitter is drawn once per chunk, by the base pass, and shared by the suns)."""
    from ... import ops
    for k in keys:
        if _bare(k) not in _KEY_SHAPES or _bare(k).endswith("_sc"):
            raise KeyError(f"lean_relight: '{k}' is not a result of the main pass")
    suns = list(suns)
    if not suns:
        raise ValueError("lean_relight: no sun")
    ops.release_workspaces()
    one = result_buffers(keys, 0, n_render_samples(cfgs.pipeline), models["coarse"].spec.n_classes, rays.device)
    out = {k: torch.empty((len(suns), rays.shape[0]) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device) for k, v in one.items()}
    for _ in relight_chunks(cfgs, renderer, models, rays, extras, suns, out, render_options, frame_sized=True, show_tqdm=show_tqdm):
        pass
    return out


PER_RAY_RESULTS = ("rgb", "depth", "semantic_label", "semantic_logits")   # (N, ...) results: what a frame / point cloud is made of


@torch.no_grad()
def guided_lean_inference(cfgs, renderer, models, rays, extras, guide, keys=("rgb_coarse", "depth_coarse", "semantic_label_coarse"),
                          render_options={}, show_tqdm=False):
    """lean_inference with the samples of every ray that meets a DSM placed in a band round the hit, not over the whole
    [near, far] slab.  `guide` (eval/utils/raycast.py DsmGuide) carries frame, grid, dsm, bias, front_m,
    back_m and n_samples: the rays are cast on the DSM (raycast.cast_rays), the near / far of the rows that hit are narrowed
    (raycast.guide_rays), ops.sample_z spreads guide.n_samples depths over every ray's -- narrowed or full -- bounds without jitter,
    and lean_inference renders the guided rays under {"given_z_vals": z, "perturb": 0}.  A pass costs about in proportion to its
    samples, so a quarter of the samples is about a quarter of the render.  Rows without a hit (END, OUTSIDE) are rendered over their
    full bounds with the same guide.n_samples.
    Only per-ray results may be asked for (PER_RAY_RESULTS and 'depth'): a per-sample key is a KeyError, because the frame buffers
    take their width from the config, not from the guide.  `given_z_vals` bypasses the proposal pass, so n_importance is not
    honoured here: the guide takes its place.  render_options may not pin depths or jitter of its own ("given_z_vals",
    "perturb_rand", "importance_rand": ValueError).  render_options["depth_mode"] = "median" works at the guided width: the median
    launch takes its sample count from the pass, and its scratch is sized by it (ops.render_pass_into).
    Returns lean_inference's results plus "guide_state" (n) u8, the cast's state per ray (raycast.TOP ... raycast.BAD)."""
    from ... import ops
    from . import raycast
    for k in keys:
        if _bare(k) not in _KEY_SHAPES:
            raise KeyError(f"guided_lean_inference: unknown result '{k}'")
        if _bare(k) not in PER_RAY_RESULTS:
            raise KeyError(f"guided_lean_inference: '{k}' is a per-sample result; only per-ray results {PER_RAY_RESULTS} can be asked "
                           "for (the frame buffers take their width from the config, not from the guide)")
    for k in _PER_RAY_OPTIONS:
        if (render_options or {}).get(k) is not None:
            raise ValueError(f"guided_lean_inference: render_options['{k}'] cannot be pinned: the guide places the depths")
    S = int(guide.n_samples)
    if S < 1:
        raise ValueError(f"guided_lean_inference: guide.n_samples = {guide.n_samples} must be >= 1")
    cast = raycast.cast_rays(rays, guide.frame, guide.grid, guide.dsm, guide.bias)
    guided, _ = raycast.guide_rays(rays, cast, guide.front_m, guide.back_m, guide.frame.params.range)
    opts = dict(render_options) if render_options else {}
    opts["given_z_vals"] = ops.sample_z(guided[:, :8], z_steps_on(rays.device, S), None)      # (snerf_sample_z reads rows of 8 columns)
    opts["perturb"] = 0
    out = lean_inference(cfgs, renderer, models, guided, extras, keys=keys, render_options=opts, show_tqdm=show_tqdm)
    out["guide_state"] = cast["state"]
    return out


def shard_and_gather(render_rows, n: int, rank: int = None, world: int = None) -> dict:
    """`render_rows(lo, hi)` -> dict of results for the rays [lo, hi) of an n-ray frame; this rank renders its contiguous
    slice (parallel.frame_shard) and the per-ray results (PER_RAY_RESULTS, with or without the `_coarse` postfix) are
    all-gathered into full-frame tensors on every rank -- ragged tails and empty shards included.  Per-sample results
    ((N, S, ...): weights, sigmas, ...) stay local under their key; `out["_rows"]` = (lo, hi) names the rows they cover."""
    from ... import parallel
    lo, hi = parallel.frame_shard(n, rank, world)
    local = render_rows(lo, hi)
    out = {"_rows": (lo, hi)}
    for k, v in local.items():
        out[k] = parallel.allgather_rows(v, n) if _bare(k) in PER_RAY_RESULTS else v
    return out


@torch.no_grad()
def sharded_lean_inference(cfgs, renderer, models, rays, extras, keys=("rgb_coarse", "depth_coarse", "semantic_label_coarse"),
                           render_options={}, show_tqdm=False):
    """lean_inference with the frame's rays sharded over the ranks of the process group (SURVEY 8(e), config 5's full-frame
    half; reference callers eval/utils/util.py:13-42, eval/extract_pointcloud.py:66-114 are single-device): every rank holds
    the frame's rays, renders rows frame_shard(n) of them and receives the per-ray results of all ranks; the exchange is one
    all_gather per requested per-ray result (rgb: 12 B, depth: 4 B, label: 8 B per ray).  Equal to lean_inference on one rank
    bit for bit (rays are independent; per-ray jitter given for the whole frame is sliced with the rays)."""
    n = rays.shape[0]

    def rows(lo, hi):
        if hi == lo:      # more ranks than rays: contribute nothing (a zero-ray launch has no defined result)
            return result_buffers(keys, 0, n_render_samples(cfgs.pipeline), models["coarse"].spec.n_classes, rays.device)
        return lean_inference(cfgs, renderer, models, rays[lo:hi], extras[lo:hi] if extras is not None else None, keys=keys,
                              render_options=shard_options(render_options, lo, hi, n), show_tqdm=show_tqdm)
    return shard_and_gather(rows, n)
