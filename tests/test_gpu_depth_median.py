"""The median depth (SNERF_FLAG_DEPTH_MEDIAN, depth_mode="median") on the device (run with -m gpu on an MI355X).

The bar everywhere is BIT EQUALITY.  The launch against tests/raymedian_numpy.py: the spec is fp64 with every operation rounded on
its own and every sum over int64 masses, so a differing bit is a defect of the kernel or of the restatement, not a tolerance
question.  Every other result against the same pass without the flag: the flag adds one launch behind the pass and touches nothing
else.

The network is the small one of the other GPU tests (SIREN, W = 64, 3 layers with a skip), random parameters, both arithmetic modes.
Shapes: N in {1, 5, 77} -- one ray, a ragged workgroup of four waves, many workgroups -- x S in {1, 2, 63, 64, 65, 130}: the run
lengths per lane 1 -> 2 -> 3 and their boundaries.

With S = 1 the one interval is the open-ended last one: a ray's weight is 0 or 1, a saturated ray's mean IS z_0, and the median of
every ray is z_0 -- so the shape test asks for a depth that differs from the mean pass's only where S > 1 (there it fails on a
library without the flag, where the bit changes nothing); at S = 1 the comparison with the restatement is the check."""
import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import raymedian_numpy as RM
from tests.test_gpu_geometry_pass import _Mode
from tests.test_gpu_kernels import _gpu_params, _spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NET = dict(fc_units=64, fc_layers=3, fc_skips=(1,))
GEO = ("depth", "weights", "transparency", "sigmas", "z_vals")

_SETUP = {}


def _setup(N, S):
    """model and inputs, computed once per (N, S)"""
    if (N, S) not in _SETUP:
        cfg = O.OracleCfg(n_samples=S, **NET)
        spec = _spec(cfg)
        pn = O.init_params_numpy(cfg, 7)
        b = O.batch_to_torch(O.synthetic_batch(N, S, seed=41 + S))
        rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
        emb = torch.from_numpy(O.init_embedding_numpy(cfg, 7)).to(DEV)
        t = emb[extras[:, 3].long()].contiguous()
        sun2 = torch.nn.functional.normalize(extras[:, :3] + torch.tensor([0.4, -0.3, 0.2], device=DEV), dim=1).contiguous()
        _SETUP[(N, S)] = dict(cfg=cfg, spec=spec, pn=pn, gp=_gpu_params(pn, DEV), rays=rays, sun=extras[:, :3].contiguous(), sun2=sun2,
                              t=t, zs=torch.linspace(0, 1, S).to(DEV), u=u)
    return _SETUP[(N, S)]


def _pin(s, sun="sun", rays=None, z_vals=None):
    from snerf_amd import ops
    if z_vals is not None:
        return ops.PassInputs(sun_d=s[sun] if sun else None, rays=s["rays"] if rays is None else rays, z_vals=z_vals)
    return ops.PassInputs(sun_d=s[sun] if sun else None, rays=s["rays"] if rays is None else rays, z_steps=s["zs"], u=s["u"])


def _out(spec, N, S, keys=None, fill=None):
    from snerf_amd import ops
    if keys is None:
        keys = list(ops.output_keys(spec, False)) + ["z_vals"] + (["semantic_label"] if spec.n_classes > 0 else [])
    o = {}
    for k in keys:
        shape = (N,) if k == "semantic_label" else ((N, S) if k == "z_vals" else ops._OUT_SHAPES[k](N, S, spec.n_classes))
        o[k] = torch.empty(shape, dtype=torch.int64 if k == "semantic_label" else torch.float32, device=DEV)
        if fill is not None:
            o[k].view(torch.uint8).fill_(fill)
    return o


def _same(a, b):
    """bit equality (NaN equals the same NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def _assert_others_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        if k != "depth":
            assert _same(got[k], want[k]), (what, k)


def _restated(out):
    sig = out["sigmas"].cpu().numpy() if "sigmas" in out else None
    return RM.ray_median(out["weights"].cpu().numpy(), out["z_vals"].cpu().numpy(), sig)


def _assert_depth_is_restated(out, what):
    want = _restated(out)
    got = out["depth"].cpu().numpy()
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), (what, f"{int((~same).sum())} of {same.size} rays differ", got[~same][:4], want[~same][:4])


_PASSES = {}


def _passes(N, S, mode):
    """the main pass with "mean" and with "median", every result asked for; cached: the reference the tests share (never edited)"""
    from snerf_amd import ops
    if (N, S, mode) not in _PASSES:
        s = _setup(N, S)
        with _Mode(mode):
            packed = ops.pack_params(s["spec"], s["gp"])
            mean, med = _out(s["spec"], N, S), _out(s["spec"], N, S)
            ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, mean, packed=packed, depth_mode="mean")
            ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, med, packed=packed, depth_mode="median")
        torch.cuda.synchronize()
        _PASSES[(N, S, mode)] = (mean, med)
    return _PASSES[(N, S, mode)]


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("f16x2", "f16x1-fused"))
@pytest.mark.parametrize("S", (1, 2, 63, 64, 65, 130))
@pytest.mark.parametrize("N", (1, 5, 77))
def test_median_pass_equals_the_restatement_and_moves_nothing_else(N, S, mode):
    mean, med = _passes(N, S, mode)
    assert all(bool(torch.isfinite(v).all()) for k, v in mean.items() if v.is_floating_point()), (N, S, mode)
    _assert_depth_is_restated(med, (N, S, mode))
    assert bool(torch.isfinite(med["depth"]).all())
    _assert_others_same(med, mean, (N, S, mode))
    if S > 1:      # (S = 1: see the module's docstring)
        assert not _same(med["depth"], mean["depth"]), "the flag changed no depth"
        z = med["z_vals"]
        assert bool(((med["depth"] >= z[:, 0]) & (med["depth"] <= z[:, -1])).all())
    else:
        assert _same(med["depth"], med["z_vals"][:, 0].contiguous())      # the one sample, whatever its weight


# ---- 2. geometry and relight --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("f16x2", "f16x1-fused"))
@pytest.mark.parametrize("N,S", ((5, 63), (77, 65), (77, 130)))
def test_geometry_pass_takes_the_flag(N, S, mode):
    from snerf_amd import ops
    s = _setup(N, S)
    mean, med = _passes(N, S, mode)
    with _Mode(mode):
        packed = ops.pack_params(s["spec"], s["gp"])
        got = _out(s["spec"], N, S, GEO)
        ops.geometry_pass_into(s["spec"], s["gp"], _pin(s, sun=None), got, packed=packed, depth_mode="median")
        plain = _out(s["spec"], N, S, GEO)
        ops.geometry_pass_into(s["spec"], s["gp"], _pin(s, sun=None), plain, packed=packed)
    _assert_depth_is_restated(got, ("geometry", N, S, mode))
    for k in GEO:
        assert _same(got[k], med[k]), ("geometry vs main pass", k)
        assert _same(plain[k], mean[k]), ("geometry at the default", k)


@pytest.mark.parametrize("mode", ("f16x2", "f16x1-fused"))
@pytest.mark.parametrize("base_mode", ("mean", "median"))
def test_relight_takes_the_flag_after_either_base_pass(base_mode, mode):
    """the relit median under a second sun equals the median of a full pass under that sun; a relight without the flag after a base
    pass with it is the mean relight"""
    from snerf_amd import ops
    N, S = 77, 65
    s = _setup(N, S)
    with _Mode(mode):
        packed = ops.pack_params(s["spec"], s["gp"])
        full_med, full_mean = _out(s["spec"], N, S), _out(s["spec"], N, S)
        ops.render_pass_into(s["spec"], s["gp"], _pin(s, sun="sun2"), s["t"], None, full_med, packed=packed, depth_mode="median")
        ops.render_pass_into(s["spec"], s["gp"], _pin(s, sun="sun2"), s["t"], None, full_mean, packed=packed)
        ws = ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, _out(s["spec"], N, S), packed=packed, depth_mode=base_mode)
        relit = _out(s["spec"], N, S)
        assert ops.relight_pass_into(s["spec"], s["gp"], s["sun2"], s["t"], None, relit, ws, packed=packed, depth_mode="median") is ws
        relit_mean = _out(s["spec"], N, S)
        ops.relight_pass_into(s["spec"], s["gp"], s["sun2"], s["t"], None, relit_mean, ws, packed=packed)
        only = {"depth": torch.empty(N, device=DEV)}      # the depth alone: ops' scratch, S from n_samples
        ops.relight_pass_into(s["spec"], s["gp"], s["sun2"], s["t"], None, only, ws, packed=packed, n_samples=S, depth_mode="median")
    torch.cuda.synchronize()
    _assert_depth_is_restated(relit, ("relight", base_mode, mode))
    for k in full_med:
        assert _same(relit[k], full_med[k]), ("relit median vs full pass", k)
        assert _same(relit_mean[k], full_mean[k]), ("relit mean vs full pass", k)
    assert _same(only["depth"], full_med["depth"])
    assert not _same(full_med["depth"], full_mean["depth"])


# ---- 3. scratch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", (False, True), ids=("main", "geometry"))
def test_ops_scratch_stands_in_for_weights_and_z_vals(geometry):
    from snerf_amd import ops
    N, S = 77, 65
    s = _setup(N, S)
    _, med = _passes(N, S, "f16x2")
    packed = ops.pack_params(s["spec"], s["gp"])
    t = None if geometry else s["t"]
    pin = _pin(s, sun=None if geometry else "sun")
    scratch = {}
    a = {"depth": torch.empty(N, device=DEV)}
    ws = ops.render_pass_into(s["spec"], s["gp"], pin, t, None, a, packed=packed, geometry=geometry, depth_mode="median", scratch=scratch)
    assert set(scratch) == {"weights", "z_vals", "sigmas"} and all(v.numel() >= N * S and v.dtype == torch.float32 for v in scratch.values())
    kept = dict(scratch)
    b = {"depth": torch.empty(N, device=DEV)}
    ops.render_pass_into(s["spec"], s["gp"], pin, t, None, b, packed=packed, workspace=ws, geometry=geometry, depth_mode="median", scratch=scratch)
    assert all(scratch[k] is kept[k] for k in kept), "the scratch tensors were not reused"
    m = 5      # a ragged last chunk: fewer rays on the same scratch
    s5 = _setup(m, S)
    c = {"depth": torch.empty(m, device=DEV)}
    ops.render_pass_into(s5["spec"], s5["gp"], _pin(s5, sun=None if geometry else "sun"), None if geometry else s5["t"], None, c,
                         packed=packed, geometry=geometry, depth_mode="median", scratch=scratch)
    assert all(scratch[k] is kept[k] for k in kept)
    d = {"depth": torch.empty(N, device=DEV), "weights": torch.empty(N, S, device=DEV)}      # one of the two named: the other from scratch
    ops.render_pass_into(s["spec"], s["gp"], pin, t, None, d, packed=packed, geometry=geometry, depth_mode="median", scratch=scratch)
    e = {"depth": torch.empty(N, device=DEV)}      # no dict given: tensors of the call's own
    ops.render_pass_into(s["spec"], s["gp"], pin, t, None, e, packed=packed, geometry=geometry, depth_mode="median")
    torch.cuda.synchronize()
    for got in (a, b, d, e):
        assert _same(got["depth"], med["depth"])
    assert _same(d["weights"], med["weights"])
    assert _same(c["depth"], _passes(m, S, "f16x2")[1]["depth"])
    assert _same(scratch["weights"][:m * S].view(m, S), _passes(m, S, "f16x2")[1]["weights"])      # what the last pass left there


# ---- 4. degenerate rays through the network -----------------------------------------------------------------------------------------
def _with_sigma_bias(s, value):
    gp = dict(s["gp"])
    gp["sigma_from_xyz.0.bias"] = torch.full_like(gp["sigma_from_xyz.0.bias"], value)
    return gp


@pytest.mark.parametrize("S", (2, 65))
def test_empty_and_saturated_rays(S):
    from snerf_amd import ops
    N = 5
    s = _setup(N, S)
    out = _out(s["spec"], N, S, GEO)
    ops.geometry_pass_into(s["spec"], _with_sigma_bias(s, -1e4), _pin(s, sun=None), out, depth_mode="median")
    assert float(out["weights"].abs().max()) == 0.0
    assert _same(out["depth"], out["z_vals"][:, S - 1].contiguous())      # nothing on the ray: the far end
    _assert_depth_is_restated(out, "empty")
    out = _out(s["spec"], N, S, GEO)
    ops.geometry_pass_into(s["spec"], _with_sigma_bias(s, 1e4), _pin(s, sun=None), out, depth_mode="median")
    assert bool((out["weights"][:, 0] > 0.5).all())
    z = out["z_vals"]
    assert bool(((out["depth"] >= z[:, 0]) & (out["depth"] <= z[:, 1])).all())      # the mass in the first interval
    _assert_depth_is_restated(out, "saturated")


def _duplicated_depths(s, N, S):
    near, far = s["rays"][:, 6:7], s["rays"][:, 7:8]
    g = torch.Generator().manual_seed(3)
    z = (near + (far - near) * torch.sort(torch.rand(N, S, generator=g), dim=1).values.to(DEV)).float()
    z[:, 1::3] = z[:, 0:-1:3][:, :z[:, 1::3].shape[1]].clone()      # every third depth repeats its neighbour: intervals of no length
    z = z.contiguous()
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((z[:, 1] == z[:, 0]).all())
    return z


def test_explicit_depths_with_duplicates():
    from snerf_amd import ops
    N, S = 130, 64
    s = _setup(N, S)
    z = _duplicated_depths(s, N, S)
    out = _out(s["spec"], N, S)
    ops.render_pass_into(s["spec"], s["gp"], _pin(s, z_vals=z), s["t"], None, out, depth_mode="median")
    assert _same(out["z_vals"], z) and bool(torch.isfinite(out["depth"]).all())
    _assert_depth_is_restated(out, "duplicated depths")
    assert bool(((out["depth"] >= z[:, 0]) & (out["depth"] <= z[:, -1])).all())


def _nan_ray_run(column, seam):
    """130 x 64 with a NaN in `column` of the LAST ray's row of `rays` (its points are rows 129 * 64 ..: the last 128-row block of the
    activations, which it shares with ray 128 alone) -> (the clean median pass, the pass with the NaN)"""
    from snerf_amd import ops
    N, S = 130, 64
    s = _setup(N, S)
    packed = ops.pack_params(s["spec"], s["gp"])
    z = _duplicated_depths(s, N, S) if seam == "given" else None
    clean = _out(s["spec"], N, S)
    ops.render_pass_into(s["spec"], s["gp"], _pin(s, z_vals=z), s["t"], None, clean, packed=packed, depth_mode="median")
    rays = s["rays"].clone()
    rays[N - 1, column] = float("nan")
    got = _out(s["spec"], N, S)
    ops.render_pass_into(s["spec"], s["gp"], _pin(s, rays=rays, z_vals=z), s["t"], None, got, packed=packed, depth_mode="median")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(clean["depth"]).all())
    return clean, got


@pytest.mark.parametrize("seam", ("sampled", "given"))
def test_a_ray_with_a_nan_origin(seam):
    """A NaN origin gives a NaN depth and leaves the other rays alone.  The pass writes sigmas = NaN for that ray but weights = 0.0 for
    every sample -- the composite takes fmaxf(sigma, 0), which drops a NaN -- and finite z_vals: by the weights alone the ray would
    read as empty (depth z_{S-1}; the mean pass gives 0.0).  The launch is therefore handed the sigmas the pass wrote (named in `out`
    here, ops' scratch otherwise: test_the_nan_origin_is_seen_through_ops_scratch), and a sigma that is not finite makes the ray bad."""
    N = 130
    clean, got = _nan_ray_run(0, seam)
    _assert_depth_is_restated(got, "NaN origin")      # (covers ray 128, whatever the shared block did to its weights)
    assert _same(got["depth"][:N - 2], clean["depth"][:N - 2]), "a NaN ray moved the depth of a ray in another block"
    print(f"NaN origin ({seam}): depth {float(got['depth'][N - 1])!r}, weights sum {float(got['weights'][N - 1].sum())!r}, "
          f"sigmas finite {bool(torch.isfinite(got['sigmas'][N - 1]).all())}, z_last {float(got['z_vals'][N - 1, -1])!r}")
    assert bool(torch.isnan(got["depth"][N - 1])), float(got["depth"][N - 1])


@pytest.mark.parametrize("geometry", (False, True), ids=("main", "geometry"))
def test_the_nan_origin_is_seen_through_ops_scratch(geometry):
    """`out` names the depth alone: the sigmas the launch reads are ops' scratch; and a relight of that chunk sees the ray as well"""
    from snerf_amd import ops
    N, S = 130, 64
    s = _setup(N, S)
    packed = ops.pack_params(s["spec"], s["gp"])
    rays = s["rays"].clone()
    rays[N - 1, 4] = float("nan")      # (the direction this time)
    got, clean = ({"depth": torch.empty(N, device=DEV)} for _ in range(2))
    t = None if geometry else s["t"]
    sun = None if geometry else "sun"
    ops.render_pass_into(s["spec"], s["gp"], _pin(s, sun=sun), t, None, clean, packed=packed, geometry=geometry, depth_mode="median")
    ws = ops.render_pass_into(s["spec"], s["gp"], _pin(s, sun=sun, rays=rays), t, None, got, packed=packed, geometry=geometry, depth_mode="median")
    relit = {"depth": torch.empty(N, device=DEV)}
    if not geometry:
        ops.relight_pass_into(s["spec"], s["gp"], s["sun2"], s["t"], None, relit, ws, packed=packed, n_samples=S, depth_mode="median")
    torch.cuda.synchronize()
    for d in (got,) if geometry else (got, relit):
        assert bool(torch.isnan(d["depth"][N - 1]))
        assert _same(d["depth"][:N - 2], clean["depth"][:N - 2]) and bool(torch.isfinite(d["depth"][:N - 2]).all())


def test_a_nan_that_reaches_the_depths():
    """a NaN `near` makes the sampled depths of the ray NaN, and with them its weights: the ray is bad, its depth a NaN; the others keep
    their bits"""
    N = 130
    clean, got = _nan_ray_run(6, "sampled")
    assert bool(torch.isnan(got["z_vals"][N - 1]).all())
    assert bool(torch.isnan(got["depth"][N - 1]))
    assert _same(got["depth"][:N - 2], clean["depth"][:N - 2])
    _assert_depth_is_restated(got, "NaN near")


# ---- 5. frame walks -------------------------------------------------------------------------------------------------------------
def _walk_pipeline(n_importance=0, S=24):
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=64, n_samples=S, render_chunk_size=64)
    extra = {"n_importance": n_importance} if n_importance else {}
    pipe, _ = _pipeline_for(cfg, 64, 5, **extra)
    n = 3 * 67
    b = O.batch_to_torch(O.synthetic_batch(n, S, seed=17))
    return pipe, n, b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)


def test_lean_inference_with_a_ragged_last_chunk_equals_one_pass():
    from snerf_amd.eval.utils.util import lean_inference, result_buffers
    S = 24
    pipe, n, rays, extras, u = _walk_pipeline(S=S)
    ro = {"perturb_rand": u, "depth_mode": "median"}
    keys = ("rgb_coarse", "depth_coarse", "semantic_label_coarse")      # no per-sample result: weights and z_vals are ops' scratch
    walk = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=ro)
    one = result_buffers(keys + ("weights_coarse",), n, S, pipe.model_coarse.spec.n_classes, DEV)
    one["z_vals_coarse"] = torch.empty(n, S, device=DEV)
    pipe.renderer.render_rays_into(pipe.models, rays, extras, one, ro)
    mean = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options={"perturb_rand": u})
    torch.cuda.synchronize()
    for k in keys:
        assert _same(walk[k], one[k]), k
    _assert_depth_is_restated({"depth": one["depth_coarse"], "weights": one["weights_coarse"], "z_vals": one["z_vals_coarse"]}, "one pass")
    assert _same(mean["rgb_coarse"], walk["rgb_coarse"]) and not _same(mean["depth_coarse"], walk["depth_coarse"])


def test_the_final_pass_of_a_resampled_render_takes_the_flag(monkeypatch):
    from snerf_amd import ops
    from snerf_amd.eval.utils.util import lean_inference, result_buffers
    S, Ni = 7, 5
    pipe, n, rays, extras, u = _walk_pipeline(n_importance=Ni, S=S)
    ui = torch.rand(n, Ni, generator=torch.Generator().manual_seed(4)).to(DEV)
    ro = {"perturb_rand": u, "importance_rand": ui, "depth_mode": "median"}
    seen = []
    keep = ops.render_pass_into

    def into(*a, **k):
        seen.append((bool(k.get("geometry")), k.get("depth_mode", "mean")))
        return keep(*a, **k)

    monkeypatch.setattr(ops, "render_pass_into", into)
    walk = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=("depth_coarse", "rgb_coarse"), render_options=ro)
    assert seen == [(True, "mean"), (False, "median")] * 4      # per chunk: the proposal without the flag, the final pass with it
    one = result_buffers(("depth_coarse", "weights_coarse"), n, S + Ni, pipe.model_coarse.spec.n_classes, DEV)
    one["z_vals_coarse"] = torch.empty(n, S + Ni, device=DEV)
    pipe.renderer.render_rays_into(pipe.models, rays, extras, one, ro)
    torch.cuda.synchronize()
    assert one["z_vals_coarse"].shape == (n, S + Ni)
    _assert_depth_is_restated({"depth": one["depth_coarse"], "weights": one["weights_coarse"], "z_vals": one["z_vals_coarse"]}, "merged depths")
    assert _same(walk["depth_coarse"], one["depth_coarse"])


def test_extract_pointcloud_places_the_points_at_the_median(monkeypatch):
    from snerf_amd import ops
    from snerf_amd.eval.extract_pointcloud import extract_pointcloud, get_xyz_from_nerf_prediction
    from snerf_amd.eval.utils.util import lean_inference
    pipe, n, rays, extras, u = _walk_pipeline()
    ro = {"perturb_rand": u}
    want = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=("depth_coarse", "weights_coarse", "rgb_coarse"),
                          render_options=dict(ro, depth_mode="median"))["depth_coarse"]
    seen = []
    keep = ops.render_pass_into

    def into(*a, **k):
        seen.append((bool(k.get("geometry")), k.get("depth_mode", "mean")))
        return keep(*a, **k)

    monkeypatch.setattr(ops, "render_pass_into", into)
    cloud = extract_pointcloud(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro, with_colors=False,
                               with_labels=False, depth_mode="median")
    mean = extract_pointcloud(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro, with_colors=False, with_labels=False)
    torch.cuda.synchronize()
    assert seen == [(True, "median")] * 4 + [(True, "mean")] * 4      # the automatic geometry walk, chunks of 64, 64, 64, 9
    assert _same(cloud["depth"], want)
    assert _same(cloud["xyz_n"], get_xyz_from_nerf_prediction(rays, want))
    assert not _same(mean["depth"], cloud["depth"])


# ---- 6. no dependence on unwritten bytes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,mode", ((77, 65, "f16x2"), (5, 130, "f16x1-fused")))
def test_no_result_depends_on_bytes_the_library_did_not_write(N, S, mode, monkeypatch):
    """the harness of tests/test_gpu_fill.py: depth, weights, z_vals, ops' scratch and the workspace carry 0x00 / 0xFF / 0x7B before
    the call; bit-identical under every fill, every element written, and the bits of the cached pass"""
    from snerf_amd import ops
    from tests.test_gpu_fill import _poison, run_filled
    s = _setup(N, S)
    _, med = _passes(N, S, mode)

    def run(fill):
        _poison(monkeypatch, fill)      # the workspace and the scratch are ops' own allocations: they carry the fill
        with _Mode(mode):
            packed = ops.pack_params(s["spec"], s["gp"])
            named = _out(s["spec"], N, S, ("depth", "weights", "z_vals"), fill=fill)
            ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, named, packed=packed, depth_mode="median")
            alone = _out(s["spec"], N, S, ("depth",), fill=fill)
            scratch = {}
            ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, alone, packed=packed, depth_mode="median", scratch=scratch)
            geo = _out(s["spec"], N, S, ("depth",), fill=fill)
            ops.geometry_pass_into(s["spec"], s["gp"], _pin(s, sun=None), geo, packed=packed, depth_mode="median", scratch=scratch)
        torch.cuda.synchronize()
        return {"named_depth": named["depth"], "named_weights": named["weights"], "named_z": named["z_vals"],
                "alone_depth": alone["depth"], "geo_depth": geo["depth"], "scratch_weights": scratch["weights"][:N * S].clone()}

    r = run_filled(run)[0xFF]
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
    for k in ("named_depth", "alone_depth", "geo_depth"):
        assert _same(r[k], med["depth"]), k
    assert _same(r["named_weights"], med["weights"]) and _same(r["scratch_weights"].view(N, S), med["weights"])


# ---- 7. the default is untouched ------------------------------------------------------------------------------------------------------
def test_the_default_calls_the_library_exactly_as_before(monkeypatch):
    """the library queues the extra launch if and only if the descriptor carries the bit (one `if` behind the pass in snerf_forward):
    at "mean" -- spelled out or not -- every call into the library and its descriptor flags are those of a call without the argument,
    and "median" differs from them in that one bit of the one snerf_forward alone"""
    from snerf_amd import ops, _lib
    N, S = 77, 65
    s = _setup(N, S)
    packed = ops.pack_params(s["spec"], s["gp"])
    calls = []
    keep = _lib.call

    def call(name, *a, **k):
        calls.append((name, int(a[0].flags) if a and isinstance(a[0], _lib.SnerfDesc) else None))
        return keep(name, *a, **k)

    monkeypatch.setattr(_lib, "call", call)

    def traced(**kw):
        calls.clear()
        out = _out(s["spec"], N, S)
        ws = ops.render_pass_into(s["spec"], s["gp"], _pin(s), s["t"], None, out, packed=packed, **kw)
        geo = _out(s["spec"], N, S, GEO)
        ops.geometry_pass_into(s["spec"], s["gp"], _pin(s, sun=None), geo, packed=packed, **kw)
        ops.relight_pass_into(s["spec"], s["gp"], s["sun2"], s["t"], None, _out(s["spec"], N, S), ws, packed=packed, **kw)
        return list(calls)

    bare, mean, med = traced(), traced(depth_mode="mean"), traced(depth_mode="median")
    assert [c[0] for c in bare] == ["snerf_forward"] * 3
    assert bare == mean and all(c[1] & _lib.FLAG_DEPTH_MEDIAN == 0 for c in bare)
    assert med == [(n, f | _lib.FLAG_DEPTH_MEDIAN) for n, f in bare]
