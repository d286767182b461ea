"""Importance resampling of the depths on the device (snerf_resample_z, ops.resample_z, the renderers' proposal pass; DESIGN.md
section 5p).  Run with -m gpu on an MI355X.

The bar everywhere is BIT EQUALITY.  The kernel against tests/resample_numpy.py: the spec is fp64 with every operation rounded on
its own and integer sums, so it has one result.  The renderer against the manual chain -- proposal pass, the restatement on the
host, the same pass on the merged depths through `given_z_vals`: the same kernels on operands that must be bit-identical."""
import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import resample_numpy as RN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 3, 1), (5, 3, 7), (77, 7, 5), (130, 64, 64), (33, 65, 63), (9, 130, 200), (2, 512, 512), (5, 1021, 3)]
FAMILIES = 6


def _weights_row(rng, S, family):
    """0 random, 1 peaked with exact zeros, 2 all zero, 3 / 4 a one-hot at the first / last interior sample, 5 a row with NaN, -1,
    +Inf and 2.0 among random weights"""
    w = np.zeros(S, np.float32)
    if family == 0:
        r = rng.random(S) ** 3
        w[:] = (r / r.sum() * rng.uniform(0.3, 1.0)).astype(np.float32)
    elif family == 1:
        k0 = int(rng.integers(1, max(S - 3, 2)))
        w[k0:min(k0 + 3, S - 1)] = rng.uniform(0.05, 0.3, min(k0 + 3, S - 1) - k0).astype(np.float32)
    elif family == 3:
        w[1] = 1.0
    elif family == 4:
        w[S - 2] = 0.75
    elif family == 5:
        w[:] = rng.uniform(0.0, 0.1, S).astype(np.float32)
        for i, v in enumerate((np.nan, -1.0, np.inf, 2.0)):
            w[1 + (int(rng.integers(0, S - 2)) + i) % (S - 2)] = v      # interior (for S - 2 < 4 the later ones overwrite)
    return w


def _case(N, S, Ni, shift):
    rng = np.random.default_rng(100000 * shift + 1000 * S + Ni + N)
    z = np.sort(rng.uniform(0.25, 4.0, (N, S)).astype(np.float32), 1)
    z[0, 1::2] = z[0, 0:S - 1:2]                                        # repeated depths
    r = 1 % N
    z[r, 0], z[r, 1] = -0.0, 0.0                                        # signed zeros (equal values: still non-decreasing)
    w = np.stack([_weights_row(rng, S, (n + shift) % FAMILIES) for n in range(N)])
    u = rng.random((N, Ni)).astype(np.float32)
    special = (0.0, np.nextafter(np.float32(1), np.float32(0)), 1.0, 0.5)
    for i in range(min(Ni, 4)):
        u[0, i] = special[(i + shift) % 4]
    if Ni > 5:
        u[0, 5:5 + Ni // 3] = u[0, 4]                                   # repeated values
    if N > 1:
        for i, v in enumerate((np.nan, -0.5, 1.5, -0.0)):               # what the rule of the uniforms maps to 0 and 1
            u[N - 1, (Ni // 2 + i) % Ni] = v
    return z, w, u


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize("N,S,Ni", SHAPES, ids=[f"{n}x{s}+{i}" for n, s, i in SHAPES])
def test_kernel_equals_the_restatement_bit_for_bit(N, S, Ni):
    """z_out and z_fine, with u given and with u = NULL, every launch twice (the bits must repeat).  Rows cycle through the six
    weight families; a shape with fewer rows than families is launched once per remaining offset, so every shape sees all of them.
    Row 0 has repeated depths and a u row with exactly 0, nextafter(1, 0), 1.0 and repeated values; one row starts -0.0, +0.0."""
    from snerf_amd import ops
    for shift in range(0, FAMILIES, min(N, FAMILIES)):
        z, w, u = _case(N, S, Ni, shift)
        zd, wd, ud = (torch.from_numpy(a).to(DEV) for a in (z, w, u))
        for uu, ug in ((u, ud), (None, None)):
            want_out, want_fine = RN.resample_z(z, w, Ni, uu)
            for again in range(2):
                out, fine = ops.resample_z(zd, wd, Ni, ug, return_fine=True)
                assert out.shape == (N, S + Ni) and fine.shape == (N, Ni) and out.dtype == fine.dtype == torch.float32
                what = (shift, "u" if uu is not None else "det", again)
                bad = _bits(fine) != want_fine.view(np.uint32)
                assert not bad.any(), (what, "z_fine", int(bad.sum()), np.argwhere(bad)[:4].tolist())
                bad = _bits(out) != want_out.view(np.uint32)
                assert not bad.any(), (what, "z_out", int(bad.sum()), np.argwhere(bad)[:4].tolist())
            only = ops.resample_z(zd, wd, Ni, ug)                       # z_fine = NULL
            assert np.array_equal(_bits(only), want_out.view(np.uint32))


def test_no_output_depends_on_bytes_the_library_did_not_write(monkeypatch):
    """the harness of tests/test_gpu_fill.py on the entry's two outputs, z_out and z_fine (pure outputs; z, weights, u are read only): both carry the
    fill before the launch, under 0x00, 0xFF and 0x7B; the results are bit-identical, those of the restatement, and every element
    was written.  A shape with a ragged last workgroup and several elements per lane."""
    from snerf_amd import ops
    from tests.test_gpu_fill import _poison, run_filled
    N, S, Ni = 9, 130, 200
    z, w, u = _case(N, S, Ni, 0)
    zd, wd, ud = (torch.from_numpy(a).to(DEV) for a in (z, w, u))
    want_out, want_fine = RN.resample_z(z, w, Ni, u)

    def run(fill):
        _poison(monkeypatch, fill)
        out, fine = ops.resample_z(zd, wd, Ni, ud, return_fine=True)
        return {"z_out": out, "z_fine": fine}

    for fill, got in run_filled(run).items():
        assert np.array_equal(_bits(got["z_out"]), want_out.view(np.uint32)), hex(fill)
        assert np.array_equal(_bits(got["z_fine"]), want_fine.view(np.uint32)), hex(fill)
        assert bool(torch.isfinite(got["z_out"]).all()) and bool(torch.isfinite(got["z_fine"]).all())


# ---- the renderer ------------------------------------------------------------------------------------------------------------------
N_RAYS, S_COARSE, N_IMP = 77, 7, 5
S_ALL = S_COARSE + N_IMP


@pytest.fixture(scope="module")
def setup():
    """one model (fc_units = 64, feat_last = 32, default arithmetic), one batch, the renderer with n_importance = 5 and its twin
    with n_importance = 0 on the same models, and the manual chain's merged depths for given and for absent uniforms"""
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=64, n_samples=S_COARSE, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, 64, 3, n_importance=N_IMP, render_chunk_size=4096)
    assert pipe.model_coarse.spec.feat_last == 32 and pipe.model_coarse.spec.mfma == "f16x2" and pipe.cfgs.pipeline.sc_lambda > 0
    import types
    cfgs0 = types.SimpleNamespace(run=pipe.cfgs.run, pipeline=pipe.cfgs.pipeline.model_copy(update={"n_importance": 0}))
    plain = type(pipe.renderer)(cfgs0)
    b = O.batch_to_torch(O.synthetic_batch(N_RAYS, S_COARSE, seed=21))
    rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
    ui = torch.rand(N_RAYS, N_IMP, generator=torch.Generator().manual_seed(4)).to(DEV)
    prop = {"weights_coarse": torch.empty(N_RAYS, S_COARSE, device=DEV), "z_vals_coarse": torch.empty(N_RAYS, S_COARSE, device=DEV)}
    plain.render_rays_into(pipe.models, rays, extras, prop, {"perturb_rand": u})                 # the proposal pass, by today's path
    zc, wc = prop["z_vals_coarse"].cpu().numpy(), prop["weights_coarse"].cpu().numpy()
    assert float(wc.sum(1).max()) > 1e-3                                                          # the pdf is not flat everywhere
    zm = torch.from_numpy(RN.resample_z(zc, wc, N_IMP, ui.cpu().numpy())[0]).to(DEV)
    zm_det = torch.from_numpy(RN.resample_z(zc, wc, N_IMP, None)[0]).to(DEV)
    return {"pipe": pipe, "plain": plain, "semantic": b["semantic"].to(DEV), "rays": rays, "extras": extras, "u": u, "ui": ui, "zm": zm, "zm_det": zm_det}


def _into_keys(spec):
    from snerf_amd import ops
    return [k + "_coarse" for k in list(ops.output_keys(spec, False)) + ["semantic_label", "z_vals", "weights_sc", "transparency_sc", "sun_sc"]]


def _buffers(keys, spec, n=N_RAYS, S=S_ALL):
    from snerf_amd.eval.utils.util import result_buffers
    out = result_buffers([k for k in keys if k != "z_vals_coarse"], n, S, spec.n_classes, DEV)
    if "z_vals_coarse" in keys:
        out["z_vals_coarse"] = torch.empty(n, S, device=DEV)
    return out


def _assert_same(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        same = got[k].detach().contiguous().view(torch.uint8) == want[k].detach().contiguous().view(torch.uint8)
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} bytes differ")


def test_render_rays_into_equals_the_manual_chain(setup):
    """inference: every main-pass key, the label, the depths and the three solar-correction keys; per-sample results have 12 columns
    (on a build that drops n_importance the 12-column buffers are refused: the assertion that fails without the feature)"""
    s = setup
    pipe, spec = s["pipe"], s["pipe"].model_coarse.spec
    keys = _into_keys(spec)
    for name, opts, zm in (("given uniforms", {"perturb_rand": s["u"], "importance_rand": s["ui"]}, s["zm"]),
                           ("perturb = 0 around a pinned jitter: the regular grid", {"perturb_rand": s["u"], "perturb": 0}, s["zm_det"])):
        want = _buffers(keys, spec)
        s["plain"].render_rays_into(pipe.models, s["rays"], s["extras"], want, {"perturb_rand": s["u"], "given_z_vals": zm})
        got = _buffers(keys, spec)
        pipe.renderer.render_rays_into(pipe.models, s["rays"], s["extras"], got, opts)
        assert got["weights_coarse"].shape == (N_RAYS, S_ALL) and got["albedo_coarse"].shape == (N_RAYS, S_ALL, 3)
        _assert_same(got, want, name)
        assert torch.equal(got["z_vals_coarse"], zm) and bool((got["z_vals_coarse"].diff(dim=1) >= 0).all())
    # absent uniforms are drawn from torch's generator (perturb > 0): the same seed, the same picture
    a, b = _buffers(("rgb_coarse", "z_vals_coarse"), spec), _buffers(("rgb_coarse", "z_vals_coarse"), spec)
    torch.manual_seed(9)
    pipe.renderer.render_rays_into(pipe.models, s["rays"], s["extras"], a, {"perturb_rand": s["u"]})
    torch.manual_seed(9)
    pipe.renderer.render_rays_into(pipe.models, s["rays"], s["extras"], b, {"perturb_rand": s["u"]})
    _assert_same(a, b, "drawn uniforms")
    assert not torch.equal(a["z_vals_coarse"], s["zm_det"])
    # depths given: no proposal pass, the caller's depths are the pass's
    c = _buffers(("z_vals_coarse",), spec)
    pipe.renderer.render_rays_into(pipe.models, s["rays"], s["extras"], c, {"given_z_vals": s["zm_det"]})
    assert torch.equal(c["z_vals_coarse"], s["zm_det"])


def test_render_rays_under_grad_equals_the_manual_chain(setup):
    """training: every result, and after a backward from a fixed cotangent every parameter gradient and the gradient of the
    transient embedding; the merged depths carry no gradient"""
    s = setup
    pipe = s["pipe"]
    params = [p for p in pipe.parameters() if p.requires_grad]
    names = [n for n, p in pipe.named_parameters() if p.requires_grad]
    assert any("model_t" in n for n in names)

    def run(renderer, opts):
        for p in params:
            p.grad = None
        with torch.enable_grad():
            res = renderer.render_rays(pipe.models, s["rays"], s["extras"], render_options=dict(opts, return_z_vals=True))
            z = res.pop("z_vals_coarse")
            assert not z.requires_grad
            diff = [k for k in sorted(res) if res[k].requires_grad]
            g = torch.Generator().manual_seed(17)
            cots = [torch.randn(res[k].shape, generator=g).to(DEV) for k in diff]
            torch.autograd.backward([res[k] for k in diff], cots)
        torch.cuda.synchronize()
        return {k: v.detach() for k, v in res.items()}, z, diff, {n: p.grad.clone() for n, p in zip(names, params) if p.grad is not None}

    want, z_w, diff_w, g_want = run(s["plain"], {"perturb_rand": s["u"], "given_z_vals": s["zm"]})
    got, z_g, diff_g, g_got = run(pipe.renderer, {"perturb_rand": s["u"], "importance_rand": s["ui"]})
    assert torch.equal(z_g, s["zm"]) and torch.equal(z_w, s["zm"])
    assert diff_g == diff_w and {"rgb_coarse", "weights_coarse", "sun_sc_coarse"} <= set(diff_g)
    assert got["weights_coarse"].shape == (N_RAYS, S_ALL) and got["sun_sc_coarse"].shape == (N_RAYS, S_ALL, 1)
    _assert_same(got, want, "render_rays")
    assert set(g_got) == set(g_want) and len(g_got) >= len(pipe.model_coarse.spec.param_names()) + 1
    _assert_same(g_got, g_want, "gradients")
    assert float(g_got["model_t.weight"].abs().max()) > 0


def test_relight_after_a_resampled_base_pass(setup):
    """a relight on the workspace of a resampled base pass equals a full pass on the merged depths under the new sun"""
    from snerf_amd import ops
    s = setup
    pipe, spec = s["pipe"], s["pipe"].model_coarse.spec
    keys = [k + "_coarse" for k in list(ops.output_keys(spec, False)) + ["semantic_label", "z_vals"]]
    sun_b = torch.nn.functional.normalize(s["extras"][:, :3] + torch.tensor([0.3, -0.2, 0.1], device=DEV), dim=1)
    extras_b = s["extras"].clone()
    extras_b[:, :3] = sun_b
    base = _buffers(keys, spec)
    ws = pipe.renderer.render_rays_into(pipe.models, s["rays"], s["extras"], base,
                                        {"perturb_rand": s["u"], "importance_rand": s["ui"], "workspace": None})
    got = _buffers(keys, spec)
    assert pipe.renderer.relight_rays_into(pipe.models, extras_b, got, {"workspace": ws}) is ws
    want = _buffers(keys, spec)
    s["plain"].render_rays_into(pipe.models, s["rays"], extras_b, want, {"given_z_vals": s["zm"]})
    _assert_same(got, want, "relight")
    assert torch.equal(got["z_vals_coarse"], s["zm"]) and not torch.equal(got["rgb_coarse"], base["rgb_coarse"])


def test_lean_inference_over_ragged_chunks(setup):
    """three ragged chunks (30, 30, 17 rays) against one chunk, with a per-sample result (weights, beta) among the keys: the
    frame-sized buffers have S + Ni columns and the frame's uniforms are sliced with its rays; the semantic evaluator's
    chunk-sized buffers take the same width"""
    from snerf_amd.eval.utils.semantic import lean_semantic_eval
    from snerf_amd.eval.utils.util import lean_inference
    s = setup
    pipe = s["pipe"]
    keys = ("rgb_coarse", "depth_coarse", "weights_coarse", "beta_coarse")
    opts = {"perturb_rand": s["u"], "importance_rand": s["ui"]}
    keep = pipe.cfgs.pipeline.render_chunk_size
    try:
        one = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, s["rays"], s["extras"], keys=keys, render_options=opts)
        pipe.cfgs.pipeline.render_chunk_size = 30
        three = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, s["rays"], s["extras"], keys=keys, render_options=opts)
        ev = lean_semantic_eval(pipe.cfgs, pipe.renderer, pipe.models, s["rays"], s["extras"], s["semantic"], render_options=opts)
    finally:
        pipe.cfgs.pipeline.render_chunk_size = keep
    assert one["weights_coarse"].shape == (N_RAYS, S_ALL) and one["beta_coarse"].shape == (N_RAYS, S_ALL, 1)
    _assert_same(three, one, "three chunks vs one")
    want = _buffers(keys, pipe.model_coarse.spec)
    s["plain"].render_rays_into(pipe.models, s["rays"], s["extras"], want, {"given_z_vals": s["zm"]})
    _assert_same(one, want, "lean_inference vs the manual chain")
    assert ev.image_entry() is not None


def test_n_importance_zero_is_todays_path(setup):
    """a renderer built with n_importance = 0 renders what the same call gives with no such key at all"""
    import types
    s = setup
    pipe, spec = s["pipe"], s["pipe"].model_coarse.spec
    pc = {k: v for k, v in pipe.cfgs.pipeline.model_dump().items() if k != "n_importance"}
    bare = type(pipe.renderer)(types.SimpleNamespace(pipeline=types.SimpleNamespace(**pc), run=pipe.cfgs.run))   # a config without the key
    assert (s["plain"].N_importance, s["plain"].n_render_samples, bare.N_importance) == (0, S_COARSE, 0)
    keys = _into_keys(spec)
    a, b = _buffers(keys, spec, S=S_COARSE), _buffers(keys, spec, S=S_COARSE)
    s["plain"].render_rays_into(pipe.models, s["rays"], s["extras"], a, {"perturb_rand": s["u"]})
    bare.render_rays_into(pipe.models, s["rays"], s["extras"], b, {"perturb_rand": s["u"]})
    _assert_same(a, b, "n_importance = 0")
    # ... and the library's pass on the stratified depths, called directly
    from snerf_amd import ops
    from snerf_amd.semantic.components.rendering import _pass_operands
    from snerf_amd.framework.components.rendering import z_steps_on
    sun_d, rt, rts, params, packed = _pass_operands(pipe.models, pipe.model_coarse, s["extras"], {})
    direct = {k: torch.empty_like(a[k + "_coarse"]) for k in ("rgb", "weights", "z_vals")}
    ops.render_pass_into(spec, params, ops.PassInputs(sun_d=sun_d, rays=s["rays"], z_steps=z_steps_on(s["rays"].device, S_COARSE), u=s["u"]),
                         rt, rts, direct, packed=packed)
    for k, v in direct.items():
        assert torch.equal(v, a[k + "_coarse"]), k


def test_training_step_runs_on_the_resampled_depths(setup):
    """the pipeline's own training step (renderer, losses, backward) with n_importance = 5: the jitter and the uniforms come from
    torch's generator, so a seed fixes the loss; the loss and every gradient are finite; the losses read 12-column results"""
    from tests.test_gpu_pipeline import _batch_to_dev
    s = setup
    pipe = s["pipe"]
    batch = _batch_to_dev(O.batch_to_torch(O.synthetic_batch(N_RAYS, S_COARSE, seed=21)))
    pipe.current_epoch = 0
    losses = []
    for _ in range(2):
        for p in pipe.parameters():
            p.grad = None
        torch.manual_seed(3)
        out = pipe.training_step(batch, 0)
        out["loss"].backward()
        torch.cuda.synchronize()
        losses.append(float(out["loss"].detach()))
        grads = [p.grad for p in pipe.parameters() if p.grad is not None]
        assert len(grads) >= len(pipe.model_coarse.spec.param_names()) + 1
        assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert losses[0] == losses[1] and np.isfinite(losses[0])
    for p in pipe.parameters():
        p.grad = None
