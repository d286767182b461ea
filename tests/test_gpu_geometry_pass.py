"""The geometry pass (SNERF_FLAG_GEOMETRY, ops.geometry_pass_into) on the device (run with -m gpu on an MI355X).

(tests/test_gpu_geometry.py is an older file about TRUNK geometries -- depth, skips, encoding width; this one is about the pass kind.)

The bar is BIT EQUALITY with the plain inference pass of the same descriptor and inputs: the geometry pass runs that pass's own
leading launches (depths, encoding, trunk, sigma) and the composite kernel's geometry instantiation of the same body, so depth,
weights, transparency, sigmas and z_vals must carry the same bits -- a differing bit is a defect, not a tolerance question.  Against
the reference's own outputs the bar is the suite's OUT_TOL (tests/test_gpu_kernels.py; tests/helpers.py holds the fixtures and the
error measures, no tolerance of its own).

Shapes: N = 130 rays (no row count below is a multiple of the 128-row block) x S in {3, 64, 65, 130}: a partial wave, exactly one
chunk of 64, a carried transmittance into a one-lane chunk, three chunks.  Networks: SIREN at W = 256 and W = 512 (sigma folded into
the last trunk layer's epilogue: Plan::nd_sig) and at W = 64 / 32 (sigma's 32-wide launch; Wf = 128 > W; W = 32 is not composed),
ReLU at W = 64 with a skip layer, SatNeRF (raw xyz).  Both arithmetic modes; the one-plane mode at W = 512 with the one-launch trunk
on and off, and at L = 3, where only the full pass can fuse its trunk."""
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import load_fixture, fixture_params, max_abs
from tests.test_gpu_kernels import _gpu_params, _spec, OUT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 130
GEO = ("depth", "weights", "transparency", "sigmas", "z_vals")

NETS = {
    "siren256": dict(fc_units=256),                                                     # nd_sig on; skip at 4; composed in two planes
    "siren64": dict(fc_units=64, fc_layers=3, fc_skips=(1,)),                           # nd_sig off: sigma's 32-wide launch; Wf = 128 > W
    "relu64": dict(fc_units=64, activation_function="relu"),                            # ReLU, 8 layers, skip at 4, Wf > W
    "siren32": dict(fc_units=32),                                                       # feat_last = 16: not composed (two planes only)
    "satnerf64": dict(model="satnerf", fc_units=64),                                    # raw xyz: the encode kernel's own block maximum
    "siren512": dict(fc_units=512),                                                     # the headline width: the fused trunk in one plane
    "siren512-L3": dict(fc_units=512, fc_layers=3, fc_skips=()),                        # one plane: the full pass fuses its trunk (with the
    #                                                                                     feats entry), the geometry pass cannot (L = 3
    #                                                                                     without it) and runs layer per launch
}
WIDE = ("siren512", "siren512-L3")
CASES = [(n, s, "f16x2") for n in NETS if n not in WIDE for s in (3, 64, 65, 130)]
CASES += [(n, s, "f16x1") for n in ("siren256", "siren64", "relu64") for s in (3, 64, 65, 130)]
CASES += [("siren512", 64, m) for m in ("f16x2", "f16x1-fused", "f16x1-perlayer")] + [("siren512-L3", 64, "f16x1-fused")]


def _id(c):
    return f"{c[0]}-S{c[1]}-{c[2]}"


class _Mode:
    """arithmetic (ops.BASE_FLAGS) and trunk fusion of one case, restored on exit"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from snerf_amd import ops, _lib
        self.keep = ops.BASE_FLAGS
        ops.BASE_FLAGS = 0 if self.mode == "f16x2" else _lib.FLAG_F16X1
        _lib.lib().snerf_test_set_trunk_fusion(0 if self.mode.endswith("perlayer") else 1)

    def __exit__(self, *exc):
        from snerf_amd import ops, _lib
        ops.BASE_FLAGS = self.keep
        _lib.lib().snerf_test_set_trunk_fusion(1)
        return False


_SETUP = {}


def _setup(net, S):
    """model, packed-independent inputs of the three seams; computed once per (net, S)"""
    if (net, S) not in _SETUP:
        cfg = O.OracleCfg(n_samples=S, **NETS[net])
        spec = _spec(cfg)
        gp = _gpu_params(O.init_params_numpy(cfg, 7), DEV)
        b = O.batch_to_torch(O.synthetic_batch(N, S, seed=31 + S))
        rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
        emb = torch.from_numpy(O.init_embedding_numpy(cfg, 7)).to(DEV)
        t = emb[extras[:, 3].long()].contiguous()
        zs = torch.linspace(0, 1, S).to(DEV)
        g = torch.Generator().manual_seed(5 + S)
        near, far = b["rays"][:, 6:7], b["rays"][:, 7:8]
        z_given = (near + (far - near) * torch.sort(torch.rand(N, S, generator=g), dim=1).values).float().to(DEV).contiguous()
        xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z_given[:, :, None]).contiguous()
        _SETUP[(net, S)] = dict(cfg=cfg, spec=spec, gp=gp, rays=rays, sun=extras[:, :3], t=t, zs=zs, u=u, z_given=z_given, xyz=xyz)
    return _SETUP[(net, S)]


def _pins(s, with_sun):
    from snerf_amd import ops
    sun = s["sun"] if with_sun else None
    return {"sampled": ops.PassInputs(sun_d=sun, rays=s["rays"], z_steps=s["zs"], u=s["u"]),
            "given_z": ops.PassInputs(sun_d=sun, rays=s["rays"], z_vals=s["z_given"]),
            "xyz": ops.PassInputs(sun_d=sun, xyz=s["xyz"], z_vals=s["z_given"])}


def _out(S, keys=GEO, fill=None):
    o = {}
    for k in keys:
        shape = (N,) if k == "depth" else ((N, 3) if k == "rgb" else (N, S))
        o[k] = torch.empty(shape, device=DEV)
        if fill is not None:
            o[k].view(torch.uint8).fill_(fill)
    return o


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    for k in GEO:
        same = _bits(got[k]) == _bits(want[k])
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} elements differ")


_FULL = {}


def _full_pass(net, S, mode, seam):
    """the plain inference pass, asked for rgb as well (an ordinary pass); cached: the reference every test shares"""
    from snerf_amd import ops
    key = (net, S, mode, seam)
    if key not in _FULL:
        s = _setup(net, S)
        with _Mode(mode):
            packed = ops.pack_params(s["spec"], s["gp"])
            out = _out(S, GEO + ("rgb",))
            ops.render_pass_into(s["spec"], s["gp"], _pins(s, True)[seam], s["t"], None, out, packed=packed)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), key
        assert float(out["weights"].sum()) > 0
        _FULL[key] = out
    return _FULL[key]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_geometry_pass_has_the_bits_of_the_full_pass(case):
    """the three seams -- sampled depths with jitter, given z_vals, explicit xyz -- with sun_d / t handed over (and ignored) and with
    all three NULL; every geometry call on a workspace of exactly snerf_workspace_bytes(geometry), which is smaller than the full
    pass's.  Fails on a library without the flag: the descriptor's unknown bit changes nothing there and out->rgb = NULL would be
    the only difference -- the size assertion and ops.geometry_pass_into do not exist."""
    from snerf_amd import ops, _lib
    net, S, mode = case
    s = _setup(net, S)
    with _Mode(mode):
        fl = ops.BASE_FLAGS
        d_full, d_geo = s["spec"].desc(N, S), s["spec"].desc(N, S, _lib.FLAG_GEOMETRY)
        assert d_geo.flags == (fl | _lib.FLAG_GEOMETRY)
        n_full, n_geo = (_lib.call_size("snerf_workspace_bytes", d) for d in (d_full, d_geo))
        assert 0 < n_geo < n_full
    for seam in ("sampled", "given_z", "xyz"):
        want = _full_pass(net, S, mode, seam)
        with _Mode(mode):
            packed = ops.pack_params(s["spec"], s["gp"])
            ws = torch.empty(n_geo, dtype=torch.uint8, device=DEV)
            got = _out(S)
            back = ops.render_pass_into(s["spec"], s["gp"], _pins(s, True)[seam], s["t"], None, got, packed=packed, workspace=ws, geometry=True)
            assert back is ws
            _assert_bits(got, want, (seam, "sun_d and t given"))
            got = _out(S)
            assert ops.geometry_pass_into(s["spec"], s["gp"], _pins(s, False)[seam], got, packed=packed, workspace=ws) is ws
            _assert_bits(got, want, (seam, "sun_d, t, t_s NULL"))
            one = {"depth": torch.empty(N, device=DEV)}      # a single result: every other pointer NULL
            ops.geometry_pass_into(s["spec"], s["gp"], _pins(s, False)[seam], one, packed=packed)
            assert torch.equal(_bits(one["depth"]), _bits(want["depth"]))
    if S > 1:
        assert torch.equal(_full_pass(net, S, mode, "given_z")["z_vals"], s["z_given"])


@pytest.mark.parametrize("name", ["inference_sem_small", "inference_satnerf_small"])
def test_geometry_pass_against_the_references_outputs(name):
    """the reference's inference() outputs on explicit xyz (the fixtures of test_gpu_kernels.test_inference_seam_explicit_xyz), at
    that test's bar for the same keys"""
    from snerf_amd import ops
    z, meta, cfg = load_fixture(name)
    gp = _gpu_params(fixture_params(z, meta, cfg), DEV)
    xyz, zv = torch.from_numpy(z["in_xyz"]).to(DEV), torch.from_numpy(z["in_z"]).to(DEV)
    n, S = zv.shape
    keys = [k for k in ("depth", "weights", "transparency", "sigmas") if "out_" + k in z.files]
    assert {"depth", "weights"} <= set(keys)
    out = {k: torch.empty(z["out_" + k].shape, device=DEV) for k in keys}
    ops.geometry_pass_into(_spec(cfg), gp, ops.PassInputs(xyz=xyz, z_vals=zv), out)
    for k in keys:
        err = max_abs(out[k].cpu(), z["out_" + k])
        print(f"{name}: {k} max abs err {err:.3e}")
        assert err <= OUT_TOL, (name, k, err)


FILL_CASES = [("siren256", 65, "f16x2"), ("relu64", 130, "f16x2"), ("relu64", 3, "f16x1"), ("siren32", 64, "f16x2"),
              ("siren512", 64, "f16x2"), ("siren512", 64, "f16x1-fused"), ("siren512", 64, "f16x1-perlayer")]


@pytest.mark.parametrize("case", FILL_CASES, ids=_id)
def test_no_result_depends_on_bytes_the_pass_did_not_write(case, monkeypatch):
    """the harness of tests/test_gpu_fill.py: workspace and outputs carry 0x00 / 0xFF / 0x7B before the call.  (i) the workspace the
    library's Python side makes for a geometry descriptor; (ii) a larger workspace that a FULL pass of another shape wrote last --
    what a chunk walk hands on.  Bit-identical under every fill, every element written, and the bits of the full pass."""
    from snerf_amd import ops, _lib
    from tests.test_gpu_fill import _poison, run_filled
    net, S, mode = case
    s = _setup(net, S)
    want = _full_pass(net, S, mode, "sampled")
    other = _setup(net, 33)      # another shape: 130 x 33

    def run(fill):
        _poison(monkeypatch, fill)
        with _Mode(mode):
            packed = ops.pack_params(s["spec"], s["gp"])
            a = _out(S, fill=fill)
            ws = ops.geometry_pass_into(s["spec"], s["gp"], _pins(s, False)["sampled"], a, packed=packed)
            assert ws.numel() == _lib.call_size("snerf_workspace_bytes", s["spec"].desc(N, S, _lib.FLAG_GEOMETRY))
            big = torch.empty(2 * _lib.call_size("snerf_workspace_bytes", s["spec"].desc(N, max(S, 33))), dtype=torch.uint8, device=DEV)
            big.fill_(fill)
            ops.render_pass_into(other["spec"], other["gp"], _pins(other, True)["sampled"], other["t"], None, _out(33, GEO + ("rgb",)),
                                 packed=packed, workspace=big)
            b = _out(S, fill=fill)
            assert ops.geometry_pass_into(s["spec"], s["gp"], _pins(s, False)["sampled"], b, packed=packed, workspace=big) is big
        res = {"own_" + k: v for k, v in a.items()}
        res.update({"big_" + k: v for k, v in b.items()})
        return res

    r = run_filled(run)[0xFF]
    assert all(bool(torch.isfinite(v).all()) for v in r.values())
    for pre in ("own_", "big_"):
        _assert_bits({k: r[pre + k] for k in GEO}, want, pre)


def test_a_relight_on_a_geometry_workspace_is_refused():
    from snerf_amd import ops
    s = _setup("siren64", 64)
    packed = ops.pack_params(s["spec"], s["gp"])
    full_bytes = ops._lib.call_size("snerf_workspace_bytes", s["spec"].desc(N, 64))
    ws = torch.empty(full_bytes, dtype=torch.uint8, device=DEV)
    ops.geometry_pass_into(s["spec"], s["gp"], _pins(s, False)["sampled"], _out(64), packed=packed, workspace=ws)
    with pytest.raises(RuntimeError, match=r"last pass was a geometry \(SNERF_FLAG_GEOMETRY\) pass"):
        ops.relight_pass_into(s["spec"], s["gp"], s["sun"], s["t"], None, {"rgb": torch.empty(N, 3, device=DEV)}, ws, packed=packed, n_samples=64)
    # a full pass on the same workspace makes it relightable again
    ops.render_pass_into(s["spec"], s["gp"], _pins(s, True)["sampled"], s["t"], None, _out(64), packed=packed, workspace=ws)
    ops.relight_pass_into(s["spec"], s["gp"], s["sun"], s["t"], None, {"rgb": torch.empty(N, 3, device=DEV)}, ws, packed=packed, n_samples=64)
    torch.cuda.synchronize()


# ---- the renderers ---------------------------------------------------------------------------------------------------------------
def _same_bytes(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        same = got[k].detach().contiguous().view(torch.uint8) == want[k].detach().contiguous().view(torch.uint8)
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} bytes differ")


@pytest.mark.parametrize("n,S,Ni", [(16, 7, 5), (64, 64, 64)], ids=("16x7+5", "64x64+64"))
def test_resampled_render_with_a_geometry_proposal(n, S, Ni, monkeypatch):
    """render_rays, render_rays_into and one training step with n_importance > 0: the default (geometry) proposal against
    proposal_pass = "full", pinned jitter and uniforms; every result key, the loss, every parameter gradient and the embedding's, bit
    for bit.  The geometry proposal launches no embedding lookup and sets the flag (both spied on)."""
    from snerf_amd import ops
    from snerf_amd.eval.utils.util import result_buffers
    from snerf_amd.semantic.components import rendering as R
    from tests.test_gpu_pipeline import _pipeline_for, _batch_to_dev
    cfg = O.OracleCfg(fc_units=64, n_samples=S, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, n, 3, n_importance=Ni, render_chunk_size=4096)
    spec = pipe.model_coarse.spec
    b = O.batch_to_torch(O.synthetic_batch(n, S, seed=21))
    rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
    ui = torch.rand(n, Ni, generator=torch.Generator().manual_seed(4)).to(DEV)
    pinned = {"perturb_rand": u, "importance_rand": ui}
    seen = {"lookups": 0, "geometry": []}
    keep_rows, keep_into = R.transient_rows, ops.render_pass_into

    def rows(*a, **k):
        seen["lookups"] += 1
        return keep_rows(*a, **k)

    def into(*a, **k):
        seen["geometry"].append(bool(k.get("geometry")))
        return keep_into(*a, **k)

    monkeypatch.setattr(R, "transient_rows", rows)
    monkeypatch.setattr(ops, "render_pass_into", into)
    with torch.no_grad():
        geo = pipe.renderer.render_rays(pipe.models, rays, extras, render_options=dict(pinned, return_z_vals=True))
        n_geo, flags_geo = seen["lookups"], list(seen["geometry"])
        seen.update(lookups=0, geometry=[])
        full = pipe.renderer.render_rays(pipe.models, rays, extras, render_options=dict(pinned, return_z_vals=True, proposal_pass="full"))
    assert flags_geo == [True] and seen["geometry"] == [False]      # the proposal is the one *_into call of a render_rays
    assert seen["lookups"] == 2 * n_geo > 0                          # the full proposal looks the rows up once more
    assert geo["weights_coarse"].shape == (n, S + Ni) and "sun_sc_coarse" in geo
    _same_bytes(geo, full, "render_rays")
    keys = [k + "_coarse" for k in list(ops.output_keys(spec, False)) + ["semantic_label", "weights_sc", "transparency_sc", "sun_sc"]]
    got, want = (result_buffers(keys, n, S + Ni, spec.n_classes, DEV) for _ in range(2))
    for o in (got, want):
        o["z_vals_coarse"] = torch.empty(n, S + Ni, device=DEV)
    pipe.renderer.render_rays_into(pipe.models, rays, extras, got, pinned)
    pipe.renderer.render_rays_into(pipe.models, rays, extras, want, dict(pinned, proposal_pass="full"))
    _same_bytes(got, want, "render_rays_into")
    assert torch.equal(got["z_vals_coarse"], geo["z_vals_coarse"])
    # one training step, the jitter and the uniforms from torch's generator under one seed
    batch = _batch_to_dev(O.batch_to_torch(O.synthetic_batch(n, S, seed=22)))
    pipe.current_epoch = 0
    keep_render = pipe.renderer.render_rays

    def step(proposal):
        def render(*a, **k):
            k["render_options"] = dict(k.get("render_options") or {}, proposal_pass=proposal)
            return keep_render(*a, **k)
        monkeypatch.setattr(pipe.renderer, "render_rays", render)
        for p in pipe.parameters():
            p.grad = None
        torch.manual_seed(3)
        out = pipe.training_step(batch, 0)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in pipe.named_parameters() if p.grad is not None}
        return out["loss"].detach().clone(), grads

    seen.update(lookups=0, geometry=[])
    loss_g, grads_g = step("geometry")
    assert seen["geometry"] == [True]
    loss_f, grads_f = step("full")
    assert bool(torch.isfinite(loss_g)) and torch.equal(loss_g.view(torch.int32), loss_f.view(torch.int32))
    assert len(grads_g) >= len(spec.param_names()) + 1 and float(grads_g["model_t.weight"].abs().max()) > 0
    _same_bytes(grads_g, grads_f, "gradients")


def test_walks_pick_the_geometry_pass_and_keep_the_bits(monkeypatch):
    """lean_inference for the depth alone, extract_pointcloud without colours, and a two-sun sweep asked for the depth alone
    (which must NOT take the geometry pass: its base pass is relit); 300 rays in chunks of 128"""
    from snerf_amd import ops
    from snerf_amd.eval.extract_pointcloud import extract_pointcloud
    from snerf_amd.eval.utils.util import lean_inference, lean_relight
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=64, n_samples=24, render_chunk_size=128)
    pipe, _ = _pipeline_for(cfg, 64, 5)
    b = O.batch_to_torch(O.synthetic_batch(300, 24, seed=15))
    rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
    ro = {"perturb_rand": u}
    seen = []
    keep = ops.render_pass_into

    def into(*a, **k):
        seen.append(bool(k.get("geometry")))
        return keep(*a, **k)

    monkeypatch.setattr(ops, "render_pass_into", into)
    three = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro)
    assert seen == [False] * 3
    seen.clear()
    one = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=("depth_coarse",), render_options=ro)
    assert seen == [True] * 3 and set(one) == {"depth_coarse"}
    assert torch.equal(_bits(one["depth_coarse"]), _bits(three["depth_coarse"])) and float(one["depth_coarse"].abs().sum()) > 0
    seen.clear()
    cloud = extract_pointcloud(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro)
    bare = extract_pointcloud(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro, with_colors=False, with_labels=False)
    assert seen == [False] * 3 + [True] * 3
    assert "colors" in cloud and "colors" not in bare and "labels" not in bare
    assert torch.equal(bare["xyz_n"].view(torch.int64), cloud["xyz_n"].view(torch.int64))
    assert torch.equal(_bits(bare["depth"]), _bits(three["depth_coarse"]))
    seen.clear()
    sweep = lean_relight(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, [(60.0, 120.0), (35.0, 200.0)], keys=("depth_coarse",), render_options=ro)
    torch.cuda.synchronize()
    assert seen == [False] * 3      # three relightable base passes (the relights go through relight_pass_into)
    assert sweep["depth_coarse"].shape == (2, 300)
    for k in range(2):              # the depth does not depend on the sun
        assert torch.equal(_bits(sweep["depth_coarse"][k]), _bits(three["depth_coarse"]))
