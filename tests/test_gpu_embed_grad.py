"""The embedding-only backward (SNERF_FLAG_EMBED_GRAD), the vector override of the renderers and the embedding fit (-m gpu).

| check | what |
|---|---|
| 1 test_equals_the_full_backward | d_t / d_t_s of the flagged backward, torch.equal with the full backward's, on two identical forwards; packed_grads a sentinel buffer that comes back untouched, then NULL |
| 2 test_solar_correction_pass | zeros, sentinel untouched, no launch in any profiled variant |
| 3 test_launch_structure | no trunk / wide dW launch, at most 3 K-contiguous + 32-wide launches, fewer than the full backward |
| 4 test_fills | bit-identical and finite under the fills 0x00 / 0xFF / 0x7B |
| 5 test_autograd_* | frozen parameters take the flagged path through ops._RenderPass; parameters that need gradients do not |
| 6 test_vector_override_* | render_options["t_vector"] = row r has the bits of ts = r; its gradient is the row's |
| 7 test_fit_follows_the_fp64_oracle | 30 Adam steps against the same optimisation of oracle.render_rays in fp64 |
| 8 test_evaluation_on_the_fixture_scene | eval_nerf_images / eval_semantic_images with fit_embedding on tests/golden/scene_small |

Shapes of check 1: 37 x 24 (one composite chunk), 5 x 130 (S walks three 64-lane chunks), 130 x 8 (P = 1040 crosses 128-row tiles),
each at W = 64, and 37 x 24 at W = 512 (the folded final layers).  Modes: the default arithmetic with the composed and with the
separate first head layer, and one plane (which never composes).  Variants: VARIANTS of test_gpu_cotangents, the default model and
"tj" (use_tj_instead_of_beta + use_tj_for_s: the rgb and semantic blocks read t too, so the narrow launch contracts three blocks).
SatNeRF x one plane is no case: the plan refuses raw xyz under SNERF_FLAG_F16X1 (tests/test_abi_cpu.py).
"""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import test_gpu_cotangents as CT
from tests.test_gpu_cotangents import _inputs, _hip_backward, VARIANTS, TABLES
from tests.test_gpu_compose import SWITCH
from tests.test_gpu_fill import run_filled, _poison
from tests.test_gpu_kernels import _dev, _gpu_params, _spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scene_small")
SENTINEL = 1234.5
EMBED = 16          # _lib.FLAG_EMBED_GRAD

ALL_VARIANTS = dict(VARIANTS, default={}, tj=dict(use_tj_instead_of_beta=True, use_tj_for_s=True))
SHAPES = [(37, 24, 64), (5, 130, 64), (130, 8, 64), (37, 24, 512)]
MODES = {"composed": ("f16x2", None), "separate": ("f16x2", "0"), "one-plane": ("f16x1", None)}
_INPUTS = {}      # (variant, N, S, W) -> _inputs(...): computed once, never edited


def _case_inputs(variant, N, S, W):
    key = (variant, N, S, W)
    if key not in _INPUTS:
        cfg = O.OracleCfg(fc_units=W, n_samples=S, **ALL_VARIANTS[variant])
        _INPUTS[key] = (cfg, _inputs(cfg, N, seed=91))
    return _INPUTS[key]


def _mode(monkeypatch, mode):
    arith, setting = MODES[mode]
    CT._default_mode(monkeypatch, arith)
    if setting is not None:
        monkeypatch.setenv(SWITCH, setting)


class _Pass:
    """one pass of a model through the C-ABI itself: forward(), backward(full or flagged, any packed_grads)"""

    def __init__(self, cfg, inputs, sc=False):
        from snerf_amd import ops
        pn, emb_np, emb_s_np, b = inputs
        dev = _dev()
        self.spec, self.sc = _spec(cfg), sc
        self.packed = ops.pack_params(self.spec, _gpu_params(pn, dev))
        rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
        ts = extras[:, 3].long()
        self.t = torch.from_numpy(emb_np).to(dev)[ts].contiguous()
        self.t_s = torch.from_numpy(emb_s_np).to(dev)[ts].contiguous() if emb_s_np is not None else None
        self.N, self.S = rays.shape[0], cfg.n_samples
        z = ops.sample_z(rays, torch.linspace(0, 1, self.S).to(dev), u)
        self.pin = ops.PassInputs(sun_d=extras[:, :3], rays=rays, z_vals=z)
        self.keys = ops.output_keys(self.spec, sc)

    def desc(self, extra=0):
        from snerf_amd import _lib
        return self.spec.desc(self.N, self.S, _lib.FLAG_TRAIN | (_lib.FLAG_SC_PASS if self.sc else 0) | extra)

    def forward(self, extra=0):
        from snerf_amd import _lib, ops
        d = self.desc(extra)
        ws = ops._empty(_lib.call_size("snerf_workspace_bytes", d), dtype=torch.uint8, device=self.t.device)
        outs = {k: ops._empty(ops._OUT_SHAPES[k](self.N, self.S, self.spec.n_classes), dtype=torch.float32, device=self.t.device) for k in self.keys}
        so = _lib.SnerfOutputs()
        for k, v in outs.items():
            setattr(so, k, v.data_ptr())
        _lib.call("snerf_forward", d, self.packed, self.pin.struct(self.t, self.t_s), so, ws, ws.numel())
        return ws, outs

    def cotangents(self, keys):
        name = (lambda k: k + "_sc_coarse") if self.sc else (lambda k: k + "_coarse")
        return {k: CT._cotangent(name(k), CT_SHAPE(self, k)).to(self.t.device) for k in keys}

    def backward(self, ws, g, flagged, pg):
        from snerf_amd import _lib, ops
        go = _lib.SnerfOutGrads()
        for k, v in g.items():
            setattr(go, k, v.data_ptr())
        d_t = ops._empty(tuple(self.t.shape), dtype=torch.float32, device=self.t.device)
        d_ts = ops._empty(tuple(self.t_s.shape), dtype=torch.float32, device=self.t.device) if self.t_s is not None else None
        _lib.call("snerf_backward", self.desc(_lib.FLAG_EMBED_GRAD if flagged else 0), self.packed, self.pin.struct(self.t, self.t_s),
                  go, pg, d_t, d_ts, ws, ws.numel())
        return d_t, d_ts

    def grad_buffer(self, value):
        from snerf_amd import _lib
        return torch.full((_lib.call_size("snerf_grad_floats", self.desc()),), value, dtype=torch.float32, device=self.t.device)


def CT_SHAPE(p, k):
    from snerf_amd import ops
    return ops._OUT_SHAPES[k](p.N, p.S, p.spec.n_classes)


def _profiled(fn):
    from snerf_amd import _lib
    lib = _lib.lib()
    _lib.check(lib.snerf_profile_begin(), "snerf_profile_begin")
    try:
        out = fn()
    finally:
        prof = _lib.SnerfProfile()
        _lib.check(lib.snerf_profile_end(C.byref(prof)), "snerf_profile_end")
    return out, [int(prof.launches[i]) for i in range(4)]


def _cotangent_sets(p):
    sets = {"rgb": ["rgb"], "loss-set": [k for k in ("rgb", "beta", "semantic_logits") if k in p.keys], "every-key": list(p.keys),
            "depth": ["depth"]}
    return sets


def _same_pair(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# ---- 1. equality with the full backward --------------------------------------------------------------------------------------------
CASES = [(v, n, s, w, m) for v in ALL_VARIANTS for (n, s, w) in SHAPES for m in MODES if not (v == "satnerf" and m == "one-plane")]


@pytest.mark.parametrize("variant,N,S,W,mode", CASES, ids=[f"{v}-{n}x{s}-W{w}-{m}" for v, n, s, w, m in CASES])
def test_equals_the_full_backward(variant, N, S, W, mode, monkeypatch):
    _mode(monkeypatch, mode)
    cfg, inputs = _case_inputs(variant, N, S, W)
    p = _Pass(cfg, inputs)
    assert (p.t_s is not None) == (variant == "t_s")
    for name, keys in _cotangent_sets(p).items():
        g = p.cotangents(keys)
        ws, outs = p.forward()
        full = p.backward(ws, g, False, p.grad_buffer(0.0))
        # a second, identical forward -- with the bit set: same results, same bits
        ws, outs2 = p.forward(extra=EMBED)
        assert all(torch.equal(outs[k], outs2[k]) for k in outs), (name, "the flagged forward differs")
        pg = p.grad_buffer(SENTINEL)
        got = p.backward(ws, g, True, pg)
        assert bool((pg == SENTINEL).all()), (name, "packed_grads was written")
        ws, _ = p.forward()              # a plain TRAIN forward, the bit at backward time only, and no gradient buffer at all
        null = p.backward(ws, g, True, None)
        for what, (a, b, c) in {"d_t": (full[0], got[0], null[0]), "d_t_s": (full[1], got[1], null[1])}.items():
            assert _same_pair(a, b) and _same_pair(a, c), (name, what, "differs from the full backward")
            if a is not None:
                assert bool(torch.isfinite(a).all()), (name, what)
                if name == "depth":      # the depth reads the density alone
                    assert float(a.abs().max()) == 0.0 and float(b.abs().max()) == 0.0, (name, what)
        if name == "every-key":
            assert float(full[0].abs().max()) > 0.0      # not vacuous: gradient reaches t
            if full[1] is not None:
                assert float(full[1].abs().max()) > 0.0


# ---- 2. the solar-correction pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,mode", [("default", "composed"), ("default", "separate"), ("t_s", "one-plane")])
def test_solar_correction_pass(variant, mode, monkeypatch):
    _mode(monkeypatch, mode)
    cfg, inputs = _case_inputs(variant, 37, 24, 64)
    p = _Pass(cfg, inputs, sc=True)
    g = p.cotangents(["weights", "transparency", "sun"])
    ws, _ = p.forward()
    pg = p.grad_buffer(SENTINEL)
    (d_t, d_ts), launches = _profiled(lambda: p.backward(ws, g, True, pg))
    assert launches == [0, 0, 0, 0], launches
    assert bool((pg == SENTINEL).all())
    assert float(d_t.abs().max()) == 0.0 and bool(torch.isfinite(d_t).all())
    if variant == "t_s":
        assert float(d_ts.abs().max()) == 0.0
    ws, _ = p.forward()
    d_t2, _ = p.backward(ws, g, True, None)
    assert float(d_t2.abs().max()) == 0.0


# ---- 3. launch structure of the main pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,mode", [(512, "composed"), (512, "separate"), (512, "one-plane"), (64, "composed")])
def test_launch_structure(W, mode, monkeypatch):
    _mode(monkeypatch, mode)
    cfg, inputs = _case_inputs("default", 37, 24, W)
    p = _Pass(cfg, inputs)
    g = p.cotangents(list(p.keys))
    ws, _ = p.forward()
    _, full = _profiled(lambda: p.backward(ws, g, False, p.grad_buffer(0.0)))
    ws, _ = p.forward()
    _, flagged = _profiled(lambda: p.backward(ws, g, True, None))
    print("launches per variant, full / flagged:", full, flagged)
    assert flagged[1] == 0 and flagged[2] == 0, flagged             # no trunk launch, no wide dW
    assert 1 <= flagged[0] + flagged[3] <= 3, flagged                 # the dX launch and the narrow launch into d extras
    assert flagged[0] + flagged[3] < full[0] + full[3], (flagged, full)
    assert full[2] > 0


# ---- 4. fills ------------------------------------------------------------------------------------------------------------------------
def test_fills(monkeypatch):
    _mode(monkeypatch, "composed")
    cfg, inputs = _case_inputs("t_s", 37, 24, 64)

    def run(fill):
        _poison(monkeypatch, fill)
        p = _Pass(cfg, inputs)
        ws, _ = p.forward()
        d_t, d_ts = p.backward(ws, p.cotangents(list(p.keys)), True, None)
        return {"d_t": d_t, "d_t_s": d_ts}

    r = run_filled(run)[0xFF]
    for k, v in r.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0.0, k


# ---- 5. the autograd path ------------------------------------------------------------------------------------------------------------
def _frozen_backward(cfg, inputs, keys):
    """_hip_backward with every parameter frozen: the leaves are the embedding tables alone"""
    from tests.test_gpu_kernels import _hip_render
    pn, emb_np, emb_s_np, b = inputs
    dev = _dev()
    gp = _gpu_params(pn, dev, requires_grad=False)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    emb_s_g = torch.from_numpy(emb_s_np).to(dev).requires_grad_(True) if emb_s_np is not None else None
    hip = _hip_render(cfg, gp, emb_g, b, dev, emb_s_g)
    hip.pop("_z_vals")
    outs = [hip[k] for k in keys]
    cots = [CT._cotangent(k, hip[k].shape).to(dev) for k in keys]
    _, launches = _profiled(lambda: torch.autograd.backward(outs, cots))
    return emb_g.grad, (emb_s_g.grad if emb_s_g is not None else None), launches


@pytest.mark.parametrize("variant,mode", [("default", "composed"), ("t_s", "separate"), ("tj", "one-plane")])
def test_autograd_takes_the_flagged_path_when_no_parameter_needs_a_gradient(variant, mode, monkeypatch):
    _mode(monkeypatch, mode)
    cfg, inputs = _case_inputs(variant, 37, 24, 64)
    keys = CT._keys_of(cfg)      # main + sc pass
    g_t, g_ts, launches = _frozen_backward(cfg, inputs, keys)
    assert launches[2] == 0 and launches[1] == 0, launches      # no wide dW, no trunk launch in either pass
    (grads, _), full_launches = _profiled(lambda: _hip_backward(cfg, inputs, keys))
    assert full_launches[2] > 0
    assert torch.equal(g_t, grads[TABLES[0]]) and float(g_t.abs().max()) > 0.0
    if variant == "t_s":
        assert torch.equal(g_ts, grads[TABLES[1]]) and float(g_ts.abs().max()) > 0.0
    # parameters that require gradients still get every one of them
    missing = [k for k, v in grads.items() if v is None]
    assert not missing, missing


def test_autograd_grad_of_t_alone_from_a_trainable_network(monkeypatch):
    """torch.autograd.grad(..., inputs=[table]) on a network whose parameters DO require gradients: ctx.needs_input_grad reports what
    required a gradient at the forward, not what this call asks for, so the pass goes the full way, exactly as before the flag --
    the same d_t, and no parameter's .grad is touched"""
    from tests.test_gpu_kernels import _hip_render
    _mode(monkeypatch, "composed")
    cfg, inputs = _case_inputs("default", 37, 24, 64)
    pn, emb_np, _, b = inputs
    dev = _dev()
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    hip = _hip_render(cfg, gp, emb_g, b, dev)
    keys = [k for k in CT._keys_of(cfg)]
    (g,), launches = _profiled(lambda: torch.autograd.grad([hip[k] for k in keys], [emb_g], [CT._cotangent(k, hip[k].shape).to(dev) for k in keys]))
    assert launches[2] > 0, launches                 # the unchanged path: its wide dW launches run
    assert all(v.grad is None for v in gp.values())
    grads, _ = _hip_backward(cfg, inputs, keys)
    assert torch.equal(g, grads[TABLES[0]])


# ---- 6. the vector override ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth():
    """a small synthetic pipeline whose colour head reads t (use_tj_instead_of_beta), 64 rays x 8 samples, W = 64, tau = 4, SIREN, 5 classes"""
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import load_pipeline
    dev = _dev()
    cfg = O.OracleCfg(fc_units=64, n_samples=8, use_tj_instead_of_beta=True, sc_lambda=0.0)
    cfgs = MainConfig(run={"max_train_steps": 10, "synthetic_rays": 4096},
                      pipeline={"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64, "n_samples": 8,
                                "batch_size": 64, "ignore_car_index": True, "depth_enabled": False, "first_beta_epoch": 0,
                                "use_tj_instead_of_beta": True, "render_chunk_size": 1 << 20})
    pipe = load_pipeline(cfgs).to(dev)
    params = O.init_params_numpy(cfg, 4)
    emb = O.init_embedding_numpy(cfg, 4)
    with torch.no_grad():
        named = dict(pipe.model_coarse.named_parameters())
        for k, v in params.items():
            named[k].copy_(torch.from_numpy(v))
        pipe.model_t.weight.copy_(torch.from_numpy(emb))
    b = O.batch_to_torch(O.synthetic_batch(64, 8, seed=17))
    return cfg, cfgs, pipe, params, emb, b


def _with_ts(extras, r):
    e = extras.clone()
    e[:, 3] = float(r)
    return e


@pytest.mark.parametrize("r", [0, 3])
def test_vector_override_has_the_bits_of_the_row(synth, r):
    from snerf_amd.eval.utils.util import result_buffers
    cfg, cfgs, pipe, _, _, b = synth
    dev = _dev()
    rays, extras = b["rays"].to(dev), _with_ts(b["extras"].to(dev), r)
    other = _with_ts(extras, 7)                                     # the override wins over whatever ts says
    vec = pipe.model_t.weight[r].detach().clone()
    keys = ("rgb_coarse", "beta_coarse", "semantic_logits_coarse", "depth_coarse")
    ref, got = (result_buffers(keys, 64, 8, 5, dev) for _ in range(2))
    ws = pipe.renderer.render_rays_into(pipe.models, rays, extras, ref, {"perturb": 0})
    ws2 = pipe.renderer.render_rays_into(pipe.models, rays, other, got, {"perturb": 0, "t_vector": vec})
    for k in keys:
        assert torch.equal(ref[k], got[k]), k
    wrong = result_buffers(keys, 64, 8, 5, dev)
    pipe.renderer.render_rays_into(pipe.models, rays, other, wrong, {"perturb": 0})
    assert not torch.equal(wrong["rgb_coarse"], ref["rgb_coarse"])      # (row 7 is another colour: the comparison can fail)
    # relight on each base pass, under another sun
    sun = extras.clone()
    sun[:, :3] = torch.nn.functional.normalize(sun[:, :3] + torch.tensor([0.3, -0.2, 0.1], device=dev), dim=1)
    sun_other = other.clone()
    sun_other[:, :3] = sun[:, :3]
    rk = ("rgb_coarse", "sun_coarse", "beta_coarse")
    ref2, got2 = (result_buffers(rk, 64, 8, 5, dev) for _ in range(2))
    pipe.renderer.relight_rays_into(pipe.models, sun, ref2, {"workspace": ws})
    pipe.renderer.relight_rays_into(pipe.models, sun_other, got2, {"workspace": ws2, "t_vector": vec})
    for k in rk:
        assert torch.equal(ref2[k], got2[k]), k
    assert not torch.equal(ref2["rgb_coarse"], ref["rgb_coarse"])
    with pytest.raises(ValueError, match="t_vector"):
        pipe.renderer.render_rays_into(pipe.models, rays, extras, got, {"perturb": 0, "t_vector": vec[:3]})


def test_vector_override_gradient_is_the_rows(synth):
    cfg, cfgs, pipe, _, _, b = synth
    dev = _dev()
    rays, extras = b["rays"].to(dev), _with_ts(b["extras"].to(dev), 3)
    cot = CT._cotangent("rgb_coarse", (64, 3)).to(dev)
    pipe.model_t.weight.grad = None
    res = pipe.renderer.render_rays(pipe.models, rays, extras, render_options={"perturb": 0})
    torch.autograd.backward([res["rgb_coarse"]], [cot], inputs=[pipe.model_t.weight])
    want = pipe.model_t.weight.grad[3].clone()
    rest = pipe.model_t.weight.grad.clone()
    rest[3] = 0
    assert float(rest.abs().max()) == 0.0 and float(want.abs().max()) > 0.0      # every ray is row 3's
    pipe.model_t.weight.grad = None
    vec = pipe.model_t.weight[3].detach().clone().requires_grad_(True)
    res = pipe.renderer.render_rays(pipe.models, rays, extras, render_options={"perturb": 0, "t_vector": vec})
    torch.autograd.backward([res["rgb_coarse"]], [cot], inputs=[vec])
    assert torch.equal(vec.grad, want)      # snerf_embedding_backward's fixed-order sum over the rays, either way
    assert pipe.model_t.weight.grad is None


# ---- 7. the fit against the oracle ---------------------------------------------------------------------------------------------------
# Tolerance of the loss history against the fp64 oracle's, relative to the oracle's first loss.  It is to be 10 x the deviation
# MEASURED on the GPU; no run of this module on a GPU has been recorded yet (the test prints the figure), so until one is it
# is DERIVED from the suite's own output bar: loss = mean((rgb - target)^2), so an error of at most OUT_TOL = 1e-4 per colour value
# (tests/test_gpu_kernels.py, the bar of every forward parity test) moves the loss by at most 2 sqrt(loss) OUT_TOL + OUT_TOL^2; at the
# first loss of this case, 1.07e-4 (fp64 oracle on the CPU), that is 2.1e-6 = 1.9e-2 of it.  For scale: the fp32 oracle's history
# departs from the fp64 one's by 2.6e-6 of the first loss on the CPU.
FIT_TOL = 2e-2


def test_fit_follows_the_fp64_oracle(synth):
    """64 rays, S = 8, W = 64, tau = 4, SIREN, 5 classes; target = the oracle's render under table row 5, init = row 2, 30 Adam steps
    (lr 0.05) on all 64 rays; the same optimisation of oracle.render_rays in fp64 with torch autograd and torch.optim.Adam.
    The loss history must stay within FIT_TOL x (the oracle's first loss) of the oracle's at every step.
    Measured deviation on an MI355X: NOT YET (see FIT_TOL); on the CPU the oracle's loss falls from 1.07e-4 to 2.09e-6 in the 30 steps."""
    from snerf_amd.eval.utils.embedding import fit_image_embedding
    cfg, cfgs, pipe, params, emb, b = synth
    dev = _dev()
    a_row, b_row, steps, lr = 5, 2, 30, 0.05
    p64 = O.to_torch(params, dtype=torch.float64)
    rays64, extras64 = b["rays"].double(), b["extras"].double().clone()
    extras64[:, 3] = 0
    table = torch.from_numpy(emb).double()
    with torch.no_grad():
        target = O.render_rays(p64, table[a_row].view(1, -1), cfg, rays64, extras64, None)["rgb_coarse"]
    vec = table[b_row].clone().requires_grad_(True)
    opt = torch.optim.Adam([vec], lr=lr)
    want = []
    for k in range(steps + 1):
        loss = O.snerf_loss(O.render_rays(p64, vec.view(1, -1), cfg, rays64, extras64, None), target, cfg)["coarse_color"]
        want.append(float(loss.detach()))
        if k < steps:
            opt.zero_grad()
            loss.backward()
            opt.step()
    fit = fit_image_embedding(cfgs, pipe.renderer, pipe.models, b["rays"].to(dev), b["extras"].to(dev), target.float().to(dev),
                              init=b_row, steps=steps, lr=lr, rays_per_fit=64)
    got = fit["loss"]
    assert len(got) == steps + 1 and fit["rays"] == 64 and tuple(fit["t"].shape) == (4,)
    dev_rel = max(abs(g - w) for g, w in zip(got, want)) / want[0]
    print("fit: first / best loss", got[0], got[fit["best_step"]], "best step", fit["best_step"], "oracle first / last", want[0], want[-1],
          "max |loss - oracle| / oracle first:", dev_rel)
    assert fit["best_step"] > 0 and got[fit["best_step"]] < got[0]
    assert got[fit["best_step"]] == min(got)
    assert dev_rel <= FIT_TOL, (dev_rel, FIT_TOL)


def test_fit_refuses_a_model_whose_colour_does_not_read_t():
    from snerf_amd.eval.utils.embedding import fit_image_embedding
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import load_pipeline
    dev = _dev()
    cfgs = MainConfig(run={"max_train_steps": 10, "synthetic_rays": 4096},
                      pipeline={"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64, "n_samples": 8,
                                "batch_size": 64, "ignore_car_index": True, "depth_enabled": False, "first_beta_epoch": 0,
                                "render_chunk_size": 1 << 20})
    pipe = load_pipeline(cfgs).to(dev)
    b = O.batch_to_torch(O.synthetic_batch(64, 8, seed=17))
    with pytest.raises(ValueError, match="use_tj_instead_of_beta"):
        fit_image_embedding(cfgs, pipe.renderer, pipe.models, b["rays"].to(dev), b["extras"].to(dev), b["rgbs"].to(dev), steps=1, lr=0.05, rays_per_fit=8)


# ---- 8. evaluation on the fixture scene ----------------------------------------------------------------------------------------------
def test_evaluation_on_the_fixture_scene(tmp_path):
    from snerf_amd.baseline.dataset.satnerf_dataset import unlisted_test_views
    from snerf_amd.eval.eval_nerf import eval_nerf_images
    from snerf_amd.eval.eval_semantic import eval_semantic_images
    from snerf_amd.eval.utils import metrics
    from snerf_amd.eval.utils.util import lean_inference
    from snerf_amd.framework.configs import MainConfig
    from snerf_amd.framework.pipelines import load_pipeline
    torch.manual_seed(0)
    c = MainConfig(run={"max_train_steps": 6, "dataset_dp": SCENE, "cache_dp": str(tmp_path), "dataset_name": "scene_small"},
                   pipeline={"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64, "n_samples": 16,
                             "batch_size": 128, "depth_enabled": False, "first_beta_epoch": 0, "sparsity_n_images": 2,
                             "use_tj_instead_of_beta": True, "render_chunk_size": 512})
    pipe = load_pipeline(c).to(_dev())
    bank = pipe.datasets["rgb_test"]
    images = bank.scene_images()
    names = [im["name"] for im in images]
    assert names == ["JAX_068_013_RGB", "JAX_068_002_RGB", "JAX_068_005_RGB"]
    with open(os.path.join(SCENE, "root.json")) as f:
        root = json.load(f)
    assert unlisted_test_views(root["train_split"] + root["test_split"]) == [f"JAX_068_{i}_RGB.json" for i in ("007", "009", "005")]
    assert unlisted_test_views(names[1:]) == ["JAX_068_005_RGB"]

    def plain(tag):
        torch.manual_seed(1)
        eval_nerf_images(c, pipe.renderer, pipe.models, images, output_dp=str(tmp_path / tag))
        return open(tmp_path / tag / "results.json", "rb").read()

    assert plain("a") == plain("b") and not os.path.exists(tmp_path / "a" / "t_fit.json")
    opts = {"steps": 6, "lr": 0.05, "rays_per_fit": 200, "n_train": len(root["train_split"])}
    torch.manual_seed(1)
    d = eval_nerf_images(c, pipe.renderer, pipe.models, images, output_dp=str(tmp_path / "fit"), fit_embedding=opts)
    vectors = json.load(open(tmp_path / "fit" / "t_fit.json"))
    assert list(vectors) == names[1:] and all(len(v) == 4 for v in vectors.values())
    assert json.load(open(tmp_path / "fit" / "results.json")) == d
    torch.manual_seed(1)
    for im in images[1:]:
        e = d[im["name"]]
        assert set(e) == {"psnr", "ssim", "psnr_heldout", "t_fit"}
        tf = e["t_fit"]
        assert tf["region"] == "left" and tf["steps"] == 6 and 0 <= tf["best_step"] <= 6 and tf["loss_best"] <= tf["loss_first"]
        rays, extras = (im[k].reshape(-1, im[k].shape[-1]) for k in ("rays", "extras"))
        vec = torch.tensor(vectors[im["name"]], dtype=torch.float32, device=rays.device)
        frame = lean_inference(c, pipe.renderer, pipe.models, rays, extras, keys=("rgb_coarse", "depth_coarse"), render_options={"t_vector": vec})
        rgbs = im["rgbs"].reshape(-1, 3)
        assert e["psnr"] == "{:.2f}".format(float(metrics.psnr(frame["rgb_coarse"], rgbs)))
        right = (torch.arange(im["w"], device=rays.device) >= im["w"] // 2).repeat(im["h"])
        assert e["psnr_heldout"] == "{:.2f}".format(float(metrics.psnr(frame["rgb_coarse"], rgbs, valid_mask=right)))
    # region "all": no held-out key; the semantic evaluator carries the same two entries
    d_all = eval_nerf_images(c, pipe.renderer, pipe.models, images, fit_embedding=dict(opts, region="all"))
    assert all(set(d_all[n]) == {"psnr", "ssim", "t_fit"} and d_all[n]["t_fit"]["region"] == "all" for n in names[1:])
    s = eval_semantic_images(c, pipe.renderer, pipe.models, images, bank.semantic_n_classes, bank.car_cls_idx, output_dp=str(tmp_path / "sem"),
                             fit_embedding=opts)
    for n in names[1:]:
        assert "psnr_heldout" in s[n] and s[n]["t_fit"]["loss_best"] <= s[n]["t_fit"]["loss_first"] and "mIoU" in s[n]
    sem_vectors = json.load(open(tmp_path / "sem" / "t_fit.json"))
    assert sem_vectors == vectors                                   # the same seed, the same subset, the same fit
    s0 = eval_semantic_images(c, pipe.renderer, pipe.models, images, bank.semantic_n_classes, bank.car_cls_idx)
    assert all("t_fit" not in s0[n] and "psnr_heldout" not in s0[n] for n in names[1:])
