"""Every output cotangent of the render pass against the oracle run in fp64 on the device.

The loss set (O.training_losses, the fused loss kernels) sends gradient into rgb, depth, weights, beta, beta_semantic and
semantic_logits of the main pass and into sun of the solar-correction (sc) pass only; the reference detaches weights_sc and
transparency_sc.  ops._RenderPass hands snerf_backward a cotangent on every one of its differentiable results, though, and the
composite backward (csrc/composite.hip) has a term for each.  Here seeded cotangents, uniform in [-1, 1], go into chosen outputs of
main + sc pass on both sides: torch.autograd.backward on the library's outputs, tests/helpers.py: chunked_oracle(g_out=...) on the
oracle's (itself pinned on the CPU by tests/test_oracle_chunked_cpu.py).  Every parameter gradient and the embedding tables'
gradients are compared; where the oracle's gradient is None or exactly zero the library's must be None or exactly 0.0.

| test | shapes | what is live |
|---|---|---|
| test_single_cotangent | 37 x 24 at W = 64 / 512, 5 x 130 at W = 64 (three composite chunks, two live lanes in the last) | one key at a time |
| test_single_cotangent_beta_semantic | 37 x 24, W = 512, beta_s | beta_semantic alone |
| test_model_variants | 37 x 24, W = 512: 9 classes, beta_s, separate t_s, SatNeRF | the never-trained-on set; every key |
| test_sc_density_branch | 37 x 24, W = 512, composed and separate first head layer | sc weights + transparency |
| test_zero_structure_* | 37 x 24, W = 64 | sigmas alone; the sc keys alone; nothing |
| test_dense_regime | 5 x 130, W = 64, sigma bias + 6 | every key |
| test_one_plane | 37 x 24, W = 512, FLAG_F16X1 | every key; sc weights + transparency |

Bars: default arithmetic GRAD_REL_TOL 2e-4 relative L2 per tensor, or max_abs <= 1e-7 + GRAD_ABS_ESCAPE max|ref| (printed when a
tensor needs it); one plane ONE_PLANE_BARS["grad_tol"] 3 %.  A single-cotangent case whose tensor misses the bar may rise to 4 x
the fp32 oracle's own departure from fp64 on that tensor, and only where that departure exceeds GRAD_REL_TOL / 4 (measured inside
the test, recorded in COTANGENT_STATS as "raised").

Measured: NOT YET on an MI355X -- no run of this module on a GPU has been recorded, so no library error stands here and no tensor's
bar is raised.  What is measured is the bars' reach: with the fp32 oracle on the CPU standing in for the library (the same
comparison code, every one of the 56 cases, the dense regime included) each tensor stays within GRAD_REL_TOL of the fp64 oracle and
every zero-structure assertion holds, so fp32 arithmetic of another summation order can meet these bars.  Every comparison prints
its record (COTANGENT_STATS, -s): the first GPU run's worst error per case belongs here.
"""
import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import chunked_oracle, max_abs, rel_err
from tests.test_gpu_compose import SWITCH
from tests.test_gpu_geometry import ONE_PLANE_BARS
from tests.test_gpu_heads import SATURATION, regime
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render, GRAD_REL_TOL, GRAD_ABS_ESCAPE

pytestmark = pytest.mark.gpu

COTANGENT_STATS = []   # one record per comparison (printed with -s)

MAIN_KEYS = ["rgb", "depth", "weights", "transparency", "albedo", "sun", "sky", "beta", "sigmas", "beta_semantic", "semantic_logits"]
SC_KEYS = ["weights_sc", "transparency_sc", "sun_sc"]
ALL_KEYS = [k + "_coarse" for k in MAIN_KEYS + SC_KEYS]
# what no loss of the reference sends gradient into (baseline/components/loss.py detaches the two sc tensors)
NEVER_TRAINED_ON = [k + "_coarse" for k in ("transparency", "albedo", "sun", "sky", "sigmas", "weights_sc", "transparency_sc")]
SC_DENSITY = ["weights_sc_coarse", "transparency_sc_coarse"]
SIGMA_ROWS = ("sigma_from_xyz.0.weight", "sigma_from_xyz.0.bias")
TABLES = ("model_t.weight", "model_t_s.weight")


def _keys_of(cfg):
    """the differentiable results of main + sc pass for this model, in ALL_KEYS order"""
    sem = cfg.model == "semantic"
    drop = set() if sem else {"beta_semantic_coarse", "semantic_logits_coarse"}
    if sem and not cfg.use_separate_beta_for_s:
        drop.add("beta_semantic_coarse")
    return [k for k in ALL_KEYS if k not in drop]


def _cotangent(key, shape):
    """seeded by the key alone: a key carries the same cotangent in every set it is part of"""
    g = torch.Generator().manual_seed(1000 + ALL_KEYS.index(key))
    return torch.rand(tuple(shape), generator=g, dtype=torch.float32) * 2 - 1


def _inputs(cfg, N, seed, edit=None):
    assert (N * cfg.n_samples) % 128 != 0     # ragged against the 128-point row tile
    pn = O.init_params_numpy(cfg, seed)
    for k, v in (edit or {}).items():
        pn[k] = (pn[k] + np.asarray(v, dtype=np.float32)).astype(np.float32)
    sep = cfg.model == "semantic" and cfg.use_separate_tj_for_semantic
    emb_s_np = O.init_embedding_numpy(cfg, seed + 1) if sep else None
    b = O.batch_to_torch(O.synthetic_batch(N, cfg.n_samples, seed=seed + 100, n_classes=max(cfg.n_classes, 1)))
    return pn, O.init_embedding_numpy(cfg, seed), emb_s_np, b


def _hip_backward(cfg, inputs, keys, wrap=None):
    """a fresh render of main + sc pass (a pass's workspace goes back to the pool after its first backward), the parameters and the
    embedding tables as leaves, then ONE backward of `keys` with their seeded cotangents.  Returns ({name: gradient or None},
    {key: cotangent})."""
    pn, emb_np, emb_s_np, b = inputs
    dev = _dev()
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    emb_s_g = torch.from_numpy(emb_s_np).to(dev).requires_grad_(True) if emb_s_np is not None else None
    hip = _hip_render(cfg, gp, emb_g, b, dev, emb_s_g)
    hip.pop("_z_vals")
    assert [k for k in ALL_KEYS if k in hip] == _keys_of(cfg)
    g_out = {k: _cotangent(k, hip[k].shape) for k in keys}
    outs = [hip[k] if wrap is None else wrap(hip[k]) for k in keys]
    if outs:
        torch.autograd.backward(outs, [g_out[k].to(dev) for k in keys])
    grads = {k: v.grad for k, v in gp.items()}
    grads[TABLES[0]] = emb_g.grad
    if emb_s_g is not None:
        grads[TABLES[1]] = emb_s_g.grad
    return grads, g_out


def _oracle_grads(cfg, inputs, g_out, dtype=torch.float64):
    pn, emb_np, emb_s_np, b = inputs
    r = chunked_oracle(cfg, pn, emb_np, b, 0, _dev(), emb_s_np=emb_s_np, dtype=dtype, g_out=g_out)
    host = lambda t: None if t is None else t.double().cpu()
    ref = {k: host(v) for k, v in r["grads"].items()}
    ref[TABLES[0]] = host(r["emb"])
    if emb_s_np is not None:
        ref[TABLES[1]] = host(r["emb_s"])
    return ref, {k: v.cpu() for k, v in r["out"].items()}


def _is_zero(t):
    return t is None or float(t.abs().max()) == 0.0


def _compare(cfg, inputs, keys, grad_tol, tag, may_raise=False):
    """library against the fp64 oracle on every parameter and table gradient.  Returns (library gradients, oracle gradients, oracle
    outputs, the record appended to COTANGENT_STATS)."""
    grads, g_out = _hip_backward(cfg, inputs, keys)
    ref, out = _oracle_grads(cfg, inputs, g_out)
    assert set(ref) == set(grads)
    st = {**tag, "keys": [k[:-len("_coarse")] for k in keys], "W": cfg.fc_units, "S": cfg.n_samples, "worst": 0.0, "worst_tensor": None,
          "live": 0, "zero": 0, "escaped": [], "raised": []}
    ref32 = None
    for k, r in ref.items():
        g = grads[k]
        if _is_zero(r):      # zero structure: no noise where nothing arrives
            assert _is_zero(g), (tag, k, "the oracle's gradient is zero / None, the library's is not")
            st["zero"] += 1
            continue
        assert g is not None, (tag, k)
        g = g.detach().double().cpu()
        assert bool(torch.isfinite(g).all()), (tag, k)
        err = rel_err(g, r)
        st["live"] += 1
        if err > st["worst"]:
            st["worst"], st["worst_tensor"] = err, k
        if err <= grad_tol:
            continue
        if max_abs(g, r) <= 1e-7 + GRAD_ABS_ESCAPE * (grad_tol / GRAD_REL_TOL) * float(r.abs().max()):
            st["escaped"].append((k, err))
            continue
        dep = None
        if may_raise:        # the fp32 arithmetic's own departure from fp64 on this tensor, under the same cotangents
            if ref32 is None:
                ref32 = _oracle_grads(cfg, inputs, g_out, dtype=torch.float32)[0]
            dep = rel_err(ref32[k], r)
            if dep > grad_tol / 4 and err <= 4 * dep:
                st["raised"].append((k, err, dep))
                continue
        print("cotangents:", st)
        raise AssertionError((tag, st["keys"], k, "relative L2", err, "bar", grad_tol, "fp32 oracle vs fp64", dep))
    COTANGENT_STATS.append(st)
    print("cotangents:", st)
    if st["escaped"]:
        print("passed only by GRAD_ABS_ESCAPE:", st["escaped"])
    if st["raised"]:
        print("passed only by the raised bar (tensor, error, fp32 oracle vs fp64):", st["raised"])
    assert st["live"] > 0, "no gradient reached any parameter: a vacuous comparison"
    return grads, ref, out, st


def _default_mode(monkeypatch, mode="f16x2"):
    from snerf_amd import ops, _lib
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.MFMA_FLAGS[mode])
    monkeypatch.delenv(SWITCH, raising=False)


# ----------------------------------------------------------------------------------------------------------------------
# 1. one output at a time: a loud path cannot mask a quiet one
# ----------------------------------------------------------------------------------------------------------------------
# 37 x 24: S < 64, one composite chunk.  5 x 130: three chunks, lanes 0 and 1 of the last live, carryT / suffix_carry live.
SINGLE_SHAPES = [(37, 24, 64), (5, 130, 64), (37, 24, 512)]
SINGLE_KEYS = _keys_of(O.OracleCfg())


@pytest.mark.parametrize("N,S,W", SINGLE_SHAPES, ids=[f"{n}x{s}-W{w}" for n, s, w in SINGLE_SHAPES])
@pytest.mark.parametrize("key", SINGLE_KEYS, ids=[k[:-len("_coarse")] for k in SINGLE_KEYS])
def test_single_cotangent(key, N, S, W, monkeypatch):
    """default arithmetic, the default semantic model (5 classes: at W = 512 the final head layers fold, Plan::nd_fin)"""
    _default_mode(monkeypatch)
    cfg = O.OracleCfg(fc_units=W, n_samples=S)
    _compare(cfg, _inputs(cfg, N, seed=81), [key], GRAD_REL_TOL, {"case": "single"}, may_raise=True)


def test_single_cotangent_beta_semantic(monkeypatch):
    """the one key the default model does not have, alone: its own head and nothing else"""
    _default_mode(monkeypatch)
    cfg = O.OracleCfg(fc_units=512, n_samples=24, use_separate_beta_for_s=True, use_beta_for_s=True)
    _, ref, _, _ = _compare(cfg, _inputs(cfg, 37, seed=81), ["beta_semantic_coarse"], GRAD_REL_TOL, {"case": "single"}, may_raise=True)
    assert not _is_zero(ref["semantic_beta_from_xyz.2.weight"]) and _is_zero(ref["beta_from_xyz.2.weight"])


# ----------------------------------------------------------------------------------------------------------------------
# 2. model variants
# ----------------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "c9": dict(n_classes=9, car_index=8),                                       # the 32-wide final launch
    "sbeta": dict(use_separate_beta_for_s=True, use_beta_for_s=True),
    "t_s": dict(use_separate_tj_for_semantic=True, use_tj_for_s=True),           # the second embedding table
    "satnerf": dict(model="satnerf"),                                           # no semantic keys
}


@pytest.mark.parametrize("which", ["never-trained-on", "every-key"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_model_variants(variant, which, monkeypatch):
    """37 x 24 at W = 512: the set no loss reaches in ONE backward, and every key at once"""
    _default_mode(monkeypatch)
    cfg = O.OracleCfg(fc_units=512, n_samples=24, **VARIANTS[variant])
    keys = NEVER_TRAINED_ON if which == "never-trained-on" else _keys_of(cfg)
    _, ref, _, _ = _compare(cfg, _inputs(cfg, 37, seed=82), keys, GRAD_REL_TOL, {"case": f"variant-{variant}"})
    if variant == "t_s" and which == "every-key":
        assert not _is_zero(ref[TABLES[1]])


# ----------------------------------------------------------------------------------------------------------------------
# 3. the density branch of the sc pass (sig_live in backward_bsp), on both first-head-layer plans
# ----------------------------------------------------------------------------------------------------------------------
def _sc_density(monkeypatch, mode, grad_tol, setting):
    _default_mode(monkeypatch, mode)
    if setting is not None:
        monkeypatch.setenv(SWITCH, setting)
    cfg = O.OracleCfg(fc_units=512, n_samples=24)
    grads, ref, _, st = _compare(cfg, _inputs(cfg, 37, seed=83), SC_DENSITY, grad_tol,
                                 {"case": "sc-density", "mode": mode, "compose": setting or "default"})
    for k in SIGMA_ROWS:      # not vacuous: the oracle's sigma rows carry gradient, and so do the library's (compared above)
        assert not _is_zero(ref[k]), k
        assert not _is_zero(grads[k]), k
    # nothing but the trunk and the sigma row lies under the density of the sc pass
    assert {k for k, r in ref.items() if not _is_zero(r)} == set(SIGMA_ROWS) | {k for k in ref if k.startswith("fc_net.")}
    return st


@pytest.mark.parametrize("setting", [None, "0"], ids=["composed", "separate"])
def test_sc_density_branch(setting, monkeypatch):
    """cotangents on sc weights + transparency only: the sigma bias sums, the sigma-row dW launch and the K = h1w + 32 dX launch of an
    sc pass, which no training step runs; SNERF_COMPOSE_FEATS unset (composed at W = 512) and "0" (separate)"""
    _sc_density(monkeypatch, "f16x2", GRAD_REL_TOL, setting)


# ----------------------------------------------------------------------------------------------------------------------
# 4. zero structure
# ----------------------------------------------------------------------------------------------------------------------
def _small():
    cfg = O.OracleCfg(fc_units=64, n_samples=24)
    return cfg, _inputs(cfg, 37, seed=84)


def test_zero_structure_only_sigmas_live(monkeypatch):
    """d sigmas reaches the trunk and the sigma row; every head, the sky MLP and the embedding get exactly nothing"""
    _default_mode(monkeypatch)
    cfg, inputs = _small()
    grads, ref, _, _ = _compare(cfg, inputs, ["sigmas_coarse"], GRAD_REL_TOL, {"case": "zero-sigmas"})
    heads = [k for k in ref if not (k.startswith("fc_net.") or k in SIGMA_ROWS)]
    assert any(k.startswith("sky_color.") for k in heads) and TABLES[0] in heads and len(heads) >= 20
    for k in heads:
        assert _is_zero(ref[k]) and _is_zero(grads[k]), k
    for k in SIGMA_ROWS:
        assert not _is_zero(grads[k]), k


def test_zero_structure_only_sc_live(monkeypatch):
    """the three sc cotangents alone: the main pass contributes nothing and the sc pass reads no transient code, so the embedding
    gradient is the sc pass's cleared d_t buffer (allocated poisoned): exactly zero, finite"""
    _default_mode(monkeypatch)
    cfg, inputs = _small()
    grads, ref, _, _ = _compare(cfg, inputs, [k + "_coarse" for k in SC_KEYS], GRAD_REL_TOL, {"case": "zero-sc"})
    assert _is_zero(ref[TABLES[0]])
    g = grads[TABLES[0]]
    assert g is None or (bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0)
    live = {k for k, r in ref.items() if not _is_zero(r)}
    assert live == set(SIGMA_ROWS) | {k for k in ref if k.startswith(("fc_net.", "sun_v_net.", "feats_from_xyz."))}, sorted(live)


class _NoGradient(torch.autograd.Function):
    """a consumer whose backward hands nothing back: the pass's backward then runs with every cotangent None"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


def test_zero_structure_no_output_live(monkeypatch):
    _default_mode(monkeypatch)
    cfg, inputs = _small()
    grads, _ = _hip_backward(cfg, inputs, _keys_of(cfg), wrap=_NoGradient.apply)
    assert all(g is None for g in grads.values()), [k for k, g in grads.items() if g is not None]


# ----------------------------------------------------------------------------------------------------------------------
# 5. dense regime: the transparency / weights cotangents through real transmittance decay and the chunk carry
# ----------------------------------------------------------------------------------------------------------------------
def test_dense_regime(monkeypatch):
    _default_mode(monkeypatch)
    cfg = O.OracleCfg(fc_units=64, n_samples=130)
    edit, _ = SATURATION["dense"]
    inputs = _inputs(cfg, 5, seed=85, edit=edit)
    _, _, out, st = _compare(cfg, inputs, _keys_of(cfg), GRAD_REL_TOL, {"case": "dense"})
    m = regime(out, inputs[3], cfg)
    st["regime"] = m
    print("regime:", m)
    assert m["mean_t_final"] <= 0.1, m


# ----------------------------------------------------------------------------------------------------------------------
# 6. one plane
# ----------------------------------------------------------------------------------------------------------------------
def test_one_plane_every_key(monkeypatch):
    _default_mode(monkeypatch, "f16x1")
    cfg = O.OracleCfg(fc_units=512, n_samples=24)
    _compare(cfg, _inputs(cfg, 37, seed=86), _keys_of(cfg), ONE_PLANE_BARS["grad_tol"], {"case": "one-plane", "mode": "f16x1"})


def test_one_plane_sc_density_branch(monkeypatch):
    """one plane never composes: the separate branch of test_sc_density_branch in the reduced arithmetic"""
    _sc_density(monkeypatch, "f16x1", ONE_PLANE_BARS["grad_tol"], None)
