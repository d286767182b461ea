"""feats_from_xyz composed into the fused first head layer (Plan::compose_feats, csrc/api.hip / csrc/bsp_pass.hip) on the GPU.

  b  one c2 training render with SNERF_COMPOSE_FEATS=0 and one with the default, same batch and weights, one process, fresh plans:
     both within the output / loss / gradient bars of tests/test_gpu_fullbatch.py against the chunked fp64 oracle, and per parameter
     tensor the composed path's relative-L2 error no more than TWICE the separate path's (the oracle is the measure; the factor is room
     for another rounding order of the same arithmetic); a tensor whose separate-path error is below GRAD_REL_TOL / 10 only has to
     stay below GRAD_REL_TOL / 4
  c  the composed path is bitwise reproducible, outputs and gradients
  e  batched_inference / lean_inference of the composed path within OUT_TOL of the oracle, labels by the qualified-argmax rule
  m  a pass planned under the other setting of the switch than the pack is refused

  a  the compose and the un-compose launch, with the job tables the pack / a backward pass build (snerf_test_bsp_dw, planes = 0), against
     fp64 on the same fp32 inputs: EVERY element within the fp32 dot-product bound (K + 2) 2^-24 (|A| |B|) of its contraction (the
     rank-one and additive terms counted into |A| |B|), at W = 512 with H = 256, at a narrow network and for the sc pass's row block

The algebra itself is pinned on the CPU (tests/test_compose_cpu.py)."""
import os

import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import max_abs, rel_err
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render, _compare_outputs, OUT_TOL, GRAD_REL_TOL
from tests.test_gpu_pipeline import _pipeline_for, LOSS_RTOL
from tests.test_gpu_fullbatch import _inputs, _oracle, _check_grads, _check_losses

pytestmark = pytest.mark.gpu
SWITCH = "SNERF_COMPOSE_FEATS"


U = 2.0 ** -24


def _hook(mode, A, B, Cbuf, M, FA, W):
    import ctypes as C
    from snerf_amd import _lib
    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.snerf_test_bsp_dw(ptr(A), 0, ptr(B), 0, W, M, FA, 0, 0, 0, mode, ptr(Cbuf), 0, None), "snerf_test_bsp_dw(planes=0)")
    torch.cuda.synchronize()


def _within(got, ref, mag, K, what):
    """every element: |got - ref| <= (K + 2) 2^-24 mag, mag = sum of the absolute values of the terms of that element"""
    err = (got.double().cpu() - ref).abs()
    bound = (K + 2) * U * mag
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / bound.clamp_min(1e-300)).max()))


# (W, FA, N1, row block of the un-compose launch): the headline layer; a narrow network (FA - W = 80, tail tiles in every job);
# the sc pass: the sun-visibility block, the last H = 256 rows of the headline layer
@pytest.mark.parametrize("W,FA,N1,r0,M", [(512, 528, 1024, 0, 1024), (64, 144, 160, 0, 160), (512, 528, 1024, 768, 256), (64, 144, 160, 128, 32)],
                         ids=["w512-h256", "narrow", "w512-sc-block", "narrow-sc-block"])
def test_compose_and_uncompose_kernels_elementwise(W, FA, N1, r0, M):
    dev = _dev()
    g = torch.Generator().manual_seed(W + N1 + r0)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    w_h1, b_h1 = r(N1, FA) / FA ** 0.5, r(N1)
    w_f, b_f = r(W + 32, W) / W ** 0.5, r(W)              # feats rows, then the 32 sigma rows
    d = lambda t: t.double()
    # ---- compose (the whole layer: main and sc pass share the pack)
    A = torch.cat([w_h1.reshape(-1), b_h1]).to(dev)
    B = torch.cat([w_f.reshape(-1), b_f]).to(dev)
    Cb = torch.full(((N1 + 32) * FA + N1,), float("nan"), device=dev)
    _hook(0, A, B, Cb, N1, FA, W)
    wc = Cb[:(N1 + 32) * FA].reshape(N1 + 32, FA)
    bc = Cb[(N1 + 32) * FA:]
    a64, wf64 = d(w_h1[:, :W]), d(w_f[:W])
    _within(wc[:N1, :W], a64 @ wf64, a64.abs() @ wf64.abs(), W, "W_c[:, :W]")
    assert torch.equal(wc[:N1, W:].cpu(), w_h1[:, W:]) and torch.equal(wc[N1:, :W].cpu(), w_f[W:])       # copies: exact
    assert float(wc[N1:, W:].abs().max()) == 0.0
    _within(bc, d(b_h1) + a64 @ d(b_f), d(b_h1).abs() + a64.abs() @ d(b_f).abs(), W, "b_c")
    # ---- un-compose of rows [r0, r0 + M), added to what the gradient buffers hold
    G, gc = r(M, FA), r(M)
    blk = w_h1[r0:r0 + M]
    init = [r(M, FA), r(M), r(W, W), r(W)]
    A = torch.cat([G.reshape(-1), gc]).to(dev)
    B = torch.cat([blk.reshape(-1), w_f[:W].reshape(-1), b_f]).to(dev)
    Cb = torch.cat([t.reshape(-1) for t in init]).to(dev)
    _hook(1, A, B, Cb, M, FA, W)
    o = 0
    outs = []
    for t in init:
        outs.append(Cb[o:o + t.numel()].reshape(t.shape)); o += t.numel()
    dw_h1, db_h1, dw_f, db_f = outs
    G64, gc64, blk64, bf64 = d(G[:, :W]), d(gc), d(blk[:, :W]), d(b_f)
    _within(dw_h1[:, :W], d(init[0][:, :W]) + G64 @ wf64.T + torch.outer(gc64, bf64),
            d(init[0][:, :W]).abs() + G64.abs() @ wf64.abs().T + torch.outer(gc64.abs(), bf64.abs()), W, "dW_h1[:, :W]")
    assert torch.equal(dw_h1[:, W:].cpu(), init[0][:, W:])                 # the extras columns are not this launch's (a reduction job adds them)
    _within(db_h1, d(init[1]) + gc64, d(init[1]).abs() + gc64.abs(), 0, "db_h1")
    _within(dw_f, d(init[2]) + blk64.T @ G64, d(init[2]).abs() + blk64.abs().T @ G64.abs(), M, "dW_f")
    _within(db_f, d(init[3]) + blk64.T @ gc64, d(init[3]).abs() + blk64.abs().T @ gc64.abs(), M, "db_f")


def _step(monkeypatch, setting, name="c2"):
    """one training render + the oracle's loss set + backward, planned under SNERF_COMPOSE_FEATS = setting (None: unset, the default)"""
    if setting is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, setting)
    dev = _dev()
    cfg, pn, emb_np, b, epoch = _inputs(name)
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    hip = _hip_render(cfg, gp, emb_g, b, dev)
    hip.pop("_z_vals")
    ld = O.training_losses(hip, {k: v.to(dev) for k, v in b.items()}, cfg, epoch)
    O.total_loss(ld).backward()
    terms = {k: float(v.detach()) for k, v in ld.items()}
    grads = {k: v.grad.detach().clone() for k, v in gp.items() if v.grad is not None}
    return cfg, {k: v.detach().cpu() for k, v in hip.items()}, terms, grads, emb_g.grad.detach().clone()


def test_composed_and_separate_against_the_oracle(monkeypatch):
    ora = _oracle("c2")
    runs = {}
    for label, setting in (("separate", "0"), ("composed", None)):
        cfg, out, terms, grads, emb = _step(monkeypatch, setting)
        _compare_outputs(out, ora["out"], cfg)
        st = {}
        _check_losses(terms, ora, LOSS_RTOL, st)
        _check_grads({k: grads.get(k) for k in ora["grads"]}, emb, ora, GRAD_REL_TOL, st)
        errs = {}
        for k, r in ora["grads"].items():
            if r is not None and float(r.abs().max()) > 0.0:
                errs[k] = rel_err(grads[k].cpu().double(), r)
        errs["model_t.weight"] = rel_err(emb.cpu().double(), ora["emb"])
        runs[label] = (errs, st, max(max_abs(out[k], v) for k, v in ora["out"].items() if k != "semantic_label_coarse"))
    sep, com = runs["separate"][0], runs["composed"][0]
    # the witness that the default plan WAS composed at this shape: another rounding order, so not the same bits
    assert any(sep[k] != com[k] for k in sep), "the default path gave the separate path's gradients bit for bit: not composed?"
    lines = ["| tensor | separate | composed | ratio |", "|---|---|---|---|"]
    for k in sep:
        lines.append(f"| {k} | {sep[k]:.3e} | {com[k]:.3e} | {com[k] / max(sep[k], 1e-300):.2f} |")
    lines.append("")
    for label in ("separate", "composed"):
        lines.append(f"{label}: worst output error {runs[label][2]:.3e}, worst loss term {runs[label][1]['loss_rel']:.3e}")
    table = "\n".join(lines)
    print(table)
    if os.environ.get("SNERF_COMPOSE_NUMERICS_OUT"):
        with open(os.environ["SNERF_COMPOSE_NUMERICS_OUT"], "w") as f:
            f.write(table + "\n")
    for k in sep:
        if sep[k] < GRAD_REL_TOL / 10:
            assert com[k] < GRAD_REL_TOL / 4, (k, sep[k], com[k])
        else:
            assert com[k] <= 2 * sep[k], (k, sep[k], com[k])


def test_composed_path_is_bitwise_reproducible(monkeypatch):
    a = _step(monkeypatch, None)
    b = _step(monkeypatch, None)
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert torch.equal(a[4], b[4])


@pytest.mark.parametrize("fc_units", [64, 512])
def test_composed_inference_values_vs_oracle(monkeypatch, fc_units):
    from snerf_amd.eval.utils.util import batched_inference, lean_inference
    monkeypatch.delenv(SWITCH, raising=False)
    dev = _dev()
    cfg = O.OracleCfg(fc_units=fc_units, n_samples=24, render_chunk_size=100)
    pipe, params = _pipeline_for(cfg, 64, 5)
    b = O.batch_to_torch(O.synthetic_batch(333, 24, seed=15))
    rays, extras, u = b["rays"].to(dev), b["extras"].to(dev), b["u"].to(dev)
    ro = {"perturb_rand": u}
    bi = batched_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro)
    ora = O.render_rays(O.to_torch(params), torch.from_numpy(O.init_embedding_numpy(cfg, 5)), cfg, b["rays"], b["extras"], b["u"])
    ora.pop("_z_vals")
    assert set(bi) == set(ora)
    for k, v in ora.items():
        if k == "semantic_label_coarse":
            top2 = ora["semantic_logits_coarse"].topk(2, dim=-1).values
            sure = (top2[:, 0] - top2[:, 1]) > 2 * OUT_TOL
            assert torch.equal(bi[k].cpu()[sure], v[sure])
        else:
            assert max_abs(bi[k].cpu(), v) <= OUT_TOL, (k, max_abs(bi[k].cpu(), v))
    keys = tuple(ora)
    lean = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=ro)
    for k in keys:
        if k == "semantic_label_coarse":
            assert torch.equal(lean[k].cpu()[sure], ora[k][sure])
        else:
            assert max_abs(lean[k].cpu(), ora[k]) <= OUT_TOL, (k, max_abs(lean[k].cpu(), ora[k]))


def test_pack_and_pass_must_agree_on_the_switch(monkeypatch):
    from snerf_amd import ops
    dev = _dev()
    cfg = O.OracleCfg(fc_units=64, n_samples=8)
    pn, emb_np = O.init_params_numpy(cfg, 3), O.init_embedding_numpy(cfg, 3)
    b = O.batch_to_torch(O.synthetic_batch(32, 8, seed=4))
    real = ops.pack_params

    def pack_separate(*a, **k):       # the pack planned with the switch off, everything after it with the default
        os.environ[SWITCH] = "0"
        try:
            return real(*a, **k)
        finally:
            del os.environ[SWITCH]
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setattr(ops, "pack_params", pack_separate)
    with pytest.raises(RuntimeError, match="SNERF_COMPOSE_FEATS"):
        _hip_render(cfg, _gpu_params(pn, dev), torch.from_numpy(emb_np).to(dev), b, dev)
