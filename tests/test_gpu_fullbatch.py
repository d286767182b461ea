"""Whole training batches at the BASELINE per-GPU shapes, every ray live, against the oracle run in fp64 on the device.

tests/test_gpu_configs.py renders these shapes in full but can afford the CPU oracle on a subset only: the loss then lives on that
subset and every other ray's output gradient is exactly zero.  Training never looks like that -- every 128-point row tile of every
dZ / dX operand is live and every chunk of a dW split carries gradient.  Here the oracle (oracle/snerf_oracle.py, plain torch: its own
fp64 kernels, not this library's) takes the WHOLE batch on the GPU, with the autograd state of one ray chunk at a time
(tests/helpers.py: chunked_oracle -- forward over chunks, the real loss set on the whole batch, then every chunk's backward with its
slice of d loss / d output).  fp64 is the yardstick up to 10 frequencies (tests/test_gpu_geometry.py: the reference's own fp32 lies
within a quarter of OUT_TOL of it there).

| case | shape | path |
|---|---|---|
| c2 headline | 4096 x 64, epoch 2 | pipe.training_step: fused loss kernels, merged loss plan, gradient sinks |
| c2 per-ray rows | 4096 x 64, epoch 2 | the rays' transient codes as a leaf: d loss / d t of every ray (backward alone, and the step) |
| c3 | 4096 x 96, epoch 3, L_t, car_prob 0.1 | _hip_render + O.training_losses, default arithmetic and one plane |
| c4 | 2048 x 128, epoch 2 | the same, default arithmetic |
| c5 | 4096 x 128, epoch 2 | the same, default arithmetic and one plane |
| ragged | 4093 x 64, 4091 x 96 | default arithmetic: a partial last row tile, an odd row-tile count (tile maps' remainder branch) |

Bars are the suite's, imported: default arithmetic OUT_TOL 1e-4 on every rendered tensor of every ray, labels by _compare_outputs,
loss terms 2e-4, every parameter gradient and the embedding gradient GRAD_REL_TOL 2e-4 relative L2 (or GRAD_ABS_ESCAPE; tensors that
pass only by the escape are printed); one plane the bars of test_c3_*_bf16 (5e-3, class agreement >= 98 %, 1e-2, 3 %); per-ray
rows on every ray above 2^-20 of the loudest ROW_TOL 4e-6 (tests/test_gpu_rows.py) against the fp32 oracle, the yardstick it was
measured against: fp32 arithmetic itself lies up to 4.6e-6 from fp64 on these rows (test_c2_per_ray_rows_backward).

Measured on an MI355X (FULLBATCH_STATS; outputs max abs, loss terms relative, gradients worst relative L2 over tensors):
  c2 training step   losses 5.4e-8, gradients 1.3e-5 (sigma_from_xyz.0.bias), embedding 2.3e-7, no escape
  c3 default         outputs 3.4e-5, losses 4.5e-8, gradients 1.2e-5, embedding 2.0e-7
  c4 default         outputs 4.2e-5, losses 1.1e-7, gradients 8.2e-5 (sigma_from_xyz.0.bias), embedding 2.1e-7
  c5 default         outputs 3.7e-5, losses 8.2e-8, gradients 7.2e-6, embedding 2.7e-7
  c3 one plane       outputs 1.4e-3, labels 99.85 %, losses 6.6e-6, gradients 1.5e-3, embedding 2.4e-4
  c5 one plane       outputs 1.2e-3, labels 99.85 %, losses 2.5e-6, gradients 1.5e-3, embedding 5.1e-4
  ragged 4093 x 64   outputs 5.1e-5, losses 1.5e-8, gradients 6.7e-6
  ragged 4091 x 96   outputs 4.6e-5, losses 5.9e-8, gradients 7.1e-6
  sampled depths     bit-exact with the fp32 sampler, 2.0e-7 from fp64
  per-ray rows       backward against the fp32 oracle: max 6.7e-7, median 1.7e-7 (fp32 oracle vs fp64: 4.6e-6, library vs fp64
                     4.5e-6); through the training step: 6.6e-7 x the loss's own kappa, 2.2e-7 median
No tensor passed by the escape.  The oracle's peak allocation: 3.7 GB (ORACLE_PEAK_LIMIT: 12 GB), 1.2-3.5 s per shape; the module's
wall time: 18 s.
"""
import functools
import time

import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import PerRayRows, chunked_oracle, max_abs, rel_err
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render, _compare_outputs, OUT_TOL, GRAD_REL_TOL, GRAD_ABS_ESCAPE
from tests.test_gpu_pipeline import _pipeline_for, _batch_to_dev, LOSS_RTOL
from tests.test_gpu_rows import ROW_TOL

pytestmark = pytest.mark.gpu

DEFAULT = dict(out_tol=OUT_TOL, loss_rtol=LOSS_RTOL, grad_tol=GRAD_REL_TOL)
ONE_PLANE = dict(out_tol=5e-3, loss_rtol=1e-2, grad_tol=3e-2)   # test_gpu_configs.py: test_c3_semantic_car_reg_4096x96_bf16
ONE_PLANE_AGREE = 0.98
ORACLE_PEAK_LIMIT = 12 << 30    # bytes the fp64 oracle may allocate above what the test holds (the machines are shared)
FULLBATCH_STATS = []            # measured worst errors per case (printed with -s)
KAPPA_CALM = 4                  # rays whose loss factor d loss / d bbar is this well conditioned are held to plain ROW_TOL

CASES = {   # name: (cfg kwargs, N, seed, epoch, car_prob)
    "c2": (dict(n_samples=64), 4096, 22, 2, 0.03),
    "c3": (dict(n_samples=96, use_car_reg_loss=True), 4096, 24, 3, 0.1),
    "c4": (dict(n_samples=128), 2048, 25, 2, 0.03),
    "c5": (dict(n_samples=128), 4096, 26, 2, 0.03),
    "ragged-64": (dict(n_samples=64), 4093, 28, 2, 0.03),
    "ragged-96": (dict(n_samples=96), 4091, 29, 2, 0.03),
}


def _inputs(name):
    kw, N, seed, epoch, car_prob = CASES[name]
    cfg = O.OracleCfg(**kw)
    b = O.batch_to_torch(O.synthetic_batch(N, cfg.n_samples, seed=seed + 100, car_prob=car_prob))
    return cfg, O.init_params_numpy(cfg, seed), O.init_embedding_numpy(cfg, seed), b, epoch


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the fp64 whole-batch oracle of a case, on the GPU, moved to the host (the default and the one-plane test of a shape share it)"""
    cfg, pn, emb_np, b, epoch = _inputs(name)
    t0 = time.perf_counter()
    r = chunked_oracle(cfg, pn, emb_np, b, epoch, _dev())
    secs = time.perf_counter() - t0
    assert r["peak_bytes"] <= ORACLE_PEAK_LIMIT, ("oracle peak allocation", r["peak_bytes"])
    host = lambda t: None if t is None else t.cpu()
    out = {"out": {k: v.cpu() for k, v in r["out"].items() if k != "_z_vals"}, "z": r["out"]["_z_vals"].cpu(), "loss": r["loss"],
           "grads": {k: host(v) for k, v in r["grads"].items()}, "emb": host(r["emb"]), "t_rows": host(r["t_rows"]),
           "g_out": {k: v.cpu() for k, v in r["g_out"].items()},
           "peak_gb": r["peak_bytes"] / 2 ** 30, "secs": secs}
    del r
    torch.cuda.empty_cache()
    return out


def _check_grads(grads, emb_grad, ora, grad_tol, st):
    """every parameter gradient and the embedding gradient within grad_tol relative L2, or (noise around zero) within the escape"""
    worst, worst_k, escaped = 0.0, None, []
    for k, r in ora["grads"].items():
        g = grads[k]
        if r is None or float(r.abs().max()) == 0.0:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        g = g.detach().cpu().double()
        err = rel_err(g, r)
        if err > worst:
            worst, worst_k = err, k
        if err > grad_tol:
            assert max_abs(g, r) <= 1e-7 + GRAD_ABS_ESCAPE * (grad_tol / GRAD_REL_TOL) * float(r.abs().max()), (k, err)
            escaped.append((k, err))
    st.update(grad_rel_l2=worst, grad_worst=worst_k, escaped=escaped)
    if escaped:
        print("passed only by GRAD_ABS_ESCAPE:", escaped)
    if ora["emb"] is not None:
        e = rel_err(emb_grad.detach().cpu().double(), ora["emb"])
        st["emb_rel_l2"] = e
        assert e <= grad_tol, ("model_t.weight", e)
    else:
        assert emb_grad is None or float(emb_grad.abs().max()) == 0.0


def _check_losses(terms, ora, loss_rtol, st):
    assert set(terms) == set(ora["loss"]), (sorted(terms), sorted(ora["loss"]))
    worst = 0.0
    for k, ref in ora["loss"].items():
        d = abs(terms[k] - ref) / max(1.0, abs(ref))
        worst = max(worst, d)
        assert d <= loss_rtol, (k, terms[k], ref)
    st["loss_rel"] = worst


def _render_case(name, mode, monkeypatch, bars):
    """the full batch through _hip_render + the oracle's loss set on the HIP outputs, against the whole-batch fp64 oracle"""
    from snerf_amd import ops, _lib
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.MFMA_FLAGS[mode])
    dev = _dev()
    cfg, pn, emb_np, b, epoch = _inputs(name)
    N, S = b["rays"].shape[0], cfg.n_samples
    t0 = time.perf_counter()
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    hip = _hip_render(cfg, gp, emb_g, b, dev)
    zv = hip.pop("_z_vals").cpu()
    ld = O.training_losses(hip, {k: v.to(dev) for k, v in b.items()}, cfg, epoch)
    O.total_loss(ld).backward()
    terms = {k: float(v.detach()) for k, v in ld.items()}
    hip = {k: v.detach().cpu() for k, v in hip.items()}
    ora = _oracle(name)
    st = {"case": name, "mode": mode, "N": N, "S": S, "oracle_peak_gb": ora["peak_gb"], "oracle_s": ora["secs"]}
    out = ora["out"]
    st["out_abs"] = max(max_abs(hip[k], v) for k, v in out.items() if k != "semantic_label_coarse")
    # sampled depths: bit for bit the fp32 oracle's sampler (no FMA contraction), within OUT_TOL of the fp64 oracle's
    assert torch.equal(zv, O.sample_rays(b["rays"], S, b["u"])[1]), "sampled depths are not bit-identical"
    st["z_abs"] = max_abs(zv, ora["z"])
    assert st["z_abs"] <= OUT_TOL, st["z_abs"]
    if bars["out_tol"] <= OUT_TOL:
        _compare_outputs(hip, out, cfg)
    else:
        agree = float((hip["semantic_label_coarse"] == out["semantic_label_coarse"]).float().mean())
        st["label_agreement"] = agree
        assert agree >= ONE_PLANE_AGREE, ("class agreement", agree)
        for k, v in out.items():
            if k != "semantic_label_coarse":
                e = max_abs(hip[k], v)
                assert e <= bars["out_tol"], (k, e)
    _check_losses(terms, ora, bars["loss_rtol"], st)
    _check_grads({k: v.grad for k, v in gp.items()}, emb_g.grad, ora, bars["grad_tol"], st)
    st["wall_s"] = time.perf_counter() - t0
    FULLBATCH_STATS.append(st)
    print("full batch:", st)


# ----------------------------------------------------------------------------------------------------------------------
# c2: the product's training step
# ----------------------------------------------------------------------------------------------------------------------
def _training_step(monkeypatch, t_leaf=False):
    """pipe.training_step on the c2 batch, jitter drawn through torch.rand as in test_training_step_matches_reference_fixture;
    t_leaf: the rays' transient codes (ops.embed_rows) become one leaf, whose gradient is d loss / d t per ray"""
    from snerf_amd import ops
    cfg, _, _, b, epoch = _inputs("c2")
    pipe, _ = _pipeline_for(cfg, b["rays"].shape[0], CASES["c2"][2])
    pipe.current_epoch = epoch
    u = b["u"].to(_dev())
    monkeypatch.setattr(torch, "rand", lambda *a, **k: u.clone())
    leaves = []
    if t_leaf:
        real = ops.embed_rows

        def rows(embedding, idx):
            leaves.append(real(embedding, idx).detach().requires_grad_(True))
            return leaves[-1]
        monkeypatch.setattr(ops, "embed_rows", rows)
    out = pipe.training_step(_batch_to_dev(b), 0)
    out["loss"].backward()
    return pipe, out, leaves


def test_c2_headline_training_step(monkeypatch):
    """BASELINE c2 (the shape bench.py times): 4096 x 64, fc_units 512, epoch 2, through pipe.training_step -- the fused loss kernels
    with the whole batch's normalisers, the merged loss plan and the gradient sinks -- against the fp64 oracle: every loss term and
    the total within 2e-4, every parameter gradient and the embedding gradient within GRAD_REL_TOL"""
    t0 = time.perf_counter()
    pipe, out, _ = _training_step(monkeypatch)
    terms = {k[len("train/"):]: float(v) for k, v in pipe.logged.items() if k.startswith("train/coarse_")}
    grads = {k: p.grad for k, p in pipe.model_coarse.named_parameters()}
    emb_grad = pipe.model_t.weight.grad
    ora = _oracle("c2")
    st = {"case": "c2-training-step", "mode": "f16x2", "N": 4096, "S": 64, "oracle_peak_gb": ora["peak_gb"], "oracle_s": ora["secs"]}
    _check_losses(terms, ora, LOSS_RTOL, st)
    total = sum(ora["loss"].values())
    assert abs(float(out["loss"].detach()) - total) <= LOSS_RTOL * max(1.0, abs(total)), (float(out["loss"].detach()), total)
    _check_grads(grads, emb_grad, ora, GRAD_REL_TOL, st)
    st["wall_s"] = time.perf_counter() - t0
    FULLBATCH_STATS.append(st)
    print("full batch:", st)


def _row_errors(dt_h, dt_o, S, st):
    """per-ray relative error of d loss / d t on the rows above 2^-20 of the loudest, with the pattern over the tiles: by tile half
    (the ray's first point in rows 0-63 / 64-127 of its row tile) and by row-tile residue mod 8"""
    N = dt_o.shape[0]
    row = dt_o.norm(dim=1)
    live = row >= row.max() * 2.0 ** -20
    err = (dt_h - dt_o).norm(dim=1) / row.clamp_min(1e-300)
    first = torch.arange(N) * S
    half, resid = first % 128 // 64, first // 128 % 8
    st.update(live_rows=int(live.sum()), row_err_max=float(err[live].max()), row_err_median=float(err[live].median()),
              by_half=[float(err[live & (half == h)].max()) for h in (0, 1)],
              by_residue=[float(err[live & (resid == q)].max()) for q in range(8)])
    return err, live, row


@functools.lru_cache(maxsize=None)
def _oracle32(name, driven_by_fp64=False):
    """the same whole-batch oracle in fp32 on the device: the yardstick ROW_TOL was measured against (an fp32 oracle, as in
    test_heavy_tailed_gradients).  driven_by_fp64: its backward driven by the fp64 oracle's output gradients (cast to fp32), i.e. what
    fp32 arithmetic alone makes of exact output gradients"""
    cfg, pn, emb_np, b, epoch = _inputs(name)
    r = chunked_oracle(cfg, pn, emb_np, b, epoch, _dev(), dtype=torch.float32,
                       g_out=_oracle(name)["g_out"] if driven_by_fp64 else None)
    out = {"t_rows": r["t_rows"].double().cpu(), "g_out": {k: v.cpu() for k, v in r["g_out"].items()}}
    del r
    torch.cuda.empty_cache()
    return out


def _hip_rows(name, g_out):
    """d loss / d t per ray of the library's backward of the whole batch, driven by the given output gradients (rounded to fp32)"""
    cfg, pn, emb_np, b, _ = _inputs(name)
    dev = _dev()
    gp = _gpu_params(pn, dev, requires_grad=True)
    t_g = torch.from_numpy(emb_np)[b["extras"][:, 3].long()].to(dev).requires_grad_(True)
    hip = _hip_render(cfg, gp, PerRayRows(t_g), b, dev)
    keys = sorted(g_out)
    torch.autograd.backward([hip[k] for k in keys], [g_out[k].float().to(dev) for k in keys])
    return t_g.grad.detach().cpu().double(), keys


def test_c2_per_ray_rows_backward(monkeypatch):
    """Localisation of the backward kernels at the headline shape: the real loss set's d loss / d output (epoch 2: beta-weighted
    colour, log beta, solar correction, CE) drives the library's backward of all 4096 rays, the rays' transient codes a leaf (as
    test_heavy_tailed_gradients): d loss / d t of every ray above 2^-20 of the loudest within ROW_TOL of the oracle's.
    Yardstick: the fp32 oracle, driven by its own output gradients -- as in test_heavy_tailed_gradients, where ROW_TOL was measured.
    Why not fp64: fp32 arithmetic itself departs from fp64 on these rows beyond ROW_TOL.  Driven by the SAME exact (fp64) output
    gradients, the fp32 oracle's rows lie up to 4.6e-6 from the fp64 oracle's (median 4.5e-7; asserted below: > ROW_TOL / 4), and the
    library's up to 4.5e-6 (median 4.4e-7, flat over row-tile residues and tile halves, worst on loud rays): the same tail, the fp32
    arithmetic's, whichever fp32 implementation computes the rows.  Against the fp32 oracle the library's rows measure 6.7e-7 at most
    (median 1.7e-7, every residue and both halves 4.8e-7 ... 6.7e-7): ROW_TOL holds with 6x to spare, as it did on 192 rays."""
    cfg, _, _, b, _ = _inputs("c2")
    o64, o32 = _oracle("c2"), _oracle32("c2")
    dt_h, keys = _hip_rows("c2", o32["g_out"])
    st = {"case": "c2-per-ray-rows-backward", "outputs_driven": keys}
    err, live, row = _row_errors(dt_h, o32["t_rows"], cfg.n_samples, st)
    # the fp32 arithmetic's own departure from fp64 under exact output gradients, and the library's against fp64 on the same footing
    ref = o64["t_rows"]
    dep = ((_oracle32("c2", driven_by_fp64=True)["t_rows"] - ref).norm(dim=1) / ref.norm(dim=1))[live]
    h64 = ((_hip_rows("c2", o64["g_out"])[0] - ref).norm(dim=1) / ref.norm(dim=1))[live]
    st.update(fp32_oracle_vs_fp64_max=float(dep.max()), fp32_oracle_vs_fp64_median=float(dep.median()),
              hip_vs_fp64_max=float(h64.max()), hip_vs_fp64_median=float(h64.median()))
    FULLBATCH_STATS.append(st)
    print("full batch:", st)
    assert st["live_rows"] == b["rays"].shape[0]
    assert st["fp32_oracle_vs_fp64_max"] > ROW_TOL / 4, ("fp32 arithmetic is close enough to fp64 here: use the fp64 yardstick", st)
    worst = torch.argsort(torch.where(live, err, torch.zeros_like(err)), descending=True)[:5]
    assert st["row_err_max"] <= ROW_TOL, (st, [(int(i), float(err[i]), float(row[i] / row.max())) for i in worst])


def test_c2_per_ray_rows_training_step(monkeypatch):
    """d loss / d t of all 4096 rays through the c2 training step (fused loss kernels included), against the fp32 oracle's rows (the
    yardstick of test_c2_per_ray_rows_backward).  At epoch 2 a ray's whole row carries ONE loss factor, d loss / d bbar =
    -|c - c*|^2 / (3 N bbar^3) + 1 / (2 N bbar) (colour term + log-beta term, bbar = sum_j w_j beta_j + 0.05).  Where the two terms
    nearly cancel, fp32 rounding of either (in the loss kernel on one side, torch's fp32 loss on the other, and of the colour and bbar
    they read) grows by kappa = (|a| + |b|) / |a + b| (from the fp64 oracle; up to 1.5e3 on this batch, median 2): a property of the
    loss, not of the kernels.  Measured: error / kappa 6.6e-7 at most (max 2.5e-4, on a ray with kappa > 380; median 2.2e-7; the worst
    ray with kappa < 10 at 5.1e-6, inside the same 6.6e-7 x kappa).  Bars: ROW_TOL x kappa on every ray, and plain
    ROW_TOL on the rays with kappa < KAPPA_CALM = 4 (3,458 of 4,096 here; measured 1.5e-6 at most), where the loss factor's rounding
    cannot reach it."""
    _, _, leaves = _training_step(monkeypatch, t_leaf=True)
    assert len(leaves) == 1, "one lookup of the transient codes per step (shared by the main and the sc pass)"
    cfg, _, _, b, _ = _inputs("c2")
    o = _oracle("c2")["out"]
    N = b["rays"].shape[0]
    bbar = (o["weights_coarse"] * o["beta_coarse"][..., 0]).sum(-1) + 0.05
    d2 = ((o["rgb_coarse"] - b["rgbs"].double()) ** 2).sum(-1)
    a_, b_ = -d2 / (3 * N * bbar ** 3), 1.0 / (2 * N * bbar)
    kappa = (a_.abs() + b_.abs()) / (a_ + b_).abs()
    st = {"case": "c2-per-ray-rows-training-step", "kappa_max": float(kappa.max()), "kappa_median": float(kappa.median())}
    err, live, row = _row_errors(leaves[0].grad.detach().cpu().double(), _oracle32("c2")["t_rows"], cfg.n_samples, st)
    calm = live & (kappa < KAPPA_CALM)
    st.update(rays_calm=int(calm.sum()), row_err_max_calm=float(err[calm].max()), row_err_over_kappa_max=float((err / kappa)[live].max()))
    FULLBATCH_STATS.append(st)
    print("full batch:", st)
    assert st["live_rows"] >= N - 8, "the real loss set leaves nearly every ray's row live"
    assert st["rays_calm"] >= N // 2, st
    worst = torch.argsort(torch.where(live, err / kappa, torch.zeros_like(err)), descending=True)[:5]
    detail = [(int(i), float(err[i]), float(kappa[i]), float(row[i] / row.max())) for i in worst]
    assert st["row_err_max_calm"] <= ROW_TOL, (st, detail)
    assert st["row_err_over_kappa_max"] <= ROW_TOL, (st, detail)


# ----------------------------------------------------------------------------------------------------------------------
# c3 / c4 / c5 and ragged production shapes through _hip_render
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3", "c4", "c5"])
def test_config_default_arithmetic(name, monkeypatch):
    """BASELINE c3 (L_t at epoch 3, car_prob 0.1), c4 and c5 per-GPU shapes, every ray live, default arithmetic"""
    _render_case(name, "f16x2", monkeypatch, DEFAULT)


@pytest.mark.parametrize("name", ["c3", "c5"])
def test_config_one_plane(name, monkeypatch):
    """c3 and c5 in the arithmetic BASELINE names for them (bf16 = the one-plane mode), every ray live, at test_c3_*_bf16's bars"""
    _render_case(name, "bf16", monkeypatch, ONE_PLANE)


@pytest.mark.parametrize("name", ["ragged-64", "ragged-96"])
def test_ragged_production_shape(name, monkeypatch):
    """production-size launches whose last row tile is partial and whose tile count is not a multiple of 8: the remainder branch of
    tile_of_block (csrc/tiles.h) inside the launch, for the 256-wide head layers (one column tile) and the 512-wide trunk (two)"""
    kw, N, _, _, _ = CASES[name]
    P = N * kw["n_samples"]
    tiles_i = (P + 127) // 128
    assert P % 128 != 0
    for tiles_j in (1, 2):
        assert (tiles_i * tiles_j) % 8 != 0, (tiles_i, tiles_j)
    _render_case(name, "f16x2", monkeypatch, DEFAULT)
