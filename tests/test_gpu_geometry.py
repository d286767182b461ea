"""The whole pass at trunk geometries other than the default (8 layers, skip at 4, 10 frequencies), against the oracle.

The reference builds its trunk from `fc_layers`, `fc_skips` and `mapping_pos_n_freq` (rs_semantic.py:118-140, satnerf.py) and the library
accepts 1 <= L <= 16, any skip set without layer 0 and 0 ... 16 frequencies (csrc/api.hip: make_plan; one-plane mode refuses raw xyz,
n_freq = 0).  Depth, skip layers and the encoding width decide the first and last layer's shapes, the gamma segments of the skip layers,
the encoding's padding (Ep = 32 / 64 / 96 / 128) and, in one-plane mode at W = 512, whether the trunk runs as one persistent launch
(csrc/bsp_trunk.hip: 3 <= L <= 8, Ep = 64).

Pattern of tests/test_gpu_configs.py (_subset_parity): the HIP path renders N rays (N x S ragged: not a multiple of the 128-point tile),
the oracle re-renders a subset of them (strided, with an offset per ray: tests/helpers.py, dealiased_subset); outputs, the loss set of
the subset (epoch 3 with L_t for the semantic model, epoch 2 for SatNeRF) and every parameter gradient must agree.  The oracle runs in fp64 wherever the reference's own fp32 arithmetic agrees with fp64
(up to 10 frequencies: 2.7e-5 on the outputs at most, a quarter of OUT_TOL).  From 12 frequencies on it does not (sin(2^15 x) turns the
fp32 rounding of the sample positions into 1e-3 at 16 frequencies, 1.3e-4 at 12): there the yardstick is the fp32 oracle, as in
test_gpu_configs.py and the golden tests, and the test asserts that departure.  Bars are the suite's, imported, whatever the yardstick:
default arithmetic OUT_TOL 1e-4, loss terms 2e-4, gradients GRAD_REL_TOL 2e-4 (tests/test_gpu_kernels.py); one plane the bars of
test_model_variants_at_full_width_one_plane (5e-3 outputs, class agreement >= 98 %, 1e-2 loss terms, 3 % gradients)."""
import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import dealiased_subset, max_abs, rel_err
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render, _compare_outputs, OUT_TOL, GRAD_REL_TOL, GRAD_ABS_ESCAPE

pytestmark = pytest.mark.gpu

ONE_PLANE_BARS = dict(out_tol=5e-3, loss_rtol=1e-2, grad_tol=3e-2)     # test_gpu_configs.py: test_model_variants_at_full_width_one_plane
DEFAULT_BARS = dict(out_tol=OUT_TOL, loss_rtol=2e-4, grad_tol=GRAD_REL_TOL)
GEOMETRY_STATS = []   # measured worst errors per case (printed with -s)
FP64_MAX_FREQ = 10    # the fp64 oracle up to here; beyond, the fp32 oracle (module docstring)


def _oracle_parity(cfg, N, n_sub, seed, epoch, mode, out_tol, loss_rtol, grad_tol, monkeypatch, car_prob=0.1, n_classes=None,
                   param_edit=None, fp64=None, stats=None, tag=None):
    """returns the oracle's outputs on the subset (detached) and its batch; pass-through options of tests/test_gpu_heads.py: `n_classes`
    (labels of synthetic_batch; default its own 5), `param_edit` ({name: shift} added to the seeded weights on both sides), `fp64` (the
    yardstick: True / False, "auto" = measured on the subset, default: by frequency count as above), `stats` / `tag` (the list the measured errors go to, and extra fields)"""
    from snerf_amd import ops, _lib
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.MFMA_FLAGS[mode])
    dev = _dev()
    S = cfg.n_samples
    assert (N * S) % 128 != 0
    if fp64 is None:
        fp64 = cfg.model != "semantic" or cfg.mapping_pos_n_freq <= FP64_MAX_FREQ
    pn = O.init_params_numpy(cfg, seed)
    for k, v in (param_edit or {}).items():
        pn[k] = (pn[k] + np.asarray(v, dtype=np.float32)).astype(np.float32)
    emb_np = O.init_embedding_numpy(cfg, seed)
    sep_ts = cfg.model == "semantic" and cfg.use_separate_tj_for_semantic   # the second embedding as in the fixtures: seed + 1
    emb_s_np = O.init_embedding_numpy(cfg, seed + 1) if sep_ts else None
    bn = O.synthetic_batch(N, S, seed=seed + 100, car_prob=car_prob, **({"n_classes": n_classes} if n_classes else {}))
    idx, residues, halves = dealiased_subset(N, n_sub, S)   # live rays in every row-tile residue mod 8 and both tile halves
    assert residues == set(range(8)) and halves == {0, 1}, ("live rays miss row tiles", residues, halves)
    if fp64 == "auto":   # measured: fp64 where the reference's own fp32 agrees with it to a quarter of OUT_TOL on this subset
        with torch.no_grad():
            o = [O.render_rays(O.to_torch(pn, dtype=d), torch.from_numpy(emb_np).to(d), cfg, *(lambda t: (t["rays"], t["extras"], t["u"]))(
                     O.batch_to_torch({k: v[idx.numpy()] for k, v in bn.items()}, dtype=d)), torch.from_numpy(emb_s_np).to(d) if sep_ts else None)
                 for d in (torch.float32, torch.float64)]
        fp64 = max(max_abs(o[0][k], o[1][k]) for k in o[1] if k not in ("semantic_label_coarse", "_z_vals")) <= OUT_TOL / 4
    b = O.batch_to_torch(bn)
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    emb_s_g = torch.from_numpy(emb_s_np).to(dev).requires_grad_(True) if sep_ts else None
    hip = _hip_render(cfg, gp, emb_g, b, dev, emb_s_g)
    zv = hip.pop("_z_vals")
    # ---- the oracle on the subset
    dt = torch.float64 if fp64 else torch.float32
    bs = O.batch_to_torch({k: v[idx.numpy()] for k, v in bn.items()}, dtype=dt)
    po = O.to_torch(pn, requires_grad=True, dtype=dt)
    emb_o = torch.from_numpy(emb_np).to(dt).requires_grad_(True)
    emb_s_o = torch.from_numpy(emb_s_np).to(dt).requires_grad_(True) if sep_ts else None
    ora = O.render_rays(po, emb_o, cfg, bs["rays"], bs["extras"], bs["u"], emb_s_o)
    zo = ora.pop("_z_vals")
    if not fp64:
        assert torch.equal(zv[idx.to(dev)].cpu(), zo), "sampled depths are not bit-identical"
        # why not fp64 here: the reference's own fp32 arithmetic departs from it by more than a quarter of OUT_TOL
        b64 = O.batch_to_torch({k: v[idx.numpy()] for k, v in bn.items()}, dtype=torch.float64)
        with torch.no_grad():
            o64 = O.render_rays(O.to_torch(pn, dtype=torch.float64), torch.from_numpy(emb_np).double(), cfg, b64["rays"], b64["extras"], b64["u"],
                                torch.from_numpy(emb_s_np).double() if sep_ts else None)
        dep = max(max_abs(ora[k].detach(), o64[k]) for k in ora if k != "semantic_label_coarse")
        assert dep > OUT_TOL / 4, dep
    hip_sub = {k: v[idx.to(dev)] for k, v in hip.items()}
    worst_out = 0.0
    for k, v in ora.items():
        if k != "semantic_label_coarse":
            worst_out = max(worst_out, max_abs(hip_sub[k].detach().cpu(), v.detach()))
    if out_tol <= OUT_TOL:
        _compare_outputs(hip_sub, ora, cfg)
    else:   # one plane: PSNR-style bar, class agreement as a rate (test_gpu_configs.py: _subset_parity)
        for k, v in ora.items():
            if k == "semantic_label_coarse":
                assert float((hip_sub[k].cpu() == v).float().mean()) >= 0.98, "class agreement below 98 %"
            else:
                e = max_abs(hip_sub[k].detach().cpu(), v.detach())
                assert e <= out_tol, (k, e)
    # ---- the loss set on the subset's outputs (every other ray: zero output gradient)
    bsg = {k: v.to(dev).to(b[k].dtype) for k, v in bs.items()}
    ld_h = O.training_losses(hip_sub, bsg, cfg, epoch)
    ld_o = O.training_losses(ora, bs, cfg, epoch)
    assert set(ld_h) == set(ld_o)
    worst_loss = 0.0
    for k in ld_o:
        ref = float(ld_o[k].detach())
        d = abs(float(ld_h[k].detach()) - ref) / max(1.0, abs(ref))
        worst_loss = max(worst_loss, d)
        assert d <= loss_rtol, (k, float(ld_h[k].detach()), ref)
    O.total_loss(ld_h).backward()
    O.total_loss(ld_o).backward()
    worst_grad, n = 0.0, 0
    for k in po:
        if po[k].grad is None:
            assert gp[k].grad is None or float(gp[k].grad.abs().max()) == 0.0, k
            continue
        g, r = gp[k].grad.cpu(), po[k].grad
        err = rel_err(g, r)
        worst_grad = max(worst_grad, err)
        assert err <= grad_tol or max_abs(g, r) <= 1e-7 + GRAD_ABS_ESCAPE * (grad_tol / GRAD_REL_TOL) * float(r.abs().max()), (k, err)
        n += 1
    assert n >= 2 * cfg.fc_layers
    if emb_o.grad is not None:
        assert rel_err(emb_g.grad.cpu(), emb_o.grad) <= grad_tol
    if sep_ts and emb_s_o.grad is not None:
        assert rel_err(emb_s_g.grad.cpu(), emb_s_o.grad) <= grad_tol
    out = GEOMETRY_STATS if stats is None else stats
    out.append({"mode": mode, "W": cfg.fc_units, "model": cfg.model, "L": cfg.fc_layers, "skips": tuple(cfg.fc_skips),
                "n_freq": cfg.mapping_pos_n_freq, "oracle": "fp64" if fp64 else "fp32", "out_abs": worst_out,
                "loss_rel": worst_loss, "grad_rel_l2": worst_grad, **(tag or {})})
    print("geometry:" if stats is None else "heads:", out[-1])
    return {k: v.detach() for k, v in ora.items()}, bs


def _cfg(geom, W, S):
    if geom == "satnerf":
        return O.OracleCfg(model="satnerf", fc_units=W, n_samples=S)
    L, skips, F = geom
    return O.OracleCfg(fc_units=W, n_samples=S, fc_layers=L, fc_skips=skips, mapping_pos_n_freq=F, use_car_reg_loss=True)


DEPTHS = [(1, (), 10), (2, (), 10), (3, (), 10), (3, (1,), 10), (5, (1, 3), 10), (9, (2, 4, 6), 10)]
FREQS = [(8, (4,), 1), (8, (4,), 6), (8, (4,), 12), (8, (4,), 16)]
FULL_WIDTH = DEPTHS + FREQS + ["satnerf"]
FULL_WIDTH_CASES = [(g, m) for g in FULL_WIDTH for m in ("f16x2", "f16x1") if not (g == "satnerf" and m == "f16x1")]
NARROW = DEPTHS + [(8, (4,), 1), (8, (4,), 16)]


def _id(g):
    return g if isinstance(g, str) else f"L{g[0]}-skips{'_'.join(map(str, g[1])) or 'none'}-F{g[2]}"


@pytest.mark.parametrize("geom,mode", FULL_WIDTH_CASES, ids=[f"{_id(g)}-{m}" for g, m in FULL_WIDTH_CASES])
def test_full_width_geometry_against_oracle(geom, mode, monkeypatch):
    """W = 512, S = 32, 449 rays (14,368 points: 112.25 tiles), 64 of them through the oracle, in both arithmetic modes.  These are
    training passes: one plane runs the fused trunk at L = 5 and at 1 / 6 frequencies, the launch-per-layer path at L = 1 / 2 / 9, at
    12 / 16 frequencies (Ep = 128) and at L = 3 (not fused for training).  SatNeRF in the default arithmetic: raw xyz, whose one-plane
    mode the plan refuses (test_one_plane_satnerf_is_refused)."""
    cfg = _cfg(geom, 512, 32)
    _oracle_parity(cfg, 449, 64, seed=51, epoch=2 if geom == "satnerf" else 3, mode=mode, monkeypatch=monkeypatch,
                   **(ONE_PLANE_BARS if mode == "f16x1" else DEFAULT_BARS))


def test_one_plane_satnerf_is_refused(monkeypatch):
    """raw xyz in one fp16 plane would enter the w0 = 30 first layer rounded to 11 bits (sigma 5.0e-3 off the fp64 oracle, beyond the
    mode's bar): the pass raises the plan's named error instead of computing it"""
    from snerf_amd import ops, _lib
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.FLAG_F16X1)
    dev = _dev()
    cfg = _cfg("satnerf", 512, 32)
    b = O.batch_to_torch(O.synthetic_batch(16, 32, seed=3))
    gp = _gpu_params(O.init_params_numpy(cfg, 3), dev)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, 3)).to(dev)
    with torch.no_grad(), pytest.raises(RuntimeError, match="raw xyz"):
        _hip_render(cfg, gp, emb, b, dev)


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("geom", NARROW, ids=_id)
def test_narrow_geometry_against_oracle(geom, W, monkeypatch):
    """W = 64 / 128, two planes (the default arithmetic, always launch-per-layer): every depth and skip set above, and the encoding
    padded to Ep = 32 (1 frequency: 6 columns) and 96 (16 frequencies); 301 rays x 32 samples (75.25 tiles), 100 of them through the
    oracle"""
    cfg = _cfg(geom, W, 32)
    _oracle_parity(cfg, 301, 100, seed=52, epoch=3, mode="f16x2", monkeypatch=monkeypatch, **DEFAULT_BARS)
