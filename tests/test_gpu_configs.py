"""Every BASELINE.json configuration's PER-GPU workload through the HIP path, checked against the CPU oracle.

The oracle (oracle/snerf_oracle.py, pinned to the reference by tests/test_oracle_golden.py) is too slow for a whole
4096-ray batch at fc_units = 512, but rays are independent: the HIP path renders the FULL batch in one launch
sequence (full-size tile maps, split-K factors, multi-GB workspace offsets, operand scales taken over the whole
batch) and the oracle re-renders a fixed subset of its rays -- an exact check of those rays in the full-size
launch.  The subset is de-aliased from the 128-point row tiles (tests/helpers.py: dealiased_subset): its live points fall in
every row-tile residue mod 8 and in both halves of a tile.  The backward check uses the real loss set evaluated on the subset's outputs only: every other ray then
has a zero output gradient, so the parameter gradients of the full-size backward launch sequence must equal the
oracle's gradients of the subset alone.  Every ray live, against an fp64 oracle of the whole batch: tests/test_gpu_fullbatch.py.

| BASELINE config | per-GPU shape | test |
|---|---|---|
| c1 JAX_004 baseline SatNeRF 512 x 32, fp32 | 512 x 32, W = 512 | test_c1_* (whole batch through the oracle) |
| c2 JAX_068 semantic 4096 x 64, fp32 | 4096 x 64 | test_c2_* |
| c3 JAX_214 semantic + L_t, 8192 x 96 on 2 GPUs, bf16 | 4096 x 96 | test_c3_* (default arithmetic at 1e-4 AND the bf16 mode at its own bar) |
| c4 JAX_260 semantic 16384 x 128 on 8 GPUs, fp32 | 2048 x 128 | test_c4_* |
| c5 four scenes 32768 x 128 on 8 GPUs, bf16 | 4096 x 128 | test_c5_* (bf16 mode; full-frame half: tests/test_gpu_pipeline.py) |

Tolerances: 1e-4 absolute on every rendered tensor, class argmax exact wherever the oracle's top-2 margin exceeds
twice the measured logit error, z_vals bit-exact, parameter gradients 2e-4 relative L2 (GRAD_REL_TOL: ten times the largest
error measured on any tensor of any case; BASELINE.json north_star: 1e-4 outputs, argmax bit-exact).  The bf16 mode (REDUCED precision, the reference's `precision = 16`: here the one-plane mode) is judged
PSNR-style: outputs within 5e-3, class agreement >= 98 %, loss terms within 1 %, gradients within 3 % -- stated in the test.  These bars
are what the REFERENCE itself does when its weights carry 1e-3 relative noise (tests/golden/sem_siren_full.npz, yard_*: outputs
5.6e-3, gradients 3.5 %; tools/gen_golden.py), and the mode's training outcome is pinned to the reference's own runs in
tests/test_gpu_pipeline.py (400-step convergence on the synthetic scene, the full-width trajectory inside the reference's noise envelope).
"""
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import dealiased_subset, max_abs, rel_err
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render, _compare_outputs, OUT_TOL, GRAD_REL_TOL, GRAD_ABS_ESCAPE, LABEL_STATS

pytestmark = pytest.mark.gpu


def _sub(d, idx):
    return {k: v[idx] for k, v in d.items()}


REDUCED_MEASURED = []   # what the one-plane mode measured at the configuration sizes (printed with -s)


def _subset_parity(cfg, N, n_sub, seed, epoch, monkeypatch=None, mode=None, out_tol=OUT_TOL, loss_rtol=2e-4,
                   grad_tol=GRAD_REL_TOL, exact_z=True, car_prob=0.03, n_images=19):
    """Render N rays on the HIP path; oracle on n_sub of them (tests/helpers.py: dealiased_subset -- stride N // n_sub plus an
    offset per subset ray, so that the live rays reach every row-tile residue mod 8 and both halves of a tile); outputs, loss
    terms and the parameter gradients of the subset loss must agree."""
    from snerf_amd import ops, _lib
    if mode is not None:
        monkeypatch.setattr(ops, "BASE_FLAGS", _lib.MFMA_FLAGS[mode])
    dev = _dev()
    S = cfg.n_samples
    pn = O.init_params_numpy(cfg, seed)
    emb_np = O.init_embedding_numpy(cfg, seed)
    b = O.batch_to_torch(O.synthetic_batch(N, S, seed=seed + 100, car_prob=car_prob, n_images=n_images))
    idx, residues, halves = dealiased_subset(N, n_sub, S)
    assert residues == set(range(8)) and halves == {0, 1}, ("live rays miss row tiles", residues, halves)
    gp = _gpu_params(pn, dev, requires_grad=True)
    emb_g = torch.from_numpy(emb_np).to(dev).requires_grad_(True)
    sep_ts = cfg.model == "semantic" and cfg.use_separate_tj_for_semantic   # the second embedding as in the fixtures: seed + 1
    emb_s_np = O.init_embedding_numpy(cfg, seed + 1) if sep_ts else None
    emb_s_g = torch.from_numpy(emb_s_np).to(dev).requires_grad_(True) if sep_ts else None
    hip = _hip_render(cfg, gp, emb_g, b, dev, emb_s_g)
    zv = hip.pop("_z_vals")
    # ---- oracle on the subset
    bs = _sub(b, idx)
    po = O.to_torch(pn, requires_grad=True)
    emb_o = torch.from_numpy(emb_np).requires_grad_(True)
    emb_s_o = torch.from_numpy(emb_s_np).requires_grad_(True) if sep_ts else None
    ora = O.render_rays(po, emb_o, cfg, bs["rays"], bs["extras"], bs["u"], emb_s_o)
    zo = ora.pop("_z_vals")
    if exact_z:
        assert torch.equal(zv[idx.to(dev)].cpu(), zo), "sampled depths are not bit-identical"
    hip_sub = {k: v[idx.to(dev)] for k, v in hip.items()}
    if out_tol <= 1e-3:
        _compare_outputs(hip_sub, ora, cfg)
    else:   # REDUCED mode: PSNR-style bar, class agreement as a rate
        worst_out = 0.0
        for k, v in ora.items():
            if k == "semantic_label_coarse":
                agree = float((hip_sub[k].cpu() == v).float().mean())
                assert agree >= 0.98, "class agreement below 98 %"
            else:
                e = max_abs(hip_sub[k].detach().cpu(), v.detach())
                worst_out = max(worst_out, e)
                assert e <= out_tol, (k, e)
        REDUCED_MEASURED.append({"mode": mode, "N": N, "S": S, "worst_output_abs_err": worst_out, "label_agreement": agree if cfg.model == "semantic" else None})
    # ---- the real loss set on the subset's outputs (all other rays get zero output gradients)
    bsg = {k: v.to(dev) for k, v in bs.items()}
    ld_h = O.training_losses(hip_sub, bsg, cfg, epoch)
    ld_o = O.training_losses(ora, bs, cfg, epoch)
    assert set(ld_h) == set(ld_o)
    for k in ld_o:
        ref = float(ld_o[k].detach())
        assert abs(float(ld_h[k].detach()) - ref) <= loss_rtol * max(1.0, abs(ref)), (k, float(ld_h[k].detach()), ref)
    O.total_loss(ld_h).backward()
    O.total_loss(ld_o).backward()
    worst = 0.0
    for k in po:
        if po[k].grad is None:
            assert gp[k].grad is None or float(gp[k].grad.abs().max()) == 0.0, k
            continue
        g, r = gp[k].grad.cpu(), po[k].grad
        err = rel_err(g, r)
        worst = max(worst, err)
        assert err <= grad_tol or max_abs(g, r) <= 1e-7 + GRAD_ABS_ESCAPE * (grad_tol / GRAD_REL_TOL) * float(r.abs().max()), (k, err)
    if emb_o.grad is not None:
        assert rel_err(emb_g.grad.cpu(), emb_o.grad) <= grad_tol
    if sep_ts and emb_s_o.grad is not None:
        assert rel_err(emb_s_g.grad.cpu(), emb_s_o.grad) <= grad_tol
    if mode is not None and REDUCED_MEASURED:
        REDUCED_MEASURED[-1]["worst_grad_rel_l2"] = worst
        print("reduced-precision config:", REDUCED_MEASURED[-1])
    return worst, ld_o


def test_c1_baseline_satnerf_512x32():
    """configs[0]: baseline SatNeRF (no PE, no semantic head), 512 rays x 32 samples, fc_units 512 -- the WHOLE batch
    goes through the oracle (outputs, loss_dict of SatNerfLoss + solar correction, every parameter gradient)."""
    cfg = O.OracleCfg(model="satnerf", n_samples=32)
    _subset_parity(cfg, 512, 512, seed=21, epoch=2)


def test_c2_semantic_4096x64():
    """configs[1] (the headline): 4096 x 64, fc_units 512, SatNerfLoss + sc + SemanticLoss(ignore car)."""
    cfg = O.OracleCfg(n_samples=64)
    _subset_parity(cfg, 4096, 256, seed=22, epoch=2)
    st = LABEL_STATS[-1]   # "class argmax bit-exact": how many rays the exact check covered, and what happened to the rest
    print("c2 labels:", st)
    assert st["rays"] == 256 and st["qualified"] >= 0.99 and st["logit_err"] <= 1e-5


def test_c2_before_first_beta_epoch():
    """same shape in epochs 0-1 (SNerfLoss: no beta term): the beta head and the transient embedding receive NO gradient,
    as in the reference (baseline/components/training_step.py:22-25)"""
    cfg = O.OracleCfg(n_samples=64)
    _subset_parity(cfg, 4096, 128, seed=23, epoch=0)


def test_c3_semantic_car_reg_4096x96_default_arithmetic():
    """configs[2] per-GPU shape (8192 x 96 over 2 GPUs) with L_t active (epoch >= car_reg_loss_start), default arithmetic
    at the fp32 bar; car_prob raised so that the 256-ray subset holds car rays (an empty set is NaN by definition)."""
    cfg = O.OracleCfg(n_samples=96, use_car_reg_loss=True)
    _, ld = _subset_parity(cfg, 4096, 256, seed=24, epoch=3, car_prob=0.1)
    assert "coarse_car_reg_loss" in ld and torch.isfinite(ld["coarse_car_reg_loss"])


def test_c3_semantic_car_reg_4096x96_bf16(monkeypatch):
    """configs[2] in the arithmetic BASELINE names for it (bf16, the reference's precision = 16): REDUCED precision,
    judged PSNR-style -- outputs within 5e-3 of the fp32 oracle (measured 1.3e-3: PSNR of the rendered colours > 57 dB), class
    agreement >= 98 % (measured 100 %), loss terms within 1 %, gradients within 3 % relative L2 (measured 0.4 %).  These bars are
    UNPINNED: the reference publishes no reduced-precision numbers and runs no half-precision path here; they are this build's own
    statement of what the one-plane mode (SNERF_FLAG_F16X1; "bf16" is BASELINE.json's name for it) may cost -- 4x what it measures."""
    cfg = O.OracleCfg(n_samples=96, use_car_reg_loss=True)
    _subset_parity(cfg, 4096, 256, seed=24, epoch=3, car_prob=0.1, monkeypatch=monkeypatch, mode="bf16", out_tol=5e-3,
                   loss_rtol=1e-2, grad_tol=3e-2)


def test_c4_semantic_2048x128():
    """configs[3] per-GPU shape (16384 x 128 over 8 GPUs): S = 128 -> two wavefront chunks per ray in the scans."""
    cfg = O.OracleCfg(n_samples=128)
    _subset_parity(cfg, 2048, 128, seed=25, epoch=2)


def test_c5_semantic_4096x128_bf16(monkeypatch):
    """configs[4] per-GPU training shape (32768 x 128 over 8 GPUs, bf16): 524 k points per pass; REDUCED-precision bars as
    in test_c3_*_bf16 (UNPINNED, see there; measured here: outputs 9.7e-4, gradients 0.7 %).  (The configuration's full-frame inference half:
    test_full_frame_inference_chunk_beyond_4gib.)"""
    cfg = O.OracleCfg(n_samples=128)
    _subset_parity(cfg, 4096, 128, seed=26, epoch=2, monkeypatch=monkeypatch, mode="bf16", out_tol=5e-3, loss_rtol=1e-2,
                   grad_tol=3e-2)


def test_c5_semantic_4096x128_default_arithmetic():
    """the same shape in the default fp32-class arithmetic at the 1e-4 bar"""
    cfg = O.OracleCfg(n_samples=128)
    _subset_parity(cfg, 4096, 128, seed=26, epoch=2)


def test_c5_raised_embedding_vocab_96():
    """configs[4] concatenates four scenes under one model: `t_embedding_vocab` is raised beyond the default 50.
    96 images, image indices up to 95 in the batch: transient codes and their gradient rows beyond index 50 through the whole
    step, as in test_c2 (the library's embedding kernels at this vocabulary: test_embedding_rows_forward_backward[96])."""
    cfg = O.OracleCfg(n_samples=64, t_embedding_vocab=96)
    _subset_parity(cfg, 2048, 192, seed=27, epoch=2, n_images=96)


@pytest.mark.parametrize("kw", [
    {"use_separate_beta_for_s": True, "use_beta_for_s": True},                       # a fourth head block: five column tiles in the first head layer
    {"use_separate_beta_for_s": True, "use_beta_for_s": True, "use_tj_for_s": True},
    {"use_tj_for_s": True}, {"use_tj_instead_of_beta": True}, {"semantic_activation_function": "none"},
    {"activation_function": "relu"},                                                  # no folded projections: the 32-wide launches at full width
    {"n_classes": 4},                                                                 # labels 0..3 valid, 4 = car = the ignore index (outside [0, C): allowed)
    {"fc_use_full_features": True},                                                   # feat_last = 512: head blocks of two column tiles (no final-layer fold)
    {"use_separate_tj_for_semantic": True, "use_tj_for_s": True},                     # t_s: extras block [sun | t | t_s], 11 of 16 columns
], ids=lambda kw: "+".join(sorted(kw)))
def test_model_variants_at_full_width(kw):
    """Every model switch of the reference at fc_units = 512 (where the folded projections -- sigma, sun, and for feat_last = 256 the
    final head layers with up to five projections per column tile -- replace the 32-wide launches), 256 rays x 32 samples, the WHOLE batch
    through the oracle: outputs, the epoch-3 loss set (beta-weighted CE where switched on) and every parameter gradient.  The small-width
    variant tests (tests/test_gpu_kernels.py) run the same switches through the unfolded launches."""
    cfg = O.OracleCfg(n_samples=32, **kw)
    _subset_parity(cfg, 256, 256, seed=31, epoch=3)


@pytest.mark.parametrize("kw", [{"use_separate_beta_for_s": True, "use_beta_for_s": True}, {"fc_use_full_features": True}, {"activation_function": "relu"}],
                         ids=lambda kw: "+".join(sorted(kw)))
def test_model_variants_at_full_width_one_plane(kw, monkeypatch):
    """the same at the REDUCED-precision bars of the one-plane mode (test_c3_*_bf16): the PL = 1 instantiations of the five-tile first
    head layer with folded final layers, of the two-tile head blocks (feat_last = 512) and of the ReLU epilogues"""
    cfg = O.OracleCfg(n_samples=32, **kw)
    # gradients: 3 % for the default head layout (measured 0.4 %); 5 % where a single scalar decides the worst case (measured: the ReLU
    # network 2.5 %; feat_last = 512: 3.4 % on the ONE-element sigma bias, every matrix below 1 %) -- UNPINNED bars, as in test_c3_*_bf16
    loose = "activation_function" in kw or "fc_use_full_features" in kw
    _subset_parity(cfg, 256, 256, seed=31, epoch=3, monkeypatch=monkeypatch, mode="bf16", out_tol=5e-3, loss_rtol=1e-2,
                   grad_tol=5e-2 if loose else 3e-2)
