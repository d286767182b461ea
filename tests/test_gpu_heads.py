"""The heads and the compositing kernel at every class count, head width, embedding width and saturation the plan accepts, against the oracle.

The class count comes from the dataset (semantic_dataset.py: len(semantic_cls_labels)) and make_plan accepts 0 ... 16 (MAX_CLASSES); the head
width feat_last any multiple of 16 up to 512 (fc_units // 2, or fc_units with fc_use_full_features); the transient code tau as long as
3 + tau (x2 with a separate t_s) <= 16 (csrc/api.hip: make_plan).  Each switches code paths the paper's config never runs:
- C <= 5 at H = 256 folds the final head layers into the first head layer's epilogue (Plan::nd_fin); C >= 6 takes the 32-wide launch;
- H = 48 / 80 / 192 / 384 put head blocks across the 128-column exponent blocks (Plan::KF), H = 48 / 80 / 192 leave the sky MLP's last
  lane group partly empty (composite.hip: sky_forward, u = lane + 64 i);
- W = 768 / 1024 fold sigma as 3 / 4 partial tiles (Plan::nd_sig);
- saturated heads -- the regime of a trained model -- run alpha = 1 (tau = 1e-10 and the backward's division by it), transmittance that
  underflows, softplus above its threshold, closed clamp gates of the colour and mass carried from one 64-sample chunk into the next.

Pattern of tests/test_gpu_geometry.py (_oracle_parity): the HIP path renders N rays (N x S ragged), the oracle re-renders a subset
(tests/helpers.py: dealiased_subset -- strided with an offset per ray, live rays in every row-tile residue and both tile halves);
outputs, the loss set of the subset and every parameter gradient must agree at the suite's bars (imported).  The oracle runs in fp64 where
the reference's own fp32 agrees with fp64 to a quarter of OUT_TOL on the case's subset, otherwise in fp32 with the departure asserted
(_oracle_parity, fp64="auto": measured per case, recorded as "oracle").  The departure is on `sigmas` throughout -- the SIREN trunk's w0 = 30
first layer at init (1.2e-5 ... 2.8e-5, either side of the quarter), the fp32 resolution of sigma itself when saturated (up to 8e-5
at sigma bias 1000, where an fp32 ulp of sigma is 6.1e-5).  Worst errors per case: HEADS_STATS (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests.test_gpu_geometry import _oracle_parity, ONE_PLANE_BARS, DEFAULT_BARS
from tests.test_gpu_kernels import _dev, _gpu_params, _hip_render

pytestmark = pytest.mark.gpu

HEADS_STATS = []   # measured worst errors per case (printed with -s)


def _run(cfg, N, n_sub, seed, mode, monkeypatch, edit=None, name=""):
    bars = ONE_PLANE_BARS if mode == "f16x1" else DEFAULT_BARS
    return _oracle_parity(cfg, N, n_sub, seed, epoch=3, mode=mode, monkeypatch=monkeypatch, n_classes=cfg.n_classes, param_edit=edit,
                          fp64="auto", stats=HEADS_STATS, tag={"case": name, "C": cfg.n_classes, "H": cfg.feat_last, "tau": cfg.t_embedding_tau,
                                                             "S": cfg.n_samples}, **bars)


def _cls_cfg(C, W=512, **kw):
    """labels from synthetic_batch(n_classes=C): its car class is C - 1.  One class has no valid label once the car class is ignored."""
    return O.OracleCfg(fc_units=W, n_samples=32, n_classes=C, car_index=C - 1, ignore_car_index=C > 1, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# class counts
# ---------------------------------------------------------------------------------------------------------------------------------
CLASS_CASES = [(C, "f16x2", {}) for C in (1, 2, 6, 9, 16)] + [(C, "f16x1", {}) for C in (6, 16)] + [
    (16, "f16x2", {"semantic_activation_function": "none"}),
    (16, "f16x2", {"use_separate_beta_for_s": True, "use_beta_for_s": True}),          # beta_s + 16 classes: columns 0 ... 20
    (16, "f16x1", {"use_separate_beta_for_s": True, "use_beta_for_s": True})]


@pytest.mark.parametrize("C,mode,kw", CLASS_CASES, ids=[f"C{c}-{m}" + "".join("-" + k for k in sorted(kw)) for c, m, kw in CLASS_CASES])
def test_class_counts_at_full_width(C, mode, kw, monkeypatch):
    """W = 512 SIREN, 301 rays x 32 samples (75.25 tiles), 64 through the oracle: C <= 5 folds the final head layers, C >= 6 runs the
    32-wide final launch up to column 5 + C of the narrow buffer, the per-class accumulators / argmax of the composite and the CE gradient"""
    _run(_cls_cfg(C, **kw), 301, 64, seed=71, mode=mode, monkeypatch=monkeypatch, name="classes")


@pytest.mark.parametrize("C", [9, 16])
def test_class_counts_at_narrow_width(C, monkeypatch):
    """W = 64 (no folded projections at all): 301 rays x 32 samples, 100 through the oracle"""
    _run(_cls_cfg(C, W=64), 301, 100, seed=72, mode="f16x2", monkeypatch=monkeypatch, name="classes-narrow")


def _launches(fn):
    """fn()'s result and the launch count per SnerfProfile variant (3: the 32-wide head launches)"""
    from snerf_amd import _lib
    lib = _lib.lib()
    _lib.check(lib.snerf_profile_begin(), "snerf_profile_begin")
    try:
        out = fn()
    finally:
        prof = _lib.SnerfProfile()
        _lib.check(lib.snerf_profile_end(C.byref(prof)), "snerf_profile_end")
    return out, [int(prof.launches[i]) for i in range(4)]


@pytest.mark.parametrize("n_classes", [5, 6])
def test_final_layer_fold_on_each_side_of_five_classes(n_classes, monkeypatch):
    """Plan::nd_fin: at W = 512 SIREN with C <= ND_FIN = 5 the rgb / semantic / beta final layers ride in the first head layer's epilogue
    and the inference forward (main + solar-correction pass) makes no 32-wide launch at all (sigma and sun visibility fold too); at C = 6
    exactly one -- the final head layers.  Then the same case at the suite's bars."""
    from snerf_amd import ops, _lib
    monkeypatch.setattr(ops, "BASE_FLAGS", _lib.MFMA_FLAGS["f16x2"])
    dev = _dev()
    cfg = _cls_cfg(n_classes)
    gp = _gpu_params(O.init_params_numpy(cfg, 73), dev)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, 73)).to(dev)
    b = O.batch_to_torch(O.synthetic_batch(77, 32, seed=74, n_classes=n_classes))
    with torch.no_grad():
        _, n = _launches(lambda: _hip_render(cfg, gp, emb, b, dev))
    assert n[3] == (0 if n_classes <= 5 else 1), n
    _run(cfg, 301, 64, seed=73, mode="f16x2", monkeypatch=monkeypatch, name="fold")


# ---------------------------------------------------------------------------------------------------------------------------------
# head widths
# ---------------------------------------------------------------------------------------------------------------------------------
WIDTH_CASES = ([(W, False, "f16x2") for W in (96, 160, 384, 768, 1024)] + [(W, True, "f16x2") for W in (96, 160, 384)] +
               [(W, False, "f16x1") for W in (384, 768, 1024)])


@pytest.mark.parametrize("W,full,mode", WIDTH_CASES, ids=[f"W{W}{'-full' if f else ''}-{m}" for W, f, m in WIDTH_CASES])
def test_head_widths(W, full, mode, monkeypatch):
    """H = 48, 80, 192, 384, 512 (fc_units // 2) and H = W (fc_use_full_features): head blocks that straddle the 128-column exponent blocks
    of the fused first head layer (KF = round_up((nblk - 1) H, 128)), a sky MLP whose hidden units do not fill whole lane groups, sigma
    folded as 3 / 4 partial tiles at W = 768 / 1024.  301 rays x 32 samples, 64 through the oracle.  One plane needs W % 64 == 0 and
    H % 32 == 0 (test_abi_cpu.py: W = 96 is refused)."""
    cfg = O.OracleCfg(fc_units=W, n_samples=32, fc_use_full_features=full)
    _run(cfg, 301, 64, seed=75, mode=mode, monkeypatch=monkeypatch, name="width")


# ---------------------------------------------------------------------------------------------------------------------------------
# embedding widths
# ---------------------------------------------------------------------------------------------------------------------------------
TAU_CASES = [(1, {"use_tj_instead_of_beta": True, "use_tj_for_s": True}), (13, {"use_tj_instead_of_beta": True, "use_tj_for_s": True}),
             (13, {}), (6, {"use_separate_tj_for_semantic": True, "use_tj_for_s": True}),
             (6, {"use_separate_tj_for_semantic": True, "use_tj_for_s": True, "use_separate_beta_for_s": True, "use_beta_for_s": True})]


@pytest.mark.parametrize("tau,kw", TAU_CASES, ids=[f"tau{t}" + "".join("-" + k for k in sorted(kw)) for t, kw in TAU_CASES])
def test_embedding_widths_at_full_width(tau, kw, monkeypatch):
    """3 + tau (x2 with a separate t_s) columns of the extras block behind the feats: 4, 16 (exactly full) and 15, W = 512"""
    cfg = O.OracleCfg(n_samples=32, t_embedding_tau=tau, **kw)
    _run(cfg, 301, 64, seed=76, mode="f16x2", monkeypatch=monkeypatch, name="tau")


# ---------------------------------------------------------------------------------------------------------------------------------
# saturation
# ---------------------------------------------------------------------------------------------------------------------------------
SIG, RGB, SUN = "sigma_from_xyz.0.bias", "rgb_from_xyzdir.2.bias", "sun_v_net.6.bias"
# name: (bias shifts, {regime measure: (lo, hi)} on the oracle's subset)
SATURATION = {
    # sigma ~ 6: most of the mass inside the volume, transmittance well above underflow
    "dense": ({SIG: 6.0}, {"t_final_lt_1e-6": (0.0, 0.0), "mean_t_final": (0.0, 0.1), "sigma_pre_gt_20": (0.0, 0.0), "raw_rgb_out": (0.0, 0.0)}),
    # sigma pre-activations around 20: both branches of softplus / its gradient (+25, as first estimated, is above 20 everywhere)
    "softplus20": ({SIG: 20.0}, {"t_final_lt_1e-6": (0.7, 1.0), "sigma_pre_gt_20": (0.2, 0.8), "raw_rgb_out": (0.0, 0.0)}),
    # sigma ~ 1000: alpha rounds to exactly 1 in fp32 where delta * sigma > 17 (S = 32 mostly), T underflows to zero within a few samples
    # (1000, not 4000: fp32 itself resolves sigma ~ 4000 to 2.4e-4, beyond OUT_TOL on the `sigmas` output; ~ 1000 to 6.1e-5)
    "opaque": ({SIG: 1000.0}, {"t_final_lt_1e-6": (1.0, 1.0), "sigma_pre_gt_20": (1.0, 1.0), "t_underflow": (0.99, 1.0), "raw_rgb_out": (0.0, 0.0)}),
    # opaque, albedo and sun visibility at sigmoid(12): raw rgb ~ 1.0009 > 1, the clamp gate closed
    "bright": ({SIG: 20.0, RGB: 12.0, SUN: 12.0}, {"t_final_lt_1e-6": (0.7, 1.0), "raw_rgb_above_1": (1.0, 1.0)}),
    # albedo at sigmoid(-12): raw rgb ~ -0.0007 < 0
    "dark": ({RGB: -12.0}, {"t_final_lt_1e-6": (0.0, 0.0), "raw_rgb_below_0": (1.0, 1.0)}),
    # sigma ~ 1e-13: nearly empty space, the far sample's 1e10 delta carries the weight
    "empty": ({SIG: -30.0}, {"t_final_lt_1e-6": (0.0, 0.0), "far_weight_share": (0.99, 1.0), "raw_rgb_out": (0.0, 0.0)}),
}
BEHIND = {SIG: 3.0}   # S = 130: T at sample 64 in [1e-3, 0.5] and >= 10 % of the weight mass behind sample 64 (asserted)


def regime(ora, bs, cfg):
    """measures of the regime a case reached, on the oracle's outputs for the subset"""
    w, T, sig = ora["weights_coarse"].double(), ora["transparency_coarse"].double(), ora["sigmas_coarse"].double()
    v = ora["sun_coarse"].double()
    raw = (w[..., None] * ora["albedo_coarse"].double() * (v + (1 - v) * ora["sky_coarse"].double())).sum(-2)   # before the clamp
    _, z = O.sample_rays(bs["rays"].float(), cfg.n_samples, bs["u"].float())
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    alpha32 = 1 - torch.exp(-delta * torch.relu(ora["sigmas_coarse"].float()))            # fp32, as the kernels compute it
    m = {"t_final_lt_1e-6": float((T[:, -1] < 1e-6).double().mean()), "mean_t_final": float(T[:, -1].mean()),
         # softplus(x) > 20 <=> x > 20 (up to 2e-9)
         "sigma_pre_gt_20": float((sig > 20).double().mean()),
         "raw_rgb_out": float(((raw < -1e-4) | (raw > 1 + 1e-4)).any(-1).double().mean()),
         "raw_rgb_above_1": float((raw > 1 + 1e-4).all(-1).double().mean()), "raw_rgb_below_0": float((raw < -1e-4).all(-1).double().mean()),
         "t_underflow": float((T < 1e-38).any(-1).double().mean()), "alpha_is_1": float((alpha32[:, :-1] == 1).double().mean()),
         "far_weight_share": float((w[:, -1] / w.sum(-1) > 0.9).double().mean()),
         # rays with a channel within fp32 noise of a clamp boundary, where the two sides may take different gates
         "near_clamp": int((torch.minimum(raw.abs(), (raw - 1).abs()) < 1e-5).any(-1).sum())}
    if cfg.n_samples > 64:
        m["t64_in"] = float(((T[:, 64] >= 1e-3) & (T[:, 64] <= 0.5)).double().mean())
        m["mass_behind_64"] = float(w[:, 64:].sum() / w.sum())
    return m


SAT_CASES = [(n, W, S) for n in SATURATION for W in (512, 64) for S in (32, 96, 130)] + [("behind", W, 130) for W in (512, 64)]


@pytest.mark.parametrize("name,W,S", SAT_CASES, ids=[f"{n}-W{W}-S{S}" for n, W, S in SAT_CASES])
def test_compositing_saturated(name, W, S, monkeypatch):
    """head biases of the seeded weights shifted on both sides (the regime of a trained model), 301 rays (64 / 100 through the oracle);
    every case first asserts that it reached the regime it names, and that no ray lies within fp32 noise of a clamp boundary"""
    cfg = O.OracleCfg(fc_units=W, n_samples=S)
    edit, want = (BEHIND, {}) if name == "behind" else SATURATION[name]
    ora, bs = _run(cfg, 301, 64 if W == 512 else 100, seed=77, mode="f16x2", monkeypatch=monkeypatch, edit=edit, name=name)
    m = regime(ora, bs, cfg)
    HEADS_STATS[-1]["regime"] = m
    print("regime:", name, W, S, m)
    assert m["near_clamp"] == 0, m
    for k, (lo, hi) in want.items():
        assert lo <= m[k] <= hi, (k, m[k], (lo, hi))
    if name == "opaque" and S == 32:
        assert m["alpha_is_1"] >= 0.5, m                     # the division by tau = 1e-10 in the backward
    if name == "behind":
        assert m["t64_in"] >= 0.9 and m["mass_behind_64"] >= 0.1, m   # carryT / suffix_carry carry real mass
