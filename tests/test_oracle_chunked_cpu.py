"""The chunked whole-batch oracle of the full-batch GPU tests (tests/helpers.py: chunked_oracle) against one whole-batch backward
of the same oracle, on CPU in fp64, and the de-aliased oracle subsets (tests/helpers.py: dealiased_subset)."""
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import chunked_oracle, dealiased_subset, max_abs, rel_err


@pytest.mark.parametrize("kw,epoch", [({"use_car_reg_loss": True}, 3), ({"use_separate_tj_for_semantic": True, "use_tj_for_s": True,
                                                                          "use_separate_beta_for_s": True, "use_beta_for_s": True}, 3),
                                      ({}, 0)], ids=["car_reg", "t_s+sbeta", "epoch0"])
def test_chunked_oracle_equals_whole_batch_backward(kw, epoch):
    """300 rays in ragged chunks of 37 rays: the two-phase gradients equal one whole-batch backward to fp64 rounding (the loss's
    normalisers -- means, CE ignore-index count, L_t car-ray count -- are the whole batch's in both)"""
    cfg = O.OracleCfg(fc_units=64, n_samples=24, **kw)
    N = 300
    pn = O.init_params_numpy(cfg, 5)
    emb_np = O.init_embedding_numpy(cfg, 5)
    sep = cfg.use_separate_tj_for_semantic
    emb_s_np = O.init_embedding_numpy(cfg, 6) if sep else None
    b = O.batch_to_torch(O.synthetic_batch(N, 24, seed=7, car_prob=0.1))
    got = chunked_oracle(cfg, pn, emb_np, b, epoch, "cpu", emb_s_np=emb_s_np, chunk_points=37 * 24)
    # the same loss set over one whole-batch graph
    po = O.to_torch(pn, dtype=torch.float64, requires_grad=True)
    emb = torch.from_numpy(emb_np).double().requires_grad_(True)
    emb_s = torch.from_numpy(emb_s_np).double().requires_grad_(True) if sep else None
    b64 = O.batch_to_torch(O.synthetic_batch(N, 24, seed=7, car_prob=0.1), dtype=torch.float64)
    ora = O.render_rays(po, emb, cfg, b64["rays"], b64["extras"], b64["u"], emb_s)
    ld = O.training_losses(ora, b64, cfg, epoch)
    O.total_loss(ld).backward()
    assert set(got["loss"]) == set(ld)
    for k, v in ld.items():
        assert abs(got["loss"][k] - float(v.detach())) <= 1e-12 * max(1.0, abs(float(v.detach()))), k
    for k, v in ora.items():      # (fp64 GEMMs of another row count block differently: equal to rounding, not bit for bit)
        assert got["out"][k].dtype == v.dtype and max_abs(got["out"][k], v.detach()) <= 1e-12, k
    n = 0
    for k, v in po.items():
        if v.grad is None or float(v.grad.abs().max()) == 0.0:
            assert got["grads"][k] is None or float(got["grads"][k].abs().max()) == 0.0, k
            continue
        assert rel_err(got["grads"][k], v.grad) <= 1e-12, (k, rel_err(got["grads"][k], v.grad))
        n += 1
    assert n >= 20
    if epoch >= cfg.first_beta_epoch:
        assert rel_err(got["emb"], emb.grad) <= 1e-12
        t = b64["extras"][:, 3].long()
        assert got["t_rows"].shape == (N, cfg.t_embedding_tau) and float(got["t_rows"][t == t[0]].abs().sum()) > 0
    if sep:
        assert rel_err(got["emb_s"], emb_s.grad) <= 1e-12
    assert got["peak_bytes"] is None
    # driven by given output gradients (the backward alone): the same gradients, no loss terms
    again = chunked_oracle(cfg, pn, emb_np, b, epoch, "cpu", emb_s_np=emb_s_np, chunk_points=50 * 24, g_out=got["g_out"])
    assert again["loss"] == {}
    for k, v in got["grads"].items():
        assert (v is None) == (again["grads"][k] is None) and (v is None or max_abs(again["grads"][k], v) <= 1e-12 * float(v.abs().max() + 1e-300)), k


def test_chunked_oracle_backpropagates_given_cotangents_on_any_output():
    """the yardstick of tests/test_gpu_cotangents.py: cotangents on the outputs no loss sends gradient into (main-pass transparency,
    albedo, sun, sky, sigmas) and on all three sc outputs, which the loss set detaches or never reads -- chunked_oracle(g_out=...)
    in ragged chunks of 13 rays against ONE torch.autograd.backward over an un-chunked O.render_rays, 50 x 24 at W = 32, fp64"""
    cfg = O.OracleCfg(fc_units=32, n_samples=24)
    N = 50
    pn, emb_np = O.init_params_numpy(cfg, 9), O.init_embedding_numpy(cfg, 9)
    b = O.batch_to_torch(O.synthetic_batch(N, 24, seed=11))
    keys = [k + "_coarse" for k in ("transparency", "albedo", "sun", "sky", "sigmas", "weights_sc", "transparency_sc", "sun_sc")]
    po = O.to_torch(pn, dtype=torch.float64, requires_grad=True)
    emb = torch.from_numpy(emb_np).double().requires_grad_(True)
    b64 = O.batch_to_torch(O.synthetic_batch(N, 24, seed=11), dtype=torch.float64)
    ora = O.render_rays(po, emb, cfg, b64["rays"], b64["extras"], b64["u"])
    g = torch.Generator().manual_seed(3)
    g_out = {k: torch.rand(ora[k].shape, generator=g, dtype=torch.float32) * 2 - 1 for k in keys}     # fp32, as the GPU tests draw them
    torch.autograd.backward([ora[k] for k in keys], [g_out[k].double() for k in keys])
    got = chunked_oracle(cfg, pn, emb_np, b, 0, "cpu", chunk_points=13 * 24, g_out=g_out)
    assert got["loss"] == {} and set(got["g_out"]) == set(keys)
    live = 0
    for k, v in po.items():
        if v.grad is None or float(v.grad.abs().max()) == 0.0:
            assert got["grads"][k] is None or float(got["grads"][k].abs().max()) == 0.0, k
            continue
        assert rel_err(got["grads"][k], v.grad) <= 1e-12, (k, rel_err(got["grads"][k], v.grad))
        live += 1
    # trunk, sigma, feats, rgb head, sun head, sky MLP; beta and the semantic head lie under none of these outputs
    assert live == 2 * cfg.fc_layers + 2 + 2 + 4 + 8 + 4
    zero = lambda t: t is None or float(t.abs().max()) == 0.0      # (the heads leave one concatenated tensor: exact zeros, not None)
    for k in ("beta_from_xyz.0.weight", "semantic_prediction.2.weight"):
        assert zero(po[k].grad) and zero(got["grads"][k]), k
    assert zero(emb.grad) and zero(got["emb"]) and zero(got["t_rows"])            # no transient code under them either
    # one key alone, and a cotangent that does reach the transient codes
    for k, table in (("sky_coarse", False), ("beta_coarse", True)):
        for p in po.values():
            p.grad = None
        emb.grad = None
        ora = O.render_rays(po, emb, cfg, b64["rays"], b64["extras"], b64["u"])
        go = {k: torch.rand(ora[k].shape, generator=g, dtype=torch.float32) * 2 - 1}
        ora[k].backward(go[k].double())
        got = chunked_oracle(cfg, pn, emb_np, b, 0, "cpu", chunk_points=13 * 24, g_out=go)
        names = {n for n, p in po.items() if not zero(p.grad)}
        assert names == {n for n, v in got["grads"].items() if not zero(v)}
        assert names == ({n for n in po if n.startswith("sky_color.")} if k == "sky_coarse" else names) and names
        for n in names:
            assert rel_err(got["grads"][n], po[n].grad) <= 1e-12, (k, n)
        assert zero(got["emb"]) == zero(emb.grad) == (not table) and (not table or rel_err(got["emb"], emb.grad) <= 1e-12)


@pytest.mark.parametrize("N,n_sub,S", [(4096, 256, 64), (4096, 128, 64), (4096, 256, 96), (2048, 128, 128), (4096, 128, 128),
                                       (2048, 192, 64), (449, 64, 32)] + [(301, n, S) for n in (64, 100) for S in (32, 96, 130)])
def test_dealiased_subsets_reach_every_tile_residue_and_both_halves(N, n_sub, S):
    """the oracle subsets of tests/test_gpu_configs.py, tests/test_gpu_geometry.py and tests/test_gpu_heads.py (their shapes): live points in every row-tile
    residue mod 8 and in both halves of a tile; the plain stride of the same count at 4096 x 64 reached one residue and one half"""
    idx, residues, halves = dealiased_subset(N, n_sub, S)
    assert len(idx) == n_sub and residues == set(range(8)) and halves == {0, 1}
    if (N, n_sub, S) == (4096, 256, 64):
        plain = torch.arange(0, N, N // n_sub)
        pts = (plain[:, None] * S + torch.arange(S)).reshape(-1)
        assert set((pts // 128 % 8).tolist()) == {0} and set((pts % 128 // 64).tolist()) == {0}
