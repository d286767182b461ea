"""Pins the CPU oracle (oracle/snerf_oracle.py) against golden vectors produced by the REFERENCE's
own modules (tools/gen_golden.py). CPU only; the oracle is the checker for every GPU parity test."""
import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import load_fixture, fixture_params, fixture_batch, max_abs, rel_err

TRAIN_CASES = ["sem_siren_small", "sem_relu_small", "sem_variants_small", "sem_tj_small", "sem_cartreg_small",
               "satnerf_small", "satnerf_relu_small", "sem_siren_full", "satnerf_full_c1",
               "sem_geom3_small", "sem_geom5_small", "sem_geom1_small"]   # trunk depths 3 / 5 / 1, two skips, 6 / 16 frequencies
TRAIN_CASES += ["sem_c9_small", "sem_c16_small", "sem_tau13_small", "sem_ts6_small", "sem_dense_small"]   # 9 / 16 classes, tau 13 / 6 (+ t_s),
                                                                                                       # saturated head biases at S = 80
# fp32 oracle vs fp32 reference on the same CPU: same ATen ops, so tight bounds
OUT_TOL = 2e-6
GRAD_REL = 2e-5


def _run(name):
    z, meta, cfg = load_fixture(name)
    p = O.to_torch(fixture_params(z, meta, cfg), requires_grad=True)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"])).requires_grad_(True)
    emb_s = None
    if cfg.model == "semantic" and cfg.use_separate_tj_for_semantic:
        emb_s = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"] + 1)).requires_grad_(True)
    b = fixture_batch(z)
    res = O.render_rays(p, emb, cfg, b["rays"], b["extras"], b["u"], emb_s)
    depth_res = None
    if meta["with_depth"]:
        bd = fixture_batch(z, "in_depth_")
        depth_res = O.render_rays(p, emb, cfg, bd["rays"], bd["extras"], bd["u"], emb_s)
    ld = O.training_losses(res, b, cfg, meta["epoch"], depth_res)
    return z, meta, cfg, p, emb, emb_s, res, depth_res, ld


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_outputs_match_reference(name):
    z, meta, cfg, p, emb, emb_s, res, depth_res, ld = _run(name)
    n = 0
    for k in z.files:
        if not k.startswith("out_") or k.startswith("out_depth_"):
            continue
        key = k[4:]
        if key == "semantic_label_coarse":
            assert np.array_equal(res[key].numpy(), z[k]), key
        else:
            assert max_abs(res[key].detach(), z[k]) <= OUT_TOL, (key, max_abs(res[key].detach(), z[k]))
        n += 1
    assert n >= 4
    if depth_res is not None:
        assert max_abs(depth_res["depth_coarse"].detach(), z["out_depth_depth_coarse"]) <= OUT_TOL


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_losses_and_grads_match_reference(name):
    z, meta, cfg, p, emb, emb_s, res, depth_res, ld = _run(name)
    ref_terms = {k[5:]: float(z[k]) for k in z.files if k.startswith("loss_") and k != "loss_total"}
    assert set(ref_terms) == set(ld), (sorted(ref_terms), sorted(ld))
    for k, v in ref_terms.items():
        assert abs(float(ld[k].detach()) - v) <= 2e-6 * max(1.0, abs(v)), (k, float(ld[k].detach()), v)
    O.total_loss(ld).backward()
    grads = {k: v.grad for k, v in p.items()}
    grads["model_t.weight"] = emb.grad
    if emb_s is not None:
        grads["model_t_s.weight"] = emb_s.grad
    checked = 0
    for k in z.files:
        if k.startswith("grad_"):
            g = grads[k[5:]]
            g = torch.zeros_like(p[k[5:]]) if g is None else g
            assert rel_err(g, z[k]) <= GRAD_REL or max_abs(g, z[k]) <= 1e-9, (k, rel_err(g, z[k]))
            checked += 1
        elif k.startswith("gradnorm_"):
            g = grads[k[9:]]
            nrm = float(g.double().norm())
            assert abs(nrm - float(z[k])) <= 1e-4 * max(float(z[k]), 1e-12), (k, nrm, float(z[k]))
            s = g.detach().reshape(-1)[:: max(1, g.numel() // 64)][:64]
            assert rel_err(s, z["gradsample_" + k[9:]]) <= 1e-3 or max_abs(s, z["gradsample_" + k[9:]]) <= 1e-8, k
            checked += 1
    assert checked >= 20


def test_nan_semantics_preserved():
    """MSE over an empty car set and CE with every target ignored are NaN in the reference
    (semantic/components/loss.py:147-151; SURVEY hard parts) -- the oracle keeps that."""
    cfg = O.OracleCfg(fc_units=32, n_samples=8, use_car_reg_loss=True)
    res = {"weights_coarse": torch.rand(4, 8), "beta_coarse": torch.rand(4, 8, 1),
           "semantic_logits_coarse": torch.rand(4, 5)}
    labels = torch.zeros(4, 1, dtype=torch.long)
    assert torch.isnan(O.car_reg_loss(res, labels, None, cfg)["coarse_car_reg_loss"])
    labels = torch.full((4, 1), 4, dtype=torch.long)
    assert torch.isnan(O.semantic_loss(res, labels, None, cfg)["coarse_semantic"])


@pytest.mark.parametrize("name", ["inference_sem_small", "inference_satnerf_small"])
def test_inference_seam(name):
    z, meta, cfg = load_fixture(name)
    p = O.to_torch(fixture_params(z, meta, cfg))
    r = O.inference(p, cfg, torch.from_numpy(z["in_xyz"]), torch.from_numpy(z["in_z"]),
                    torch.from_numpy(z["in_sun"]), torch.from_numpy(z["in_t"]))
    for k in z.files:
        if k.startswith("out_"):
            if k == "out_semantic_label":
                assert np.array_equal(r["semantic_label"].numpy(), z[k])
            else:
                assert max_abs(r[k[4:]], z[k]) <= OUT_TOL, k


def test_adam_trajectory():
    """a18: Adam(lr 5e-4, wd 0) on the total loss reproduces the reference model's 3-step trajectory."""
    z, meta, cfg = load_fixture("sem_siren_small")
    p = O.to_torch(fixture_params(z, meta, cfg), requires_grad=True)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"])).requires_grad_(True)
    b = fixture_batch(z)
    opt = torch.optim.Adam(list(p.values()) + [emb], lr=5e-4, weight_decay=0)
    traj = []
    for _ in range(len(z["adam_traj"])):
        opt.zero_grad()
        res = O.render_rays(p, emb, cfg, b["rays"], b["extras"], b["u"])
        loss = O.total_loss(O.training_losses(res, b, cfg, meta["epoch"]))
        traj.append(float(loss))
        loss.backward()
        opt.step()
    assert np.allclose(traj, z["adam_traj"], rtol=0, atol=5e-6), (traj, z["adam_traj"])


@pytest.mark.parametrize("name,loss_atol,w_rel", [("traj25_small", 2e-5, 2e-4), ("traj10_full", 5e-5, 5e-4)])
def test_long_adam_trajectory(name, loss_atol, w_rel):
    """a16 + a18 over many steps: the oracle's composed step -- render, gated losses, stock Adam -- follows
    the REFERENCE's own trajectory for 25 steps at W = 32 (L_t on) and 10 steps at W = 512: total loss and every loss term before
    each step, the final fc_net.8.weight (the skip layer) and the final embedding.  Measured in the build container: 0.0 on every value
    (the oracle runs the same ATen kernels in the same order on the same host); the bars leave room for another host's vectorisation
    (the GPU box's CPU) amplified by the optimiser, and are 20x below what the HIP path is allowed (tests/test_gpu_pipeline.py)."""
    z, meta, cfg = load_fixture(name)
    p = O.to_torch(fixture_params(z, meta, cfg), requires_grad=True)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"])).requires_grad_(True)
    b = fixture_batch(z)
    opt = torch.optim.Adam(list(p.values()) + [emb], lr=5e-4, weight_decay=0)
    steps = meta["steps"]
    worst = 0.0
    for it in range(steps + 1):
        opt.zero_grad()
        res = O.render_rays(p, emb, cfg, b["rays"], b["extras"], b["u"])
        ld = O.training_losses(res, b, cfg, 0)
        loss = O.total_loss(ld)
        assert set(ld) == {k[5:] for k in z.files if k.startswith("traj_") and k != "traj_total"}
        for k, v in ld.items():
            dv = abs(float(v.detach()) - z["traj_" + k][it])
            worst = max(worst, dv)
            assert dv <= loss_atol, (it, k, float(v.detach()), z["traj_" + k][it])
        assert abs(float(loss.detach()) - z["traj_total"][it]) <= loss_atol, (it, float(loss.detach()), z["traj_total"][it])
        if it == steps:
            break
        loss.backward()
        opt.step()
    ew = rel_err(p["fc_net.8.weight"].detach(), z["final_fc_net.8.weight"])
    ee = rel_err(emb.detach(), z["final_model_t.weight"])
    print(f"{name}: worst loss-term deviation {worst:.2e}, final fc_net.8.weight rel {ew:.2e}, embedding rel {ee:.2e}")
    assert ew <= w_rel and ee <= w_rel, (ew, ee)
    # the trajectory is a real one: the weights moved by far more than the bar
    moved = rel_err(O.init_params_numpy(cfg, meta["seed"])["fc_net.8.weight"], z["final_fc_net.8.weight"])
    assert moved > 20 * w_rel, moved


def test_fp64_oracle_close_to_fp32():
    """The fp64 oracle bounds the fp32 rounding noise of the path (used to set GPU tolerances)."""
    z, meta, cfg = load_fixture("sem_siren_small")
    p64 = O.to_torch(fixture_params(z, meta, cfg), dtype=torch.float64)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"])).double()
    b = O.batch_to_torch({k[3:]: z[k] for k in z.files if k.startswith("in_")}, dtype=torch.float64)
    res = O.render_rays(p64, emb, cfg, b["rays"], b["extras"], b["u"])
    assert max_abs(res["rgb_coarse"], z["out_rgb_coarse"]) < 1e-4


def test_oracle_trains_like_the_reference_on_the_synthetic_scene():
    """The first 100 steps of tools/gen_golden.py's convergence_case with the ORACLE in the reference's place: render, gated losses
    (SNerf loss in epochs 0-1, SatNerf loss from step 80 on), Adam + StepLR(0.9) per epoch on contiguous batches of the learnable
    scene -- PSNR / accuracy / mIoU / depth error on the held-out rays at steps 0, 50, 100 against the reference's curves."""
    z, meta, cfg = load_fixture("converge_small")
    B, every, seed = meta["batch"], meta["eval_every"], meta["seed"]
    train, test = O.synthetic_scene(meta["n_bank"], meta["n_test"], seed=meta["scene_seed"], n_classes=cfg.n_classes)
    spe = meta["n_bank"] // B
    p = O.to_torch(O.init_params_numpy(cfg, seed), requires_grad=True)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, seed)).requires_grad_(True)
    opt = torch.optim.Adam(list(p.values()) + [emb], lr=5e-4, weight_decay=0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.9)
    tt = O.batch_to_torch({k: test[k] for k in ("rays", "extras")})
    u_test = torch.from_numpy(O.scene_jitter(seed, -1, meta["n_test"], cfg.n_samples))
    got = {k: [] for k in ("psnr", "acc", "miou", "depth_mae")}
    steps = 2 * every
    for it in range(steps + 1):
        if it % every == 0:
            with torch.no_grad():
                r = O.render_rays(p, emb, cfg, tt["rays"], tt["extras"], u_test)
            m = O.scene_metrics(r["rgb_coarse"].numpy(), r["depth_coarse"].numpy(), r["semantic_logits_coarse"].numpy(), test, cfg.car_index)
            for k, v in m.items():
                got[k].append(v)
        if it == steps:
            break
        epoch, k = divmod(it, spe)
        idx = np.arange(k * B, (k + 1) * B) % meta["n_bank"]
        b = O.batch_to_torch({"rays": train["rays"][idx], "extras": train["extras"][idx], "rgbs": train["rgbs"][idx],
                              "semantic": train["semantic"][idx], "mask": train["mask"][idx],
                              "u": O.scene_jitter(seed, it, B, cfg.n_samples)})
        opt.zero_grad()
        res = O.render_rays(p, emb, cfg, b["rays"], b["extras"], b["u"])
        O.total_loss(O.training_losses(res, b, cfg, epoch)).backward()
        opt.step()
        if (it + 1) % spe == 0:
            sched.step()
    for k, bar in (("psnr", 5e-3), ("acc", 5e-3), ("miou", 5e-3), ("depth_mae", 1e-4)):
        ref = z["run0_" + k][: len(got[k])]
        assert np.abs(np.array(got[k]) - ref).max() <= bar, (k, got[k], ref.tolist())
    assert got["psnr"][-1] > got["psnr"][0] + 8.0
