"""No result may depend on bytes the library did not write (run with -m gpu on an MI355X).

Every case runs under three fills of the memory the library has not written yet -- workspaces, outputs, scratch:

    0x00  zeros (what a fresh allocation usually holds in a short-lived process)
    0xFF  NaN in fp16 / fp32 / fp64, -1 as an integer
    0x7B  fp16 61280, fp32 ~1.3e36, a large positive integer: a leftover that looks like plausible finite data

and holds it to three things: (a) the three results are bit-identical (compared as integers, so NaN equals NaN), (b) the 0xFF result
is finite wherever the reference is, so every output element was written, (c) the result meets the entry's existing bar against its
existing reference -- the bars are imported from the entry's own test module, or, where that module states them inline, repeated
here with the name of the test that owns them.  Before fills are compared each case runs twice under one fill: every entry below is
bit-reproducible by construction (fixed-order reductions; the only atomics are integer min / max / add, which commute), none
needed the weaker comparison.

Part A drives the render pass, the fused loss, ops.sample_z and the embedding rows through snerf_amd.ops with the diagnostic switch
(ops._WS_POISON, ops._WS_POISON_BYTE): every buffer the library allocates carries the fill.  Part B calls the other C-ABI entries
with buffers the test owns and fills itself.

POINTERS classifies every pointer parameter of every entry of include/snerf_hip.h (test hooks and the profile hook excepted):
    in     read only
    out    pure output: filled by the test before the call
    ws     workspace: filled by the test before the call
    acc    accumulator the CALLER initialises, as the header states: initialised exactly so, never filled (several of them steer a
           loop or an address: the update count of snerf_rpc_*, the bounds of snerf_vis_colormap -- DESIGN.md "Unwritten memory")
    inout  read and overwritten in place
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests.helpers import load_fixture, fixture_params, fixture_batch, max_abs, rel_err
from tests import test_gpu_kernels as K
from tests.test_gpu_kernels import OUT_TOL, GRAD_REL_TOL, GRAD_ABS_ESCAPE, kc_grid_3   # noqa: F401  (kc_grid_3: a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
FILLS = (0x00, 0xFF, 0x7B)

POINTERS = {
    "snerf_pack_params": {"desc": "in", "params": "in", "packed": "out"},
    "snerf_unpack_grads": {"desc": "in", "packed_grads": "in", "grads": "out"},      # accumulate = 1: "acc" (the sinks; not filled)
    "snerf_forward": {"desc": "in", "packed_params": "in", "in": "in", "out": "out", "workspace": "ws"},
    "snerf_sample_z": {"rays": "in", "z_steps": "in", "u": "in", "z": "out"},
    "snerf_embedding_rows": {"table": "in", "idx": "in", "rows": "out"},
    "snerf_embedding_backward": {"idx": "in", "d_rows": "in", "grad_table": "acc"},
    "snerf_backward": {"desc": "in", "packed_params": "in", "in": "in", "gout": "in", "packed_grads": "acc", "d_t": "out",
                       "d_t_s": "out", "workspace": "ws"},     # the workspace holds the forward's activations: leftovers beside them
    "snerf_loss_partial": {"cfg": "in", "in": "in", "totals": "out", "workspace": "ws"},
    "snerf_loss_finish": {"cfg": "in", "in": "in", "totals": "in", "terms": "out", "grads": "out"},
    "snerf_adam_step": {"params": "inout", "grads": "in", "exp_avg": "acc", "exp_avg_sq": "acc"},
    "snerf_dsm_accumulate": {"xyz": "in", "grid": "in", "count": "acc", "sum": "acc", "stats": "acc"},
    "snerf_dsm_finish": {"count": "in", "sum": "in", "dsm": "out", "stats": "acc"},
    "snerf_dsm_downsample2x": {"u": "in", "out": "out"},
    "snerf_dsm_ncc_search": {"u": "in", "v": "in", "stats": "out", "workspace": "ws"},
    "snerf_dsm_shift_diff": {"pred": "in", "gt": "in", "rdsm": "out", "diff": "out", "totals": "out", "workspace": "ws"},
    "snerf_ortho_top": {"xyz": "in", "grid": "in", "top": "acc", "stats": "acc"},
    "snerf_ortho_gather": {"top": "in", "rgb": "in", "labels": "in", "scalar": "in", "alt_out": "out", "idx_out": "out",
                           "rgb_out": "inout", "label_out": "inout", "scalar_out": "inout"},      # payloads: written only in won cells
    "snerf_ortho_votes": {"xyz": "in", "labels": "in", "grid": "in", "votes": "acc", "stats": "acc"},
    "snerf_ortho_votes_finish": {"votes": "in", "label_out": "out", "share_out": "out", "stats": "acc"},
    "snerf_ssim": {"x": "in", "y": "in", "weights2d": "in", "map_or_null": "out", "per_image_sum": "out", "workspace": "ws"},
    "snerf_semeval_accumulate": {"pred": "in", "gt": "in", "gt_no_cars": "in", "gt_non_corrupted": "in", "weights": "in",
                                 "beta": "in", "acc": "acc", "workspace": "ws"},
    "snerf_vis_fold": {"in": "in", "out": "out", "stats": "acc"},
    "snerf_vis_minmax": {"plane": "in", "stats": "acc"},
    "snerf_vis_colormap": {"plane": "in", "stats": "in", "table": "in", "out": "out"},
    "snerf_rpc_rays": {"images_host": "in", "images_dev": "in", "pixels": "in", "rays": "out", "counters": "acc"},
    "snerf_rpc_localize": {"rpc_host": "in", "rpc_dev": "in", "col": "in", "row": "in", "alt": "in", "lon": "out", "lat": "out",
                           "counters": "acc"},
    "snerf_rpc_project": {"rpc_host": "in", "rpc_dev": "in", "lon": "in", "lat": "in", "alt": "in", "col": "out", "row": "out"},
    "snerf_rpc_reprojection_error": {"rpc_host": "in", "rpc_dev": "in", "xyz_ecef": "in", "pts2d": "in", "col_row": "out",
                                     "err": "out"},
    "snerf_ray_bounds": {"rays": "in", "n_rows": "in", "out": "out", "workspace": "ws"},
    "snerf_normalize_rows": {"rows": "inout", "center_range": "in"},
    "snerf_geo_cloud": {"rays": "in", "depth": "in", "params": "in", "enu_out": "out", "lla_out": "out", "stats": "acc"},
    "snerf_geo_points": {"xyz_n": "in", "params": "in", "enu_out": "out", "lla_out": "out", "stats": "acc"},
    # the fill test of these two is tests/test_gpu_shadow.py test_no_output_depends_on_bytes_the_library_did_not_write
    "snerf_shadow_cast": {"dsm": "in", "suns_host": "in", "lit_out": "out", "dist_out": "out"},
    "snerf_shadow_agreement": {"sun": "in", "lit": "in", "valid": "in", "acc": "acc"},
    # the fill tests of these two are test_no_output_depends_on_bytes_the_library_did_not_write of tests/test_gpu_resample.py and
    # of tests/test_gpu_raydist.py
    "snerf_resample_z": {"z": "in", "weights": "in", "u": "in", "z_out": "out", "z_fine": "out"},
    "snerf_ray_distortion": {"weights": "in", "z_vals": "in", "rays": "in", "d_weights": "out", "per_ray": "out", "acc": "acc"},
}
# entries with no device pointer to classify: sizes, version, error text; and the hooks the issue excepts
_NO_POINTERS = ("snerf_version", "snerf_last_error", "snerf_packed_floats", "snerf_grad_floats", "snerf_workspace_bytes",
                "snerf_loss_workspace_bytes", "snerf_dsm_workspace_bytes", "snerf_ssim_workspace_bytes",
                "snerf_semeval_workspace_bytes", "snerf_ray_bounds_workspace_bytes")


def test_pointer_table_covers_the_header():
    from snerf_amd import _lib
    want = {n for n in _lib.SIGNATURES if not n.startswith(("snerf_test_", "snerf_profile_")) and n not in _NO_POINTERS}
    assert set(POINTERS) == want, sorted(set(POINTERS) ^ want)
    for name, roles in POINTERS.items():
        n_ptr = sum(1 for slot in _lib._PLANS[name][0] if slot is None)
        assert len(roles) == n_ptr, (name, len(roles), n_ptr)
        assert set(roles.values()) <= {"in", "out", "ws", "acc", "inout"}


# ---- the harness -------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.float32, torch.float64):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    return t


def _assert_same(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        same = _bits(a[k]) == _bits(b[k])
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} elements differ")


def run_filled(fn, fills=FILLS):
    """fn(fill) -> {name: tensor}, run for every fill; under each fill it runs twice first and must reproduce itself bit for bit.
    Returns {fill: result} after asserting (a): all results are bit-identical."""
    res = {}
    for f in fills:
        res[f] = fn(f)
        _assert_same(res[f], fn(f), f"two runs under fill 0x{f:02X}")
    for f in fills[1:]:
        _assert_same(res[fills[0]], res[f], f"fill 0x{fills[0]:02X} vs 0x{f:02X}")
    return res


def _finite_where(got, ref, what):
    """(b): finite wherever the reference is"""
    g, r = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref)
    if not g.is_floating_point():
        return
    ok = torch.isfinite(r) if r.is_floating_point() else torch.ones_like(g, dtype=torch.bool)
    assert bool(torch.isfinite(g.reshape(ok.shape))[ok].all()), what


def _filled(shape, dtype, fill):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if t.numel():
        t.reshape(-1).view(torch.uint8).fill_(fill)
    return t


def _is_fill(t, fill):
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device).copy_(t.reshape(-1))      # (a strided view has no byte view)
    return bool((flat.view(torch.uint8) == fill).all())


def _poison(mp, fill):
    """the library's own buffers carry `fill` from here on; idle workspaces go back first, so every lease is a fresh fill"""
    from snerf_amd import ops
    mp.setattr(ops, "_WS_POISON", True)
    mp.setattr(ops, "_WS_POISON_BYTE", fill)
    ops.release_workspaces()


# ==============================================================================================================================
# Part A: the render pass, through ops
# ==============================================================================================================================
def _train_pass(cfg, pn, b, emb, emb_s=None, epoch=2, depth_batch=None):
    """main + sc forward, the oracle's losses on the HIP outputs, backward into every parameter and, through t = emb[ts], d_t /
    d_t_s of both passes (the sc pass's are the zeros it writes) -- the pass assembled by test_gpu_kernels._hip_render"""
    dev = torch.device(DEV)
    gp = K._gpu_params(pn, dev, requires_grad=True)
    emb_g = emb.clone().to(dev).requires_grad_(True)
    emb_s_g = emb_s.clone().to(dev).requires_grad_(True) if emb_s is not None else None
    hip = K._hip_render(cfg, gp, emb_g, b, dev, emb_s_g)
    res = {"z_vals": hip.pop("_z_vals")}
    depth_res = K._hip_render(cfg, gp, emb_g, depth_batch, dev, emb_s_g) if depth_batch is not None else None
    bg = {k: v.to(dev) for k, v in b.items()}
    ld = O.training_losses(hip, bg, cfg, epoch, depth_res)
    O.total_loss(ld).backward()
    res.update({"out_" + k: v.detach() for k, v in hip.items()})
    res.update({"loss_" + k: v.detach() for k, v in ld.items()})
    res.update({"grad_" + k: v.grad for k, v in gp.items()})
    res["grad_model_t.weight"] = emb_g.grad
    if emb_s_g is not None:
        res["grad_model_t_s.weight"] = emb_s_g.grad
    assert all(v is not None for v in res.values())
    return res


def _check_grad(name, g, ref):
    ref = torch.as_tensor(ref)
    err = rel_err(g.cpu(), ref)
    scale = float(ref.abs().max())
    assert err <= GRAD_REL_TOL or max_abs(g.cpu(), ref) <= 1e-7 + GRAD_ABS_ESCAPE * scale, (name, err, scale)


FIXTURES = ["sem_siren_small", "sem_relu_small", "satnerf_small", "sem_c9_small", "sem_geom3_small", "sem_tau13_small",
            "sem_ts6_small", "sem_tj_small"]      # the last two: a separate t_s embedding (d_t_s), with and without the sc pass
SEPARATE_TS = ("sem_ts6_small", "sem_tj_small")


@pytest.mark.parametrize("name", FIXTURES)
def test_render_pass_fixtures(name, monkeypatch):
    z, meta, cfg = load_fixture(name)
    pn = fixture_params(z, meta, cfg)
    b = fixture_batch(z)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"]))
    emb_s = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"] + 1)) if cfg.use_separate_tj_for_semantic else None
    bd = fixture_batch(z, "in_depth_") if meta["with_depth"] else None

    def run(fill):
        _poison(monkeypatch, fill)
        return _train_pass(cfg, pn, b, emb, emb_s, meta["epoch"], bd)

    r = run_filled(run)[0xFF]
    assert all(k in z.files for k in r if k.startswith("loss_"))
    # d_t_s is allocated, filled and written exactly where the model has a separate t_s: its gradient must be there, and be checked
    assert ("grad_model_t_s.weight" in r) == (name in SEPARATE_TS) == bool(cfg.use_separate_tj_for_semantic)
    assert ("grad_model_t_s.weight" in z.files) == (name in SEPARATE_TS)
    # the depths against the oracle's sampler, bit for bit (the bar of test_forward_matches_oracle_and_golden)
    _, want_z = O.sample_rays(b["rays"], cfg.n_samples, b["u"])
    assert torch.equal(r["z_vals"].cpu().view(torch.int32), want_z.view(torch.int32))
    # (b) + (c): the bars of test_forward_matches_oracle_and_golden / test_backward_matches_oracle_and_golden on the fixture's reference
    n = 0
    for k in z.files:
        if k.startswith("out_") and not k.startswith("out_depth_") and k != "out_semantic_label_coarse":
            _finite_where(r[k], z[k], k)
            assert max_abs(r[k].cpu(), z[k]) <= OUT_TOL, k
        if k.startswith("loss_") and k in r:
            ref = float(z[k])
            assert abs(float(r[k]) - ref) <= 2e-4 * max(1.0, abs(ref)), (k, float(r[k]), ref)
        if k.startswith("grad_"):
            _finite_where(r[k], z[k], k)
            _check_grad(k, r[k], z[k])
            n += 1
    assert n >= 20


_RAGGED = {}


def _ragged_reference(N, S, W):
    if (N, S, W) not in _RAGGED:
        cfg = O.OracleCfg(fc_units=W, n_samples=S)
        pn = O.init_params_numpy(cfg, 3)
        emb = torch.from_numpy(O.init_embedding_numpy(cfg, 3))
        b = O.batch_to_torch(O.synthetic_batch(N, S, seed=N + S))
        po = O.to_torch(pn, requires_grad=True)
        emb_o = emb.clone().requires_grad_(True)
        ora = O.render_rays(po, emb_o, cfg, b["rays"], b["extras"], b["u"])
        zv = ora.pop("_z_vals").detach()
        O.total_loss(O.training_losses(ora, b, cfg, 2)).backward()
        grads = {k: v.grad.clone() for k, v in po.items()}
        grads["model_t.weight"] = emb_o.grad.clone()
        _RAGGED[(N, S, W)] = (cfg, pn, emb, b, dict({k: v.detach() for k, v in ora.items()}, _z_vals=zv), grads)
    return _RAGGED[(N, S, W)]


@pytest.mark.parametrize("N,S,W", [(37, 96, 64), (5, 130, 32), (129, 7, 32), (1, 64, 32), (3, 130, 512), (37, 96, 512)])
def test_render_pass_ragged_and_multi_chunk_sizes(N, S, W, monkeypatch):
    """the sizes of test_gpu_kernels.test_ragged_and_multi_chunk_sizes: a last 128-row tile partly beyond the points, two wavefront
    chunks per ray, the folded projections' partial sums of a mostly empty tile"""
    cfg, pn, emb, b, ora, grads = _ragged_reference(N, S, W)

    def run(fill):
        _poison(monkeypatch, fill)
        return _train_pass(cfg, pn, b, emb)

    r = run_filled(run)[0xFF]
    ora = dict(ora)
    assert torch.equal(r["z_vals"].cpu().view(torch.int32), ora.pop("_z_vals").view(torch.int32))      # the oracle's depths, bit for bit
    for k, v in ora.items():
        _finite_where(r["out_" + k], v, k)
    K._compare_outputs({k[4:]: v for k, v in r.items() if k.startswith("out_")}, ora, cfg)
    for k, g in grads.items():
        _finite_where(r["grad_" + k], g, k)
        if k == "model_t.weight":
            assert rel_err(r["grad_" + k].cpu(), g) <= GRAD_REL_TOL
        else:
            _check_grad(k, r["grad_" + k], g)


_FULL = {}


def _full_fixture():
    if not _FULL:
        z, meta, cfg = load_fixture("sem_siren_full")
        _FULL.update(z=z, meta=meta, cfg=cfg, pn=fixture_params(z, meta, cfg), b=fixture_batch(z),
                     emb=torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"])))
    return _FULL


@pytest.mark.parametrize("fusion", (1, 0), ids=("trunk-fused", "trunk-per-layer"))
@pytest.mark.parametrize("mode", ("f16x2", "f16x1"))
def test_render_pass_full_width_on_a_forced_small_grid(mode, fusion, kc_grid_3, monkeypatch):
    """W = 512 with three persistent workgroups per launch: the tile loop runs and draws from the tile counters, which the pass's
    first kernel clears.  Default arithmetic (bars of test_full_width_forward_backward) and the one-plane mode (bars of
    test_reduced_precision_mode_full_width, selected as there), with the one-launch trunk on and off."""
    from snerf_amd import ops, _lib
    f = _full_fixture()
    z, cfg = f["z"], f["cfg"]
    L = _lib.lib()

    def run(fill):
        _poison(monkeypatch, fill)
        return _train_pass(cfg, f["pn"], f["b"], f["emb"], None, f["meta"]["epoch"])

    try:
        L.snerf_test_set_trunk_fusion(fusion)
        base = None
        if mode == "f16x1":      # the default arithmetic's gradients, the yardstick of the one-plane mode: computed in this case's own
            #                      trunk-fusion setting and grid, as test_reduced_precision_mode_full_width computes both in one setting
            monkeypatch.setattr(ops, "BASE_FLAGS", 0)
            monkeypatch.setattr(ops, "_WS_POISON", False)
            r0 = _train_pass(cfg, f["pn"], f["b"], f["emb"], None, f["meta"]["epoch"])
            base = {k[5:]: v.cpu() for k, v in r0.items() if k.startswith("grad_") and k != "grad_model_t.weight"}
        monkeypatch.setattr(ops, "BASE_FLAGS", 0 if mode == "f16x2" else _lib.FLAG_F16X1)
        r = run_filled(run)[0xFF]
        if mode == "f16x2":
            # the inference-mode pass (other instantiations of the same kernels, no stored activations) under the last fill: the
            # training pass's outputs bit for bit, as test_full_width_forward_backward asserts of the default arithmetic
            with torch.no_grad():
                inf = K._hip_render(cfg, K._gpu_params(f["pn"], torch.device(DEV)), f["emb"].to(DEV), f["b"], torch.device(DEV))
            inf.pop("_z_vals")
            assert len(inf) >= 10
            for k, v in inf.items():
                assert torch.equal(_bits(v), _bits(r["out_" + k])), k
    finally:
        L.snerf_test_set_trunk_fusion(1)
    yard_out, yard_grad = float(z["yard_out_abs_noise_1e-3"]), float(z["yard_grad_rel_noise_1e-3"])
    out_tol, loss_tol = (OUT_TOL, 2e-4) if mode == "f16x2" else (yard_out, 1e-2)
    for k in z.files:
        if k.startswith("out_") and k != "out_semantic_label_coarse":
            _finite_where(r[k], z[k], k)
            assert max_abs(r[k].cpu(), z[k]) <= out_tol, (k, max_abs(r[k].cpu(), z[k]))
        if k.startswith("loss_") and k in r:
            ref = float(z[k])
            assert abs(float(r[k]) - ref) <= loss_tol * max(1.0, abs(ref)), (k, float(r[k]), ref)
    grads = {k[5:]: v for k, v in r.items() if k.startswith("grad_")}
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    if mode == "f16x2":
        n_full = 0
        for k in z.files:
            if k.startswith("gradnorm_"):
                g = grads[k[9:]]
                nrm, ref = float(g.double().norm()), float(z[k])
                assert abs(nrm - ref) <= GRAD_REL_TOL * max(ref, 1e-9), (k, nrm, ref)
                smp = g.detach().cpu().reshape(-1)[:: max(1, g.numel() // 64)][:64]
                rs = z["gradsample_" + k[9:]]
                assert rel_err(smp, rs) <= 10 * GRAD_REL_TOL or max_abs(smp, rs) <= GRAD_ABS_ESCAPE * float(np.abs(rs).max() + 1e-12), k
            if k.startswith("grad_"):
                assert rel_err(grads[k[5:]].cpu(), z[k]) <= GRAD_REL_TOL, k
                n_full += 1
        assert n_full == 5
    else:
        rel = {k: float(rel_err(grads[k].cpu(), base[k])) for k in base if float(base[k].abs().max()) > 0}
        assert max(rel.values()) <= 1.5 * yard_grad, sorted(rel.items(), key=lambda kv: -kv[1])[:3]


def test_lean_and_batched_inference(monkeypatch):
    """the shape of test_gpu_rows.test_batched_and_lean_inference_values_vs_oracle: ragged render chunks, the inference workspace of
    ops.render_pass_into"""
    from snerf_amd.eval.utils.util import batched_inference, lean_inference
    from tests.test_gpu_pipeline import _pipeline_for
    cfg = O.OracleCfg(fc_units=64, n_samples=24, render_chunk_size=100)
    pipe, params = _pipeline_for(cfg, 64, 5)
    b = O.batch_to_torch(O.synthetic_batch(333, 24, seed=15))
    rays, extras, u = b["rays"].to(DEV), b["extras"].to(DEV), b["u"].to(DEV)
    ro = {"perturb_rand": u}
    ora = O.render_rays(O.to_torch(params), torch.from_numpy(O.init_embedding_numpy(cfg, 5)), cfg, b["rays"], b["extras"], b["u"])
    ora.pop("_z_vals")
    keys = tuple(ora)

    def run(fill):
        _poison(monkeypatch, fill)
        bi = batched_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, render_options=ro)
        lean = lean_inference(pipe.cfgs, pipe.renderer, pipe.models, rays, extras, keys=keys, render_options=ro)
        res = {"batched_" + k: v for k, v in bi.items()}
        res.update({"lean_" + k: lean[k] for k in keys})
        return res

    r = run_filled(run)[0xFF]
    assert {k[8:] for k in r if k.startswith("batched_")} == set(ora)
    for k, v in ora.items():
        assert torch.equal(r["lean_" + k], r["batched_" + k]), k
        if k == "semantic_label_coarse":
            top2 = ora["semantic_logits_coarse"].topk(2, dim=-1).values
            sure = (top2[:, 0] - top2[:, 1]) > 2 * OUT_TOL
            assert torch.equal(r["batched_" + k].cpu()[sure], v[sure])
        else:
            _finite_where(r["batched_" + k], v, k)
            assert max_abs(r["batched_" + k].cpu(), v) <= OUT_TOL, (k, max_abs(r["batched_" + k].cpu(), v))


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: f"0x{f:02X}")
def test_reused_workspace_gives_the_first_steps_bits(fill, monkeypatch):
    """Training reuses its leased workspaces step after step.  With the parameters reset, step 2 (the lease of step 1, refilled by
    lease_workspace) and step 3 (the switch off: the lease holds step 2's planes, exponents, counters and partial sums as they
    were left -- what a training run really hands a pass) must both give step 1 bit for bit."""
    from snerf_amd import ops
    z, meta, cfg = load_fixture("sem_siren_small")
    pn = fixture_params(z, meta, cfg)
    b = fixture_batch(z)
    emb = torch.from_numpy(O.init_embedding_numpy(cfg, meta["seed"]))
    _poison(monkeypatch, fill)
    first = _train_pass(cfg, pn, b, emb, None, meta["epoch"])
    def leases():
        return {k: sorted(t.data_ptr() for t in v) for k, v in ops._WS_FREE.items()}

    idle = leases()
    assert idle, "the pass leased no workspace"
    second = _train_pass(cfg, pn, b, emb, None, meta["epoch"])
    assert leases() == idle, "step 2 did not reuse step 1's workspaces"
    _assert_same(first, second, "step 2 on refilled leases")
    monkeypatch.setattr(ops, "_WS_POISON", False)
    third = _train_pass(cfg, pn, b, emb, None, meta["epoch"])
    assert leases() == idle
    _assert_same(first, third, "step 3 on the leftovers of step 2")
    for k in z.files:
        if k.startswith("grad_"):
            _check_grad(k, third[k], z[k])


@pytest.mark.parametrize("C_", (5, 64))
@pytest.mark.parametrize("N,S", [(77, 16), (77, 100), (513, 64)])
def test_fused_loss(N, S, C_, monkeypatch):
    """values and every gradient of every loss module against the oracle, at the bars test_gpu_pipeline._loss_modules_vs_oracle
    asserts itself (it runs under every fill); workspace, totals, terms and the gradient buffers carry the fill"""
    from tests.test_gpu_pipeline import _loss_modules_vs_oracle

    def run(fill):
        _poison(monkeypatch, fill)
        got = {}
        _loss_modules_vs_oracle(N, S, C_, collect=got)
        return got

    r = run_filled(run)[0xFF]
    assert len(r) > 30 and all(bool(torch.isfinite(v).all()) for v in r.values())


@pytest.mark.parametrize("N,S,sem,C_", [(77, 16, "plain", 64), (513, 64, "uncertainty_sbeta", 5)])
def test_merged_loss_call(N, S, sem, C_, monkeypatch):
    """colour + semantic + L_t as ONE fused call (loss_ops.run_plans), the configuration a training step really allocates for: under
    every fill, at the bars test_gpu_pipeline._merged_loss_call_equals_module_by_module asserts itself against the modules one by one
    (which test_fused_loss holds to the oracle)"""
    from tests.test_gpu_pipeline import _merged_loss_call_equals_module_by_module

    def run(fill):
        _poison(monkeypatch, fill)
        got = {}
        _merged_loss_call_equals_module_by_module(N, S, sem, C_, collect=got)
        return got

    r = run_filled(run)[0xFF]
    assert len(r) > 8 and all(bool(torch.isfinite(v).all()) for v in r.values())


# ==============================================================================================================================
# Part B: the other entries, on buffers the test owns
# ==============================================================================================================================
@pytest.mark.parametrize("jitter", (False, True), ids=("u-none", "u-given"))
def test_sample_z(jitter, monkeypatch):
    from snerf_amd import _lib, ops
    from tests.test_gpu_call import _inputs, N, S
    rays, steps, u = _inputs()
    u = u if jitter else None
    want = ops.sample_z(rays, steps, u)
    # and independently of the kernel: the oracle's sampler on the CPU, which the render pass's depths equal bit for bit
    # (test_gpu_kernels.test_forward_matches_oracle_and_golden)
    _, want_cpu = O.sample_rays(rays.cpu(), S, u.cpu() if u is not None else None)

    def run(fill):
        z = _filled((N, S), torch.float32, fill)
        _lib.call("snerf_sample_z", rays, steps, u, z, N, S)
        _poison(monkeypatch, fill)
        return {"z": z, "ops": ops.sample_z(rays, steps, u)}

    r = run_filled(run)[0xFF]
    for k in ("z", "ops"):      # the bar of test_gpu_call.test_call_equals_the_module_function
        assert torch.equal(r[k].view(torch.int32), want.view(torch.int32))
        assert torch.equal(r[k].cpu().view(torch.int32), want_cpu.view(torch.int32))
        assert bool(torch.isfinite(r[k]).all()) and bool((r[k][:, 1:] > r[k][:, :-1]).all())


@pytest.mark.parametrize("vocab", [50, 96])
def test_embedding_rows(vocab, monkeypatch):
    from snerf_amd import _lib, ops
    torch.manual_seed(7)
    emb = torch.nn.Embedding(vocab, 4).to(DEV)
    idx = torch.randint(0, vocab, (4099,), device=DEV)
    idx[:7] = vocab - 1
    table = emb.weight.detach().contiguous()
    want = table[idx]

    def run(fill):
        rows = _filled((4099, 4), torch.float32, fill)
        _lib.call("snerf_embedding_rows", table, vocab, 4, idx, 4099, rows)
        _poison(monkeypatch, fill)
        return {"rows": rows, "ops": ops.embed_rows(emb, idx).detach()}

    r = run_filled(run)[0xFF]
    assert torch.equal(r["rows"], want) and torch.equal(r["ops"], want)     # test_gpu_rows.test_embedding_rows_forward_backward


def test_adam_step_between_filled_neighbours():
    """no workspace and no pure output: the step runs on slices of one filled arena and must leave the bytes beside them alone.
    Bar: test_gpu_optim_ckpt.test_fused_adam_matches_torch_adam (rtol 2e-6, atol 1e-7 against torch.optim.Adam on the CPU)."""
    from snerf_amd import _lib
    g = torch.Generator().manual_seed(3)
    n, gap = 8164, 64          # the present test's ragged shapes hold 8163 values; n must be a multiple of 4
    p0 = torch.randn(n, generator=g)
    gr = [torch.randn(n, generator=g) * s for s in (1e-3, 1.0)]
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([ref_p], lr=5e-4, weight_decay=0)
    for x in gr:
        ref_p.grad = x.clone()
        ref.step()

    def run(fill):
        arena = _filled((4 * (n + gap) + gap,), torch.float32, fill)
        at = [gap + k * (n + gap) for k in range(4)]
        p, gd, m, v = (arena[a:a + n] for a in at)
        p.copy_(p0)
        m.zero_()
        v.zero_()
        for step, x in enumerate(gr, 1):
            gd.copy_(x)
            _lib.call("snerf_adam_step", p, gd, m, v, n, 5e-4, 0.9, 0.999, 1e-8, step, 1.0)
        for a in [0] + [x + n for x in at]:
            assert _is_fill(arena[a:a + gap], fill), "the step wrote beside its buffers"
        return {"p": p.clone(), "m": m.clone(), "v": v.clone()}

    r = run_filled(run)[0xFF]
    assert torch.allclose(ref_p.detach(), r["p"].cpu(), rtol=2e-6, atol=1e-7)


def _synthetic_rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    rays = torch.randn(n, 8, generator=g)
    rays[:, :3] = rays[:, :3] * 300.0 + torch.tensor([7.0e5, -5.4e6, 3.2e6])
    rays[:, 3:6] = torch.nn.functional.normalize(rays[:, 3:6], dim=1)
    rays[:, 6] = 0.0
    rays[:, 7] = 50.0 + 10.0 * torch.rand(n, generator=g)
    return rays.float().contiguous()


@pytest.mark.parametrize("sizes", [(1, 300), (263000,)], ids=("1+300", "263000"))
def test_ray_bounds_and_normalize_rows(sizes):
    """two small arrays, and one above the 1024 x 256 grid-stride cap: the stride loop and all 1024 partial slots of the workspace.
    Reference and bar: the torch-CPU min / max of test_gpu_scene.test_normalisation_parameters (exact); the normalised rows at
    test_gpu_scene.assert_rays_match against torch's correctly rounded fp32 (o - c) / range."""
    from snerf_amd import _lib
    from tests.test_gpu_scene import assert_rays_match
    host = [_synthetic_rays(n, 11 + n) for n in sizes]
    dev = [t.to(DEV) for t in host]
    cat = torch.cat(host)
    far = cat[:, :3] + cat[:, 7:8] * cat[:, 3:6]
    pts = torch.cat([cat[:, :3], far]).numpy()
    mn, mx = pts.min(0), pts.max(0)
    scale = (mx - mn) / np.float32(2)
    n_rows = (C.c_longlong * len(dev))(*[int(t.shape[0]) for t in dev])
    ptrs = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    nbytes = _lib.call_size("snerf_ray_bounds_workspace_bytes", n_rows, len(dev))

    def run(fill):
        ws, out = _filled((nbytes,), torch.uint8, fill), _filled((13,), torch.float32, fill)
        _lib.call("snerf_ray_bounds", ptrs, n_rows, len(dev), out, ws, nbytes)
        rows = _filled((dev[0].shape[0], 9), torch.float32, fill)       # stride 9: the ninth column is not the library's
        rows[:, :8] = dev[0]
        _lib.call("snerf_normalize_rows", rows, rows.shape[0], 9, 1, out[9:13].clone())
        assert _is_fill(rows[:, 8], fill), "normalize_rows wrote beside its columns"
        return {"bounds": out, "rows": rows[:, :8].contiguous()}

    r = run_filled(run)[0xFF]
    bnd = r["bounds"].cpu().numpy()
    np.testing.assert_array_equal(bnd[0:3], mn)
    np.testing.assert_array_equal(bnd[3:6], mx)
    np.testing.assert_array_equal(bnd[6:9], scale)
    np.testing.assert_array_equal(bnd[9:12], mn + scale)
    assert bnd[12] == scale.max()
    c, rng = torch.from_numpy(bnd[9:12]), torch.tensor(bnd[12])
    want = host[0].clone()
    want[:, :3] = (want[:, :3] - c) / rng
    want[:, 6:8] = want[:, 6:8] / rng
    assert_rays_match(r["rows"].cpu().numpy(), want.numpy())


def _scene_meta(name):
    with open(os.path.join(GOLDEN, "scene_small", "metas", name)) as f:
        return json.load(f)


RPC_IMAGES = (("JAX_068_009_RGB.json", (5, 3)), ("JAX_068_013_RGB.json", (7, 2)))      # with / without the inverse polynomials


def test_rpc_rays():
    """both images in one launch, on 5 x 3 and 7 x 2 pixel grids; counters are the caller's zeroed accumulators (they hold the
    update count the second launch loops to).  Reference: tests/rpc_numpy.py through test_scene_cpu.numpy_rays, at the ulp bar of
    test_gpu_scene.assert_rays_match."""
    from snerf_amd import _lib
    from snerf_amd.baseline.components.camera_models import rpc_struct, struct_to_device
    from tests.test_gpu_scene import assert_rays_match
    from tests.test_scene_cpu import numpy_rays
    metas = [_scene_meta(n) for n, _ in RPC_IMAGES]
    assert "lat_num" in metas[0]["rpc"] and "lat_num" not in metas[1]["rpc"]
    table = (_lib.SnerfRayImage * 2)()
    row0, want = 0, []
    for k, (m, (_, (w, h))) in enumerate(zip(metas, RPC_IMAGES)):
        e = table[k]
        e.rpc = rpc_struct(m["rpc"])
        e.min_alt, e.max_alt, e.w, e.h, e.row0, e.n_rays = float(m["min_alt"]), float(m["max_alt"]), w, h, row0, w * h
        row0 += w * h
        cols, rows = np.meshgrid(np.arange(w), np.arange(h))
        want.append(numpy_rays(m, cols, rows))
    want = np.concatenate(want)
    table_dev = struct_to_device(table, DEV)

    def run(fill):
        rays = _filled((row0, 8), torch.float32, fill)
        counters = torch.zeros(6, dtype=torch.int32, device=DEV)
        _lib.call("snerf_rpc_rays", table, table_dev, 2, None, row0, rays, counters)
        return {"rays": rays, "counters": counters}

    r = run_filled(run)[0xFF]
    assert r["counters"][:2].tolist() == [0, 0]
    _finite_where(r["rays"], want, "rays")
    assert_rays_match(r["rays"].cpu().numpy(), want)


@pytest.mark.parametrize("image", RPC_IMAGES, ids=("inverse", "iterative"))
def test_rpc_localize_project_reproject(image):
    """bars of test_gpu_scene.test_localisation_and_projection_against_numpy: normalised lon / lat within 1e-12 of rpc_numpy, the
    projection of the localisation within 1e-6 px of the pixel.  Reprojection: ECEF points of geo_cloud_small, whose geodetic
    coordinates the reference's own ecef_to_latlon_custom wrote into the fixture; their rpc_numpy projection at the same 1e-6 px"""
    from snerf_amd import _lib
    from snerf_amd.baseline.components.camera_models import rpc_struct, struct_to_device
    from tests import rpc_numpy
    name, (w, h) = image
    m = _scene_meta(name)
    cam = rpc_numpy.RPCModel(m["rpc"])
    s = rpc_struct(m["rpc"])
    s_dev = struct_to_device(s, DEV)
    cols, rows = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    cols, rows = cols.ravel(), rows.ravel()
    n = cols.size
    alts = np.linspace(m["min_alt"], m["max_alt"], n)
    want_n = cam.localization(cols, rows, alts, return_normalized=True)
    lon, lat = cam.localization(cols, rows, alts)
    fx = np.load(os.path.join(GOLDEN, "geo_cloud_small.npz"))
    ecef = np.ascontiguousarray(fx["ecef"][:n])
    want_cr = np.stack(cam.projection(fx["lon"][:n], fx["lat"][:n], fx["alt"][:n]), 1)
    assert np.isfinite(want_cr).all()
    pts2d = want_cr + 0.25
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in
         (("col", cols), ("row", rows), ("alt", alts), ("lon", lon), ("lat", lat), ("ecef", ecef), ("pts2d", pts2d))}

    def run(fill):
        o = {k: _filled((n,), torch.float64, fill) for k in ("lon_n", "lat_n", "lon", "lat", "col", "row", "err")}
        o["col_row"] = _filled((n, 2), torch.float64, fill)
        for norm, a, b in ((1, "lon_n", "lat_n"), (0, "lon", "lat")):
            counters = torch.zeros(2, dtype=torch.int32, device=DEV)
            _lib.call("snerf_rpc_localize", s, s_dev, d["col"], d["row"], d["alt"], n, norm, o[a], o[b], counters)
            o["counters_" + a] = counters
        _lib.call("snerf_rpc_project", s, s_dev, o["lon"], o["lat"], d["alt"], n, o["col"], o["row"])
        _lib.call("snerf_rpc_reprojection_error", s, s_dev, d["ecef"], d["pts2d"], n, o["col_row"], o["err"])
        return o

    r = {k: v.cpu().numpy() for k, v in run_filled(run)[0xFF].items()}
    assert r["counters_lon"][0] == 0 and r["counters_lon_n"][0] == 0
    assert all(np.isfinite(v).all() for v in r.values())
    assert np.abs(r["lon_n"] - want_n[0]).max() <= 1e-12 and np.abs(r["lat_n"] - want_n[1]).max() <= 1e-12
    assert np.abs(r["col"] - cols).max() <= 1e-6 and np.abs(r["row"] - rows).max() <= 1e-6
    print("reprojection: max |col_row - rpc_numpy| =", float(np.abs(r["col_row"] - want_cr).max()))
    assert np.abs(r["col_row"] - want_cr).max() <= 1e-6
    assert np.abs(r["err"] - np.hypot(pts2d[:, 0] - r["col_row"][:, 0], pts2d[:, 1] - r["col_row"][:, 1])).max() <= 1e-12


@pytest.mark.parametrize("ws", (3, 11))
@pytest.mark.parametrize("name", ("ssim_inria_37x53", "ssim_inria_11"))
def test_ssim(name, ws):
    """bar and reference of test_gpu_ssim.test_ssim_inria_vs_reference_fixtures (MEAN_TOL on the reference's fp64 means); the map
    is asked for too, so that its every element is held to (a) and (b)"""
    from snerf_amd import _lib
    from tests.test_gpu_ssim import MEAN_TOL, _M
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    x, y = torch.from_numpy(z["x"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    b, c, h, w = x.shape
    k2 = _M()._window("inria", ws, torch.device(DEV))
    nbytes = _lib.call_size("snerf_ssim_workspace_bytes", b, c, h, w, ws)

    def run(fill):
        work, sums, smap = _filled((nbytes,), torch.uint8, fill), _filled((b,), torch.float64, fill), _filled(x.shape, torch.float32, fill)
        _lib.call("snerf_ssim", x, y, b, c, h, w, ws, _lib.SSIM_ZERO, k2, 0.01 ** 2, 0.03 ** 2, 0.0, smap, sums, work, nbytes)
        return {"sums": sums, "map": smap}

    r = run_filled(run)[0xFF]
    assert bool(torch.isfinite(r["map"]).all()) and bool(torch.isfinite(r["sums"]).all())
    f64, f32 = z[f"f64_ws{ws}"], z[f"f32_ws{ws}"].astype(np.float64)
    per_image = r["sums"].cpu().numpy() / (c * h * w)
    got = (per_image.mean() if bool(z["size_average"]) else per_image).astype(np.float32).astype(np.float64)
    assert np.abs(got - f64).max() <= MEAN_TOL
    assert np.all(np.abs(got - f32) <= np.abs(f32 - f64) + MEAN_TOL)
    # the map's own sum is the per-image sum to fp32 rounding of its elements
    assert np.abs(r["map"].double().sum((1, 2, 3)).cpu().numpy() / (c * h * w) - per_image).max() <= MEAN_TOL


@pytest.mark.parametrize("name", ("dsmr_odd", "dsmr_holes_water"))
def test_dsm_registration_entries(name):
    """downsample2x, ncc_search and shift_diff on the reference's registration fixtures.  Bars of
    test_gpu_dsm.test_registration_and_mae_vs_reference_golden: the pyramid level exact, the level's best shift equal to the
    numpy restatement's, b within 1e-9 relative, rdsm within 1 ulp of the reference's with the same NaNs, the mean within 1e-6."""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import dsm as D
    from tests import dsm_numpy as N
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    gt, v, pred = (torch.from_numpy(z[k]).to(DEV).contiguous() for k in ("gt", "v", "pred"))
    assert gt.dtype == torch.float32 and v.dtype == torch.float32
    h, w = gt.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    cx, cy = (int(t) for t in z["init"])
    dx, dy, b = int(z["dx"]), int(z["dy"]), float(z["b"])
    rad = D.IRANGE
    S = (2 * rad + 1) ** 2
    nb_ncc = _lib.call_size("snerf_dsm_workspace_bytes", h, w, rad)
    nb_diff = _lib.call_size("snerf_dsm_workspace_bytes", h, w, 0)

    def run(fill):
        o = {"ds_u": _filled((h2, w2), torch.float64, fill), "ds_v": _filled((h2, w2), torch.float64, fill),
             "ncc": _filled((S, 6), torch.float64, fill), "at": _filled((1, 6), torch.float64, fill),
             "rdsm": _filled((h, w), torch.float32, fill), "diff": _filled((h, w), torch.float32, fill),
             "totals": _filled((2,), torch.float64, fill), "totals_only": _filled((2,), torch.float64, fill)}
        _lib.call("snerf_dsm_downsample2x", gt, 0, h, w, o["ds_u"])
        _lib.call("snerf_dsm_downsample2x", v, 0, h, w, o["ds_v"])
        ws = _filled((nb_ncc,), torch.uint8, fill)
        _lib.call("snerf_dsm_ncc_search", gt, v, 0, h, w, cx, cy, rad, o["ncc"], ws, nb_ncc)
        ws0 = _filled((nb_diff,), torch.uint8, fill)
        _lib.call("snerf_dsm_ncc_search", gt, v, 0, h, w, dx, dy, 0, o["at"], ws0, nb_diff)
        _lib.call("snerf_dsm_shift_diff", v, gt, h, w, dx, dy, b, o["rdsm"], o["diff"], o["totals"], ws0, nb_diff)
        _lib.call("snerf_dsm_shift_diff", v, gt, h, w, dx, dy, b, None, None, o["totals_only"], ws0, nb_diff)
        return o

    r = {k: t.cpu().numpy() for k, t in run_filled(run)[0xFF].items()}
    assert np.array_equal(r["ds_u"], N.downsample2x(z["gt"]), equal_nan=True)
    assert np.array_equal(r["ds_v"], N.downsample2x(z["v"]), equal_nan=True)
    if int(z["n_levels"]) >= 1:
        assert np.array_equal(r["ds_u"], z["ds_u_1"], equal_nan=True) and np.array_equal(r["ds_v"], z["ds_v_1"], equal_nan=True)
    assert np.isfinite(r["ncc"]).all() and np.isfinite(r["at"]).all() and np.isfinite(r["totals"]).all()
    best, at = -math.inf, None
    for s_, row in enumerate(r["ncc"].tolist()):
        c = D._ncc(row)
        if c > best:
            best, at = c, (cx - rad + s_ % (2 * rad + 1), cy - rad + s_ // (2 * rad + 1))
    assert at == N.compute_ncc(z["gt"], z["v"], rad, cx, cy)
    count, su, sv = r["at"][0][:3]
    muu, muv = N.mean_std(z["gt"], z["v"], dx, dy)[:2]
    assert abs((su / count - sv / count) - (muu - muv)) <= 1e-9 * abs(muu - muv)
    want = (N._shifted(z["v"].astype(np.float64), dx, dy) + b).astype(np.float32)
    assert np.array_equal(np.isnan(r["rdsm"]), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.all(np.abs(r["rdsm"][fin] - want[fin]) <= np.spacing(np.abs(want[fin])))
    assert torch.equal(D.apply_shift(v, dx, dy, 1, b).cpu().view(torch.int32), torch.from_numpy(r["rdsm"]).view(torch.int32))
    g = np.where(z["gt"] < -500, np.float32(0), z["gt"])
    dref = np.abs((want - g).astype(np.float64))
    ok = np.isfinite(dref)
    assert np.array_equal(np.isfinite(r["diff"]), ok)
    assert r["totals"][1] == ok.sum() and abs(r["totals"][0] - dref[ok].sum()) <= 1e-6 * dref[ok].sum()
    assert np.array_equal(r["totals"], r["totals_only"])


def test_dsm_finish():
    """snerf_dsm_finish on the integer accumulators of a rasterised cloud (count / sum / stats are the caller's zeroed accumulators
    and are never filled): reference and bar of test_gpu_dsm.test_rasterize_matches_numpy"""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import dsm as D
    from tests import dsm_numpy as N
    from tests.test_gpu_dsm import _cloud
    res = 0.5
    grid = D.DsmGrid(1000.0, 2000.0 + 37 * res, res, 41, 37)
    cloud = _cloud(150, 41, 37, res, 300.0, 20.0, seed=1)       # sparse: cells without a point stay NaN
    want, cnt = N.rasterize(cloud, *grid, radius=1)
    c = torch.from_numpy(cloud).to(DEV)
    count, total, stats0 = D._accumulate(c, grid, (0, 0, grid.xsize, grid.ysize), 1)
    assert np.array_equal(count.cpu().numpy().reshape(37, 41), cnt) and (cnt == 0).any()

    def run(fill):
        dsm, stats = _filled((37 * 41,), torch.float32, fill), stats0.clone()
        _lib.call("snerf_dsm_finish", count, total, 37 * 41, D.Z0, D.Q, dsm, stats)
        return {"dsm": dsm, "stats": stats}

    r = run_filled(run)[0xFF]
    got = r["dsm"].cpu().numpy().reshape(37, 41)
    assert np.array_equal(np.isnan(got), cnt == 0)
    ok = cnt > 0
    assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= float(np.spacing(np.float32(np.abs(cloud[:, 2]).max())))
    assert int(r["stats"][2]) == int(cnt.max())


@pytest.mark.parametrize("name", ("semeval_metrics_c5", "semeval_metrics_c16"))
def test_semeval_accumulate(name):
    """the fp64 partials of the uncertainty sum live in the workspace; the accumulator block is the caller's zeroed one.  Bars of
    test_gpu_semeval.test_metric_fixtures_through_the_kernel: counts and metrics exact, the beta sum within 1e-12 relative."""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import semantic as S_
    from tests import semeval_ref as R
    from tests.test_semeval_cpu import _load
    z = _load(name)
    Cn, car = int(z["n_classes"]), int(z["car_idx"])
    t = {k: torch.from_numpy(z[k]).to(DEV) for k in ("pred", "gt", "gt_no_cars", "weights", "beta")}
    n, S = t["weights"].shape
    nbytes = _lib.call_size("snerf_semeval_workspace_bytes", n, S)
    keep = {}

    def run(fill):
        acc = S_.SemanticEvalAccumulator(Cn, car, DEV)
        acc._work = _filled((nbytes // 8 + 16,), torch.float64, fill)        # the accumulator takes a workspace that is large enough
        work = acc._work
        acc.add(t["pred"], t["gt"], t["gt_no_cars"], t["gt"], weights=t["weights"], beta=t["beta"])
        assert acc._work is work
        keep[fill] = acc
        return {"acc": acc.buf.clone()}

    run_filled(run)
    acc = keep[0xFF]
    e = acc.image_entry()
    assert e["semantic_accuracy"] == float(z["acc"]) and e["semantic_accuracy_wo_cars"] == float(z["acc_no_cars"])
    assert e["semantic_accuracy_comparison_non_corrupted_wo_cars"] == float(z["acc_filter"])
    assert np.array_equal(np.array(e["confusion_matrix"], np.float32).view(np.uint32), z["cm"].view(np.uint32))
    m = float(z["miou"])
    assert (math.isnan(m) and math.isnan(e["mIoU"])) or e["mIoU"] == m
    st = R.stats(z["pred"], z["gt"], Cn, car, weights=z["weights"], beta=z["beta"])
    got = acc._read()["beta_car_sum"]
    assert math.isfinite(got) and abs(got - st["beta_car_sum"]) <= 1e-12 * abs(st["beta_car_sum"])
    u = float(z["unc"])
    if not math.isnan(u):
        assert abs(e["uncertainty_at_transient"] - u) <= 1e-5 * abs(u)


def test_vis_fold():
    """every plane of the frame is the test's and carries the fill; the stats block is the caller's zeroed accumulator.  Folded in
    two ragged chunks.  Bars of test_gpu_vis.test_fold_against_reference_fixtures (test_vis_cpu.check_maps_against_fixture)."""
    from snerf_amd.eval.utils import vismaps as V
    from tests.test_gpu_vis import OUTS, _inputs, _want_bounds
    from tests.test_vis_cpu import check_maps_against_fixture, load
    z = load("vis_5x7_s3")
    c = _inputs(z)
    n, S = c["weights"].shape
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in c.items()}

    def run(fill):
        planes = {}
        for p, field in OUTS.items():
            bands = 3 if p in ("albedo", "sky", "rgb_diff", "sem_color", "sem_shaded") else 1
            dt = torch.uint8 if p in ("sem_color", "sem_shaded") else torch.float32
            planes[field] = _filled((bands, n) if bands > 1 else (n,), dt, fill)
        stats = V.new_stats(DEV)
        for i, k in ((0, 13), (13, n - 13)):
            V.fold_chunk(planes, stats, i, n, k, S, **{key: (t if key == "palette" else t[i:i + k]) for key, t in d.items()})
        return dict(planes, stats=stats)

    r = run_filled(run)[0xFF]
    got = {p: r[field].cpu().numpy() for p, field in OUTS.items()}
    assert all(np.isfinite(g).all() for g in got.values())
    check_maps_against_fixture(z, got)
    assert np.array_equal(got["depth"], z["depth"])
    st = V.decode_stats(r["stats"].cpu().numpy())
    assert st["bad_labels"] == 0
    for k, wnt in _want_bounds(got).items():
        assert st["bounds"][k] == wnt, k


def test_vis_minmax_and_colormap():
    """snerf_vis_minmax folds into a zeroed block; snerf_vis_colormap writes a filled (3, n) output from the slot's bounds and from
    explicit ones.  Planes of vis_5x7_s3 and the NaN / zero / constant planes of vis_nan_const, fp32 and fp64: the indices of
    test_gpu_vis.test_colormap_indices_and_stats, exact."""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import vismaps as V
    from tests.test_gpu_vis import _identity
    from tests.test_vis_cpu import CMAPS, load
    tab = _identity()
    z = load("vis_5x7_s3")
    cases = [(k, z[f"cmap_{k}"], z[f"idx_{k}"], z[f"bounds_{k}"], z[f"idxb_{k}"]) for k in CMAPS]
    z = load("vis_nan_const")
    for dt in ("float32", "float64"):
        cases += [(f"nan_{dt}", z[f"cmap_nan_{dt}"], z[f"idx_nan_{dt}"], None, None),
                  (f"zero_{dt}", z[f"cmap_zero_{dt}"], z[f"idx_zero_{dt}"], None, None),
                  (f"const_{dt}", z[f"cmap_const_{dt}"], z[f"idx_const_{dt}"], z[f"bounds_const_{dt}"], z[f"idxb_const_{dt}"])]
    slot = _lib.VIS_SLOT["user"]

    def run(fill):
        o = {}
        for what, plane, _, bounds, _ in cases:
            p = torch.from_numpy(np.ascontiguousarray(plane)).to(DEV).reshape(-1)
            dt = _lib.VIS_F32 if p.dtype == torch.float32 else _lib.VIS_F64
            stats = V.new_stats(DEV)
            _lib.call("snerf_vis_minmax", p, dt, p.numel(), stats, slot)
            o[what] = _filled((3, p.numel()), torch.uint8, fill)
            _lib.call("snerf_vis_colormap", p, dt, p.numel(), stats, slot, 0.0, 0.0, tab, o[what])
            o[what + "/stats"] = stats
            if bounds is not None:
                o[what + "/b"] = _filled((3, p.numel()), torch.uint8, fill)
                _lib.call("snerf_vis_colormap", p, dt, p.numel(), None, -1, float(bounds[0]), float(bounds[1]), tab, o[what + "/b"],
                          device=p.device)
        return o

    r = run_filled(run)[0xFF]
    for what, plane, idx, bounds, idxb in cases:
        out = r[what].cpu().numpy()
        assert (out[0] == out[1]).all() and (out[0] == out[2]).all() and np.array_equal(out[0], idx.reshape(-1)), what
        if bounds is not None:
            assert np.array_equal(r[what + "/b"].cpu().numpy()[0], idxb.reshape(-1)), what
        n2n = torch.nan_to_num(torch.from_numpy(np.ascontiguousarray(plane)))
        lo, hi = V.decode_stats(r[what + "/stats"].cpu().numpy())["bounds"]["user"]
        assert lo == float(torch.amin(n2n)) and hi == float(torch.amax(n2n)), what


@pytest.mark.parametrize("entry", ("cloud", "points"))
def test_geo_cloud_and_points(entry):
    """the first 1,000 rows of geo_cloud_small; enu / lla carry the fill, the stats words are the caller's {~0, 0, ~0, 0, 0...}.
    Bars of test_gpu_geo.test_stage_parity_with_the_reference: lat / lon 1e-12 deg, alt / east / north 1e-6 m."""
    from snerf_amd import _lib
    from snerf_amd.baseline.components.normalization import StandardNormalization
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    from tests.test_gpu_geo import KEYS, _torch_bounds
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    fx = np.load(os.path.join(GOLDEN, "geo_cloud_small.npz"))
    n = 1000
    frame = GeoFrame(StandardNormalization().set_params(dict(zip(KEYS, fx["norm_params"].tolist()))), str(fx["zone_string"]))
    rays, depth, xyz_n = (torch.from_numpy(fx[k][:n]).to(DEV).contiguous() for k in ("rays", "depth", "xyz_n"))

    def run(fill):
        enu, lla = _filled((n, 3), torch.float64, fill), _filled((n, 3), torch.float64, fill)
        enu_only = _filled((n, 3), torch.float64, fill)
        stats = torch.tensor([-1, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int64, device=DEV)
        stats2 = stats.clone()
        if entry == "cloud":
            _lib.call("snerf_geo_cloud", rays, rays.shape[1], depth, n, frame.params, enu, lla, stats)
            _lib.call("snerf_geo_cloud", rays, rays.shape[1], depth, n, frame.params, enu_only, None, stats2)
        else:
            _lib.call("snerf_geo_points", xyz_n, n, frame.params, enu, lla, stats)
            _lib.call("snerf_geo_points", xyz_n, n, frame.params, enu_only, None, stats2)
        return {"enu": enu, "lla": lla, "enu_only": enu_only, "stats": stats, "stats2": stats2}

    r = run_filled(run)[0xFF]
    assert torch.equal(r["enu"].view(torch.int64), r["enu_only"].view(torch.int64)) and torch.equal(r["stats"], r["stats2"])
    enu, lla = r["enu"].cpu().numpy(), r["lla"].cpu().numpy()
    assert np.isfinite(enu).all() and np.isfinite(lla).all()
    assert np.abs(lla[:, 0] - fx["lat"][:n]).max() <= 1e-12 and np.abs(lla[:, 1] - fx["lon"][:n]).max() <= 1e-12
    assert np.abs(lla[:, 2] - fx["alt"][:n]).max() <= 1e-6
    assert np.abs(enu[:, 0] - fx["east_restated"][:n]).max() <= 1e-6 and np.abs(enu[:, 1] - fx["north_restated"][:n]).max() <= 1e-6
    assert np.array_equal(enu[:, 2], lla[:, 2])
    words = [int(x) & (2 ** 64 - 1) for x in r["stats"].cpu().tolist()]
    bounds, bad = decode_geo_stats(words)
    assert bad == 0 and bounds == _torch_bounds(r["enu"])
