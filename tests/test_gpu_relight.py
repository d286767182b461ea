"""The relight pass (SNERF_FLAG_RELIGHT, ops.relight_pass_into) on the device (run with -m gpu on an MI355X).

The bar everywhere is BIT EQUALITY: a relight runs the full pass's own kernels on operands that must be bit-identical, so any
differing bit is a defect, not a tolerance question.  Reference side: render_pass_into under sun B on a fresh workspace.  Test side:
render_pass_into under sun A, then relight_pass_into under sun B on that workspace.  Compared: every key of output_keys(spec, False)
plus semantic_label and z_vals, with one jitter tensor shared by both sides.

Shapes are the smallest at which the new code can go wrong: narrow ReLU nets (Wf > W: the pad columns exist; one partial row
block; three row blocks and a tail of 3), the product shape in both arithmetics (composed plan with every fold; fused trunk), and
feat_last = 512 (the non-composed plan, two-tile nd_sun, no nd_fin)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import test_gpu_kernels as K
from tests.test_gpu_fill import _poison, run_filled
from tests.test_gpu_nadir import H, OPTS, T, W, _args, _same, scene, truth      # noqa: F401  (scene, truth: fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RELU = dict(fc_units=64, fc_layers=3, fc_skips=(), activation_function="relu", t_embedding_tau=4)
NETS = {
    "relu-c0": O.OracleCfg(n_classes=0, **RELU),
    "relu-c5-sbeta-ts": O.OracleCfg(n_classes=5, use_separate_beta_for_s=True, use_separate_tj_for_semantic=True, **RELU),
    "product": O.OracleCfg(),
    "feat512": O.OracleCfg(fc_use_full_features=True),
}
_PARAMS = {}


def _unit(n, seed):
    """a different unit sun per ray"""
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(DEV).contiguous()


class Case:
    """one model, one ray batch, one jitter tensor; full(sun) and relight(sun, ws) fill fresh result tensors"""

    def __init__(self, net, N, S, mode="f16x2", t_scale=1.0):
        from snerf_amd import ops
        cfg = NETS[net]
        self.spec = dataclasses.replace(K._spec(cfg), mfma=mode)
        if net not in _PARAMS:      # one set of parameters per net, shared by its cases
            _PARAMS[net] = K._gpu_params(O.init_params_numpy(cfg, 11), torch.device(DEV))
        self.gp = _PARAMS[net]
        self.packed = ops.pack_params(self.spec, self.gp)
        self.N, self.S = N, S
        b = O.batch_to_torch(O.synthetic_batch(N, S, seed=N + S))
        self.rays, self.u = b["rays"].to(DEV), b["u"].to(DEV)
        self.zs = torch.linspace(0, 1, S).to(DEV)
        g = torch.Generator().manual_seed(5)
        self.t = (torch.randn(N, cfg.t_embedding_tau, generator=g) * t_scale).to(DEV)
        self.t_s = (torch.randn(N, cfg.t_embedding_tau, generator=g) * t_scale).to(DEV) if self.spec.use_separate_tj_for_semantic else None
        self.keys = tuple(ops.output_keys(self.spec, False)) + (("semantic_label",) if self.spec.n_classes else ()) + ("z_vals",)

    def buffers(self, keys=None):
        from snerf_amd import ops
        out = {}
        for k in keys or self.keys:
            shape = (self.N,) if k == "semantic_label" else (self.N, self.S) if k == "z_vals" else ops._OUT_SHAPES[k](self.N, self.S, self.spec.n_classes)
            out[k] = ops._empty(shape, dtype=torch.int64 if k == "semantic_label" else torch.float32, device=DEV)
        return out

    def pin(self, sun, **kw):
        from snerf_amd import ops
        return ops.PassInputs(sun_d=sun, rays=self.rays, z_steps=self.zs, u=self.u, **kw)

    def full(self, sun, keys=None, ws=None):
        from snerf_amd import ops
        out = self.buffers(keys)
        ws = ops.render_pass_into(self.spec, self.gp, self.pin(sun), self.t, self.t_s, out, packed=self.packed, workspace=ws)
        return out, ws

    def relight(self, sun, ws, keys=None, n_samples=None):
        from snerf_amd import ops
        out = self.buffers(keys)
        got = ops.relight_pass_into(self.spec, self.gp, sun, self.t, self.t_s, out, ws, packed=self.packed,
                                    n_samples=self.S if n_samples is None else n_samples)
        assert got is ws
        return out


def _assert_bits(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        same = got[k].contiguous().view(torch.uint8) == want[k].contiguous().view(torch.uint8)
        assert bool(same.all()), (what, k, f"{int((~same).sum())} of {same.numel()} bytes differ")
        if want[k].is_floating_point():
            assert bool(torch.isfinite(want[k]).all()), (what, k)


def _moved(a, b):
    """the two suns really give different pictures: a relight that returned the base pass's results would not pass"""
    return not torch.equal(a["rgb"], b["rgb"]) and not torch.equal(a["sun"], b["sun"])


CASES = [("relu-c0", 5, 13, "f16x2"), ("relu-c0", 37, 7, "f16x2"), ("relu-c5-sbeta-ts", 5, 13, "f16x2"),
         ("relu-c5-sbeta-ts", 37, 7, "f16x2"), ("product", 96, 8, "f16x2"), ("product", 96, 8, "f16x1"), ("feat512", 32, 8, "f16x2")]


@pytest.mark.parametrize("net,N,S,mode", CASES, ids=[f"{n}-{a}x{b}-{m}" for n, a, b, m in CASES])
def test_relight_has_the_bits_of_a_full_pass(net, N, S, mode):
    c = Case(net, N, S, mode)
    sun_a, sun_b = _unit(N, 1), _unit(N, 2)
    want, _ = c.full(sun_b)
    base, ws = c.full(sun_a)
    got = c.relight(sun_b, ws)
    _assert_bits(got, want, "relight(B) after base(A) vs full(B)")
    assert _moved(base, want)
    for k in ("depth", "weights", "transparency", "albedo", "beta", "sigmas", "z_vals"):      # what no sun changes
        assert torch.equal(got[k], base[k]), k


@pytest.mark.parametrize("what,t_scale", [("sun-sets-the-exponent", 2.0 ** -12), ("t-sets-the-exponent", 2.0 ** 4)])
def test_extras_block_exponent(what, t_scale):
    """the extras block [sun | t | t_s] shares one exponent per 128 points: with small t the (unit) sun sets it, with large t the
    embedding does; either way the whole block is rewritten under the new sun's maximum.  Sun B = sun A reproduces the base pass."""
    c = Case("relu-c5-sbeta-ts", 37, 7, t_scale=t_scale)
    sun_a, sun_b = _unit(37, 3), _unit(37, 4)
    if t_scale < 1:      # make the block maximum move between the suns: sun A's largest component is well below sun B's in some rows
        sun_a = torch.nn.functional.normalize(torch.ones(37, 3, device=DEV) + 0.01 * sun_a, dim=1)      # |max| ~ 0.58: exponent of [0.5, 1)
        sun_b[::2] = torch.tensor([0.0, 0.0, 1.0], device=DEV)                                            # |max| = 1: the next exponent
    tt = torch.cat([c.t, c.t_s], 1).abs()
    assert float(tt.max()) < 0.25 if t_scale < 1 else bool((tt.amax(1) > 1.0).all())      # who holds the block maximum
    want, _ = c.full(sun_b)
    base, ws = c.full(sun_a)
    _assert_bits(c.relight(sun_b, ws), want, what)
    _assert_bits(c.relight(sun_a, ws), base, what + ": sun B = sun A")
    assert _moved(base, want)


def test_relights_chain_and_return_to_the_base_sun():
    c = Case("product", 96, 8)
    sun_a, sun_b, sun_c = _unit(96, 1), _unit(96, 2), _unit(96, 6)
    want_c, _ = c.full(sun_c)
    base, ws = c.full(sun_a)
    c.relight(sun_b, ws)
    _assert_bits(c.relight(sun_c, ws), want_c, "base(A), relight(B), relight(C) vs full(C)")
    _assert_bits(c.relight(sun_a, ws), base, "... then relight(A) vs the base pass")


def test_a_subset_has_the_bits_of_the_whole():
    c = Case("product", 96, 8)
    sun_a, sun_b = _unit(96, 1), _unit(96, 2)
    _, ws = c.full(sun_a)
    everything = c.relight(sun_b, ws)
    only = c.relight(sun_b, ws, keys=("rgb",))
    assert list(only) == ["rgb"] and torch.equal(only["rgb"], everything["rgb"])


@pytest.mark.parametrize("net,N,S,mode", [("relu-c5-sbeta-ts", 37, 7, "f16x2"), ("product", 96, 8, "f16x2"), ("product", 96, 8, "f16x1")],
                         ids=("relu", "product", "product-f16x1"))
def test_relight_does_not_depend_on_what_the_workspace_held(net, N, S, mode, monkeypatch):
    """the harness of tests/test_gpu_fill.py: the workspace (and every result tensor) carries the fill before the base pass; the
    relight's results are identical under every fill, and those of a full pass"""
    c = Case(net, N, S, mode)
    sun_a, sun_b = _unit(N, 1), _unit(N, 2)
    want, _ = c.full(sun_b)

    def run(fill):
        _poison(monkeypatch, fill)
        _, ws = c.full(sun_a)
        return c.relight(sun_b, ws)

    for fill, got in run_filled(run).items():
        _assert_bits(got, want, f"fill 0x{fill:02X}")


def test_refusals_on_the_device_path():
    from snerf_amd import _lib, ops
    c = Case("relu-c5-sbeta-ts", 37, 7)
    sun_a, sun_b = _unit(37, 1), _unit(37, 2)
    want, _ = c.full(sun_b)
    # after a solar-correction pass on the same workspace
    base, ws = c.full(sun_a)
    z = base["z_vals"]
    sc = {k: torch.empty_like(base[k]) for k in ("weights", "transparency", "sun")}
    assert ops.render_pass_into(c.spec, c.gp, ops.PassInputs(sun_d=sun_a, rays=c.rays, z_vals=z), c.t, c.t_s, sc, sc_pass=True,
                                packed=c.packed, workspace=ws) is ws
    with pytest.raises(RuntimeError, match=r"last pass was a solar-correction \(SNERF_FLAG_SC_PASS\) pass"):
        c.relight(sun_b, ws)
    # a fresh base pass makes the same workspace good again
    _, ws2 = c.full(sun_a, ws=ws)
    assert ws2 is ws
    _assert_bits(c.relight(sun_b, ws), want, "after a new base pass")
    # another n_samples
    with pytest.raises(RuntimeError, match="descriptor differs from the base pass"):
        c.relight(sun_b, ws, keys=("rgb",), n_samples=6)
    # after a training pass on the same workspace (one large enough for it)
    d_train = c.spec.desc(37, 7, _lib.FLAG_TRAIN)
    big = torch.empty(_lib.call_size("snerf_workspace_bytes", d_train), dtype=torch.uint8, device=DEV)
    _, ws3 = c.full(sun_a, ws=big)
    assert ws3 is big
    _assert_bits(c.relight(sun_b, big), want, "on a larger workspace")
    pin = c.pin(sun_a)
    so = _lib.SnerfOutputs()
    rgb = torch.empty(37, 3, device=DEV)
    so.rgb = rgb.data_ptr()
    _lib.call("snerf_forward", d_train, c.packed, pin.struct(c.t, c.t_s), so, big, big.numel())
    with pytest.raises(RuntimeError, match=r"last pass was a training \(SNERF_FLAG_TRAIN\) pass"):
        c.relight(sun_b, big)
    torch.cuda.synchronize()


def test_beta_of_a_base_pass_that_skipped_it_is_refused():
    """the product shape: a base pass asked for no beta does not compute the beta block of the first head layer (tj_skip)"""
    c = Case("product", 96, 8)
    sun_a, sun_b = _unit(96, 1), _unit(96, 2)
    want, _ = c.full(sun_b)
    lean = ("rgb", "depth", "sun", "semantic_label")
    _, ws = c.full(sun_a, keys=lean)
    with pytest.raises(RuntimeError, match="beta is asked of a base pass that was asked for no beta"):
        c.relight(sun_b, ws, keys=("rgb", "beta"))
    got = c.relight(sun_b, ws, keys=lean)      # what such a base pass can give, it gives bit for bit
    _assert_bits(got, {k: want[k] for k in lean}, "lean relight")


# ---- products on the fixture scene: the 9 x 7 window of tests/test_gpu_nadir.py, {"perturb": 0}, three suns ---------------------------
MORE_SUNS = [(35.0, 120.0), (62.5, 201.0)]      # behind sun 0, the first image's (what nadir_products defaults to)
INDEPENDENT = ("dsm", "albedo", "beta", "label")


def _suns(ds):
    return [(float(ds.metas[0]["sun_elevation"]), float(ds.metas[0]["sun_azimuth"]))] + MORE_SUNS


def _sweep_args(ds, geo, truth):
    a = _args(ds, geo, truth)
    a.pop("sun_elevation"), a.pop("sun_azimuth")
    return a


@pytest.fixture(scope="module")
def per_sun(scene, truth):
    """the reference: nadir_products under each sun, computed once"""
    from snerf_amd.eval.utils.ortho import nadir_products
    c, pipe, ds, geo = scene
    a = _sweep_args(ds, geo, truth)
    return [nadir_products(c, pipe.renderer, pipe.models, sun_elevation=el, sun_azimuth=az, gt=truth["gt"],
                           water_mask=truth["water_mask"], **a) for el, az in _suns(ds)]


@pytest.fixture(scope="module")
def sweep(scene, truth):
    from snerf_amd.eval.utils.ortho import nadir_sun_sweep
    c, pipe, ds, geo = scene
    return nadir_sun_sweep(c, pipe.renderer, pipe.models, suns=_suns(ds), gt=truth["gt"], water_mask=truth["water_mask"],
                           **_sweep_args(ds, geo, truth))


def test_sweep_maps_are_nadir_products_under_each_sun(scene, sweep, per_sun):
    ds = scene[2]
    assert sweep["suns"] == _suns(ds)
    assert tuple(sweep["rgb"].shape) == (3, 3, H, W) and tuple(sweep["sun"].shape) == (3, H, W) and tuple(sweep["lit_share"].shape) == (H, W)
    for k, ref in enumerate(per_sun):
        assert _same(sweep["rgb"][k], ref["rgb"]), k
        assert _same(sweep["sun"][k], ref["sun"]), k
    assert not torch.equal(sweep["sun"][0], sweep["sun"][1]) and not torch.equal(sweep["rgb"][1], sweep["rgb"][2])
    for key in INDEPENDENT + ("rays",):
        assert _same(sweep[key], per_sun[0][key]), key
    assert sweep["grid"] == per_sun[0]["grid"] and sweep["planimetric_error"] == per_sun[0]["planimetric_error"]
    assert sweep["scene_bounds"] == per_sun[0]["scene_bounds"] and sweep["mae"] == per_sun[0]["mae"]
    total = torch.zeros((H, W), dtype=torch.float64, device=DEV)
    for k in range(3):
        total += sweep["sun"][k].double()
    assert _same(sweep["lit_share"], (total / 3).float())


def test_sweep_does_not_depend_on_chunking_sharding_or_where_the_suns_come_from(scene, truth, sweep):
    from snerf_amd.eval.utils.ortho import nadir_sun_sweep
    c, pipe, ds, geo = scene
    a = _sweep_args(ds, geo, truth)
    keys = INDEPENDENT + ("rgb", "sun", "lit_share")
    keep = c.pipeline.render_chunk_size
    try:
        for chunk in (16, 4096):
            c.pipeline.render_chunk_size = chunk
            again = nadir_sun_sweep(c, pipe.renderer, pipe.models, suns=_suns(ds), **a)
            assert all(_same(again[k], sweep[k]) for k in keys), chunk
    finally:
        c.pipeline.render_chunk_size = keep
    sharded = nadir_sun_sweep(c, pipe.renderer, pipe.models, suns=_suns(ds), sharded=True, **a)
    assert all(_same(sharded[k], sweep[k]) for k in keys)
    # a loaded dataset supplies the suns of its images, in split order
    dflt = nadir_sun_sweep(c, pipe.renderer, pipe.models, dataset=ds, grid=truth["window"], t=T, render_options=OPTS)
    assert dflt["suns"] == [(float(m["sun_elevation"]), float(m["sun_azimuth"])) for m in ds.metas]
    assert _same(dflt["rgb"][0], sweep["rgb"][0]) and _same(dflt["sun"][0], sweep["sun"][0])
    assert all(_same(dflt[k], sweep[k]) for k in INDEPENDENT)


def test_lean_relight_is_lean_inference_under_each_sun(scene):
    from snerf_amd.eval.utils.util import lean_inference, lean_relight, sun_extras
    c, pipe, ds, _ = scene
    im = pipe.datasets["rgb_test"].scene_images()[0]
    rays, extras = (im[k].reshape(-1, im[k].shape[-1]) for k in ("rays", "extras"))
    keys = ("rgb_coarse", "sun_coarse", "depth_coarse", "semantic_label_coarse")
    suns = _suns(ds)
    keep = c.pipeline.render_chunk_size
    try:
        c.pipeline.render_chunk_size = max(16, rays.shape[0] // 3 + 1)      # three ragged chunks
        got = lean_relight(c, pipe.renderer, pipe.models, rays, extras, suns, keys=keys, render_options=OPTS)
        for k, sun in enumerate(suns):
            ref = lean_inference(c, pipe.renderer, pipe.models, rays, sun_extras(extras, sun), keys=keys, render_options=OPTS)
            for key in keys:
                assert tuple(got[key].shape) == (3,) + tuple(ref[key].shape) and _same(got[key][k], ref[key]), (k, key)
    finally:
        c.pipeline.render_chunk_size = keep
    assert not torch.equal(got["rgb_coarse"][0], got["rgb_coarse"][1])


def test_export_writes_the_named_files_and_the_pngs_of_export_nadir(scene, truth, sweep, tmp_path):
    from snerf_amd.eval.ortho import export_nadir, export_sun_sweep
    from snerf_amd.framework.util import img_utils as I
    c, pipe, ds, geo = scene
    a = _sweep_args(ds, geo, truth)
    out = export_sun_sweep(c, pipe.renderer, pipe.models, str(tmp_path / "sweep"), suns=_suns(ds), **a)
    assert all(_same(out[k], sweep[k]) for k in ("rgb", "sun", "lit_share"))
    names = {f"{p}_{k:03d}{e}" for p in ("rgb", "sun") for k in range(3) for e in (".png", ".tif")} | {"lit_share.png", "lit_share.tif", "suns.json"}
    d = tmp_path / "sweep" / "nadir" / "sweep"
    assert set(out["files"]) == names == set(os.listdir(d))
    with open(d / "suns.json") as f:
        assert [(s["elevation_deg"], s["azimuth_deg"]) for s in json.load(f)] == _suns(ds)
    arr, _ = I.load_dsm_geotiff(out["files"]["lit_share.tif"])
    assert arr.dtype == np.float32 and arr.tobytes() == out["lit_share"].cpu().numpy().tobytes()
    for k, (el, az) in enumerate(_suns(ds)):
        ref = export_nadir(c, pipe.renderer, pipe.models, str(tmp_path / f"nadir{k}"), sun_elevation=el, sun_azimuth=az, **a)
        for p in ("rgb", "sun"):
            with open(ref["files"][p + ".png"], "rb") as f1, open(out["files"][f"{p}_{k:03d}.png"], "rb") as f2:
                assert f1.read() == f2.read(), (k, p)
