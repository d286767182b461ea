"""The density-gradient pass on the GPU (-m gpu): snerf_density_grad (include/snerf_normals.h, csrc/normals.hip, bsp_pass.hip:
density_grad_bsp), ops.density_grad_into, eval/utils/normals.py and the normals options of extract_pointcloud / export_nadir.

| check | what |
|---|---|
| 1 test_bit_for_bit_against_the_restatement | grad_ray / grad_sample == tests/normals_numpy.py on the operands the pass itself read (test hook), again on a forced grid |
| 2 test_against_the_fp64_oracle | grad_sample (coef = 1) and grad_ray (coef = weights) against autograd through oracle.mlp_forward in fp64 |
| 3 test_normals_follow_the_oracle / test_a_nan_origin_is_a_counted_nan_normal | ray_normals against the oracle's normal; a NaN origin is a counted NaN normal |
| 4 _run / test_a_backward_afterwards_has_its_own_bits / test_workspace_sizes_are_the_recorded_ones | the forward's outputs, a snerf_backward afterwards, snerf_workspace_bytes of every recorded descriptor |
| 5 test_public_paths_on_the_fixture_scene | extract_pointcloud(with_normals), the PLY, export_nadir(normals) |
| 6 test_no_fill_dependence | outputs and scratch pre-filled with 0xFF and 0x00 bytes |

Shapes: the smallest at which the kernels can still go wrong -- 5 x 7 (P = 35: under one 128-row tile and one 256-point workgroup),
33 x 65 (ragged tiles, S just over one wave of the fold), 64 x 8 at W = 512 (P = 512, full width, skip at 4), 130 x 9 (a trunk without a
skip layer, and a skip at layer 1); SIREN and ReLU, the positional and the identity encoding, the composed and the separate first
head layer (W = 32 uses fc_use_full_features so that feat_last = 32 composes)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import snerf_oracle as O
from tests import normals_numpy as NN
from tests.test_gpu_compose import SWITCH
from tests.test_gpu_cotangents import _default_mode
from tests.test_gpu_kernels import GRAD_REL_TOL, _dev, _gpu_params, _spec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(fc_use_full_features=True)
CASES = {
    # name: (N, S, cfg fields, SNERF_COMPOSE_FEATS)
    "5x7-siren-pe": (5, 7, dict(fc_units=32, **FULL), None),
    "33x65-relu-identity-separate": (33, 65, dict(fc_units=32, model="satnerf", activation_function="relu", **FULL), "0"),
    "33x65-siren-identity": (33, 65, dict(fc_units=32, model="satnerf", **FULL), None),
    "64x8-W512": (64, 8, dict(fc_units=512), None),
    "130x9-noskip-separate": (130, 9, dict(fc_units=32, fc_skips=(), **FULL), "0"),
    "130x9-skip1-relu": (130, 9, dict(fc_units=32, fc_skips=(1,), fc_layers=4, activation_function="relu", mapping_pos_n_freq=4, **FULL), None),
}
SEED = 7
_RUNS = {}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Case:
    """one model and ray batch, the training forward on a workspace of its own and what snerf_density_grad needs"""

    def __init__(self, name):
        from snerf_amd import _lib, ops
        N, S, fields, _ = CASES[name]
        self.cfg = cfg = O.OracleCfg(n_samples=S, **fields)
        self.pn = O.init_params_numpy(cfg, SEED)
        self.b = b = O.batch_to_torch(O.synthetic_batch(N, S, seed=SEED + 100, n_classes=max(cfg.n_classes, 1)))
        dev = _dev()
        self.spec = _spec(cfg)
        self.packed = ops.pack_params(self.spec, _gpu_params(self.pn, dev))
        self.rays, extras = b["rays"].to(dev), b["extras"].to(dev)
        self.emb = torch.from_numpy(O.init_embedding_numpy(cfg, SEED))
        self.ts = extras[:, 3].long()
        self.t = self.emb.to(dev)[self.ts].contiguous()
        self.N, self.S, self.P = N, S, N * S
        self.z = ops.sample_z(self.rays, torch.linspace(0, 1, S).to(dev), b["u"].to(dev))
        self.pin = ops.PassInputs(sun_d=extras[:, :3].contiguous(), rays=self.rays, z_vals=self.z)
        self.desc = self.spec.desc(N, S, _lib.FLAG_TRAIN)
        self.keys = ops.output_keys(self.spec, False)
        n = C.c_size_t(0)
        _lib.check(_lib.lib().snerf_normals_scratch_bytes(C.byref(self.desc), C.byref(n)), "snerf_normals_scratch_bytes")
        self.scratch_bytes = n.value
        self.enc_layers = [i for i in range(cfg.fc_layers - 1, 0, -1) if i in cfg.fc_skips] + [0]
        self.F = self.spec.n_freq
        self.E = 6 * self.F if self.F else 3
        self.Ep = (self.E + 31) // 32 * 32

    def forward(self, fill=None):
        from snerf_amd import _lib, ops
        dev = self.t.device
        ws = torch.empty(_lib.call_size("snerf_workspace_bytes", self.desc), dtype=torch.uint8, device=dev)
        if fill is not None:
            ws.fill_(fill)
        outs = {k: torch.empty(ops._OUT_SHAPES[k](self.N, self.S, self.spec.n_classes), dtype=torch.float32, device=dev) for k in self.keys}
        so = _lib.SnerfOutputs()
        for k, v in outs.items():
            setattr(so, k, v.data_ptr())
        _lib.call("snerf_forward", self.desc, self.packed, self.pin.struct(self.t, None), so, ws, ws.numel())
        return ws, outs

    def density_grad(self, ws, coef, fill=0xFF, samples=True):
        """-> (grad_ray (N, 3) f64, grad_sample (N, S, 3) f32 or None), both pre-filled with `fill` bytes, like the scratch"""
        from snerf_amd import _lib
        dev = self.t.device
        scratch = torch.full((self.scratch_bytes,), fill, dtype=torch.uint8, device=dev)
        gr = torch.full((self.N * 3 * 8,), fill, dtype=torch.uint8, device=dev).view(torch.float64).view(self.N, 3)
        gs = torch.full((self.P * 3 * 4,), fill, dtype=torch.uint8, device=dev).view(torch.float32).view(self.N, self.S, 3) if samples else None
        _lib.call("snerf_density_grad", self.desc, self.packed, self.pin.struct(self.t, None), coef, gr, gs, ws, scratch)
        return gr, gs


def _run(name, monkeypatch):
    """the case's pass, once: the forward, then coef = 1 with the dump hook on, then coef = weights; everything on the host, never edited"""
    _default_mode(monkeypatch)
    if CASES[name][3] is not None:
        monkeypatch.setenv(SWITCH, CASES[name][3])
    if name in _RUNS:
        return _RUNS[name]
    from snerf_amd import _lib
    L = _lib.lib()
    c = _Case(name)
    dev = c.t.device
    ws, outs = c.forward()
    before = {k: v.clone() for k, v in outs.items()}
    dz = torch.full((len(c.enc_layers), c.P, c.cfg.fc_units), float("nan"), dtype=torch.float32, device=dev)
    enc = torch.full((c.P, c.Ep), float("nan"), dtype=torch.float32, device=dev)
    ones = torch.ones((c.N, c.S), dtype=torch.float32, device=dev)
    _lib.check(L.snerf_test_normals_dump(_ptr(dz), _ptr(enc)), "snerf_test_normals_dump")
    try:
        gr1, gs1 = c.density_grad(ws, ones)
    finally:
        _lib.check(L.snerf_test_normals_dump(None, None), "snerf_test_normals_dump")
    _lib.check(L.snerf_test_normals_grid(2 if c.P > 512 else 1), "snerf_test_normals_grid")
    try:
        gr1_small, gs1_small = c.density_grad(ws, ones, fill=0x00)
    finally:
        _lib.check(L.snerf_test_normals_grid(0), "snerf_test_normals_grid")
    grw, _ = c.density_grad(ws, outs["weights"], samples=False)
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k].view(torch.int32), before[k].view(torch.int32)), k     # check 4a: the forward's outputs keep their bits
    r = dict(case=c, dz=dz.cpu().numpy(), enc=enc.cpu().numpy(), gr1=gr1.cpu().numpy(), gs1=gs1.cpu().numpy(),
             gr1_small=gr1_small.cpu().numpy(), gs1_small=gs1_small.cpu().numpy(), grw=grw.cpu().numpy(),
             weights=outs["weights"].cpu(), z=c.z.cpu())
    _RUNS[name] = r
    return r


def _oracle_grads(c, z, weights, dtype):
    """autograd through oracle.mlp_forward at the pass's own positions: (d sum sigma / d xyz (P, 3), sum_s w d sigma / d xyz (N, 3))"""
    b, cfg = c.b, c.cfg
    o, d = b["rays"][:, 0:3], b["rays"][:, 3:6]
    xyz = (o.unsqueeze(1) + d.unsqueeze(1) * z.unsqueeze(2)).reshape(-1, 3)          # fp32, as the encode kernel forms it: one product, one sum
    p = O.to_torch(c.pn, dtype)
    x = xyz.to(dtype).requires_grad_(True)
    rep = lambda a: a.unsqueeze(1).expand(c.N, c.S, a.shape[-1]).reshape(c.P, -1).to(dtype)
    sigma = O.mlp_forward(p, x, rep(b["extras"][:, :3]), rep(c.emb[c.ts.cpu()]), cfg)[:, 3]
    g1, = torch.autograd.grad(sigma.sum(), x, retain_graph=True)
    gw, = torch.autograd.grad((sigma * weights.reshape(-1).to(dtype)).sum(), x)
    return g1.double().numpy(), gw.double().reshape(c.N, c.S, 3).sum(1).numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", list(CASES))
def test_bit_for_bit_against_the_restatement(name, monkeypatch):
    r = _run(name, monkeypatch)
    c = r["case"]
    assert np.isfinite(r["dz"]).all() and np.isfinite(r["enc"]).all()                 # the hook wrote every word
    w_layers = [c.pn[f"fc_net.{2 * i}.weight"][:, :c.E] for i in c.enc_layers]
    G = NN.point_gradient(list(r["dz"]), w_layers, r["enc"], c.F)
    ray, sample = NN.ray_fold(G, c.N, c.S)
    assert np.abs(G).max() > 0
    for tag, gr, gs in (("default grid", r["gr1"], r["gs1"]), ("forced grid", r["gr1_small"], r["gs1_small"])):
        assert np.array_equal(gr.view(np.int64), ray.view(np.int64)), (name, tag)
        assert np.array_equal(gs.view(np.int32), sample.view(np.int32)), (name, tag)


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_fp64_oracle(name, monkeypatch):
    """per-tensor relative L2; the bar: the larger of GRAD_REL_TOL (2e-4) and 4 x the relative L2 between the oracle in fp32 and in
    fp64 on the same inputs (the default arithmetic carries about two bits fewer than fp32)"""
    r = _run(name, monkeypatch)
    c = r["case"]
    ref1, refw = _oracle_grads(c, r["z"], r["weights"], torch.float64)
    f1, fw = _oracle_grads(c, r["z"], r["weights"], torch.float32)
    for what, got, ref, f32 in (("grad_sample, coef = 1", r["gs1"].reshape(-1, 3).astype(np.float64), ref1, f1),
                                ("grad_ray, coef = weights", r["grw"], refw, fw)):
        bar = max(GRAD_REL_TOL, 4.0 * _rel(f32, ref))
        err = _rel(got, ref)
        print(f"{name}: {what}: rel L2 {err:.3e} (bar {bar:.3e}; oracle fp32 vs fp64 {_rel(f32, ref):.3e})")
        assert err <= bar, (name, what, err, bar)


# ---- 3. normals through the public walk ---------------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    """what eval's walks need of a model: .spec and named_parameters() under the reference's names"""

    def __init__(self, spec, params):
        super().__init__()
        self.spec = spec
        self._names = list(params)
        for k, v in params.items():
            self.register_parameter(k.replace(".", "__"), torch.nn.Parameter(v, requires_grad=False))

    def named_parameters(self, *a, **k):
        return [(n, getattr(self, n.replace(".", "__"))) for n in self._names]


def _walk(c, rays):
    from types import SimpleNamespace
    from snerf_amd.eval.utils import normals as NM
    dev = rays.device
    emb = torch.nn.Embedding.from_pretrained(c.emb.to(dev))
    models = {"coarse": _Model(c.spec, _gpu_params(c.pn, dev)), "t": emb}
    cfgs = SimpleNamespace(pipeline=SimpleNamespace(batch_size=50, n_samples=c.S, n_importance=0))
    renderer = SimpleNamespace(N_samples=c.S)
    return NM.ray_normals(cfgs, renderer, models, rays, c.b["extras"].to(dev), {"perturb_rand": c.b["u"].to(dev)})


def test_normals_follow_the_oracle(monkeypatch):
    """angle between ray_normals (three chunks of at most 50 rays) and the oracle's normal <= asin(bar of check 2) on every ray whose
    oracle gradient norm is at least 1e-3 of the median; at most 5 % of the rays may fall under that rule (a condition on the seed,
    met by the oracle alone)"""
    name = "130x9-noskip-separate"
    r = _run(name, monkeypatch)
    c = r["case"]
    _, refw = _oracle_grads(c, r["z"], r["weights"], torch.float64)
    _, fw = _oracle_grads(c, r["z"], r["weights"], torch.float32)
    bar = max(GRAD_REL_TOL, 4.0 * _rel(fw, refw))
    norm = np.linalg.norm(refw, axis=1)
    keep = norm >= 1e-3 * np.median(norm)
    assert (~keep).mean() <= 0.05
    res = _walk(c, c.rays)
    assert res["bad"] == 0 and tuple(res["normal_n"].shape) == (c.N, 3) and res["normal_n"].dtype == torch.float32
    got = res["normal_n"].double().cpu().numpy()
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-6)
    # (a chunk of 50 rays cuts the 128-point exponent blocks elsewhere than the whole batch does: close, not bit-equal)
    assert np.allclose(res["grad_norm"].cpu().numpy(), np.linalg.norm(r["grw"], axis=1), rtol=1e-3)
    ref = -refw / norm[:, None]
    sin = np.linalg.norm(np.cross(got, ref), axis=1)
    print(f"{name}: largest sin(angle) {sin[keep].max():.3e} over {int(keep.sum())} rays (bar {bar:.3e})")
    assert (sin[keep] <= bar).all() and ((got * ref).sum(1)[keep] > 0).all()


def test_a_nan_origin_is_a_counted_nan_normal(monkeypatch):
    """Ray 3 gets a NaN origin: its normal is NaN and `bad` counts every NaN normal.  The training FORWARD already hands the ray
    before a NaN ray non-finite head results (albedo, sun, beta and the logits of that ray; its sigma, weights and depth are finite),
    and the composite backward the pass shares with snerf_backward multiplies them by its zero cotangents (0 x NaN): that ray's
    d sigma, hence its normal, may be NaN too and is then counted; no other ray is."""
    r = _run("130x9-noskip-separate", monkeypatch)
    c = r["case"]
    rays = c.rays.clone()
    rays[3, 0] = float("nan")
    res = _walk(c, rays)
    n = res["normal_n"].cpu()
    nan_rows = torch.nonzero(torch.isnan(n).any(1)).flatten().tolist()
    assert 3 in nan_rows and set(nan_rows) <= {2, 3} and res["bad"] == len(nan_rows)
    assert bool(torch.isnan(n[3]).all()) and bool(torch.isfinite(torch.cat([n[:2], n[4:]])).all())


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x7-siren-pe", "130x9-noskip-separate", "64x8-W512"])
def test_a_backward_afterwards_has_its_own_bits(name, monkeypatch):
    from snerf_amd import _lib
    _run(name, monkeypatch)
    c = _RUNS[name]["case"]
    dev = c.t.device

    def backward(with_call):
        ws, outs = c.forward()
        if with_call:
            c.density_grad(ws, outs["weights"])
        go = _lib.SnerfOutGrads()
        keep = []
        for k in ("rgb", "weights", "sigmas", "beta"):
            v = torch.randn(tuple(outs[k].shape), generator=torch.Generator().manual_seed(len(k))).to(dev)
            keep.append(v)
            setattr(go, k, v.data_ptr())
        pg = torch.zeros(_lib.call_size("snerf_grad_floats", c.desc), dtype=torch.float32, device=dev)
        d_t = torch.empty_like(c.t)
        _lib.call("snerf_backward", c.desc, c.packed, c.pin.struct(c.t, None), go, pg, d_t, None, ws, ws.numel())
        torch.cuda.synchronize()
        return pg.cpu(), d_t.cpu()

    a, b = backward(False), backward(True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert float(a[0].abs().max()) > 0


def test_workspace_sizes_are_the_recorded_ones():
    from snerf_amd import _lib
    L = _lib.lib()
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_sizes.json")))
    for c in doc["cases"]:
        d = _lib.SnerfDesc(*c["desc"])
        assert L.snerf_workspace_bytes(C.byref(d)) == c["sizes"][2], c["desc"]


# ---- 5. public paths on the fixture scene -------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_public_paths_on_the_fixture_scene(tmp_path, monkeypatch):
    from snerf_amd.eval import ortho as EO
    from snerf_amd.eval.extract_pointcloud import extract_pointcloud, save_ply
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.framework.pipelines import load_pipeline
    from tests.test_gpu_scene import _pipeline_cfgs
    _default_mode(monkeypatch)
    torch.manual_seed(0)
    cfgs = _pipeline_cfgs(False, tmp_path / "cache")
    pipe = load_pipeline(cfgs).to(_dev())
    ds = pipe.datasets["rgb_test"].dataset
    geo = ds.geo
    total = ds.t["rays"].shape[0]
    rows = torch.arange(300, device=_dev()) * (total // 300)
    rays, extras = ds.t["rays"][rows].contiguous(), ds.t["extras"][rows].contiguous()
    opts = {"perturb": 0}
    base = extract_pointcloud(cfgs, pipe.renderer, pipe.models, rays, extras, render_options=opts, geo=geo)
    got = extract_pointcloud(cfgs, pipe.renderer, pipe.models, rays, extras, render_options=opts, geo=geo, with_normals=True)
    assert sorted(got) == sorted(list(base) + ["normals_n", "normals_enu"])
    for k in base:
        assert _same(base[k], got[k]), k
    for k in ("normals_n", "normals_enu"):
        n = got[k]
        assert tuple(n.shape) == (300, 3) and n.dtype == torch.float32
        fin = torch.isfinite(n).all(1)
        assert int(fin.sum()) >= 285 and bool(((n[fin].double().norm(dim=1) - 1.0).abs() < 1e-6).all()), k
    fp = save_ply(str(tmp_path / "cloud.ply"), got["xyz_utm"], got["colors"], got["labels"], normals=got["normals_enu"])
    raw = open(fp, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in head and b"element vertex 300\n" in head
    rec = np.frombuffer(body, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                     ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("label", "u1")])
    assert rec.shape == (300,) and np.array_equal(rec["nz"].view(np.int32), got["normals_enu"][:, 2].cpu().numpy().view(np.int32))

    from snerf_amd.framework.util import img_utils as I
    d = os.path.join(ROOT, "tests", "golden", "scene_small_dsm", "dsm")
    roi = D.roi_grid(I.load_dsm_ground_truth(os.path.join(d, "JAX_068_DSM.tif"), os.path.join(d, "JAX_068_DSM.txt"), os.path.join(d, "JAX_068_CLS.tif"))["roi"])
    args = dict(geo=geo, grid=D.grid_struct(roi, (0, 0, 9, 7)), min_alt=min(it["alt_min"] for it in ds.items),
                max_alt=max(it["alt_max"] for it in ds.items), sun_elevation=float(ds.metas[0]["sun_elevation"]),
                sun_azimuth=float(ds.metas[0]["sun_azimuth"]), t=0, render_options=opts)
    plain = EO.export_nadir(cfgs, pipe.renderer, pipe.models, str(tmp_path / "plain"), **args)
    withn = EO.export_nadir(cfgs, pipe.renderer, pipe.models, str(tmp_path / "normals"), normals=True, **args)
    assert sorted(set(withn["files"]) - set(plain["files"])) == ["normal.png", "normal_up.tif", "normals.json"]
    for name, path in withn["files"].items():
        assert os.path.getsize(path) > 0, name
        if name in plain["files"]:
            assert open(path, "rb").read() == open(plain["files"][name], "rb").read(), name
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert _same(v, withn[k]), k
    assert tuple(withn["normal"].shape) == (3, 7, 9) and tuple(withn["normal_angle"].shape) == (7, 9)
    doc = json.load(open(withn["files"]["normals.json"]))
    agree = doc["agreement_with_dsm_normals"]
    assert sorted(agree) == ["bad", "cells", "mean_deg", "median_deg", "share_under_15deg"] and agree["cells"] + agree["bad"] <= 63
    print(f"untrained fixture model, 9 x 7 nadir cells: density normals against the DSM's raster normals: {agree} (no bar)")


# ---- 6. fills -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x7-siren-pe", "33x65-relu-identity-separate"])
def test_no_fill_dependence(name, monkeypatch):
    """outputs, scratch and the workspace of the forward pre-filled with NaN bytes and with zeros: identical results"""
    _run(name, monkeypatch)
    c = _RUNS[name]["case"]
    res = []
    for fill in (0xFF, 0x00):
        ws, outs = c.forward(fill)
        gr, gs = c.density_grad(ws, outs["weights"], fill=fill)
        torch.cuda.synchronize()
        res.append((gr.cpu(), gs.cpu()))
    assert torch.equal(res[0][0].view(torch.int64), res[1][0].view(torch.int64)) and torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    assert np.array_equal(res[0][0].numpy().view(np.int64), _RUNS[name]["grw"].view(np.int64))
