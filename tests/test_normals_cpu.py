"""CPU-side checks of the density-gradient pass (include/snerf_normals.h, csrc/normals.hip, eval/utils/normals.py; DESIGN.md section
5za): the numpy restatement of the two new kernels (tests/normals_numpy.py, the oracle of tests/test_gpu_normals.py) against
torch.autograd in fp64, every refusal of the entries through the binding (none reaches a launch), the new header against its binding
rows with the frozen main header and ABI version, the host functions on closed forms, and the defaults of the public paths on stubs."""
import ctypes as C
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import snerf_oracle as O
from snerf_amd import _lib
from snerf_amd.eval.utils import normals as NM          # the feature under test: every test of this file needs it
from tests import normals_numpy as NN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DUMMY = 4096        # a non-null, 256-byte aligned address no refusal path dereferences
NAMES = {
    "snerf_normals_scratch_bytes": ["desc", "bytes"],
    "snerf_density_grad": ["desc", "packed_params", "inputs", "coef", "grad_ray", "grad_sample", "workspace", "scratch", "stream"],
    "snerf_test_normals_grid": ["n"],
    "snerf_test_normals_dump": ["dz", "enc"],
}


# ---- the restatement against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skips,layers", [((4,), 8), ((), 8), ((1,), 3)], ids=["skip4", "noskip", "skip1"])
@pytest.mark.parametrize("n_freq", [10, 0], ids=["F10", "identity"])
@pytest.mark.parametrize("act", ["siren", "relu"])
def test_the_restatement_is_autograds_d_sigma_d_xyz(act, n_freq, skips, layers):
    """dz at layer 0 and at the skip layer from autograd (retain_grad) on the oracle's trunk(encode(xyz)) in fp64, fed to the
    restatement with the exact encoding: d xyz to 1e-12 relative -- fp64 rounding of a 512-term sum, not a tuned number"""
    W, P = 512, 6
    cfg = O.OracleCfg(fc_units=W, fc_layers=layers, fc_skips=skips, activation_function=act, mapping_pos_n_freq=n_freq,
                      model="semantic" if n_freq else "satnerf")
    p = O.to_torch(O.init_params_numpy(cfg, 3), torch.float64)
    rng = np.random.default_rng(11)
    xyz = torch.from_numpy(rng.uniform(-1, 1, (P, 3))).requires_grad_(True)
    coef = torch.from_numpy(rng.uniform(0.1, 1.0, (P,)))
    enc = O.encode(xyz, cfg)
    zs, h = {}, enc
    for i in range(cfg.fc_layers):                      # oracle.trunk, layer by layer, so that the pre-activations can keep their gradients
        if i in cfg.fc_skips:
            h = torch.cat([enc, h], -1)
        z = F.linear(h, p[f"fc_net.{2 * i}.weight"], p[f"fc_net.{2 * i}.bias"])
        z.retain_grad()
        zs[i] = z
        h = O._act(z, cfg, 30.0 if i == 0 else 1.0)
    sigma = F.softplus(F.linear(h, p["sigma_from_xyz.0.weight"], p["sigma_from_xyz.0.bias"]))
    assert torch.equal(sigma, O.trunk(p, enc, cfg)[0])   # the loop above IS the oracle's trunk
    (sigma[:, 0] * coef).sum().backward()
    ref = xyz.grad.numpy()
    order = [i for i in range(cfg.fc_layers - 1, 0, -1) if i in cfg.fc_skips] + [0]
    E = cfg.enc_dim
    G = NN.point_gradient([zs[i].grad.numpy() for i in order], [p[f"fc_net.{2 * i}.weight"].numpy()[:, :E] for i in order],
                          enc.detach().numpy(), n_freq)
    assert np.abs(ref).max() > 0
    assert np.linalg.norm(G - ref) <= 1e-12 * np.linalg.norm(ref) and np.abs(G - ref).max() <= 1e-12 * np.abs(ref).max()
    ray, sample = NN.ray_fold(G, 2, 3)
    assert np.array_equal(ray[0], (G[0] + G[1]) + G[2]) and sample.dtype == np.float32 and sample.shape == (2, 3, 3)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _desc(flags=_lib.FLAG_TRAIN, **kw):
    from snerf_amd.ops import ModelSpec
    return ModelSpec(fc_units=64, **kw).desc(8, 16, flags)


def _grad(d=None, **edit):
    """snerf_density_grad on the descriptor `d` with dummy addresses, the arguments named in `edit` replaced (None: NULL) -> (code,
    message).  Every caller passes something the entry refuses before a launch: a call with nothing to refuse is a mistake of the test
    and never made."""
    assert d is not None or edit, "nothing to refuse"
    L = _lib.lib()
    inputs = _lib.SnerfInputs()
    inputs.sun_d, inputs.sun_stride = DUMMY, 3
    a = dict(desc=C.byref(d if d is not None else _desc()), packed_params=DUMMY, inputs=C.byref(inputs), coef=DUMMY, grad_ray=DUMMY,
             grad_sample=None, workspace=DUMMY, scratch=DUMMY)
    for k, v in edit.items():
        assert k in a, k
        a[k] = v
    rc = L.snerf_density_grad(a["desc"], a["packed_params"], a["inputs"], a["coef"], a["grad_ray"], a["grad_sample"], a["workspace"],
                              a["scratch"], None)
    return rc, L.snerf_last_error().decode()


@pytest.mark.parametrize("arg", ["desc", "packed_params", "inputs", "coef", "grad_ray", "workspace", "scratch"])
def test_a_null_argument_is_refused_by_name(arg):
    rc, msg = _grad(**{arg: None})
    assert rc == 3 and msg == f"snerf_density_grad: {arg} is NULL"        # SNERF_ERR_NULL


@pytest.mark.parametrize("flags,needle", [
    (0, "lacks SNERF_FLAG_TRAIN"),
    (_lib.FLAG_TRAIN | _lib.FLAG_SC_PASS, "SNERF_FLAG_SC_PASS is not a flag of this pass"),
    (_lib.FLAG_TRAIN | _lib.FLAG_RELIGHT, "SNERF_FLAG_RELIGHT is not a flag of this pass"),
    (_lib.FLAG_TRAIN | _lib.FLAG_GEOMETRY, "SNERF_FLAG_GEOMETRY is not a flag of this pass"),
    (_lib.FLAG_TRAIN | _lib.FLAG_EMBED_GRAD, "SNERF_FLAG_EMBED_GRAD is not a flag of this pass"),
    (_lib.FLAG_TRAIN | _lib.FLAG_DEPTH_MEDIAN, "SNERF_FLAG_DEPTH_MEDIAN is not a flag of this pass"),
    (_lib.FLAG_TRAIN | _lib.FLAG_F16X1, "one-plane arithmetic SNERF_FLAG_F16X1 is not supported"),
])
def test_descriptors_of_other_passes_are_refused(flags, needle):
    d = _desc(flags)
    rc, msg = _grad(d)
    assert rc == 1 and msg.startswith("snerf_density_grad: ") and needle in msg          # SNERF_ERR_BAD_DESC
    n = C.c_size_t(77)
    assert _lib.lib().snerf_normals_scratch_bytes(C.byref(d), C.byref(n)) == 1 and n.value == 77
    assert _lib.lib().snerf_last_error().decode().startswith("snerf_normals_scratch_bytes: ") and needle in _lib.lib().snerf_last_error().decode()


def test_sizes_the_plan_refuses_and_alignment():
    d = _desc()
    d.n_rays = 0
    rc, msg = _grad(d)
    assert rc == 1 and msg == "snerf_density_grad: bad SnerfDesc: n_rays and n_samples must be positive"
    d = _desc()
    d.fc_units = 40
    rc, msg = _grad(d)
    assert rc == 1 and msg.startswith("snerf_density_grad: bad SnerfDesc: fc_units")
    d = _desc()
    d.n_rays, d.n_samples = 1 << 20, 1 << 11
    assert _grad(d) == (1, "snerf_density_grad: bad SnerfDesc: n_rays * n_samples too large for one pass (chunk the rays)")
    for arg in ("workspace", "scratch", "packed_params"):
        rc, msg = _grad(**{arg: DUMMY + 64})
        assert rc == 2 and msg == "snerf_density_grad: workspace, scratch and packed params must be 256-byte aligned"      # SNERF_ERR_WORKSPACE
    L = _lib.lib()
    assert L.snerf_normals_scratch_bytes(None, C.byref(C.c_size_t())) == 3 and L.snerf_last_error().decode() == "snerf_normals_scratch_bytes: desc is NULL"
    assert L.snerf_normals_scratch_bytes(C.byref(_desc()), None) == 3 and L.snerf_last_error().decode() == "snerf_normals_scratch_bytes: bytes is NULL"


def test_scratch_size_and_the_cpu_refusal_of_ops():
    from snerf_amd import ops
    from snerf_amd.ops import ModelSpec
    n = C.c_size_t(0)
    up = lambda v: (v + 255) // 256 * 256
    for spec, N, S, ldw in ((ModelSpec(), 4096, 64, 60), (ModelSpec(fc_units=64, n_freq=0, n_classes=0), 5, 7, 4),
                            (ModelSpec(fc_units=64, n_freq=4), 33, 65, 30), (ModelSpec(fc_units=64, n_freq=16), 3, 3, 120)):
        d = spec.desc(N, S, _lib.FLAG_TRAIN)
        assert _lib.lib().snerf_normals_scratch_bytes(C.byref(d), C.byref(n)) == 0
        P = N * S
        assert n.value == up(P * 24) + up(spec.fc_units * ldw * 8) + up((P + 255) // 256 * 128), (spec, n.value)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.density_grad_into(ModelSpec(), {}, ops.PassInputs(), torch.zeros(4, 4))


# ---- header and ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_new_header_matches_its_binding_rows():
    """include/snerf_normals.h (the pass, its scratch size and the two test hooks) against its rows of _lib.HEADER_SIGNATURES"""
    from tests.abi_header import check_header
    check_header("snerf_normals.h", NAMES)


def test_the_main_header_is_what_it_was():
    """the frozen entry-point list of include/snerf_hip.h: the symbols of _lib.SIGNATURES, none of them new, nothing of this feature"""
    main = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    assert "normals" not in main and "density_grad" not in main and "#define SNERF_ABI_VERSION 6" in main
    src = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    names = re.findall(r"\b(snerf_[a-z_0-9]+)\s*\(", src)
    assert names == list(_lib.EXPORTED_SYMBOLS) and len(names) == 53


# ---- host functions -------------------------------------------------------------------------------------------------------------------------
def _fixture_frame():
    from snerf_amd.baseline.components.normalization import StandardNormalization
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    z = np.load(os.path.join(GOLDEN, "geo_cloud_small.npz"))
    keys = ("X_scale", "X_offset", "Y_scale", "Y_offset", "Z_scale", "Z_offset")
    return GeoFrame(StandardNormalization().set_params(dict(zip(keys, z["norm_params"].tolist()))), str(z["zone_string"]))


def test_to_enu_at_the_fixtures_site():
    geo = _fixture_frame()
    cx, cy, cz = [float(v) for v in geo.params.centre]
    lat, lon = NM.ecef_to_geodetic(cx, cy, cz)
    assert 30.0 < math.degrees(lat) < 30.6 and -82.0 < math.degrees(lon) < -81.3                  # Jacksonville
    R = NM.enu_rotation(geo)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1.0) < 1e-14
    up = np.array([math.cos(lat) * math.cos(lon), math.cos(lat) * math.sin(lon), math.sin(lat)])
    east = np.array([-math.sin(lon), math.cos(lon), 0.0])
    north = np.cross(up, east)
    got = NM.to_enu(geo, np.stack([up, east, north, -up, 2.0 * east]))
    assert np.allclose(got, [[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, -1], [2, 0, 0]], atol=1e-15)
    # the geodetic up is NOT the radial direction: the ellipsoid's normal leans by up to 0.19 degrees
    radial = np.array([cx, cy, cz]) / np.linalg.norm([cx, cy, cz])
    lean = math.degrees(math.acos(NM.to_enu(geo, radial[None])[0, 2]))
    assert 0.1 < lean < 0.2
    t = torch.from_numpy(np.stack([up, east]).astype(np.float32))
    out = NM.to_enu(geo, t)
    assert out.dtype == torch.float32 and torch.allclose(out, torch.tensor([[0.0, 0, 1], [1, 0, 0]]), atol=1e-6)
    nan = NM.to_enu(geo, np.full((1, 3), np.nan))
    assert np.isnan(nan).all()
    # the UTM grid convergence the frame ignores: (lon - lon0) sin(lat)
    conv = math.degrees(lon - float(geo.params.lon0)) * math.sin(lat)          # (lon0: the zone's central meridian, radians)
    assert abs(conv + 0.353) < 0.002


def test_normal_agreement_on_closed_forms():
    ge = np.array([[0.0, 1.0, 0.0], [0.5, np.nan, 0.0]])
    gn = np.array([[0.0, 0.0, -1.0], [0.5, 0.0, 0.0]])
    s2, s15 = math.sqrt(0.5), 1.0 / math.sqrt(1.5)
    n = np.array([[0.0, 0.0, 1.0], [-s2, 0.0, s2], [0.0, 0.0, 1.0], [-0.5 * s15, -0.5 * s15, s15], [0.0, 0.0, 1.0], [np.nan, 0.0, 1.0]])
    ang, stats = NM.normal_agreement(n, ge, gn)
    assert ang.shape == (2, 3) and np.allclose(ang[0], [0.0, 0.0, 45.0], atol=1e-12) and abs(ang[1, 0]) < 1e-6
    assert np.isnan(ang[1, 1]) and np.isnan(ang[1, 2])
    assert stats["cells"] == 4 and abs(stats["mean_deg"] - 11.25) < 1e-6 and abs(stats["median_deg"]) < 1e-6 and stats["share_under_15deg"] == 0.75
    ang2, stats2 = NM.normal_agreement(torch.from_numpy(n.T.reshape(3, 2, 3).copy()), torch.from_numpy(ge), torch.from_numpy(gn))
    assert np.array_equal(np.isnan(ang2), np.isnan(ang)) and np.allclose(np.nan_to_num(ang2), np.nan_to_num(ang)) and stats2 == stats
    # unnormalised input, opposite direction
    assert abs(NM.normal_agreement(np.array([[0.0, 0.0, -3.0]]), np.zeros((1, 1)), np.zeros((1, 1)))[0][0, 0] - 180.0) < 1e-12
    none = NM.normal_agreement(np.full((1, 3), np.nan), np.zeros((1, 1)), np.zeros((1, 1)))[1]
    assert none == {"cells": 0, "mean_deg": None, "median_deg": None, "share_under_15deg": None}
    with pytest.raises(ValueError, match="normal_agreement"):
        NM.normal_agreement(np.zeros((3, 3)), np.zeros((2, 2)), np.zeros((2, 2)))


def test_save_ply_round_trips_normals_and_keeps_its_bytes_without(tmp_path):
    from snerf_amd.eval.extract_pointcloud import save_ply
    rng = np.random.default_rng(4)
    n = 7
    xyz, colors, labels = rng.normal(size=(n, 3)), rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.integers(0, 5, n)
    normals = rng.normal(size=(n, 3)).astype(np.float32)
    normals[2] = np.nan
    fp = save_ply(str(tmp_path / "n.ply"), torch.from_numpy(xyz), torch.from_numpy(colors), torch.from_numpy(labels), normals=torch.from_numpy(normals))
    head, body = open(fp, "rb").read().split(b"end_header\n", 1)
    assert head.decode() == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty double x\nproperty double y\nproperty double z\n"
                             "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                             "property uchar blue\nproperty uchar label\n")
    rec = np.frombuffer(body, dtype=[("xyz", "<f8", 3), ("n", "<f4", 3), ("rgb", "u1", 3), ("label", "u1")])
    assert rec.shape == (n,) and np.array_equal(rec["xyz"], xyz) and np.array_equal(rec["n"].view(np.int32), normals.view(np.int32))
    assert np.array_equal(rec["rgb"], np.clip(np.rint(colors * 255.0), 0, 255).astype("u1")) and np.array_equal(rec["label"], labels.astype("u1"))
    with pytest.raises(ValueError, match="normals must be"):
        save_ply(str(tmp_path / "bad.ply"), xyz, normals=normals[:3])
    # without normals: the header and record layout of the function as it was before it took normals, written out here
    for cols, labs in ((colors, labels), (colors, None), (None, None), (None, labels)):
        props = ["property double x", "property double y", "property double z"]
        fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
        if cols is not None:
            props += ["property uchar red", "property uchar green", "property uchar blue"]
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        if labs is not None:
            props += ["property uchar label"]
            fields += [("label", "u1")]
        want = np.empty(n, dtype=fields)
        want["x"], want["y"], want["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        if cols is not None:
            c8 = np.clip(np.rint(cols * 255.0), 0, 255).astype("u1")
            want["red"], want["green"], want["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
        if labs is not None:
            want["label"] = labs.astype("u1")
        expected = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s\nend_header\n" % (n, "\n".join(props))).encode() + want.tobytes()
        got = open(save_ply(str(tmp_path / "plain.ply"), xyz, cols, labs), "rb").read()
        assert got == expected


# ---- defaults ---------------------------------------------------------------------------------------------------------------------------------
def test_the_defaults_do_not_touch_the_new_module(monkeypatch):
    """extract_pointcloud(with_normals=False) and nadir_products(normals=False) on stubs: eval/utils/normals.py is replaced by a module
    whose every attribute raises, and the walks below it by recorders"""
    from snerf_amd.eval import extract_pointcloud as X
    from snerf_amd.eval.utils import ortho as OR

    class _Trap(types.ModuleType):
        def __getattr__(self, name):
            raise AssertionError(f"the default path touched eval/utils/normals.py ({name})")

    trap = _Trap("snerf_amd.eval.utils.normals")
    monkeypatch.setitem(sys.modules, "snerf_amd.eval.utils.normals", trap)
    import snerf_amd.eval.utils as U
    monkeypatch.setattr(U, "normals", trap, raising=False)
    rays = torch.arange(40, dtype=torch.float32).reshape(5, 8)
    calls = []

    def lean(cfgs, renderer, models, r, e, keys, render_options):
        calls.append(tuple(keys))
        return {"rgb_coarse": torch.zeros(5, 3), "depth_coarse": torch.ones(5)}

    monkeypatch.setattr(X, "lean_inference", lean)
    models = {"coarse": types.SimpleNamespace(spec=types.SimpleNamespace(n_classes=0))}
    out = X.extract_pointcloud(None, None, models, rays, None)
    assert sorted(out) == ["colors", "depth", "xyz_n"] and calls == [("rgb_coarse", "depth_coarse")]
    assert torch.equal(out["xyz_n"], X.get_xyz_from_nerf_prediction(rays, torch.ones(5)))

    walked = {"suns": [(45.0, 120.0)], "rgb": torch.zeros(1, 3, 2, 2), "sun": torch.zeros(1, 2, 2), "dsm": torch.zeros(2, 2)}
    monkeypatch.setattr(OR, "_nadir_walk", lambda *a, **k: dict(walked))
    prod = OR.nadir_products(None, None, None, sun_elevation=45.0, sun_azimuth=120.0)
    assert sorted(prod) == ["dsm", "rgb", "sun"] and tuple(prod["rgb"].shape) == (3, 2, 2)
    with pytest.raises(ValueError, match="single-device"):
        OR.nadir_products(None, None, None, normals=True, sharded=True)
