"""Host side of the geometry pass (SNERF_FLAG_GEOMETRY): the flag, the sizes, every refusal that returns
before the device is touched, and the key selection of the chunk walks on a stub renderer.  No GPU work."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_hip.h")
BAD_DESC = 1      # SNERF_ERR_BAD_DESC


def _specs():
    from snerf_amd.ops import ModelSpec
    return [ModelSpec(), ModelSpec(siren=False), ModelSpec(fc_units=64, feat_last=32, fc_layers=3, fc_skips=()),
            ModelSpec(fc_units=64, feat_last=32, fc_layers=4, fc_skips=(2,), siren=False), ModelSpec(n_freq=0, n_classes=0)]


def test_flag_mirrors_the_header_and_the_abi_version_stays():
    from snerf_amd import _lib
    text = open(HEADER).read()
    value = int(re.search(r"#define\s+SNERF_FLAG_GEOMETRY\s+(\d+)u", text).group(1))
    assert _lib.FLAG_GEOMETRY == value == 32
    others = (_lib.FLAG_TRAIN, _lib.FLAG_SC_PASS, _lib.FLAG_RELIGHT, _lib.FLAG_EMBED_GRAD, _lib.FLAG_F16X1, _lib.FLAG_F16X2)
    assert all(value & f == 0 for f in others) and value < _lib.FLAG_F16X2
    assert int(re.search(r"#define\s+SNERF_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == _lib.lib().snerf_version() == 6


@pytest.mark.parametrize("other", ("FLAG_TRAIN", "FLAG_SC_PASS", "FLAG_RELIGHT", "FLAG_EMBED_GRAD"))
def test_the_flag_combines_with_no_other_pass_kind(other):
    """the plan refuses it, hence the size entries and both hot calls, before they look at a pointer"""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    for extra in (0, _lib.FLAG_F16X1, _lib.FLAG_TRAIN):
        d = ModelSpec().desc(64, 8, _lib.FLAG_GEOMETRY | getattr(_lib, other) | extra)
        assert L.snerf_workspace_bytes(C.byref(d)) == 0
        msg = L.snerf_last_error().decode()
        assert "SNERF_FLAG_GEOMETRY" in msg and "SNERF_" + other in msg, msg
        assert L.snerf_forward(C.byref(d), None, None, None, None, 0, None) == BAD_DESC
        assert "SNERF_FLAG_GEOMETRY" in L.snerf_last_error().decode()
        assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) == BAD_DESC


def test_a_geometry_descriptor_is_no_backward_descriptor():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, _lib.FLAG_GEOMETRY)
    assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) == BAD_DESC


@pytest.mark.parametrize("arith", ("default", "f16x1"))
def test_the_geometry_workspace_is_strictly_smaller(arith):
    from snerf_amd import _lib
    n = 0
    for spec in _specs():
        if arith == "f16x1" and spec.n_freq == 0:
            continue      # raw xyz in one plane is refused (tests/test_abi_cpu.py)
        fl = _lib.FLAG_F16X1 if arith == "f16x1" else 0
        for N, S in ((1, 1), (130, 3), (130, 130), (4096, 64), (4096, 128)):
            full = _lib.call_size("snerf_workspace_bytes", spec.desc(N, S, fl))
            geo = _lib.call_size("snerf_workspace_bytes", spec.desc(N, S, fl | _lib.FLAG_GEOMETRY))
            assert 0 < geo < full, (spec, N, S, geo, full)
            # the packed parameters are the model's: the same buffer serves both passes
            assert _lib.call_size("snerf_packed_floats", spec.desc(N, S, fl | _lib.FLAG_GEOMETRY)) == _lib.call_size("snerf_packed_floats", spec.desc(N, S, fl))
            n += 1
    assert n >= 20


HEAD_FIELDS = ("rgb", "albedo", "sun", "sky", "beta", "beta_semantic", "semantic_logits", "semantic_label")
GEOMETRY_FIELDS = ("depth", "weights", "transparency", "sigmas", "z_vals")


def _call_forward(flags, out_field=None, sun_and_t=True, ws_bytes=None):
    """snerf_forward with addresses nobody may read (host memory for the workspace, made-up numbers elsewhere): every refusal
    checked here returns on the host"""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, flags)
    nbytes = L.snerf_workspace_bytes(C.byref(d))
    assert nbytes > 0
    raw = (C.c_char * 1024)()
    ws = (C.addressof(raw) + 255) & ~255
    si, so = _lib.SnerfInputs(), _lib.SnerfOutputs()
    si.sun_stride = 3
    if sun_and_t:
        si.sun_d, si.t = 0x1000, 0x2000
    if out_field is not None:
        setattr(so, out_field, 0x3000)
    rc = L.snerf_forward(C.byref(d), C.c_void_p(0x100000), C.byref(si), C.byref(so), C.c_void_p(ws), nbytes if ws_bytes is None else ws_bytes, None)
    return rc, L.snerf_last_error().decode()


def test_the_struct_has_the_fields_this_file_lists():
    from snerf_amd import _lib
    assert {n for n, _ in _lib.SnerfOutputs._fields_} == set(HEAD_FIELDS) | set(GEOMETRY_FIELDS)


@pytest.mark.parametrize("field", HEAD_FIELDS)
@pytest.mark.parametrize("arith", ("default", "f16x1"))
def test_a_head_result_is_refused_by_name_before_any_launch(field, arith):
    from snerf_amd import _lib
    rc, msg = _call_forward(_lib.FLAG_GEOMETRY | (_lib.FLAG_F16X1 if arith == "f16x1" else 0), field)
    assert rc == BAD_DESC
    assert "SNERF_FLAG_GEOMETRY" in msg and f"out->{field} " in msg, msg


@pytest.mark.parametrize("field", GEOMETRY_FIELDS)
def test_a_geometry_result_passes_the_output_check(field):
    """... and the call then stops at the next host check: rays are missing (sun_d and t are NULL too, and are not asked for)"""
    from snerf_amd import _lib
    rc, msg = _call_forward(_lib.FLAG_GEOMETRY, field, sun_and_t=False)
    assert rc == 3 and "rays or xyz is required" in msg, (rc, msg)      # SNERF_ERR_NULL


def test_other_passes_still_ask_for_sun_and_t():
    rc, msg = _call_forward(0, "depth", sun_and_t=False)
    assert rc == 3 and "sun_d" in msg, (rc, msg)


def test_a_geometry_pass_checks_its_own_smaller_size():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    geo = _lib.call_size("snerf_workspace_bytes", ModelSpec().desc(64, 8, _lib.FLAG_GEOMETRY))
    rc, msg = _call_forward(_lib.FLAG_GEOMETRY, "depth", ws_bytes=geo - 1)
    assert rc == 2 and "workspace too small" in msg      # SNERF_ERR_WORKSPACE
    rc, msg = _call_forward(_lib.FLAG_GEOMETRY, "depth", ws_bytes=geo)
    assert rc == 3 and "rays or xyz" in msg             # past the size check


def test_render_pass_into_names_the_key():
    from snerf_amd import ops
    spec = ops.ModelSpec(fc_units=64, feat_last=32, fc_layers=3, fc_skips=())
    N, S = 5, 13
    pin = ops.PassInputs(rays=torch.zeros(N, 8), z_steps=torch.zeros(S))
    assert ops.GEOMETRY_KEYS == ("depth", "weights", "transparency", "sigmas", "z_vals")
    for key, shape in (("rgb", (N, 3)), ("sun", (N, S, 1)), ("semantic_label", (N,)), ("nonsense", (N,))):
        with pytest.raises(KeyError, match=f"'{key}' is not a result of a geometry pass"):
            ops.render_pass_into(spec, {}, pin, None, None, {"depth": torch.zeros(N), key: torch.zeros(shape)}, geometry=True)
        with pytest.raises(KeyError, match=f"'{key}' is not a result of a geometry pass"):
            ops.geometry_pass_into(spec, {}, pin, {key: torch.zeros(shape)})
    with pytest.raises(ValueError, match="solar-correction"):
        ops.render_pass_into(spec, {}, pin, None, None, {"weights": torch.zeros(N, S)}, sc_pass=True, geometry=True)
    with pytest.raises(ValueError, match="t .* is required"):      # t = None is the geometry pass's alone
        ops.render_pass_into(spec, {}, pin, None, None, {"depth": torch.zeros(N)})


def test_fused_model_rendering_into_names_the_key():
    from snerf_amd.semantic.components.rendering import fused_model_rendering_into
    for key, shape in (("rgb", (3, 3)), ("sun_sc", (3, 8, 1)), ("weights_sc", (3, 8))):
        with pytest.raises(KeyError, match=f"'{key}' is not a result of a geometry pass"):
            fused_model_rendering_into(None, {}, "coarse", torch.zeros(3, 8), torch.zeros(3, 4), {"geometry_only": True},
                                       {"depth": torch.zeros(3), key: torch.zeros(shape)})


def test_importance_depths_names_a_bad_proposal_kind():
    from snerf_amd.semantic.components.rendering import importance_depths
    renderer = types.SimpleNamespace(N_samples=7, N_importance=5)
    model = types.SimpleNamespace(spec=None)
    with pytest.raises(ValueError, match="proposal_pass"):
        importance_depths(renderer, {"coarse": model}, "coarse", torch.zeros(3, 8), torch.zeros(3, 4), {"proposal_pass": "fast"})


class _StubRenderer:
    """records what the walk asks of every chunk; touches no device"""

    def __init__(self):
        self.calls = []

    def render_rays_into(self, models, rays, extras, out, render_options):
        self.calls.append(("render", rays.shape[0], tuple(sorted(out)), bool(render_options.get("geometry_only"))))
        return "ws"

    def relight_rays_into(self, models, extras, out, render_options):
        assert render_options["workspace"] == "ws"
        self.calls.append(("relight", extras.shape[0], tuple(sorted(out)), bool(render_options.get("geometry_only"))))
        return "ws"


def _walk_fixture(monkeypatch):
    from snerf_amd import ops
    from snerf_amd.ops import ModelSpec
    monkeypatch.setattr(ops, "pack_params", lambda spec, params: None)
    model = types.SimpleNamespace(spec=ModelSpec(), named_parameters=lambda: [])
    cfgs = types.SimpleNamespace(pipeline=types.SimpleNamespace(render_chunk_size=128, n_samples=8, n_importance=0))
    return cfgs, _StubRenderer(), {"coarse": model}, torch.zeros(300, 8), torch.zeros(300, 4)


def test_lean_inference_picks_the_geometry_pass_for_geometry_keys_alone(monkeypatch):
    from snerf_amd.eval.utils.util import lean_inference
    cfgs, r, models, rays, extras = _walk_fixture(monkeypatch)
    out = lean_inference(cfgs, r, models, rays, extras, keys=("depth_coarse",))
    assert out["depth_coarse"].shape == (300,)
    assert r.calls == [("render", 128, ("depth_coarse",), True), ("render", 128, ("depth_coarse",), True), ("render", 44, ("depth_coarse",), True)]
    r.calls.clear()
    lean_inference(cfgs, r, models, rays, extras, keys=("depth_coarse", "weights_coarse", "transparency_coarse", "sigmas_coarse"))
    assert [c[3] for c in r.calls] == [True] * 3
    r.calls.clear()
    lean_inference(cfgs, r, models, rays, extras)      # the default three keys: rgb and the label need the heads
    assert [c[3] for c in r.calls] == [False] * 3
    for keys in (("depth_coarse", "rgb_coarse"), ("depth_coarse", "sun_coarse"), ("weights_coarse", "weights_sc_coarse")):
        r.calls.clear()
        lean_inference(cfgs, r, models, rays, extras, keys=keys)
        assert [c[3] for c in r.calls] == [False] * 3, keys


def test_a_sweep_never_picks_the_geometry_pass(monkeypatch):
    """its base pass must leave a workspace that can be relit, whatever the keys"""
    from snerf_amd.eval.utils import util
    cfgs, r, models, rays, extras = _walk_fixture(monkeypatch)
    monkeypatch.setattr(util, "sun_extras", lambda e, sun, device=None: e)
    out = util.lean_relight(cfgs, r, models, rays, extras, [(60.0, 120.0), (40.0, 200.0)], keys=("depth_coarse",))
    assert out["depth_coarse"].shape == (2, 300)
    assert [c[0] for c in r.calls] == ["render", "relight"] * 3 and not any(c[3] for c in r.calls)
    r.calls.clear()
    util.lean_relight(cfgs, r, models, rays, extras, [(60.0, 120.0)], keys=("depth_coarse",))      # one explicit sun: still a sweep's base pass
    assert [c[0] for c in r.calls] == ["render"] * 3 and not any(c[3] for c in r.calls)


def test_extract_pointcloud_asks_for_the_depth_alone(monkeypatch):
    from snerf_amd.eval import extract_pointcloud as E
    cfgs, r, models, rays, extras = _walk_fixture(monkeypatch)
    out = E.extract_pointcloud(cfgs, r, models, rays, extras, with_colors=False, with_labels=False)
    assert "colors" not in out and "labels" not in out and out["xyz_n"].shape == (300, 3) and out["xyz_n"].dtype == torch.float64
    assert [c[2:] for c in r.calls] == [(("depth_coarse",), True)] * 3
    r.calls.clear()
    out = E.extract_pointcloud(cfgs, r, models, rays, extras)
    assert "colors" in out and "labels" in out
    assert [c[2:] for c in r.calls] == [(("depth_coarse", "rgb_coarse", "semantic_label_coarse"), False)] * 3
    r.calls.clear()
    out = E.extract_pointcloud(cfgs, r, models, rays, extras, with_colors=False)      # labels need the semantic head
    assert "colors" not in out and "labels" in out and not any(c[3] for c in r.calls)
