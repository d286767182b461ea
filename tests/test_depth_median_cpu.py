"""Host side of the median depth (SNERF_FLAG_DEPTH_MEDIAN): the flag on the frozen ABI 6, the plan's refusals,
the sizes, the NULL outputs, the numpy restatement (tests/raymedian_numpy.py) against exact rational arithmetic, and the host
plumbing of depth_mode from ops up to the evaluators.  Every check returns before any launch: no GPU work."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import raymedian_numpy as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_hip.h")
BAD_DESC, ERR_NULL = 1, 3      # SNERF_ERR_BAD_DESC, SNERF_ERR_NULL


# ---- header and binding -----------------------------------------------------------------------------------------------------
def test_flag_mirrors_the_header_and_shares_no_bit():
    from snerf_amd import _lib
    text = open(HEADER).read()
    value = int(re.search(r"#define\s+SNERF_FLAG_DEPTH_MEDIAN\s+(\d+)u", text).group(1))
    assert _lib.FLAG_DEPTH_MEDIAN == value == 128
    others = (_lib.FLAG_TRAIN, _lib.FLAG_SC_PASS, _lib.FLAG_RELIGHT, _lib.FLAG_EMBED_GRAD, _lib.FLAG_GEOMETRY, _lib.FLAG_F16X1,
              _lib.FLAG_F16X2)
    assert len(set(others)) == 7 and all(value & f == 0 for f in others)
    for name, f in zip(("TRAIN", "SC_PASS", "RELIGHT", "EMBED_GRAD", "GEOMETRY", "F16X1", "F16X2"), others):
        assert int(re.search(rf"#define\s+SNERF_FLAG_{name}\s+(\d+)u", text).group(1)) == f


def test_abi_version_and_descriptor_size_stay():
    from snerf_amd import _lib
    assert re.search(r"#define\s+SNERF_ABI_VERSION\s+6\b", open(HEADER).read())
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    assert C.sizeof(_lib.SnerfDesc) == 64


# ---- plan refusals -----------------------------------------------------------------------------------------------------------
def _variant_specs():
    """the model variants tests/test_abi_cpu.py walks the plan builder over"""
    from snerf_amd.ops import ModelSpec
    return [ModelSpec(**kw) for kw in ({}, {"siren": False}, {"use_separate_beta_for_s": True}, {"use_tj_for_s": True},
                                       {"use_tj_instead_of_beta": True}, {"fc_units": 64},
                                       {"fc_units": 128, "fc_layers": 4, "fc_skips": (2,)})]


@pytest.mark.parametrize("other", ("TRAIN", "SC_PASS", "TRAIN|EMBED_GRAD"))
def test_the_bit_is_refused_with_the_passes_that_have_no_median(other):
    """by the plan: hence by the size entries and both hot calls, before they look at a pointer"""
    from snerf_amd import _lib
    L = _lib.lib()
    extra = 0
    for name in other.split("|"):
        extra |= getattr(_lib, "FLAG_" + name)
    for spec in _variant_specs():
        for arith in (0, _lib.FLAG_F16X1):
            d = spec.desc(64, 8, _lib.FLAG_DEPTH_MEDIAN | extra | arith)
            assert L.snerf_workspace_bytes(C.byref(d)) == 0
            assert b"SNERF_FLAG_DEPTH_MEDIAN" in L.snerf_last_error(), L.snerf_last_error()
            assert L.snerf_packed_floats(C.byref(d)) == 0 and L.snerf_grad_floats(C.byref(d)) == 0
            assert L.snerf_forward(C.byref(d), None, None, None, None, 0, None) == BAD_DESC
            assert b"SNERF_FLAG_DEPTH_MEDIAN" in L.snerf_last_error()
            assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) == BAD_DESC
            assert b"SNERF_FLAG_DEPTH_MEDIAN" in L.snerf_last_error()


def test_backward_refuses_the_bit_on_an_inference_descriptor():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, _lib.FLAG_DEPTH_MEDIAN)
    assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) == BAD_DESC
    assert b"SNERF_FLAG_DEPTH_MEDIAN" in L.snerf_last_error()


def test_the_sample_limit():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    for extra in (0, _lib.FLAG_GEOMETRY, _lib.FLAG_RELIGHT):
        d = ModelSpec().desc(16, 1025, _lib.FLAG_DEPTH_MEDIAN | extra)
        assert L.snerf_workspace_bytes(C.byref(d)) == 0
        msg = L.snerf_last_error()
        assert b"SNERF_FLAG_DEPTH_MEDIAN" in msg and b"n_samples" in msg, msg
        assert L.snerf_forward(C.byref(d), None, None, None, None, 0, None) == BAD_DESC
        assert L.snerf_workspace_bytes(C.byref(ModelSpec().desc(16, 1024, _lib.FLAG_DEPTH_MEDIAN | extra))) > 0, L.snerf_last_error()


# ---- sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("plain", "GEOMETRY", "RELIGHT"))
def test_the_sizes_ignore_the_bit(kind):
    from snerf_amd import _lib
    base = 0 if kind == "plain" else getattr(_lib, "FLAG_" + kind)
    n = 0
    for spec in _variant_specs():
        for arith in (0, _lib.FLAG_F16X1):
            for N, S in ((1, 1), (77, 7), (4096, 64), (2048, 130)):
                for entry in ("snerf_workspace_bytes", "snerf_packed_floats", "snerf_grad_floats"):
                    without = _lib.call_size(entry, spec.desc(N, S, base | arith))
                    assert _lib.call_size(entry, spec.desc(N, S, base | arith | _lib.FLAG_DEPTH_MEDIAN)) == without > 0, (entry, spec, N, S)
                    n += 1
    assert n == 7 * 2 * 4 * 3


# ---- NULL outputs ------------------------------------------------------------------------------------------------------------
def _call_forward(flags, missing):
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
    si.sun_d, si.t = 0x1000, 0x2000
    for k, field in enumerate(("depth", "weights", "z_vals")):
        if field != missing:
            setattr(so, field, 0x3000 + 0x1000 * k)
    rc = L.snerf_forward(C.byref(d), C.c_void_p(0x100000), C.byref(si), C.byref(so), C.c_void_p(ws), nbytes, None)
    return rc, L.snerf_last_error().decode()


@pytest.mark.parametrize("field", ("weights", "z_vals", "depth"))
@pytest.mark.parametrize("kind", ("plain", "GEOMETRY", "F16X1"))
def test_a_missing_output_is_refused_by_name_before_any_launch(field, kind):
    from snerf_amd import _lib
    rc, msg = _call_forward(_lib.FLAG_DEPTH_MEDIAN | (0 if kind == "plain" else getattr(_lib, "FLAG_" + kind)), field)
    assert rc == ERR_NULL, (rc, msg)
    assert "SNERF_FLAG_DEPTH_MEDIAN" in msg and f"out->{field} " in msg, msg


def test_with_all_three_the_call_reaches_the_next_host_check():
    from snerf_amd import _lib
    rc, msg = _call_forward(_lib.FLAG_DEPTH_MEDIAN, None)
    assert rc == ERR_NULL and "rays or xyz is required" in msg, (rc, msg)
    rc, msg = _call_forward(0, "weights")      # without the bit nothing asks for the three
    assert rc == ERR_NULL and "rays or xyz is required" in msg, (rc, msg)


# ---- the restatement against exact arithmetic -----------------------------------------------------------------------------------
def _round_f32(x: Fraction) -> np.float32:
    """x correctly rounded to fp32 (ties to even do not occur for the candidates compared here: the nearest of three neighbours)"""
    c = np.float32(float(x))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    return min((v for v in cands if np.isfinite(v)), key=lambda v: abs(Fraction(float(v)) - x))


def _exact(w32, z32):
    """one ray in Python integers and Fractions: -> (j or -1, the exact median as a Fraction or None)"""
    a = [int(v) for v in RM.masses(w32[None])[0]]
    AT, S = sum(a), len(a)
    if AT == 0:
        return -1, Fraction(float(z32[S - 1]))
    A = 0
    for j in range(S):
        if 2 * (A + a[j]) >= AT:
            break
        A += a[j]
    assert a[j] > 0
    if j == S - 1:
        return j, Fraction(float(z32[S - 1]))
    zj, zn = Fraction(float(z32[j])), Fraction(float(z32[j + 1]))
    return j, zj + Fraction(AT - 2 * A, 2 * a[j]) * (zn - zj)


def _random_rays(rng, N, S):
    """weights of a composite along sorted depths: thin haze, one or two opaque lobes, rays that do not saturate"""
    z = np.sort(rng.uniform(0.5, 9.5, (N, S)).astype(np.float32), axis=1)
    sigma = rng.uniform(0.0, 0.3, (N, S))
    for r in range(N):
        for _ in range(int(rng.integers(0, 3))):
            c = int(rng.integers(0, S))
            sigma[r, c:c + 1 + int(rng.integers(0, 3))] += rng.uniform(0.5, 40.0)
    delta = np.diff(z.astype(np.float64), axis=1, append=1e10)
    alpha = 1.0 - np.exp(-sigma * delta)
    T = np.cumprod(np.concatenate([np.ones((N, 1)), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    return (alpha * T).astype(np.float32), z


@pytest.mark.parametrize("S", (1, 2, 3, 63, 64, 65, 130, 1024))
def test_the_restatement_equals_exact_arithmetic(S):
    rng = np.random.default_rng(1000 + S)
    N = 24
    w, z = _random_rays(rng, N, S)
    depth, jj = RM.ray_median(w, z, return_index=True)
    assert depth.dtype == np.float32 and depth.shape == (N,)
    for r in range(N):
        j, x = _exact(w[r], z[r])
        assert jj[r] == j, (S, r, jj[r], j)
        c = _round_f32(x)
        assert np.nextafter(c, np.float32(-np.inf)) <= depth[r] <= np.nextafter(c, np.float32(np.inf)), (S, r, depth[r], c)
        if j >= 0 and j < S - 1:
            assert z[r, j] <= depth[r] <= z[r, j + 1], (S, r, j, depth[r])
        else:
            assert depth[r] == z[r, S - 1]


def _one(w, z):
    return RM.ray_median(np.asarray([w], np.float32), np.asarray([z], np.float32), return_index=True)


def test_fixed_cases():
    z = [1.0, 2.0, 4.0]
    d, j = _one([0.0, -0.0, 0.0], z)                      # nothing on the ray: the far end
    assert d[0] == np.float32(4.0) and j[0] == -1
    d, j = _one([0.0, 0.0, 0.7], z)                       # all mass in the last (open-ended) sample: its near edge
    assert d[0] == np.float32(4.0) and j[0] == 2
    d, j = _one([0.9, 0.0, 0.0], z)                       # all mass in the first: the middle of its interval
    assert d[0] == np.float32(1.5) and j[0] == 0
    d, j = _one([0.5, 0.5, 0.0], z)                       # an exact tie: frac = 1 of interval 0, i.e. z_1
    assert d[0] == np.float32(2.0) and j[0] == 0
    d, j = _one([0.25, 0.5, 0.25], z)                     # the median in the middle of interval 1
    assert d[0] == np.float32(3.0) and j[0] == 1
    d, j = _one([0.1, 0.8, 0.1], [1.0, 3.0, 3.0])         # equal neighbouring depths: an interval of no length
    assert d[0] == np.float32(3.0) and j[0] == 1
    d, j = _one([-5.0, 7.0, 0.25], z)                     # weights below 0 and above 1 are clamped to 0 and 1: masses 0, 1, 0.25
    assert j[0] == 1 and d[0] == np.float32(2.0 + (1.25 / 2.0) * 2.0)
    d, j = _one([0.2, np.nan, 0.2], z)                    # a NaN weight
    assert np.isnan(d[0]) and j[0] == -1
    d, j = _one([0.2, 0.2, 0.2], [1.0, np.inf, np.inf])   # a depth that is not finite
    assert np.isnan(d[0])
    d, j = _one([0.2, 0.2, 0.2], [1.0, 3.0, 2.0])         # a decreasing depth
    assert np.isnan(d[0]) and j[0] == -1
    # a sigma that is not finite, where the launch is handed the sigmas: the pass gives such a ray zero weights
    zz = np.asarray([z], np.float32)
    assert RM.ray_median(np.zeros((1, 3), np.float32), zz)[0] == np.float32(4.0)
    assert np.isnan(RM.ray_median(np.zeros((1, 3), np.float32), zz, np.asarray([[0.5, np.nan, 0.5]], np.float32))[0])
    assert np.isnan(RM.ray_median(np.asarray([[0.9, 0, 0]], np.float32), zz, np.asarray([[np.inf, 0, 0]], np.float32))[0])
    assert RM.ray_median(np.asarray([[0.9, 0, 0]], np.float32), zz, np.asarray([[3.0, 0, 0]], np.float32))[0] == np.float32(1.5)
    d, j = _one([0.3], [2.5])                             # S = 1
    assert d[0] == np.float32(2.5) and j[0] == 0
    # a bad ray leaves its neighbours alone
    d = RM.ray_median(np.asarray([[0.9, 0, 0], [np.nan, 0, 0], [0.9, 0, 0]], np.float32), np.asarray([z] * 3, np.float32))
    assert d[0] == d[2] == np.float32(1.5) and np.isnan(d[1])


def test_the_result_is_the_median_of_the_normalised_weight():
    """a ray that does not saturate has the median of its own total: scaling every weight by a power of two moves nothing"""
    rng = np.random.default_rng(7)
    w, z = _random_rays(rng, 16, 65)
    assert np.array_equal(RM.ray_median(w, z), RM.ray_median(w * np.float32(0.25), z))


# ---- host plumbing -----------------------------------------------------------------------------------------------------------
def test_ops_entries_refuse_an_unknown_mode_before_anything_is_sized():
    from snerf_amd import ops
    assert ops.DEPTH_MODES == ("mean", "median")
    out = {"depth": torch.zeros(4)}
    for mode in ("mode", "Median", None, 1):
        with pytest.raises(ValueError, match="depth_mode"):
            ops.render_pass_into(None, {}, None, None, None, out, depth_mode=mode)
        with pytest.raises(ValueError, match="depth_mode"):
            ops.geometry_pass_into(None, {}, None, out, depth_mode=mode)
        with pytest.raises(ValueError, match="depth_mode"):
            ops.relight_pass_into(None, {}, None, None, None, out, None, depth_mode=mode)


def test_ops_refuses_the_median_of_a_solar_correction_pass_and_a_missing_depth():
    from snerf_amd import ops
    with pytest.raises(ValueError, match="solar-correction"):
        ops.render_pass_into(None, {}, None, None, None, {"weights": torch.zeros(4, 8)}, sc_pass=True, depth_mode="median")
    for out in ({}, {"weights": torch.zeros(4, 8), "z_vals": torch.zeros(4, 8)}, {"rgb": torch.zeros(4, 3)}):
        with pytest.raises(KeyError, match="depth"):
            ops.render_pass_into(None, {}, None, None, None, out, depth_mode="median")
        with pytest.raises(KeyError, match="depth"):
            ops.geometry_pass_into(None, {}, None, out, depth_mode="median")
        with pytest.raises(KeyError, match="depth"):
            ops.relight_pass_into(None, {}, None, None, None, out, None, depth_mode="median")


def test_the_training_entry_does_not_take_the_mode():
    import inspect
    from snerf_amd import ops
    assert "depth_mode" not in inspect.signature(ops.render_pass).parameters
    for f in (ops.render_pass_into, ops.geometry_pass_into, ops.relight_pass_into):
        p = inspect.signature(f).parameters
        assert p["depth_mode"].default == "mean" and p["scratch"].default is None


def _renderer():
    from snerf_amd.semantic.components.rendering import RSSemanticRendering
    cfgs = types.SimpleNamespace(pipeline=types.SimpleNamespace(n_samples=8, n_importance=0, sc_lambda=0.0))
    return RSSemanticRendering(cfgs)


def test_the_renderer_refuses_an_unknown_mode_and_a_training_render_with_the_median():
    r = _renderer()
    rays, extras = torch.zeros(3, 8), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="depth_mode"):
        r.render_rays_into({}, rays, extras, {"depth_coarse": torch.zeros(3)}, {"depth_mode": "mode"})
    with pytest.raises(ValueError, match="depth_mode"):
        r.relight_rays_into({}, extras, {"depth_coarse": torch.zeros(3)}, {"depth_mode": "mode"})
    with pytest.raises(ValueError, match="depth_mode"):
        r.render_rays({}, rays, extras, render_options={"depth_mode": "mode"})
    with pytest.raises(ValueError, match="median.*inference"):      # render_rays is the differentiable render
        r.render_rays({}, rays, extras, render_options={"depth_mode": "median"})
    from snerf_amd.baseline.components.rendering import SatNeRFRendering
    with pytest.raises(ValueError, match="median.*inference"):
        SatNeRFRendering(r.cfgs).render_rays({}, rays, extras, render_options={"depth_mode": "median"})
    from snerf_amd.semantic.components.rendering import fused_model_rendering
    with pytest.raises(ValueError, match="median"):
        fused_model_rendering(r, {}, "coarse", rays, extras, {"depth_mode": "median"}, None, None)


def test_fit_image_embedding_refuses_the_median():
    from snerf_amd.eval.utils.embedding import fit_image_embedding
    with pytest.raises(ValueError, match="median"):
        fit_image_embedding(None, None, {}, None, None, None, steps=1, lr=0.1, rays_per_fit=1, render_options={"depth_mode": "median"})


def test_the_walk_hands_the_mode_and_one_scratch_dict_to_every_pass(monkeypatch):
    from snerf_amd import ops
    from snerf_amd.eval.utils import util
    from snerf_amd.ops import ModelSpec
    monkeypatch.setattr(ops, "pack_params", lambda spec, params: None)
    monkeypatch.setattr(util, "sun_extras", lambda e, sun, device=None: e)
    seen = []

    class Stub:
        def render_rays_into(self, models, rays, extras, out, render_options):
            seen.append(("render", render_options.get("depth_mode"), render_options.get("depth_scratch"), bool(render_options.get("geometry_only"))))
            return "ws"

        def relight_rays_into(self, models, extras, out, render_options):
            seen.append(("relight", render_options.get("depth_mode"), render_options.get("depth_scratch"), False))
            return "ws"

    model = types.SimpleNamespace(spec=ModelSpec(), named_parameters=lambda: [])
    cfgs = types.SimpleNamespace(pipeline=types.SimpleNamespace(render_chunk_size=128, n_samples=8, n_importance=0))
    rays, extras = torch.zeros(300, 8), torch.zeros(300, 4)
    util.lean_inference(cfgs, Stub(), {"coarse": model}, rays, extras, keys=("depth_coarse",), render_options={"depth_mode": "median"})
    assert [s[0] for s in seen] == ["render"] * 3 and all(s[1] == "median" and s[3] for s in seen)      # the automatic geometry walk
    assert isinstance(seen[0][2], dict) and all(s[2] is seen[0][2] for s in seen)
    seen.clear()
    util.lean_relight(cfgs, Stub(), {"coarse": model}, rays, extras, [(60.0, 120.0), (40.0, 200.0)], keys=("depth_coarse",),
                      render_options={"depth_mode": "median"})
    assert [s[0] for s in seen] == ["render", "relight"] * 3 and all(s[1] == "median" for s in seen)
    assert all(s[2] is seen[0][2] for s in seen)
    seen.clear()
    util.lean_inference(cfgs, Stub(), {"coarse": model}, rays, extras, keys=("depth_coarse",))      # the default: nothing rides along
    assert all(s[1] is None and s[2] is None for s in seen) and len(seen) == 3
    with pytest.raises(ValueError, match="depth_mode"):
        util.lean_inference(cfgs, Stub(), {"coarse": model}, rays, extras, keys=("depth_coarse",), render_options={"depth_mode": "mode"})


def test_with_depth_mode_leaves_the_default_alone():
    from snerf_amd.eval.utils.util import with_depth_mode
    ro = {"perturb": 0}
    assert with_depth_mode(ro, "mean") is ro and with_depth_mode(None, "mean") is None
    got = with_depth_mode(ro, "median")
    assert got == {"perturb": 0, "depth_mode": "median"} and ro == {"perturb": 0}
    with pytest.raises(ValueError, match="depth_mode"):
        with_depth_mode(ro, "mode")


def test_consumers_take_the_mode_and_default_to_the_mean():
    import inspect
    from snerf_amd.eval import eval_nerf, extract_pointcloud
    from snerf_amd.eval.utils import ortho
    from snerf_amd.framework import visualize
    for f in (extract_pointcloud.extract_pointcloud, ortho.ortho_products, ortho.nadir_products, ortho.nadir_sun_sweep,
              eval_nerf.eval_nerf_images, visualize.run_visualizer):
        assert inspect.signature(f).parameters["depth_mode"].default == "mean", f


def test_extract_pointcloud_hands_the_mode_down(monkeypatch):
    from snerf_amd.eval import extract_pointcloud as E
    got = []

    def infer(cfgs, renderer, models, rays, extras, keys, render_options):
        got.append((tuple(keys), dict(render_options)))
        return {"depth_coarse": torch.ones(rays.shape[0])}

    monkeypatch.setattr(E, "lean_inference", infer)
    models = {"coarse": types.SimpleNamespace(spec=types.SimpleNamespace(n_classes=0))}
    rays = torch.zeros(5, 8)
    E.extract_pointcloud(None, None, models, rays, None, with_colors=False, with_labels=False)
    E.extract_pointcloud(None, None, models, rays, None, {"perturb": 0}, with_colors=False, with_labels=False, depth_mode="median")
    assert got == [(("depth_coarse",), {}), (("depth_coarse",), {"perturb": 0, "depth_mode": "median"})]
    with pytest.raises(ValueError, match="depth_mode"):
        E.extract_pointcloud(None, None, models, rays, None, depth_mode="mode")


def test_config_default_and_validation_options():
    from snerf_amd.baseline.pipelines.base_ray_pipeline import BaseRayPipeline
    from snerf_amd.framework.configs import MainConfig
    pl = {"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64}
    cfgs = MainConfig(run={"max_train_steps": 10, "synthetic_rays": 4096}, pipeline=dict(pl))
    assert cfgs.pipeline.depth_mode == "mean" and "depth_mode" not in cfgs.pipeline.model_fields_set
    assert BaseRayPipeline._val_render_options(types.SimpleNamespace(cfgs=cfgs), "test") == {}
    med = MainConfig(run={"max_train_steps": 10, "synthetic_rays": 4096}, pipeline=dict(pl, depth_mode="median"))
    assert med.pipeline.depth_mode == "median"
    assert BaseRayPipeline._val_render_options(types.SimpleNamespace(cfgs=med), "val") == {"depth_mode": "median"}
    with pytest.raises(Exception, match="depth_mode"):
        MainConfig(run={"max_train_steps": 10, "synthetic_rays": 4096}, pipeline=dict(pl, depth_mode="mode"))


def test_eval_nerf_images_names_the_mode_only_when_it_is_not_the_mean(monkeypatch):
    from snerf_amd.eval import eval_nerf as E
    got = []

    def infer(cfgs, renderer, models, rays, extras, keys, render_options={}):
        got.append(dict(render_options))
        return {"rgb_coarse": torch.zeros(rays.shape[0], 3), "depth_coarse": torch.ones(rays.shape[0])}

    monkeypatch.setattr(E, "lean_inference", infer)
    monkeypatch.setattr(E, "metrics", types.SimpleNamespace(psnr=lambda *a, **k: 20.0, ssim=lambda *a, **k: 0.5))
    img = {"name": "a", "rays": torch.zeros(16, 8), "extras": torch.zeros(16, 4), "rgbs": torch.zeros(16, 3), "w": 4, "h": 4}
    d = E.eval_nerf_images(None, None, {}, [img], split="val")
    assert "depth_mode" not in d and got == [{}]
    assert d == {"a": {"psnr": "20.00", "ssim": "0.500"}, "PSNR (Mean)": "20.00", "SSIM (Mean)": "0.500"}
    d = E.eval_nerf_images(None, None, {}, [img], split="val", depth_mode="median")
    assert d["depth_mode"] == "median" and got[1] == {"depth_mode": "median"}
    with pytest.raises(ValueError, match="depth_mode"):
        E.eval_nerf_images(None, None, {}, [img], split="val", depth_mode="mode")
