"""Host side of the relight pass (SNERF_FLAG_RELIGHT): the flag, the sizes and every refusal that happens
before a launch.  No GPU work: the library's host entries run, nothing is dereferenced."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_hip.h")


def test_flag_mirrors_the_header_and_takes_a_free_bit():
    from snerf_amd import _lib
    text = open(HEADER).read()
    value = int(re.search(r"#define SNERF_FLAG_RELIGHT (\d+)u", text).group(1))
    assert _lib.FLAG_RELIGHT == value
    others = [int(v) for v in re.findall(r"#define SNERF_FLAG_(?!RELIGHT)\w+ (\d+)u", text)]
    assert sorted(others) == [1, 2, 8, 64]
    assert value & (value - 1) == 0 and all(value != o for o in others)      # one bit, nobody else's
    assert int(re.search(r"#define SNERF_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 6      # additive: no new version


@pytest.mark.parametrize("arith", ("default", "f16x1"))
def test_a_relight_plans_the_workspace_of_its_base_pass(arith):
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    fl = _lib.FLAG_F16X1 if arith == "f16x1" else 0
    for spec, n, s in ((ModelSpec(), 4096, 64), (ModelSpec(), 96, 8), (ModelSpec(fc_units=64, feat_last=32, fc_layers=3, fc_skips=()), 37, 7)):
        base = _lib.call_size("snerf_workspace_bytes", spec.desc(n, s, fl))
        assert _lib.call_size("snerf_workspace_bytes", spec.desc(n, s, fl | _lib.FLAG_RELIGHT)) == base > 0


@pytest.mark.parametrize("other", ("FLAG_TRAIN", "FLAG_SC_PASS"))
def test_relight_of_a_training_or_solar_correction_pass_is_no_plan(other):
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, _lib.FLAG_RELIGHT | getattr(_lib, other))
    assert L.snerf_workspace_bytes(C.byref(d)) == 0
    assert "SNERF_FLAG_RELIGHT" in L.snerf_last_error().decode()
    assert L.snerf_packed_floats(C.byref(d)) == 0


def test_relight_on_a_workspace_no_pass_has_written_is_refused_before_any_launch():
    """the buffer is host memory at a 256-byte aligned address; packed parameters, inputs and outputs are addresses nobody may
    read: the refusal comes from the note table, on the host"""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, _lib.FLAG_RELIGHT)
    nbytes = L.snerf_workspace_bytes(C.byref(d))
    raw = (C.c_char * 1024)()
    ws = (C.addressof(raw) + 255) & ~255
    si, so = _lib.SnerfInputs(), _lib.SnerfOutputs()
    si.sun_d, si.sun_stride, si.t = 0x1000, 3, 0x2000
    so.rgb = 0x3000
    rc = L.snerf_forward(C.byref(d), C.c_void_p(0x100000), C.byref(si), C.byref(so), C.c_void_p(ws), nbytes, None)
    assert rc == 1                                                   # SNERF_ERR_BAD_DESC
    msg = L.snerf_last_error().decode()
    assert "SNERF_FLAG_RELIGHT" in msg and "no base pass" in msg


def test_relight_pass_into_checks_its_results_before_any_library_call():
    from snerf_amd import ops
    spec = ops.ModelSpec(fc_units=64, feat_last=32, fc_layers=3, fc_skips=())
    N, S = 5, 13
    sun, t, ws = torch.zeros(N, 3), torch.zeros(N, 4), torch.zeros(16, dtype=torch.uint8)
    for key in ("weights_sc", "sun_sc", "nonsense"):
        with pytest.raises(KeyError, match="not a result of this pass"):
            ops.relight_pass_into(spec, {}, sun, t, None, {key: torch.zeros(N, S)}, ws, n_samples=S)
    with pytest.raises(ValueError, match=r"out\['rgb'\] must be a contiguous \(5, 3\)"):
        ops.relight_pass_into(spec, {}, sun, t, None, {"rgb": torch.zeros(N, 4)}, ws, n_samples=S)
    with pytest.raises(ValueError, match=r"out\['weights'\] must be a contiguous \(5, 13\)"):
        ops.relight_pass_into(spec, {}, sun, t, None, {"weights": torch.zeros(N, S + 1)}, ws, n_samples=S)
    with pytest.raises(ValueError, match="n_samples"):      # nothing to take S from
        ops.relight_pass_into(spec, {}, sun, t, None, {"rgb": torch.zeros(N, 3)}, ws)
    with pytest.raises(ValueError, match="dtype"):
        ops.relight_pass_into(spec, {}, sun, t, None, {"rgb": torch.zeros(N, 3, dtype=torch.float64)}, ws, n_samples=S)


def test_renderer_relight_refuses_solar_correction_keys():
    from snerf_amd.semantic.components.rendering import fused_model_relighting_into
    with pytest.raises(KeyError, match="solar-correction"):
        fused_model_relighting_into(None, {}, "coarse", torch.zeros(3, 4), {}, {"sun_sc": torch.zeros(3, 8, 1)})


def test_a_sweep_needs_a_sun():
    from snerf_amd.eval.utils.ortho import nadir_sun_sweep
    from snerf_amd.eval.utils.util import lean_relight
    for suns in ([], None):
        with pytest.raises(ValueError, match="no sun"):
            nadir_sun_sweep(None, None, {}, suns=suns)
    with pytest.raises(ValueError, match="no sun"):
        lean_relight(None, None, {}, torch.zeros(3, 8), torch.zeros(3, 4), [])
