"""SNERF_FLAG_EMBED_GRAD and the embedding fit, host side: every check returns before any launch (no GPU here).

The flag rides on the frozen ABI 6: a new bit of SnerfDesc.flags and the d_t / d_t_s slots snerf_backward already has -- no
prototype, no struct field, no version change.  The refusals are make_plan's and snerf_backward's argument checks; the driver
checks are the pure host logic of eval/utils/embedding.py (region masks, init modes, the seeded subset, best-iterate selection)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every symbol include/snerf_hip.h declares at ABI 6: those from before the flag (the flag adds none), the two cast-shadow entries,
# and the two per-ray entries snerf_resample_z and snerf_ray_distortion, whose declarations moved here from headers of their own
# (the library exported them already: the version did not move)
ABI6_SYMBOLS = """snerf_adam_step snerf_backward snerf_dsm_accumulate snerf_dsm_downsample2x snerf_dsm_finish
snerf_dsm_ncc_search snerf_dsm_shift_diff snerf_dsm_workspace_bytes snerf_embedding_backward snerf_embedding_rows
snerf_forward snerf_geo_cloud snerf_geo_points snerf_grad_floats snerf_last_error snerf_loss_finish snerf_loss_partial
snerf_loss_workspace_bytes snerf_normalize_rows snerf_ortho_gather snerf_ortho_top snerf_ortho_votes
snerf_ortho_votes_finish snerf_pack_params snerf_packed_floats snerf_profile_begin snerf_profile_end snerf_ray_bounds
snerf_ray_bounds_workspace_bytes snerf_ray_distortion snerf_resample_z snerf_rpc_localize snerf_rpc_project snerf_rpc_rays snerf_rpc_reprojection_error
snerf_sample_z snerf_semeval_accumulate snerf_semeval_workspace_bytes snerf_shadow_agreement snerf_shadow_cast
snerf_ssim snerf_ssim_workspace_bytes snerf_test_bsp_dw snerf_test_bsp_kc snerf_test_bsp_roundtrip
snerf_test_set_kc_grid snerf_test_set_trunk_fusion snerf_unpack_grads snerf_version snerf_vis_colormap snerf_vis_fold
snerf_vis_minmax snerf_workspace_bytes""".split()


def _header():
    return open(os.path.join(ROOT, "include", "snerf_hip.h")).read()


def test_flag_value_in_header_and_binding():
    from snerf_amd import _lib
    m = re.search(r"#define\s+SNERF_FLAG_EMBED_GRAD\s+(\d+)u", _header())
    assert m and int(m.group(1)) == _lib.FLAG_EMBED_GRAD == 16
    others = (_lib.FLAG_TRAIN, _lib.FLAG_SC_PASS, _lib.FLAG_RELIGHT, _lib.FLAG_F16X1, _lib.FLAG_F16X2)
    assert all(_lib.FLAG_EMBED_GRAD & f == 0 for f in others)


def test_abi_version_and_symbols_unchanged():
    from snerf_amd import _lib
    assert re.search(r"#define\s+SNERF_ABI_VERSION\s+6\b", _header())
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(snerf_[a-z_0-9]+)\s*\(", src)))
    assert declared == sorted(ABI6_SYMBOLS) and len(declared) == 53
    assert C.sizeof(_lib.SnerfDesc) == 16 * 4


def _variant_specs():
    """the model variants of test_abi_cpu.test_plan_builder_over_model_variants_and_null_arguments"""
    from snerf_amd.ops import ModelSpec
    return [ModelSpec(**kw) for kw in ({}, {"siren": False}, {"use_separate_beta_for_s": True}, {"use_tj_for_s": True},
                                       {"use_tj_instead_of_beta": True}, {"fc_units": 64}, {"fc_units": 128, "fc_layers": 4, "fc_skips": (2,)})]


def test_workspace_and_buffer_sizes_ignore_the_bit():
    from snerf_amd import _lib
    L = _lib.lib()
    n = 0
    for spec in _variant_specs():
        for flags in (_lib.FLAG_TRAIN, _lib.FLAG_TRAIN | _lib.FLAG_SC_PASS, _lib.FLAG_TRAIN | _lib.FLAG_F16X1,
                      _lib.FLAG_TRAIN | _lib.FLAG_F16X2, _lib.FLAG_F16X1 | _lib.FLAG_TRAIN | _lib.FLAG_SC_PASS):
            for N, S in ((1, 1), (77, 7), (4096, 64), (2048, 130)):
                d, e = spec.desc(N, S, flags), spec.desc(N, S, flags | _lib.FLAG_EMBED_GRAD)
                for fn in (L.snerf_workspace_bytes, L.snerf_packed_floats, L.snerf_grad_floats):
                    a, b = fn(C.byref(d)), fn(C.byref(e))
                    assert a == b > 0, (spec, flags, N, S, fn.__name__, a, b, L.snerf_last_error())
                n += 1
    assert n == 7 * 5 * 4


@pytest.mark.parametrize("flags,why", [(0, "without TRAIN"), (2, "SC_PASS without TRAIN"), (4, "with RELIGHT"), (8, "F16X1 without TRAIN")])
def test_bit_refused_without_train_or_with_relight(flags, why):
    """SNERF_ERR_BAD_DESC from the plan, hence from the size entries and from both hot calls before they look at a pointer"""
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    d = ModelSpec().desc(64, 8, flags | _lib.FLAG_EMBED_GRAD)
    assert L.snerf_workspace_bytes(C.byref(d)) == 0, why
    assert b"SNERF_FLAG_EMBED_GRAD" in L.snerf_last_error(), L.snerf_last_error()
    assert L.snerf_forward(C.byref(d), None, None, None, None, 0, None) == 1        # SNERF_ERR_BAD_DESC
    assert b"SNERF_FLAG_EMBED_GRAD" in L.snerf_last_error()
    assert L.snerf_backward(C.byref(d), None, None, None, None, None, None, None, 0, None) == 1
    assert b"SNERF_FLAG_EMBED_GRAD" in L.snerf_last_error()
    ok = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN | (flags & (2 | 8)) | _lib.FLAG_EMBED_GRAD)
    assert L.snerf_workspace_bytes(C.byref(ok)) > 0, L.snerf_last_error()


# Stand-ins for device pointers: 256-byte aligned, non-NULL, never dereferenced -- each call below is refused on the host (a
# workspace of 0 bytes is too small for any plan), before any launch.
_P = C.c_void_p(0x1000)


def _structs():
    """empty SnerfInputs / SnerfOutGrads for the two struct slots (never read either: the refusal comes first)"""
    from snerf_amd import _lib
    return C.byref(_lib.SnerfInputs()), C.byref(_lib.SnerfOutGrads())


def test_null_packed_grads_passes_the_argument_checks_only_with_the_bit():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    _I, _G = _structs()
    for extra in (0, _lib.FLAG_SC_PASS, _lib.FLAG_F16X1):
        plain = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN | extra)
        flagged = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN | extra | _lib.FLAG_EMBED_GRAD)
        # without the bit: refused as before, as a NULL argument
        assert L.snerf_backward(C.byref(plain), _P, _I, _G, None, _P, _P, _P, 0, None) == 3      # SNERF_ERR_NULL
        assert b"null argument" in L.snerf_last_error()
        # with the bit: the NULL checks pass; the next check (the workspace size) refuses
        assert L.snerf_backward(C.byref(flagged), _P, _I, _G, None, _P, _P, _P, 0, None) == 2    # SNERF_ERR_WORKSPACE
        assert b"workspace too small" in L.snerf_last_error()
        assert L.snerf_backward(C.byref(flagged), _P, _I, _G, None, _P, None, _P, 0, None) == 2  # d_t alone is enough
        assert L.snerf_backward(C.byref(flagged), _P, _I, _G, None, None, _P, _P, 0, None) == 2  # d_t_s alone too
        # the other pointers are still required
        assert L.snerf_backward(C.byref(flagged), None, _I, _G, None, _P, _P, _P, 0, None) == 3
        assert L.snerf_backward(C.byref(flagged), _P, _I, None, None, _P, _P, _P, 0, None) == 3
        assert L.snerf_backward(C.byref(flagged), _P, _I, _G, None, _P, _P, None, 0, None) == 3


def test_bit_with_neither_d_t_nor_d_t_s_is_refused():
    from snerf_amd import _lib
    from snerf_amd.ops import ModelSpec
    L = _lib.lib()
    _I, _G = _structs()
    flagged = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN | _lib.FLAG_EMBED_GRAD)
    for pg in (None, _P):
        assert L.snerf_backward(C.byref(flagged), _P, _I, _G, pg, None, None, _P, 0, None) == 3      # SNERF_ERR_NULL
        assert b"d_t and d_t_s are both NULL" in L.snerf_last_error(), L.snerf_last_error()
    plain = ModelSpec().desc(64, 8, _lib.FLAG_TRAIN)      # the full backward may still be asked for parameter gradients alone
    assert L.snerf_backward(C.byref(plain), _P, _I, _G, _P, None, None, _P, 0, None) == 2


# ---- the fit driver's host logic -----------------------------------------------------------------------------------------------
def test_region_masks_for_odd_and_even_widths():
    from snerf_amd.eval.utils.embedding import region_mask
    for w, h in ((6, 3), (7, 3), (1, 4), (2, 1)):
        m = region_mask(w, h, "left").reshape(h, w)
        assert m.dtype == torch.bool and int(m.sum()) == h * (w // 2)
        assert bool(m[:, :w // 2].all()) and not bool(m[:, w // 2:].any())      # columns [0, w // 2) of every row
        a = region_mask(w, h, "all")
        assert a.shape == (h * w,) and bool(a.all())
    with pytest.raises(ValueError, match="region"):
        region_mask(4, 4, "right")


def test_init_modes():
    from snerf_amd.eval.utils.embedding import initial_vector
    g = torch.Generator().manual_seed(3)
    table = torch.randn(50, 4, generator=g) * 1e3 + 1.0
    mean = initial_vector(table, "mean", n_train=7)
    assert mean.dtype == torch.float32 and torch.equal(mean, table[:7].double().mean(0).float())      # fp64 mean, rounded once
    assert torch.equal(initial_vector(table, "mean"), table.double().mean(0).float())
    assert torch.equal(initial_vector(table, 3), table[3])
    row = initial_vector(table, 0)
    row += 1.0
    assert not torch.equal(row, table[0])                                 # a copy: the table is never edited through it
    v = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    assert torch.equal(initial_vector(table, v), v.float())
    for bad in (50, -1, "median", torch.zeros(5)):
        with pytest.raises(ValueError):
            initial_vector(table, bad)
    with pytest.raises(ValueError):
        initial_vector(table, "mean", n_train=51)


def test_seeded_subset():
    from snerf_amd.eval.utils.embedding import fit_subset, region_mask
    mask = region_mask(10, 6, "left")
    a, b = fit_subset(60, mask, 12, seed=5), fit_subset(60, mask, 12, seed=5)
    assert torch.equal(a, b) and a.dtype == torch.int64 and a.shape == (12,)
    assert len(set(a.tolist())) == 12 and bool(mask[a].all())              # distinct rays, all inside the region
    assert not torch.equal(a, fit_subset(60, mask, 12, seed=6))
    allowed = torch.nonzero(mask).reshape(-1)
    g = torch.Generator().manual_seed(5)
    assert torch.equal(a, allowed[torch.randperm(30, generator=g)[:12]])   # a randperm PREFIX: a larger subset extends a smaller one
    assert torch.equal(fit_subset(60, mask, 20, seed=5)[:12], a)
    assert sorted(fit_subset(60, mask, 1000, seed=0).tolist()) == allowed.tolist()      # fewer allowed rays than asked for: all of them
    assert fit_subset(9, None, 4).shape == (4,)
    with pytest.raises(ValueError):
        fit_subset(60, torch.zeros(60, dtype=torch.bool), 4)
    with pytest.raises(ValueError):
        fit_subset(61, mask, 4)


def test_best_iterate_on_recorded_losses():
    from snerf_amd.eval.utils.embedding import best_iterate
    assert best_iterate([0.5, 0.4, 0.41, 0.3, 0.35]) == 3
    assert best_iterate([0.2, 0.4, 0.3]) == 0                              # the start is an iterate: a fit never reports worse
    assert best_iterate([0.5, 0.3, 0.3]) == 1                              # the earliest of equals
    assert best_iterate([0.5]) == 0
    nan = float("nan")
    assert best_iterate([0.5, nan, 0.4]) == 2 and best_iterate([nan, 0.7, nan]) == 1 and best_iterate([nan, nan]) == 0


def test_fit_options_and_unlisted_views():
    from snerf_amd.eval.utils.embedding import FIT_DEFAULTS, fit_options
    from snerf_amd.baseline.dataset.satnerf_dataset import VAL_T_INDEX, unlisted_test_views
    region, kw = fit_options({})
    assert region == "left" and kw == FIT_DEFAULTS and kw is not FIT_DEFAULTS
    region, kw = fit_options({"region": "all", "steps": 3, "seed": 9})
    assert region == "all" and kw["steps"] == 3 and kw["seed"] == 9 and kw["lr"] == FIT_DEFAULTS["lr"]
    with pytest.raises(ValueError):
        fit_options({"region": "top"})
    names = [f"JAX_068_{i:03d}_RGB.json" for i in (13, 7, 9, 2, 5)]
    assert unlisted_test_views(names) == ["JAX_068_007_RGB.json", "JAX_068_009_RGB.json", "JAX_068_005_RGB.json"]
    assert unlisted_test_views(list(VAL_T_INDEX)) == []
