"""ctypes binding of libsnerf_hip.so -- mirrors include/snerf_hip.h field for field."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SNERF_LIB_PATH: an alternative build of the library (ablation harness of tools/ablate; diagnostics only)
LIB_PATH = os.environ.get("SNERF_LIB_PATH") or os.path.join(_HERE, "libsnerf_hip.so")
MAX_LAYERS = 16
ABI_VERSION = 6   # include/snerf_hip.h SNERF_ABI_VERSION

FLAG_TRAIN = 1
FLAG_SC_PASS = 2
FLAG_RELIGHT = 4      # relight of the inference main pass that the workspace holds (include/snerf_hip.h: SNERF_FLAG_RELIGHT)
FLAG_EMBED_GRAD = 16  # snerf_backward writes d_t / d_t_s alone, packed_grads may be NULL (include/snerf_hip.h: SNERF_FLAG_EMBED_GRAD)
FLAG_GEOMETRY = 32    # geometry-only inference pass: trunk + sigma + composite, no head launch (include/snerf_hip.h: SNERF_FLAG_GEOMETRY)
FLAG_DEPTH_MEDIAN = 128  # one launch behind an inference pass rewrites out->depth with the rays' median depth (include/snerf_hip.h: SNERF_FLAG_DEPTH_MEDIAN)
# arithmetic bits of SnerfDesc.flags (include/snerf_hip.h): none set = the default, f16x2
FLAG_F16X2 = 64       # default: fp32-class on the fp16 matrix cores, two fp16 planes of power-of-two-scaled operands, three products
FLAG_F16X1 = 8        # reduced precision: ONE fp16 plane of the same block-scaled tensors, one product (precision = 16 / "medium" / "high")
# ModelSpec.mfma -> SnerfDesc.flags ("bf16" = the name BASELINE.json's configs use for the reduced-precision runs: same mode)
MFMA_FLAGS = {"f16x2": 0, "f16x1": FLAG_F16X1, "bf16": FLAG_F16X1}

_fp = C.POINTER(C.c_float)


class SnerfDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_rays", "n_samples", "fc_units", "fc_layers", "feat_last")] + [
        ("skip_mask", C.c_uint32)] + [(n, C.c_int32) for n in (
            "n_freq", "siren", "t_dim", "n_classes", "sem_sigmoid", "use_tj_instead_of_beta", "use_tj_for_s",
            "use_separate_beta_for_s", "use_separate_tj_for_semantic")] + [("flags", C.c_uint32)]


_PARAM_FIELDS = (["sigma_w", "sigma_b", "feats_w", "feats_b", "rgb_w0", "rgb_b0", "rgb_w2", "rgb_b2",
                  "sem_w0", "sem_b0", "sem_w2", "sem_b2"], ["sky_w0", "sky_b0", "sky_w2", "sky_b2",
                                                             "beta_w0", "beta_b0", "beta_w2", "beta_b2",
                                                             "sbeta_w0", "sbeta_b0", "sbeta_w2", "sbeta_b2"])


class SnerfParams(C.Structure):
    _fields_ = ([("fc_w", C.c_void_p * MAX_LAYERS), ("fc_b", C.c_void_p * MAX_LAYERS)]
                + [(n, C.c_void_p) for n in _PARAM_FIELDS[0]]
                + [("sun_w", C.c_void_p * 4), ("sun_b", C.c_void_p * 4)]
                + [(n, C.c_void_p) for n in _PARAM_FIELDS[1]])


class SnerfInputs(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("xyz", C.c_void_p), ("z_vals", C.c_void_p), ("z_steps", C.c_void_p),
                ("u", C.c_void_p), ("sun_d", C.c_void_p), ("sun_stride", C.c_int32), ("_pad", C.c_int32),
                ("t", C.c_void_p), ("t_s", C.c_void_p)]


OUTPUT_FIELDS = ("rgb", "depth", "weights", "transparency", "albedo", "sun", "sky", "beta", "sigmas",
                 "beta_semantic", "semantic_logits", "semantic_label", "z_vals")
GRAD_FIELDS = ("rgb", "depth", "weights", "transparency", "albedo", "sun", "sky", "beta", "sigmas",
               "beta_semantic", "semantic_logits")


class SnerfOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUTPUT_FIELDS]


class SnerfOutGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in GRAD_FIELDS]


class SnerfLossCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_rays", "n_samples", "n_classes", "color_mode", "has_sc", "sem_mode",
                                          "ignore_index", "use_sbeta", "detach_beta_for_s", "car_reg", "car_label",
                                          "has_depth")] + [(n, C.c_float) for n in (
                                              "sc_lambda", "lambda_s", "lambda_c", "ds_lambda")]


LOSS_IN_FIELDS = ("rgb", "weights", "beta", "beta_semantic", "semantic_logits", "sun_sc", "transparency_sc",
                  "weights_sc", "depth", "gt_rgb", "labels", "mask", "gt_depth", "depth_weights")
LOSS_GRAD_FIELDS = ("rgb", "weights", "beta", "beta_semantic", "semantic_logits", "sun_sc", "depth")
LOSS_NTOT = 16
LOSS_TERMS = ("coarse_color", "coarse_logbeta", "coarse_sc_term2", "coarse_sc_term3", "coarse_semantic",
              "coarse_semantic_logbeta", "coarse_car_reg_loss", "coarse_ds")


class SnerfLossIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOSS_IN_FIELDS]


class SnerfLossGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOSS_GRAD_FIELDS]


class SnerfDsmGrid(C.Structure):
    _fields_ = [("xoff", C.c_double), ("yoff", C.c_double), ("res", C.c_double)] + [
        (n, C.c_int32) for n in ("xsize", "ysize", "ioff", "joff", "out_w", "out_h")]


SSIM_REFLECT = 0    # include/snerf_hip.h SNERF_SSIM_REFLECT
SSIM_ZERO = 1       # include/snerf_hip.h SNERF_SSIM_ZERO

SEMEVAL_MAX_CLASSES = 16   # include/snerf_hip.h SNERF_SEMEVAL_MAX_CLASSES
SEMEVAL_U8 = 0             # include/snerf_hip.h SNERF_SEMEVAL_U8
SEMEVAL_I64 = 1            # include/snerf_hip.h SNERF_SEMEVAL_I64


class SnerfSemevalAcc(C.Structure):
    _fields_ = [("conf", C.c_uint64 * (SEMEVAL_MAX_CLASSES * SEMEVAL_MAX_CLASSES)), ("errors", C.c_uint64 * 4)] + [
        (n, C.c_uint64) for n in ("rays", "car_rays", "out_of_range")] + [("beta_car_sum", C.c_double)]


VIS_MAX_SAMPLES = 1024     # include/snerf_hip.h SNERF_VIS_MAX_SAMPLES
VIS_SLOTS = 8              # include/snerf_hip.h SNERF_VIS_SLOTS
VIS_SLOT = {"depth": 0, "sun": 1, "beta": 2, "beta_semantic": 3, "rgb_diff_distance": 4, "sem_error": 5, "user": 6}   # SNERF_VIS_SLOT_*
VIS_U8, VIS_I64 = 0, 1     # include/snerf_hip.h SNERF_VIS_U8 / SNERF_VIS_I64
VIS_F32, VIS_F64 = 0, 1    # include/snerf_hip.h SNERF_VIS_F32 / SNERF_VIS_F64
VIS_IN_FIELDS = ("weights", "albedo", "sun", "sky", "beta", "beta_semantic", "depth", "rgb", "rgbs_gt", "label", "semantic_gt",
                 "palette")
VIS_OUT_FIELDS = ("albedo_map", "sun_map", "sky_map", "beta_map", "beta_semantic_map", "depth_map", "rgb_diff",
                  "rgb_diff_distance", "sem_color", "sem_shaded", "sem_error")


class SnerfVisIn(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VIS_IN_FIELDS] + [("gt_dtype", C.c_int32), ("n_palette", C.c_int32)]


class SnerfVisOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VIS_OUT_FIELDS]


class SnerfVisStats(C.Structure):
    _fields_ = [("minmax", C.c_uint64 * 2 * VIS_SLOTS), ("bad_labels", C.c_uint64), ("reserved", C.c_uint64 * 7)]


class SnerfRpc(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("row_offset", "col_offset", "lat_offset", "lon_offset", "alt_offset", "row_scale",
                                          "col_scale", "lat_scale", "lon_scale", "alt_scale")] + [
        (n, C.c_double * 20) for n in ("row_num", "row_den", "col_num", "col_den", "lat_num", "lat_den", "lon_num", "lon_den")] + [
        ("has_inverse", C.c_int), ("reserved", C.c_int)]


class SnerfRayImage(C.Structure):
    _fields_ = [("rpc", SnerfRpc), ("min_alt", C.c_double), ("max_alt", C.c_double), ("row0", C.c_longlong),
                ("n_rays", C.c_longlong), ("w", C.c_int), ("h", C.c_int)]


class SnerfRectImage(C.Structure):
    _fields_ = [("rpc", SnerfRpc), ("row0", C.c_longlong), ("w", C.c_int), ("h", C.c_int)]


RECT_MAX_IMAGES = 64       # include/snerf_orthorect.h SNERF_RECT_MAX_IMAGES
RECT_SEEN, RECT_HOLE, RECT_OUTSIDE, RECT_HIDDEN = 0, 1, 2, 3     # include/snerf_orthorect.h SNERF_RECT_*


class SnerfWarpMap(C.Structure):
    """include/snerf_warp.h: the destination lattice in the source's cell coordinates"""
    _fields_ = [(n, C.c_double) for n in ("off_x", "step_x", "off_y", "step_y")] + [(n, C.c_int) for n in ("src_w", "src_h", "dst_w", "dst_h")]


class SnerfGeoParams(C.Structure):
    _fields_ = [("centre", C.c_double * 3), ("range", C.c_double), ("lon0", C.c_double), ("south", C.c_int), ("direction", C.c_int)]


GEO_TO_WORLD, GEO_TO_SCENE = 0, 1                                # SnerfGeoParams.direction (snerf_geo_points; snerf_geo_cloud: 0 only)
GEO_STATS_INIT = (2 ** 64 - 1, 0, 2 ** 64 - 1, 0, 0, 0, 0, 0)   # include/snerf_hip.h: the caller's initial stats words


class SnerfProfile(C.Structure):
    _fields_ = [("ms", C.c_double * 4), ("flops", C.c_double * 4), ("launches", C.c_int64 * 4)]


PROFILE_VARIANTS = ("K-contiguous dense layers (forward X.W^T and dX = dZ.W): gemm_kc_kernel, 128 x 256 tile", "SIREN trunk as one persistent launch (one-plane mode): trunk_kernel, activation tile resident in LDS",
                    "weight gradients (dW = dZ^T.X, split-K slabs): gemm_dw_kernel, 256 x 256 tile", "32-wide head variants (forward + dW)")


class c_stream(C.c_void_p):
    """The `void* stream` parameter of an entry point.  The marker tells call() which slot it fills itself (the current stream of
    the call's device); a direct caller of lib() passes what a void* takes."""

    @classmethod
    def from_param(cls, value):
        return C.c_void_p.from_param(value)


def _signatures():
    i, ll, ull, sz, f, d, p, st, P = C.c_int, C.c_longlong, C.c_ulonglong, C.c_size_t, C.c_float, C.c_double, C.c_void_p, c_stream, C.POINTER
    desc, grid = P(SnerfDesc), P(SnerfDsmGrid)
    return {
        "snerf_version": (i, ()),
        "snerf_last_error": (C.c_char_p, ()),
        "snerf_packed_floats": (sz, (desc,)),
        "snerf_grad_floats": (sz, (desc,)),
        "snerf_workspace_bytes": (sz, (desc,)),
        "snerf_pack_params": (i, (desc, P(SnerfParams), p, st)),
        "snerf_unpack_grads": (i, (desc, p, P(SnerfParams), i, st)),
        "snerf_forward": (i, (desc, p, P(SnerfInputs), P(SnerfOutputs), p, sz, st)),
        "snerf_sample_z": (i, (p, p, p, p, i, i, st)),
        "snerf_embedding_rows": (i, (p, i, i, p, i, p, st)),
        "snerf_embedding_backward": (i, (p, p, i, i, i, p, st)),
        "snerf_backward": (i, (desc, p, P(SnerfInputs), P(SnerfOutGrads), p, p, p, p, sz, st)),
        "snerf_loss_workspace_bytes": (sz, (P(SnerfLossCfg),)),
        "snerf_loss_partial": (i, (P(SnerfLossCfg), P(SnerfLossIn), p, p, sz, st)),
        "snerf_loss_finish": (i, (P(SnerfLossCfg), P(SnerfLossIn), p, f, f, p, P(SnerfLossGrads), st)),
        "snerf_adam_step": (i, (p, p, p, p, ull, f, f, f, f, i, f, st)),
        "snerf_dsm_accumulate": (i, (p, i, grid, i, d, d, p, p, p, st)),
        "snerf_dsm_finish": (i, (p, p, ll, d, d, p, p, st)),
        "snerf_dsm_downsample2x": (i, (p, i, i, i, p, st)),
        "snerf_dsm_workspace_bytes": (sz, (i, i, i)),
        "snerf_dsm_ncc_search": (i, (p, p, i, i, i, i, i, i, p, p, sz, st)),
        "snerf_dsm_shift_diff": (i, (p, p, i, i, i, i, d, p, p, p, p, sz, st)),
        "snerf_ortho_top": (i, (p, ll, ll, grid, i, d, d, p, p, st)),
        "snerf_ortho_gather": (i, (p, ll, ll, ll, d, d) + (p,) * 8 + (st,)),
        "snerf_ortho_votes": (i, (p, p, ll, grid, i, i, p, p, st)),
        "snerf_ortho_votes_finish": (i, (p, i, ll, p, p, p, st)),
        "snerf_ssim_workspace_bytes": (sz, (i,) * 5),
        "snerf_ssim": (i, (p, p) + (i,) * 6 + (p, d, d, d, p, p, p, sz, st)),
        "snerf_semeval_workspace_bytes": (sz, (i, i)),
        "snerf_semeval_accumulate": (i, (p,) * 4 + (i,) * 4 + (p, p, i, p, p, sz, st)),
        # SnerfVisStats lives in device memory: void*
        "snerf_vis_fold": (i, (P(SnerfVisIn), P(SnerfVisOut), i, i, ll, ll, p, st)),
        "snerf_vis_minmax": (i, (p, i, ll, p, i, st)),
        "snerf_vis_colormap": (i, (p, i, ll, p, i, d, d, p, p, st)),
        # SnerfRayImage / SnerfRpc tables go as void*: the same slot type serves the host copy (a ctypes array or byref) and the
        # device copy (a tensor)
        "snerf_rpc_rays": (i, (p, p, i, p, ll, p, p, st)),
        "snerf_rpc_localize": (i, (p,) * 5 + (ll, i) + (p,) * 3 + (st,)),
        "snerf_rpc_project": (i, (p,) * 5 + (ll, p, p, st)),
        "snerf_rpc_reprojection_error": (i, (p,) * 4 + (ll, p, p, st)),
        "snerf_ray_bounds_workspace_bytes": (sz, (p, i)),
        "snerf_ray_bounds": (i, (p, p, i, p, p, sz, st)),
        "snerf_normalize_rows": (i, (p, ll, i, i, p, st)),
        "snerf_geo_cloud": (i, (p, i, p, ll, P(SnerfGeoParams), p, p, p, st)),
        "snerf_geo_points": (i, (p, ll, P(SnerfGeoParams), p, p, p, st)),
        # suns_host is a HOST table (a ctypes array): void*, as the RPC tables
        "snerf_shadow_cast": (i, (p, i, i, p, i, d, d, p, p, st)),
        "snerf_shadow_agreement": (i, (p, p, p, ll, i, d, p, st)),
        "snerf_resample_z": (i, (p,) * 5 + (i,) * 3 + (st,)),
        "snerf_ray_distortion": (i, (p,) * 3 + (i,) * 3 + (p,) * 3 + (st,)),
        "snerf_profile_begin": (i, ()),
        "snerf_profile_end": (i, (P(SnerfProfile),)),
        "snerf_test_set_kc_grid": (i, (i,)),
        "snerf_test_set_trunk_fusion": (i, (i,)),
        "snerf_test_bsp_roundtrip": (i, (p, i, i, i, i, p, p, i, st)),
        "snerf_test_bsp_kc": (i, (p, p, i, p, p, i, i, i, i, i, i, f, i) + (p,) * 7 + (P(i), i, i, st)),
        "snerf_test_bsp_dw": (i, (p, i, p, i, i, i, i, i, i, i, i, p, i, st)),
    }


# THE binding table: symbol -> (restype, argtypes), one row per prototype of include/snerf_hip.h in the header's order
# (tests/test_abi_cpu.py compares the two, parameter by parameter).  A new entry point is declared there and here.
SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(SIGNATURES)

# Entries declared OUTSIDE include/snerf_hip.h, whose list of symbols is frozen at ABI 6: header -> rows in that header's order, the
# headers in the order they were added (tests/abi_header.py compares each group with its header as tests/test_abi_cpu.py does for
# the table above, and freezes the symbols of every group).  lib() and call() serve both tables alike.  The groups are frozen there: a
# newer header's group goes into ADDED_HEADER_SIGNATURES below.
HEADER_SIGNATURES = {
    # the SnerfRectImage table goes as void* twice: the host copy (a ctypes array), the device copy (a tensor)
    "snerf_orthorect.h": {"snerf_orthorectify": (C.c_int, (C.c_void_p, C.POINTER(SnerfDsmGrid), C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                                          C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int) + (C.c_void_p,) * 9 + (c_stream,))},
    "snerf_raycast.h": {"snerf_dsm_segment_hit": (C.c_int, (C.c_void_p, C.c_void_p, C.c_longlong, C.POINTER(SnerfDsmGrid), C.c_void_p,
                                                            C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, c_stream))},
    # quantiles_host is a HOST table (a ctypes array): void*, as suns_host
    "snerf_fuse.h": {
        "snerf_fuse_count": (C.c_int, (C.c_void_p, C.c_longlong, C.POINTER(SnerfDsmGrid), C.c_int, C.c_double, C.c_double, C.c_void_p,
                                       C.c_void_p, c_stream)),
        "snerf_fuse_scatter": (C.c_int, (C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(SnerfDsmGrid), C.c_int, C.c_double, C.c_double,
                                         C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_fuse_select": (C.c_int, (C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, c_stream)),
    },
    # member_host and ground_host are HOST tables (ctypes arrays of 256 bytes): void*
    "snerf_objects.h": {
        "snerf_objects_link": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_objects_stats": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int,
                                          C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, c_stream)),
    },
    # blocked_host is a HOST table (a ctypes array of 256 bytes): void*.  snerf_terrain_workspace_bytes returns a long long, -1 for a
    # refusal
    "snerf_terrain.h": {
        "snerf_terrain_workspace_bytes": (C.c_longlong, (C.c_int, C.c_int)),
        "snerf_terrain_keys": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_void_p, c_stream)),
        "snerf_terrain_open": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, c_stream)),
        "snerf_terrain_fill": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_stream)),
    },
    # `planes` is a device array of doubles
    "snerf_roofs.h": {
        "snerf_roofs_normals": (C.c_int, (C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int) + (C.c_double,) * 6
                                + (C.c_void_p,) * 5 + (c_stream,)),
        "snerf_roofs_link": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_roofs_moments": (C.c_int, (C.c_void_p,) * 4 + (C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                              c_stream)),
        "snerf_roofs_residuals": (C.c_int, (C.c_void_p,) * 3 + (C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, c_stream)),
    },
    # `dirs_host` and `suns_host` are host tables
    "snerf_solar.h": {
        "snerf_solar_horizon": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                          c_stream)),
        "snerf_solar_svf": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, c_stream)),
        "snerf_solar_irradiate": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_void_p, c_stream)),
    },
    # the density-gradient pass, the size of its scratch buffer (an int return, the size through a size_t*) and its two test hooks
    "snerf_normals.h": {
        "snerf_normals_scratch_bytes": (C.c_int, (C.POINTER(SnerfDesc), C.POINTER(C.c_size_t))),
        "snerf_density_grad": (C.c_int, (C.POINTER(SnerfDesc), C.c_void_p, C.POINTER(SnerfInputs)) + (C.c_void_p,) * 5 + (c_stream,)),
        "snerf_test_normals_grid": (C.c_int, (C.c_int,)),
        "snerf_test_normals_dump": (C.c_int, (C.c_void_p, C.c_void_p)),
    },
}
# The headers added after tests/abi_header.py froze the table above: the same shape, merged the same way, each group compared with its
# header by its own test (include/snerf_warp.h: tests/test_warp_cpu.py).  That test pins this table's headers too, so it is frozen
# as well: a newer header's group goes into LATER_HEADER_SIGNATURES below.
ADDED_HEADER_SIGNATURES = {
    "snerf_warp.h": {
        "snerf_warp_planes": (C.c_int, (C.c_void_p, C.c_int, C.POINTER(SnerfWarpMap), C.c_int, C.c_double, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_warp_labels": (C.c_int, (C.c_void_p, C.POINTER(SnerfWarpMap), C.c_int, C.c_void_p, C.c_void_p, c_stream)),
    },
}
# The headers added after that: the same shape, merged the same way, each group compared with its header by its own test
# (include/snerf_outline.h: tests/test_outline_cpu.py, which pins the symbols of a group and not the list of headers).  A newer
# header adds its group here.  snerf_outline_workspace_bytes returns a long long, -1 for a refusal.
LATER_HEADER_SIGNATURES = {
    "snerf_outline.h": {
        "snerf_outline_sides": (C.c_int, (C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_outline_link": (C.c_int, (C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, c_stream)),
        "snerf_outline_workspace_bytes": (C.c_longlong, (C.c_longlong,)),
        "snerf_outline_rank": (C.c_int, (C.c_void_p, C.c_void_p, C.c_longlong) + (C.c_void_p,) * 5 + (C.c_longlong, C.c_void_p, c_stream)),
        "snerf_outline_emit": (C.c_int, (C.c_void_p,) * 7 + (C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong) + (C.c_void_p,) * 3
                               + (c_stream,)),
    },
    # facet growth and the arcs of a partition (tests/test_rooflines_cpu.py compares the group with its header)
    "snerf_rooflines.h": {
        "snerf_roofs_grow": (C.c_int, (C.c_void_p,) * 5 + (C.c_int, C.c_int, C.c_longlong, C.c_double, C.c_longlong, C.c_int) + (C.c_void_p,) * 3
                             + (c_stream,)),
        "snerf_arcs_first": (C.c_int, (C.c_void_p,) * 4 + (C.c_int, C.c_int, C.c_longlong, C.c_longlong) + (C.c_void_p,) * 3 + (c_stream,)),
        "snerf_arcs_mark": (C.c_int, (C.c_void_p,) * 12 + (C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_longlong) + (C.c_void_p,) * 7
                            + (c_stream,)),
        "snerf_arcs_fold": (C.c_int, (C.c_void_p,) * 16 + (C.c_int, C.c_int) + (C.c_longlong,) * 4 + (C.c_void_p,) * 3 + (c_stream,)),
    },
}
_ALL_SIGNATURES = dict(SIGNATURES)
for _rows in list(HEADER_SIGNATURES.values()) + list(ADDED_HEADER_SIGNATURES.values()) + list(LATER_HEADER_SIGNATURES.values()):
    assert not set(_rows) & set(_ALL_SIGNATURES)
    _ALL_SIGNATURES.update(_rows)

HIT_TOP, HIT_WALL, HIT_START, HIT_END, HIT_OUTSIDE, HIT_BAD = range(6)     # include/snerf_raycast.h SNERF_HIT_*

SHADOW_MAX_SUNS = 64       # include/snerf_hip.h SNERF_SHADOW_MAX_SUNS
SHADOW_UNKNOWN = 255       # include/snerf_hip.h SNERF_SHADOW_UNKNOWN

ORTHO_MAX_RADIUS = 7       # include/snerf_hip.h SNERF_ORTHO_MAX_RADIUS
ORTHO_MAX_CLASSES = 255    # include/snerf_hip.h SNERF_ORTHO_MAX_CLASSES
ORTHO_NO_LABEL = 255       # include/snerf_hip.h SNERF_ORTHO_NO_LABEL
FUSE_MAX_QUANTILES = 8     # include/snerf_fuse.h SNERF_FUSE_MAX_QUANTILES
OBJECTS_ROW_WORDS = 16     # include/snerf_objects.h SNERF_OBJECTS_ROW_WORDS
TERRAIN_HOLE = -2 ** 31    # include/snerf_terrain.h SNERF_TERRAIN_HOLE
TERRAIN_MAX_RADIUS = 512   # include/snerf_terrain.h SNERF_TERRAIN_MAX_RADIUS
TERRAIN_FLAGGED, TERRAIN_BLOCKED, TERRAIN_IS_HOLE = 1, 2, 4     # include/snerf_terrain.h: the bits of a flags byte
ROOFS_MAX_RADIUS = 4       # include/snerf_roofs.h SNERF_ROOFS_MAX_RADIUS
ROOFS_MAX_SIDE = 8192      # include/snerf_roofs.h SNERF_ROOFS_MAX_SIDE
ROOFS_MAX_OBJECTS = 2 ** 27    # include/snerf_roofs.h SNERF_ROOFS_MAX_OBJECTS
ROOFS_MOMENT_WORDS, ROOFS_RESIDUAL_WORDS = 16, 8               # include/snerf_roofs.h SNERF_ROOFS_*_WORDS
# include/snerf_roofs.h: the orientation codes (1..8 = the downslope octants N, NE, E, SE, S, SW, W, NW)
ROOFS_FLAT, ROOFS_STEEP, ROOFS_HOLE, ROOFS_DEGENERATE, ROOFS_NONE = 0, 9, 253, 254, 255
SOLAR_MAX_DIRS = 64        # include/snerf_solar.h SNERF_SOLAR_MAX_DIRS
SOLAR_MAX_SECTORS = 720    # include/snerf_solar.h SNERF_SOLAR_MAX_SECTORS
SOLAR_MAX_SUNS = 64        # include/snerf_solar.h SNERF_SOLAR_MAX_SUNS
WARP_NEAREST, WARP_BILINEAR, WARP_AVERAGE, WARP_MIN, WARP_MAX, WARP_MODE = range(6)      # include/snerf_warp.h SNERF_WARP_*: the methods
WARP_MAX_STEP = 64         # include/snerf_warp.h SNERF_WARP_MAX_STEP
WARP_MAX_PLANES = 16       # include/snerf_warp.h SNERF_WARP_MAX_PLANES
OUTLINE_ROW_WORDS = 8      # include/snerf_outline.h SNERF_OUTLINE_ROW_WORDS
OUTLINE_MAX_CELLS = 2 ** 29    # include/snerf_outline.h SNERF_OUTLINE_MAX_CELLS
OUTLINE_CORNER = 1         # include/snerf_outline.h SNERF_OUTLINE_CORNER: bit 0 of an edge's flags; bits 1-2 hold its side
ARCS_ROW_WORDS = 12        # include/snerf_rooflines.h SNERF_ARCS_ROW_WORDS
ARCS_NO_FIRST = 2 ** 31 - 1    # include/snerf_rooflines.h SNERF_ARCS_NO_FIRST: the initial word of a ring's first break
GROW_MAX_ROUNDS = 64       # include/snerf_rooflines.h SNERF_GROW_MAX_ROUNDS: the rounds of one snerf_roofs_grow call

# symbol -> (per argument a caller of call() passes: int / float for a scalar slot, None for a pointer slot; whether a trailing
# stream follows them)
_PLANS = {name: (tuple(float if t in (C.c_float, C.c_double) else None if issubclass(t, (C.c_void_p, C._Pointer)) else int
                       for t in args if t is not c_stream), c_stream in args)
          for name, (_, args) in _ALL_SIGNATURES.items()}
assert all(c_stream not in args[:-1] for _, args in _ALL_SIGNATURES.values())

_lib = None


def lib():
    """Load the HIP library; no fallback of any kind."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libsnerf_hip.so not found at {LIB_PATH}: the HIP extension is the product path and has no "
            "fallback. Build it with `make -C semantic-nerf-for-satellite-data_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).")
    # torch bundles its own HIP runtime and is imported above, FIRST, so that libsnerf_hip.so binds to the runtime that
    # owns torch's device context and streams (loading ours first brings up a second runtime that then
    # reports "no ROCm-capable device").
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _ALL_SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    if L.snerf_version() != ABI_VERSION:
        raise RuntimeError(f"libsnerf_hip.so ABI version {L.snerf_version()} != {ABI_VERSION}")
    _lib = L
    return L


def check(rc, what, exc=RuntimeError):
    if rc != 0:
        raise exc(f"{what} failed (code {rc}): {lib().snerf_last_error().decode()}")


def _invoke(name, args, device):
    slots, has_stream = _PLANS[name]
    if len(args) != len(slots):
        raise TypeError(f"{name} takes {len(slots)} arguments{' (the stream is filled in)' if has_stream else ''}, {len(args)} given")
    out = []
    for k, (scalar, a) in enumerate(zip(slots, args)):
        if scalar is not None:
            a = scalar(a)
        elif isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise RuntimeError(f"snerf_amd: argument {k} of {name} must live on the GPU (the HIP path has no CPU fallback)")
            if not a.is_contiguous():
                raise RuntimeError(f"snerf_amd: argument {k} of {name} must be contiguous (the library takes no strides)")
            if device is None:
                device = a.device
            a = a.data_ptr()
        elif isinstance(a, C.Structure):
            a = C.byref(a)
        # else None (NULL), a raw address, a ctypes array or pointer: as ctypes takes them
        out.append(a)
    fn = getattr(lib(), name)
    if not has_stream:
        return fn(*out)
    if device is None:
        raise TypeError(f"{name}: no tensor argument to take the device from; pass device=")
    with torch.cuda.device(device):
        return fn(*out, torch.cuda.current_stream().cuda_stream)


def call(name, *args, device=None, exc=RuntimeError):
    """Call an int-returning entry point by the table: tensors go as their device address (refused unless on the GPU and
    contiguous; no copies are made here), None as NULL, structs by reference, scalars converted; the stream is not passed --
    the launch runs under the device of the first tensor argument (or `device`) on that device's current stream.  A non-zero
    return raises `exc` with the library's message."""
    check(_invoke(name, args, device), name, exc)


def call_size(name, *args, exc=RuntimeError):
    """The size_t-returning *_bytes / *_floats entries: a returned 0 is the library's refusal and raises with its message."""
    n = _invoke(name, args, None)
    if n == 0:
        check(1, name, exc)
    return n
