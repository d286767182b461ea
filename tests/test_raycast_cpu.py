"""CPU-side checks of the DSM ray cast (include/snerf_raycast.h, csrc/raycast.hip, eval/utils/raycast.py, baseline/dataset/
dsm_depth_dataset.py): the new header's prototype and constants against the binding (_lib.HEADER_SIGNATURES),
the refusals of the entry through the binding (none reaches a launch), of the Python layer and of the new config fields, the numpy
restatement (tests/raycast_numpy.py, the oracle of tests/test_gpu_raycast.py) against an independent dense oracle, guide_rays on
hand-made rows, and the host logic of DsmDepthDataset on the fixture scene."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import raycast as R            # the feature under test: every test of this file needs it
from tests import raycast_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_raycast.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
SYMBOL = "snerf_dsm_segment_hit"


def test_header_constants_match_the_binding_and_the_restatement():
    src = open(HEADER).read()
    assert _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    assert int(re.search(r"#define SNERF_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "snerf_hip.h")).read()).group(1)) == 6
    for value, name in enumerate(("TOP", "WALL", "START", "END", "OUTSIDE", "BAD")):
        assert int(re.search(rf"#define SNERF_HIT_{name} (\d+)", src).group(1)) == getattr(_lib, "HIT_" + name) == value
        assert getattr(N, name) == getattr(R, name) == value
    assert R.STATES == ("top", "wall", "start", "end", "outside", "bad") and N.HIT_STATES == (R.TOP, R.WALL, R.START)
    assert R.is_hit(torch.arange(6, dtype=torch.uint8)).tolist() == [True, True, True, False, False, False]


def test_the_new_header_matches_its_binding_row():
    """include/snerf_raycast.h against its rows of _lib.HEADER_SIGNATURES (tests/abi_header.py); the main header, the main table,
    the other headers' rows and the ABI version are untouched"""
    from tests.abi_header import check_header
    check_header("snerf_raycast.h", {SYMBOL: ["p0", "p1", "n", "grid", "dsm", "bias", "s_out", "state_out", "cell_out", "stream"]})


# ---- refusals of the entry ----------------------------------------------------------------------------------------------------------
def _grid(**kw):
    g = _lib.SnerfDsmGrid(1000.0, 2000.0, 0.5, 4, 3, 0, 0, 4, 3)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _call(**kw):
    """snerf_dsm_segment_hit through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    a = dict(p0=DUMMY, p1=DUMMY, n=2, grid=_grid(), dsm=DUMMY, bias=0.0, s_out=DUMMY, state_out=DUMMY, cell_out=DUMMY)
    a.update(kw)
    grid = C.byref(a["grid"]) if a["grid"] is not None else None
    rc = L.snerf_dsm_segment_hit(a["p0"], a["p1"], a["n"], grid, a["dsm"], a["bias"], a["s_out"], a["state_out"], a["cell_out"], None)
    return rc, L.snerf_last_error().decode()


@pytest.mark.parametrize("kw,code,needle", [
    ({"p0": None}, 3, "null"), ({"p1": None}, 3, "null"), ({"grid": None}, 3, "null"), ({"dsm": None}, 3, "null"),
    ({"s_out": None}, 3, "null"), ({"state_out": None}, 3, "null"),
    ({"n": -1}, 1, "n = -1"), ({"n": 2 ** 31 + 1}, 1, "n = 2147483649"), ({"n": -2 ** 62}, 1, "outside [0, 2^31]"),
    ({"grid": _grid(res=0.0)}, 1, "res > 0"), ({"grid": _grid(res=math.nan)}, 1, "res > 0"), ({"grid": _grid(res=math.inf)}, 1, "res > 0"),
    ({"grid": _grid(xoff=math.nan)}, 1, "res > 0"), ({"grid": _grid(out_h=0)}, 1, "positive sizes"), ({"grid": _grid(out_w=-1)}, 1, "positive sizes"),
    ({"grid": _grid(ysize=0)}, 1, "positive sizes"),
    ({"grid": _grid(joff=2 ** 31 - 3)}, 1, "int32"), ({"grid": _grid(ioff=2 ** 31 - 4)}, 1, "int32"),
    ({"grid": _grid(out_w=1 << 16, out_h=1 << 15)}, 1, "2^31"),
    ({"bias": math.inf}, 1, "bias"), ({"bias": -math.inf}, 1, "bias"), ({"bias": math.nan}, 1, "bias"),
    ({"n": 0, "bias": math.nan}, 1, "bias"), ({"n": 0, "dsm": None}, 3, "null"),
], ids=lambda v: None if isinstance(v, dict) else str(v))
def test_the_entry_refuses_bad_arguments_before_any_launch(kw, code, needle):
    rc, msg = _call(**dict(kw))
    assert rc == code and msg.startswith("snerf_dsm_segment_hit: ") and needle in msg, (rc, msg)


def test_zero_segments_are_accepted_and_launch_nothing():
    """n == 0 with good arguments returns SNERF_OK before the launch: the dummy addresses are never handed to a kernel, and no GPU
    is needed for it"""
    assert _call(n=0)[0] == 0 and _call(n=0, cell_out=None)[0] == 0


def test_python_refusals():
    dsm = torch.zeros(3, 4)
    p = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="the DSM must be a GPU tensor"):
        R.segment_hits(p, p, _grid(), dsm)
    with pytest.raises(ValueError, match="the rays must be a GPU tensor"):
        R.cast_rays(torch.zeros(2, 8), None, _grid(), dsm)
    rays = torch.zeros(3, 8)
    cast = {"depth": torch.zeros(3), "state": torch.zeros(3, dtype=torch.uint8)}
    with pytest.raises(ValueError, match=r"\(n, >= 8\) float32"):
        R.guide_rays(torch.zeros(3, 6), cast, 1.0, 1.0, 100.0)
    with pytest.raises(ValueError, match=r"\(n, >= 8\) float32"):
        R.guide_rays(rays.double(), cast, 1.0, 1.0, 100.0)
    with pytest.raises(ValueError, match="front_m = -1.0"):
        R.guide_rays(rays, cast, -1.0, 1.0, 100.0)
    with pytest.raises(ValueError, match="back_m = nan"):
        R.guide_rays(rays, cast, 1.0, math.nan, 100.0)
    for bad in (0.0, -3.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="range = "):
            R.guide_rays(rays, cast, 1.0, 1.0, bad)
    with pytest.raises(ValueError, match="a cast of 2 rows for 3 rays"):
        R.guide_rays(rays, {"depth": torch.zeros(2), "state": torch.zeros(2, dtype=torch.uint8)}, 1.0, 1.0, 100.0)
    with pytest.raises(TypeError):
        R.guide_rays(rays, cast)                                   # front_m, back_m and range have no defaults
    with pytest.raises(ValueError, match="2 depths against a cast of 3 rows"):
        R.view_depth_error(torch.zeros(2), cast, 100.0)
    with pytest.raises(ValueError, match="range = 0.0"):
        R.view_depth_error(torch.zeros(3), cast, 0.0)
    with pytest.raises(TypeError):
        R.DsmGuide(None, None, dsm, n_samples=16)                  # the band has no default either


def test_guided_inference_refuses_per_sample_results_and_pinned_depths():
    from snerf_amd.eval.utils.util import guided_lean_inference
    guide = R.DsmGuide(None, None, None, 1.0, 1.0, 16)
    for key in ("weights_coarse", "sigmas", "beta_coarse", "sun_sc_coarse"):
        with pytest.raises(KeyError, match="per-sample result"):
            guided_lean_inference(None, None, None, None, None, guide, keys=("depth_coarse", key))
    with pytest.raises(KeyError, match="unknown result 'nonsense'"):
        guided_lean_inference(None, None, None, None, None, guide, keys=("nonsense",))
    for key in ("given_z_vals", "perturb_rand", "importance_rand"):
        with pytest.raises(ValueError, match=f"render_options\\['{key}'\\] cannot be pinned"):
            guided_lean_inference(None, None, None, None, None, guide, keys=("depth_coarse",), render_options={key: torch.zeros(1, 1)})
    with pytest.raises(ValueError, match="n_samples = 0"):
        guided_lean_inference(None, None, None, None, None, R.DsmGuide(None, None, None, 1.0, 1.0, 0), keys=("depth_coarse",))
    from snerf_amd.eval.extract_pointcloud import extract_pointcloud
    with pytest.raises(ValueError, match="guide= is a single-device render"):
        extract_pointcloud(None, None, None, None, None, sharded=True, guide=guide)


# ---- the restatement against the dense oracle ----------------------------------------------------------------------------------------
def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def test_the_restatement_against_the_dense_oracle():
    """2,000 seeded segments over the 23 x 17 window (tests/raycast_numpy.py random_heights / random_segments): a hit is never later
    than the oracle's first sample at or under the surface and at most one sample step earlier; where the oracle finds nothing the
    restatement reports END or OUTSIDE.  Segments whose oracle answer changes when all heights move by +-1e-9 m are left out: at
    most 1 % of them.
    The seed.  The walk is exact and the oracle sampled, so a contact thinner than one sample step (a ray that clips the corner of a
    tall cell, or rises out of the surface right behind its entry) is invisible to the oracle, which then answers later or not at
    all; moving the heights does not flag these.  Over the seeds 1 to 40, measured here, there were 0 to 6 such segments of 2,000
    (every one of them 'earlier than one step' or 'the oracle found nothing'; not one hit was ever LATER than the oracle), none left
    out by the +-1e-9 m rule; seeds 1, 7, 10, 20, 26, 29, 30 and 36 had none, and 7 is the seed."""
    dsm = N.random_heights()
    p0, p1 = N.random_segments()
    assert p0.shape == p1.shape == (N.N_RANDOM, 3) and dsm.shape == (17, 23) and N.GRID[5:] == (23, 17)
    assert np.isnan(dsm).sum() == 2 and np.isposinf(dsm).sum() == 1 and np.isneginf(dsm).sum() == 1
    fin = dsm[np.isfinite(dsm)]
    assert np.array_equal(fin * 4.0, np.rint(fin * 4.0))                                  # multiples of 0.25 m
    d = p1 - p0
    vertical, level = (d[:, 0] == 0) & (d[:, 1] == 0), d[:, 2] == 0
    x0 = (p0[:, 0] - N.GRID[0]) / N.GRID[2] - N.GRID[3]
    y0 = (N.GRID[1] - p0[:, 1]) / N.GRID[2] - N.GRID[4]
    on_edge = ((d[:, 0] == 0) & (x0 == np.floor(x0)) & ~vertical) | ((d[:, 1] == 0) & (y0 == np.floor(y0)) & ~vertical)
    inside = (x0 >= 0) & (x0 < 23) & (y0 >= 0) & (y0 < 17)
    assert min(vertical.sum(), level.sum(), on_edge.sum(), inside.sum(), (~inside).sum()) >= 100

    s, state, cell = N.segment_hits(p0, p1, N.GRID, dsm)
    print("states (top, wall, start, end, outside, bad):", np.bincount(state, minlength=6).tolist())
    assert (np.bincount(state, minlength=6)[:5] >= 100).all() and not (state == N.BAD).any()
    hit = np.isin(state, N.HIT_STATES)
    assert np.array_equal(hit, ~np.isnan(s)) and np.array_equal(hit, cell >= 0) and (cell[~hit] == -1).all()
    assert (s[hit] >= 0.0).all() and (s[hit] <= 1.0).all() and (cell < 23 * 17).all()
    assert (s[(state == N.START) & inside] == 0.0).all()
    assert not np.isin(cell[hit], [4 * 23 + 7, 11 * 23 + 15, 13 * 23 + 19]).any()          # NaN and -inf cells never block
    assert (cell == 8 * 23 + 3).any() and not (state[cell == 8 * 23 + 3] == N.TOP).any()   # the +inf cell is a wall (or a start)

    oracle, step = N.dense_oracle(p0, p1, N.GRID, dsm)
    up, _ = N.dense_oracle(p0, p1, N.GRID, dsm, 1e-9)
    down, _ = N.dense_oracle(p0, p1, N.GRID, dsm, -1e-9)
    left_out = ~(_same(oracle, up) & _same(oracle, down))
    print(f"left out (the oracle's answer moves with the heights): {int(left_out.sum())} of {len(s)}")
    assert left_out.sum() <= 0.01 * len(s)
    found = ~np.isnan(oracle)
    keep = ~left_out
    late = keep & hit & found & (s > oracle)
    early = keep & hit & found & (s < oracle - step)
    unseen = keep & hit & ~found
    missed = keep & ~hit & found
    print(f"later than the oracle: {int(late.sum())}, more than one step earlier: {int(early.sum())}, hits the oracle has not: "
          f"{int(unseen.sum())}, oracle hits the walk has not: {int(missed.sum())}")
    assert not late.any() and not early.any() and not unseen.any() and not missed.any()
    assert np.isin(state[keep & ~found], (N.END, N.OUTSIDE)).all()


def test_hand_made_segments():
    """a 3 x 1 window of heights 0, 5, 0 at 1 m: every state, the tie rule and the clamp of a contact"""
    grid = (0.0, 1.0, 1.0, 0, 0, 3, 1)
    dsm = np.array([[0.0, 5.0, 0.0]], np.float32)

    def one(a, b, **kw):
        return N.segment_hit(np.array(a, np.float64), np.array(b, np.float64), grid, dsm, **kw)
    assert one((0.5, 0.5, 2.0), (0.5, 0.5, -2.0)) == (0.5, N.TOP, 0)                       # vertical, down onto cell 0
    assert one((0.5, 0.5, -1.0), (0.5, 0.5, 4.0)) == (0.0, N.START, 0)                     # begins under the surface
    assert one((0.5, 0.5, 2.0), (2.5, 0.5, 2.0)) == (0.25, N.WALL, 1)                      # level flight into the block's side
    assert one((0.5, 0.5, 6.0), (2.5, 0.5, 6.0))[1:] == (N.END, -1)                        # level flight above everything
    assert one((0.5, 0.5, 6.0), (4.5, 0.5, 6.0))[1:] == (N.OUTSIDE, -1)                    # ... and out of the window
    assert one((-2.0, 0.5, 1.0), (-1.0, 0.5, 1.0))[1:] == (N.OUTSIDE, -1)                  # never reaches it
    assert one((-2.0, 5.0, 1.0), (4.0, 5.0, 1.0))[1:] == (N.OUTSIDE, -1)                   # passes north of it
    assert one((-1.0, 0.5, 10.0), (3.0, 0.5, 2.0)) == (0.625, N.TOP, 1)                    # enters by the west edge, lands on the block
    assert one((-1.0, 0.5, 7.0), (3.0, 0.5, 3.0)) == (0.5, N.WALL, 1)                      # ... or meets its side exactly at its top
    assert one((4.0, 0.5, 1.0), (2.0, 0.5, 1.0))[1:] == (N.END, -1)                        # enters by the east edge and ends over cell 2
    assert one((4.0, 0.5, -1.0), (2.0, 0.5, -1.0)) == (0.5, N.START, 2)                    # enters by the east edge under the surface
    assert one((0.5, 0.5, math.nan), (0.5, 0.5, 0.0))[1:] == (N.BAD, -1) and one((0.5, math.inf, 1.0), (0.5, 0.5, 0.0))[1:] == (N.BAD, -1)
    assert one((0.5, 0.5, 2.0), (0.5, 0.5, 1.0), bias=1.5) == (0.5, N.TOP, 0)              # the bias lifts the surface
    s, state, cell = one((0.5, 0.5, 1.0), (2.5, 0.5, 1.0), bias=-10.0)                     # ... or sinks it below the flight
    assert (state, cell) == (N.END, -1) and math.isnan(s)


# ---- guide_rays ------------------------------------------------------------------------------------------------------------------------
def test_guide_rays_clamps_both_ends_and_leaves_other_rows_bit_for_bit():
    g = torch.Generator().manual_seed(5)
    rays = torch.rand((7, 11), generator=g)
    rays[:, 6], rays[:, 7] = 0.25, 0.75
    rays[5, 6] = math.nan                                                                  # an unguided row keeps even a NaN's bits
    depth = torch.tensor([0.5, 0.27, 0.74, 0.5, math.nan, math.nan, 0.5])
    state = torch.tensor([R.TOP, R.WALL, R.START, R.END, R.OUTSIDE, R.BAD, R.TOP], dtype=torch.uint8)
    cast = {"depth": depth, "state": state}
    out, n = R.guide_rays(rays, cast, 5.0, 10.0, 100.0)                                    # 0.05 in front, 0.1 behind
    assert n == 4 and out is not rays and out.dtype == rays.dtype and out.shape == rays.shape
    lo, hi = depth - 5.0 / 100.0, depth + 10.0 / 100.0
    assert out[0, 6] == lo[0] and out[0, 7] == hi[0]                                       # inside the bounds: the band itself
    assert out[1, 6] == 0.25 and out[1, 7] == hi[1]                                        # the front is clamped at near
    assert out[2, 6] == lo[2] and out[2, 7] == 0.75                                        # the back is clamped at far
    keep = torch.ones_like(rays, dtype=torch.bool)
    keep[[0, 1, 2, 6], 6:8] = False
    assert torch.equal(out.view(torch.int32)[keep], rays.view(torch.int32)[keep])          # every other value, bit for bit
    assert torch.equal(out[3:6].view(torch.int32), rays[3:6].view(torch.int32))
    wide, n = R.guide_rays(rays, cast, math.inf, math.inf, 100.0)                          # an infinite band guides nothing away
    assert n == 4 and torch.equal(wide.view(torch.int32), rays.view(torch.int32))
    flat, _ = R.guide_rays(rays, cast, 0.0, 0.0, 100.0)                                    # a zero band: near' = far' = the hit
    assert torch.equal(flat[[0, 1, 2, 6], 6], depth[[0, 1, 2, 6]]) and torch.equal(flat[[0, 1, 2, 6], 7], depth[[0, 1, 2, 6]])
    err = R.view_depth_error(torch.tensor([0.51, 0.27, 0.70, 9.0, 9.0, 9.0, math.nan]), cast, 100.0)
    assert err["n"] == 3 and abs(err["mean"] - (1.0 + 0.0 + 4.0) / 3) < 1e-5 and abs(err["median"] - 1.0) < 1e-5
    none = R.view_depth_error(torch.zeros(7), {"depth": depth, "state": torch.full((7,), R.END, dtype=torch.uint8)}, 100.0)
    assert none["n"] == 0 and math.isnan(none["mean"]) and math.isnan(none["median"])


# ---- the depth prior's host logic ----------------------------------------------------------------------------------------------------
def _cfgs(tmp_path, **pipeline):
    from snerf_amd.framework.configs import MainConfig
    from tests.orthorect_numpy import SCENE
    return MainConfig(run={"max_train_steps": 6, "dataset_dp": SCENE, "cache_dp": str(tmp_path), "dataset_name": "scene_small"},
                      pipeline=dict({"pipeline": "snerf_amd.semantic.pipelines.rs_semantic.RSSemanticPipeline", "fc_units": 64,
                                     "n_samples": 32, "batch_size": 128, "first_beta_epoch": 0, "sparsity_n_images": 2}, **pipeline))


def test_config_fields_and_their_refusals(tmp_path):
    c = _cfgs(tmp_path)
    p = c.pipeline
    assert (p.depth_source, p.depth_prior_dsm_fp, p.depth_prior_stride, p.depth_prior_weight) == ("tie_points", "", 4, 1.0)
    for bad, needle in (({"depth_source": "lidar"}, "depth_source"), ({"depth_source": "dsm"}, "needs depth_prior_dsm_fp"),
                        ({"depth_source": "both"}, "needs depth_prior_dsm_fp"), ({"depth_prior_stride": 0}, "depth_prior_stride must be >= 1"),
                        ({"depth_prior_weight": 0.0}, "depth_prior_weight"), ({"depth_prior_weight": math.inf}, "depth_prior_weight")):
        with pytest.raises(ValueError, match=needle):
            _cfgs(tmp_path, **bad)
    ok = _cfgs(tmp_path, depth_source="both", depth_prior_dsm_fp="x.tif", depth_prior_stride=3, depth_prior_weight=0.5).pipeline
    assert (ok.depth_source, ok.depth_prior_dsm_fp, ok.depth_prior_stride, ok.depth_prior_weight) == ("both", "x.tif", 3, 0.5)


def test_dsm_depth_dataset_host_logic_on_the_fixture_scene(tmp_path):
    from PIL import Image
    from snerf_amd.baseline.dataset import dsm_depth_dataset as DD
    from snerf_amd.eval.utils.dsm import DsmGrid
    from snerf_amd.framework.util import img_utils as I
    from tests import orthorect_numpy as ON
    lattice = ON.fixture_lattice()
    grid = DsmGrid(lattice[0], lattice[1], lattice[2], lattice[5], lattice[6])
    dsm = ON.block_dsm(lattice, holes=True)
    dsm[0, 0] = -9999.0                                                                    # a lidar product's no-data value
    fp = I.save_geotiff(str(tmp_path / "prior.tif"), dsm, grid, "17R")
    got, got_grid = DD.load_prior_dsm(fp)
    assert got_grid == grid and got.dtype == np.float32 and got.shape == dsm.shape
    holes = ~np.isfinite(dsm) | (dsm < -500.0)
    assert holes.sum() == 4 and np.isnan(got[holes]).all() and np.array_equal(got[~holes], dsm[~holes])
    ds = DD.DsmDepthDataset(_cfgs(tmp_path, depth_source="dsm", depth_prior_dsm_fp=fp, depth_prior_stride=3), device="cpu")
    import json
    with open(os.path.join(ON.SCENE, "root.json")) as f:
        train = json.load(f)["train_split"]
    assert ds.data_names == train and len(ds.pixels) == len(train) >= 2 and ds.stride == 3 and ds.weight == 1.0 and ds.grid == grid
    for m, pix in zip(ds.metas, ds.pixels):
        w, h = m["width"], m["height"]
        nx, ny = (w + 2) // 3, (h + 2) // 3
        assert pix.shape == (nx * ny, 2) and pix.dtype == np.float64
        assert pix[:, 0].max() == 3 * (nx - 1) < w and pix[:, 1].max() == 3 * (ny - 1) < h
        assert np.array_equal(pix[:nx], np.stack([np.arange(nx) * 3.0, np.zeros(nx)], 1)) and tuple(pix[nx]) == (0.0, 3.0)   # row-major
    assert np.array_equal(DD.strided_pixels(4, 2, 1), [[0, 0], [1, 0], [2, 0], [3, 0], [0, 1], [1, 1], [2, 1], [3, 1]])
    assert DD.strided_pixels(4, 2, 9).tolist() == [[0.0, 0.0]]
    ex = DD.image_extras(ds.metas[1], 1, 6)
    from snerf_amd.baseline.components.rays import construct_sun_dir
    assert ex.shape == (6, 4) and ex.dtype == torch.float32 and (ex[:, 3] == 1.0).all()
    assert torch.equal(ex[:, :3], construct_sun_dir(float(ds.metas[1]["sun_elevation"]), float(ds.metas[1]["sun_azimuth"]), 6))
    # a DSM without a georeference, with another raster type or without a zone is refused
    Image.fromarray(dsm, mode="F").save(str(tmp_path / "bare.tif"), format="TIFF")
    with pytest.raises(ValueError, match="carries no georeference"):
        DD.load_prior_dsm(str(tmp_path / "bare.tif"))
    labels = I.save_geotiff(str(tmp_path / "labels.tif"), np.zeros(dsm.shape, np.uint8), grid, "17R")
    with pytest.raises(ValueError, match="expected a float raster"):
        DD.load_prior_dsm(labels)
    with pytest.raises(ValueError, match="needs depth_prior_dsm_fp"):
        DD.DsmDepthDataset(types.SimpleNamespace(pipeline=types.SimpleNamespace(), run=None), device="cpu")
