"""Cast shadows on the map (include/snerf_hip.h, csrc/shadow.hip, eval/utils/shadow.py, eval/ortho.py export_shadow_check;
DESIGN.md section 5o) on an MI355X.  The kernels do only fp64 + - * / and integer work, so every comparison with the numpy
restatement (tests/shadow_numpy.py, itself held to a brute-force formulation by tests/test_shadow_cpu.py) is bit for bit:
torch.equal on `lit`, the fp32 bit patterns on `dist`, the integer words of the agreement."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import shadow_numpy as SN
from tests.test_gpu_fill import _filled, run_filled
from tests.test_gpu_geo import DSM_DIR
from tests.test_gpu_nadir import OPTS, T, _same, scene      # noqa: F401  (scene: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = 0.5
S2 = math.sqrt(0.5)

# azimuths 0 / 90 / 180 / 270 / 45 / 33.3 at elevations 2 (the march crosses the whole window) and 35 degrees, and the zenith
SUNS = [(el, az) for el in (2.0, 35.0) for az in (0.0, 90.0, 180.0, 270.0, 45.0, 33.3)] + [(90.0, 10.0)]
# hand-made rows: ux == 0 exactly and uy == 0 exactly (an infinite tDelta, both signs of the other component), ux == uy exactly (every
# step of the march is a tie) in all four quadrants
HAND = [(0.0, -1.0, 0.02), (0.0, 1.0, 0.3), (1.0, 0.0, 0.02), (-1.0, -0.0, 0.3), (S2, S2, 0.05), (-S2, S2, 0.3), (S2, -S2, 0.02),
        (-S2, -S2, 0.4)]
ROWS = np.concatenate([SN.sun_rows(SUNS, RES), np.asarray(HAND, np.float64)])
# the subset the largest shape runs (the restatement loops over h + w steps in Python): a low sun off the axes, a tie row, an infinite
# tDelta, a high sun
ROWS_LARGE = np.concatenate([SN.sun_rows([(2.0, 33.3), (35.0, 270.0)], RES), np.asarray([HAND[0], HAND[5], HAND[2]], np.float64)])
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 7), (16, 17), (33, 64), (130, 150)]
KINDS = ("flat", "tower", "random", "wall", "holes", "all-nan")


def _make_dsm(kind, h, w):
    rng = np.random.default_rng(1000 * h + w)
    if kind == "flat":
        d = np.full((h, w), 3.0)
    elif kind == "tower":
        d = np.zeros((h, w))
        d[h // 2, w // 2] = 30.0
    elif kind == "random":
        d = rng.uniform(0.0, 20.0, (h, w))
    elif kind == "wall":
        d = np.zeros((h, w))
        d[:, w // 2] = 15.0
    elif kind == "holes":
        d = rng.uniform(0.0, 20.0, (h, w))
        d[rng.random((h, w)) < 0.1] = np.nan
        d.flat[(h * w) // 2] = np.nan                    # a NaN start cell at every size
    else:
        d = np.full((h, w), np.nan)
    return d.astype(np.float32)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _assert_cast(dsm, rows, bias=0.0, z_top=None, ref_z_top=np.inf):
    """cast_rows with and without dist against the restatement: -> (lit, dist) as numpy"""
    from snerf_amd.eval.utils import shadow as S
    t = torch.from_numpy(dsm).to(DEV)
    lit, dist = S.cast_rows(t, rows, bias, z_top, want_dist=True)
    alone = S.cast_rows(t, rows, bias, z_top)
    assert torch.equal(lit, alone)                       # independent of dist_out being NULL
    want_lit, want_dist = SN.cast(dsm, rows, bias, ref_z_top)
    assert lit.dtype == torch.uint8 and tuple(lit.shape) == want_lit.shape and dist.dtype == torch.float32
    assert torch.equal(lit.cpu(), torch.from_numpy(want_lit))
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist))
    return want_lit, want_dist


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cast_matches_the_restatement_bit_for_bit(shape, kind):
    h, w = shape
    dsm = _make_dsm(kind, h, w)
    rows = ROWS_LARGE if h * w > 4096 else ROWS
    lit, dist = _assert_cast(dsm, rows)                  # z_top: the default (the largest finite altitude) against +inf
    assert np.array_equal(lit == SN.UNKNOWN, np.broadcast_to(np.isnan(dsm), lit.shape))
    assert np.array_equal(np.isnan(dist), lit != 0)
    if kind == "flat":
        assert bool((lit == 1).all())
    if kind == "all-nan":
        assert bool((lit == SN.UNKNOWN).all())
    if kind in ("tower", "wall") and w >= 5:
        assert bool((lit == 0).any())


def test_analytic_box():
    """A box of height 10 m on a plane at res = 0.5, elevation 45 degrees, sun due east: rise = tan(45 deg) * 0.5 = 0.5 m per cell,
    ux = 1 so tDeltaX = 1 and the entries are t = 0.5, 1.5, ...  A ground cell d cells west of the box's west face (h0 = 0 + bias,
    bias = 0) enters the face's cell at its d-th step, t = d - 0.5, where hr = 0.5 (d - 0.5); the cells before it are ground
    (0 > hr is false).  It is shadowed iff 10 > 0.5 (d - 0.5), i.e. d < 20.5: EXACTLY 20 cells, d = 1 .. 20, west of each box row,
    at distances 0.5 .. 19.5.  The box's own cells and everything east of it are lit (10 > 10 + 0.5 t is false)."""
    from snerf_amd.eval.utils import shadow as S
    dsm = np.zeros((5, 40), np.float32)
    dsm[1:4, 30:33] = 10.0
    rows = np.array([[1.0, -0.0, 0.5]])                  # what sun_rows gives up to the last bits of cos(90 deg) and tan(45 deg)
    assert np.allclose(S.sun_rows([(45.0, 90.0)], 0.5), rows, rtol=0, atol=1e-15)
    lit, dist = _assert_cast(dsm, rows)
    for j in (1, 2, 3):
        assert int((lit[0, j] == 0).sum()) == 20 and bool((lit[0, j, 10:30] == 0).all())
        assert np.array_equal(dist[0, j, 10:30], np.arange(20, 0, -1, dtype=np.float32) - 0.5)
    assert bool((lit[0, (0, 4)] == 1).all()) and bool((lit[0, :, 30:] == 1).all())
    # the public entry under the degrees themselves: the same 20 cells (the march stays 1e-16 from the axis over 40 cells)
    pub = S.cast_shadows(torch.from_numpy(dsm).to(DEV), [(45.0, 90.0)], 0.5).cpu().numpy()
    assert [int((pub[0, j] == 0).sum()) for j in range(5)] == [0, 20, 20, 20, 0]


def test_the_ray_height_is_rounded_twice():
    """hr = h0 + rise * t is a product rounded to fp64 and a sum rounded to fp64, never one fused multiply-add -- the restatement
    (two numpy ufuncs) can only be matched bit for bit that way, and random DSMs do not show the difference.  A case that does:
    rise = 1 + 2^-52 and t = 1.5 (the second x step under ux = 1), where 1.5 rise lies exactly between two doubles and rounds up
    to p = 1.5 + 2^-51; with bias = -p on a plane at 0, two roundings give hr = 0 at that step, and 0 > 0 does not block, while a
    fused multiply-add gives the product's rounding error, -2^-53 < 0, and the plane would shadow itself.  (The first step's cell
    is a hole, which never blocks; from the third step on hr > 0.)"""
    from fractions import Fraction
    rise = np.nextafter(1.0, 2.0)
    p = np.float64(1.5) * rise
    assert Fraction(float(p)) - Fraction(1.5) * Fraction(float(rise)) == Fraction(1, 2 ** 53) and -p + p == 0.0
    dsm = np.zeros((1, 6), np.float32)
    dsm[0, 1] = np.nan
    rows = np.array([[1.0, 0.0, rise]])
    lit, _ = _assert_cast(dsm, rows, bias=float(-p), z_top=math.inf)
    assert lit[0, 0, 0] == 1                             # shadowed under a fused multiply-add


def test_z_top_is_only_an_early_exit_and_bias_lifts_the_start():
    from snerf_amd.eval.utils import shadow as S
    dsm = _make_dsm("holes", 33, 64)
    t = torch.from_numpy(dsm).to(DEV)
    top = float(np.nanmax(dsm))
    res = [S.cast_rows(t, ROWS, 0.0, z, want_dist=True) for z in (math.inf, top, None, top + 100.0)]
    for lit, dist in res[1:]:
        assert torch.equal(lit, res[0][0]) and _same(dist, res[0][1])
    _assert_cast(dsm, ROWS, z_top=top, ref_z_top=top)                   # the restatement takes the same exit
    low = float(np.nanmedian(dsm))                                      # below the top it IS a different question: lit can only grow
    lit_low = S.cast_rows(t, ROWS, 0.0, low)
    assert torch.equal(lit_low.cpu(), torch.from_numpy(SN.cast(dsm, ROWS, 0.0, low)[0]))
    assert bool((lit_low >= res[0][0]).all()) and not torch.equal(lit_low, res[0][0])
    lit_b, _ = _assert_cast(dsm, ROWS, bias=0.75)
    assert int((lit_b == 0).sum()) < int((res[0][0] == 0).sum())


@pytest.mark.parametrize("K", (1, 3, 64))
def test_k_suns_in_one_call_equal_k_calls(K):
    from snerf_amd.eval.utils import shadow as S
    rng = np.random.default_rng(K)
    suns = np.stack([rng.uniform(1.0, 80.0, K), rng.uniform(0.0, 360.0, K)], 1)
    dsm = _make_dsm("holes", 16, 17)
    rows = SN.sun_rows(suns, RES)
    lit, dist = _assert_cast(dsm, rows)
    t = torch.from_numpy(dsm).to(DEV)
    for k in range(K):
        one_lit, one_dist = S.cast_rows(t, rows[k:k + 1], want_dist=True)
        assert torch.equal(one_lit[0].cpu(), torch.from_numpy(lit[k]))
        assert np.array_equal(_bits(one_dist[0].cpu().numpy()), _bits(dist[k]))
    pub = S.cast_shadows(t, [tuple(s) for s in suns], RES)               # the public entry evaluates the same rows
    assert torch.equal(pub.cpu(), torch.from_numpy(lit))


def test_more_than_64_suns_are_cut_into_calls():
    from snerf_amd.eval.utils import shadow as S
    suns = [(5.0 + k, 5.0 * k) for k in range(70)]
    dsm = _make_dsm("random", 5, 7)
    t = torch.from_numpy(dsm).to(DEV)
    lit, dist = S.cast_shadows(t, suns, RES, want_dist=True)
    want = SN.cast(dsm, SN.sun_rows(suns, RES))
    assert tuple(lit.shape) == (70, 5, 7) and torch.equal(lit.cpu(), torch.from_numpy(want[0]))
    assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want[1]))
    with pytest.raises(ValueError, match="n_suns = 65"):                  # the library itself refuses what the host layer cuts
        from snerf_amd import _lib
        rows = np.ascontiguousarray(SN.sun_rows(suns[:65], RES))
        _lib.call("snerf_shadow_cast", t, 5, 7, rows.ctypes.data, 65, 0.0, math.inf, torch.empty((65, 5, 7), dtype=torch.uint8, device=DEV),
                  None, exc=ValueError)


# ---- the agreement ---------------------------------------------------------------------------------------------------------------
VALUES = np.array([0.0, 0.25, 0.3, 0.5, 0.75, 1.0, -1.5, 3e38, np.nan, np.inf, -np.inf], np.float32)


def _agreement_case(cells, K, seed):
    rng = np.random.default_rng(seed)
    sun = np.concatenate([VALUES[rng.integers(0, len(VALUES), (K, cells // 2))], rng.random((K, cells - cells // 2)).astype(np.float32)], 1)
    lit = rng.choice(np.array([0, 1, 255], np.uint8), (K, cells), p=(0.45, 0.45, 0.1))
    valid = (rng.random(cells) < 0.8).astype(np.uint8)
    return sun, lit, valid


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("cells", (1, 63, 64, 65, 4097))
def test_agreement_words_are_the_integer_restatement(cells, K):
    from snerf_amd.eval.utils import shadow as S
    sun, lit, valid = _agreement_case(cells, K, 7 * cells + K)
    ts, tl, tv = (torch.from_numpy(a).to(DEV) for a in (sun, lit, valid))
    for v, tvv in ((None, None), (valid, tv)):
        for thr in (0.5, 0.3):                           # 0.5 occurs in `sun`; fp32(0.3) occurs and is >= the fp64 0.3
            want = SN.agreement(sun, lit, v, thr)
            got = S.agreement_words(ts, tl, tvv, thr)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy().view(np.uint64), want), (v is None, thr)
            assert bool((want[:, :5].sum(1) == cells).all()) and bool((want[:, 7] == 0).all())
            figures = S.shadow_agreement(ts, tl, tvv, thr)
            for k in range(K):
                m = SN.metrics(want[k])
                f = dict(figures[k])
                assert f.pop("words") == [int(x) for x in want[k]]
                assert all(f[key] == m[key] or (math.isnan(f[key]) and math.isnan(m[key])) for key in m), (f, m)
    if cells > 1:                                        # the two halves of a map accumulated in two calls equal one call
        cut = cells // 2 - 1 if cells > 2 else 1
        acc = S.agreement_words(ts[:, :cut], tl[:, :cut], tv[:cut], 0.5)
        acc = S.agreement_words(ts[:, cut:], tl[:, cut:], tv[cut:], 0.5, acc=acc)
        assert np.array_equal(acc.cpu().numpy().view(np.uint64), SN.agreement(sun, lit, valid, 0.5))


# ---- unwritten memory ------------------------------------------------------------------------------------------------------------
def test_no_output_depends_on_bytes_the_library_did_not_write():
    """both entries under the fills of tests/test_gpu_fill.py: lit_out / dist_out are pure outputs (filled before the call), acc is an
    accumulator the caller zeroes; two runs under each fill and the three fills are bit-identical, and equal the restatement"""
    from snerf_amd import _lib
    h, w = 33, 64
    dsm = _make_dsm("holes", h, w)
    rows = np.ascontiguousarray(ROWS)
    K = len(rows)
    t = torch.from_numpy(dsm).to(DEV)
    sun, lit_in, valid = _agreement_case(h * w, K, 5)
    ts, tl, tv = (torch.from_numpy(a).to(DEV) for a in (sun, lit_in, valid))

    def run(fill):
        lit, dist = _filled((K, h, w), torch.uint8, fill), _filled((K, h, w), torch.float32, fill)
        _lib.call("snerf_shadow_cast", t, h, w, rows.ctypes.data, K, 0.0, math.inf, lit, dist)
        acc = torch.zeros((K, 8), dtype=torch.int64, device=DEV)
        _lib.call("snerf_shadow_agreement", ts, tl, tv, h * w, K, 0.5, acc)
        return {"lit": lit, "dist": dist, "acc": acc}

    r = run_filled(run)[0xFF]
    want = SN.cast(dsm, rows)
    assert torch.equal(r["lit"].cpu(), torch.from_numpy(want[0])) and np.array_equal(_bits(r["dist"].cpu().numpy()), _bits(want[1]))
    assert np.array_equal(r["acc"].cpu().numpy().view(np.uint64), SN.agreement(sun, lit_in, valid, 0.5))


# ---- end to end: the fixture scene's seeded, untrained model on a 9 x 11 window, three suns, {"perturb": 0} --------------------------
H, W = 9, 11
SWEEP_SUNS = [(35.0, 120.0), (62.5, 201.0), (12.0, 300.0)]


@pytest.fixture(scope="module")
def truth():
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.framework.util import img_utils as I
    d = os.path.join(DSM_DIR, "dsm")
    g = I.load_dsm_ground_truth(os.path.join(d, "JAX_068_DSM.tif"), os.path.join(d, "JAX_068_DSM.txt"), os.path.join(d, "JAX_068_CLS.tif"))
    roi = D.roi_grid(g["roi"])
    return {"window": D.grid_struct(roi, (0, 0, W, H)), "gt": g["gt"][:H, :W].contiguous().to(DEV),
            "water_mask": g["water_mask"][:H, :W].contiguous().to(DEV)}


def _sweep_args(ds, geo, truth):
    return dict(geo=geo, grid=truth["window"], min_alt=min(it["alt_min"] for it in ds.items),
                max_alt=max(it["alt_max"] for it in ds.items), t=T, render_options=OPTS, suns=SWEEP_SUNS)


@pytest.fixture(scope="module")
def sweep(scene, truth):
    from snerf_amd.eval.utils.ortho import nadir_sun_sweep
    c, pipe, ds, geo = scene
    return nadir_sun_sweep(c, pipe.renderer, pipe.models, **_sweep_args(ds, geo, truth))


def test_shadow_check_on_the_sweep(sweep, truth):
    from snerf_amd.eval.utils import shadow as S
    chk = S.shadow_check(sweep, gt=truth["gt"], water_mask=truth["water_mask"])
    assert sorted(chk) == ["agreement_gt", "agreement_model", "cast_gt", "cast_model", "disagree", "suns"]
    assert sorted(S.shadow_check(sweep)) == ["agreement_model", "cast_model", "disagree", "suns"]
    assert chk["suns"] == SWEEP_SUNS
    for key in ("cast_model", "cast_gt", "disagree"):
        assert tuple(chk[key].shape) == (3, H, W) and chk[key].dtype == torch.uint8 and chk[key].is_cuda, key
    res = sweep["grid"].resolution
    assert torch.equal(chk["cast_model"], S.cast_shadows(sweep["dsm"], SWEEP_SUNS, res))
    assert torch.equal(chk["cast_model"].cpu(), torch.from_numpy(SN.cast(sweep["dsm"].cpu().numpy(), SN.sun_rows(SWEEP_SUNS, res))[0]))
    gt = truth["gt"].cpu().numpy().astype(np.float32)
    gt[gt < -500.0] = np.nan
    assert torch.equal(chk["cast_gt"].cpu(), torch.from_numpy(SN.cast(gt, SN.sun_rows(SWEEP_SUNS, res))[0]))
    valid = (truth["water_mask"] != 9).cpu().numpy().astype(np.uint8)
    for key, cast in (("agreement_model", chk["cast_model"]), ("agreement_gt", chk["cast_gt"])):
        want = SN.agreement(sweep["sun"].cpu().numpy(), cast.cpu().numpy(), valid, 0.5)
        assert len(chk[key]) == 3
        for k, a in enumerate(chk[key]):
            assert sorted(a) == sorted(S.METRICS + ("words",))
            assert a["words"] == [int(v) for v in want[k]] and sum(a["words"][:5]) == H * W
            print(f"{key} sun {k} {SWEEP_SUNS[k]}: " + ", ".join(f"{m} {a[m]:.4g}" for m in S.METRICS))
    for k, a in enumerate(chk["agreement_model"]):
        assert int((chk["disagree"][k] == 1).sum()) == a["words"][1] + a["words"][2]
        assert int((chk["disagree"][k] == 255).sum()) == a["words"][4]


def _read_all(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_export_writes_the_named_files_and_leaves_the_sweep_export_alone(scene, truth, sweep, tmp_path):
    from snerf_amd.eval.ortho import export_shadow_check, export_sun_sweep
    from snerf_amd.eval.utils import shadow as S
    from snerf_amd.framework.util import img_utils as I
    c, pipe, ds, geo = scene
    a = _sweep_args(ds, geo, truth)
    before = export_sun_sweep(c, pipe.renderer, pipe.models, str(tmp_path / "a"), **a)
    out = export_shadow_check(c, pipe.renderer, pipe.models, str(tmp_path / "s"), gt=truth["gt"], water_mask=truth["water_mask"], **a)
    after = export_sun_sweep(c, pipe.renderer, pipe.models, str(tmp_path / "b"), **a)
    files_a, files_b = _read_all(tmp_path / "a" / "nadir" / "sweep"), _read_all(tmp_path / "b" / "nadir" / "sweep")
    assert files_a == files_b and len(files_a) == 4 * 3 + 3 and set(before["files"]) == set(after["files"]) == set(files_a)
    chk = out["shadow_check"]
    assert _same(out["sun"], sweep["sun"]) and _same(out["dsm"], sweep["dsm"])
    assert torch.equal(chk["cast_model"], S.shadow_check(sweep)["cast_model"])
    names = {f"cast_{k:03d}{e}" for k in range(3) for e in (".png", ".tif")} | {f"disagree_{k:03d}.png" for k in range(3)} | {"shadow_check.json"}
    d = tmp_path / "s" / "nadir" / "shadow"
    assert set(out["files"]) == names == set(os.listdir(d))
    grid = out["grid"]
    for k in range(3):
        arr, tf = I.load_dsm_geotiff(out["files"][f"cast_{k:03d}.tif"])
        assert arr.dtype == np.uint8 and tf == (grid.xoff, grid.yoff, grid.resolution, grid.resolution)
        assert np.array_equal(arr, chk["cast_model"][k].cpu().numpy())
    with open(out["files"]["shadow_check.json"]) as f:
        doc = json.load(f)
    assert doc["bias"] == 0.0 and doc["threshold"] == 0.5
    assert [(s["elevation_deg"], s["azimuth_deg"]) for s in doc["suns"]] == SWEEP_SUNS
    for key in ("agreement_model", "agreement_gt"):
        assert [a["words"] for a in doc[key]] == [a["words"] for a in chk[key]]
        for got, want in zip(doc[key], chk[key]):
            assert all(got[m] == want[m] or (math.isnan(got[m]) and math.isnan(want[m])) for m in S.METRICS)
