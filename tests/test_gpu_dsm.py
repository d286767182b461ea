"""DSM evaluation on the GPU (csrc/dsm.hip through snerf_amd.eval.utils.dsm): rasterisation against the numpy fp64
restatement, bit-reproducibility and the ROI crop, the overflow guard, the pyramid + NCC search + shift + MAE against the
reference's golden vectors, an end-to-end run from rays and depths, the validation step, and two data-parallel ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dsm_numpy as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(p for p in (os.path.join(ROOT, "tests", "golden", f) for f in os.listdir(os.path.join(ROOT, "tests", "golden")))
                if os.path.basename(p).startswith("dsmr_"))
DEV = "cuda:0"


def _dsm():
    from snerf_amd.eval.utils import dsm
    return dsm


def _cloud(n, xsize, ysize, res, zc, zs, seed, margin=3.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-margin * res, (xsize + margin) * res, n) + 1000.0
    y = rng.uniform(-margin * res, (ysize + margin) * res, n) + 2000.0
    z = zc + zs * rng.standard_normal(n)
    return np.stack([x, y, z], 1)


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("zc,zs", [(300.0, 20.0), (1.0, 0.2)], ids=["metric", "normalised"])
def test_rasterize_matches_numpy(radius, zc, zs):
    D = _dsm()
    res = 0.5
    # grid (xoff, yoff) = (1000, 2000 + 40 res): points fall up to 3 cells outside it on every side
    grid = D.DsmGrid(1000.0, 2000.0 + 40 * res, res, 50, 40)
    cloud = _cloud(20000, 50, 40, res, zc, zs, seed=radius)
    want, cnt = N.rasterize(cloud, *grid, radius=radius)
    c = torch.from_numpy(cloud).to(DEV)
    got = D.rasterize(c, grid, radius=radius).cpu().numpy()
    count, _, _ = D._accumulate(c, grid, (0, 0, grid.xsize, grid.ysize), radius)
    assert np.array_equal(count.cpu().numpy().reshape(40, 50), cnt)
    assert np.array_equal(np.isnan(got), cnt == 0)
    ulp = float(np.spacing(np.float32(np.abs(cloud[:, 2]).max())))
    ok = cnt > 0
    assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= ulp


def test_rasterize_contention_1m_points_bitwise_and_roi_crop():
    """1M points on 50 x 50 cells (~3,600 contributions per cell with radius 1): numpy parity, two calls bit-identical, the ROI
    path = the bounds grid cropped by an integer offset, bit for bit"""
    D = _dsm()
    cloud = _cloud(1 << 20, 50, 50, 0.5, 250.0, 10.0, seed=7, margin=0.0)
    c = torch.from_numpy(cloud).to(DEV)
    bounds = D.dsm_grid_from_cloud(c)
    assert bounds == N.bounds_grid(cloud)
    want, cnt = N.rasterize(cloud, *bounds)
    a = D.create_dsm(c)
    b = D.create_dsm(c[torch.randperm(c.shape[0], device=DEV)])          # another arrival order of the same points
    assert torch.equal(a.view(torch.int32), D.create_dsm(c).view(torch.int32))
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    got = a.cpu().numpy()
    assert cnt.min() > 100
    assert np.abs(got.astype(np.float64) - want).max() <= float(np.spacing(np.float32(np.abs(cloud[:, 2]).max())))
    # ROI: 20 x 20 cells starting 7 cells east and 5 cells south of the bounds corner, and one hanging over the east edge
    res = bounds.resolution
    for i0, j0, n in ((7, 5, 20), (bounds.xsize - 6, 3, 12)):
        meta = [bounds.xoff + i0 * res, bounds.yoff - j0 * res - n * res, n, res]
        roi = D.create_dsm(c, roi=meta).cpu().numpy()
        crop = np.full((n, n), np.nan, np.float32)
        w = min(n, bounds.xsize - i0)
        crop[:, :w] = got[j0:j0 + n, i0:i0 + w]
        assert np.array_equal(roi.view(np.uint32), crop.view(np.uint32))
    with pytest.raises(ValueError, match="off the DSM lattice"):
        D.create_dsm(c, roi=[bounds.xoff + 0.25, bounds.yoff - 10.0, 8, res])
    with pytest.raises(ValueError, match="resolution"):
        D.create_dsm(c, roi=[bounds.xoff, bounds.yoff - 10.0, 8, 1.0])


def test_rasterize_overflow_is_an_error(monkeypatch):
    """a quantisation step so fine that the int64 cell sums could wrap: an error from the host-side bound, never a DSM"""
    D = _dsm()
    c = torch.from_numpy(_cloud(50000, 10, 10, 0.5, 300.0, 1.0, seed=3, margin=0.0)).to(DEV)
    grid = D.dsm_grid_from_cloud(c)
    monkeypatch.setattr(D, "Q", 1e-15)                  # |k| ~ 3e17, hundreds of points per cell: sums up to ~1e20 > 2^63
    with pytest.raises(OverflowError, match="overflow"):
        D.rasterize(c, grid)
    monkeypatch.setattr(D, "Q", 1e-17)                  # |k| ~ 3e19 > 2^62: not representable at all
    with pytest.raises(OverflowError, match="2\\^62"):
        D.rasterize(c, grid)
    monkeypatch.undo()
    assert bool(torch.isfinite(D.rasterize(c, grid)).any())


def test_bad_point_count_is_a_count():
    """stats[1] counts the points with an unusable altitude (include/snerf_hip.h): three in the first wave, one of them at its
    last lane, and one in each of the next two waves give 6 -- a sum over the waves, not a maximum per wave"""
    D = _dsm()
    grid = D.DsmGrid(1000.0, 2000.0 + 7 * 0.5, 0.5, 9, 7)
    cloud = _cloud(200, 9, 7, 0.5, 300.0, 20.0, seed=23, margin=0.0)
    bad = [0, 1, 2, 63, 64, 130]
    cloud[bad, 2] = np.nan
    c = torch.from_numpy(cloud).to(DEV)
    count, _, stats = D._accumulate(c, grid, (0, 0, grid.xsize, grid.ysize), 1)
    print("stats", stats.tolist())
    assert int(stats[1]) == len(bad) == 6
    assert np.array_equal(count.cpu().numpy().reshape(7, 9), N.rasterize(np.delete(cloud, bad, 0), *grid, radius=1)[1])
    with pytest.raises(OverflowError, match="6 point"):
        D.rasterize(c, grid)


# ---- one cell arithmetic for the DSM, the top surface and the votes (csrc/lattice.h) --------------------------------------------
LW, LH, LRES = 9, 7, 0.5
LGRID = (1000.0, 2000.0 + LH * LRES, LRES, LW, LH)
# (ioff, joff, out_w, out_h): the whole extent, inside it, larger than the lattice from a negative origin, over the east edge
LWINDOWS = {"whole": (0, 0, LW, LH), "inside": (2, 1, 6, 5), "beyond": (-2, -1, 20, 30), "east-edge": (6, 2, 6, 4)}
_LATTICE = {}


def _lattice_cloud():
    """2,000 points up to 8 cells outside the 9 x 7 lattice on every side, five of them without a finite x or y; labels in range"""
    if not _LATTICE:
        xyz = _cloud(2000, LW, LH, LRES, 100.0, 150.0, seed=29, margin=8.0)
        xyz[:, 2] = np.clip(xyz[:, 2], -1000.0, 1000.0)
        xyz[[3, 700], 0] = np.nan, -np.inf
        xyz[[64, 1999], 1] = np.inf, np.nan
        xyz[1000, :2] = np.inf, -np.inf
        _LATTICE.update(xyz=xyz, labels=np.random.default_rng(30).integers(0, 5, 2000), dev=torch.from_numpy(xyz).to(DEV), counts={})
        _LATTICE["dev_labels"] = torch.from_numpy(_LATTICE["labels"]).to(DEV)
    return _LATTICE


def _window_count(radius, window):
    """tests/dsm_numpy.py's count on the whole extent (once per radius), read through the window; 0 outside the lattice"""
    L = _lattice_cloud()
    if radius not in L["counts"]:
        L["counts"][radius] = N.rasterize(L["xyz"], *LGRID, radius=radius)[1]
    ioff, joff, w, h = window
    out = np.zeros((h, w), np.int64)
    i0, i1, j0, j1 = max(ioff, 0), min(ioff + w, LW), max(joff, 0), min(joff + h, LH)
    out[j0 - joff:j1 - joff, i0 - ioff:i1 - ioff] = L["counts"][radius][j0:j1, i0:i1]
    return out


@pytest.mark.parametrize("radius", (0, 1, 2, 7))
@pytest.mark.parametrize("window", LWINDOWS)
def test_the_three_splats_agree_cell_for_cell(window, radius):
    """a cell's DSM count = the sum of its votes over the classes, and it has a top-surface key exactly when that count is not 0:
    all three entries offer a point to the same cells (both header sections state one rule); the count is dsm_numpy's"""
    from snerf_amd import _lib
    from snerf_amd.eval.utils import ortho as OR
    D = _dsm()
    L = _lattice_cloud()
    ioff, joff, w, h = LWINDOWS[window]
    grid = D.DsmGrid(*LGRID)
    g = _lib.SnerfDsmGrid(*LGRID, ioff, joff, w, h)
    count, _, dstats = D._accumulate(L["dev"], grid, LWINDOWS[window], radius)
    top, tstats = OR.top_surface(L["dev"], g, radius)
    votes, vstats = OR.label_votes(L["dev"], L["dev_labels"], g, 5, radius)
    count = count.cpu().numpy().astype(np.int64).reshape(h, w)
    want = _window_count(radius, LWINDOWS[window])
    print(window, radius, "cells reached", int((count > 0).sum()), "of", h * w, "offers", int(count.sum()), "bad", int(dstats[1]),
          int(tstats[0]), int(vstats[0]))
    assert (want > 0).any()
    assert np.array_equal(count, want)
    assert np.array_equal(votes.cpu().numpy().astype(np.int64).sum(0), count)
    assert np.array_equal(top.cpu().numpy() != 0, count > 0)
    assert int(dstats[1]) == 0 and int(tstats[0]) == 0 and int(vstats[0]) == 5


@pytest.mark.parametrize("radius", (8, 64))
def test_rasterize_radius_beyond_the_ortho_limit(radius):
    """the DSM's own radius bound is 64, above the ortho entries' 7: windows far wider than the lattice, clipped on every side"""
    D = _dsm()
    grid = D.DsmGrid(*LGRID)
    cloud = _cloud(300, LW, LH, LRES, 300.0, 20.0, seed=31, margin=radius + 6.0)      # some own cells lie too far out to reach a cell
    want, cnt = N.rasterize(cloud, *grid, radius=radius)
    c = torch.from_numpy(cloud).to(DEV)
    got = D.rasterize(c, grid, radius=radius).cpu().numpy()
    count, _, _ = D._accumulate(c, grid, (0, 0, grid.xsize, grid.ysize), radius)
    print(radius, "count min / max", int(cnt.min()), int(cnt.max()))
    assert np.array_equal(count.cpu().numpy().reshape(LH, LW), cnt) and 1 < cnt.max() < 300
    assert np.array_equal(np.isnan(got), cnt == 0)
    ulp = float(np.spacing(np.float32(np.abs(cloud[:, 2]).max())))
    ok = cnt > 0
    assert np.abs(got[ok].astype(np.float64) - want[ok]).max() <= ulp


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_registration_and_mae_vs_reference_golden(path):
    D = _dsm()
    z = np.load(path)
    gt = torch.from_numpy(z["gt"]).to(DEV)
    v = torch.from_numpy(z["v"]).to(DEV)
    u_l, v_l = gt, v
    for k in range(1, int(z["n_levels"]) + 1):
        u_l, v_l = D.downsample2x(u_l), D.downsample2x(v_l)
        assert np.array_equal(u_l.cpu().numpy(), z[f"ds_u_{k}"], equal_nan=True)
        assert np.array_equal(v_l.cpu().numpy(), z[f"ds_v_{k}"], equal_nan=True)
    trace = []
    dx, dy, a, b = D.compute_shift(gt, v, init=tuple(int(x) for x in z["init"]), trace=trace)
    assert [list(t) for t in trace] == z["shifts"].tolist()
    assert (dx, dy, a) == (int(z["dx"]), int(z["dy"]), 1)
    assert abs(b - float(z["b"])) <= 1e-9 * abs(float(z["b"]))
    kw = {}
    if "water" in z.files:
        kw["water_mask"] = torch.from_numpy(z["water"]).to(DEV)
    pred = torch.from_numpy(z["pred"]).to(DEV)
    init = tuple(int(x) for x in z["init"])
    m = D.compute_mae(pred, gt, init=init, **kw)
    assert (m["dx"], m["dy"]) == (int(z["dx"]), int(z["dy"]))
    r, rz = m["rdsm"].cpu().numpy(), z["rdsm"]
    assert np.array_equal(np.isnan(r), np.isnan(rz))
    fin = ~np.isnan(rz)
    assert np.all(np.abs(r[fin] - rz[fin]) <= np.spacing(np.abs(rz[fin])))       # 1 ulp
    assert abs(m["mean"] - float(z["mean"])) <= 1e-6 * float(z["mean"])
    assert abs(m["median"] - float(z["median"])) <= 1e-6 * float(z["median"])
    assert torch.equal(D.apply_shift(v, dx, dy, 1, m["b"]).view(torch.int32), m["rdsm"].view(torch.int32))


def test_apply_shift_and_median_rule():
    D = _dsm()
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 10, (6, 7)).astype(np.float32)
    x[2, 3] = np.nan
    got = D.apply_shift(torch.from_numpy(x).to(DEV), 2, -1, 1, 0.125).cpu().numpy()
    want = (N._shifted(x.astype(np.float64), 2, -1) + 0.125).astype(np.float32)
    assert np.array_equal(got, want, equal_nan=True)
    for n in (8, 9):                                         # even and odd finite counts
        a = rng.uniform(0, 1, n).astype(np.float32)
        a = np.concatenate([a, [np.nan, np.inf]]).astype(np.float32)
        assert D.nanmedian_numpy(torch.from_numpy(a).to(DEV)) == float(np.median(a[np.isfinite(a)]))


@pytest.mark.parametrize("shape", ((37, 53), (520, 521)))
def test_shift_diff_totals_are_the_restated_summation_order_bit_for_bit(shape):
    """snerf_dsm_shift_diff's (sum |diff|, count) against tests/dsm_numpy.py shift_diff_totals as bits; (520, 521) has more
    than 1024 x 256 cells, so the grid-stride loop runs"""
    D = _dsm()
    rng = np.random.default_rng(shape[0])
    pred = (rng.standard_normal(shape) * 2.0 ** rng.integers(-8, 9, shape)).astype(np.float32)
    pred[rng.random(shape) < 0.05] = np.nan
    gt = (rng.standard_normal(shape) * 30).astype(np.float32)
    gt[rng.random(shape) < 0.05] = -9999.0
    want = N.shift_diff_totals(pred, gt, 3, -2, 0.37)
    _, _, totals = D._shift_diff(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), 3, -2, 0.37)
    got = totals.cpu().numpy()
    print(f"{shape}: kernel {got.tolist()!r}, restated {want!r}")
    assert np.array_equal(got.view(np.int64), np.array(want, np.float64).view(np.int64)), (got.tolist(), want)


def _nadir(field, res, xoff, yoff, z_top=500.0):
    """one nadir ray per cell centre of `field` (rows from the north), with the depth that puts its end point on the field"""
    h, w = field.shape
    jj, ii = np.mgrid[0:h, 0:w]
    e = xoff + (ii + 0.5) * res
    n = yoff - (jj + 0.5) * res
    rays = np.zeros((h * w, 8))
    rays[:, 0], rays[:, 1], rays[:, 2] = e.ravel(), n.ravel(), z_top
    rays[:, 5] = -1.0
    depth = z_top - field.ravel()
    return rays, depth


def test_end_to_end_rays_to_mae_recovers_injected_shift():
    D = _dsm()
    res, h, w = 0.5, 120, 130
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(11)
    field = 30.0 + 3.0 * np.sin(x / 9.0) + 2.0 * np.cos(y / 7.0)
    for _ in range(25):
        j, i = rng.integers(0, h - 10), rng.integers(0, w - 10)
        field[j:j + rng.integers(3, 10), i:i + rng.integers(3, 10)] += rng.uniform(3.0, 12.0)
    xoff, yoff = 5000.0, 8000.0
    rays, depth = _nadir(field, res, xoff, yoff)
    cloud = rays[:, :3] + rays[:, 3:6] * depth[:, None]
    bounds = N.bounds_grid(cloud)
    gt = N.rasterize(cloud, *bounds)[0].astype(np.float32)
    n = 100
    meta = [bounds[0] + 8 * res, bounds[1] - 6 * res - n * res, n, res]
    gt_roi = torch.from_numpy(gt[6:6 + n, 8:8 + n].copy()).to(DEV)
    r64, d64 = torch.from_numpy(rays).to(DEV), torch.from_numpy(depth).to(DEV)
    out = D.compute_dsm_and_mae(r64, d64, gt_roi, meta)
    assert (out["dx"], out["dy"]) == (0, 0) and abs(out["b"]) <= 1e-5
    assert out["mean"] <= 1e-5 and out["median"] <= 1e-5
    # inject a shift of (+2, -1) cells and a bias of 0.7 m through to_world: the registration undoes both
    shift = torch.tensor([2 * res, 1 * res, 0.7], dtype=torch.float64, device=DEV)
    out = D.compute_dsm_and_mae(r64, d64, gt_roi, meta, to_world=lambda xyz: xyz + shift)
    assert (out["dx"], out["dy"]) == (2, -1)
    assert abs(out["b"] + 0.7) <= 1e-5
    assert out["mean"] <= 1e-5


_DDP_DSM_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
from snerf_amd import parallel
from snerf_amd.eval.utils import dsm as D
rank, world, dev = parallel.init_distributed(backend="gloo")
cloud = torch.from_numpy(np.load({cloud!r})).to("cuda:0")
lo, hi = parallel.frame_shard(cloud.shape[0])
out = D.create_dsm(cloud[lo:hi], roi={meta!r}, distributed=True)
np.save({out!r} + f".{{rank}}.npy", out.cpu().numpy())
dist.barrier()
"""


def test_data_parallel_dsm_equals_single_process(tmp_path):
    """2 ranks (gloo, both on this GPU), each with half of the cloud: the all-reduced integer accumulators give every rank the
    DSM of the whole cloud, bit for bit"""
    D = _dsm()
    cloud = _cloud(200000, 60, 60, 0.5, 120.0, 5.0, seed=17, margin=0.0)
    c = torch.from_numpy(cloud).to(DEV)
    b = D.dsm_grid_from_cloud(c)
    meta = [b.xoff + 3 * 0.5, b.yoff - 4 * 0.5 - 50 * 0.5, 50, 0.5]
    single = D.create_dsm(c, roi=meta).cpu().numpy()
    np.save(tmp_path / "cloud.npy", cloud)
    script = tmp_path / "worker.py"
    out = str(tmp_path / "dsm")
    script.write_text(_DDP_DSM_WORKER.format(root=ROOT, cloud=str(tmp_path / "cloud.npy"), meta=meta, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29637", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0"), cwd=ROOT)
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    for r in range(2):
        got = np.load(out + f".{r}.npy")
        assert np.array_equal(got.view(np.uint32), single.view(np.uint32)), r


def test_validation_step_logs_mae_only_with_a_dsm_entry():
    """validation_step with batch["dsm"]: logs f"{split}/mae" for batch_idx <= 1 from depth_coarse (= compute_dsm_and_mae on
    the step's own rays and depths); without the entry the return dict and the logged keys are those of the plain step"""
    from oracle import snerf_oracle as O
    from tests.test_gpu_pipeline import _pipeline_for
    D = _dsm()
    cfg = O.OracleCfg(fc_units=32, n_samples=16, first_beta_epoch=0)
    pipe, _ = _pipeline_for(cfg, 256, 3)
    pipe._val_render_options = lambda split: {"perturb": 0}
    bank = O.batch_to_torch(O.synthetic_batch(4096, 16, seed=12))
    batch = {"rays": bank["rays"].to(DEV), "rgbs": bank["rgbs"].to(DEV), "extras": bank["extras"].to(DEV), "split": "test",
             "semantic": bank["semantic"].to(torch.uint8).to(DEV), "semantic_sparsity_mask": bank["mask"].to(DEV)}
    pipe.logged.clear()
    plain = pipe.validation_step(dict(batch), 0)
    plain_logged = sorted(pipe.logged)
    assert "mae" not in plain and not any(k.endswith("/mae") for k in plain_logged)
    xyz = (batch["rays"][:, :3].double() + batch["rays"][:, 3:6].double() * plain["results"]["depth_coarse"].double()[:, None])
    ext = float((xyz[:, :2].max(0).values - xyz[:, :2].min(0).values).max())
    scale = 30.0 / ext                                            # the cloud spans ~60 cells at 0.5 m
    to_world = lambda p: p * scale                                # noqa: E731
    bounds = D.dsm_grid_from_cloud(to_world(xyz))
    n = min(bounds.xsize, bounds.ysize) - 4
    meta = [bounds.xoff + 2 * 0.5, bounds.yoff - 2 * 0.5 - n * 0.5, n, 0.5]
    gt = D.create_dsm(to_world(xyz), roi=meta) + 0.25
    gt = torch.where(torch.isnan(gt), torch.zeros_like(gt), gt)
    pipe.logged.clear()
    out = pipe.validation_step(dict(batch, dsm={"gt": gt, "roi": meta, "to_world": to_world}), 1)
    want = D.compute_dsm_and_mae(batch["rays"], out["results"]["depth_coarse"], gt, meta, to_world=to_world)
    assert sorted(pipe.logged) == sorted(plain_logged + ["test/mae"])
    assert pipe.logged["test/mae"] == want["mean"] and np.isfinite(want["mean"])
    assert sorted(out) == sorted(list(plain) + ["mae"])
    assert torch.equal(out["mae"]["dsm"].view(torch.int32), want["dsm"].view(torch.int32))
    pipe.logged.clear()
    late = pipe.validation_step(dict(batch, dsm={"gt": gt, "roi": meta, "to_world": to_world}), 2)
    assert sorted(late) == sorted(plain) and sorted(pipe.logged) == plain_logged
