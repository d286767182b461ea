"""World -> scene on the GPU (csrc/geo.hip with SnerfGeoParams.direction = 1, GeoFrame.to_scene, conversions, and the nadir rays
of baseline/components/rays.py) against the numpy restatements of tests/utm_inverse_numpy.py.  DESIGN.md section 5l.

Bars, those of tests/test_gpu_geo.py and by its reasoning: lat / lon within 1e-12 deg of the restated to_latlon and xyz_n * range
within 1e-6 m of the numpy chain (to_latlon -> latlon_to_ecef_custom restated -> normalise): the coordinates are about 6.4e6 m,
where one fp64 ulp is 9e-10 m, and the chain is a few dozen operations whose sin / cos may differ from numpy's in the last place.
Wherever a point goes into the scene AND back, the two series do not close exactly (tests/test_geo_inverse_cpu.py: 4e-5 m near
the fixture): that residual is computed in the test by the restatements alone, never by the code under test, and 2e-6 m is added
for the two kernel legs at 1e-6 m each.  The `utm` package is not installed: parity with it is UNPINNED."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import utm_inverse_numpy as V
from tests import utm_numpy as U
from tests.test_gpu_geo import DEV, U64, _bits, _norm, _ptr, _torch_bounds, dev, frame, fx  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INIT = [-1, 0, -1, 0, 0, 0, 0, 0]
BIG = 4096 * 256 + 1                  # the only size at which the grid-stride loop runs twice (GEO_MAX_GRID x GEO_THREADS + 1)
ERR_BAD_DESC = 1                      # include/snerf_hip.h SNERF_ERR_BAD_DESC
PAD = 64                              # rows behind the n a launch may write


def _params(frame, direction):
    from snerf_amd import _lib
    p = _lib.SnerfGeoParams.from_buffer_copy(frame.params)
    p.direction = direction
    return p


def _centre_range(frame):
    return np.array(list(frame.params.centre)), float(frame.params.range)


def _run(params, n, enu, want_lla=True, fill=-7.0):
    """one raw snerf_geo_points launch -> (out (n + PAD, 3), lla or None, stats words as unsigned ints, return code); the
    output buffers are PAD rows longer than n and pre-filled with `fill`"""
    from snerf_amd import _lib
    L = _lib.lib()
    out = torch.full((n + PAD, 3), fill, dtype=torch.float64, device=DEV)
    lla = torch.full((n + PAD, 3), fill, dtype=torch.float64, device=DEV) if want_lla else None
    stats = torch.tensor(INIT, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = L.snerf_geo_points(_ptr(enu), n, C.byref(params), _ptr(out), _ptr(lla), _ptr(stats), st)
    torch.cuda.synchronize()
    return out, lla, [int(w) & U64 for w in stats.cpu().tolist()], rc


@pytest.fixture(scope="module")
def world(fx):
    """the fixture's points in the world: (east_restated, north_restated, alt), host and device"""
    enu = np.ascontiguousarray(np.stack([fx["east_restated"], fx["north_restated"], fx["alt"]], 1))
    return {"np": enu, "dev": torch.from_numpy(enu).to(DEV)}


@pytest.fixture(scope="module")
def full(frame, world):
    """the whole fixture through direction 1, once; the tests below only read it"""
    n = world["dev"].shape[0]
    out, lla, stats, rc = _run(_params(frame, 1), n, world["dev"], fill=123.0)
    assert rc == 0
    return {"xyz": out[:n], "lla": lla[:n], "stats": stats}


def _synthetic(south):
    """2,048 points of one hemisphere in zone 17, up to 3 degrees from the meridian (both edges included), -500 .. 9000 m"""
    rng = np.random.default_rng(7 + south)
    n = 2048
    lat = rng.uniform(-60.0, 0.0, n) if south else rng.uniform(0.0, 70.0, n)
    dl = rng.uniform(-3.0, 3.0, n)
    dl[:4] = [-3.0, 3.0, -3.0, 3.0]
    lat[:4] = [-60.0, -60.0, -0.5, -0.5] if south else [70.0, 70.0, 0.5, 0.5]
    east, north = U.from_latlon(lat, -81.0 + dl, 17, south=bool(south))
    return np.ascontiguousarray(np.stack([east, north, rng.uniform(-500.0, 9000.0, n)], 1))


def _assert_parity(name, frame, enu, south, out, lla):
    centre, rng = _centre_range(frame)
    want, lat, lon = V.to_scene(enu, centre, rng, 17, south)
    out, lla = out.cpu().numpy(), lla.cpu().numpy()
    d = {"lat": float(np.abs(lla[:, 0] - lat).max()), "lon": float(np.abs(lla[:, 1] - lon).max()),
         "xyz": float(np.abs(out - want).max() * rng)}
    print(f"inverse parity maxima, {name}:", d)
    assert d["lat"] <= 1e-12 and d["lon"] <= 1e-12 and d["xyz"] <= 1e-6
    assert np.array_equal(lla[:, 2], enu[:, 2])                       # the altitude passes through


def test_kernel_against_the_restated_chain(fx, frame, world, full):
    _assert_parity("fixture", frame, world["np"], False, full["xyz"], full["lla"])
    assert full["stats"][4:] == [0, 0, 0, 0]
    from snerf_amd.framework.components.coordinate_systems import GeoFrame
    for south, zone_string in ((0, "17R"), (1, "17M")):
        f = GeoFrame(_norm(fx), zone_string)
        assert f.params.south == south
        enu = _synthetic(south)
        out, lla, stats, rc = _run(_params(f, 1), enu.shape[0], torch.from_numpy(enu).to(DEV))
        assert rc == 0 and stats[4] == 0
        _assert_parity(zone_string, f, enu, bool(south), out[:enu.shape[0]], lla[:enu.shape[0]])


def test_fixture_points_come_back_to_their_scene_coordinates(fx, frame, world, full):
    """the fixture's own xyz_n from its (east_restated, north_restated, alt): within the numpy residual of those points + 2e-6 m"""
    centre, rng = _centre_range(frame)
    residual = float(np.abs(V.to_scene(world["np"], centre, rng, 17)[0] - fx["xyz_n"]).max() * rng)
    d = float(np.abs(full["xyz"].cpu().numpy() - fx["xyz_n"]).max() * rng)
    print(f"fixture xyz_n recovered to {d:.3e} m (numpy residual {residual:.3e} m)")
    assert residual <= 1e-4                       # the series' round trip near the fixture (tests/test_geo_inverse_cpu.py)
    assert d <= residual + 2e-6


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_tails_prefixes_and_determinism(n, frame, world, full):
    from snerf_amd.framework.components.coordinate_systems import GeoBounds, decode_geo_stats
    p = _params(frame, 1)
    enu = world["dev"][:n].contiguous()
    out, lla, stats, rc = _run(p, n, enu)
    assert rc == 0
    assert torch.equal(_bits(out[:n]), _bits(full["xyz"][:n])) and torch.equal(_bits(lla[:n]), _bits(full["lla"][:n]))
    assert bool((out[n:] == -7.0).all()) and bool((lla[n:] == -7.0).all())               # nothing is written behind n
    out2, lla2, stats2, _ = _run(p, n, enu)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(lla), _bits(lla2)) and stats == stats2
    out3, none, stats3, rc = _run(p, n, enu, want_lla=False)
    assert rc == 0 and none is None and torch.equal(_bits(out3), _bits(out)) and stats3 == stats
    bounds, bad = decode_geo_stats(stats)
    assert bad == 0
    if n == 0:
        assert stats == [U64, 0, U64, 0, 0, 0, 0, 0]                                     # nothing was launched
        assert bounds == GeoBounds(np.inf, -np.inf, np.inf, -np.inf)
    else:
        assert bounds == _torch_bounds(out[:n])
        xyz, b = frame.to_scene(enu)
        assert torch.equal(_bits(xyz), _bits(out[:n])) and b == bounds
        xyz, lla4, b = frame.to_scene(enu.float(), want_lla=True)                        # fp32 points are widened, not refused
        assert tuple(xyz.shape) == tuple(lla4.shape) == (n, 3)


def test_the_grid_stride_loop_runs_twice(frame, world, full):
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    m = world["dev"].shape[0]
    reps = -(-BIG // m)
    enu = world["dev"].repeat(reps, 1)[:BIG].contiguous()
    p = _params(frame, 1)
    out, lla, stats, rc = _run(p, BIG, enu)
    assert rc == 0
    assert torch.equal(_bits(out[:BIG]), _bits(full["xyz"].repeat(reps, 1)[:BIG]))
    assert torch.equal(_bits(lla[:BIG]), _bits(full["lla"].repeat(reps, 1)[:BIG]))
    assert bool((out[BIG:] == -7.0).all()) and bool((lla[BIG:] == -7.0).all())
    assert decode_geo_stats(stats) == decode_geo_stats(full["stats"])
    out2, lla2, stats2, _ = _run(p, BIG, enu)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(lla), _bits(lla2)) and stats == stats2


def test_device_round_trip(frame, world):
    """frame.points(frame.to_scene(P)) = P within the numpy residual of the same points + 2e-6 m"""
    centre, rng = _centre_range(frame)
    residual = V.round_trip_residual(world["np"], centre, rng, 17)
    xyz, _ = frame.to_scene(world["dev"])
    back, _ = frame.points(xyz)
    d = float((back - world["dev"]).abs().max())
    print(f"device round trip {d:.3e} m (numpy residual {residual:.3e} m)")
    assert residual <= 1e-4 and d <= residual + 2e-6
    assert frame.params.direction == 0                                 # the frame keeps its forward params


def test_conversions_on_device_tensors(fx, frame, world, full):
    import types
    from snerf_amd.framework.util import conversions as Cv
    e, n = world["dev"][:, 0], world["dev"][:, 1]
    lats, lons = Cv.latlon_from_utm(e, n, "17R")
    assert lats.dtype == torch.float64 and torch.equal(_bits(lats), _bits(full["lla"][:, 0]))
    assert torch.equal(_bits(lons), _bits(full["lla"][:, 1]))
    lo2, la2 = Cv.lonlat_from_utm(e.reshape(-1, 1), n.reshape(-1, 1), "17R")
    assert tuple(la2.shape) == (e.shape[0], 1) and torch.equal(_bits(la2.reshape(-1)), _bits(lats))
    assert torch.equal(_bits(lo2.reshape(-1)), _bits(lons))
    ds = types.SimpleNamespace(geo=frame)
    xyz = Cv.convert_utm_to_local(ds, world["dev"])
    assert torch.equal(_bits(xyz), _bits(full["xyz"]))
    assert torch.equal(_bits(Cv.convert_local_to_utm(ds, xyz)), _bits(frame.points(xyz)[0]))


def test_refusals_launch_nothing(frame, dev, world):
    from snerf_amd import _lib
    L = _lib.lib()
    enu = world["dev"][:8].contiguous()
    rays, depth = dev["rays"][:8].contiguous(), dev["depth"][:8].contiguous()
    out = torch.zeros((8, 3), dtype=torch.float64, device=DEV)
    stats = torch.tensor(INIT, dtype=torch.int64, device=DEV)
    for direction in (2, -1):
        p = _params(frame, direction)
        assert L.snerf_geo_points(_ptr(enu), 8, C.byref(p), _ptr(out), None, _ptr(stats), None) == ERR_BAD_DESC
        assert b"direction" in L.snerf_last_error()
        assert L.snerf_geo_cloud(_ptr(rays), 8, _ptr(depth), 8, C.byref(p), _ptr(out), None, _ptr(stats), None) == ERR_BAD_DESC
        assert L.snerf_geo_points(_ptr(enu), 0, C.byref(p), _ptr(out), None, _ptr(stats), None) == ERR_BAD_DESC    # also for n = 0
    p = _params(frame, 1)
    assert L.snerf_geo_cloud(_ptr(rays), 8, _ptr(depth), 8, C.byref(p), _ptr(out), None, _ptr(stats), None) == ERR_BAD_DESC
    assert b"direction" in L.snerf_last_error()
    assert L.snerf_geo_points(None, 8, C.byref(p), _ptr(out), None, _ptr(stats), None) != 0
    assert L.snerf_geo_points(_ptr(enu), 8, None, _ptr(out), None, _ptr(stats), None) != 0
    assert L.snerf_geo_points(_ptr(enu), 8, C.byref(p), None, None, _ptr(stats), None) != 0
    assert L.snerf_geo_points(_ptr(enu), 8, C.byref(p), _ptr(out), None, None, None) != 0
    assert L.snerf_geo_points(_ptr(enu), -1, C.byref(p), _ptr(out), None, _ptr(stats), None) != 0
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == INIT and not bool(out.any())        # nothing ran
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        frame.to_scene(world["dev"][:, :2])
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        frame.to_scene(world["dev"].reshape(-1))


def test_direction_zero_is_untouched(frame, dev):
    """snerf_geo_points with direction = 0 on the whole fixture: the bits GeoFrame.cloud (snerf_geo_cloud) gives"""
    from snerf_amd.eval.extract_pointcloud import get_xyz_from_nerf_prediction
    cloud, lla, bounds = frame.cloud(dev["rays"], dev["depth"], want_lla=True)
    n = cloud.shape[0]
    xyz_n = get_xyz_from_nerf_prediction(dev["rays"], dev["depth"]).contiguous()
    out, lla0, stats, rc = _run(_params(frame, 0), n, xyz_n)
    assert rc == 0 and torch.equal(_bits(out[:n]), _bits(cloud)) and torch.equal(_bits(lla0[:n]), _bits(lla))
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    assert decode_geo_stats(stats) == (bounds, 0)


def test_stats_are_the_scene_bounds_and_count_what_is_not_finite(frame, world, full):
    from snerf_amd.framework.components.coordinate_systems import decode_geo_stats
    assert decode_geo_stats(full["stats"]) == (_torch_bounds(full["xyz"]), 0)
    n = 257
    enu = world["dev"][:n].clone()
    enu[128, 1] = float("nan")
    out, lla, stats, rc = _run(_params(frame, 1), n, enu)
    assert rc == 0
    bounds, bad = decode_geo_stats(stats)
    assert bad == 1 and bool(torch.isnan(out[128]).all())
    keep = torch.arange(n, device=DEV) != 128
    assert torch.equal(_bits(out[:n][keep]), _bits(full["xyz"][:n][keep]))
    assert bounds == _torch_bounds(out[:n])
    with pytest.raises(ValueError, match="1 of 257"):
        frame.to_scene(enu)
    enu[5, 2] = float("inf")
    assert decode_geo_stats(_run(_params(frame, 1), n, enu)[2])[1] == 2


# ---- nadir rays ------------------------------------------------------------------------------------------------------------------
MIN_ALT, MAX_ALT = -20.0, 60.0
XOFF, YOFF, RES = 432664.5, 3352265.5, 0.5             # the north-west corner of the fixture scene's ROI


def nadir_tolerance(rays, frame, grid_points):
    """metres: each origin component is rounded once to fp32 (2^-24 of max(1, |o|), times range), the direction's rounding is
    multiplied by the depth <= far, and the factor 4 covers the three components' norm and the 2^-24 of the far column; plus the
    numpy round-trip residual of the lattice's own points and 2e-6 m for the two kernel legs"""
    centre, rng = _centre_range(frame)
    residual = V.round_trip_residual(grid_points, centre, rng, 17)
    o = float(rays[:, :3].abs().max())
    far = float(rays[:, 7].max())
    return 4.0 * 2.0 ** -24 * rng * max(1.0, o) * (1.0 + far) + residual + 2e-6, residual


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (33, 17)])
def test_nadir_rays_stand_on_their_cells(h, w, frame):
    from snerf_amd.baseline.components import rays as R
    from snerf_amd.eval.utils import dsm as D
    from snerf_amd.eval.utils import ortho as OR
    grid = D.DsmGrid(XOFF, YOFF, RES, w, h)
    rays, bounds = R.nadir_construct(grid, frame, MIN_ALT, MAX_ALT, want_bounds=True)
    assert rays.dtype == torch.float32 and rays.is_contiguous() and tuple(rays.shape) == (h * w, 8) and rays.is_cuda
    assert bool((rays[:, 6] == 0).all()) and bool((rays[:, 7] > 0).all())
    norm = rays[:, 3:6].double().norm(dim=1)
    assert float((norm - 1.0).abs().max()) <= 2.0 ** -23
    assert torch.equal(R.nadir_construct(grid, frame, MIN_ALT, MAX_ALT), rays)
    assert bounds.xmin <= float(rays[:, 0].min()) + 1e-6 and bounds.xmax >= float(rays[:, 0].max()) - 1e-6
    # the cell centres, on the host: row 0 is the north edge, row-major
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    east, north = (XOFF + (ii + 0.5) * RES).reshape(-1), (YOFF - (jj + 0.5) * RES).reshape(-1)
    pts = np.concatenate([np.stack([east, north, np.full(h * w, a)], 1) for a in (MAX_ALT, MIN_ALT)])
    tol, residual = nadir_tolerance(rays, frame, pts)
    worst = 0.0
    for depth, alt in ((torch.zeros_like(rays[:, 7]), MAX_ALT), (rays[:, 7].contiguous(), MIN_ALT)):
        cloud = frame.cloud(rays, depth)[0].cpu().numpy()
        worst = max(worst, float(np.abs(cloud[:, 0] - east).max()), float(np.abs(cloud[:, 1] - north).max()),
                    float(np.abs(cloud[:, 2] - alt).max()))
    print(f"nadir {h} x {w}: worst {worst:.3e} m, tol {tol:.3e} m (numpy residual {residual:.3e} m)")
    assert worst <= tol
    assert tol < 1e-2 * RES                             # the bar itself is far inside a cell
    # the cell convention against the lattice splat: the cloud at half depth fills every cell exactly once, in row-major order
    mid = frame.cloud(rays, (rays[:, 7] * 0.5).contiguous())[0]
    top, stats = OR.top_surface(mid, grid, radius=0)
    got = OR.gather(top, 0, h * w)
    assert torch.equal(got["index"], torch.arange(h * w, device=DEV).reshape(h, w))
    assert int(stats[1]) == h * w and int(stats[0]) == 0
    # a window of a larger lattice gives the rays of its cells
    if h > 1:
        win = D.grid_struct(grid, (1, 1, w - 1, h - 1))
        sub = R.nadir_construct(win, frame, MIN_ALT, MAX_ALT)
        assert torch.equal(sub, rays.reshape(h, w, 8)[1:, 1:].reshape(-1, 8))
