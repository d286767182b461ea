"""DSM evaluation, CPU side: the numpy restatement of the registration + MAE (tests/dsm_numpy.py) reproduces the reference's
own output (tests/golden/dsmr_*.npz, written by tools/gen_golden_dsm.py from eval/utils/dsmr.py), the grid arithmetic, the
argument checks of the new C-ABI entries (no GPU work), and the hazard scan of csrc/dsm.hip's generated code."""
import ctypes as C
import glob
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dsm_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "dsmr_*.npz")))
CSRC = os.path.join(ROOT, "semantic-nerf-for-satellite-data_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_golden_cases_present():
    names = {os.path.basename(p)[:-4] for p in GOLDEN}
    assert names == {"dsmr_64", "dsmr_130x150", "dsmr_odd", "dsmr_shift", "dsmr_holes_water", "dsmr_gt_low", "dsmr_flat"}


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_numpy_restatement_reproduces_reference(path):
    z = np.load(path)
    u, v = z["gt"].astype(np.float64), z["v"].astype(np.float64)
    for k in range(1, int(z["n_levels"]) + 1):          # every pyramid level, bit for bit
        u, v = N.downsample2x(u), N.downsample2x(v)
        np.testing.assert_array_equal(u, z[f"ds_u_{k}"])
        np.testing.assert_array_equal(v, z[f"ds_v_{k}"])
    mask = z["mask"] if "mask" in z.files else None
    r = N.compute_mae(z["pred"], z["gt"], mask=mask, init=tuple(int(x) for x in z["init"]))
    assert [list(t) for t in r["trace"]] == z["shifts"].tolist()     # the shift found at every level, exactly
    assert (r["dx"], r["dy"]) == (int(z["dx"]), int(z["dy"]))
    for k in ("muu", "muv", "b"):
        assert _rel(r[k], float(z[k])) <= 1e-12, k
    np.testing.assert_array_equal(np.isnan(r["rdsm"]), np.isnan(z["rdsm"]))
    np.testing.assert_array_equal(r["rdsm"], z["rdsm"])
    np.testing.assert_array_equal(r["diff"], z["diff"])
    # the reference's nanmean / nanmedian run in float32 (numpy on the float32 difference); ours in float64
    assert _rel(r["mean"], float(z["mean"])) <= 1e-6
    assert _rel(r["median"], float(z["median"])) <= 1e-6


def test_downsample_off_by_one():
    """the reference's loop writes every output cell up to four times; the last write (odd row and column) wins"""
    u = np.arange(20, dtype=np.float64).reshape(4, 5)
    d = N.downsample2x(u)
    assert d.shape == (2, 3)
    assert d[0, 0] == 9.0                                   # mean of u[1:3, 1:3], not of u[0:2, 0:2] (= 3.0)
    assert d[0, 2] == (9 + 14) / 2                          # last column: i = min(5, 4) = 4, one column in range
    assert d[1, 2] == 19.0                                  # corner: only u[3, 4]


def test_grid_arithmetic():
    from snerf_amd.eval.utils import dsm
    cloud = np.array([[10.2, 20.7, 0.0], [11.9, 19.1, 0.0], [10.26, 20.2, 0.0]])
    g = N.bounds_grid(cloud)
    # xoff = floor(10.2/0.5)*0.5 = 10.0; xsize = 1 + floor((11.9-10)/0.5) = 4; yoff = ceil(20.7/0.5)*0.5 = 21.0;
    # ysize = 1 - floor((19.1-21)/0.5) = 1 - (-4) = 5
    assert g == (10.0, 21.0, 0.5, 4, 5)
    cloud = np.array([[-3.0, -1.0, 0.0], [-1.0, 1.0, 0.0]])   # corners on the lattice
    assert N.bounds_grid(cloud) == (-3.0, 1.0, 0.5, 5, 5)
    r = dsm.roi_grid([500.0, 1000.0, 4, 0.5])
    assert r == dsm.DsmGrid(500.0, 1002.0, 0.5, 4, 4)        # yoff += size * resolution; square
    r = dsm.roi_grid(np.array([500.0, 1000.0, 7.9, 0.5]))
    assert (r.xsize, r.ysize, r.yoff) == (7, 7, 1003.5)      # int(meta[2]); yoff moved by int(size) * res


def test_numpy_rasterize_by_hand():
    # radius 1: a point adds to its 3 x 3 window, also when its own cell is outside the grid
    cloud = np.array([[0.25, 1.75, 10.0], [0.75, 1.75, 20.0], [-0.25, 0.75, 6.0]])
    mean, count = N.rasterize(cloud, 0.0, 2.0, 0.5, 3, 4, radius=1)
    assert count.tolist() == [[2, 2, 1], [3, 2, 1], [1, 0, 0], [1, 0, 0]]   # the third point: cell (-1, 2), window column 0
    assert mean[0, 0] == 15.0 and mean[1, 0] == 12.0 and mean[0, 2] == 20.0 and mean[3, 0] == 6.0 and np.isnan(mean[3, 1])


def test_median_rule():
    a = np.array([1.0, 4.0, np.nan, 2.0, 3.0], np.float32)
    assert np.nanmedian(a) == 2.5                            # numpy: the mean of the two middle values


# ---- C-ABI argument checks (host only: no GPU work is reached) ----------------------------------------------------------------
def test_dsm_abi_rejects_bad_arguments():
    from snerf_amd import _lib
    L = _lib.lib()
    P = C.c_void_p(16)                                       # never dereferenced: every call below fails its checks first
    g = _lib.SnerfDsmGrid(0.0, 0.0, 0.5, 8, 8, 0, 0, 8, 8)
    assert L.snerf_dsm_accumulate(None, 4, C.byref(g), 1, 0.0, 1.0, P, P, P, None) == 3
    assert L.snerf_dsm_accumulate(P, 4, None, 1, 0.0, 1.0, P, P, P, None) == 3
    assert L.snerf_dsm_accumulate(P, 4, C.byref(g), 1, 0.0, 1.0, None, P, P, None) == 3
    assert b"null" in L.snerf_last_error()
    assert L.snerf_dsm_accumulate(P, -1, C.byref(g), 1, 0.0, 1.0, P, P, P, None) == 1
    assert L.snerf_dsm_accumulate(P, 4, C.byref(g), -1, 0.0, 1.0, P, P, P, None) == 1
    assert b"radius" in L.snerf_last_error()
    assert L.snerf_dsm_accumulate(P, 4, C.byref(g), 1, 0.0, 0.0, P, P, P, None) == 1
    for bad in (_lib.SnerfDsmGrid(0.0, 0.0, 0.0, 8, 8, 0, 0, 8, 8), _lib.SnerfDsmGrid(0.0, 0.0, 0.5, 0, 8, 0, 0, 8, 8),
                _lib.SnerfDsmGrid(0.0, 0.0, 0.5, 8, 8, 0, 0, 8, -2)):
        assert L.snerf_dsm_accumulate(P, 4, C.byref(bad), 1, 0.0, 1.0, P, P, P, None) == 1
    assert L.snerf_dsm_finish(P, P, 64, 0.0, 1.0, None, P, None) == 3
    assert L.snerf_dsm_finish(P, P, 0, 0.0, 1.0, P, P, None) == 1
    assert L.snerf_dsm_downsample2x(None, 0, 4, 4, P, None) == 3
    assert L.snerf_dsm_downsample2x(P, 0, 0, 4, P, None) == 1
    assert L.snerf_dsm_downsample2x(P, 1, 4, -4, P, None) == 1
    assert L.snerf_dsm_workspace_bytes(0, 4, 5) == 0
    assert L.snerf_dsm_workspace_bytes(4, 4, -1) == 0
    assert L.snerf_dsm_workspace_bytes(4, 4, 8) == 0
    n = L.snerf_dsm_workspace_bytes(1024, 1024, 5)
    assert n >= 32 * 32 * 3 * 121 * 8
    assert L.snerf_dsm_ncc_search(P, None, 0, 8, 8, 0, 0, 5, P, P, n, None) == 3
    assert L.snerf_dsm_ncc_search(P, P, 0, 8, 0, 0, 0, 5, P, P, n, None) == 1
    assert L.snerf_dsm_ncc_search(P, P, 0, 8, 8, 0, 0, -1, P, P, n, None) == 1
    assert L.snerf_dsm_ncc_search(P, P, 0, 8, 8, 0, 0, 5, P, P, 8, None) == 2
    assert L.snerf_dsm_shift_diff(None, P, 8, 8, 0, 0, 0.0, P, P, P, P, n, None) == 3
    assert L.snerf_dsm_shift_diff(P, P, -8, 8, 0, 0, 0.0, P, P, P, P, n, None) == 1
    assert L.snerf_dsm_shift_diff(P, P, 8, 8, 0, 0, 0.0, P, P, P, P, 8, None) == 2


def test_ncc_search_abi_limits():
    from snerf_amd import _lib
    L = _lib.lib()
    P = C.c_void_p(16)                                       # never dereferenced: every call below fails its checks
    lim = 1 << 20
    need = L.snerf_dsm_workspace_bytes(65, 33, 5)
    assert need == 6 * 3 * 121 * 8 and L.snerf_dsm_workspace_bytes(40, 8200, 2) == 514 * 3 * 25 * 8 and L.snerf_dsm_workspace_bytes(1, 1, 0) == 2 * 1024 * 8
    # a centre of +-2^20 passes the argument checks: the refusal is the next check's, the workspace one byte short
    for cx, cy in ((lim, 0), (-lim, 0), (0, lim), (0, -lim), (lim, -lim)):
        assert L.snerf_dsm_ncc_search(P, P, 0, 65, 33, cx, cy, 5, P, P, need - 1, None) == 2
        assert b"workspace" in L.snerf_last_error()
    for cx, cy in ((lim + 1, 0), (-lim - 1, 0), (0, lim + 1), (0, -lim - 1)):
        assert L.snerf_dsm_ncc_search(P, P, 0, 65, 33, cx, cy, 5, P, P, need, None) == 1
        assert b"centre" in L.snerf_last_error()
    assert L.snerf_dsm_ncc_search(P, P, 0, 65, 33, 0, 0, 8, P, P, 1 << 30, None) == 1
    assert b"radius" in L.snerf_last_error()
    for h, w, r in ((65, 33, 5), (40, 8200, 2), (1, 1, 0)):
        n = L.snerf_dsm_workspace_bytes(h, w, r)
        assert L.snerf_dsm_ncc_search(P, P, 1, h, w, 0, 0, r, P, P, n - 1, None) == 2


def test_no_vgpr_hazards_in_dsm_kernels(tmp_path):
    """tools/check_vgpr_hazards.py over csrc/dsm.hip compiled as the product build compiles it"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path / "dsm.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed",
                    "-Wno-unused-command-line-argument", "-I" + CSRC, "--cuda-device-only", "-S",
                    os.path.join(CSRC, "dsm.hip"), "-o", str(out)], check=True, timeout=900)
    lines = out.read_text().splitlines()
    assert any("ncc_tile_kernel" in ln for ln in lines)
    spec = importlib.util.spec_from_file_location("check_vgpr_hazards", os.path.join(ROOT, "tools", "check_vgpr_hazards.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert not chk.scan_store(lines)
    assert not chk.scan_lds(lines)
    assert not chk.scan_trans(lines)
