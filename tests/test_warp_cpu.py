"""CPU-side checks of the raster warp (include/snerf_warp.h, csrc/warp.hip, eval/utils/warp.py): the new
header's prototypes, struct and constants against the binding (_lib.ADDED_HEADER_SIGNATURES), the restatement (tests/warp_numpy.py, the
oracle of tests/test_gpu_warp.py) against closed forms, scipy.ndimage and brute-force counts, the host layer's lattices and snapping,
what stays as it was without the new arguments, and every refusal of the two entries through the binding (none reaches a launch)."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from snerf_amd import _lib
from snerf_amd.eval.utils import dsm as D
from snerf_amd.eval.utils import warp as W          # the feature under test: every test of this file needs it
from tests import warp_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snerf_warp.h")
DUMMY = 4096        # a non-null address no refusal path dereferences
NAMES = {
    "snerf_warp_planes": ["src", "planes", "map", "method", "min_valid", "dst", "stats", "stream"],
    "snerf_warp_labels": ["src", "map", "method", "dst", "stats", "stream"],
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- header and binding -------------------------------------------------------------------------------------------------------------------
def test_the_new_header_matches_its_binding_rows():
    """include/snerf_warp.h against _lib.ADDED_HEADER_SIGNATURES["snerf_warp.h"], as tests/abi_header.py holds the older headers to the
    frozen table: names, order, return type, per parameter class, width and signedness, the stream marker; lib() and call() serve the
    rows; the frozen tables are what they were; the main header names nothing of this one"""
    from tests.abi_header import FROZEN
    from tests.test_abi_cpu import _c_type, _table_type
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    src = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", src, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(snerf_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        protos[name] = (_c_type(ret), [(_c_type(t), n) for t, n in (re.fullmatch(r"\s*(.*?)(\w+)\s*", p).groups() for p in params.split(","))])
    assert list(_lib.ADDED_HEADER_SIGNATURES) == ["snerf_warp.h"]
    rows = _lib.ADDED_HEADER_SIGNATURES["snerf_warp.h"]
    assert list(rows) == list(protos) == list(NAMES)
    for symbol, (ret, params) in protos.items():
        restype, argtypes = rows[symbol]
        assert _table_type(restype) == ret == ("int", 4, True), (symbol, restype, ret)
        assert len(argtypes) == len(params) and [n for _, n in params] == NAMES[symbol], (symbol, params)
        for k, (t, (want, pname)) in enumerate(zip(argtypes, params)):
            got = _table_type(t)
            assert got == want or (want[0] == "pointer" and got == ("pointer", None)), (symbol, k, pname, t, want)
            assert (t is _lib.c_stream) == (pname == "stream"), (symbol, k, pname)
        fn = getattr(_lib.lib(), symbol)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes) and symbol in _lib._PLANS
        assert symbol not in _lib.SIGNATURES and symbol not in _lib.EXPORTED_SYMBOLS
        assert all(symbol not in other for other in _lib.HEADER_SIGNATURES.values())
    assert rows["snerf_warp_planes"][1][2] is C.POINTER(_lib.SnerfWarpMap) and rows["snerf_warp_labels"][1][1] is C.POINTER(_lib.SnerfWarpMap)
    assert {h: list(r) for h, r in _lib.HEADER_SIGNATURES.items()} == FROZEN and list(_lib.HEADER_SIGNATURES) == list(FROZEN)
    assert len(_lib.EXPORTED_SYMBOLS) == 53 and _lib.lib().snerf_version() == _lib.ABI_VERSION == 6
    main = open(os.path.join(ROOT, "include", "snerf_hip.h")).read()
    own = ["snerf_warp"] + list(protos) + re.findall(r"\} (\w+);", text) + re.findall(r"^#define (SNERF_[A-Z0-9]+_)", text, flags=re.M)
    assert "SnerfWarpMap" in own and "SNERF_WARP_" in own and not [word for word in own if word in main]
    assert '#include "snerf_hip.h"' in text


def test_the_struct_and_the_constants():
    text = open(HEADER).read()
    body = re.search(r"typedef struct SnerfWarpMap \{(.*?)\} SnerfWarpMap;", text, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(double|int) ([^;]+);", body) for n in names.split(",")]
    assert fields == [("double", n) for n in ("off_x", "step_x", "off_y", "step_y")] + [("int", n) for n in ("src_w", "src_h", "dst_w", "dst_h")]
    assert [n for n, _ in _lib.SnerfWarpMap._fields_] == [n for _, n in fields] == list(N.Map._fields)
    assert C.sizeof(_lib.SnerfWarpMap) == 48
    assert [getattr(_lib.SnerfWarpMap, n).offset for _, n in fields] == [0, 8, 16, 24, 32, 36, 40, 44]
    consts = {k: int(v) for k, v in re.findall(r"#define (SNERF_WARP_\w+) (\d+)", text)}
    methods = [consts["SNERF_WARP_" + n] for n in ("NEAREST", "BILINEAR", "AVERAGE", "MIN", "MAX", "MODE")]
    assert methods == [0, 1, 2, 3, 4, 5]
    assert methods == [_lib.WARP_NEAREST, _lib.WARP_BILINEAR, _lib.WARP_AVERAGE, _lib.WARP_MIN, _lib.WARP_MAX, _lib.WARP_MODE]
    assert methods == [W.NEAREST, W.BILINEAR, W.AVERAGE, W.MIN, W.MAX, W.MODE] == [N.NEAREST, N.BILINEAR, N.AVERAGE, N.MIN, N.MAX, N.MODE]
    assert methods == [W.METHODS[n] for n in ("nearest", "bilinear", "average", "min", "max", "mode")]
    assert consts["SNERF_WARP_MAX_STEP"] == _lib.WARP_MAX_STEP == W.MAX_STEP == N.MAX_STEP == 64
    assert consts["SNERF_WARP_MAX_PLANES"] == _lib.WARP_MAX_PLANES == W.MAX_PLANES == N.MAX_PLANES == 16
    assert W.NO_LABEL == N.NO_LABEL == _lib.ORTHO_NO_LABEL == 255 and len(consts) == 8


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
MAPS = [N.Map(-1.3, 34 / 13, 0.4, 2.0, 65, 7, 9, 5), N.Map(0.25, 0.37, -0.75, 0.5, 9, 7, 30, 17), N.Map(3.0, 1.0, -2.0, 1.0, 9, 7, 8, 9),
        N.Map(0.5, 1.0, 0.0, 3.0, 9, 7, 9, 3), N.Map(20.0, 2.0, 0.0, 2.0, 9, 7, 3, 2)]


@pytest.mark.parametrize("m", MAPS, ids=[str(k) for k in range(len(MAPS))])
def test_the_two_restatements_agree_bit_for_bit(m):
    """every cell at once (the oracle of the GPU tests) against one cell at a time (the header's text in Python floats)"""
    src = N.float_raster(m.src_h, m.src_w, "random", planes=2, seed=3, infs=True)
    for method in N.FLOAT_METHODS:
        for min_valid in (0.25, 1.0):
            a, sa = N.warp_planes(src, m, method, min_valid)
            b, sb = N.planes_by_cells(src, m, method, min_valid)
            assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b)) and sa == sb, (method, min_valid)
            assert sum(sa[:2]) == a.size
    lab = N.label_raster(m.src_h, m.src_w, seed=3)
    for method in N.LABEL_METHODS:
        a, sa = N.warp_labels(lab, m, method)
        b, sb = N.labels_by_cells(lab, m, method)
        assert a.dtype == np.uint8 and np.array_equal(a, b) and sa == sb, method


def test_an_integer_shift_returns_the_bits_of_the_slice():
    """step 1 and whole offsets: every method reads exactly one cell of weight 1, -0 and a hole included; beyond the source NaN / 255"""
    src = N.float_raster(7, 9, "random", planes=2, seed=1)
    src[0, 2, 3], src[1, 4, 4] = -0.0, np.float32(1e-45)
    m = N.Map(3.0, 1.0, -2.0, 1.0, 9, 7, 8, 9)
    want = np.full((2, 9, 8), N.NAN32, np.float32)
    want[:, 2:9, 0:6] = src[:, 0:7, 3:9]
    for method in N.FLOAT_METHODS:
        for min_valid in (0.25, 1.0):
            got, stats = N.warp_planes(src, m, method, min_valid)
            assert np.array_equal(bits(got), bits(want)), method
            assert stats == [int(np.isfinite(want).sum()), int(np.isnan(want).sum()), 9 * 8 - 7 * 6]
    lab = N.label_raster(7, 9, seed=1)
    want = np.full((9, 8), 255, np.uint8)
    want[2:9, 0:6] = lab[0:7, 3:9]
    for method in N.LABEL_METHODS:
        got, stats = N.warp_labels(lab, m, method)
        assert np.array_equal(got, want) and stats == [int((want != 255).sum()), int((want == 255).sum()), 9 * 8 - 7 * 6]


def test_integer_steps_average_to_the_block_mean():
    """steps 2 x 3 on |v| <= 100: every destination cell is the mean of its 3 x 2 block, to 1e-12 (measured 0 to the printed digits; an indexing
    error is O(1))"""
    src = N.float_raster(21, 34, "none", seed=2)[0]
    m = N.Map(0.0, 2.0, 0.0, 3.0, 34, 21, 17, 7)
    got, stats = N.warp_planes(src, m, N.AVERAGE, 1.0, out64=True)
    want = src.astype(np.float64).reshape(7, 3, 17, 2).mean(axis=(1, 3))
    err = np.abs(got[0] - want).max()
    print(f"block mean: max error {err:.3e}")
    assert err <= 1e-12 and stats == [7 * 17, 0, 0]
    lo, _ = N.warp_planes(src, m, N.MIN, 1.0)
    hi, _ = N.warp_planes(src, m, N.MAX, 1.0)
    assert np.array_equal(lo[0], src.reshape(7, 3, 17, 2).min(axis=(1, 3))) and np.array_equal(hi[0], src.reshape(7, 3, 17, 2).max(axis=(1, 3)))


@pytest.mark.parametrize("dst_w,dst_h", [(13, 5), (77, 50)], ids=["down", "up"])
def test_the_average_conserves_the_sum(dst_w, dst_h):
    """the destination extent equal to the source extent, no holes: sum(dst) step_x step_y == sum(src) to 1e-12 relative (measured
    1.3e-16 both ways: the weights of a source cell add up to its area)"""
    src = N.float_raster(21, 34, "none", seed=4)[0] + np.float32(150.0)
    m = N.Map(0.0, 34 / dst_w, 0.0, 21 / dst_h, 34, 21, dst_w, dst_h)
    got, stats = N.warp_planes(src, m, N.AVERAGE, 1.0, out64=True)
    total, want = got.sum() * m.step_x * m.step_y, src.astype(np.float64).sum()
    print(f"{dst_w} x {dst_h}: relative difference {abs(total - want) / want:.3e}")
    assert abs(total - want) <= 1e-12 * want and stats[1] == 0


def _plane(m):
    jj, ii = np.mgrid[0:m.src_h, 0:m.src_w]
    return (3.0 + 0.25 * (ii + 0.5) - 1.5 * (jj + 0.5)).astype(np.float32)          # multiples of 1 / 8: exact in float32


def _centres(m):
    cx = m.off_x + (np.arange(m.dst_w) + 0.5) * m.step_x
    cy = m.off_y + (np.arange(m.dst_h) + 0.5) * m.step_y
    return cx, cy


def test_bilinear_reproduces_a_plane():
    """3 + 0.25 x - 1.5 y at the destination's centres, to 1e-12 (measured 7.1e-15), wherever all four taps lie inside the source"""
    m = N.Map(1.2, 0.37, 0.9, 0.61, 34, 21, 77, 28)
    got, stats = N.warp_planes(_plane(m), m, N.BILINEAR, 1.0, out64=True)
    cx, cy = _centres(m)
    want = 3.0 + 0.25 * cx[None, :] - 1.5 * cy[:, None]
    err = np.abs(got[0] - want).max()
    print(f"plane: max error {err:.3e}")
    assert stats == [77 * 28, 0, 0] and err <= 1e-12


def test_bilinear_is_scipys_map_coordinates():
    """order 1, mode="constant", cval=nan at the same centres (scipy's pixel k has its centre at k, ours at k + 0.5): agreement to
    1e-9 where both are finite (measured 1.4e-14; a wrong tap or weight is O(1e-2)), and scipy is finite nowhere we are not"""
    ndimage = pytest.importorskip("scipy.ndimage")
    m = N.Map(-2.3, 0.37, -1.1, 1.7, 34, 21, 110, 15)
    src = N.float_raster(21, 34, "none", seed=5)[0]
    got, _ = N.warp_planes(src, m, N.BILINEAR, 1.0, out64=True)
    cx, cy = _centres(m)
    yy, xx = np.meshgrid(cy - 0.5, cx - 0.5, indexing="ij")
    want = ndimage.map_coordinates(src.astype(np.float64), [yy, xx], order=1, mode="constant", cval=np.nan)
    both = np.isfinite(got[0]) & np.isfinite(want)
    err = np.abs(got[0] - want)[both].max()
    print(f"scipy: max error {err:.3e} over {both.sum()} cells")
    assert both.sum() > 300 and err <= 1e-9
    assert not (np.isfinite(want) & ~np.isfinite(got[0])).any()


def test_mode_is_the_brute_force_count():
    """members = the source cells whose centre lies in the destination cell; the most votes, the lowest class on a tie, 255 without a vote"""
    lab = N.label_raster(21, 34, seed=6)
    lab[0:3, 0:4] = 255                                     # an all-255 cell
    lab[3:6, 0:4] = np.array([[5, 5, 2, 2], [2, 5, 5, 2], [1, 1, 1, 255]], np.uint8)      # 5 and 2 tie with four votes each
    m = N.Map(0.0, 4.0, 0.0, 3.0, 34, 21, 9, 7)
    got, stats = N.warp_labels(lab, m, N.MODE)
    assert got[0, 0] == 255 and got[1, 0] == 2
    ties = 0
    for j in range(7):
        for i in range(9):
            block = lab[3 * j:3 * j + 3, 4 * i:min(4 * i + 4, 34)].reshape(-1)
            counts = np.bincount(block[block != 255], minlength=256)
            ties += int((counts == counts.max()).sum() > 1 and counts.max() > 0)
            assert got[j, i] == (255 if counts.max() == 0 else int(np.flatnonzero(counts == counts.max())[0])), (j, i)
    assert ties >= 1 and stats[2] == 7            # the last column's cells reach beyond the 34 source columns
    # centres, not overlap: a destination cell [0.6, 1.4) holds no centre of its own and takes floor(c)
    fine, _ = N.warp_labels(np.array([[7, 8, 9]], np.uint8), N.Map(0.6, 0.8, 0.0, 1.0, 3, 1, 3, 1), N.MODE)
    assert fine.tolist() == [[8, 8, 9]]           # [0.6, 1.4): floor(1.0) = 1;  [1.4, 2.2): the centre 1.5;  [2.2, 3.0): the centre 2.5


def test_min_valid_on_a_hand_made_case():
    """four bilinear taps of weight 1/4, one NaN: den = 0.75 of tot = 1 -- finite at min_valid 0.75, a hole at 0.76"""
    src = np.array([[1.0, 2.0], [np.nan, 4.0]], np.float32)
    m = N.Map(0.5, 1.0, 0.5, 1.0, 2, 2, 1, 1)
    for restate in (N.warp_planes, N.planes_by_cells):
        got, stats = restate(src, m, N.BILINEAR, 0.75)
        assert got.reshape(-1).tolist() == [np.float32((0.25 + 0.5 + 1.0) / 0.75)] and stats == [1, 0, 0]
        got, stats = restate(src, m, N.BILINEAR, 0.76)
        assert np.isnan(got).all() and stats == [0, 1, 0]
    lo, _ = N.warp_planes(src, N.Map(0.0, 2.0, 0.0, 2.0, 2, 2, 1, 1), N.MIN, 0.75)
    hi, _ = N.warp_planes(src, N.Map(0.0, 2.0, 0.0, 2.0, 2, 2, 1, 1), N.MAX, 0.76)
    assert lo.item() == 1.0 and np.isnan(hi).all()


def test_an_infinity_is_a_hole():
    src = np.array([[1.0, np.inf], [-np.inf, 4.0]], np.float32)
    whole = N.Map(0.0, 2.0, 0.0, 2.0, 2, 2, 1, 1)
    assert N.warp_planes(src, whole, N.AVERAGE, 0.5)[0].item() == 2.5
    assert N.warp_planes(src, whole, N.MIN, 0.5)[0].item() == 1.0 and N.warp_planes(src, whole, N.MAX, 0.5)[0].item() == 4.0
    assert np.isnan(N.warp_planes(src, whole, N.AVERAGE, 0.51)[0]).all()
    same = N.Map(0.0, 1.0, 0.0, 1.0, 2, 2, 2, 2)
    for method in N.FLOAT_METHODS:
        got, stats = N.warp_planes(src, same, method, 0.5)
        assert np.array_equal(bits(got[0]), bits(np.array([[1.0, N.NAN32], [N.NAN32, 4.0]], np.float32))) and stats == [2, 2, 0]


# ---- the host layer -------------------------------------------------------------------------------------------------------------------------
def test_lattices_and_snapping():
    grid = D.DsmGrid(1000.0, 2000.0, 0.5, 40, 30)
    lat = W.lattice_of(grid)
    assert lat == W.Lattice(1000.0, 2000.0, 0.5, 0.5, 40, 30) and W.lattice_of(lat) is lat
    assert W.lattice_of((1000.0, 2000.0, 0.5, 0.5), (30, 40)) == lat and W.lattice_of((1000.0, 2000.0, 0.5, 0.5), (3, 30, 40)) == lat
    window = D.grid_struct(grid, (4, 6, 10, 8))
    assert W.lattice_of(window) == W.Lattice(1002.0, 1997.0, 0.5, 0.5, 10, 8)
    with pytest.raises(ValueError, match="needs the raster's shape"):
        W.lattice_of((1000.0, 2000.0, 0.5, 0.5))
    with pytest.raises(ValueError, match="30 x 40 cells, the raster 30 x 41"):
        W.lattice_of(grid, (30, 41))
    with pytest.raises(ValueError, match="positive cell sizes"):
        W.lattice_of((0.0, 0.0, 0.5, -0.5), (3, 4))
    # a 1 m raster whose corner is 0.25 m off, onto the 0.5 m grid: half-cell steps, the offsets in source cells, rows growing south
    src = W.Lattice(999.75, 2000.25, 1.0, 1.0, 25, 20)
    m = W.warp_map(src, grid)
    assert (m.off_x, m.step_x, m.off_y, m.step_y) == (0.25, 0.5, 0.25, 0.5) and (m.src_w, m.src_h, m.dst_w, m.dst_h) == (25, 20, 40, 30)
    back = W.warp_map(grid, src)
    assert (back.off_x, back.step_x, back.off_y, back.step_y) == (-0.5, 2.0, -0.5, 2.0)
    # snapping: a step within 1e-9 (relative) of 1 is 1; at step 1 an offset within 1e-6 of an integer is that integer
    near = W.Lattice(1000.0 + 3 * 0.5 + 2e-7, 2000.0 - 2 * 0.5 - 3e-7, 0.5 * (1 + 5e-10), 0.5 * (1 - 5e-10), 8, 9)
    m = W.warp_map(grid, near)
    assert (m.off_x, m.step_x, m.off_y, m.step_y) == (3.0, 1.0, 2.0, 1.0)
    off = W.warp_map(grid, W.Lattice(1000.0 + 3 * 0.5 + 2e-6, 2000.0, 0.5, 0.5, 8, 9))
    assert off.step_x == 1.0 and off.off_x != 3.0 and abs(off.off_x - 3.0) < 1e-5 and off.off_y == 0.0
    loose = W.warp_map(grid, W.Lattice(1000.0 + 1e-7, 2000.0, 0.5 * (1 + 1e-8), 0.5, 8, 9))
    assert loose.step_x != 1.0 and loose.off_x != 0.0                                  # no snapping of the offset off step 1
    assert W.same_lattice(grid, lat) and W.same_lattice(lat, grid)
    assert W.same_lattice(grid, W.Lattice(1000.0 + 1e-7, 2000.0, 0.5, 0.5 * (1 + 1e-10), 40, 30))
    assert not W.same_lattice(grid, W.Lattice(1000.5, 2000.0, 0.5, 0.5, 40, 30))      # a whole cell off: a shift, not the same
    assert not W.same_lattice(grid, W.Lattice(1000.0, 2000.0, 0.5, 0.5, 40, 29)) and not W.same_lattice(grid, src)
    assert [W.default_method(W.warp_map(src, grid), lab) for lab in (False, True)] == ["bilinear", "nearest"]
    assert [W.default_method(W.warp_map(grid, src), lab) for lab in (False, True)] == ["average", "mode"]
    mixed = W.warp_map(grid, W.Lattice(1000.0, 2000.0, 0.25, 1.0, 8, 9))
    assert [W.default_method(mixed, lab) for lab in (False, True)] == ["average", "mode"]


def test_an_integer_shift_is_a_slice_without_a_launch():
    """host tensors pass: nothing is launched; the result is the restatement's, the stats included"""
    grid = D.DsmGrid(1000.0, 2000.0, 0.5, 9, 7)
    dst = D.DsmGrid(1001.5, 2001.0, 0.5, 8, 9)
    src = N.float_raster(7, 9, "random", planes=3, seed=7)
    lab = N.label_raster(7, 9, seed=7)
    m = N.Map(3.0, 1.0, -2.0, 1.0, 9, 7, 8, 9)
    for x in (src, src[0]):
        got, stats = W.warp(torch.from_numpy(x), grid, dst, return_stats=True)
        want, want_stats = N.warp_planes(x, m, N.BILINEAR)
        assert tuple(got.shape) == x.shape[:-2] + (9, 8) and np.array_equal(bits(got.numpy()), bits(want).reshape(got.shape)) and stats == want_stats
    for method in W.FLOAT_METHODS:
        assert np.array_equal(bits(W.warp(torch.from_numpy(src), grid, dst, method).numpy()), bits(N.warp_planes(src, m, W.METHODS[method])[0]))
    got, stats = W.warp(torch.from_numpy(lab), grid, dst, "mode", return_stats=True)
    want, want_stats = N.warp_labels(lab, m, N.MODE)
    assert np.array_equal(got.numpy(), want) and stats == want_stats
    assert W.warp(torch.from_numpy(src).double(), grid, dst).dtype == torch.float32
    away = W.warp(torch.from_numpy(src[0]), grid, D.DsmGrid(2000.0, 2000.0, 0.5, 4, 3))
    assert tuple(away.shape) == (3, 4) and torch.isnan(away).all()
    same = W.warp(torch.from_numpy(src), grid, grid)
    assert np.array_equal(bits(same.numpy()), bits(src))


def test_warp_products_moves_every_plane():
    """a whole-cell shift, so nothing is launched: float planes, the label plane and the uint8 colour plane move, "grid" becomes the
    new lattice, everything else is passed on"""
    grid, dst = D.DsmGrid(1000.0, 2000.0, 0.5, 9, 7), D.DsmGrid(1001.5, 2001.0, 0.5, 8, 9)
    m = N.Map(3.0, 1.0, -2.0, 1.0, 9, 7, 8, 9)
    alt, lab = N.float_raster(7, 9, "random", seed=8)[0], N.label_raster(7, 9, seed=8)
    rgb = np.random.default_rng(8).integers(0, 256, (3, 7, 9)).astype(np.uint8)
    products = {"grid": grid, "dsm": torch.from_numpy(alt), "label": torch.from_numpy(lab), "rgb_u8": torch.from_numpy(rgb),
                "rgb": torch.from_numpy(rgb.astype(np.float32) / 255.0), "count": torch.zeros((7, 9), dtype=torch.int32), "name": "x"}
    out = W.warp_products(products, dst)
    assert list(out) == list(products) and out["grid"] is dst and out["name"] == "x" and out["count"] is products["count"]
    assert np.array_equal(bits(out["dsm"].numpy()), bits(N.warp_planes(alt, m, N.BILINEAR)[0][0]))
    assert np.array_equal(out["label"].numpy(), N.warp_labels(lab, m, N.NEAREST)[0])
    want = np.zeros((3, 9, 8), np.uint8)
    want[:, 2:9, 0:6] = rgb[:, 0:7, 3:9]
    assert out["rgb_u8"].dtype == torch.uint8 and np.array_equal(out["rgb_u8"].numpy(), want)                # holes -> 0
    assert np.array_equal(bits(out["rgb"].numpy()), bits(N.warp_planes(rgb.astype(np.float32) / 255.0, m, N.BILINEAR)[0]))


def test_warp_refuses_by_name_what_it_does_not_take():
    grid, coarse = D.DsmGrid(1000.0, 2000.0, 0.5, 9, 7), D.DsmGrid(1000.0, 2000.0, 1.0, 4, 3)
    x = torch.zeros((7, 9))
    with pytest.raises(ValueError, match="must be a GPU tensor"):
        W.warp(x, grid, coarse)
    with pytest.raises(ValueError, match="'mode' is none of"):
        W.warp(x, grid, coarse, "mode")
    with pytest.raises(ValueError, match="'bilinear' is none of"):
        W.warp(x.to(torch.uint8), grid, coarse, "bilinear")
    with pytest.raises(ValueError, match="min_valid"):
        W.warp(x, grid, coarse, min_valid=0.0)
    with pytest.raises(ValueError, match="a float or uint8 raster"):
        W.warp(x.to(torch.int32), grid, coarse)
    with pytest.raises(ValueError, match=r"a label raster is \(h, w\)"):
        W.warp(torch.zeros((3, 7, 9), dtype=torch.uint8), grid, coarse)
    with pytest.raises(ValueError, match="7 x 9 cells, the raster 7 x 8"):
        W.warp(torch.zeros((7, 8)), grid, coarse)


def test_the_defaults_keep_what_was(tmp_path):
    """every new argument defaults to None: an off-lattice ground truth still raises, the exports' signatures only grew at the end"""
    from snerf_amd.eval import ortho as EO
    from snerf_amd.framework.util import img_utils as IU
    for fn, names in ((IU.crop_to_roi, ("resample", "device")), (IU.load_dsm_ground_truth, ("resample", "device")),
                      (EO.export_terrain, ("reference_grid", "reference_resample")), (EO.export_objects, ("reference_grid", "reference_resample"))):
        p = inspect.signature(fn).parameters
        assert all(p[n].default is None for n in names), fn.__name__
    assert list(inspect.signature(IU.crop_to_roi).parameters)[:4] == ["raster", "geotransform", "roi_meta", "what"]
    assert list(inspect.signature(EO.export_terrain).parameters)[:7] == ["products", "output_dp", "alt_key", "label_key", "blocked", "reference",
                                                                         "zone_string"]
    for name in ("export_roofs", "export_solar", "export_rectified"):
        assert "reference_grid" not in inspect.signature(getattr(EO, name)).parameters
    roi = np.array([1000.0, 2000.0, 8, 0.5])
    raster = np.arange(400, dtype=np.float32).reshape(20, 20)
    with pytest.raises(ValueError, match="resampling is not supported"):
        IU.crop_to_roi(raster, (999.75, 2006.25, 1.0, 1.0), roi)
    with pytest.raises(ValueError, match="off the ROI lattice"):
        IU.crop_to_roi(raster, (999.75, 2006.0, 0.5, 0.5), roi)
    with pytest.raises(ValueError, match="reaches beyond"):
        IU.crop_to_roi(raster, (1003.0, 2006.0, 0.5, 0.5), roi)
    # on the lattice and containing the ROI: the crop of before, with or without `resample` (no device is touched)
    on = IU.crop_to_roi(raster, (999.0, 2006.0, 0.5, 0.5), roi)
    assert np.array_equal(on, raster[4:12, 2:10]) and np.array_equal(IU.crop_to_roi(raster, (999.0, 2006.0, 0.5, 0.5), roi, resample=True), on)
    with pytest.raises(ValueError, match=r"\(3, 4\) cells, the reference on \(2, 2\)"):
        EO.export_terrain({"grid": D.DsmGrid(0.0, 0.0, 0.5, 4, 3), "dsm": torch.zeros((3, 4))}, str(tmp_path), reference={"alt": torch.zeros((2, 2))})


# ---- refusals of the entries ----------------------------------------------------------------------------------------------------------
def _call(symbol, map_kw=None, **kw):
    """an entry through the binding with dummy addresses: (rc, message); every refusal returns before a launch"""
    L = _lib.lib()
    fields = dict(off_x=0.25, step_x=2.0, off_y=-1.5, step_y=2.0, src_w=8, src_h=6, dst_w=4, dst_h=3)
    fields.update(map_kw or {})
    a = dict(src=DUMMY, planes=1, map=C.byref(_lib.SnerfWarpMap(**fields)), method=_lib.WARP_AVERAGE if symbol.endswith("planes") else _lib.WARP_MODE,
             min_valid=0.5, dst=2 * DUMMY, stats=3 * DUMMY)
    a.update(kw)
    rc = getattr(L, symbol)(*[a[name] for name in NAMES[symbol][:-1]], None)
    return rc, L.snerf_last_error().decode()


BOTH = [
    ({}, {"src": None}, 3, "null"), ({}, {"map": None}, 3, "null"), ({}, {"dst": None}, 3, "null"), ({}, {"stats": None}, 3, "null"),
    ({}, {"dst": DUMMY}, 1, "must not alias"),
    ({"src_w": 0}, {}, 1, ">= 1"), ({"src_h": -1}, {}, 1, ">= 1"), ({"dst_w": 0}, {}, 1, ">= 1"), ({"dst_h": 0}, {}, 1, ">= 1"),
    ({"src_w": 65536, "src_h": 32768}, {}, 1, "below 2^31"), ({"dst_w": 2 ** 31 - 1, "dst_h": 2 ** 31 - 1}, {}, 1, "below 2^31"),
    ({"step_x": 0.0}, {}, 1, "step_x"), ({"step_y": -1.0}, {}, 1, "step_y"), ({"step_x": math.nan}, {}, 1, "step_x"),
    ({"step_y": math.inf}, {}, 1, "step_y"),
    ({"off_x": 2.0 ** 31}, {}, 1, "below 2^31"), ({"off_y": -2.0 ** 31 + 4}, {}, 1, "below 2^31"), ({"off_x": math.nan}, {}, 1, "below 2^31"),
    ({"off_y": -math.inf}, {}, 1, "below 2^31"), ({"step_x": 1e9}, {}, 1, "below 2^31"),
    ({"step_x": 64.5}, {}, 1, "SNERF_WARP_MAX_STEP"), ({"step_y": 65.0}, {}, 1, "SNERF_WARP_MAX_STEP"),
]
PLANES = [
    ({}, {"method": -1}, 1, "method = -1"), ({}, {"method": _lib.WARP_MODE}, 1, "method = 5"),
    ({}, {"planes": 0}, 1, "planes = 0"), ({}, {"planes": 17}, 1, "planes = 17"),
    ({}, {"min_valid": 0.0}, 1, "min_valid"), ({}, {"min_valid": 1.0000001}, 1, "min_valid"), ({}, {"min_valid": math.nan}, 1, "min_valid"),
    ({}, {"min_valid": -0.5, "method": _lib.WARP_NEAREST}, 1, "min_valid"),
]
LABELS = [
    ({}, {"method": _lib.WARP_BILINEAR}, 1, "method = 1"), ({}, {"method": _lib.WARP_MAX}, 1, "method = 4"), ({}, {"method": 6}, 1, "method = 6"),
]
CASES = ([("snerf_warp_planes",) + c for c in BOTH + PLANES] + [("snerf_warp_labels",) + c for c in BOTH + LABELS])


@pytest.mark.parametrize("symbol,map_kw,kw,code,needle", CASES, ids=[f"{c[0][11:]}-{n}" for n, c in enumerate(CASES)])
def test_the_entries_refuse_bad_arguments_before_any_launch(symbol, map_kw, kw, code, needle):
    rc, msg = _call(symbol, map_kw, **kw)
    assert rc == code and msg.startswith(symbol + ": ") and needle in msg, (rc, msg)

